"""The trunk's layer primitives (libairpose_grad.so: trunk_grad.hip) against torch CPU fp64 at the shapes where kernels go wrong:
every distinct conv geometry of the ResNet-50 trunk at its real spatial size with a multi-chunk, ragged split-K weight gradient;
shapes the API accepts but the trunk does not use (H != W, R != S, stride 3, channel counts that select each loader, partial
tiles, 1 x 1 maps, a misaligned input); BatchNorm from 1 to 401 408 rows (the capped-tile regime above 65 536 rows), a
cancellation-prone batch, in-place calls; the pools at the trunk's size and at H = 1, 2, 3.

Each check runs the kernel on fp32 inputs and the same operation in fp64 on the same fp32 values, and asserts two bars per tensor:
  - rel_err <= 1e-5 (max |got - ref| / max |ref|, as in tests/test_trunk_grad.py);
  - element-wise |got - ref| <= TAU * A, where A is the same expression in fp64 with every operand replaced by its absolute value
    and every subtraction turned into an addition (conv of |x| and |w|, dgrad of |gy| and |w|, wgrad of |x| and |gy|, likewise for
    BatchNorm).  A bounds the magnitude of every term that enters an element, so a missing, doubled or misplaced term fails at any
    element, not only near the tensor's maximum; where A == 0 the kernel must give exactly 0.
TAU = 1e-5 is an empirical bar, not a derived one.  The rigorous bound for a k-term fp32 sum is about k u A (u = 6e-8), which passes
1e-5 A once k exceeds ~170, and the trunk's sums are longer (C R S up to 4608, split-K chunks of hundreds of pixels).  For these
signed random operands the partial sums grow like sqrt(k) and the rounding errors do not line up, so the measured error stays near
u A: the worst err / (TAU A) over every case here is about 0.05 with the fixed seeds (each case prints its own).  A rewrite that
changes the summation order should re-measure that margin rather than assume it."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, rel_err

pytestmark = pytest.mark.gpu
TAU = 1e-5
MOM, EPS = 0.1, 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _check(what, name, got, ref, A, out, rel_bar=1e-5):
    """rel_err(got, ref) <= rel_bar (None: not asserted, see the caller) and |got - ref| <= TAU A element-wise; records the worst
    err / (TAU A) in out[name]"""
    got = got.detach().cpu().double()
    ref, A = ref.detach().cpu().double(), A.detach().cpu().double()
    assert got.shape == ref.shape == A.shape, (what, name, got.shape, ref.shape, A.shape)
    assert torch.isfinite(got).all(), (what, name, "non-finite output (an element never written?)")
    e = rel_err(got.numpy(), ref.numpy())
    err, lim = (got - ref).abs(), TAU * A
    zero = lim == 0
    assert not (err[zero] > 0).any(), (what, name, "%d elements nonzero where every term is 0" % int((err[zero] > 0).sum()))
    ratio = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    out[name] = ratio
    assert rel_bar is None or e <= rel_bar, (what, name, "rel_err %.3e" % e)
    assert ratio <= 1.0, (what, name, "worst |err| / (tau A) %.3f at tau %.0e" % (ratio, TAU))


def _report(what, ratios, extra=""):
    print("%-40s %s  worst err/(tau A): %s" % (what, extra, "  ".join("%s %.4f" % kv for kv in ratios.items())))


# ------------------------------------------------------------------------------------------------ convolution
def _conv64(x, w, gy, st, pad):
    """fp64 y, gx, gw of conv2d(x, w) with output gradient gy (NCHW / OIHW)"""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    y = F.conv2d(x, w, stride=st, padding=pad)
    y.backward(gy.double())
    return y.detach(), x.grad, w.grad


def _run_conv(dev, geom, seed, offset=0):
    """geom = (n, H, W, C, K, R, S, stride, pad); offset: x starts that many floats into its buffer (offset 1: the per-element
    loaders).  Returns the worst err / (tau A) per tensor and the weight gradient's split-K chunk count."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, H, W, C, K, R, S, st, pad = geom
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, H, W, generator=g)                          # fp32: the values both sides see
    w = torch.randn(K, C, R, S, generator=g) * (2.0 / (C * R * S)) ** 0.5
    gy = torch.randn(n, K, Ho, Wo, generator=g)
    y64, gx64, gw64 = _conv64(x, w, gy, st, pad)
    Ay, Agx, Agw = _conv64(x.abs(), w.abs(), gy.abs(), st, pad)
    L = G.lib()
    s = N.stream_ptr(dev)
    xbuf = torch.empty(x.numel() + 4, device=dev)
    xd = xbuf[offset:offset + x.numel()].view(n, H, W, C)
    xd.copy_(_nhwc(x))
    assert (xd.data_ptr() % 16 == 0) == (offset % 4 == 0)
    wd, gyd = w.to(dev), _nhwc(gy).to(dev)
    nb = L.apg_conv_bwd_workspace_bytes(n, H, W, C, K, R, S, st, pad)
    per = 4 * K * C * R * S
    assert nb > 0 and nb % per == 0, (geom, nb)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # an element the kernel never writes stays NaN
    yd, gxd, gwd = nan(n, Ho, Wo, K), nan(n, H, W, C), nan(K, C, R, S)
    gxd2, gwd2 = nan(n, H, W, C), nan(K, C, R, S)
    G.check(L.apg_conv_fwd(N.dptr(xd), n, H, W, C, N.dptr(wd), K, R, S, st, pad, N.dptr(yd), s), "apg_conv_fwd")
    for gx_, gw_ in ((gxd, gwd), (gxd2, gwd2)):
        G.check(L.apg_conv_bwd(N.dptr(xd), n, H, W, C, N.dptr(wd), K, R, S, st, pad, N.dptr(gyd), N.dptr(gx_), N.dptr(gw_),
                               ws.data_ptr(), nb, s), "apg_conv_bwd")
    torch.cuda.synchronize()
    ratios = {}
    _check(geom, "y", yd, _nhwc(y64), _nhwc(Ay), ratios)
    _check(geom, "gx", gxd, _nhwc(gx64), _nhwc(Agx), ratios)
    _check(geom, "gw", gwd, gw64, Agw, ratios)
    assert torch.equal(gwd, gwd2) and torch.equal(gxd, gxd2), (geom, "two identical calls differ")
    return ratios, nb // per


@functools.lru_cache(maxsize=None)
def _trunk_geoms():
    """Every distinct (H, C, K, R, stride, pad) of the trunk's 53 convolutions, H = the conv's input size, walking the [3, 4, 6, 3]
    plan over trunk_grad.conv_bn_pairs' modules (224 -> stem -> 112 -> max-pool -> 56 -> ... -> 7)."""
    from airpose_amd import copenet_model, trunk_grad
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32")
    size = {}
    H = 56
    size[net.conv1] = 224
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            st = blk.conv2.stride[0]
            Ho = (H + 2 * blk.conv2.padding[0] - blk.conv2.kernel_size[0]) // st + 1
            size[blk.conv1], size[blk.conv2], size[blk.conv3] = H, H, Ho
            if blk.downsample is not None:
                size[blk.downsample[0]] = H
            H = Ho
    convs = [c for c, _ in trunk_grad.conv_bn_pairs(net)]
    assert len(convs) == 53 and set(map(id, convs)) == set(map(id, size)) and H == 7
    out = []
    for c in convs:
        assert c.kernel_size[0] == c.kernel_size[1] and c.stride[0] == c.stride[1] and c.padding[0] == c.padding[1]
        geo = (size[c], c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0])
        if geo not in out:
            out.append(geo)
    return out


TRUNK_GEOMS = _trunk_geoms()


def _gid(geo):
    H, C, K, R, st, pad = geo
    return "H%d-%dto%d-%dx%ds%dp%d" % (H, C, K, R, R, st, pad)


def test_the_trunk_has_23_distinct_conv_geometries():
    assert len(TRUNK_GEOMS) == 23, TRUNK_GEOMS
    assert TRUNK_GEOMS[0] == (224, 3, 64, 7, 2, 3)


@pytest.mark.parametrize("geo", TRUNK_GEOMS, ids=[_gid(g) for g in TRUNK_GEOMS])
def test_trunk_conv_geometry_matches_fp64(dev, geo):
    """The geometry at its real size, with the smallest n <= 16 whose weight gradient runs in >= 2 split-K chunks of which the
    last is ragged: n Ho Wo not divisible by the chunk count, so no equal split exists."""
    from airpose_amd import _native_grad as G
    H, C, K, R, st, pad = geo
    Ho = (H + 2 * pad - R) // st + 1
    L = G.lib()
    per = 4 * K * C * R * R
    for n in range(1, 17):
        nch = L.apg_conv_bwd_workspace_bytes(n, H, H, C, K, R, R, st, pad) // per
        if nch >= 2 and (n * Ho * Ho) % nch != 0:
            break
    else:
        pytest.fail("no n <= 16 gives a multi-chunk, ragged weight gradient for %s" % (geo,))
    ratios, nch = _run_conv(dev, (n, H, H, C, K, R, R, st, pad), seed=sum(geo) + n)
    _report(_gid(geo), ratios, "n %2d, %2d wgrad chunks over %6d pixels" % (n, nch, n * Ho * Ho))


GEOMS_OUT7 = [g for g in TRUNK_GEOMS if (g[0] + 2 * g[5] - g[3]) // g[4] + 1 == 7]      # layer4, all but its first 1 x 1


def test_the_trunk_has_5_geometries_with_a_7x7_output():
    assert len(GEOMS_OUT7) == 5, GEOMS_OUT7


@pytest.mark.parametrize("geo", GEOMS_OUT7, ids=[_gid(g) for g in GEOMS_OUT7])
def test_layer4_geometry_at_one_image_matches_fp64(dev, geo):
    """layer4 as the walker runs it at n = 1: M = 49 output rows, below one 64-row tile"""
    H, C, K, R, st, pad = geo
    ratios, nch = _run_conv(dev, (1, H, H, C, K, R, R, st, pad), seed=3 * sum(geo))
    _report(_gid(geo) + " n 1", ratios, "%d wgrad chunks over 49 pixels" % nch)


API_GEOMS = [  # (n, H, W, C, K, R, S, stride, pad), x offset in floats
    ((2, 13, 21, 64, 64, 3, 3, 2, 1), 0),        # H != W
    ((2, 12, 12, 32, 32, 1, 5, 1, 2), 0),        # R != S (Ho = 16, Wo = 12)
    ((2, 17, 17, 16, 32, 5, 5, 3, 2), 0),        # 5 x 5, stride 3
    ((2, 10, 10, 8, 32, 3, 3, 1, 1), 0),         # C = 8: per-element forward and weight-gradient loaders
    ((2, 9, 9, 48, 64, 3, 3, 2, 1), 0),          # C = 48: float4 forward, per-element weight gradient
    ((2, 11, 11, 96, 48, 3, 3, 1, 1), 0),        # C = 96: the same, a 64-column tile across two taps
    ((2, 12, 12, 64, 16, 3, 3, 1, 1), 0),        # K = 16: one partial N tile (forward), partial M tile (weight gradient)
    ((2, 10, 10, 32, 80, 1, 1, 1, 0), 0),        # K = 80: a full and a partial tile
    ((1, 1, 1, 64, 64, 1, 1, 1, 0), 0),          # n = 1, a 1 x 1 map
    ((1, 1, 1, 64, 64, 3, 3, 1, 1), 0),          # n = 1, 1 x 1 map, 3 x 3 / p1: eight of nine taps in the padding
    ((2, 16, 16, 32, 32, 3, 3, 2, 0), 0),        # 3 x 3 / s2 / p0 on an even H: the last row / column is read by no window
    ((2, 7, 7, 2048, 16, 1, 1, 1, 0), 0),        # C = 2048 -> K = 16 at 7 x 7
    ((2, 14, 14, 64, 64, 3, 3, 1, 1), 1),        # float4 geometry, x one float off alignment: the per-element loaders
    ((3, 15, 15, 128, 64, 3, 3, 2, 1), 1),       # the same for a strided 3 x 3
]
API_IDS = ["HneW", "RneS", "5x5s3", "C8", "C48", "C96", "K16", "K80", "1x1map-1x1", "1x1map-3x3p1", "3x3s2p0-evenH", "C2048-K16",
           "misaligned-x", "misaligned-x-s2"]


@pytest.mark.parametrize("geom,offset", API_GEOMS, ids=API_IDS)
def test_conv_api_shapes_match_fp64(dev, geom, offset):
    ratios, nch = _run_conv(dev, geom, seed=7 + sum(geom), offset=offset)
    _report("%s offset %d" % (geom, offset), ratios, "%d wgrad chunks" % nch)


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_inputs(M, C, seed, ratio=None, spread=1.0):
    """fp32 x (M, C) with per-channel shift and scale (ratio: |shift| / scale of every channel, sign alternating; spread != 1
    multiplies the scale and zeroes the shift), gamma of both signs, beta, a residual, running statistics, an output gradient"""
    g = torch.Generator().manual_seed(seed)
    scale = (torch.rand(C, generator=g) + 0.5) * spread
    if spread != 1.0:
        shift = torch.zeros(C)
    elif ratio is None:
        shift = torch.randn(C, generator=g) * 2
    else:
        shift = ratio * scale * torch.tensor([(-1.0) ** c for c in range(C)])
    x = torch.randn(M, C, generator=g) * scale + shift
    gam = torch.randn(C, generator=g)
    bet = torch.randn(C, generator=g)
    res = torch.randn(M, C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    gy = torch.randn(M, C, generator=g)
    return x, gam, bet, res, rm, rv, gy


def _run_bn(dev, M, C, train, res, relu, seed, ratio=None, spread=1.0):
    """apg_bn_fwd / apg_bn_bwd on (M, C) rows against F.batch_norm + autograd in fp64; then the same calls in place (y over x,
    gx over gy) must give the same bits.  The backward's ReLU mask is the kernel's own y > 0 (the documented contract); where it
    differs from fp64's, fp64's pre-ReLU value must lie within TAU A of zero."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    x, gam, bet, r, rm, rv, gy = _bn_inputs(M, C, seed, ratio, spread)
    L = G.lib()
    s = N.stream_ptr(dev)
    nb = L.apg_bn_workspace_bytes(M, C)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    xd, gd, bd, rd, gyd = (t.to(dev) for t in (x, gam, bet, r, gy))
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)

    def fwd(x_in, y_out):
        rmd, rvd, mean, invstd = rm.to(dev), rv.to(dev), nan(C), nan(C)
        G.check(L.apg_bn_fwd(N.dptr(x_in), M, C, N.dptr(gd), N.dptr(bd), N.dptr(rmd), N.dptr(rvd), train, MOM, EPS,
                             N.dptr(rd) if res else None, int(relu), N.dptr(y_out), N.dptr(mean), N.dptr(invstd), ws.data_ptr(), nb,
                             s), "apg_bn_fwd")
        return rmd, rvd, mean, invstd

    def bwd(gy_in, gx_out, yd):
        gres, gg, gb = nan(M, C), nan(C), nan(C)
        G.check(L.apg_bn_bwd(N.dptr(gy_in), N.dptr(yd) if relu else None, N.dptr(xd), M, C, N.dptr(gd), N.dptr(mean), N.dptr(invstd),
                             train, N.dptr(gx_out), N.dptr(gres), N.dptr(gg), N.dptr(gb), ws.data_ptr(), nb, s), "apg_bn_bwd")
        return gres, gg, gb

    yd = nan(M, C)
    rmd, rvd, mean, invstd = fwd(xd, yd)
    gxd = nan(M, C)
    gres, gg, gb = bwd(gyd, gxd, yd)
    # in place
    yi = xd.clone()
    inplace_f = fwd(yi, yi)
    gxi = gyd.clone()
    inplace_b = bwd(gxi, gxi, yd)
    torch.cuda.synchronize()
    assert torch.equal(yi, yd) and all(torch.equal(a, b) for a, b in zip(inplace_f, (rmd, rvd, mean, invstd))), "apg_bn_fwd in place"
    assert torch.equal(gxi, gxd) and all(torch.equal(a, b) for a, b in zip(inplace_b, (gres, gg, gb))), "apg_bn_bwd in place"

    # fp64
    x64, r64 = x.double().requires_grad_(True), r.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    rm64, rv64 = rm.double(), rv.double()
    pre = F.batch_norm(x64, rm64, rv64, g64, b64, bool(train), MOM, EPS)
    if res:
        pre = pre + r64
    mask = (yd.cpu() > 0).double() if relu else torch.ones(M, C, dtype=torch.float64)
    (pre * mask * gy.double()).sum().backward()
    if train:
        mu, var = x64.detach().mean(0), x64.detach().var(0, unbiased=False)
    else:
        mu, var = rm.double(), rv.double()
    istd = 1 / torch.sqrt(var + EPS)
    # magnitudes: |.| of every operand, subtractions as additions
    xa = (x.double().abs() + mu.abs()) * istd                          # |xhat|
    Ay = xa * gam.double().abs() + bet.double().abs() + (r.double().abs() if res else 0)
    ga = gy.double().abs() * mask
    if train:
        Agx = gam.double().abs() * istd * (ga + ga.mean(0) + xa * (ga * xa).mean(0))
    else:
        Agx = gam.double().abs() * istd * ga
    ratios = {}
    what = (M, C, train, res, relu)
    y64 = pre.detach().clamp_min(0) if relu else pre.detach()
    _check(what, "y", yd, y64, Ay, ratios)
    if relu:
        flip = (yd.cpu() > 0) != (pre.detach() > 0)
        assert (pre.detach()[flip].abs() <= TAU * Ay[flip]).all(), (what, "ReLU mask flips away from zero")
    # train mode at M = 2 with var >> eps: xhat = +-sqrt(var / (var + eps)), so gx = gamma invstd (g_1 - g_2) / 2 * eps / (var + eps)
    # per row is ~1e-5 of its own terms: fp32 rounding of the terms leaves ~1e-4 .. 1e-2 of gx (torch's own fp32 CPU batch_norm:
    # 3.2e-4 on this case), so rel_err measures fp32 there, not the kernel.  The element-wise bar left is about the terms' size,
    # above |gx| itself: that case checks only that gx has the right scale (a kernel returning 0 would pass it).  Two rows with
    # var ~ eps, where gx is of the order of its terms, get every bar in test_batchnorm_two_rows_at_eps_scale.
    _check(what, "gx", gxd, x64.grad, Agx, ratios, None if train and M == 2 and spread == 1.0 else 1e-5)
    _check(what, "ggamma", gg, g64.grad, (ga * xa).sum(0), ratios)
    _check(what, "gbeta", gb, b64.grad, ga.sum(0), ratios)
    assert torch.equal(gres.cpu(), gy * mask.float()), (what, "g_res is g = gy (y > 0)")
    e = {"mean": rel_err(mean.cpu().numpy(), mu.numpy()), "invstd": rel_err(invstd.cpu().numpy(), istd.numpy())}
    if train:
        e["running_mean"] = rel_err(rmd.cpu().numpy(), rm64.numpy())
        e["running_var"] = rel_err(rvd.cpu().numpy(), rv64.numpy())
    else:
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv), (what, "eval mode changed the running statistics")
    assert all(v <= 1e-5 for v in e.values()), (what, e)
    return ratios, e


def _bid(case):
    M, C, train, res, relu = case
    return "M%d-C%d-%s%s%s" % (M, C, "train" if train else "eval", "-res" if res else "", "-relu" if relu else "")


BN_CASES = [  # (M, C, train, res, relu); tiles: 256 rows up to M = 65 536, then ceil(M / 256) rounded up to 4 (at most 256 tiles)
    (2, 64, 1, 0, 0), (3, 64, 1, 0, 1), (49, 64, 1, 1, 1), (255, 64, 1, 0, 0), (257, 64, 1, 0, 1), (65536, 64, 1, 0, 0),
    (65537, 64, 1, 1, 1), (401408, 64, 1, 0, 0), (401408, 64, 1, 1, 1),
    (1, 64, 0, 0, 0), (2, 64, 0, 0, 1), (49, 64, 0, 1, 1), (65537, 64, 0, 0, 0), (401408, 64, 0, 1, 1),
    (49, 1, 1, 0, 0), (300, 3, 1, 0, 1), (300, 96, 1, 1, 1), (49, 2048, 1, 0, 0), (98, 2048, 1, 1, 1),
    (300, 3, 0, 0, 0), (98, 2048, 0, 0, 1),
]


@pytest.mark.parametrize("case", BN_CASES, ids=[_bid(c) for c in BN_CASES])
def test_batchnorm_sizes_match_fp64(dev, case):
    ratios, e = _run_bn(dev, *case, seed=sum(case))
    _report(_bid(case), ratios, " ".join("%s %.1e" % kv for kv in e.items()))


def test_batchnorm_two_rows_at_eps_scale(dev):
    """Two rows per channel with std ~ sqrt(eps): var ~ eps, so train-mode gx = gamma invstd (g_1 - g_2) / 2 * eps / (var + eps) is
    of the order of its terms and every bar applies, rel_err on gx included"""
    ratios, e = _run_bn(dev, 2, 64, 1, 0, 0, seed=23, spread=EPS ** 0.5)
    _report("M2 train, var ~ eps", ratios, " ".join("%s %.1e" % kv for kv in e.items()))


def test_batchnorm_cancellation_at_stem_size(dev):
    """|mean| / std = 100 in every channel over the stem's 401 408 rows (n = 32): the centred per-tile partials with Chan's
    combination hold 1e-5; a one-pass sum x, sum x^2 variance in fp32 loses ~1e-4 of the variance here (worse by ratio^2)."""
    ratios, e = _run_bn(dev, 401408, 64, 1, 0, 1, seed=99, ratio=100.0)
    _report("cancellation M401408 ratio 100", ratios, " ".join("%s %.1e" % kv for kv in e.items()))


# ------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("n,H,C", [(2, 112, 64), (2, 1, 64), (2, 2, 64), (2, 3, 64), (1, 3, 16)])
def test_maxpool_matches_torch_bitwise(dev, n, H, C):
    """Integer post-ReLU data: ~60 % zeros make all-tie windows, integer gradients sum exactly, so the result must be bitwise
    torch's (ties: the first maximum in row-major window order)."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    g = torch.Generator().manual_seed(5 + H)
    x = torch.relu(torch.randint(-2, 3, (n, C, H, H), generator=g).double()).requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    gy = torch.randint(-4, 5, y.shape, generator=g).double()
    (y * gy).sum().backward()
    Ho = y.shape[2]
    L = G.lib()
    s = N.stream_ptr(dev)
    xd, gyd = _nhwc(x.detach()).float().to(dev), _nhwc(gy).float().to(dev)
    yd, gxd = torch.full((n, Ho, Ho, C), float("nan"), device=dev), torch.full((n, H, H, C), float("nan"), device=dev)
    G.check(L.apg_maxpool_fwd(N.dptr(xd), n, H, H, C, N.dptr(yd), s), "apg_maxpool_fwd")
    G.check(L.apg_maxpool_bwd(N.dptr(xd), n, H, H, C, N.dptr(gyd), N.dptr(gxd), s), "apg_maxpool_bwd")
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), _nhwc(y.detach()).float())
    assert torch.equal(gxd.cpu(), _nhwc(x.grad).float())


def test_avgpool_matches_fp64(dev):
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, C = 3, 2048
    g = torch.Generator().manual_seed(6)
    a = torch.randn(n, C, 7, 7, generator=g)
    ga = torch.randn(n, C, generator=g)
    a64 = a.double().requires_grad_(True)
    ya = F.avg_pool2d(a64, 7, stride=1).flatten(1)
    ya.backward(ga.double())
    L = G.lib()
    s = N.stream_ptr(dev)
    yad, gxa = torch.full((n, C), float("nan"), device=dev), torch.full((n, 7, 7, C), float("nan"), device=dev)
    G.check(L.apg_avgpool_fwd(N.dptr(_nhwc(a).to(dev)), n, C, N.dptr(yad), s), "apg_avgpool_fwd")
    G.check(L.apg_avgpool_bwd(N.dptr(ga.to(dev)), n, C, N.dptr(gxa), s), "apg_avgpool_bwd")
    torch.cuda.synchronize()
    ratios = {}
    _check("avgpool", "y", yad, ya.detach(), F.avg_pool2d(a.double().abs(), 7, stride=1).flatten(1), ratios)
    _check("avgpool", "gx", gxa, _nhwc(a64.grad), _nhwc(a64.grad.abs()), ratios)
    _report("avgpool n3 C2048", ratios)
