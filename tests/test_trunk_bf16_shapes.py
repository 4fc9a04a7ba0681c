"""The bf16 training mode's layer primitives (libairpose_grad.so: trunk_grad_bf16.hip) against torch CPU fp64 on bf16-representable
inputs: fp32 values are drawn, rounded to bf16 (round to nearest even) and handed to both sides.

Bars (derived, not measured; u = 2^-8 is bf16's unit roundoff, TAU = 1e-5 and A as in tests/test_trunk_grad_shapes.py: the same
expression in fp64 with every operand replaced by its absolute value and every subtraction turned into an addition):
  - bf16-stored outputs (conv y, conv gx, BatchNorm y, gx): element-wise |got - ref| <= u |ref| + (1 + u) TAU A -- one final RNE on
    top of the fp32-accumulation bar the fp32 kernels meet; where A == 0 the result must be exactly 0;
  - fp32 outputs (gw, g_gamma, g_beta, save_mean, save_invstd, running statistics, xf): rel_err <= 1e-5 and |got - ref| <= TAU A;
  - g_res, max-pool forward and backward: bitwise.
Each case prints its worst err / bar per tensor; DESIGN 4.3.4 records them."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, rel_err

pytestmark = pytest.mark.gpu
TAU = 1e-5
U = 2.0 ** -8
MOM, EPS = 0.1, 1e-5
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _q(t):
    """fp32 -> the nearest bf16 value (RNE), as fp32"""
    return t.to(BF).float()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _check16(what, name, got, ref, A, out):
    """a bf16-stored output: |got - ref| <= u |ref| + (1 + u) TAU A element-wise, exactly 0 where A == 0"""
    got = got.detach().cpu().double()
    ref, A = ref.detach().cpu().double(), A.detach().cpu().double()
    assert got.shape == ref.shape == A.shape, (what, name, got.shape, ref.shape, A.shape)
    assert torch.isfinite(got).all(), (what, name, "non-finite output (an element never written?)")
    err, lim = (got - ref).abs(), U * ref.abs() + (1 + U) * TAU * A
    zero = A == 0
    assert not (got[zero] != 0).any(), (what, name, "%d elements nonzero where every term is 0" % int((got[zero] != 0).sum()))
    ratio = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    out[name] = ratio
    assert ratio <= 1.0, (what, name, "worst |err| / (u |ref| + (1 + u) tau A) %.3f" % ratio)


def _check32(what, name, got, ref, A, out, rel_bar=1e-5):
    """an fp32 output: the fp32 file's bars unchanged"""
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
    print("%-40s %s  worst err/bar: %s" % (what, extra, "  ".join("%s %.4f" % kv for kv in ratios.items())))


# ------------------------------------------------------------------------------------------------ weight pack
@pytest.mark.parametrize("K,C,Cp,R", [(64, 3, 8, 7), (64, 64, 64, 3), (136, 72, 72, 1), (16, 5, 16, 3)])
def test_weight_pack_is_rne_in_both_layouts(dev, K, C, Cp, R):
    """fp32 values that are NOT bf16-representable: the packed copies must be torch's RNE cast bit for bit, wf as [co][r][s][c]
    and wd as [c][r][s][co], padded channels zero (truncation, or the two layouts swapped, fails here)"""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    w = torch.randn(K, C, R, R, generator=torch.Generator().manual_seed(K + C))
    want = torch.zeros(K, Cp, R, R, dtype=BF)
    want[:, :C] = w.to(BF)
    wf = torch.full((K, R, R, Cp), float("nan"), device=dev, dtype=BF)
    wd = torch.full((Cp, R, R, K), float("nan"), device=dev, dtype=BF)
    G.check(G.lib().apg_pack_weights_bf16(N.dptr(w.to(dev)), K, C, Cp, R, R, _p(wf), _p(wd), N.stream_ptr(dev)), "apg_pack_weights_bf16")
    torch.cuda.synchronize()
    assert torch.equal(wf.cpu().view(torch.int16), want.permute(0, 2, 3, 1).contiguous().view(torch.int16))
    assert torch.equal(wd.cpu().view(torch.int16), want.permute(1, 2, 3, 0).contiguous().view(torch.int16))
    assert (w.to(BF).float() != w).any()


# ------------------------------------------------------------------------------------------------ convolution
def _conv64(x, w, gy, st, pad):
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    y = F.conv2d(x, w, stride=st, padding=pad)
    y.backward(gy.double())
    return y.detach(), x.grad, w.grad


def _run_conv(dev, geom, seed):
    """geom = (n, H, W, C, K, R, S, stride, pad), C the real input channel count (padded with zero channels to a multiple of 8
    for the kernels, the stem's 3 -> 8).  Returns the worst err / bar per tensor and the weight gradient's split-K chunk count."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, H, W, C, K, R, S, st, pad = geom
    Cp = (C + 7) // 8 * 8
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    g = torch.Generator().manual_seed(seed)
    x = _q(torch.randn(n, C, H, W, generator=g))                      # bf16-representable: the values both sides see
    w = _q(torch.randn(K, C, R, S, generator=g) * (2.0 / (C * R * S)) ** 0.5)
    gy = _q(torch.randn(n, K, Ho, Wo, generator=g))
    add = _q(torch.randn(n, C, H, W, generator=g))
    y64, gx64, gw64 = _conv64(x, w, gy, st, pad)
    Ay, Agx, Agw = _conv64(x.abs(), w.abs(), gy.abs(), st, pad)
    L = G.lib()
    s = N.stream_ptr(dev)
    pad_c = lambda t: F.pad(_nhwc(t), (0, Cp - C))                     # NHWC with zero channels C .. Cp - 1
    xd, gyd, addd = pad_c(x).to(dev, BF), _nhwc(gy).to(dev, BF), pad_c(add).to(dev, BF)
    nan16 = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=BF)
    nan32 = lambda *shape: torch.full(shape, float("nan"), device=dev)
    wf, wd = nan16(K, R, S, Cp), nan16(Cp, R, S, K)
    G.check(L.apg_pack_weights_bf16(N.dptr(w.to(dev)), K, C, Cp, R, S, _p(wf), _p(wd), s), "apg_pack_weights_bf16")
    nb = L.apg_conv_bwd_bf16_workspace_bytes(n, H, W, Cp, K, R, S, st, pad)
    per = 4 * K * Cp * R * S
    assert nb > 0 and nb % per == 0, (geom, nb)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    yd = nan16(n, Ho, Wo, K)
    G.check(L.apg_conv_fwd_bf16(_p(xd), n, H, W, Cp, _p(wf), K, R, S, st, pad, _p(yd), s), "apg_conv_fwd_bf16")
    outs = []
    for _ in range(2):
        gxd, gwd = nan16(n, H, W, Cp), nan32(K, C, R, S)
        G.check(L.apg_conv_bwd_bf16(_p(xd), n, H, W, Cp, _p(wd), K, R, S, st, pad, _p(gyd), None, 0, _p(gxd), 0, _p(gwd), C, ws.data_ptr(), nb,
                                    s), "apg_conv_bwd_bf16")
        outs.append((gxd, gwd))
    (gxd, gwd), (gxd2, gwd2) = outs
    # the fused add (fp32 add, one rounding), in place over the addend as the walker runs it; and the fp32 form of gx
    gxa = addd.clone()
    G.check(L.apg_conv_bwd_bf16(None, n, H, W, Cp, _p(wd), K, R, S, st, pad, _p(gyd), _p(gxa), 0, _p(gxa), 0, None, 0, None, 0, s),
            "apg_conv_bwd_bf16")
    gxf = nan32(n, H, W, Cp)
    G.check(L.apg_conv_bwd_bf16(None, n, H, W, Cp, _p(wd), K, R, S, st, pad, _p(gyd), None, 0, _p(gxf), 1, None, 0, None, 0, s),
            "apg_conv_bwd_bf16")
    # an fp32 addend (a downsample branch's fp32 data gradient): the same sum, the one rounding
    gxb = nan16(n, H, W, Cp)
    G.check(L.apg_conv_bwd_bf16(None, n, H, W, Cp, _p(wd), K, R, S, st, pad, _p(gyd), _p(addd.float()), 1, _p(gxb), 0, None, 0, None, 0, s),
            "apg_conv_bwd_bf16")
    torch.cuda.synchronize()
    assert torch.equal(gxb.view(torch.int16), gxa.view(torch.int16)), (geom, "fp32 and bf16 forms of the same addend differ")
    ratios = {}
    _check16(geom, "y", yd.float(), _nhwc(y64), _nhwc(Ay), ratios)
    _check16(geom, "gx", gxd.float(), pad_c(gx64), pad_c(Agx), ratios)             # the padded channels: A == 0, exactly 0
    _check16(geom, "gx+add", gxa.float(), pad_c(gx64 + add.double()), pad_c(Agx + add.double().abs()), ratios)
    _check32(geom, "gx32", gxf, pad_c(gx64), pad_c(Agx), ratios)
    _check32(geom, "gw", gwd, gw64, Agw, ratios)
    assert torch.equal(gxf.to(BF).view(torch.int16), gxd.view(torch.int16)), (geom, "bf16 gx is not the RNE of the fp32 gx")
    assert torch.equal(gwd, gwd2) and torch.equal(gxd.view(torch.int16), gxd2.view(torch.int16)), (geom, "two identical calls differ")
    return ratios, nb // per


@functools.lru_cache(maxsize=None)
def _trunk_geoms():
    """Every distinct (H, C, K, R, stride, pad) of the trunk's 53 convolutions, H = the conv's input size (the walk of
    tests/test_trunk_grad_shapes.py)"""
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
    out = []
    for c in [c for c, _ in trunk_grad.conv_bn_pairs(net)]:
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
    assert TRUNK_GEOMS[0] == (224, 3, 64, 7, 2, 3)                   # the stem: C_in = 3 through the 8-channel padding


@pytest.mark.parametrize("geo", TRUNK_GEOMS, ids=[_gid(g) for g in TRUNK_GEOMS])
def test_trunk_conv_geometry_matches_fp64(dev, geo):
    """The geometry at its real size, with the smallest n <= 16 whose weight gradient runs in >= 2 split-K chunks of which the
    last is ragged: n Ho Wo not divisible by the chunk count, so no equal split exists."""
    from airpose_amd import _native_grad as G
    H, C, K, R, st, pad = geo
    Cp = (C + 7) // 8 * 8
    Ho = (H + 2 * pad - R) // st + 1
    L = G.lib()
    per = 4 * K * Cp * R * R
    for n in range(1, 17):
        nch = L.apg_conv_bwd_bf16_workspace_bytes(n, H, H, Cp, K, R, R, st, pad) // per
        if nch >= 2 and (n * Ho * Ho) % nch != 0:
            break
    else:
        pytest.fail("no n <= 16 gives a multi-chunk, ragged weight gradient for %s" % (geo,))
    ratios, nch = _run_conv(dev, (n, H, H, C, K, R, R, st, pad), seed=sum(geo) + n)
    _report(_gid(geo), ratios, "n %2d, %2d wgrad chunks over %6d pixels" % (n, nch, n * Ho * Ho))


GEOMS_OUT7 = [g for g in TRUNK_GEOMS if (g[0] + 2 * g[5] - g[3]) // g[4] + 1 == 7]


@pytest.mark.parametrize("geo", GEOMS_OUT7, ids=[_gid(g) for g in GEOMS_OUT7])
def test_layer4_geometry_at_one_image_matches_fp64(dev, geo):
    """layer4 as the walker runs it at n = 1: M = 49 output rows, below one 64-row tile"""
    assert len(GEOMS_OUT7) == 5
    H, C, K, R, st, pad = geo
    ratios, nch = _run_conv(dev, (1, H, H, C, K, R, R, st, pad), seed=3 * sum(geo))
    _report(_gid(geo) + " n 1", ratios, "%d wgrad chunks over 49 pixels" % nch)


API_GEOMS = [  # (n, H, W, C, K, R, S, stride, pad)
    (2, 13, 21, 64, 64, 3, 3, 2, 1),             # H != W
    (2, 12, 12, 32, 32, 1, 5, 1, 2),             # R != S
    (2, 17, 17, 16, 32, 5, 5, 3, 2),             # 5 x 5, stride 3
    (2, 10, 10, 8, 32, 3, 3, 1, 1),              # C = 8: a K stage of 64 spans 8 taps
    (2, 11, 11, 72, 40, 3, 3, 1, 1),             # 64 x 64 tile: partial N (40), a stage across two taps (C = 72), partial M
    (2, 10, 10, 32, 80, 1, 1, 1, 0),             # 64 x 64 tile: a full and a partial N tile; K total 32 < one stage
    (2, 5, 5, 3, 16, 3, 3, 1, 1),                # C = 3 padded to 8 away from the stem
    (1, 1, 1, 64, 64, 1, 1, 1, 0),               # n = 1, a 1 x 1 map
    (1, 1, 1, 64, 64, 3, 3, 1, 1),               # n = 1, 1 x 1 map, 3 x 3 / p1: eight of nine taps in the padding
    (2, 16, 16, 32, 32, 3, 3, 2, 0),             # 3 x 3 / s2 / p0 on an even H: the last row / column is read by no window
    (2, 7, 7, 2048, 16, 1, 1, 1, 0),             # C = 2048 -> K = 16 at 7 x 7
    (2, 130, 130, 136, 136, 1, 1, 1, 0),         # 128 x 128 tile in all three modes: partial M (33 800 = 264 x 128 + 8), partial N (136)
    (2, 100, 100, 136, 136, 3, 3, 1, 1),         # 128 x 128 tile, 3 x 3: stages across taps (C = 136), partial M and N
    (5, 90, 90, 128, 200, 3, 3, 2, 1),           # 128 x 128 tile, stride 2 data gradient (M = 40 500 rows x N = 128), 64 x 64 forward
]
API_IDS = ["HneW", "RneS", "5x5s3", "C8", "t64-partial", "K80", "C3pad", "1x1map-1x1", "1x1map-3x3p1", "3x3s2p0-evenH", "C2048-K16",
           "t128-1x1-partial", "t128-3x3-partial", "t128-s2-dgrad"]


@pytest.mark.parametrize("geom", API_GEOMS, ids=API_IDS)
def test_conv_api_shapes_match_fp64(dev, geom):
    ratios, nch = _run_conv(dev, geom, seed=7 + sum(geom))
    _report("%s" % (geom,), ratios, "%d wgrad chunks" % nch)


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_inputs(M, C, seed, ratio=None):
    g = torch.Generator().manual_seed(seed)
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 2 if ratio is None else ratio * scale * torch.tensor([(-1.0) ** c for c in range(C)])
    x = _q(torch.randn(M, C, generator=g) * scale + shift)
    gam = torch.randn(C, generator=g)
    bet = torch.randn(C, generator=g)
    res = _q(torch.randn(M, C, generator=g))
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    gy = _q(torch.randn(M, C, generator=g))
    return x, gam, bet, res, rm, rv, gy


def _run_bn(dev, M, C, train, res, relu, seed, ratio=None):
    """apg_bn_fwd_bf16 / apg_bn_bwd_bf16 on (M, C) rows against F.batch_norm + autograd in fp64 on the same bf16 values; then the
    same calls in place (y over x, gx over gy) must give the same bits.  The backward's ReLU mask is the kernel's own y > 0."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    x, gam, bet, r, rm, rv, gy = _bn_inputs(M, C, seed, ratio)
    L = G.lib()
    s = N.stream_ptr(dev)
    nb = L.apg_bn_bf16_workspace_bytes(M, C)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    xd, rd, gyd = (t.to(dev, BF) for t in (x, r, gy))
    gd, bd = gam.to(dev), bet.to(dev)
    nan16 = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=BF)
    nan32 = lambda *shape: torch.full(shape, float("nan"), device=dev)

    def fwd(x_in, y_out):
        rmd, rvd, mean, invstd = rm.to(dev), rv.to(dev), nan32(C), nan32(C)
        G.check(L.apg_bn_fwd_bf16(_p(x_in), M, C, N.dptr(gd), N.dptr(bd), N.dptr(rmd), N.dptr(rvd), train, MOM, EPS,
                                  _p(rd) if res else None, int(relu), _p(y_out), N.dptr(mean), N.dptr(invstd), ws.data_ptr(), nb, s),
                "apg_bn_fwd_bf16")
        return rmd, rvd, mean, invstd

    def bwd(gy_in, gx_out, yd):
        gres, gg, gb = nan16(M, C), nan32(C), nan32(C)
        G.check(L.apg_bn_bwd_bf16(_p(gy_in), _p(yd) if relu else None, _p(xd), M, C, N.dptr(gd), N.dptr(mean), N.dptr(invstd), train,
                                  _p(gx_out), _p(gres), N.dptr(gg), N.dptr(gb), ws.data_ptr(), nb, s), "apg_bn_bwd_bf16")
        return gres, gg, gb

    bits = lambda t: t.view(torch.int16) if t.dtype == BF else t
    same = lambda a, b: torch.equal(bits(a), bits(b))
    yd = nan16(M, C)
    rmd, rvd, mean, invstd = fwd(xd, yd)
    gxd = nan16(M, C)
    gres, gg, gb = bwd(gyd, gxd, yd)
    yi = xd.clone()
    inplace_f = fwd(yi, yi)
    gxi = gyd.clone()
    inplace_b = bwd(gxi, gxi, yd)
    torch.cuda.synchronize()
    assert same(yi, yd) and all(same(a, b) for a, b in zip(inplace_f, (rmd, rvd, mean, invstd))), "apg_bn_fwd_bf16 in place"
    assert same(gxi, gxd) and all(same(a, b) for a, b in zip(inplace_b, (gres, gg, gb))), "apg_bn_bwd_bf16 in place"

    x64, r64 = x.double().requires_grad_(True), r.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    rm64, rv64 = rm.double(), rv.double()
    pre = F.batch_norm(x64, rm64, rv64, g64, b64, bool(train), MOM, EPS)
    if res:
        pre = pre + r64
    mask = (yd.float().cpu() > 0).double() if relu else torch.ones(M, C, dtype=torch.float64)
    (pre * mask * gy.double()).sum().backward()
    if train:
        mu, var = x64.detach().mean(0), x64.detach().var(0, unbiased=False)
    else:
        mu, var = rm.double(), rv.double()
    istd = 1 / torch.sqrt(var + EPS)
    xa = (x.double().abs() + mu.abs()) * istd
    Ay = xa * gam.double().abs() + bet.double().abs() + (r.double().abs() if res else 0)
    ga = gy.double().abs() * mask
    if train:
        Agx = gam.double().abs() * istd * (ga + ga.mean(0) + xa * (ga * xa).mean(0))
    else:
        Agx = gam.double().abs() * istd * ga
    ratios = {}
    what = (M, C, train, res, relu)
    y64 = pre.detach().clamp_min(0) if relu else pre.detach()
    _check16(what, "y", yd.float(), y64, Ay, ratios)
    _check16(what, "gx", gxd.float(), x64.grad, Agx, ratios)
    _check32(what, "ggamma", gg, g64.grad, (ga * xa).sum(0), ratios)
    _check32(what, "gbeta", gb, b64.grad, ga.sum(0), ratios)
    assert torch.equal(gres.float().cpu(), gy * mask.float()), (what, "g_res is g = gy (y > 0)")
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
    (49, 8, 1, 0, 0), (300, 8, 1, 0, 1), (300, 8, 1, 1, 1), (49, 2048, 1, 0, 0), (98, 2048, 1, 1, 1),
    (300, 8, 0, 0, 0), (1, 8, 0, 1, 1), (98, 2048, 0, 0, 1),
]


@pytest.mark.parametrize("case", BN_CASES, ids=[_bid(c) for c in BN_CASES])
def test_batchnorm_sizes_match_fp64(dev, case):
    ratios, e = _run_bn(dev, *case, seed=sum(case))
    _report(_bid(case), ratios, " ".join("%s %.1e" % kv for kv in e.items()))


def test_batchnorm_cancellation_at_stem_size(dev):
    """|mean| / std = 100 in every channel over the stem's 401 408 rows (n = 32), on bf16-rounded values (steps of 0.5 at 100)"""
    ratios, e = _run_bn(dev, 401408, 64, 1, 0, 1, seed=99, ratio=100.0)
    _report("cancellation M401408 ratio 100", ratios, " ".join("%s %.1e" % kv for kv in e.items()))


@pytest.mark.parametrize("M,C", [(3, 8), (257, 64), (1027, 72)])
def test_batchnorm_reductions_are_bitwise_the_fp32_path(dev, M, C):
    """The fp32 and bf16 BatchNorm are one source (csrc/trunk_elem.inc) on two storage types: on bf16-representable x and gy both
    read the same fp32 values and reduce them in the same per-channel order, so every fp32 output of the reductions is equal bit
    for bit (y and gx differ in storage and are not compared).  Train mode, no residual, no ReLU.  (3, 8): one tile, only its
    first quarter has rows, one partial channel group; (257, 64): two tiles, the second of one row; (1027, 72): five tiles with a
    ragged last one, the second channel group cut at 8 of 64 lanes."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    x, gam, bet, _, rm, rv, gy = _bn_inputs(M, C, seed=M + C)
    L = G.lib()
    s = N.stream_ptr(dev)
    gd, bd = gam.to(dev), bet.to(dev)
    nan32 = lambda *shape: torch.full(shape, float("nan"), device=dev)
    outs = {}
    for name, dt, nbytes, fwd, bwd in (("fp32", torch.float32, L.apg_bn_workspace_bytes, L.apg_bn_fwd, L.apg_bn_bwd),
                                       ("bf16", BF, L.apg_bn_bf16_workspace_bytes, L.apg_bn_fwd_bf16, L.apg_bn_bwd_bf16)):
        nb = nbytes(M, C)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        xd, gyd = x.to(dev, dt), gy.to(dev, dt)
        yd, gxd = torch.empty_like(xd), torch.empty_like(xd)
        rmd, rvd, mean, invstd, gg, gb = rm.to(dev), rv.to(dev), nan32(C), nan32(C), nan32(C), nan32(C)
        G.check(fwd(_p(xd), M, C, N.dptr(gd), N.dptr(bd), N.dptr(rmd), N.dptr(rvd), 1, MOM, EPS, None, 0, _p(yd), N.dptr(mean),
                    N.dptr(invstd), ws.data_ptr(), nb, s), "apg_bn_fwd " + name)
        G.check(bwd(_p(gyd), None, _p(xd), M, C, N.dptr(gd), N.dptr(mean), N.dptr(invstd), 1, _p(gxd), None, N.dptr(gg), N.dptr(gb),
                    ws.data_ptr(), nb, s), "apg_bn_bwd " + name)
        outs[name] = {"save_mean": mean, "save_invstd": invstd, "running_mean": rmd, "running_var": rvd, "g_gamma": gg, "g_beta": gb}
    torch.cuda.synchronize()
    for k, a in outs["fp32"].items():
        b = outs["bf16"][k]
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (M, C, k, "non-finite output (an element never written?)")
        assert torch.equal(a, b), (M, C, k, "fp32 and bf16 storage differ by up to %.3e" % float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("n,H,C", [(2, 112, 64), (2, 1, 64), (2, 2, 64), (2, 3, 64), (1, 3, 16), (1, 5, 8)])
def test_maxpool_matches_torch_bitwise(dev, n, H, C):
    """Integer post-ReLU data (exact in bf16): ~60 % zeros make all-tie windows, integer gradients sum exactly"""
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
    xd, gyd = _nhwc(x.detach()).to(dev, BF), _nhwc(gy).to(dev, BF)
    yd = torch.full((n, Ho, Ho, C), float("nan"), device=dev, dtype=BF)
    gxd = torch.full((n, H, H, C), float("nan"), device=dev, dtype=BF)
    G.check(L.apg_maxpool_fwd_bf16(_p(xd), n, H, H, C, _p(yd), s), "apg_maxpool_fwd_bf16")
    G.check(L.apg_maxpool_bwd_bf16(_p(xd), n, H, H, C, _p(gyd), _p(gxd), s), "apg_maxpool_bwd_bf16")
    torch.cuda.synchronize()
    assert torch.equal(yd.float().cpu(), _nhwc(y.detach()).float())
    assert torch.equal(gxd.float().cpu(), _nhwc(x.grad).float())


def test_avgpool_matches_fp64(dev):
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, C = 3, 2048
    g = torch.Generator().manual_seed(6)
    a = _q(torch.randn(n, C, 7, 7, generator=g))
    ga = torch.randn(n, C, generator=g)
    a64 = a.double().requires_grad_(True)
    ya = F.avg_pool2d(a64, 7, stride=1).flatten(1)
    ya.backward(ga.double())
    L = G.lib()
    s = N.stream_ptr(dev)
    yad = torch.full((n, C), float("nan"), device=dev)
    gxa = torch.full((n, 7, 7, C), float("nan"), device=dev, dtype=BF)
    G.check(L.apg_avgpool_fwd_bf16(_p(_nhwc(a).to(dev, BF)), n, C, N.dptr(yad), s), "apg_avgpool_fwd_bf16")
    G.check(L.apg_avgpool_bwd_bf16(N.dptr(ga.to(dev)), n, C, _p(gxa), s), "apg_avgpool_bwd_bf16")
    torch.cuda.synchronize()
    ratios = {}
    _check32("avgpool", "xf", yad, ya.detach(), F.avg_pool2d(a.double().abs(), 7, stride=1).flatten(1), ratios)
    _check16("avgpool", "gx", gxa.float(), _nhwc(a64.grad), _nhwc(a64.grad.abs()), ratios)
    _report("avgpool n3 C2048", ratios)
