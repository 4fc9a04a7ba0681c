"""Shared by the test_real_loss_* files: a seeded VPoser encoder under the published state-dict keys (and the packed fixture
of the GPU tests, on loss_util's dev), the literal layer chain, the
copenet_real trainers' get_loss restated from torch ops (any dtype, any device; gradients by autograd), and seeded cases whose
rotations keep clear of the axis-angle conversion's branch boundaries and singularities."""
import ctypes

import pytest
import torch

from oracle import geometry_ref

NJ, NR, NZ = 22, 21, 32
LIMB1, LIMB2 = (4, 5, 18, 19), (7, 8, 20, 21)
PRED = ("rotmat", "betas", "j2d", "depth")
TERMS = ("loss", "vposer", "pose", "keypoints", "betas", "depth")
X_POSE, X_BETAS = 4, 8
# the shapes of get_loss among the five trainers: views, cross-view bits, the barrier's (column, gain)
FORMS = {"twoview": dict(nviews=2, cross=X_POSE | X_BETAS, col=2, gain=1.0), "hmr": dict(nviews=1, cross=0, col=0, gain=10.0),
         "spin": dict(nviews=1, cross=0, col=2, gain=1.0)}
W_NAMES = ("kp", "beta", "vposer", "pose", "limbs2d", "scale")
WEIGHTS = (0.001, 1.0, 1.0, 1.0, 1.5, 60.0)                   # copenet_twoview.py's defaults


def make_encoder(seed=0, prefix=""):
    """a seeded encoder_net state dict under the published keys, activations O(1) at every layer"""
    g = torch.Generator().manual_seed(9000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    sd = {}

    def bn(i, n):
        sd["encoder_net.%d.weight" % i], sd["encoder_net.%d.bias" % i] = 1 + 0.2 * r(n), 0.1 * r(n)
        sd["encoder_net.%d.running_mean" % i], sd["encoder_net.%d.running_var" % i] = 0.2 * r(n), 0.5 + u(n)
        sd["encoder_net.%d.num_batches_tracked" % i] = torch.tensor(1000)

    def lin(name, o, i):
        sd["encoder_net.%s.weight" % name], sd["encoder_net.%s.bias" % name] = r(o, i) / i ** 0.5, 0.1 * r(o)
    bn(1, 63), lin("2", 512, 63), bn(4, 512), lin("6", 512, 512), lin("7", 512, 512), lin("8.mu", 32, 512), lin("8.logvar", 32, 512)
    return {prefix + k: v for k, v in sd.items()}


def encoder_chain(sd, aa, bn_eps=1e-5):
    """the literal eval-mode layer chain of encoder_net on aa (N, 63), in aa's dtype and on its device -> (mu, s), (N, 32) each:
    BatchFlatten, BatchNorm1d(63), Linear(63, 512), LeakyReLU(0.01), BatchNorm1d(512), Dropout (identity), Linear(512, 512),
    Linear(512, 512), NormalDistDecoder's two heads (the posterior's scale is softplus(s))"""
    p = lambda k: sd["encoder_net." + k].to(device=aa.device, dtype=aa.dtype)
    F = torch.nn.functional
    x = aa.reshape(aa.shape[0], -1)
    x = F.batch_norm(x, p("1.running_mean"), p("1.running_var"), p("1.weight"), p("1.bias"), False, 0.1, bn_eps)
    x = F.leaky_relu(F.linear(x, p("2.weight"), p("2.bias")), 0.01)
    x = F.batch_norm(x, p("4.running_mean"), p("4.running_var"), p("4.weight"), p("4.bias"), False, 0.1, bn_eps)
    x = F.linear(F.linear(x, p("6.weight"), p("6.bias")), p("7.weight"), p("7.bias"))
    return F.linear(x, p("8.mu.weight"), p("8.mu.bias")), F.linear(x, p("8.logvar.weight"), p("8.logvar.bias"))


def axis_angle(rotmat, to_aa=geometry_ref.rotation_matrix_to_angle_axis):
    """the trainers' lines: rotmat[:, 1:] zero-padded to 3 x 4, tgm's conversion, (B, 63)"""
    B = rotmat.shape[0]
    pad = torch.cat([rotmat[:, 1:], torch.zeros(B, NR, 3, 1, dtype=rotmat.dtype, device=rotmat.device)], dim=3).view(-1, 3, 4)
    return to_aa(pad).reshape(B, NR * 3)


def limb_vec(l, dt, dev="cpu", sets=(LIMB1, LIMB2)):
    lw = torch.ones(NJ, dtype=dt, device=dev)
    for j in sets[0]:
        lw[j] = l
    for j in sets[1]:
        lw[j] = l * l
    return lw


def loss_terms(c, P, sd, gt=None, eps=None):
    """get_loss as the trainers write it, on per-view dicts P of PRED tensors, in their dtype and on their device -> the six terms
    (0-d tensors) in TERMS order.  c: nviews, cross, col, gain, w (W_NAMES order); gt / eps default to c's"""
    w = [float(x) for x in c["w"]]
    nv, cross = c["nviews"], c["cross"]
    ref = P[0]["rotmat"]
    d = lambda t: t.to(device=ref.device, dtype=ref.dtype)
    gt = c["gt"] if gt is None else gt
    eps = c["eps"] if eps is None else eps
    zero = torch.zeros((), dtype=ref.dtype, device=ref.device)
    lw = limb_vec(w[4], ref.dtype, ref.device)[None, :, None]
    kp, vp, betas, depth = zero, zero, zero, zero
    for v in range(nv):
        g = d(gt[v])
        kp = kp + ((P[v]["j2d"][:, :NJ] - g[:, :NJ, :2]) ** 2 * g[:, :NJ, 2:] * lw).mean()
        mu, s = encoder_chain(sd, axis_angle(P[v]["rotmat"]))
        z = mu + torch.nn.functional.softplus(s) * d(eps[v])
        vp = vp + (z * z).mean()
        betas = betas + (P[v]["betas"] * P[v]["betas"]).mean()
        depth = depth + (torch.exp(-P[v]["depth"][:, c["col"]] * c["gain"]) ** 2).mean()
    pose = ((P[0]["rotmat"][:, 1:] - P[1]["rotmat"][:, 1:]) ** 2).mean() if cross & X_POSE else zero
    if cross & X_BETAS:
        betas = betas + ((P[0]["betas"] - P[1]["betas"]) ** 2).mean()
    loss = (w[0] * kp + w[1] * betas + w[2] * vp + w[3] * pose + depth) * w[5]
    return loss, vp, pose, kp, betas, depth


# ------------------------------------------------------------------------------------------------ the encoder the GPU tests share
SD = make_encoder(1)
SD64 = {k: v.double() for k, v in SD.items()}


def folded(sd=SD, bn_eps=None):
    """loss_real.fold_encoder of sd (fp64), optionally with another BatchNorm eps"""
    from airpose_amd import loss_real
    if bn_eps is None:
        return loss_real.fold_encoder(sd)
    keep = loss_real.BN_EPS
    loss_real.BN_EPS = bn_eps
    try:
        return loss_real.fold_encoder(sd)
    finally:
        loss_real.BN_EPS = keep


@pytest.fixture(scope="module")
def packed(dev):
    """SD folded in fp64 and packed once per test file, into a NaN-filled, NaN-guarded buffer: written in full, nothing outside"""
    from airpose_amd import _native_grad as G
    L = G.lib()
    nbytes = L.apg_real_loss_encoder_bytes()
    n, guard = nbytes // 4, 512
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=dev)
    out = buf[guard:guard + n]
    src = [t.float().contiguous().to(dev) for t in folded()]
    G.check(L.apg_real_loss_pack_encoder(*[ctypes.c_void_p(t.data_ptr()) for t in src], ctypes.c_void_p(out.data_ptr()), nbytes,
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "apg_real_loss_pack_encoder")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all(), "the packed table's guard bands were written"
    assert not torch.isnan(out).any(), "the packed table was not written in full"
    return out


# ------------------------------------------------------------------------------------------------ rotations and cases
def branch_of(R):
    """the quaternion branch (0 .. 3) tgm takes for each (N, 3, 3) rotation, on its transposed matrix"""
    rt = R.transpose(1, 2)
    d2, d01, d0n1 = rt[:, 2, 2] < 1e-6, rt[:, 0, 0] > rt[:, 1, 1], rt[:, 0, 0] < -rt[:, 1, 1]
    return torch.where(d2, torch.where(d01, 0, 1), torch.where(d0n1, 2, 3))


def too_close(R):
    """(N,) bool, in fp64: within 1e-2 of a branch-selection boundary (t22 = 1e-6, t00 = t11, t00 = -t11), |w| < 1e-2, or
    sin(theta / 2) < 5e-2 (which also keeps the identity out, where the conversion's derivative is 0 / 0)"""
    R = R.double()
    rt = R.transpose(1, 2)
    near = ((rt[:, 2, 2] - 1e-6).abs() < 1e-2) | ((rt[:, 0, 0] - rt[:, 1, 1]).abs() < 1e-2) | ((rt[:, 0, 0] + rt[:, 1, 1]).abs() < 1e-2)
    q = geometry_ref.rotation_matrix_to_quaternion(R)
    return near | (q[:, 0].abs() < 1e-2) | (q[:, 1:].norm(dim=1) < 5e-2)


def draw_rot6d(n, g):
    """n seeded normal 6-vectors and their fp32 rotations (rot6d_to_rotmat), each rotation inside a band of too_close() drawn again
    (never left out) -> ((n, 6), (n, 3, 3), the number drawn again)"""
    x = torch.randn(n, 6, generator=g)
    again = 0
    while True:
        R = geometry_ref.rot6d_to_rotmat(x)
        bad = too_close(R).nonzero().flatten()
        if not len(bad):
            return x, R.contiguous(), again
        again += len(bad)
        x[bad] = torch.randn(len(bad), 6, generator=g)


def draw_rotations(n, g):
    _, R, again = draw_rot6d(n, g)
    return R, again


def make_case(form, B, J, Jg, seed=0, limbs=1.5, weights=WEIGHTS):
    f = FORMS[form]
    g = torch.Generator().manual_seed(7000 + 1000 * seed + 7 * B + J + 31 * f["nviews"])
    r = lambda *s: torch.randn(*s, generator=g)
    w = list(weights)
    w[4] = limbs
    c = dict(form=form, B=B, J=J, Jg=Jg, seed=seed, w=torch.tensor(w, dtype=torch.float32), pred=[], gt=[], eps=[], redrawn=0, **f)
    for v in range(f["nviews"]):
        R, again = draw_rotations(B * NJ, g)
        c["redrawn"] += again
        depth = torch.cat([torch.rand(B, 1, generator=g) * 2.2 - 0.2, r(B, 1), torch.rand(B, 1, generator=g) * 6 + 0.5], 1)
        j2d = r(B, J, 2) * 100 + 500
        conf = torch.rand(B, Jg, 1, generator=g)
        conf[torch.rand(B, Jg, 1, generator=g) < 0.2] = 0.0                # detector misses: confidence exactly 0
        c["pred"].append(dict(rotmat=R.view(B, NJ, 3, 3), betas=r(B, 10), j2d=j2d, depth=depth))
        c["gt"].append(torch.cat([j2d[:, :1].expand(B, Jg, 2) + r(B, Jg, 2) * 5, conf], 2).contiguous())
        c["eps"].append(r(B, NZ))
    return c
