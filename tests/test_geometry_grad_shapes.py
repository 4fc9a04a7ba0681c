"""The geometry adjoints through the C ABI (apg_rot6d_to_rotmat_bwd, apg_perspective_projection_bwd, apg_transform_points_bwd,
geom_grad.hip) against fp64 autograd through oracle/geometry_ref.py at the sizes, NULL patterns and clamp branches that
tests/test_geometry_grad.py (one number per tensor, 1e-4, P <= 2000, every output requested) does not reach.

Every case: fp32 inputs, the oracle in fp64 on the same fp32 values, outputs inside a NaN-filled arena (an output that was not
asked for, and the guards between outputs, must stay NaN), two identical calls compared with torch.equal, and per tensor
  - rel_err <= 1e-5;
  - element-wise |got - ref| <= 1e-5 A, exactly 0 where A == 0.
A is the adjoint's own expression in fp64 on absolute values with every subtraction turned into an addition: the camera-space
point |R| |p| + |t|, gZ = (fx |gx| Xa + fy |gy| Ya) / Z^2, the normalisation's (|g| + |b| (|b| . |g|)) / n, the Gram-Schmidt
d = |b1| . |a2| and u = |a2| + d |b1|, the cross products with every sign positive.  A divisor (the depth Z, a norm n) keeps its true
fp64 value: a quotient's terms are bounded from a lower bound of the divisor, not from an upper one.  The inputs keep the
divisors well conditioned (Z >= 5 against |R| |p| + |t| <= 2.5 Z, so a rounding of Z moves a quotient by a few 1e-7 of itself).

Cases: projection and transform at P in {1, 255, 256, 257, 10475} x B in {1, 3, 70} (GT = 256 threads per body; 10475 is the
real vertex count), projection with and without rotation / translation and with unequal focal lengths, every subset of the
output pointers; rot6d at n in {1, 256, 257, 22 x 64} with rows under the first clamp, under the second clamp (a2 an exact
multiple of a1, a2 = 0, |u| = 1e-13) asserted apart from the regular rows.  Nothing of the issue's list was trimmed."""
import itertools

import pytest
import torch

from grad_shapes_util import Arena, check, report

pytestmark = pytest.mark.gpu
FOCAL = (5000.0, 4000.0)
PS, BS = (1, 255, 256, 257, 10475), (1, 3, 70)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _libs(dev):
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    return N, G, G.lib(), N.stream_ptr(dev)


def _rotations(B, gen, scale):
    from oracle import smplx_ref
    return smplx_ref.batch_rodrigues(torch.randn(B, 3, generator=gen, dtype=torch.float64) * scale).float()


# ------------------------------------------------------------------------------------------------ projection
def _proj_case(B, P, with_rt, seed):
    gen = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, P, 3, generator=gen) * 0.5         # a body's scale, ten units in front of the camera
    if with_rt:
        rot, tr = _rotations(B, gen, 0.3), torch.randn(B, 3, generator=gen) * 0.2 + torch.tensor([0., 0., 10.])
    else:                                                    # the caller's form: points already in the camera frame
        pts = pts + torch.tensor([0., 0., 10.])
        rot = tr = None
    return pts, rot, tr, torch.randn(B, P, 2, generator=gen)


def _proj_ref(pts, rot, tr, g):
    """fp64 autograd through the oracle -> (gpts, gR, gt, gc), and the bound A of each"""
    from oracle import geometry_ref
    B = pts.shape[0]
    p = pts.double().requires_grad_(True)
    R = (torch.eye(3, dtype=torch.float64).expand(B, 3, 3).clone() if rot is None else rot.double()).requires_grad_(True)
    t = (torch.zeros(B, 3, dtype=torch.float64) if tr is None else tr.double()).requires_grad_(True)
    c = torch.zeros(B, 2, dtype=torch.float64).requires_grad_(True)
    (geometry_ref.perspective_projection(p, R, t, FOCAL, c) * g.double()).sum().backward()
    ref = {"gpts": p.grad, "gR": R.grad, "gt": t.grad, "gc": c.grad}
    Ra, pa, ga = R.detach().abs(), pts.double().abs(), g.double().abs()
    cam = torch.einsum("bij,bkj->bki", R.detach(), pts.double()) + t.detach().unsqueeze(1)
    cama = torch.einsum("bij,bkj->bki", Ra, pa) + t.detach().abs().unsqueeze(1)
    Z = cam[..., 2].abs()
    assert float(Z.min()) > 5.0 and float((cama[..., 2] / Z).max()) < 2.5, "the case's depths are not well conditioned"
    gv = torch.stack([FOCAL[0] * ga[..., 0] / Z, FOCAL[1] * ga[..., 1] / Z,
                      (FOCAL[0] * ga[..., 0] * cama[..., 0] + FOCAL[1] * ga[..., 1] * cama[..., 1]) / (Z * Z)], -1)
    A = {"gpts": torch.einsum("bji,bkj->bki", Ra, gv), "gR": torch.einsum("bki,bkj->bij", gv, pa), "gt": gv.sum(1), "gc": ga.sum(1)}
    return ref, A


def _run_projection(dev, case, ref, A, outs, what, ratios):
    N, G, L, s = _libs(dev)
    pts, rot, tr, g = case
    B, P = pts.shape[:2]
    d = [None if t is None else t.to(dev) for t in case]
    runs = []
    for _ in range(2):
        a = Arena(dev, {"gpts": (B, P, 3), "gR": (B, 3, 3), "gt": (B, 3), "gc": (B, 2)})
        G.check(L.apg_perspective_projection_bwd(N.dptr(d[0]), B, P, N.dptr(d[1]), N.dptr(d[2]), FOCAL[0], FOCAL[1], N.dptr(d[3]),
                                                 *[N.dptr(a[k]) if k in outs else None for k in a.names], s),
                "apg_perspective_projection_bwd")
        torch.cuda.synchronize()
        a.untouched(outs, what)
        runs.append(a)
    for k in outs:
        assert torch.equal(runs[0][k], runs[1][k]), (what, k, "two identical calls differ")
        check(what, k, runs[0][k], ref[k], A[k], ratios)


@pytest.mark.parametrize("with_rt", [True, False], ids=["Rt", "noRt"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("P", PS)
def test_projection_sizes(dev, P, B, with_rt):
    case = _proj_case(B, P, with_rt, seed=1000 * B + P + int(with_rt))
    ref, A = _proj_ref(*case)
    ratios = {}
    if with_rt:
        _run_projection(dev, case, ref, A, ("gpts", "gR", "gt", "gc"), (B, P, "Rt"), ratios)
    else:                                                    # what the wrapper can ask for without rotation / translation
        for outs in (("gpts",), ("gpts", "gc"), ("gc",)):
            _run_projection(dev, case, ref, A, outs, (B, P, "noRt", outs), ratios)
    report("projection B=%d P=%d %s" % (B, P, "R,t" if with_rt else "NULL R,t"), ratios)


@pytest.mark.parametrize("B,P", [(3, 257), (2, 10475)])
def test_projection_every_output_subset(dev, B, P):
    """the 15 non-empty subsets of (g_pts, g_rotation, g_translation, g_center): the needs_input_grad patterns of the wrapper,
    g_pts NULL among them"""
    case = _proj_case(B, P, True, seed=77 + P)
    ref, A = _proj_ref(*case)
    ratios = {}
    names = ("gpts", "gR", "gt", "gc")
    for k in range(1, 5):
        for outs in itertools.combinations(names, k):
            _run_projection(dev, case, ref, A, outs, (B, P, outs), ratios)
    report("projection B=%d P=%d, 15 output subsets" % (B, P), ratios)


# ------------------------------------------------------------------------------------------------ transform
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("P", PS)
def test_transform_sizes_and_null_outputs(dev, P, B):
    from oracle import geometry_ref
    N, G, L, s = _libs(dev)
    gen = torch.Generator().manual_seed(2000 * B + P)
    rt = torch.cat([_rotations(B, gen, 1.0), torch.randn(B, 3, 1, generator=gen)], 2).contiguous()
    pts, g = torch.randn(B, P, 3, generator=gen), torch.randn(B, P, 3, generator=gen)
    M, p = rt.double().requires_grad_(True), pts.double().requires_grad_(True)
    (geometry_ref.transform_smpl(M, p)[0] * g.double()).sum().backward()
    ref = {"grt": M.grad, "gpts": p.grad}
    ga, pa = g.double().abs(), pts.double().abs()
    A = {"grt": torch.cat([torch.einsum("bki,bkj->bij", ga, pa), ga.sum(1).unsqueeze(2)], 2),
         "gpts": torch.einsum("bji,bkj->bki", rt.double().abs()[:, :, :3], ga)}
    rtd, pd, gd = rt.to(dev), pts.to(dev), g.to(dev)
    ratios = {}
    for outs in (("grt", "gpts"), ("gpts",), ("grt",)):      # g_rt NULL: the kernel's early return
        runs = []
        for _ in range(2):
            a = Arena(dev, {"grt": (B, 3, 4), "gpts": (B, P, 3)})
            G.check(L.apg_transform_points_bwd(N.dptr(rtd), N.dptr(pd), B, P, N.dptr(gd), *[N.dptr(a[k]) if k in outs else None
                                                                                          for k in a.names], s),
                    "apg_transform_points_bwd")
            torch.cuda.synchronize()
            a.untouched(outs, (B, P, outs))
            runs.append(a)
        for k in outs:
            assert torch.equal(runs[0][k], runs[1][k]), (B, P, outs, k, "two identical calls differ")
            check((B, P, outs), k, runs[0][k], ref[k], A[k], ratios)
    report("transform B=%d P=%d" % (B, P), ratios)


# ------------------------------------------------------------------------------------------------ rot6d
def _special_rows(gen):
    """(a1, a2) rows by branch.  clamp1: a1 under F.normalize's clamp.  The second clamp needs u = a2 - (b1 . a2) b1 under 1e-12 in
    fp32 AND fp64, which rounding denies a generic parallel pair (u ~ 1e-7 |a2| in fp32), so a1 lies on an axis with a
    power-of-two length: b1 and d are exact and u is exactly the part of a2 off that axis."""
    r = lambda: torch.randn(3, generator=gen)
    e = lambda k, s: torch.eye(3)[k] * s
    return {
        "clamp1": [(r() * 1e-14, r()), (r() * 1e-14, r())],
        "clamp2 multiple": [(e(0, 2.0), e(0, 3.0)), (e(1, 4.0), e(1, -8.0)), (e(2, 0.5), e(2, 0.5))],
        "clamp2 a2=0": [(r(), torch.zeros(3)), (e(1, 1.0), torch.zeros(3))],
        "clamp2 |u|=1e-13": [(e(0, 1.0), torch.tensor([0.7, 1e-13, 0.0])), (e(2, 2.0), torch.tensor([6e-14, -8e-14, 1.5]))],
    }


def _rot6d_A(x, g):
    """the adjoint of rot6d_bwd_kernel on absolute values, divisors (the clamped norms) at their true values"""
    x, g = x.double().reshape(-1, 3, 2), g.double().abs()
    a1, a2 = x[:, :, 0], x[:, :, 1]
    n1 = a1.norm(dim=1, keepdim=True).clamp_min(1e-12)
    b1 = a1 / n1
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    n2 = u.norm(dim=1, keepdim=True).clamp_min(1e-12)
    c1, c2 = (a1.norm(dim=1, keepdim=True) > 1e-12).double(), (u.norm(dim=1, keepdim=True) > 1e-12).double()
    b1a, a2a = b1.abs(), a2.abs()
    da = (b1a * a2a).sum(1, keepdim=True)
    b2a = (a2a + da * b1a) / n2
    cross = lambda p, q: torch.stack([p[:, 1] * q[:, 2] + p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] + p[:, 0] * q[:, 2],
                                      p[:, 0] * q[:, 1] + p[:, 1] * q[:, 0]], 1)
    gb1, gb2, gb3 = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    gb1 = gb1 + cross(b2a, gb3)
    gb2 = gb2 + cross(gb3, b1a)
    gu = (gb2 + c2 * b2a * (b2a * gb2).sum(1, keepdim=True)) / n2
    gd = (gu * b1a).sum(1, keepdim=True)
    gb1 = gb1 + da * gu + gd * a2a
    ga2 = gu + gd * b1a
    ga1 = (gb1 + c1 * b1a * (b1a * gb1).sum(1, keepdim=True)) / n1
    return torch.stack([ga1, ga2], 2).reshape(-1, 6)


@pytest.mark.parametrize("n", [1, 256, 257, 22 * 64])
def test_rot6d_sizes_and_both_clamps(dev, n):
    from oracle import geometry_ref
    N, G, L, s = _libs(dev)
    gen = torch.Generator().manual_seed(300 + n)
    special = _special_rows(gen)
    rows = [(kind, a1, a2) for kind, lst in special.items() for a1, a2 in lst]
    variants = [None] + rows if n == 1 else [rows]           # n = 1: a regular row, then each special row on its own
    ratios = {}
    for var in variants:
        x = torch.randn(n, 6, generator=gen)
        kind_of = ["regular"] * n
        if var is not None:
            put = [var] if n == 1 else var
            # the special rows go to the front and, in reverse, to the back (the ragged tail of the last block)
            where = [0] if n == 1 else list(range(len(put))) + [n - 1 - i for i in range(len(put))]
            for i, r in enumerate(where):
                kind, a1, a2 = put[i % len(put)]
                x[r, 0::2], x[r, 1::2] = a1, a2
                kind_of[r] = kind
        g = torch.randn(n, 3, 3, generator=gen)
        x64 = x.double().requires_grad_(True)
        (geometry_ref.rot6d_to_rotmat(x64) * g.double()).sum().backward()
        ref, A = x64.grad, _rot6d_A(x, g)
        assert torch.isfinite(ref).all()
        xd, gd = x.to(dev), g.to(dev)
        runs = []
        for _ in range(2):
            a = Arena(dev, {"gx": (n, 6)})
            G.check(L.apg_rot6d_to_rotmat_bwd(N.dptr(xd), n, N.dptr(gd), N.dptr(a["gx"]), s), "apg_rot6d_to_rotmat_bwd")
            torch.cuda.synchronize()
            a.untouched(("gx",), n)
            runs.append(a)
        assert torch.equal(runs[0]["gx"], runs[1]["gx"]), (n, "two identical calls differ")
        got = runs[0]["gx"].cpu()
        for kind in sorted(set(kind_of)):                    # each branch apart: the clamped rows are 1e12 times the others
            idx = torch.tensor([i for i, k in enumerate(kind_of) if k == kind])
            check((n, kind), kind, got[idx], ref[idx], A[idx], ratios)
            if kind != "regular":
                assert float(got[idx].abs().max()) > 1e6, (n, kind, "the clamp branch was not taken (g / 1e-12)")
    report("rot6d n=%d" % n, ratios)
