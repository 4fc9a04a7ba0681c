"""Element-wise fp64 ground truth for apg_seq_init and apg_seq_export (airpose_amd/csrc/seq_fit.hip) through the C ABI.  Companion of
test_fit_fp64.py; Buf is loss_util's, evaluate() is test_stem_pool_fp64's, the reference and the inputs live in seq_util.py.

Bar.  Continuous outputs (z, phi; thetas, root_rot, smpl_wrt_cam, cam1_wrt_cam0): |got - ref| <= tol (|ref| + S), S = the largest |ref|
of the element's row (the last dimension: a frame's 32 latents, 6 rotation entries, 63 pose entries, a matrix row); where |ref| + S = 0
the output must be exactly 0.  tol = 8 x FP32_RATIO[kind]: the worst |fp32 - fp64| / (|ref| + S) of the SAME reference formulae
evaluated in torch float32 on the CPU over every case of this file (measured on the CPU, never on the kernel;
test_cpu_fp32_ratios_behind_tol re-measures them).  The factor 8 is for sinf / cosf / atan2f of the GPU against the CPU's, fused
multiply-adds and the order of the additions, as in test_fit_fp64.py.

    kind            fp32 ratio   tol
    z               4.8e-07      3.8e-06     (the unfolded encoder in fp32; the kernel runs the fp64-folded one)
    phi             1.7e-07      1.4e-06
    thetas          1.1e-07      8.8e-07
    root_rot        1.0e-07      8.0e-07
    smpl_wrt_cam    5.3e-08      4.2e-07     (a row's S is its translation entry, metres)
    cam1_wrt_cam0   1.6e-06      1.3e-05     (the reference's general inverse in fp32)

tau, and x and y of j2d, are copies: bit for bit.  The filtered confidences and robust are discrete: equal, the inputs being chosen so
that fp32 and fp64 cannot disagree (test_cpu_input_conditions): every detector distance is at least 1e-3 px from 100 or exactly 100 on
integer coordinates ((dx, dy) = (60, 80), which is kept), every confidence sum at least 1e-3 from 14 or exactly 14 on multiples of
0.25 (not robust), every root angle exactly 0 or in [0.05, 3.0] rad, and the decoders hold fit_util.branch_report's margins.

Shapes: L in seq_util.SIZES = {1, 2, 3, R - 1, R, R + 1, 2 R + 1, 33} with R = APG_SEQ_ROWS frames per workgroup; frame 0 carries the
(60, 80) edge, frame 1 has angles = 0, frame 2 all confidences 0, frame 3 AlphaPose confidences summing to exactly 14.  Seeds:
seq_util.INIT_SEED + L, EXPORT_SEED, VPOSER_SEED.  Every GPU call writes into NaN-filled buffers between NaN guard bands, runs twice and
must give the same bits.

Mutations (test_cpu_mutations_are_rejected): each deliberate error of seq_util.INIT_MUTATIONS / EXPORT_MUTATIONS in the fp64
reference misses the bar or the exact match in at least one case; none is undetectable.
"""
import ctypes

import pytest
import torch

import seq_util as U
from loss_util import Buf, dev  # noqa: F401  (dev: the fixture of the GPU tests)
from test_stem_pool_fp64 import evaluate

FP32_RATIO = {"z": 4.8e-07, "phi": 1.7e-07, "thetas": 1.1e-07, "root_rot": 1.0e-07, "smpl_wrt_cam": 5.3e-08, "cam1_wrt_cam0": 1.6e-06}
TOL = {k: 8.0 * v for k, v in FP32_RATIO.items()}
UNDETECTABLE = ()


def init_cases():
    return [U.init_case(L) for L in U.SIZES]


def export_cases():
    return [U.export_case(L, dec) for L in U.SIZES for dec in U.DECODERS]


def verify(got, ref, kinds, what, worst=None):
    fails = []
    for k in kinds:
        ok, r, _, msg = evaluate(got[k], ref[k], TOL[k] * U.scale(ref[k]))
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r * TOL[k])
        if not ok:
            fails.append((what, k, msg))
    return fails


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("L", U.SIZES)
def test_cpu_input_conditions(L):
    c = U.init_case(L)
    assert all(torch.equal(v, v.float().double()) for v in c.values())
    det = c["det"]
    d = det[:, :, 0, :, :2] - det[:, :, 1, :, :2]
    dist = torch.sqrt((d * d).sum(-1))
    on_edge = dist == U.AGREEMENT_PX
    assert ((dist - U.AGREEMENT_PX).abs() >= 1e-3)[~on_edge].all()
    assert bool(on_edge[1, U.FRAME_EDGE, 5]) and int(on_edge.sum()) == 1
    assert torch.equal(d[1, U.FRAME_EDGE, 5], torch.tensor([60.0, 80.0], dtype=torch.float64))
    ints = det[:, :, :, :, :2][on_edge.unsqueeze(2).expand(2, L, 2, 24)]
    assert torch.equal(ints, ints.round())                   # exact in fp32 and fp64 alike
    ref = U.ref_init(c)
    assert float(ref["j2d"][1, U.FRAME_EDGE, 1, 5, 2]) == float(det[1, U.FRAME_EDGE, 1, 5, 2]) > 0      # kept
    s = ref["j2d"][:, :, 1, :, 2].sum((0, 2))
    on14 = s == U.ROBUST_CONF
    assert ((s - U.ROBUST_CONF).abs() >= 1e-3)[~on14].all()
    if L > U.FRAME_EXACT_14:
        q = ref["j2d"][:, U.FRAME_EXACT_14, 1, :, 2]
        assert bool(on14[U.FRAME_EXACT_14]) and int(on14.sum()) == 1 and torch.equal(q * 4, (q * 4).round())
        assert int(ref["robust"][U.FRAME_EXACT_14]) == 0
    else:
        assert not on14.any()
    if L > U.FRAME_ZERO_CONF:
        assert not det[:, U.FRAME_ZERO_CONF, :, :, 2].any() and int(ref["robust"][U.FRAME_ZERO_CONF]) == 0
    if L >= 9:
        assert 0 < int(ref["robust"].sum()) < L              # both outcomes
    zeroed = (ref["j2d"][..., 2] == 0) & (det[..., 2] != 0)
    assert zeroed.any() and torch.equal(zeroed[:, :, 0], zeroed[:, :, 1])
    for v in (0, 1):
        ang = c["angles%d" % v][:, 0].norm(dim=1)
        assert (((ang >= 0.05) & (ang <= 3.0)) | (ang == 0)).all()
        if L > U.FRAME_ZERO_ANGLES:
            assert not c["angles%d" % v][U.FRAME_ZERO_ANGLES].any()
            assert torch.equal(ref["phi"][v, U.FRAME_ZERO_ANGLES], torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64))
    print("L %2d seed %d: distances >= %.3g from 100, sums >= %.3g from 14, %d of %d frames robust" % (
        L, U.init_seed(L), float((dist - 100).abs()[~on_edge].min()), float((s - 14).abs()[~on14].min()) if (~on14).any() else -1,
        int(ref["robust"].sum()), L))
    for dec in U.DECODERS:
        vp, prm = U.export_case(L, dec)
        rep = U.FU.branch_report(vp, prm["z"])
        assert rep["t"].min() >= 0.5 and rep["d22"].min() >= 0.05 and rep["d2"].min() >= 0.05, (L, dec)
        assert all(torch.equal(v, v.float().double()) for v in list(vp.values()) + list(prm.values()))


def test_cpu_fold_agrees_with_the_unfolded_encoder():
    """loss_real.fold_encoder's first 32 rows against the layer-by-layer encoder, fp64"""
    from airpose_amd.loss_real import fold_encoder
    W1, b1, W2, b2 = fold_encoder(U.state_dict(U.export_case(3, "body")[0]))
    x = U.init_case(9)["angles0"][:, 1:22].reshape(9, 63)
    z = torch.nn.functional.leaky_relu(x @ W1.t() + b1, 0.01) @ W2[:32].t() + b2[:32]
    assert U.ratio(z, U.encode_mean(U.encoder_state(), x)) < 1e-13


def measure_fp32_ratios():
    worst = {}
    for c in init_cases():
        ref, f32 = U.ref_init(c), U.ref_init(c, torch.float32)
        assert not U.exact(f32, ref, ("robust",)) and torch.equal(f32["j2d"][..., 2].double(), ref["j2d"][..., 2])
        for k in U.INIT_KINDS:
            worst[k] = max(worst.get(k, 0.0), U.ratio(f32[k], ref[k]))
    for vp, prm in export_cases():
        ref, f32 = U.ref_export(vp, prm), U.ref_export(vp, prm, torch.float32)
        for k in U.EXPORT_KINDS:
            worst[k] = max(worst.get(k, 0.0), U.ratio(f32[k], ref[k]))
    return worst


def test_cpu_fp32_ratios_behind_tol():
    """the reference in torch float32 against itself in fp64 over every case of this file: per kind this CPU's worst ratio is at
    least a third of the recorded FP32_RATIO, so tol is never wider than 24 x the fp32 arithmetic's own error here (only that side
    is asserted, as in test_fit_fp64.py).  The figures are printed."""
    worst = measure_fp32_ratios()
    print("  ".join("%s %.2e" % (k, v) for k, v in worst.items()))
    assert sorted(worst) == sorted(FP32_RATIO)
    for k, v in worst.items():
        assert v >= FP32_RATIO[k] / 3, (k, v, FP32_RATIO[k])


@pytest.mark.parametrize("mut", U.INIT_MUTATIONS + U.EXPORT_MUTATIONS)
def test_cpu_mutations_are_rejected(mut):
    fails, worst = [], {}
    if mut in U.INIT_MUTATIONS:
        for L in (U.R, 2 * U.R + 1):
            c = U.init_case(L)
            got, ref = U.ref_init(c, mut=mut), U.ref_init(c)
            fails += verify(got, ref, U.INIT_KINDS, (L,), worst)
            fails += [((L,), k, "differs") for k in U.exact(got, ref, ("tau", "j2d", "robust"))]
    else:
        for L in (3, U.R + 1):
            vp, prm = U.export_case(L, "body")
            fails += verify(U.ref_export(vp, prm, mut=mut), U.ref_export(vp, prm), U.EXPORT_KINDS, (L,), worst)
    print("%-24s worst |err| / (|ref| + S): %s; misses: %s" % (mut, "  ".join("%s %.1e" % kv for kv in worst.items()),
                                                               sorted({f[1] for f in fails})))
    if mut in UNDETECTABLE:
        assert not fails
        return
    kinds = {f[1] for f in fails}
    want = dict(sixd_from_columns="phi", logvar_rows="z", encoder_on_view1="z", bn_eps_dropped="z", agreement_ge="j2d", robust_ge="robust",
                filter_one_detector="j2d", mask_from_openpose="robust", t1_t0inv="cam1_wrt_cam0", inverse_minus_R_t="cam1_wrt_cam0")[mut]
    assert want in kinds, (mut, sorted(kinds))
    if mut in ("agreement_ge", "robust_ge"):                 # caught by the representable edge alone
        assert kinds <= {"j2d", "robust"}


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if WORST:
        print("\ntest_seq_fp64 GPU worst |err| / (|ref| + S) [tol]: %s" % "  ".join("%s %.2e [%.2e]" % (k, WORST[k], TOL[k]) for k in WORST))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def run_init(dev, L):
    """one apg_seq_init on NaN-guarded buffers -> the outputs as cpu tensors"""
    from airpose_amd import _native_grad as G
    from airpose_amd.loss_real import fold_encoder
    c = U.init_case(L)
    W1, b1, W2, b2 = fold_encoder(U.state_dict(U.export_case(3, "body")[0]))
    enc = [t.float().contiguous().to(dev) for t in (W1, b1, W2[:32], b2[:32])]
    inp = {k: v.float().contiguous().to(dev) for k, v in c.items()}
    sizes = dict(z=L * 32, phi=2 * L * 6, tau=2 * L * 3, j2d=2 * L * 2 * 24 * 3, robust=L)
    bufs = {k: Buf(dev, n) for k, n in sizes.items()}
    G.check(G.lib().apg_seq_init(L, _p(inp["angles0"]), _p(inp["angles1"]), _p(inp["trans0"]), _p(inp["trans1"]), _p(inp["det"]),
                                 *[_p(t) for t in enc], U.AGREEMENT_PX, U.ROBUST_CONF, _p(bufs["z"].out), _p(bufs["phi"].out),
                                 _p(bufs["tau"].out), _p(bufs["j2d"].out), _p(bufs["robust"].out), G.stream(dev)), "apg_seq_init")
    torch.cuda.current_stream(dev).synchronize()
    what = ("init", L)
    out = dict(z=bufs["z"].values((L, 32), what), phi=bufs["phi"].values((2, L, 6), what), tau=bufs["tau"].values((2, L, 3), what),
               j2d=bufs["j2d"].values((2, L, 2, 24, 3), what))
    out["robust"] = bufs["robust"].values((L,), what).view(torch.int32)      # (0 and 1 as int32 bits are no NaN)
    return out


def run_export(dev, L, decoder):
    from airpose_amd import _native_grad as G
    vp, prm = U.export_case(L, decoder)
    f = lambda t: t.float().contiguous().to(dev)
    w = [f(vp[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    z, phi, tau = f(prm["z"]), f(torch.stack([prm["phi0"], prm["phi1"]])), f(torch.stack([prm["tau0"], prm["tau1"]]))
    sizes = dict(thetas=L * 63, root_rot=2 * L * 9, smpl_wrt_cam=2 * L * 16, cam1_wrt_cam0=L * 16)
    bufs = {k: Buf(dev, n) for k, n in sizes.items()}
    G.check(G.lib().apg_seq_export(L, _p(z), _p(phi), _p(tau), *[_p(t) for t in w], _p(bufs["thetas"].out), _p(bufs["root_rot"].out),
                                   _p(bufs["smpl_wrt_cam"].out), _p(bufs["cam1_wrt_cam0"].out), G.stream(dev)), "apg_seq_export")
    torch.cuda.current_stream(dev).synchronize()
    what = ("export", L, decoder)
    return dict(thetas=bufs["thetas"].values((L, 63), what), root_rot=bufs["root_rot"].values((2, L, 3, 3), what),
                smpl_wrt_cam=bufs["smpl_wrt_cam"].values((2, L, 4, 4), what), cam1_wrt_cam0=bufs["cam1_wrt_cam0"].values((L, 4, 4), what))


def bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("L", U.SIZES)
def test_init_against_fp64(dev, L):
    got, again = run_init(dev, L), run_init(dev, L)
    assert bits_equal(got, again), (L, "two runs differ")
    ref = U.ref_init(U.init_case(L))
    fails = verify(got, ref, U.INIT_KINDS, ("init", L), WORST)
    assert not fails, fails[:5]
    assert not U.exact(got, ref, ("tau", "j2d", "robust")), (L, U.exact(got, ref, ("tau", "j2d", "robust")))
    if L > U.FRAME_ZERO_ANGLES:                              # r = 0: the identity exactly
        want = torch.tensor([1.0, 0, 0, 0, 1.0, 0])
        assert all(torch.equal(got["phi"][v, U.FRAME_ZERO_ANGLES].view(torch.int32), want.view(torch.int32)) for v in (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("L", U.SIZES)
def test_export_against_fp64(dev, L):
    for dec in U.DECODERS:
        got, again = run_export(dev, L, dec), run_export(dev, L, dec)
        assert bits_equal(got, again), (L, dec, "two runs differ")
        vp, prm = U.export_case(L, dec)
        ref = U.ref_export(vp, prm)
        fails = verify(got, ref, U.EXPORT_KINDS, ("export", L, dec), WORST)
        assert not fails, fails[:5]
        # the copies inside the 4 x 4s and their constant row, exactly
        tau = torch.stack([prm["tau0"], prm["tau1"]]).float()
        assert torch.equal(got["smpl_wrt_cam"][:, :, :3, 3].view(torch.int32), tau.view(torch.int32))
        assert torch.equal(got["smpl_wrt_cam"][:, :, :3, :3].view(torch.int32), got["root_rot"].view(torch.int32))
        bottom = torch.tensor([0.0, 0, 0, 1.0])
        assert (got["smpl_wrt_cam"][:, :, 3] == bottom).all() and (got["cam1_wrt_cam0"][:, 3] == bottom).all()
