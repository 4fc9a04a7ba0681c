"""Element-wise fp64 ground truth for the AirPose+ fitting loop (airpose_amd/csrc/fitting.hip, rot_aa.inc, api_fit.hip): fit_decode_kernel,
fit_frame_kernel, fit_adam_kernel and fit_backprop_adam_kernel through the C ABI (ap_fit_create / ap_fit_run).  Companion of
test_loss_fp64.py and test_optim_fp64.py; Buf is loss_util's, evaluate() is test_stem_pool_fp64's, the reference lives in fit_util.py.

Reference.  fit_util.ref_terms: the objective of oracle/fitting_ref.py from the oracle's own building blocks (vposer_decode,
body_joints, rotation_6d_to_matrix, geometry_ref.transform_smpl / perspective_projection) in fp64 on exactly the fp32 values the
kernel receives (the body as the handle holds it: fit_util.joint_model), with sigma and the weights as arguments, the per-frame parts
in the layout of the loss history, and the empty masks defined (no selected frame: the 2-D term is 0; no selected pair: the temporal
terms are 0 -- the reference script takes the mean of an empty set and gives NaN there; the kernel's zero contribution is the
contract).  Gradients by autograd.  fit_util.ref_fit: the loop with a plain Adam, a fresh state at first_iter and at switch_iter.

Bar.  For every gradient, per-frame loss part and updated parameter |got - ref| <= tol (|ref| + S), S = the largest |ref| of the
element's row (one frame's 32 values of z, 6 of phi, 3 of tau, 4 loss parts; beta's whole vector); where |ref| + S = 0 the output must
be exactly 0.  tol = 8 x FP32_RATIO[class][kind]: FP32_RATIO is the worst |fp32 - fp64| / (|ref| + S) of the SAME reference formulae
evaluated in torch float32 on the CPU over every case of this file (measured on the CPU, never on the kernel;
test_cpu_fp32_ratios_behind_tol re-measures them).  The factor 8 is for sinf / cosf / atan2f / powf of the GPU against the CPU's,
fused multiply-adds, and the kernel's order of additions (split-K decoder sums, wave reductions, LDS additions of the chain backward).
One value per output kind over ALL cases would be set by the few cases in which fp32 itself keeps the fewest digits, and be up to
50 times wider than the arithmetic of the others; so the cases are split into three classes (cls_of) with a value each, none wider
than the single one would be: "pairs" = gradient probes (lr = 0) whose mask selects a pair of neighbours; "nopair" = probes
without one (L = 1, the masks none and alternating: dphi and dtau are then the 2-D term's alone, sums that cancel); "steps" = calls
with lr > 0 (the rounding of one step moves the next step's gradient).

    fp32 ratio  dz       dphi     dtau     dbeta    loss     z        phi      tau      beta
    pairs       1.5e-6   4.7e-7   3.4e-7   4.1e-6   3.2e-7   (a probe's parameters come back bit for bit)
    nopair      1.2e-6   4.9e-6   2.9e-6   1.7e-6   2.6e-7
    steps       1.2e-6   2.2e-6   1.6e-5   4.3e-6   2.7e-6   2.1e-5   4.1e-8   5.4e-8   5.6e-6
    tol
    pairs       1.2e-5   3.8e-6   2.7e-6   3.3e-5   2.6e-6
    nopair      9.6e-6   3.9e-5   2.3e-5   1.4e-5   2.1e-6
    steps       9.6e-6   1.8e-5   1.3e-4   3.4e-5   2.2e-5   1.7e-4   3.3e-7   4.3e-7   4.5e-5

Exact zeros.  Besides the bar, every element whose reference is exactly 0 must be exactly 0: the gradients and loss parts of frames
that are not selected, the temporal parts of a selected frame whose predecessor is not (frame 0 always), column 3 of the history.

Inputs (fit_util.make_problem).  State, intrinsics, and the detections' noise and confidences of fitting_ref.synthetic_problem(L,
seed); view 1 looks through a rotated and translated camera, view 0 through the identity or a second pose (alternating over the
sizes); the decoder's last layer is scaled by 0.1 around seeded rotations: "body" (0.5 rad: matrot2aa's branch 3 only) and
"all-branch" (2.6 rad about axes near x, y, z and 0.6 .. 1.2 rad about a skew axis: each of the four branches at least five times in
every frame).  The detections sit around the projection of synthetic_problem's ground-truth motion through THIS decoder and THESE
cameras, so that the residuals of both views are of the order of sigma and not in the flat tail of Geman-McClure, where a wrong
adjoint hardly shows.  test_cpu_input_conditions checks for every (L, seed, decoder) used here: the chosen t >= 0.5, both
discriminants at least 0.05 from their thresholds (fp32 and fp64 then take the same branch), every projected joint deeper than 2 m,
the median residual of either view below 2 sigma.  The oracle's own random decoder (uniformly random rotations, some at 1 + trace =
1e-7) stays with the three test_fitting_* tests of test_gpu_parity.py at their whole-tensor bars.

Every GPU call holds z, phi, tau, beta, the loss history and the gradient in NaN-filled buffers between NaN guard bands, runs twice
and must give the same bits.  Before the switch the kernel leaves z and the dz segment of grad_out alone: z must come back bit for
bit, the segment must still hold its NaNs (AirPosePlusFitter.run hands out zeros there).

Mutations (test_cpu_mutations_are_rejected): each deliberate error of fit_util.MUTATIONS in the fp64 reference misses the bar in at
least one case -- but "rodrigues_eps_dropped" (angle = |r| instead of |r + 1e-8| on the 21 body joints), which changes the outputs by
1e-8 relative and is UNDETECTABLE at these bars; the test pins that it is below them.
"""
import collections
import ctypes
import functools

import pytest
import torch

import fit_util as U
from loss_util import Buf, dev  # noqa: F401  (dev: the fixture of the GPU tests)
from oracle import fitting_ref as Fr
from test_stem_pool_fp64 import evaluate

# worst fp32 / fp64 disagreement of the reference over the cases of this file, measured on the CPU, per class of call and output kind
FP32_RATIO = {
    "pairs": {"dz": 1.5e-06, "dphi": 4.7e-07, "dtau": 3.4e-07, "dbeta": 4.1e-06, "loss": 3.2e-07},
    "nopair": {"dz": 1.2e-06, "dphi": 4.9e-06, "dtau": 2.9e-06, "dbeta": 1.7e-06, "loss": 2.6e-07},
    "steps": {"dz": 1.2e-06, "dphi": 2.2e-06, "dtau": 1.6e-05, "dbeta": 4.3e-06, "loss": 2.7e-06, "z": 2.1e-05, "phi": 4.1e-08, "tau": 5.4e-08,
              "beta": 5.6e-06},
}
TOL = {c: {k: 8.0 * v for k, v in r.items()} for c, r in FP32_RATIO.items()}
UNDETECTABLE = ("rodrigues_eps_dropped",)

DECODERS = ("body", "all-branch")
PROBE_L = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33)               # L mod 4 = 0 .. 3; around the 16-frame beta batches; 50 L + 10 around 256
PROBE_IT = (0, 1, 23, 150)                                   # at 150 exp2f underflows: the hips weigh exactly nothing
MASK_L = (5, 9, 17)
MASKS = ("all", "none", "first_off", "last_off", "interior_off", "alternating", "odd_values")
ADAM_L = (3, 5)
ADAM_RUNS = ((0, 3, 2), (5, 3, 2), (1, 3, 3))                # (first_iter, n_iters, switch_iter)
HYPER = dict(sigma=12.5, w_vposer=0.3, w_temporal=2.5)
RESEED = {}                                                  # (L, decoder) -> seed, where the default seed broke a condition


def seed_of(L, decoder):
    return RESEED.get((L, decoder), 80)


def problem(L, decoder):
    return U.make_problem(L, seed_of(L, decoder), decoder, ("id", "rot")[PROBE_L.index(L) % 2])


# one ap_fit_run call; hyper: the hyper-parameters that differ from the defaults, as sorted (name, value) pairs
Spec = collections.namedtuple("Spec", "L decoder mask first_iter n_iters switch_iter lr hyper")


def spec(L, decoder, mask="all", first_iter=0, n_iters=1, switch_iter=0, lr=0.0, **hyper):
    return Spec(L, decoder, mask, first_iter, n_iters, switch_iter, lr, tuple(sorted(hyper.items())))


def probe_specs(L, decoder):
    return [spec(L, decoder, first_iter=it, switch_iter=sw) for it in PROBE_IT for sw in (0, it + 1)]


def mask_specs(L):
    return [spec(L, dec, mask=m, first_iter=1, switch_iter=sw) for dec in DECODERS for m in MASKS for sw in (0, 2)]


def hyper_specs():
    return [spec(7, dec, mask="interior_off", first_iter=1, switch_iter=sw, **HYPER) for dec in DECODERS for sw in (0, 2)]


def adam_specs(L):
    one = [spec(L, dec, mask="interior_off", switch_iter=sw, lr=0.01) for dec in DECODERS for sw in (0, 1)]
    return one + [spec(L, dec, first_iter=f, n_iters=n, switch_iter=sw, lr=0.01) for dec in DECODERS for f, n, sw in ADAM_RUNS]


def reuse_specs():
    return [spec(L, "all-branch", n_iters=3, switch_iter=1, lr=0.01) for L in (33, 5)]


def all_specs():
    out = [s for dec in DECODERS for L in PROBE_L for s in probe_specs(L, dec)]
    out += [s for L in MASK_L for s in mask_specs(L)] + hyper_specs() + [s for L in ADAM_L for s in adam_specs(L)] + reuse_specs()
    return out


@functools.lru_cache(maxsize=None)
def _reference(s, dtype):
    return U.ref_call(problem(s.L, s.decoder), U.mask(s.mask, s.L), first_iter=s.first_iter, n_iters=s.n_iters,
                      switch_iter=s.switch_iter, lr=s.lr, dtype=dtype, **dict(s.hyper))


def reference(s, dtype=torch.float64):
    """the call's expected outputs.  With lr = 0 nothing moves and the gradient does not depend on which optimiser is active: the
    two paths of a gradient probe share one evaluation (what the pre-switch path leaves unwritten is the caller's business)"""
    if s.lr == 0.0 and s.n_iters == 1:
        s = s._replace(switch_iter=0)
    return _reference(s, dtype)


def cls_of(s):
    """the class of a call, for its bar: "steps" if parameters move (lr > 0: the errors of one step feed the next), else "pairs" or
    "nopair" by whether the mask selects a pair of neighbours (without the temporal term, which otherwise carries most of dphi and
    dtau, the 2-D term's sums over joints, views and detectors cancel against each other and fp32 keeps fewer digits of them)"""
    if s.lr > 0:
        return "steps"
    m = U.mask(s.mask, s.L) != 0
    return "pairs" if bool((m[:-1] & m[1:]).any()) else "nopair"


def verify(got, ref, s, worst=None, skip=()):
    """every output kind of the call s against its bar -> list of failures; the worst |err| / (|ref| + S) per (class, kind) goes
    into worst"""
    fails, c = [], cls_of(s)
    for k in U.KINDS:
        if k in skip or (s.lr == 0 and k in ("z", "phi", "tau", "beta")):     # (a gradient probe's parameters: bit-equal to the input)
            continue
        ok, ratio, nz, msg = evaluate(got[k], ref[k], TOL[c][k] * U.scale(ref[k]))
        if worst is not None:
            worst[c, k] = max(worst.get((c, k), 0.0), ratio * TOL[c][k])
        if not ok:
            fails.append((tuple(s), k, msg))
    return fails


# ------------------------------------------------------------------------------------------------ CPU self-checks
def _close(a, b, rel=1e-11):
    return float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("L,it", [(5, 0), (8, 3)])
def test_cpu_ref_terms_agrees_with_the_oracle(L, it):
    """default hyper-parameters, a mask with a pair, the full body model: totals and gradients of fitting_ref to fp64 rounding"""
    model = U.full_model()
    vp, prm, data, _ = Fr.synthetic_problem(model, L=L, seed=91, dtype=torch.float64)
    data["robust"] = U.mask("interior_off", L) != 0
    total, want, parts = Fr.loss_and_grads(vp, model, prm, data, it)
    per_frame, tot = U.ref_terms(vp, model, prm, data, it)
    _, grads = U.ref_grads(vp, model, prm, data, it)
    assert _close(tot["total"], total) and _close(tot["loss_2d"], parts["loss_2d"].detach())
    assert _close(tot["loss_temporal_pose"] + tot["loss_temporal_rigid"], parts["loss_temporal"].detach())
    assert _close(per_frame.sum() + Fr.W_VPOSER * tot["loss_vposer"], total)
    assert not per_frame[L // 2].any() and not per_frame[:, 3].any() and not per_frame[0, 1:].any() and per_frame[1, 1:3].all()
    for k in U.KEYS:
        assert _close(grads[k], want[k]), k


def test_cpu_ref_fit_agrees_with_the_oracle_loop():
    """first_iter = 0: fitting_ref.fit (torch.optim.Adam, two instances) with SWITCH_ITER patched"""
    model = U.full_model()
    vp, prm, data, _ = Fr.synthetic_problem(model, L=5, seed=92, dtype=torch.float64)
    data["robust"] = U.mask("all", 5) != 0
    old = Fr.SWITCH_ITER
    Fr.SWITCH_ITER = 2
    try:
        want, losses = Fr.fit(vp, model, prm, data, n_iters=5)
    finally:
        Fr.SWITCH_ITER = old
    got, hist, _ = U.ref_fit(vp, model, prm, data, 0, 5, 2)
    for k in U.KEYS:
        assert _close(got[k], want[k]), k
    z2 = Fr.W_VPOSER * (prm["z"] ** 2).mean()                # z does not move before the switch
    assert abs(float(hist[0].sum() + z2) - losses[0]) <= 1e-11 * losses[0]


def test_cpu_empty_masks_give_zeros_not_nan():
    vp, prm, data = problem(5, "body")
    for m in ("none", "alternating"):
        parts, g = U.ref_grads(vp, U.joint_model(), prm, dict(data, robust=U.mask(m, 5)), 0)
        assert torch.isfinite(parts).all() and all(torch.isfinite(v).all() for v in g.values())
        assert not parts[:, 1:].any() and (m == "alternating") == bool(parts[:, 0].any())
        assert g["z"].abs().min() > 0                        # (the prior's gradient is always there)
        assert (m == "alternating") == bool(g["beta"].any())


@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("L", PROBE_L)
def test_cpu_input_conditions(L, decoder):
    prob = problem(L, decoder)
    vp, prm, data = prob
    for d in (vp, prm, data):
        assert all(torch.equal(v, v.float().double()) for v in d.values() if v.is_floating_point())   # fp32 values
    rep = U.branch_report(vp, prm["z"])
    print("L %2d %-10s seed %d: t >= %.3f, |aa| <= %.3f, d22 >= %.3f, d2 >= %.3f, depth >= %.2f" % (
        L, decoder, seed_of(L, decoder), rep["t"].min(), rep["angle"].max(), rep["d22"].min(), rep["d2"].min(), U.depths(prob).min()))
    assert rep["t"].min() >= 0.5 and rep["d22"].min() >= 0.05 and rep["d2"].min() >= 0.05
    assert U.depths(prob).min() > 2.0
    res = U.residuals(prob)                                  # (2 views, L, 2 detectors, 24, 2) pixels at the initial state
    assert all(float(res[v].abs().median()) < 2 * Fr.GM_SIGMA for v in (0, 1)), [float(res[v].abs().median()) for v in (0, 1)]
    counts = torch.stack([(rep["branch"] == b).sum(1) for b in range(4)], 1)                          # (L, 4)
    if decoder == "body":
        assert not counts[:, :3].any()
    else:
        assert counts.min() >= 5
    E = data["extr"]
    assert (E[1, :, :3] - torch.eye(3, dtype=E.dtype)).abs().max() > 0.1 and E[1, :, 3].abs().min() > 0.1
    assert _close(E[:, :, :3] @ E[:, :, :3].transpose(1, 2), torch.eye(3, dtype=E.dtype).expand(2, 3, 3), 1e-6)


def measure_fp32_ratios():
    """worst |fp32 - fp64| / (|ref| + S) of the reference itself per (class, kind) over all_specs(), with the case that has it"""
    worst = {}
    for s in sorted(set(all_specs())):
        c = cls_of(s)
        for k, v in U.ratios(reference(s, torch.float32), reference(s)).items():
            if (s.lr > 0 or k not in ("z", "phi", "tau", "beta")) and v >= worst.get((c, k), (0.0, None))[0]:
                worst[c, k] = (v, s)
    return worst


def test_cpu_fp32_ratios_behind_tol():
    """The reference in torch float32 against itself in fp64 over every case of this file: per (class, kind) this CPU's worst ratio
    is at least a third of the recorded FP32_RATIO, so that tol is never wider than 24 x the fp32 arithmetic's own error on the
    machine that runs the test.  Only that side is asserted: a CPU that measures MORE than the record finds tol tighter than 8 x
    its own error, which weakens no check.  The worst of a few thousand elements depends on the order of additions inside torch's
    fp32 matrix products; in the class "steps" it is set by single elements whose gradient nearly vanishes at a fresh Adam step
    (the step lr g / (|g| + 1e-8) then amplifies the gradient's rounding), and there another CPU has measured three times the
    record.  The figures are printed."""
    worst = measure_fp32_ratios()
    for c in FP32_RATIO:
        print("%-7s %s" % (c, "  ".join("%s %.2e" % (k, worst[c, k][0]) for k in U.KINDS if (c, k) in worst)))
    assert sorted(worst) == sorted((c, k) for c in FP32_RATIO for k in FP32_RATIO[c])
    for (c, k), (v, s) in worst.items():
        assert v >= FP32_RATIO[c][k] / 3, (c, k, v, FP32_RATIO[c][k], tuple(s))


MUTATION_SPECS = [spec(5, "all-branch", first_iter=0), spec(5, "body", mask="interior_off", first_iter=1),
                  spec(3, "body", first_iter=0, n_iters=3, switch_iter=2, lr=0.01)]


@pytest.mark.parametrize("mut", U.MUTATIONS)
def test_cpu_mutations_are_rejected(mut):
    fails, worst = [], {}
    for s in MUTATION_SPECS:
        got = U.ref_call(problem(s.L, s.decoder), U.mask(s.mask, s.L), first_iter=s.first_iter, n_iters=s.n_iters,
                         switch_iter=s.switch_iter, lr=s.lr, mut=mut, **dict(s.hyper))
        fails += verify(got, reference(s), s, worst)
    print("%-32s worst |err| / (|ref| + S): %s" % (mut, "  ".join("%s %s %.1e" % (c, k, v) for (c, k), v in worst.items())))
    if mut in UNDETECTABLE:
        assert not fails, "%s is listed as undetectable but misses a bar: move it out of UNDETECTABLE" % mut
        return
    assert fails, "the bars accept the mutation %s" % mut
    kinds = {f[1] for f in fails}
    want = dict(extr_transposed="dphi", extr_translation_dropped="dphi", intr_swapped="dtau", hip_weight_one_step_late="loss",
                pair_accounted_to_first_frame="loss", pairs_plus_one="dtau", leaky_slope_zero_in_backward="dz",
                adam_counter_not_restarted="phi", prior_divided_by_L="dz")[mut]
    assert want in kinds, (mut, sorted(kinds))
    if mut == "pair_accounted_to_first_frame":
        assert kinds == {"loss"}                              # the history's accounting alone


def test_cpu_binding_has_the_entries():
    from airpose_amd import _native as N
    assert all(n in N.SIGNATURES for n in ("ap_fit_create", "ap_fit_run", "ap_fit_destroy"))


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
WORST = {}                                                   # worst |err| / (|ref| + S) per kind over the GPU tests of this run


@pytest.fixture(scope="module")
def body(dev):
    from airpose_amd import smplx
    return smplx.SMPLX(model_data=U.full_model())


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if WORST:
        for c in TOL:
            print("\ntest_fit_fp64 GPU %-6s worst |err| / (|ref| + S) [tol]: %s" % (
                c, "  ".join("%s %.2e [%.2e]" % (k, WORST[c, k], TOL[c][k]) for k in U.KINDS if (c, k) in WORST)))


class Fitter(object):
    """an ap_fit handle on the raw ABI"""

    def __init__(self, dev, vp, body):
        from airpose_amd import _native as N
        self.N, self.dev, self.h = N, dev, ctypes.c_void_p()
        w = [vp[k].float().contiguous() for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
        N.check(N.lib().ap_fit_create(ctypes.byref(self.h), body._native(dev), *[ctypes.c_void_p(t.data_ptr()) for t in w],
                                      dev.index or 0), "ap_fit_create")

    def close(self):
        h, self.h = self.h, None
        if h:
            self.N.lib().ap_fit_destroy(h)

    def run(self, s):
        """one ap_fit_run -> the outputs as cpu fp32: z (L,32), phi (2,L,6), tau (2,L,3), beta (10,), loss (n_iters,L,4), and the
        gradient vector split into dz, dphi, dtau, dbeta; "dz_written" says whether the call's last iteration wrote the dz segment"""
        N, dev, L = self.N, self.dev, s.L
        vp, prm, data = problem(s.L, s.decoder)
        h = dict(U.DEFAULTS, **dict(s.hyper))
        state = U.pack_state(prm)
        nz, nphi, ntau = L * 32, 2 * L * 6, 2 * L * 3
        bufs = {k: Buf(dev, state[k].numel()) for k in ("z", "phi", "tau", "beta")}
        for k in ("z", "phi", "tau", "beta"):
            bufs[k].out.copy_(state[k].float().reshape(-1))
        bufs["loss"] = Buf(dev, s.n_iters * L * 4)
        bufs["grad"] = Buf(dev, nz + nphi + ntau + 10)
        j2d, intr, extr = (data[k].float().contiguous().to(dev) for k in ("j2d", "intr", "extr"))
        rob = U.mask(s.mask, L).contiguous()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        N.check(N.lib().ap_fit_run(self.h, L, p(bufs["z"].out), p(bufs["phi"].out), p(bufs["tau"].out), p(bufs["beta"].out), p(j2d),
                                   p(rob), p(intr), p(extr), s.first_iter, s.n_iters, s.switch_iter, s.lr, h["sigma"], h["w_vposer"],
                                   h["w_temporal"], p(bufs["loss"].out), p(bufs["grad"].out), N.stream_ptr(dev)), "ap_fit_run")
        torch.cuda.current_stream(dev).synchronize()
        what = tuple(s)
        dz_written = s.first_iter + s.n_iters - 1 >= s.switch_iter
        if not dz_written:                                   # before the switch nobody computes dz: the segment keeps its NaNs
            assert torch.isnan(bufs["grad"].out[:nz]).all(), (what, "the dz segment was written before the switch")
            bufs["grad"].out[:nz] = 0.0
        out = dict(z=bufs["z"].values((L, 32), what), phi=bufs["phi"].values((2, L, 6), what), tau=bufs["tau"].values((2, L, 3), what),
                   beta=bufs["beta"].values((10,), what), loss=bufs["loss"].values((s.n_iters, L, 4), what))
        g = bufs["grad"].values((nz + nphi + ntau + 10,), what)
        out.update(dz=g[:nz].view(L, 32), dphi=g[nz:nz + nphi].view(2, L, 6), dtau=g[nz + nphi:nz + nphi + ntau].view(2, L, 3),
                   dbeta=g[nz + nphi + ntau:], dz_written=dz_written)
        assert all(torch.isfinite(v).all() for v in out.values() if torch.is_tensor(v)), (what, "non-finite output")
        return out


def bit_equal(a, b, keys=U.KINDS):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)


def run_twice_and_verify(fitter, s):
    got = fitter.run(s)
    again = fitter.run(s)
    assert bit_equal(got, again), (tuple(s), "two runs differ")
    ref = reference(s)
    fails = verify(got, ref, s, WORST, skip=() if got["dz_written"] else ("dz",))
    assert not fails, fails[:5]
    # Where the reference is exactly 0 the output is exactly 0, whatever the bar of its row allows: the gradients and loss parts of
    # frames that are not selected, the temporal parts of a selected frame whose predecessor is not (frame 0 always), column 3.
    for k in U.KINDS:
        if k != "dz" or got["dz_written"]:
            leak = int((got[k][ref[k] == 0] != 0).sum())
            assert leak == 0, (tuple(s), k, "%d elements nonzero where the reference is exactly 0" % leak)
    off = U.mask(s.mask, s.L) == 0
    assert not got["loss"][:, :, 3].view(torch.int32).any() and not got["loss"][:, off].any(), (tuple(s), "loss history")
    state = {k: v.float() for k, v in U.pack_state(problem(s.L, s.decoder)[1]).items()}
    if s.lr == 0.0:                                          # a gradient probe moves nothing
        assert bit_equal(got, state, ("z", "phi", "tau", "beta")), (tuple(s), "lr = 0 moved a parameter")
    if not got["dz_written"]:
        assert bit_equal(got, state, ("z",)), (tuple(s), "z changed before the switch")
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("L", PROBE_L)
def test_gradient_probe_on_both_paths(dev, body, L, decoder):
    """lr = 0, one iteration at it in PROBE_IT: the fused backward path (switch_iter = 0) against fp64, the pre-switch path
    (switch_iter > it) against fp64, and dphi, dtau, dbeta and the history of the two bit-equal"""
    f = Fitter(dev, problem(L, decoder)[0], body)
    try:
        for it in PROBE_IT:
            fused, _ = run_twice_and_verify(f, spec(L, decoder, first_iter=it, switch_iter=0))
            pre, _ = run_twice_and_verify(f, spec(L, decoder, first_iter=it, switch_iter=it + 1))
            assert fused["dz_written"] and not pre["dz_written"]
            assert bit_equal(fused, pre, ("dphi", "dtau", "dbeta", "loss")), (L, decoder, it, "the two paths differ")
    finally:
        f.close()


@pytest.mark.gpu
def test_wrapper_returns_zero_dz_before_the_switch(dev, body):
    from airpose_amd.fitting import AirPosePlusFitter
    L = 5
    vp, prm, data = problem(L, "body")
    f32 = lambda d: {k: v.float() for k, v in d.items() if v.is_floating_point()}
    fitter = AirPosePlusFitter(f32(vp), body, dev)
    d = f32(data)
    state, grads = fitter.run(f32(prm), d["j2d"], U.mask("all", L), d["intr"], d["extr"], n_iters=1, first_iter=1, switch_iter=2, lr=0.0,
                              want_grad=True)
    assert not grads["z"].view(torch.int32).any()
    assert torch.equal(state["z"].cpu(), prm["z"].float())
    ref = reference(spec(L, "body", first_iter=1, switch_iter=2))
    got = dict(dphi=torch.stack([grads["phi0"], grads["phi1"]]).cpu(), dtau=torch.stack([grads["tau0"], grads["tau1"]]).cpu(),
               dbeta=grads["beta"].cpu())
    for k, v in got.items():
        ok, _, _, msg = evaluate(v, ref[k], TOL["pairs"][k] * U.scale(ref[k]))
        assert ok, (k, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("L", MASK_L)
def test_masks(dev, body, L):
    """every mask on both paths; where the reference is exactly 0 (a frame that is not selected and has no selected neighbour pair,
    every temporal part without a pair, the 2-D part and beta's gradient without a selected frame) the bar demands exactly 0; a mask
    of 2 and -1 gives the bits of the same mask of ones (it goes through the raw ABI: the Python wrapper only makes 0 and 1)"""
    for dec in DECODERS:
        f = Fitter(dev, problem(L, dec)[0], body)
        try:
            res = {}
            for s in mask_specs(L):
                if s.decoder == dec:
                    res[s] = run_twice_and_verify(f, s)
            for s, (got, ref) in res.items():
                if s.mask in ("none", "alternating"):
                    assert not got["loss"][..., 1:].any() and not ref["loss"][..., 1:].any()
                if s.mask == "none":
                    assert not got["loss"].any() and not got["dphi"].any() and not got["dtau"].any() and not got["dbeta"].any()
                if s.mask == "odd_values":
                    same = res[s._replace(mask="interior_off")][0]
                    assert bit_equal(got, same), (tuple(s), "a mask value other than 0 or 1 changed the result")
        finally:
            f.close()


@pytest.mark.gpu
def test_hyper_parameters(dev, body):
    for s in hyper_specs():
        f = Fitter(dev, problem(s.L, s.decoder)[0], body)
        try:
            got, _ = run_twice_and_verify(f, s)
            default, _ = run_twice_and_verify(f, s._replace(hyper=()))
            assert not bit_equal(got, default, ("dphi", "dtau", "dbeta", "loss"))
        finally:
            f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", ADAM_L)
def test_adam_element_wise(dev, body, L):
    """one step from a fresh state on both paths (an element whose gradient is exactly 0 does not move), then three steps across
    the switch, from first_iter past the switch (a fresh Adam, counter 1, 2, 3) and with the switch at the last step: the
    parameters after the call and the three history rows at 0, 4 L, 8 L against ref_fit"""
    for dec in DECODERS:
        f = Fitter(dev, problem(L, dec)[0], body)
        try:
            for s in adam_specs(L):
                if s.decoder != dec:
                    continue
                got, ref = run_twice_and_verify(f, s)
                state = {k: v.float() for k, v in U.pack_state(problem(L, dec)[1]).items()}
                moved = 0
                for k in ("phi", "tau", "beta") + (("z",) if got["dz_written"] else ()):
                    still = ref["d" + k] == 0
                    if s.n_iters == 1:
                        same = torch.equal(got[k][still].view(torch.int32), state[k][still].view(torch.int32))
                        assert same, (tuple(s), k, "moved without a gradient")
                    moved += int((got[k] != state[k]).sum())
                    if s.n_iters == 1 and s.mask == "interior_off" and k in ("phi", "tau"):
                        assert still[:, L // 2].all() and not still[:, 0].any()
                assert moved > 0
        finally:
            f.close()


@pytest.mark.gpu
def test_handle_reuse_and_stream(dev, body):
    """L = 33, 5, 33 on one handle: each result bit-equal to the same call on a fresh handle (the handle's buffers only grow: what a
    longer sequence left behind them must not reach a shorter one); then the short case on a stream of its own"""
    big, small = reuse_specs()
    vp = problem(33, "all-branch")[0]
    assert all(torch.equal(vp[k], problem(5, "all-branch")[0][k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")), "one decoder for both sizes"

    def fresh(s):
        f = Fitter(dev, problem(s.L, s.decoder)[0], body)
        try:
            return run_twice_and_verify(f, s)[0]
        finally:
            f.close()
    want = {s: fresh(s) for s in (big, small)}
    f = Fitter(dev, problem(5, "all-branch")[0], body)
    try:
        for s in (big, small, big, small):
            assert bit_equal(f.run(s), want[s]), (tuple(s), "a reused handle gives another result")
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            got = f.run(small)
        assert bit_equal(got, want[small]), "another stream, another result"
    finally:
        f.close()
