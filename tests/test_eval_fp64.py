"""Element-wise fp64 ground truth for apg_eval_update (airpose_amd/csrc/eval_metrics.hip): the evaluation metrics of the reference's
test_epoch_end, through the C ABI of include/airpose_grad.h.  Companion of test_optim_fp64.py; evaluate() is test_stem_pool_fp64's,
the restatement, the emulation, the bars and the cases live in eval_util.py.

Reference.  eval_util.reference(): the header's semantics in fp64 on exactly the fp32 values the kernel receives -- tgm 0.1.2's
angle-axis -> matrix (eps = 1e-6 in the denominator, first-order branch at t2 <= eps), lbs.batch_rigid_transform on joints 0 .. 21,
Euclidean norms of the differences.  Test (a) shows that at fp64 its posed joints are those of four oracle SMPLX.forward calls with
betas = 0 (the reference's recipe) to 1e-12.

Bars (counted from the kernel's instruction sequence, none measured).  u = 2^-24; |got - ref| <= n u A, and where A = 0 the output is
exactly the reference.  Every product, sum, difference, quotient, square root and fmaf is one rounding (relative u); sinf / cosf are
allowed SINCOS_ULP = 2 ulps of their result (HIP documents 1), an ulp of v being at most 2 u |v|.  All magnitudes |.| below are the
fp64 reference's own.
  conversion (t2 > eps):
    t2 = fmaf(z, z, fmaf(y, y, x * x))      three roundings on a sum of positive terms: 3 u t2
    th = sqrtf(t2)                          halves that and adds its own: dth = 2.5 u th
    d  = th + eps                           eps's own rounding to float and the sum's: 4.5 u d;  w = r / d: dw = 5.5 u |w|
    c, s                                    dc = |s| dth + 4 u |c|,  ds = |c| dth + 4 u |s|
    omc = 1 - c                             domc = dc + u |omc|      (absolute: the cancellation at small angles is tgm's own)
    a_i = w_i omc,  s_i = w_i s             da_i = |w_i| domc + |omc| dw_i + u |a_i|,  ds_i = |w_i| ds + |s| dw_i + u |s_i|
    R_ik = fmaf(w_i, a_k, c or +-s_m)       dR_ik = |w_i| da_k + |a_k| dw_i + (dc or ds_m) + u |R_ik|
  conversion (t2 <= eps): I + skew(r) holds input bits and exact ones: dR = 0.  Ground-truth and matrix-mode rotations: dR = 0.
  chain step j with parent P (matrices entry-wise, |G'| = |G| + EG, |R'| = |R| + dR, b = J_j - J_P with its rounding eb = u |b|):
    G_j = G_P R_j, three-term fmaf chains   EG_j = EG_P |R'| + |G_P| dR_j + 3 u |G'_P| |R'_j|
    p_j = p_P + G_P b                       Ep_j = Ep_P + EG_P |b'| + |G_P| eb + 3 u |G'_P| |b'| + u (|p_P| + Ep_P + |G'_P| |b'|)
    -- each step adds its matmul's roundings on the running bone-length sum; EG_0 = dR_0, Ep_0 = 0 (p_0 = J_0 bit for bit)
  joint_err: d = p_pred - p_gt              Ed = Ep_pred + Ep_gt + u (|d| + Ep_pred + Ep_gt)
             e = sqrtf(fmaf chain of d^2)   the norm moves by at most |Ed|_1; three roundings under the root (1.5 u e) and the
                                            root's own: bar = |Ed|_1 + 3 u (e + |Ed|_1)
  trans_err, angle_err: the same with Ed = u |d| (inputs are exact): at most (sqrt 3 + 3) u e, and 0 where pred == gt.
  accumulators: the elements' bars summed, plus the fp64 roundings of the partial sums (terms x 2^-53 x the sums' magnitude).
The root's placement p_0 = J_0 cancels in every error (both chains share it), so no output of the kernel can see it: it is pinned by
(a) and by the position bars of the emulation, which is why `root_not_at_j0` is judged on the positions.  `eps_dropped` moves every
converted matrix by about eps = 17 u per entry, the size of a handful of roundings: it leaves the position bars (by 2.7 x at B = 17)
but stays inside the bar of the distances, whose two chains' bounds add.

CPU part (no GPU): (a) above; (b) emulate(), an fp32 evaluation of the kernel's exact sequence (an fma is formed in fp64 -- the product
of two floats is exact there -- and rounded to float; torch's sin / cos stand in for the device's), stays inside every bar on all
cases; (c) each of MUTATIONS leaves the bars on at least one output of one case.

GPU part.  Per-sample outputs element-wise inside the bars; accumulators against fp64 sums of the reference's per-sample values,
counts exact.  views in {1, 2}; B in {1, 2, 63, 64, 65 (the wave size), SPW - 1, SPW, SPW + 1, 2 SPW + 1} with SPW = 32 / views the
kernel's samples per workgroup (65 spans three workgroups with one view, five with two); angle-axis and matrix mode; with and without
translations and gt angles.  Inputs as eval_util.make_case states.  Matrix mode fed the ground truth's bits: every joint_err is 0.0
and mpjpe is 0.  Every call runs twice into fresh buffers between NaN guard bands: bit-equal, guards untouched, inputs unchanged.
Three updates of unequal B into one accumulator equal one reference() over their concatenation; the sequence repeated is bit-equal.
"""
import itertools

import pytest
import torch

import eval_util as E
from test_stem_pool_fp64 import evaluate

OUTS = ("joint_err", "trans_err", "angle_err")


@pytest.fixture(scope="module")
def rest(smplx_model):
    from airpose_amd.eval_metrics import rest_joints
    return rest_joints(smplx_model)


CASES = [(views, B, mode, extras) for views in (1, 2) for B in E.batch_sizes(views) for mode in ("aa", "rotmat")
         for extras in (False, True)]
_ID = lambda c: "v%d-B%d-%s-%s" % (c[0], c[1], c[2], "extras" if c[3] else "bare")
_cache = {}


def prepared(rest, key):
    """(case, reference, bars) of one case, computed once and shared"""
    if key not in _cache:
        case = E.make_case(rest[0], rest[1], key[1], key[0], key[2], key[3])
        ref = E.reference(case)
        _cache[key] = (case, ref, E.bars(case, ref))
    return _cache[key]


def check_outputs(got, ref, bar, what, names=OUTS):
    worst = {}
    for n in names:
        if ref[n] is None:
            assert got.get(n) is None, "%s: %s written without its inputs" % (what, n)
            continue
        ok, ratio, _, msg = evaluate(got[n], ref[n], bar[n])
        worst[n] = ratio
        assert ok, "%s %s: %s" % (what, n, msg)
    return worst


# ------------------------------------------------------------------------------------------------ CPU
def test_reference_is_the_four_smplx_forward_recipe(smplx_model, rest):
    """(a): the chain-only form equals oracle SMPLX.forward(betas = 0) on joints 0 .. 21, for gt and pred, both views, at fp64"""
    from oracle import smplx_ref
    case = E.make_case(rest[0], rest[1], 3, 2, "aa", False, seed=5)
    j64 = (torch.as_tensor(smplx_model["J_regressor"]).double() @ torch.as_tensor(smplx_model["v_template"]).double())[:22]
    ref = E.reference(case, j_rest=j64)
    betas = torch.zeros(3, 10, dtype=torch.float64)
    for v in (0, 1):
        for name, R in (("p_gt", ref["R_gt"][v]), ("p_pred", ref["R_pred"][v])):
            joints = smplx_ref.smplx_forward(smplx_model, betas, R[:, 1:], R[:, :1], dtype=torch.float64)[1][:, :22]
            assert float((joints - ref[name][v]).abs().max()) <= 1e-12, (v, name)


@pytest.mark.parametrize("key", CASES, ids=_ID)
def test_emulation_stays_inside_the_bars(rest, key):
    """(b)"""
    case, ref, bar = prepared(rest, key)
    emu = E.emulate(case)
    check_outputs(emu, ref, bar, "emulate", OUTS + ("p_gt", "p_pred"))
    acc, abar = E.accumulate([emu], [bar], key[0])
    racc, _ = E.accumulate([ref], [bar], key[0])
    ok, _, _, msg = evaluate(acc, racc, abar)
    assert ok, msg


def test_exact_zero_bars(rest):
    """where pred == gt the translation and angle bars are 0: the output must be the reference exactly"""
    case = E.make_case(rest[0], rest[1], 4, 2, "aa", True, seed=2)
    for d in case["view"]:
        d["pred_trans"] = d["gt_trans"].clone()
        d["gt_angles"] = d["pred"].clone()
    ref = E.reference(case)
    bar = E.bars(case, ref)
    assert float(bar["trans_err"].max()) == 0 and float(bar["angle_err"].max()) == 0
    assert float(ref["trans_err"].max()) == 0 and float(ref["angle_err"].max()) == 0
    check_outputs(E.emulate(case), ref, bar, "emulate")


@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_mutations_are_rejected(rest, mutation):
    """(c): computed in fp64 with one deliberate mistake, at least one output of one case leaves its bar"""
    rejected = []
    for key in ((2, 3, "aa", True), (2, 17, "aa", True), (1, 5, "aa", True)):
        case, ref, bar = prepared(rest, key)
        mut = E.reference(case, mutation=mutation)
        for n in OUTS + ("p_gt", "p_pred"):
            if ref[n] is not None and not evaluate(mut[n], ref[n], bar[n])[0]:
                rejected.append((key, n))
        acc, abar = E.accumulate([ref], [bar], key[0])
        got, want = E.summarise(acc, key[0], mutation), E.summarise(acc, key[0])
        for k in want:                                        # the bar of a mean: its sum's bar over the same divisor
            v, col, div = int(k[-1]), {"mpjpe": 1, "mpe": 24, "angle_err": 25}[k[:-1]], {"mpjpe": 22.0, "mpe": 1.0, "angle_err": 22.0}[k[:-1]]
            if abs(got[k] - want[k]) > float(abar[v, col]) / (float(acc[v, 0]) * div):
                rejected.append((key, k))
    assert rejected, "no output of any case rejects %s" % mutation


def test_threshold_vectors_sit_on_either_side_of_eps(rest):
    """t2 = 0.81e-6 and 1.21e-6 evaluated in fp32 and in fp64 fall on the same sides of eps; every special vector is present"""
    for key in ((1, 1, "aa", False), (2, 65, "aa", True)):
        case = prepared(rest, key)[0]
        for d in case["view"]:
            r = d["pred"].reshape(-1, 3)
            n = r.double().norm(dim=-1)
            for want in E.SPECIAL_NORMS:
                assert bool(((n - want).abs() <= 1e-6 * max(want, 1e-3)).any()), want
            t32 = E.aa_to_rotmat(r, emu=True)[1]["big"]
            t64 = E.aa_to_rotmat(r.double())[1]["big"]
            assert torch.equal(t32, t64)
            lo, hi = (n - 0.9e-3).abs().argmin(), (n - 1.1e-3).abs().argmin()
            assert not bool(t32[lo]) and bool(t32[hi])
            assert bool((~t32).sum() >= 2)                        # the zero vector takes the first-order branch too


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda", 0)


def _bit_equal(a, b):
    for k in OUTS + ("acc",):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k].view(torch.int64),
                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k].view(torch.int64)), k


def _check_acc(got_acc, refs, bars_list, views, what):
    racc, abar = E.accumulate(refs, bars_list, views)
    for col in (0, 26, 27):                                       # counts are exact
        assert torch.equal(got_acc[:, col], racc[:, col]), (what, col, got_acc[:, col], racc[:, col])
    if views == 1:
        assert float(got_acc[1].abs().max()) == 0, "%s: the second view's accumulator was touched" % what
    ok, _, _, msg = evaluate(got_acc, racc, abar)
    assert ok, "%s accumulator: %s" % (what, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("key", CASES, ids=_ID)
def test_update_against_fp64(rest, key):
    case, ref, bar = prepared(rest, key)
    a = E.run_gpu(case, _dev())
    b = E.run_gpu(case, _dev())
    for r in (a, b):
        assert r["guards_ok"], "a guard band was written"
        assert r["inputs_ok"], "an input was changed"
    _bit_equal(a, b)
    worst = check_outputs(a, ref, bar, _ID(key))
    print("%s worst err / bar: %s" % (_ID(key), {k: round(v, 3) for k, v in worst.items()}))
    _check_acc(a["acc"], [ref], [bar], key[0], _ID(key))
    c = E.run_gpu(case, _dev(), per_sample=False)                 # without the optional outputs: the same sums
    assert c["guards_ok"] and torch.equal(c["acc"], a["acc"])


@pytest.mark.gpu
@pytest.mark.parametrize("views,B", [(v, B) for v in (1, 2) for B in (1, 17, 65)])
def test_matrix_mode_on_the_ground_truths_bits_is_exactly_zero(rest, views, B):
    case = E.make_case(rest[0], rest[1], B, views, "rotmat", True, seed=3)
    for d in case["view"]:
        d["pred"] = torch.cat([d["gt_orient"], case["gt_body"]], 1).clone()
    r = E.run_gpu(case, _dev())
    assert r["guards_ok"] and r["inputs_ok"]
    assert torch.equal(r["joint_err"], torch.zeros(views, B, 22)), float(r["joint_err"].abs().max())
    assert not bool(torch.signbit(r["joint_err"]).any())
    assert float(r["acc"][:views, 1:24].abs().max()) == 0
    assert E.summarise(r["acc"], views)["mpjpe0"] == 0.0
    assert float(r["acc"][0, 0]) == B


@pytest.mark.gpu
@pytest.mark.parametrize("views,mode", list(itertools.product((1, 2), ("aa", "rotmat"))))
def test_three_updates_equal_one_reference_over_their_concatenation(rest, views, mode):
    sizes = (E.spw(views) + 3, 1, 2 * E.spw(views) + 5)
    cases = [E.make_case(rest[0], rest[1], B, views, mode, True, seed=10 + i) for i, B in enumerate(sizes)]

    def sequence():
        acc = None
        for c in cases:
            r = E.run_gpu(c, _dev(), acc_init=acc, per_sample=False)
            assert r["guards_ok"] and r["inputs_ok"]
            acc = r["acc"]
        return acc
    acc = sequence()
    whole = E.concat_cases(cases)
    ref = E.reference(whole)
    _check_acc(acc, [ref], [E.bars(whole, ref)], views, "three updates")
    assert torch.equal(acc.view(torch.int64), sequence().view(torch.int64))
