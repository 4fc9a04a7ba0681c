"""fp64 ground truth for apg_align_update (airpose_amd/csrc/eval_align.hip): abs, root-aligned and Procrustes-aligned error between
two point sets, through the C ABI of include/airpose_grad.h.  Companion of test_eval_fp64.py; the reference, the emulation, the
bars and the cases live in align_util.py.

Reference.  align_util.reference(): the header's semantics in fp64 with numpy.linalg.svd on exactly the fp32 values the kernel
receives.  It is pinned three ways below: q = s0 R0 p + t0 is recovered to 1e-12, random perturbations of the returned (s, R, t)
never lower sum |s R p + t - q|^2, and a mirrored prediction gets det R = +1.

Bars (counted from the kernel's instruction sequence, none measured).  u = 2^-24, v = 2^-53; |got - ref| <= bar, where the bar is 0
the output is exactly the reference, and all magnitudes are the reference's own.
  per point, abs:   d = p - q in fp64 is exact (floats less than 2^29 apart in exponent); each component rounds to float (u |d_k|:
                    the norm moves by at most u e_i), three roundings under the root (1.5 u e_i) and the root's own (u e_i):
                    4 u e_i covers them.
            root:   (p - r_p) - (q - r_q): the two inner differences are exact, the outer one rounds: 4 v (|p - r_p|_1 + |q - r_q|_1)
                    over the components, then as abs.  Where pred == gt and the roots are equal the value is exactly 0.
            pa:     c = p - mu_p, three products and two sums of R c, the scale, mu_q - q and the last sum: 10 v (s |c|_1 + |mu_q - q|_1),
                    what the solve's own error moves (below), then as abs.
  per sample: the fp64 sum of N terms in a fixed order and the division: (N + 70) v e.  `mean` (what goes into the accumulator) is
              that; `err` adds the rounding to float, u e.
  solve (fp64): the 16 moments are sums of N terms about the pivots p_0, q_0: (N + 20) v A_K per entry of K with A_K = max(sum
              |a_i|_1 |b_i|_1, sum |a|_1 sum |b|_1 / N) (the second is what the centring subtracts).  Horn's matrix adds four of
              them per entry; SWEEPS x 6 Jacobi rotations of 6 roundings each act on entries of at most 9 sigma_1 <= 9 A_K:
                dN = (4 (N + 20) + 6 * 6 * 6 * 9) v A_K.
              Six sweeps of a 4 x 4 cyclic Jacobi are taken as converged (quadratic; the emulation below runs the same six and
              is held to the same bars, and holds them with four).  The largest eigenvalue lies 2 (sigma_2 + d sigma_3) above the
              next, so its eigenvector moves by |dN|_2 / (gap / 2) <= 4 dN / (sigma_2 + d sigma_3) and R, quadratic in it, by
                dR = 16 dN / (sigma_2 + d sigma_3 - 4 dN):        the conditioning factor, from the reference's singular values
                ds = (4 dN + s (N + 20) v sum |a|^2) / var,  dmu = (N + 4) v (mean |a|_1 + |pivot|).
  transform: s: u s + ds;  R: u |R| + dR;  t = mu_q - s R mu_p: u |t| + dmu_q + ds |R| |mu_p| + 3 s dR |mu_p|_1 + 3 s dmu_p + 10 v (..).
  With N <= 10475 and gap >= 0.05 sigma_1 every fp64 term is below 1e-9 of its magnitude: the bars are the final roundings.
  all p equal (N = 1 included): s = 0 and R = I exactly, t = mu_q, pa = mean |mu_q - q_i|.
  collinear sets (N = 2 included): R, t and pa carry no bar; every output is finite and det R = +1 within 4 u (float rounding of a
  rotation's entries moves its determinant by at most 3 u).  That determinant bar is asked of EVERY sample.
  accumulators: the samples' `mean` bars summed, plus (B + 2) v on the running sums; counts exact.

CPU part (no GPU): the three pins; emulate(), the kernel's sequence on the host in fp64 (fp32 norms), stays inside every bar on all
cases; each of MUTATIONS leaves the bars on at least one case; the generator asserts sigma_2 >= 0.05 sigma_1 and
sigma_2 + d sigma_3 >= 0.05 sigma_1 on every non-degenerate sample it makes.

GPU part.  views in {1, 2} x B in {1, 2, 5} x N in {1, 2, 3, 22, 63, 64, 65 (one wave / sixteen), 1023, 1024, 1025 (a thread's second
point), 10475}; each case once with strides 3 N and roots on every view, once with strides above 3 N (not multiples of 3, the arrays
one float past a 16-byte boundary, 1e30 between the samples) and roots on the last view only.  Sample kinds as
align_util.make_sample: a body of 0.5 m extent at 10 m depth with a plausible prediction, a rigid-plus-scale copy, a mirrored
prediction, pred == gt bit for bit, coincident points, a collinear set.  Every call runs twice into fresh buffers between NaN guard
bands: bit-equal, guards untouched, inputs unchanged.  Three updates of unequal B into one accumulator equal one reference over
their concatenation.
"""
import numpy as np
import pytest
import torch

import align_util as A

CASES = [(views, B, N) for views in (1, 2) for B in (1, 2, 5) for N in A.SIZES]
_ID = lambda c: "v%d-B%d-N%d" % c
_cache = {}


def prepared(key, padded=False):
    """(case, reference, bars) of one case, computed once and shared; the padded form holds the same points"""
    k = key + (padded,)
    if k not in _cache:
        case = A.make_case(key[0], key[1], key[2], padded)
        ref = A.reference(case)
        _cache[k] = (case, ref, A.bars(case, ref))
    return _cache[k]


def check_all(got, ref, bar, roots, what):
    views = ref["err"].shape[0]
    worst = {}
    for v in range(views):
        cols = [0, 1, 2] if roots[v] else [0, 2]
        worst["err%d" % v] = A.check(got["err"][v][:, cols], ref["err"][v][:, cols], bar["err"][v][:, cols], "%s err of view %d" % (what, v))
        if not roots[v]:
            assert not got["err"][v][:, 1].any(), "%s: root written without roots" % what
    worst["transform"] = A.check(got["transform"], ref["transform"], bar["transform"], what + " transform")
    A.check_rotations(got["transform"], bar["cls"], what)
    return worst


# ------------------------------------------------------------------------------------------------ CPU: the reference is pinned
def test_reference_recovers_an_exact_similarity():
    rng = np.random.default_rng(1)
    for N in (3, 22, 500):
        P = rng.uniform(-0.3, 0.3, (N, 3)) + np.array([0.0, 0.0, 10.0])
        s0, R0, t0 = 1.7, A._rot(rng), np.array([0.3, -1.0, 2.0])
        Q = s0 * P @ R0.T + t0
        sol = A.reference_sample(P, Q, P[0], Q[0])
        scale = np.abs(Q).max()
        assert sol["err"][2] <= 1e-12 * scale
        assert abs(sol["s"] - s0) <= 1e-12 and np.abs(sol["R"] - R0).max() <= 1e-12 and np.abs(sol["t"] - t0).max() <= 1e-11
        assert sol["err"][1] > 1e-3 and sol["err"][0] > 1e-3


def test_reference_is_a_minimum():
    rng = np.random.default_rng(2)
    for kind in ("far", "mirror", "similar"):
        P, Q, rp, rq = (x.astype(np.float64) for x in A.make_sample(kind, 40, rng))
        sol = A.reference_sample(P, Q, rp, rq)
        f = lambda s, R, t: float(((s * P @ R.T + t - Q) ** 2).sum())
        f0 = f(sol["s"], sol["R"], sol["t"])
        for _ in range(200):
            eps = 10.0 ** rng.uniform(-6, -1)
            R = A._rot(rng, eps) @ sol["R"]
            assert f(sol["s"] * (1 + eps * rng.standard_normal()), R, sol["t"] + eps * rng.standard_normal(3)) >= f0 * (1 - 1e-12)
            assert f(sol["s"], R, sol["t"]) >= f0 * (1 - 1e-12)


def test_reference_keeps_det_plus_one_on_a_mirrored_prediction():
    rng = np.random.default_rng(3)
    P, Q, rp, rq = A.make_sample("mirror", 100, rng)
    sol = A.reference_sample(P, Q, rp, rq)
    assert sol["d"] == -1.0 and abs(np.linalg.det(sol["R"]) - 1.0) <= 1e-12
    assert sol["err"][2] > 0.05                              # a mirrored body does not fit


def test_degenerate_rules():
    Q = np.array([[0.0, 1.0, 10.0], [1.0, 1.0, 11.0], [0.0, 3.0, 10.0]])
    sol = A.reference_sample(np.ones((3, 3)), Q, Q[0], Q[0])
    assert sol["s"] == 0.0 and np.array_equal(sol["R"], np.eye(3))
    assert abs(sol["err"][2] - np.linalg.norm(Q.mean(0) - Q, axis=1).mean()) <= 1e-15
    one = A.reference_sample(Q[:1] + 0.5, Q[:1], Q[0], Q[0])
    assert one["s"] == 0.0 and one["err"][2] == 0.0 and abs(one["err"][0] - 0.75 ** 0.5) <= 1e-15


# ------------------------------------------------------------------------------------------------ CPU: the kernel's sequence
@pytest.mark.parametrize("key", [c for c in CASES if c[1] == 5 or c[2] == 22], ids=_ID)
def test_emulation_stays_inside_the_bars(key):
    case, ref, bar = prepared(key)
    emu = A.emulate(case)
    check_all(emu, ref, bar, (True, True), "emulate " + _ID(key))
    roots = [(True, True)]
    acc, abar = A.accumulate([emu], [bar], roots, key[0])
    racc, _ = A.accumulate([ref], [bar], roots, key[0])
    A.check(acc, racc, abar, "emulate accumulator")


def test_every_kind_is_generated_at_every_size():
    seen = {}
    for key in CASES:
        case = prepared(key)[0]
        for d in case["view"]:
            for k in d["kinds"]:
                seen.setdefault(key[2], set()).add(k)
    for N in A.SIZES:
        assert seen[N] == set(A.KINDS), (N, seen[N])


def test_same_kind_is_exactly_zero_in_the_emulation():
    case = A.make_case(2, 3, 65, False, kinds=[["same"] * 3, ["same"] * 3])
    emu = A.emulate(case)
    assert not emu["err"][:, :, :2].any()


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_mutations_are_rejected(mutation):
    rejected = []
    for key in ((2, 5, 22), (1, 5, 1025), (2, 5, 10475)):
        case, ref, bar = prepared(key)
        mut = A.emulate(case, mutation)
        for name in ("err", "transform"):
            try:
                A.check(mut[name], ref[name], bar[name], name)
            except AssertionError:
                rejected.append((key, name))
    assert rejected, "no output of any case rejects %s" % mutation


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda", 0)


def _bit_equal(a, b):
    for k in ("err", "transform", "acc"):
        assert a[k].tobytes() == b[k].tobytes(), k


def _check_acc(got, refs, bars_list, roots_list, views, what):
    racc, abar = A.accumulate(refs, bars_list, roots_list, views)
    for col in (0, 4):
        assert np.array_equal(got[:, col], racc[:, col]), (what, col, got[:, col], racc[:, col])
    if views == 1:
        assert not got[1].any(), "%s: the second view's accumulator was touched" % what
    for v in range(views):
        if not roots_list[0][v] and len(roots_list) == 1:
            assert got[v, 2] == 0.0
    A.check(got, racc, abar, what + " accumulator")


@pytest.mark.gpu
@pytest.mark.parametrize("key", CASES, ids=_ID)
def test_update_against_fp64(key):
    views = key[0]
    for padded, roots in ((False, (True, True)), (True, (False, views == 2))):
        case, ref, bar = prepared(key, padded)
        what = "%s %s" % (_ID(key), "padded" if padded else "tight")
        a = A.run_gpu(case, _dev(), roots=roots, skew=padded)
        b = A.run_gpu(case, _dev(), roots=roots, skew=padded)
        for r in (a, b):
            assert r["guards_ok"], what + ": a guard band was written"
            assert r["inputs_ok"], what + ": an input was changed"
        _bit_equal(a, b)
        worst = check_all(a, ref, bar, roots, what)
        print("%s worst err / bar: %s" % (what, {k: round(x, 3) for k, x in worst.items()}))
        _check_acc(a["acc"], [ref], [bar], [roots], views, what)
        for v in range(views):
            for s, kind in enumerate(case["view"][v]["kinds"]):
                if kind == "same":                           # pred == gt bit for bit: exactly 0.0, not -0.0
                    assert a["err"][v, s, 0] == 0.0 and a["err"][v, s, 1] == 0.0 and not np.signbit(a["err"][v, s, :2]).any()
        c = A.run_gpu(case, _dev(), roots=roots, per_sample=False, skew=padded)      # without the optional outputs: the same sums
        assert c["guards_ok"] and c["acc"].tobytes() == a["acc"].tobytes()


@pytest.mark.gpu
def test_every_kind_at_the_production_vertex_count():
    kinds = [list(A.KINDS), list(A.KINDS[::-1])]
    case = A.make_case(2, len(A.KINDS), 10475, True, seed=4, kinds=kinds)
    ref = A.reference(case)
    bar = A.bars(case, ref)
    a = A.run_gpu(case, _dev(), skew=True)
    assert a["guards_ok"] and a["inputs_ok"]
    check_all(a, ref, bar, (True, True), "production")
    _check_acc(a["acc"], [ref], [bar], [(True, True)], 2, "production")


@pytest.mark.gpu
@pytest.mark.parametrize("views,N", [(1, 22), (2, 65), (2, 10475)])
def test_three_updates_equal_one_reference_over_their_concatenation(views, N):
    cases = [A.make_case(views, B, N, False, seed=10 + i) for i, B in enumerate((5, 1, 7))]
    roots = (True, True)

    def sequence():
        acc = None
        for c in cases:
            r = A.run_gpu(c, _dev(), acc_init=acc, per_sample=False)
            assert r["guards_ok"] and r["inputs_ok"]
            acc = r["acc"]
        return acc
    acc = sequence()
    whole = A.concat_cases(cases)
    ref = A.reference(whole)
    _check_acc(acc, [ref], [A.bars(whole, ref)], [roots], views, "three updates")
    assert acc.tobytes() == sequence().tobytes()
