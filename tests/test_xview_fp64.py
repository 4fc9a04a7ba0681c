"""fp64 ground truth for apg_xview_update and apg_xview_triangulate (airpose_amd/csrc/xview_metrics.hip): the cross-view gaps, the
reprojection error and the triangulation of a calibrated pair, through the C ABI of include/airpose_grad.h.  Companion of
test_align_fp64.py; the reference, the emulation, the bars and the cases live in xview_util.py.

Reference.  xview_util.reference(): the header's semantics in fp64 on exactly the fp32 values the kernel receives, with
numpy.linalg.inv of the 4 x 4 extrinsics and numpy.linalg.lstsq of the 4 x 3 system written as in the reference's
lstsq_triangulation.  It is pinned four ways below: W_v undoes E_v to 1e-12, noise-free projections triangulate back to the point to
1e-9, the triangulation of a rigidly moved world moves with it, and both angle gaps are invariant under a common world rotation.

Bars (counted from the kernel's instruction sequence, none measured).  u = 2^-24, v = 2^-53; |got - ref| <= bar, where the bar is 0
the output is exactly the reference, and all magnitudes are the reference's own.
  per point, a gap g = |R_0^T (p0 - o0) - R_1^T (p1 - o1)| (o = t: world, o = the root: root):
            model:  the kernel takes R^T where the reference inverts: the component-wise |R_v^T - R_v^-1| |p_v - o_v|, both views,
                    in the 2-norm.  The generator keeps |R^T R - I| <= 1e-6 on every sample that is not skipped, so this is the
                    float rounding of the extrinsics, about 1e-7 |p - o|.
            fp64:   p - o (one rounding), three products and two sums per component, the difference of the two views:
                    16 v (|p0 - o0|_1 + |p1 - o1|_1) covers them.
            fp32:   each component rounds to float (the norm moves by at most u g), three roundings under the root (1.5 u g) and the
                    root's own (u g): 4 u g.
  per sample: the fp64 sum of N terms in a fixed order and the division: (N + 70) v value.  `sums` (what goes into the accumulator)
              is that; `ps` adds the rounding to float, u value.  trans_gap is one such point.
  angles:   D = A^T B from entries with error dQ each: 3 (dQ_A + dQ_B) + 6 v per entry of D.  With s = |axial vector| = 2 sin and
            c = tr D - 1 = 2 cos: |ds| <= 2 sqrt(3) dD, |dc| <= 3 dD and d(atan2) <= (|ds| + |dc|) / 2 <= 3.3 dD: 4 dD radians, plus
            16 v pi for the square root and atan2 themselves.  dQ = 0 for matrices; for angle-axis vectors eval_util._conv_bars, the
            bound counted for the same fp32 conversion in test_eval_fp64.py (1.01: tgm's matrices are orthonormal to 1e-5 only).  The
            orientation carries the model term of R_v^T Q (the row sums of |R_v^T - R_v^-1|) and its 12 v.
  reproj:   the difference rounds to float per component, one product, one fma, the root: 4 u; the fp64 weighting and division 60 v.
  T_i:      the normal equations square the conditioning of the 4 x 3 system: 64 v kappa^2 (|T| + |b| / sigma_1) with
            kappa = sigma_1 / sigma_3 from the reference's own singular values (numpy.linalg.lstsq returns them); for the generator's
            cameras kappa <= 120 or so and the bar stays below 1e-9 m.  `tri` adds u |T| for the float it is stored as.
  tri_mpjpe: one carry (model, fp64 and fp32 terms as above) and sqrt(3) times T_i's bar.
  accumulators: the samples' `sums` bars added, plus (B + 2) v on the running sums; counts exact.
Two views that hold identical bits under identity extrinsics give every gap exactly 0.0 (asserted apart from the bars).

CPU part (no GPU): the four pins; emulate(), the kernel's sequence on the host, stays inside every bar on every case; each of
MUTATIONS leaves the bars on at least one case; the generator asserts on every sample that non-skipped extrinsics are orthonormal to
1e-6 and that no ray pair has sin^2 within a factor 2 of the gate, so that the reference's skip and valid decisions are never a
rounding question.

GPU part.  B in {1, 2, 5} x V in {none, 1, 63, 64, 65, 1023, 1025 (a second chunk), 10475}, n_joints in {1, 22} out of J in {22, 127},
matrices and angle-axis vectors, both roots; each case once densely packed and once with strides above the minimum, the arrays one
float past a 16-byte boundary, 1e30 between the samples and (3, 4) extrinsics.  Sample kinds as xview_util.make_sample.  Every call
runs twice into fresh buffers between NaN guard bands: bit-equal, guards untouched, inputs unchanged.  Three updates of unequal B into
one accumulator equal one reference over their concatenation.  apg_xview_triangulate alone gives the same tri.
"""
import math

import numpy as np
import pytest
import torch

import xview_util as X

COMBOS = ((22, 22), (1, 127), (22, 127), (1, 22))            # (n_joints, J)
CASES = [(B, V) + COMBOS[(i + k) % 4] + (("rotmat", "aa")[(i + k) % 2], ("trans", "joint0")[(i + k // 2) % 2])
         for i, B in enumerate((1, 2, 5)) for k, V in enumerate(X.SIZES)]
_ID = lambda c: "B%d-V%d-n%d-J%d-%s-%s" % c
_cache = {}


def prepared(key, padded=False):
    """(case, reference, bars) of one case, computed once and shared"""
    k = key + (padded,)
    if k not in _cache:
        B, V, nj, J, rot, root = key
        case = X.make_case(B, nj, J, V, padded, rot, root)
        ref = X.reference(case)
        _cache[k] = (case, ref, X.bars(case, ref))
    return _cache[k]


def check_all(got, ref, bar, what):
    worst = {"ps": X.check(got["ps"], ref["ps"], bar["ps"], what + " per-sample values")}
    if got.get("tri") is not None:
        worst["tri"] = X.check(got["tri"], ref["tri"], bar["tri"], what + " tri")
    return worst


def check_acc(got, refs, bars_list, what):
    racc, abar = X.accumulate(refs, bars_list)
    assert got[X.ACC - 1] == 0.0, what + ": the reserved slot was touched"
    return X.check(got, racc, abar, what + " accumulator")


def assert_identical_is_zero(case, ps, what):
    for b, kind in enumerate(case["kinds"]):
        if kind == "identical":                              # exactly 0.0, not -0.0
            assert not ps[b, 1:8].any() and not np.signbit(ps[b, 1:8]).any(), (what, b, ps[b])


# ------------------------------------------------------------------------------------------------ CPU: the reference is pinned
def _cams(rng):
    c = rng.uniform(-1, 1, 3)
    return c, [X._look_at(c + rng.uniform(6, 10) * d / np.linalg.norm(d), c, rng) for d in rng.standard_normal((2, 3))]


def test_reference_world_carry_undoes_the_extrinsics():
    rng = np.random.default_rng(1)
    case = X.make_case(4, 22, 22, 0, False, kinds=["consistent"] * 4)
    ref = X.reference(case)
    for b in range(4):
        for v in range(2):
            R, t = ref["aux"][b]["cams"][v]
            x = rng.uniform(-2, 2, (50, 3))
            back = ((x @ R.T + t) - t) @ ref["aux"][b]["inv"][v].T
            assert np.abs(back - x).max() <= 1e-12
    assert ref["ps"][:, 1].max() < 2e-6 and ref["ps"][:, 5].max() < 2e-6      # consistent views: the gaps are the inputs' rounding


def _project(E, K, x):
    p = E[0] @ x + E[1]
    return np.array([K[0, 0] * p[0] / p[2] + K[0, 2], K[1, 1] * p[1] / p[2] + K[1, 2], 1.0])


def test_reference_triangulates_noise_free_projections_back():
    rng = np.random.default_rng(2)
    K = [np.array([[1500.0, 0, 960], [0, 1480.0, 540], [0, 0, 1]]), np.array([[1450.0, 0, 940], [0, 1520.0, 560], [0, 0, 1]])]
    for _ in range(20):
        c, cams = _cams(rng)
        x = c + rng.uniform(-0.3, 0.3, 3)
        e = [np.concatenate([Rv, tv[:, None]], 1).reshape(-1) for Rv, tv in cams]
        T, valid, sv, _ = X.tri_reference(e[0], e[1], K[0], K[1], _project(cams[0], K[0], x), _project(cams[1], K[1], x), 0.0)
        assert valid and np.abs(T - x).max() <= 1e-9, (T, x, sv)
        Te, ve = X.tri_emulated(e[0], e[1], K[0], K[1], _project(cams[0], K[0], x), _project(cams[1], K[1], x), 0.0)
        assert ve and np.abs(Te - x).max() <= 1e-9


def test_reference_triangulation_moves_with_the_world():
    rng = np.random.default_rng(3)
    K = np.array([[1500.0, 0, 960], [0, 1500.0, 540], [0, 0, 1]])
    for _ in range(20):
        c, cams = _cams(rng)
        kp = [_project(cams[v], K, c + rng.uniform(-0.3, 0.3, 3)) + np.append(rng.uniform(-3, 3, 2), 0) for v in range(2)]
        G, g = X._rot(rng), rng.uniform(-5, 5, 3)
        moved = [(Rv @ G.T, tv - Rv @ G.T @ g) for Rv, tv in cams]                # x_cam = R G^T (x' - g) + t
        flat = lambda cs: [np.concatenate([Rv, tv[:, None]], 1).reshape(-1) for Rv, tv in cs]
        T = X.tri_reference(*flat(cams), K, K, kp[0], kp[1], 0.0)[0]
        Tm = X.tri_reference(*flat(moved), K, K, kp[0], kp[1], 0.0)[0]
        assert np.abs(Tm - (G @ T + g)).max() <= 1e-9


def test_reference_angle_gaps_do_not_see_a_common_world_rotation():
    rng = np.random.default_rng(4)
    for _ in range(20):
        _, cams = _cams(rng)
        Q = [X._rot(rng), X._rot(rng)]
        G = X._rot(rng)
        a = X.angle_deg(np.linalg.inv(cams[0][0]) @ Q[0], np.linalg.inv(cams[1][0]) @ Q[1])
        b = X.angle_deg(np.linalg.inv(cams[0][0] @ G.T) @ Q[0], np.linalg.inv(cams[1][0] @ G.T) @ Q[1])
        assert abs(a - b) <= 1e-10
        assert abs(X.angle_deg(G @ Q[0], G @ Q[1]) - X.angle_deg(Q[0], Q[1])) <= 1e-10
    R10 = X._rot(rng, math.radians(10.0))
    assert abs(X.angle_deg(Q[0], Q[0] @ R10) - 10.0) <= 1e-10 and X.angle_deg(Q[0], Q[0]) == 0.0


# ------------------------------------------------------------------------------------------------ CPU: the kernel's sequence
@pytest.mark.parametrize("key", [c for c in CASES if c[0] == 5 or c[1] == 65], ids=_ID)
def test_emulation_stays_inside_the_bars(key):
    for padded in (False, True):
        case, ref, bar = prepared(key, padded)
        emu = X.emulate(case)
        check_all(emu, ref, bar, "emulate " + _ID(key))
        X.check(emu["sums"], ref["sums"], bar["sums"], "emulate sums")
        acc, abar = X.accumulate([emu], [bar])
        racc, _ = X.accumulate([ref], [bar])
        X.check(acc, racc, abar, "emulate accumulator")
        assert_identical_is_zero(case, emu["ps"], "emulate")


def test_every_kind_is_generated_and_decided_as_meant():
    seen = set()
    for key in CASES:
        case, ref, _ = prepared(key)
        seen |= set(case["kinds"])
        for b, kind in enumerate(case["kinds"]):
            assert ref["ps"][b, 0] == (1.0 if kind in ("nonortho", "nan_extr") else 0.0), (key, b, kind)
            if kind in ("narrow", "identical"):
                assert ref["ps"][b, 14] == 0 and ref["ps"][b, 10] > 0         # no triangulation; the other metrics are fed
            if kind in ("consistent", "shifted"):
                assert ref["ps"][b, 14] == X.NJ
            if kind == "zero_conf":
                assert ref["ps"][b, 10] == 14 and ref["ps"][b, 11] == 16 and ref["ps"][b, 14] == 10
            if kind == "nan_kp":
                assert ref["ps"][b, 10] == 21 and ref["ps"][b, 11] == 21 and ref["ps"][b, 14] == 20
            if kind == "shifted":
                assert abs(ref["ps"][b, 5] - 0.3) < 1e-5 and abs(ref["ps"][b, 6] - 10.0) < 1e-3 and abs(ref["ps"][b, 7] - 5.0) < 1e-3
    assert seen == set(X.KINDS)


@pytest.mark.parametrize("mutation", X.MUTATIONS)
def test_mutations_are_rejected(mutation):
    rejected = []
    for key in (CASES[16 + 4], CASES[16 + 5], CASES[16 + 7]):                    # B = 5 at V = 65, 1023, 10475
        case, ref, bar = prepared(key)
        mut = X.emulate(case, mutation)
        for name in ("ps", "tri"):
            try:
                X.check(mut[name], ref[name], bar[name], name)
            except AssertionError:
                rejected.append((key, name))
    assert rejected, "no output of any case rejects %s" % mutation


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda", 0)


def _bit_equal(a, b):
    for k in ("ps", "tri", "acc"):
        assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), k


def _twice(case, what, **kw):
    a, b = X.run_gpu(case, _dev(), **kw), X.run_gpu(case, _dev(), **kw)
    for r in (a, b):
        assert r["guards_ok"], what + ": a guard band was written"
        assert r["inputs_ok"], what + ": an input was changed"
    _bit_equal(a, b)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("key", CASES, ids=_ID)
def test_update_against_fp64(key):
    for padded in (False, True):
        case, ref, bar = prepared(key, padded)
        what = "%s %s" % (_ID(key), "padded" if padded else "dense")
        a = _twice(case, what, skew=padded)
        worst = check_all(a, ref, bar, what)
        worst["acc"] = check_acc(a["acc"], [ref], [bar], what)
        print("%s worst err / bar: %s" % (what, {k: round(x, 3) for k, x in worst.items()}))
        assert_identical_is_zero(case, a["ps"], what)
        c = X.run_gpu(case, _dev(), per_sample=False, skew=padded)               # without the optional outputs: the same sums
        assert c["guards_ok"] and c["acc"].tobytes() == a["acc"].tobytes()
        alone = X.run_triangulate(case, _dev())
        assert alone.tobytes() == a["tri"].tobytes(), what + ": apg_xview_triangulate gives another tri"


@pytest.mark.gpu
def test_every_kind_at_the_production_vertex_count():
    case = X.make_case(len(X.KINDS), 22, 127, 10475, True, "aa", "trans", seed=4, kinds=X.KINDS)
    ref = X.reference(case)
    bar = X.bars(case, ref)
    a = _twice(case, "production", skew=True)
    check_all(a, ref, bar, "production")
    check_acc(a["acc"], [ref], [bar], "production")
    assert_identical_is_zero(case, a["ps"], "production")
    assert a["acc"][0] == len(X.KINDS) and a["acc"][1] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("feed,root,V", [((), None, 0), (("reproj",), "joint0", 65), (("tri", "trans"), "trans", 0), (("rot",), None, 1025)],
                         ids=["joints_only", "reproj_only", "tri_only", "rot_only"])
def test_only_what_is_fed_is_counted(feed, root, V):
    case = X.make_case(5, 22, 22, V, False, "rotmat", root, seed=7, feed=feed, kinds=["consistent", "shifted", "nonortho", "zero_conf", "narrow"])
    ref = X.reference(case)
    bar = X.bars(case, ref)
    a = _twice(case, "feed %s" % (feed,))
    check_all(a, ref, bar, "feed %s" % (feed,))
    check_acc(a["acc"], [ref], [bar], "feed %s" % (feed,))
    fed = {X.Q_NROOT: root is not None, X.Q_NVERT: V > 0, X.Q_NVROOT: V > 0 and root is not None, X.Q_NTRANS: "trans" in feed,
           X.Q_NROT: "rot" in feed, X.Q_NRP: "reproj" in feed, X.Q_NTRI: "tri" in feed}
    for q, on in fed.items():
        assert a["acc"][1 + q] == (4.0 if on else 0.0), (q, on, a["acc"])


@pytest.mark.gpu
@pytest.mark.parametrize("V", [0, 65, 10475])
def test_three_updates_equal_one_reference_over_their_concatenation(V):
    cases = [X.make_case(B, 22, 127, V, False, seed=10 + i) for i, B in enumerate((5, 1, 7))]

    def sequence():
        acc = None
        for c in cases:
            r = X.run_gpu(c, _dev(), acc_init=acc, per_sample=False)
            assert r["guards_ok"] and r["inputs_ok"]
            acc = r["acc"]
        return acc
    acc = sequence()
    whole = X.concat_cases(cases)
    ref = X.reference(whole)
    check_acc(acc, [ref], [X.bars(whole, ref)], "three updates")
    assert acc[0] == 13
    assert acc.tobytes() == sequence().tobytes()
