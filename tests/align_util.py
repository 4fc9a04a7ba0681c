"""Shared by test_align_fp64.py, test_align_abi.py and test_mesh_metrics_module.py: the fp64 reference of apg_align_update
(airpose_amd/csrc/eval_align.hip) on numpy.linalg.svd, the fp64 host emulation of the kernel's sequence (pivoted moments, Horn's
4 x 4 matrix, fixed-sweep Jacobi), the error bars counted from that sequence, the cases and the GPU call.  The derivation of the bars
is in test_align_fp64.py's docstring."""
import numpy as np
import torch

from eval_util import GuardedCall

U = 2.0 ** -24
U64 = 2.0 ** -53
ACC = 5                                  # include/airpose_grad.h: APG_ALIGN_ACC_PER_VIEW
PER_VIEW = 4                             # APG_ALIGN_PER_VIEW
NT_SMALL, NT_BIG = 64, 1024              # eval_align.hip
SWEEPS = 6
MUTATIONS = ("reflection_fix_dropped", "scale_from_q", "moments_fp32_unshifted", "root_from_wrong_set")
KINDS = ("far", "similar", "mirror", "same", "coincident", "collinear")
SIZES = (1, 2, 3, 22, 63, 64, 65, 1023, 1024, 1025, 10475)
PAD = 1e30                               # what lies between the samples of a padded array: reading it wrecks every sum


# ------------------------------------------------------------------------------------------------ the reference
def solve_svd(P, Q):
    """least-squares similarity of P onto Q ((N, 3) fp64 each) by the header's formula -> dict(s, R, t, mu_p, mu_q, sigma, d, var)"""
    mu_p, mu_q = P.mean(0), Q.mean(0)
    a, b = P - mu_p, Q - mu_q
    var = float((a * a).sum())
    K = b.T @ a
    Um, S, Vt = np.linalg.svd(K)
    d = 1.0 if np.linalg.det(Um) * np.linalg.det(Vt) >= 0 else -1.0
    D = np.diag([1.0, 1.0, d])
    if var == 0.0:
        s, R = 0.0, np.eye(3)
    else:
        R = Um @ D @ Vt
        s = float((S * np.array([1.0, 1.0, d])).sum()) / var
    return dict(s=s, R=R, t=mu_q - s * R @ mu_p, mu_p=mu_p, mu_q=mu_q, sigma=S, d=d, var=var)


def errors(P, Q, rp, rq, sol):
    """the three means of one sample in fp64"""
    e_abs = np.linalg.norm(P - Q, axis=1).mean()
    e_root = np.linalg.norm((P - rp) - (Q - rq), axis=1).mean()
    e_pa = np.linalg.norm(sol["s"] * (P - sol["mu_p"]) @ sol["R"].T + (sol["mu_q"] - Q), axis=1).mean()
    return np.array([e_abs, e_root, e_pa])


def reference_sample(P, Q, rp, rq):
    P, Q, rp, rq = (np.asarray(x, dtype=np.float64) for x in (P, Q, rp, rq))
    sol = solve_svd(P, Q)
    sol["err"] = errors(P, Q, rp, rq, sol)
    return sol


def points(case, v, which):
    """(B, N, 3) view of the pred / gt array of view v"""
    return case["view"][v][which][:, :3 * case["N"]].reshape(case["B"], case["N"], 3)


def _run(case, fn):
    views, B = case["views"], case["B"]
    err, tr, sols = np.zeros((views, B, 3)), np.zeros((views, B, 13)), []
    for v in range(views):
        d = case["view"][v]
        row = []
        for b in range(B):
            sol = fn(points(case, v, "pred")[b], points(case, v, "gt")[b], d["pred_root"][b, :3], d["gt_root"][b, :3])
            err[v, b] = sol["err"]
            tr[v, b] = np.concatenate([[sol["s"]], np.asarray(sol["R"]).reshape(9), sol["t"]])
            row.append(sol)
        sols.append(row)
    return dict(err=err, transform=tr, sols=sols)


def reference(case):
    """the header's semantics in fp64 on exactly the fp32 values the kernel receives -> err (views, B, 3), transform (views, B, 13)
    and the per-sample solutions"""
    return _run(case, reference_sample)


# ------------------------------------------------------------------------------------------------ the kernel's sequence on the host
def _jacobi4(A):
    """eval_align.hip's horn_solve loop: SWEEPS cyclic sweeps, -> (diagonal, eigenvectors in columns)"""
    A = A.copy()
    V = np.eye(4)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(SWEEPS):
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = A[p, q]
                    zero = apq == 0.0
                    th = (A[q, q] - A[p, p]) / (2.0 * (1.0 if zero else apq))
                    t = 0.0 if zero else np.copysign(1.0, th) / (abs(th) + np.sqrt(th * th + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    A[p, p] -= t * apq
                    A[q, q] += t * apq
                    A[p, q] = A[q, p] = 0.0
                    for k in range(4):
                        if k != p and k != q:
                            x, y = A[k, p], A[k, q]
                            A[k, p] = A[p, k] = c * x - s * y
                            A[k, q] = A[q, k] = s * x + c * y
                    x, y = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * x - s * y, s * x + c * y
    return np.diag(A).copy(), V


def solve_horn(Kc, var):
    """(lambda, R) of the centred moments as the kernel forms them, then the degenerate rule"""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = Kc[0, 0], Kc[1, 0], Kc[2, 0], Kc[0, 1], Kc[1, 1], Kc[2, 1], Kc[0, 2], Kc[1, 2], Kc[2, 2]
    A = np.array([[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]])
    lam_all, V = _jacobi4(A)
    k = 0
    for j in range(1, 4):
        if lam_all[j] > lam_all[k]:
            k = j
    w, x, y, z = V[:, k]
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    inv = 1.0 / ((ww + xx) + (yy + zz))
    R = np.array([[((ww + xx) - yy) - zz, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), ((ww - xx) + yy) - zz, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), ((ww - xx) - yy) + zz]]) * inv
    if not var > 0.0:
        return 0.0, np.eye(3)
    return lam_all[k] / var, R


def _norm3_f32(d):
    """sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0))) on float32 components (an fma is formed in fp64, where the product is exact)"""
    d = d.astype(np.float32)
    t = (d[:, 0] * d[:, 0]).astype(np.float32)
    t = (d[:, 1].astype(np.float64) * d[:, 1] + t).astype(np.float32)
    t = (d[:, 2].astype(np.float64) * d[:, 2] + t).astype(np.float32)
    return np.sqrt(t).astype(np.float64)


def emulate_sample(P, Q, rp, rq, mutation=None):
    P32, Q32 = np.asarray(P, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    P, Q, rp, rq = (np.asarray(x, dtype=np.float64) for x in (P, Q, rp, rq))
    N = P.shape[0]
    n = float(N)
    if mutation == "moments_fp32_unshifted":
        f = np.float32
        sp, sq = P32.sum(0, dtype=f), Q32.sum(0, dtype=f)
        spp = (P32 * P32).sum(dtype=f)
        K = (Q32[:, :, None] * P32[:, None, :]).sum(0, dtype=f)
        var = float(f(spp - f(f(sp @ sp) / f(n))))
        Kc = (K - np.outer(sq, sp).astype(f) / f(n)).astype(np.float64)
        mu_p, mu_q = (sp / f(n)).astype(np.float64), (sq / f(n)).astype(np.float64)
    else:
        cp, cq = P[0], Q[0]
        a, b = P - cp, Q - cq
        sp, sq = a.sum(0), b.sum(0)
        spp = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).sum()
        K = b.T @ a
        var = spp - ((sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]) / n
        Kc = K - np.outer(sq, sp) / n
        mu_p, mu_q = cp + sp / n, cq + sq / n
    if mutation == "scale_from_q":
        var = float(((Q - mu_q) ** 2).sum())
    if mutation == "reflection_fix_dropped":
        Um, S, Vt = np.linalg.svd(Kc)
        s, R = (float(S.sum()) / var, Um @ Vt) if var > 0 else (0.0, np.eye(3))
    else:
        s, R = solve_horn(Kc, var)
    if mutation == "root_from_wrong_set":
        rp = rq
    sol = dict(s=s, R=R, t=mu_q - s * R @ mu_p, mu_p=mu_p, mu_q=mu_q)
    d_abs = P - Q
    d_root = (P - rp) - (Q - rq)
    d_pa = s * ((P - mu_p) @ R.T) + (mu_q - Q)
    sol["err"] = np.array([_norm3_f32(d).sum() / n for d in (d_abs, d_root, d_pa)])
    return sol


def emulate(case, mutation=None):
    return _run(case, lambda P, Q, rp, rq: emulate_sample(P, Q, rp, rq, mutation))


# ------------------------------------------------------------------------------------------------ the bars
def classify(P, sol):
    """"degenerate" (all p equal: s = 0, R = I), "collinear" (rank K < 2: only finite and det R = +1) or "regular" """
    if sol["var"] == 0.0:
        return "degenerate"
    return "collinear" if sol["sigma"][1] < 1e-6 * sol["sigma"][0] or sol["sigma"][0] == 0.0 else "regular"


def gap(sol):
    """sigma_2 + d sigma_3: half the distance of Horn's largest eigenvalue from the next, the conditioning of R"""
    return sol["sigma"][1] + sol["d"] * sol["sigma"][2]


def bars_sample(P, Q, rp, rq, sol):
    """-> dict(err (3,), mean (3,): the same without the final rounding to float, transform (13,), cls).  Entries that carry no bar
    (R, t and pa of a collinear sample) are inf."""
    P, Q, rp, rq = (np.asarray(x, dtype=np.float64) for x in (P, Q, rp, rq))
    N = P.shape[0]
    cls = classify(P, sol)
    e = sol["err"]
    s, R, mu_p, mu_q = abs(sol["s"]), np.abs(sol["R"]), sol["mu_p"], sol["mu_q"]
    a, b = np.abs(P - P[0]).sum(1), np.abs(Q - Q[0]).sum(1)
    summing = (N + 70) * U64                             # the fp64 sums of N terms, the division and what surrounds them
    # moments about the pivots and what the centring subtracts; one Jacobi rotation is 6 roundings on entries of at most 9 sigma_1
    A_K = max(float((a * b).sum()), float(a.sum() * b.sum()) / N)
    dN = (4 * (N + 20) + SWEEPS * 6 * 6 * 9) * U64 * A_K
    dmu_p, dmu_q = (N + 4) * U64 * (a.mean() + np.abs(P[0]).max()), (N + 4) * U64 * (b.mean() + np.abs(Q[0]).max())
    if cls == "regular":
        g = gap(sol)
        dR = 4 * (4 * dN / max(g - 4 * dN, 1e-300))      # eigenvector: |dq| <= |dN|_2 / (gap of N / 2) with |dN|_2 <= 4 dN; R is quadratic in q
        ds = (4 * dN + s * (N + 20) * U64 * float((a * a).sum())) / sol["var"]
    elif cls == "degenerate":
        dR = ds = 0.0
    else:
        dR = ds = np.inf
    c1 = np.abs(P - mu_p).sum(1)                          # |p - mu_p|_1
    fp64_pa = 10 * U64 * (s * c1 + np.abs(mu_q - Q).sum(1)).mean()
    moved_pa = (ds * c1 + s * 3 * dR * c1).mean() + s * 3 * dmu_p + 3 * dmu_q if cls != "collinear" else np.inf
    fp64_root = 4 * U64 * (np.abs(P - rp).sum(1) + np.abs(Q - rq).sum(1)).mean()
    mean = np.array([4 * U * e[0] + summing * e[0],
                     4 * U * e[1] + summing * e[1] + fp64_root,
                     4 * U * e[2] + summing * e[2] + fp64_pa + moved_pa])
    err = mean + U * e
    t = np.abs(sol["t"])
    Rmu = R @ np.abs(mu_p)
    bt = U * t + dmu_q + ds * Rmu + s * 3 * dR * np.abs(mu_p).sum() + s * 3 * dmu_p + 10 * U64 * (np.abs(mu_q) + s * Rmu)
    if cls == "collinear":
        bt = np.full(3, np.inf)
    tr = np.concatenate([[U * s + ds], (U * R + dR).reshape(9), bt])
    return dict(err=err, mean=mean, transform=tr, cls=cls)


def bars(case, ref):
    views, B = case["views"], case["B"]
    out = dict(err=np.zeros((views, B, 3)), mean=np.zeros((views, B, 3)), transform=np.zeros((views, B, 13)), cls=[])
    for v in range(views):
        d = case["view"][v]
        row = []
        for b in range(B):
            r = bars_sample(points(case, v, "pred")[b], points(case, v, "gt")[b], d["pred_root"][b, :3], d["gt_root"][b, :3],
                            ref["sols"][v][b])
            for k in ("err", "mean", "transform"):
                out[k][v, b] = r[k]
            row.append(r["cls"])
        out["cls"].append(row)
    return out


def accumulate(refs, bars_list, roots_list, views):
    """the accumulator ((2, 5) fp64) of a sequence of updates and its bar: the samples' bars summed plus one fp64 rounding per
    addition.  roots_list: per update, per view, whether roots were given"""
    acc, bar = np.zeros((2, ACC)), np.zeros((2, ACC))
    for ref, b, roots in zip(refs, bars_list, roots_list):
        n = ref["err"].shape[1]
        for v in range(views):
            acc[v, 0] += n
            if roots[v]:
                acc[v, 4] += n
            for k in range(3):
                if k == 1 and not roots[v]:
                    continue
                s = ref["err"][v, :, k].sum()
                acc[v, 1 + k] += s
                bar[v, 1 + k] += b["mean"][v, :, k].sum() + (n + 2) * U64 * (abs(s) + abs(acc[v, 1 + k]))
    return acc, bar


def check(got, ref, bar, what):
    """|got - ref| <= bar element-wise, exact where the bar is 0, nothing asked where it is inf; got must be finite everywhere.
    -> the worst err / bar"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, "%s: shape %s against %s" % (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: %d non-finite elements" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    zero = bar == 0
    assert not (err[zero] > 0).any(), "%s: %d elements differ where the bar is 0" % (what, int((err[zero] > 0).sum()))
    fin = np.isfinite(bar) & ~zero
    ratio = np.zeros_like(err)
    ratio[fin] = err[fin] / bar[fin]
    i = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    assert ratio.size == 0 or ratio[i] <= 1, "%s: err / bar %.3f at %s (got %.17g, ref %.17g, bar %.3g)" % (
        what, ratio[i], i, got[i], ref[i], bar[i])
    return float(ratio.max()) if ratio.size else 0.0


def check_rotations(tr, cls, what):
    """every R finite with det = +1: the float rounding of a rotation's entries moves its determinant by at most
    u sum |R_ij| |cofactor_ij| = 3 u; 4 u leaves room for the fp64 solve"""
    for v in range(tr.shape[0]):
        for b in range(tr.shape[1]):
            R = np.asarray(tr[v, b, 1:10], dtype=np.float64).reshape(3, 3)
            assert np.isfinite(tr[v, b]).all(), (what, v, b)
            assert abs(np.linalg.det(R) - 1.0) <= 4 * U, "%s: det R = %.9g at view %d sample %d (%s)" % (what, np.linalg.det(R), v, b, cls[v][b])


# ------------------------------------------------------------------------------------------------ cases
def _rot(rng, angle=None):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.3, 2.8) if angle is None else angle
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_sample(kind, N, rng):
    """-> P, Q (N, 3) float32, rp, rq (3,) float32.  Q: a body of 0.5 m extent at 10 m depth"""
    Q = rng.uniform(-0.25, 0.25, (N, 3)) * np.array([0.6, 1.0, 0.4]) + np.array([0.3, -0.2, 10.0])
    if N == 3:                                           # three random points are often a sliver: a turned, jittered fat triangle
        Q = 0.2 * np.array([[1.0, 0.0, 0.0], [-0.5, 0.85, 0.1], [-0.5, -0.85, -0.1]]) @ _rot(rng).T + rng.normal(0, 0.01, (3, 3)) \
            + np.array([0.3, -0.2, 10.0])
    cen = Q.mean(0)
    if kind == "far":                                   # a plausible prediction: a few degrees, centimetres
        P = (Q - cen) @ _rot(rng, 0.1).T * 1.05 + cen + rng.normal(0, 0.03, (N, 3)) + np.array([0.05, -0.02, 0.4])
    elif kind == "similar":                              # q = s0 R0 p + t0 up to the rounding of p
        P = (Q - cen) @ _rot(rng).T * 0.8 + np.array([-0.4, 0.1, 7.0])
    elif kind == "mirror":
        P = (Q - cen) * np.array([-1.0, 1.0, 1.0]) + cen + rng.normal(0, 0.01, (N, 3))
    elif kind == "same":
        P = Q
    elif kind == "coincident":
        P = np.tile(Q[:1] + 0.1, (N, 1))
    elif kind == "collinear":
        tq, tp = rng.uniform(-0.25, 0.25, (N, 1)), rng.uniform(-0.25, 0.25, (N, 1))
        Q = cen + tq * np.array([0.6, 0.64, 0.48])
        P = cen + 0.1 + (tq + 0.02 * tp) * np.array([0.0, 0.8, -0.6])
    else:
        raise ValueError(kind)
    P, Q = P.astype(np.float32), Q.astype(np.float32)
    rq = Q[0] + np.float32(0.01)
    rp = rq.copy() if kind == "same" else (P[0] - np.float32(0.02))
    return P, Q, rp.astype(np.float32), rq.astype(np.float32)


def assert_conditions(kind, N, sol):
    """the generator's own conditions on the reference's singular values: R means something only where they hold"""
    if N < 3 or kind in ("coincident", "collinear"):
        return
    s = sol["sigma"]
    assert s[1] >= 0.05 * s[0], "%s N=%d: sigma %s is close to collinear" % (kind, N, s)
    assert gap(sol) >= 0.05 * s[0], "%s N=%d: sigma %s, d = %g: R is ill-conditioned" % (kind, N, s, sol["d"])
    if kind == "mirror" and N > 3:
        assert sol["d"] < 0, "%s N=%d is not a reflection case" % (kind, N)


def make_case(views, B, N, padded, seed=0, kinds=None):
    """sample b of view v is of kind kinds[v][b] (default: KINDS cycled from an offset that moves with N, B and the view).
    padded: sample strides 3 N + 7 and 5 (roots) with PAD between the samples, else 3 N and 3"""
    rng = np.random.default_rng(100000 * seed + 1000 * SIZES.index(N) if N in SIZES else 100000 * seed + N)
    sp, sq, sr = (3 * N + 7, 3 * N + 4, 5) if padded else (3 * N, 3 * N, 3)
    case = dict(B=B, views=views, N=N, stride_p=sp, stride_q=sq, stride_rp=sr, stride_rq=sr, view=[])
    off = (SIZES.index(N) if N in SIZES else N) + B
    for v in range(views):
        ks = kinds[v] if kinds is not None else [KINDS[(off + 3 * v + b) % len(KINDS)] for b in range(B)]
        d = dict(kinds=list(ks), pred=np.full((B, sp), PAD, np.float32), gt=np.full((B, sq), PAD, np.float32),
                 pred_root=np.full((B, sr), PAD, np.float32), gt_root=np.full((B, sr), PAD, np.float32))
        for b, kind in enumerate(ks):
            P, Q, rp, rq = make_sample(kind, N, rng)
            d["pred"][b, :3 * N], d["gt"][b, :3 * N] = P.reshape(-1), Q.reshape(-1)
            d["pred_root"][b, :3], d["gt_root"][b, :3] = rp, rq
            assert_conditions(kind, N, reference_sample(P, Q, rp, rq))
        case["view"].append(d)
    return case


def concat_cases(cases):
    out = dict(cases[0])
    out["B"] = sum(c["B"] for c in cases)
    out["view"] = []
    for v in range(out["views"]):
        d = {k: np.concatenate([c["view"][v][k] for c in cases]) for k in ("pred", "gt", "pred_root", "gt_root")}
        d["kinds"] = sum((c["view"][v]["kinds"] for c in cases), [])
        out["view"].append(d)
    return out


# ------------------------------------------------------------------------------------------------ the GPU call
def run_gpu(case, dev, roots=(True, True), acc_init=None, per_sample=True, skew=False):
    """one apg_align_update into fresh guarded buffers -> dict(err, transform, acc (2, 5), guards_ok, inputs_ok), numpy on the host.
    roots[v]: whether view v's roots are passed.  skew: every input starts one float past a 16-byte boundary"""
    from airpose_amd import _native_grad as G
    L, vp = G.lib(), G.vp
    B, views, N = case["B"], case["views"], case["N"]
    total = sum(int(np.prod(case["view"][v][k].shape)) + 80 for v in range(views) for k in ("pred", "gt", "pred_root", "gt_root"))
    gc = GuardedCall(dev, 8192 + total + views * B * 16 * 2)
    put = lambda x: gc.put(torch.from_numpy(x), skew)
    table = []
    for v in range(views):
        d = case["view"][v]
        table += [put(d["pred"]), put(d["gt"])] + ([put(d["pred_root"]), put(d["gt_root"])] if roots[v] else [None, None])
    err = gc.ar.take((views, B, 3)) if per_sample else None
    tr = gc.ar.take((views, B, 13)) if per_sample else None
    nbytes = L.apg_align_workspace_bytes(B, views, N)
    assert nbytes == B * views * 24
    acc, ws = gc.sums(ACC, acc_init, nbytes)
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    return gc.run(G, lambda: L.apg_align_update(B, views, N, case["stride_p"], case["stride_q"], case["stride_rp"], case["stride_rq"],
                                                G.ptrs(table), vp(err), vp(tr), vp(acc), vp(ws), nbytes, G.stream(dev)),
                  "apg_align_update", lambda: dict(err=host(err), transform=host(tr), acc=host(acc)))
