"""Shared by test_xview_fp64.py, test_xview_abi.py and test_xview_module.py: the fp64 reference of apg_xview_update and
apg_xview_triangulate (airpose_amd/csrc/xview_metrics.hip) on numpy.linalg.inv and numpy.linalg.lstsq, the host emulation of the
kernel's sequence (the transpose as the inverse, fp64 carries, fp32 norms, the cofactor solve of the normal equations), the error bars
counted from that sequence, the cases and the GPU calls.  The derivation of the bars is in test_xview_fp64.py's docstring."""
import math

import numpy as np
import torch

import eval_util as E
from align_util import _norm3_f32, check  # noqa: F401  (check: |got - ref| <= bar, exact where the bar is 0)
from eval_util import GuardedCall

U = 2.0 ** -24
U64 = 2.0 ** -53
ACC = 26                                 # include/airpose_grad.h: APG_XVIEW_ACC
PS = 16                                  # APG_XVIEW_PER_SAMPLE
PER_VIEW = 9                             # APG_XVIEW_PER_VIEW
NJ = 22
NS = 24                                  # sums per sample: accumulator slots 1 .. 24
PAD = 1e30                               # what lies between the samples of a padded array: reading it wrecks every sum
ORTHO_GATE = 1e-3
MIN_ANGLE_DEG = 1.0
MIN_SIN2 = math.sin(math.radians(MIN_ANGLE_DEG)) ** 2
ENTRIES = ("joints", "extr", "verts", "root", "trans", "rot", "j2d", "kp", "intr")
KINDS = ("consistent", "shifted", "identical", "nonortho", "nan_extr", "zero_conf", "nan_kp", "narrow")
SIZES = (0, 1, 63, 64, 65, 1023, 1025, 10475)
MUTATIONS = ("extr_not_inverted", "root_not_subtracted", "reproj_unweighted", "tri_weighted", "pose_mean_over_22")
# sums (slot - 1) and per-sample columns
(Q_SKIP, Q_JW, Q_JR, Q_NROOT, Q_VW, Q_VR, Q_NVERT, Q_NVROOT, Q_TRANS, Q_NTRANS, Q_ORIENT, Q_POSE, Q_NROT, Q_RP0, Q_RP1, Q_RS0, Q_RS1,
 Q_RN0, Q_RN1, Q_NRP, Q_TRI0, Q_TRI1, Q_TRIN, Q_NTRI) = range(NS)
COUNTS = (Q_SKIP, Q_NROOT, Q_NVERT, Q_NVROOT, Q_NTRANS, Q_NROT, Q_RS0, Q_RS1, Q_RN0, Q_RN1, Q_NRP, Q_TRIN, Q_NTRI)
# per-sample column -> the sum it shows (the two tri columns are divided by tri_n)
PS_OF = {0: Q_SKIP, 1: Q_JW, 2: Q_JR, 3: Q_VW, 4: Q_VR, 5: Q_TRANS, 6: Q_ORIENT, 7: Q_POSE, 8: Q_RP0, 9: Q_RP1, 10: Q_RN0, 11: Q_RN1,
         12: Q_TRI0, 13: Q_TRI1, 14: Q_TRIN}


# ------------------------------------------------------------------------------------------------ small pieces
def angle_deg(A, B):
    """the header's angle formula on D = A^T B, fp64"""
    D = A.T @ B
    ax = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return math.degrees(math.atan2(math.sqrt(float(ax @ ax)), float(np.trace(D)) - 1.0))


def rotmats(case, v, emu=False):
    """(B, 22, 3, 3) fp64 of view v's rotations: the matrices as given, or the vectors through tgm's formula (fp64, or as the
    kernel does it in fp32); -> (Q, conv: eval_util's intermediates of the fp64 conversion or None)"""
    B = case["B"]
    raw = view(case, v, "rot")
    if case["rot"] == "rotmat":
        return raw.reshape(B, NJ, 3, 3).astype(np.float64), None
    r = torch.from_numpy(raw.reshape(B * NJ, 3).copy())
    Q32 = E.aa_to_rotmat(r, emu=True)[0].double().numpy().reshape(B, NJ, 3, 3)
    Q64, conv = E.aa_to_rotmat(r.double())
    return (Q32 if emu else Q64.numpy().reshape(B, NJ, 3, 3)), conv


def view(case, v, name):
    """(B, size) view of an entry's values, without what pads it"""
    return case["view"][v][name][:, :case["size"][name]]


def cam_of(e12):
    e = np.asarray(e12, dtype=np.float64).reshape(3, 4)
    return e[:, :3], e[:, 3]


def skipped(case, b):
    for v in range(2):
        R, t = cam_of(view(case, v, "extr")[b][:12])
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            return True
        if np.abs(R.T @ R - np.eye(3)).max() > ORTHO_GATE:
            return True
    return False


def tri_reference(e0, e1, K0, K1, kp0, kp1, min_sin2):
    """lstsq_triangulation (the reference's utils/geometry.py) for two cameras -> (T, valid, singular values, |b|)"""
    a, bb, rays, ok = [], [], [], True
    for e, K, kp in ((e0, K0, kp0), (e1, K1, kp1)):
        R, t = cam_of(e)
        extr = np.concatenate([R, t[:, None]], 1)
        kp = np.asarray(kp, dtype=np.float64)
        ok = ok and bool(np.isfinite(kp).all()) and kp[2] > 0
        with np.errstate(all="ignore"):
            n = np.linalg.inv(np.asarray(K, dtype=np.float64).reshape(3, 3)) @ np.array([kp[0], kp[1], 1.0])
        a.append(np.outer(n[0:2], extr[2, 0:-1]) - extr[0:2, 0:-1])
        bb.append(extr[0:-1, -1] - extr[-1, -1] * n[0:2])
        rays.append(np.linalg.inv(R) @ np.array([n[0], n[1], 1.0]))
    Am, Bv = np.concatenate(a), np.concatenate(bb)
    if not (np.isfinite(Am).all() and np.isfinite(Bv).all()):
        return np.zeros(3), False, np.ones(3), 0.0
    x, _, _, sv = np.linalg.lstsq(Am, Bv, rcond=None)
    cr = np.cross(rays[0], rays[1])
    s2 = float(cr @ cr) / (float(rays[0] @ rays[0]) * float(rays[1] @ rays[1]))
    return x, bool(ok and s2 >= min_sin2 and np.isfinite(x).all()), sv, float(np.linalg.norm(Bv))


def tri_emulated(e0, e1, K0, K1, kp0, kp1, min_sin2, weighted=False):
    """the kernel's triangulate(): normal equations by cofactors"""
    M, y, rays, ok = np.zeros((3, 3)), np.zeros(3), [], True
    with np.errstate(all="ignore"):
        for e, K, kp in ((e0, K0, kp0), (e1, K1, kp1)):
            R, t = cam_of(e)
            K = np.asarray(K, dtype=np.float64).reshape(3, 3)
            kp = np.asarray(kp, dtype=np.float64)
            ok = ok and bool(np.isfinite(kp).all()) and kp[2] > 0
            n = np.array([(kp[0] - K[0, 2]) / K[0, 0], (kp[1] - K[1, 2]) / K[1, 1]])
            ok = ok and bool(np.isfinite(n).all())
            for r in range(2):
                arow = n[r] * R[2] - R[r]
                b = t[r] - t[2] * n[r]
                w = kp[2] if weighted else 1.0
                M += w * np.outer(arow, arow)
                y += w * arow * b
            rays.append(R.T @ np.array([n[0], n[1], 1.0]))
        c = np.array([[M[1, 1] * M[2, 2] - M[1, 2] * M[1, 2], M[0, 2] * M[1, 2] - M[0, 1] * M[2, 2], M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1]],
                      [0, M[0, 0] * M[2, 2] - M[0, 2] * M[0, 2], M[0, 1] * M[0, 2] - M[0, 0] * M[1, 2]],
                      [0, 0, M[0, 0] * M[1, 1] - M[0, 1] * M[0, 1]]])
        c = c + np.triu(c, 1).T
        det = (M[0, 0] * c[0, 0] + M[0, 1] * c[0, 1]) + M[0, 2] * c[0, 2]
        T = (c @ y) / det
        cr = np.cross(rays[0], rays[1])
        s2 = float(cr @ cr) / (float(rays[0] @ rays[0]) * float(rays[1] @ rays[1]))
    valid = bool(ok and s2 >= min_sin2 and np.isfinite(T).all())
    return (T if valid else np.zeros(3)), valid


# ------------------------------------------------------------------------------------------------ the reference and the emulation
def _run(case, emu, mutation=None, min_sin2=MIN_SIN2):
    """-> dict(sums (B, 24): each sample's share of accumulator slots 1 .. 24, ps (B, 16), tri (B, 22, 4), aux: what the bars need)"""
    B, nj, V, feed = case["B"], case["nj"], case["V"], case["feed"]
    sums, ps, tri = np.zeros((B, NS)), np.zeros((B, PS)), np.zeros((B, NJ, 4))
    aux = [None] * B
    Q = [rotmats(case, v, emu) for v in range(2)] if "rot" in feed else None
    f32 = (lambda d: _norm3_f32(np.atleast_2d(d))) if emu else (lambda d: np.linalg.norm(np.atleast_2d(d), axis=1))
    for b in range(B):
        if skipped(case, b):
            sums[b, Q_SKIP] = ps[b, 0] = 1.0
            continue
        cams = [cam_of(view(case, v, "extr")[b][:12]) for v in range(2)]
        if emu:
            inv = [c[0] if mutation == "extr_not_inverted" else c[0].T for c in cams]
        else:
            inv = [np.linalg.inv(np.vstack([np.concatenate([c[0], c[1][:, None]], 1), [0, 0, 0, 1.0]]))[:3, :3] for c in cams]
        pts = lambda name, v, n: view(case, v, name)[b][:3 * n].reshape(n, 3).astype(np.float64)
        carry = lambda v, p, o: (p - o) @ inv[v].T
        gap = lambda p0, p1, o0, o1: f32(carry(0, p0, o0) - carry(1, p1, o1))
        x = aux[b] = dict(inv=inv, cams=cams)
        J0, J1 = pts("joints", 0, max(nj, NJ if "tri" in feed else nj)), pts("joints", 1, max(nj, NJ if "tri" in feed else nj))
        roots = None
        if case["root"] is not None:
            roots = [view(case, v, "root")[b][:3].astype(np.float64) for v in range(2)]
        x["g_jw"] = gap(J0[:nj], J1[:nj], cams[0][1], cams[1][1])
        sums[b, Q_JW] = x["g_jw"].sum() / nj
        if roots is not None:
            x["g_jr"] = x["g_jw"] if mutation == "root_not_subtracted" else gap(J0[:nj], J1[:nj], roots[0], roots[1])
            sums[b, Q_JR], sums[b, Q_NROOT] = x["g_jr"].sum() / nj, 1.0
        if V:
            P0, P1 = pts("verts", 0, V), pts("verts", 1, V)
            x["g_vw"] = gap(P0, P1, cams[0][1], cams[1][1])
            sums[b, Q_VW], sums[b, Q_NVERT] = x["g_vw"].sum() / V, 1.0
            if roots is not None:
                x["g_vr"] = x["g_vw"] if mutation == "root_not_subtracted" else gap(P0, P1, roots[0], roots[1])
                sums[b, Q_VR], sums[b, Q_NVROOT] = x["g_vr"].sum() / V, 1.0
        if "trans" in feed:
            s0, s1 = pts("trans", 0, 1), pts("trans", 1, 1)
            x["g_t"] = gap(s0, s1, cams[0][1], cams[1][1])
            sums[b, Q_TRANS], sums[b, Q_NTRANS] = x["g_t"][0], 1.0
        if Q is not None:
            sums[b, Q_ORIENT] = angle_deg(inv[0] @ Q[0][0][b, 0], inv[1] @ Q[1][0][b, 0])
            pose = [angle_deg(Q[0][0][b, j], Q[1][0][b, j]) for j in range(1, NJ)]
            x["pose"] = pose
            sums[b, Q_POSE], sums[b, Q_NROT] = sum(pose) / (22 if mutation == "pose_mean_over_22" else 21), 1.0
        kps = [view(case, v, "kp")[b][:3 * NJ].reshape(NJ, 3).astype(np.float64) for v in range(2)] if ("reproj" in feed or "tri" in feed) else None
        if "reproj" in feed:
            for v in range(2):
                pr = view(case, v, "j2d")[b][:2 * NJ].reshape(NJ, 2).astype(np.float64)
                k = kps[v]
                use = np.isfinite(k).all(1) & (k[:, 2] > 0)
                d = (pr - k[:, :2])[use]
                if emu:
                    d32 = d.astype(np.float32)
                    t = (d32[:, 0] * d32[:, 0]).astype(np.float32)
                    dist = np.sqrt((d32[:, 1].astype(np.float64) * d32[:, 1] + t).astype(np.float32)).astype(np.float64)
                else:
                    dist = np.linalg.norm(d, axis=1)
                c = np.ones(int(use.sum())) if mutation == "reproj_unweighted" else k[use, 2]
                sums[b, Q_RN0 + v] = use.sum()
                if c.sum() > 0:
                    sums[b, Q_RP0 + v], sums[b, Q_RS0 + v] = (c * dist).sum() / c.sum(), 1.0
            sums[b, Q_NRP] = 1.0
        if "tri" in feed:
            x["tri"] = []
            for j in range(NJ):
                args = (view(case, 0, "extr")[b][:12], view(case, 1, "extr")[b][:12], view(case, 0, "intr")[b][:9],
                        view(case, 1, "intr")[b][:9], kps[0][j], kps[1][j], min_sin2)
                if emu:
                    T, valid = tri_emulated(*args, weighted=mutation == "tri_weighted")
                    sv, nb = None, None
                else:
                    T, valid, sv, nb = tri_reference(*args)
                x["tri"].append((valid, sv, nb))
                if valid:
                    tri[b, j] = [T[0], T[1], T[2], 1.0]
                    for v, Jv in enumerate((J0, J1)):
                        sums[b, Q_TRI0 + v] += f32(carry(v, Jv[j], cams[v][1]) - T)[0]
                    sums[b, Q_TRIN] += 1
            sums[b, Q_NTRI] = 1.0
        for col, q in PS_OF.items():
            ps[b, col] = sums[b, q]
        if sums[b, Q_TRIN] > 0:
            ps[b, 12], ps[b, 13] = sums[b, Q_TRI0] / sums[b, Q_TRIN], sums[b, Q_TRI1] / sums[b, Q_TRIN]
    return dict(sums=sums, ps=ps, tri=tri, aux=aux)


def reference(case, min_sin2=MIN_SIN2):
    """the header's semantics in fp64 on exactly the fp32 values the kernel receives: numpy.linalg.inv of the 4 x 4 extrinsics,
    numpy.linalg.lstsq for the triangulation, written as in the reference's lstsq_triangulation"""
    return _run(case, False, None, min_sin2)


def emulate(case, mutation=None, min_sin2=MIN_SIN2):
    """the kernel's sequence on the host"""
    return _run(case, True, mutation, min_sin2)


# ------------------------------------------------------------------------------------------------ the bars
def _gap_bar(g, inv, cams, P0, P1, o0, o1):
    """per point: 4 u g (the float roundings), what the transpose as the inverse moves, 16 v (|p0 - o0|_1 + |p1 - o1|_1) (fp64)"""
    d0, d1 = np.abs(np.atleast_2d(P0) - o0), np.abs(np.atleast_2d(P1) - o1)
    model = np.linalg.norm(d0 @ np.abs(cams[0][0].T - inv[0]).T + d1 @ np.abs(cams[1][0].T - inv[1]).T, axis=1)
    return 4 * U * g + (1 + 4 * U) * (model + 16 * U64 * (d0.sum(1) + d1.sum(1)))


def bars(case, ref):
    """-> dict(sums (B, 24): the bar of each sample's share of the accumulator, ps (B, 16), tri (B, 22, 4)); counts carry 0"""
    B, nj, V, feed = case["B"], case["nj"], case["V"], case["feed"]
    sums, ps, tri = np.zeros((B, NS)), np.zeros((B, PS)), np.zeros((B, NJ, 4))
    conv = [rotmats(case, v)[1] for v in range(2)] if "rot" in feed else None
    dQ = None
    if conv is not None and conv[0] is not None:
        dQ = [E._conv_bars(c, B).double().numpy().reshape(B, NJ, 9).max(2) for c in conv]      # (B, 22): a bound on every entry
    for b in range(B):
        x = ref["aux"][b]
        if x is None:
            continue
        inv, cams = x["inv"], x["cams"]
        pts = lambda name, v, n: view(case, v, name)[b][:3 * n].reshape(n, 3).astype(np.float64)
        summing = lambda n, val: (n + 70) * U64 * abs(val)
        nJ = max(nj, NJ if "tri" in feed else nj)
        J0, J1 = pts("joints", 0, nJ), pts("joints", 1, nJ)
        t0, t1 = cams[0][1], cams[1][1]
        sums[b, Q_JW] = _gap_bar(x["g_jw"], inv, cams, J0[:nj], J1[:nj], t0, t1).mean() + summing(nj, ref["sums"][b, Q_JW])
        roots = [view(case, v, "root")[b][:3].astype(np.float64) for v in range(2)] if case["root"] is not None else None
        if roots is not None:
            sums[b, Q_JR] = _gap_bar(x["g_jr"], inv, cams, J0[:nj], J1[:nj], roots[0], roots[1]).mean() + summing(nj, ref["sums"][b, Q_JR])
        if V:
            P0, P1 = pts("verts", 0, V), pts("verts", 1, V)
            sums[b, Q_VW] = _gap_bar(x["g_vw"], inv, cams, P0, P1, t0, t1).mean() + summing(V, ref["sums"][b, Q_VW])
            if roots is not None:
                sums[b, Q_VR] = _gap_bar(x["g_vr"], inv, cams, P0, P1, roots[0], roots[1]).mean() + summing(V, ref["sums"][b, Q_VR])
        if "trans" in feed:
            sums[b, Q_TRANS] = _gap_bar(x["g_t"], inv, cams, pts("trans", 0, 1), pts("trans", 1, 1), t0, t1)[0]
        if "rot" in feed:
            q = [dQ[v][b] if dQ is not None else np.zeros(NJ) for v in range(2)]
            model = [np.abs(cams[v][0].T - inv[v]).sum(1).max() for v in range(2)]
            to_deg = lambda dD: math.degrees(4 * dD + 16 * U64 * math.pi)
            sums[b, Q_ORIENT] = to_deg(3 * (1.01 * (q[0][0] + q[1][0]) + model[0] + model[1] + 12 * U64) + 6 * U64)
            pose = [to_deg(3 * 1.01 * (q[0][j] + q[1][j]) + 6 * U64) for j in range(1, NJ)]
            sums[b, Q_POSE] = sum(pose) / 21 + summing(21, ref["sums"][b, Q_POSE])
        for v in range(2):
            sums[b, Q_RP0 + v] = (4 * U + 60 * U64) * ref["sums"][b, Q_RP0 + v]
        if "tri" in feed:
            for j, (valid, sv, nb) in enumerate(x["tri"]):
                if not valid:
                    continue
                T = ref["tri"][b, j, :3]
                kappa = sv[0] / sv[2]                        # the conditioning of the reference's own 4 x 3 system
                dT = 64 * U64 * kappa * kappa * (np.linalg.norm(T) + nb / sv[0])
                tri[b, j, :3] = U * np.abs(T) + dT
                for v, Jv in enumerate((J0, J1)):                # |W_v(p) - T|: one carry, and T's own bar on every component
                    rel = np.abs(Jv[j] - cams[v][1])
                    d = np.linalg.norm((Jv[j] - cams[v][1]) @ inv[v].T - T)
                    model = np.linalg.norm(np.abs(cams[v][0].T - inv[v]) @ rel)
                    sums[b, Q_TRI0 + v] += 4 * U * d + (1 + 4 * U) * (model + 16 * U64 * rel.sum() + math.sqrt(3) * dT)
            for v in range(2):
                sums[b, Q_TRI0 + v] += summing(NJ, ref["sums"][b, Q_TRI0 + v])
        for col, qq in PS_OF.items():
            ps[b, col] = sums[b, qq] + (U * abs(ref["ps"][b, col]) if qq not in COUNTS else 0.0)
        n = ref["sums"][b, Q_TRIN]
        if n > 0:
            for c, qq in ((12, Q_TRI0), (13, Q_TRI1)):
                ps[b, c] = sums[b, qq] / n + (U + 4 * U64) * abs(ref["ps"][b, c])
    return dict(sums=sums, ps=ps, tri=tri)


def accumulate(refs, bars_list):
    """the accumulator ((26,) fp64) of a sequence of updates and its bar: the samples' bars summed plus one fp64 rounding per
    addition"""
    acc, bar = np.zeros(ACC), np.zeros(ACC)
    for ref, b in zip(refs, bars_list):
        n = ref["sums"].shape[0]
        acc[0] += n
        for q in range(NS):
            s = ref["sums"][:, q].sum()
            acc[1 + q] += s
            if q not in COUNTS:
                bar[1 + q] += b["sums"][:, q].sum() + (n + 2) * U64 * (abs(s) + abs(acc[1 + q]))
    return acc, bar


# ------------------------------------------------------------------------------------------------ cases
def _rot(rng, angle=None):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.3, 2.8) if angle is None else angle
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _aa(R):
    """axis-angle of a rotation matrix (angle in (0, pi)), fp64"""
    th = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return ax / np.linalg.norm(ax) * th


def _look_at(C, target, rng):
    """world -> camera [R | t] of a camera at C looking at target (z forward, a random roll)"""
    z = target - C
    z /= np.linalg.norm(z)
    up = rng.standard_normal(3)
    xa = np.cross(up, z)
    xa /= np.linalg.norm(xa)
    R = np.stack([xa, np.cross(z, xa), z])
    return R, -R @ C


def make_sample(kind, nJ, V, rot, rng):
    """-> per view a dict of fp32 arrays joints (nJ, 3), extr (3, 4), verts (V, 3), trans (3,), rot, j2d (nJ, 2), kp (24, 3), intr (3, 3)"""
    assert nJ >= NJ
    centre = rng.uniform(-1.0, 1.0, 3)
    body = lambda n: centre + rng.uniform(-0.25, 0.25, (n, 3)) * np.array([0.6, 1.0, 0.4])
    Xw, Yw, sw = body(nJ), body(V), centre + rng.uniform(-0.05, 0.05, 3)
    Qw = [_rot(rng) for _ in range(NJ)]
    sep = math.radians(0.2) if kind == "narrow" else math.radians(rng.uniform(20.0, 120.0))
    d0 = rng.standard_normal(3)
    d0 /= np.linalg.norm(d0)
    perp = np.cross(d0, rng.standard_normal(3))
    perp /= np.linalg.norm(perp)
    dirs = [d0, math.cos(sep) * d0 + math.sin(sep) * perp]
    dist = rng.uniform(6.0, 10.0, 2)
    if kind == "narrow":                                 # at equal range the rays to every joint stay as close as the cameras
        dist[1] = dist[0]
    out = []
    for v in range(2):
        if kind == "identical":
            R, t = np.eye(3), np.zeros(3)
            X, Y, s, Qr = (Xw - centre) + [0.1, -0.2, 8.0], (Yw - centre) + [0.1, -0.2, 8.0], (sw - centre) + [0.1, -0.2, 8.0], Qw[0]
            Xgt = X
        else:
            R, t = _look_at(centre + dist[v] * dirs[v], centre + rng.uniform(-0.1, 0.1, 3), rng)
        e32 = np.concatenate([R, t[:, None]], 1).astype(np.float32)
        R32, t32 = e32[:, :3].astype(np.float64), e32[:, 3].astype(np.float64)
        if kind != "identical":
            Xv, Yv, sv, Q0, Qb = Xw, Yw, sw, Qw[0], Qw
            if kind == "shifted" and v == 1:                 # the view-1 body: shifted 0.3 m and turned 10 degrees about its centre
                turn, shift = _rot(rng, math.radians(10.0)), 0.3 * dirs[0]
                Xv, Yv, sv = (Xw - centre) @ turn.T + centre + shift, (Yw - centre) @ turn.T + centre + shift, sw + shift
                Q0, Qb = turn @ Qw[0], [Qw[0]] + [q @ _rot(rng, math.radians(5.0)) for q in Qw[1:]]
            X, Y, s, Qr, Xgt = Xv @ R32.T + t32, Yv @ R32.T + t32, sv @ R32.T + t32, R32 @ Q0, Xw @ R32.T + t32
        Qs = [Qr] + (Qw[1:] if kind == "identical" else Qb[1:])
        K = np.array([[rng.uniform(1400, 1600), 0, rng.uniform(900, 1000)], [0, rng.uniform(1400, 1600), rng.uniform(500, 580)], [0, 0, 1]])
        proj = lambda P: np.stack([K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]], 1)
        kp = np.concatenate([proj(Xgt[:NJ]) + rng.uniform(-3.0, 3.0, (NJ, 2)),
                             rng.uniform(0.3, 1.0, (NJ, 1))], 1)
        kp = np.concatenate([kp, rng.uniform(0, 1000, (2, 3))])          # 24 rows; the last two are never read
        j2d = proj(X) + rng.uniform(-8.0, 8.0, (nJ, 2))
        d = dict(joints=X, extr=e32, verts=Y, trans=s, rot=np.stack(Qs) if rot == "rotmat" else np.stack([_aa(q) for q in Qs]),
                 j2d=j2d, kp=kp, intr=K)
        out.append({k: np.asarray(a, dtype=np.float32) for k, a in d.items()})
    if kind == "identical":
        for k in ("joints", "verts", "trans", "rot", "j2d", "kp", "intr"):
            out[1][k] = out[0][k].copy()
    if kind == "nonortho":
        out[0]["extr"][:, :3] *= np.float32(1.01)
    if kind == "nan_extr":
        out[1]["extr"][1, 2] = np.nan
    if kind == "zero_conf":
        out[0]["kp"][0:NJ:3, 2] = 0.0
        out[1]["kp"][0:NJ:4, 2] = 0.0
    if kind == "nan_kp":
        out[0]["kp"][5, 0] = np.nan
        out[1]["kp"][7, 2] = np.nan
    return out


def assert_conditions(kind, views):
    """the generator's own conditions: the reference's valid / invalid and skip decisions are never a rounding question"""
    for v in range(2):
        R = views[v]["extr"][:, :3].astype(np.float64)
        if kind not in ("nonortho", "nan_extr"):
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6, "%s: extr of view %d is not orthonormal to 1e-6" % (kind, v)
    if kind in ("nonortho", "nan_extr"):
        return
    for j in range(NJ):
        rays = []
        for v in range(2):
            K, kp = views[v]["intr"].astype(np.float64), views[v]["kp"][j].astype(np.float64)
            if not np.isfinite(kp).all():
                break
            rays.append(views[v]["extr"][:, :3].astype(np.float64).T @ np.array([(kp[0] - K[0, 2]) / K[0, 0], (kp[1] - K[1, 2]) / K[1, 1], 1.0]))
        if len(rays) == 2:
            cr = np.cross(rays[0], rays[1])
            s2 = float(cr @ cr) / (float(rays[0] @ rays[0]) * float(rays[1] @ rays[1]))
            assert s2 >= 2 * MIN_SIN2 or s2 <= 0.5 * MIN_SIN2, "%s joint %d: sin^2 = %g is within a factor 2 of the gate" % (kind, j, s2)


def make_case(B, nj, J, V, padded, rot="rotmat", root="trans", seed=0, kinds=None, feed=None):
    """sample b is of kind kinds[b] (default: KINDS cycled from an offset that moves with V and B).  padded: every sample stride
    above its entry's size with PAD in between, extr as (3, 4) rows (stride 13), else dense with extr (4, 4).  root: "trans",
    "joint0" or None.  feed: which optional inputs are passed, of {"trans", "rot", "reproj", "tri"} (vertices: V > 0)"""
    rng = np.random.default_rng(100000 * seed + 1000 * (SIZES.index(V) if V in SIZES else V) + 10 * B + J)
    feed = set(("trans", "rot", "reproj", "tri") if feed is None else feed)
    if root == "trans":
        assert "trans" in feed
    off = (SIZES.index(V) if V in SIZES else V) + B
    kinds = list(kinds) if kinds is not None else [KINDS[(off + b) % len(KINDS)] for b in range(B)]
    size = dict(joints=3 * J, extr=12, verts=3 * V, trans=3, rot=NJ * (9 if rot == "rotmat" else 3), j2d=2 * J, kp=3 * NJ, intr=9)
    extra = dict(joints=7, extr=1, verts=5, trans=2, rot=3, j2d=3, kp=3 * 24 + 11, intr=2) if padded else \
        dict(joints=0, extr=4, verts=0, trans=0, rot=0, j2d=0, kp=3 * 24 + 6, intr=0)
    case = dict(B=B, nj=nj, J=J, V=V, rot=rot, root=root, feed=feed, kinds=kinds, size=size, padded=padded,
                stride={k: size[k] + extra[k] for k in size}, view=[])
    for v in range(2):
        case["view"].append({k: np.full((B, case["stride"][k]), PAD, np.float32) for k in size})
    for b, kind in enumerate(kinds):
        views = make_sample(kind, J, V, rot, rng)
        assert_conditions(kind, views)
        for v in range(2):
            for k in size:
                flat = views[v][k].reshape(-1)
                case["view"][v][k][b, :flat.size] = flat
            if not padded:
                case["view"][v]["extr"][b, 12:16] = [0, 0, 0, 1]
    if root == "joint0":
        size["root"], case["stride"]["root"] = 3, case["stride"]["joints"]
        for v in range(2):
            case["view"][v]["root"] = case["view"][v]["joints"]
    elif root == "trans":
        size["root"], case["stride"]["root"] = 3, case["stride"]["trans"]
        for v in range(2):
            case["view"][v]["root"] = case["view"][v]["trans"]
    return case


def concat_cases(cases):
    out = dict(cases[0])
    out["B"] = sum(c["B"] for c in cases)
    out["kinds"] = sum((c["kinds"] for c in cases), [])
    out["view"] = [{k: np.concatenate([c["view"][v][k] for c in cases]) for k in cases[0]["view"][v]} for v in range(2)]
    return out


# ------------------------------------------------------------------------------------------------ the GPU calls
def run_gpu(case, dev, acc_init=None, per_sample=True, skew=False, min_sin2=MIN_SIN2):
    """one apg_xview_update into fresh guarded buffers -> dict(ps (B, 16), tri (B, 22, 4), acc (26,), guards_ok, inputs_ok), numpy.
    skew: every input starts one float past a 16-byte boundary"""
    from airpose_amd import _native_grad as G
    L, vp = G.lib(), G.vp
    B, V, feed = case["B"], case["V"], case["feed"]
    names = ["joints", "extr"] + (["verts"] if V else []) + [k for k in ("trans", "rot") if k in feed] + \
        (["j2d"] if "reproj" in feed else []) + (["kp"] if ("reproj" in feed or "tri" in feed) else []) + (["intr"] if "tri" in feed else [])
    total = sum(int(case["view"][v][k].size) + 80 for v in range(2) for k in names)
    gc = GuardedCall(dev, 16384 + total + B * (PS + NJ * 4 + 160) + 2 * ACC)
    dv = [{k: gc.put(torch.from_numpy(case["view"][v][k]), skew) for k in names} for v in range(2)]
    table = []
    for v in range(2):
        d = dict(dv[v])
        d["root"] = None if case["root"] is None else d["trans" if case["root"] == "trans" else "joints"]
        table += [d.get(k) for k in ENTRIES]
    strides = [case["stride"].get(k, 0) if (k in dv[0] or (k == "root" and case["root"] is not None)) else 0 for k in ENTRIES]
    ps = gc.ar.take((B, PS)) if per_sample else None
    tri = gc.ar.take((B, NJ, 4)) if per_sample and "tri" in feed else None
    nbytes = L.apg_xview_workspace_bytes(B, 2, V)
    assert nbytes == B * (NS + 2 * max(1, -(-V // 1024))) * 8
    acc, ws = gc.sums(ACC // 2, acc_init if acc_init is None else np.asarray(acc_init).reshape(2, ACC // 2), nbytes)
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    res = gc.run(G, lambda: L.apg_xview_update(B, 2, case["nj"], V, 1 if case["rot"] == "rotmat" else 0, (G._i64 * PER_VIEW)(*strides),
                                               G.ptrs(table), min_sin2, vp(ps), vp(tri), vp(acc), vp(ws), nbytes, G.stream(dev)),
                 "apg_xview_update", lambda: dict(ps=host(ps), tri=host(tri), acc=host(acc).reshape(-1)))
    # the inputs hold NaN on purpose (nan_extr, nan_kp): unchanged means the same bits
    res["inputs_ok"] = all(torch.equal(g.cpu().contiguous().view(torch.int32), t.contiguous().view(torch.int32)) for g, t in gc.ins)
    return res


def run_triangulate(case, dev, min_sin2=MIN_SIN2):
    """apg_xview_triangulate on the case's first 22 keypoints -> (B, 22, 4)"""
    from airpose_amd import _native_grad as G
    B = case["B"]
    dense = lambda v, k, n: torch.from_numpy(np.ascontiguousarray(view(case, v, k)[:, :n])).to(dev)
    kp, K = [dense(v, "kp", 3 * NJ) for v in range(2)], [dense(v, "intr", 9) for v in range(2)]
    Ex = [torch.cat([dense(v, "extr", 12), torch.zeros(B, 4, device=dev)], 1) for v in range(2)]
    out = torch.full((B, NJ, 4), float("nan"), device=dev)
    with torch.cuda.device(dev):
        G.check(G.lib().apg_xview_triangulate(B, NJ, G.vp(kp[0]), G.vp(kp[1]), G.vp(K[0]), G.vp(K[1]), G.vp(Ex[0]), G.vp(Ex[1]), min_sin2,
                                              G.vp(out), G.stream(dev)), "apg_xview_triangulate")
        torch.cuda.synchronize(dev)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the Python class's dicts
def dicts_of(case, dev=None):
    """(output, batch) of torch tensors as CrossViewMetrics.update reads them, from a DENSE case that feeds everything: the
    predictions in `output`, extr (B, 4, 4), intr and smpl_joints_2d (B, 2, 24, 3) in `batch`"""
    assert not case["padded"]
    B, J, V = case["B"], case["J"], case["V"]
    out, batch = {}, {}
    put = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a).reshape(shape)).to(dev if dev is not None else "cpu")
    for v in range(2):
        d = case["view"][v]
        out["pred_j3d_cam%d" % v] = put(d["joints"], (B, J, 3))
        if V:
            out["pred_vertices_cam%d" % v] = put(d["verts"], (B, V, 3))
        out["pred_smpltrans%d" % v] = put(d["trans"], (B, 3))
        out["pred_rotmat%d" % v if case["rot"] == "rotmat" else "pred_angles%d" % v] = put(d["rot"], (B, NJ, 3, 3) if case["rot"] == "rotmat" else (B, NJ, 3))
        out["pred_j2d_cam%d" % v] = put(d["j2d"], (B, J, 2))
        batch["extr%d" % v] = put(d["extr"], (B, 4, 4))
        batch["intr%d" % v] = put(d["intr"], (B, 3, 3))
        batch["smpl_joints_2d%d" % v] = put(d["kp"], (B, 2, 24, 3))
    return out, batch


def case_of(output, batch, nj=NJ, root="trans"):
    """the dense case of what an update with (output, batch) reads: the inverse of dicts_of for tensors from anywhere"""
    look = lambda k: (output[k] if k in output else batch[k]).detach().float().cpu().numpy()
    B, J = look("pred_j3d_cam0").shape[:2]
    V = look("pred_vertices_cam0").shape[1] if "pred_vertices_cam0" in output else 0
    rot = "rotmat" if "pred_rotmat0" in output else "aa"
    size = dict(joints=3 * J, extr=12, verts=3 * V, trans=3, rot=NJ * (9 if rot == "rotmat" else 3), j2d=2 * J, kp=3 * NJ, intr=9, root=3)
    case = dict(B=B, nj=nj, J=J, V=V, rot=rot, root=root, feed={"trans", "rot", "reproj", "tri"}, kinds=["consistent"] * B, size=size,
                padded=False, view=[])
    for v in range(2):
        d = dict(joints=look("pred_j3d_cam%d" % v), extr=look("extr%d" % v), trans=look("pred_smpltrans%d" % v),
                 rot=look(("pred_rotmat%d" if rot == "rotmat" else "pred_angles%d") % v), j2d=look("pred_j2d_cam%d" % v),
                 kp=look("smpl_joints_2d%d" % v), intr=look("intr%d" % v))
        d["verts"] = look("pred_vertices_cam%d" % v) if V else np.zeros((B, 0), np.float32)
        d = {k: np.ascontiguousarray(a).reshape(B, -1) for k, a in d.items()}
        d["root"] = d["trans"] if root == "trans" else d["joints"]
        case["view"].append(d)
    case["stride"] = {k: case["view"][0][k].shape[1] for k in size}
    return case
