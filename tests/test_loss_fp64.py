"""Element-wise fp64 ground truth for apg_loss_fwd_bwd (airpose_amd/csrc/loss_grad.hip): the training loss of the four reference
trainers and its gradient seeds, through the C ABI of include/airpose_grad.h.  Companion of test_smplx_fwd_fp64.py; evaluate() is
test_stem_pool_fp64's.

Reference.  reference() below: get_loss restated in fp64 from torch ops on exactly the fp32 values the kernel receives (the four
trainers differ only in the number of views, the cross-view sub-terms and whether trans / cam exist), its gradients by autograd.
Terms: loss, trans, keypoints, keypoints_3d, shape, rootrot, pose, betas, cam, in the kernel's order.

Bars (derived from the kernel, none measured).  u = 2^-24.  |got - ref| <= n u A.  Where A = 0 (rows >= 22 of g_joints / g_j2d,
columns 1, 2 of g_cam, a zero weight) the output must be exactly 0.
  Loss terms: A = the term itself (every summand is >= 0), n = the longest chain of roundings behind it:
    per element   d = a - b is one rounding, so d^2 carries 2; fmaf(d, d, acc) is one more, the element's entry into the running sum.
                  The limb-weighted terms form d^2 for each of up to three differences (3 each), add them (2), and multiply by lw,
                  itself l * l (2): 7, and the addition to the running sum is counted with the chain.
                  cam: x = -10 s (the exponent moves by 10 |s| u), expf within 1 ulp = 2 u, q = ex * ex: 2 (10 |s| + 2) + 1.
    per thread    c additions, c = the elements one thread adds: the vertex stream 16 (4 quads of 4); in a small-term workgroup of 4
                  bodies trans, rootrot, betas and cam 1 (12, 36, 40 and 12 contributing loop indices, no thread meets two), pose 4
                  (792 indices), keypoints ceil(8 J / 256), keypoints_3d ceil(12 J / 256)
    workgroup     a tree of 8 levels over 256 threads
    combine       ceil(partials / 256) strided additions per thread and a tree of 8: with the workgroup's tree, T = 16 + ceil(NSB /
                  256), NSB = ceil(B / 4); the vertex stream's NVB = ceil(3 B V / 4096)
    mean          one division by the element count N: D = 1 (2 once N >= 2^24 and the count itself is rounded)
    sub-terms     one addition per further view (v = nviews - 1) and one for a cross-view mean (x = 1 with its bit)
    shape          2 + 16 + 8 + ceil(NVB / 256) + 8 + D + v + x
    trans, rootrot 2 + 1 + T + D + v                    keypoints      2 + ceil(8 J / 256) + T + D + v
    keypoints_3d   7 + ceil(12 J / 256) + T + D         pose           7 + 4 + T + D
    betas          3 + 1 + T + D + v + x                cam            2 (10 max|s| + 2) + 1 + 1 + T + D + v
    loss           the largest of the terms present + 9 (w_k * term, seven additions, * scale)
  Gradient elements: A = the seed's expression on absolute values, |c| lw ((|a| + |gt|) + (|a| + |b|)) with the cross-view share
  (which covers the cancellation of (a - gt) + (a - b)); c = scale w 2 / N is rounded once from the host's double.
    trans, j2d, rootrot (row 0 of g_rotmat)    d, c, c * d: 3
    verts, betas                               d0, dc, d0 + dc, c, c * (..): 5
    joints, pose (rows 1 .. 21 of g_rotmat)    the same with c * lw and lw = l * l: 7
    cam                                        q as above, c, c * q: 2 (10 |s| + 2) + 3 per element

Shapes.  B in {1, 2, 3, 4, 5, 33}, V in {1, 3, 24, 1025, 10475} (10475 with B <= 3), J in {22, 23, 127} with Jg != J, all four kinds.
Partition boundaries of the kernel, one shape on each side:
  the partial quad at the end of the stream     N = 3 B V = 3 (one partial quad), 12 (none), 94275 = 3 mod 4
  vertex workgroups of 4096 floats              B = 1, V = 1365 (N = 4095: one workgroup) and V = 1366 (N = 4098: two)
  small-term workgroups of 4 bodies             B = 4 and B = 5
  the combine's 256-strided additions           B = 33, V = 10591 (256 vertex partials) and V = 10592 (257);
                                                B = 1024 (256 small partials) and B = 1025 (257), V = 1
  16-byte and 4-byte quad moves                 every vertex pointer aligned, and offset by 1, 2, 3 floats
Every call runs twice into fresh NaN-filled, NaN-guarded buffers: bit-equal.  Inputs sit at the workload's scales: trans z 10 ..
200, j2d 500 +- 100 px, vertices and joints O(1), cam[:, 0] in [-0.2, 2].

CPU self-check (no GPU): emulate(), an fp32 evaluation with the kernel's own partition and order of additions (per-thread chains,
trees, strided combine; mul + add where the kernel has an fma), stays inside every bar; each of MUTATIONS is rejected.
"""
import ctypes

import pytest
import torch

from loss_util import GUARD, LT, U32, Buf, bit_equal, dev, run_twice  # noqa: F401  (dev is a fixture)
from loss_util import place as _place, strided_sum as _strided_sum, tree as _tree
from test_stem_pool_fp64 import evaluate

EPB, SB, NJ = 4096, 4, 22                                # loss_grad.hip: LOSS_EPB, LOSS_SB; loss_common.inc: NJ
PRED = ("trans", "rotmat", "betas", "joints", "verts", "j2d", "cam")
TERMS = ("loss", "trans", "keypoints", "keypoints_3d", "shape", "rootrot", "pose", "betas", "cam")
W_NAMES = ("trans", "kp2d", "kp3d", "shape", "root", "pose", "beta", "cam", "limbs3d", "limbstheta", "scale")
X_JOINTS, X_VERTS, X_POSE, X_BETAS = 1, 2, 4, 8
KINDS = {"twoview": dict(nviews=2, cross=15, trans=True, cam=False), "singleview": dict(nviews=1, cross=0, trans=True, cam=False),
         "hmr": dict(nviews=1, cross=0, trans=False, cam=True), "muhmr": dict(nviews=2, cross=X_POSE, trans=False, cam=True)}
WEIGHTS = {"twoview": (10, 0.002, 1, 50, 1, 50, 1, 1, 3, 1, 60), "singleview": (1, 0.001, 1, 1, 1, 1, 1, 1, 3, 3, 60),
           "hmr": (1, 0.001, 1, 1, 1, 1, 1, 1, 3, 3, 60), "muhmr": (1, 0.05, 1, 100, 1, 100, 1, 1, 3, 1, 60)}
LIMB1, LIMB2 = (4, 5, 18, 19), (7, 8, 20, 21)            # 3-D joints; the pose term's 21 rotations: one less
MUTATIONS = ("wrong_denominator", "dropped_limb_weight", "limb_sets_shifted", "dropped_cross", "no_scale", "joint_rows_nonzero")


# ------------------------------------------------------------------------------------------------ cases
def make_case(kind, B, V, J, Jg, seed=0, weights=None, limbs=None):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + V + J)
    r = lambda *s: torch.randn(*s, generator=g)
    k = KINDS[kind]
    w = list(WEIGHTS[kind] if weights is None else weights)
    if limbs is not None:
        w[8] = w[9] = limbs
    c = dict(kind=kind, B=B, V=V, J=J, Jg=Jg, w=torch.tensor(w, dtype=torch.float32), pred=[], **k)
    c["gt"] = dict(pose=r(B, 21, 3, 3) * 0.5, joints=r(B, Jg, 3) * 0.5, verts=r(B, V, 3) * 0.5, root=[], j2d=[], trans=[])
    for v in range(k["nviews"]):
        z = torch.rand(B, 1, generator=g) * 190 + 10
        p = dict(trans=torch.cat([r(B, 2) * 2, z], 1) if k["trans"] else None, rotmat=r(B, 22, 3, 3) * 0.5, betas=r(B, 10),
                 joints=c["gt"]["joints"][:, :NJ].mean() + r(B, J, 3) * 0.5, verts=c["gt"]["verts"] + r(B, V, 3) * 0.05,
                 j2d=r(B, J, 2) * 100 + 500,
                 cam=torch.cat([torch.rand(B, 1, generator=g) * 2.2 - 0.2, r(B, 2)], 1) if k["cam"] else None)
        c["pred"].append(p)
        c["gt"]["root"].append(r(B, 1, 3, 3) * 0.5)
        c["gt"]["j2d"].append(p["j2d"][:, :1].expand(B, Jg, 2) + r(B, Jg, 2) * 5)
        c["gt"]["trans"].append(p["trans"] + r(B, 3) * 2 if k["trans"] else None)
    return c


def limb_vec(n, first, l, dt, sets=(LIMB1, LIMB2)):
    """per-row weights of n rows whose row 0 is 3-D joint `first`"""
    lw = torch.ones(n, dtype=dt)
    l = torch.as_tensor(l, dtype=dt)
    for j in sets[0]:
        lw[j - first] = l
    for j in sets[1]:
        lw[j - first] = l * l
    return lw


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def loss_terms(c, P, G):
    """get_loss on per-view dicts P of PRED tensors and the ground truth G, in their dtype -> the nine terms (0-d tensors), TERMS order"""
    w = [float(x) for x in c["w"]]
    nv, cross = c["nviews"], c["cross"]
    dt = P[0]["rotmat"].dtype
    d = lambda t: t.to(device=P[0]["rotmat"].device, dtype=dt)
    mse = lambda a, b: (a - b) ** 2
    zero = torch.zeros((), dtype=dt, device=P[0]["rotmat"].device)
    trans = sum((mse(P[v]["trans"], d(G["trans"][v])).mean() for v in range(nv)), zero) if c["trans"] else zero
    kp = sum((mse(P[v]["j2d"][:, :NJ], d(G["j2d"][v])[:, :NJ]).mean() for v in range(nv)), zero)
    l = sum(mse(P[v]["joints"][:, :NJ], d(G["joints"])[:, :NJ]) for v in range(nv))
    if cross & X_JOINTS:
        l = l + mse(P[0]["joints"][:, :NJ], P[1]["joints"][:, :NJ])
    l[:, list(LIMB1)] *= w[8]
    l[:, list(LIMB2)] *= w[8] ** 2
    kp3d = l.mean()
    shape = sum((mse(P[v]["verts"], d(G["verts"])).mean() for v in range(nv)), zero)
    if cross & X_VERTS:
        shape = shape + mse(P[0]["verts"], P[1]["verts"]).mean()
    root = sum((mse(P[v]["rotmat"][:, :1], d(G["root"][v])).mean() for v in range(nv)), zero)
    l = sum(mse(P[v]["rotmat"][:, 1:], d(G["pose"])) for v in range(nv))
    if cross & X_POSE:
        l = l + mse(P[0]["rotmat"][:, 1:], P[1]["rotmat"][:, 1:])
    l[:, [j - 1 for j in LIMB1]] *= w[9]
    l[:, [j - 1 for j in LIMB2]] *= w[9] ** 2
    pose = l.mean()
    betas = sum(((P[v]["betas"] * P[v]["betas"]).mean() for v in range(nv)), zero)
    if cross & X_BETAS:
        betas = betas + mse(P[0]["betas"], P[1]["betas"]).mean()
    cam = sum(((torch.exp(-P[v]["cam"][:, 0] * 10) ** 2).mean() for v in range(nv)), zero) if c["cam"] else zero
    loss = w[0] * trans + w[1] * kp + w[2] * kp3d + w[3] * shape + w[4] * root + w[5] * pose + w[6] * betas + w[7] * cam
    loss = loss * w[10]
    return loss, trans, kp, kp3d, shape, root, pose, betas, cam


def reference(c):
    """-> dict(terms (9,) fp64, grads: per view a dict of PRED (zeros where the loss does not reach), A: their magnitudes, n)"""
    P = [{n: (None if t is None else t.double().requires_grad_()) for n, t in p.items()} for p in c["pred"]]
    terms = loss_terms(c, P, c["gt"])
    terms[0].backward()
    grads = [{n: (None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad)) for n, t in p.items()} for p in P]
    return dict(terms=torch.stack(terms).detach(), grads=grads, A=magnitudes(c), n=roundings(c))


def magnitudes(c):
    """A of every gradient element: the seed's expression on absolute values"""
    w = [float(x) for x in c["w"]]
    nv, cross, B, V = c["nviews"], c["cross"], c["B"], c["V"]
    G = c["gt"]
    a = lambda t: t.double().abs()
    coef = lambda k, n: abs(w[10] * w[k] * 2.0 / n)
    out = []
    for v in range(nv):
        p, o = c["pred"][v], c["pred"][1 - v] if nv == 2 else None
        both = lambda n, bit: (a(p[n]) + a(o[n])) if (cross & bit) else 0.0
        A = dict(trans=None, cam=None)
        if c["trans"]:
            A["trans"] = coef(0, 3 * B) * (a(p["trans"]) + a(G["trans"][v]))
        A["j2d"] = torch.zeros_like(a(p["j2d"]))
        A["j2d"][:, :NJ] = coef(1, 44 * B) * (a(p["j2d"])[:, :NJ] + a(G["j2d"][v])[:, :NJ])
        A["joints"] = torch.zeros_like(a(p["joints"]))
        m = a(p["joints"]) + (both("joints", X_JOINTS))
        A["joints"][:, :NJ] = coef(2, 66 * B) * limb_vec(NJ, 0, abs(w[8]), torch.float64)[None, :, None] * (m[:, :NJ] + a(G["joints"])[:, :NJ])
        A["verts"] = coef(3, 3 * B * V) * (a(p["verts"]) + a(G["verts"]) + both("verts", X_VERTS))
        R = a(p["rotmat"])
        A["rotmat"] = torch.empty_like(R)
        A["rotmat"][:, :1] = coef(4, 9 * B) * (R[:, :1] + a(G["root"][v]))
        A["rotmat"][:, 1:] = coef(5, 189 * B) * limb_vec(21, 1, abs(w[9]), torch.float64)[None, :, None, None] * (
            R[:, 1:] + a(G["pose"]) + (both("rotmat", X_POSE)[:, 1:] if cross & X_POSE else 0.0))
        A["betas"] = coef(6, 10 * B) * (a(p["betas"]) + both("betas", X_BETAS))
        if c["cam"]:
            A["cam"] = torch.zeros_like(a(p["cam"]))
            A["cam"][:, 0] = abs(w[10] * w[7] * 20.0 / B) * torch.exp(-20.0 * p["cam"][:, 0].double())
        out.append(A)
    return out


def roundings(c):
    """n of every term (list of 9) and of every gradient (dict; rotmat per row, cam per element in verify), counted from loss_grad.hip
    as in the docstring"""
    B, V, J = c["B"], c["V"], c["J"]
    nvb, nsb = -(-3 * B * V // EPB), -(-B // SB)
    cv, cs = -(-nvb // LT), -(-nsb // LT)
    cnt = lambda n: 2 if n >= 2 ** 24 else 1                  # the division, and the count's own rounding once it is no fp32 integer
    views = c["nviews"] - 1                                   # additions of the per-view means
    xs = lambda bit: 1 if c["cross"] & bit else 0             # addition of the cross-view mean
    ch_kp, ch_j3 = -(-SB * 2 * J // LT), -(-SB * 3 * J // LT)
    smax = max([float(p["cam"][:, 0].abs().max()) for p in c["pred"]]) if c["cam"] else 0.0
    tail = 8 + cs + 8                                         # workgroup tree, strided combine, combine tree
    t = dict(trans=2 + 1 + tail + cnt(3 * B) + views, keypoints=2 + ch_kp + tail + cnt(44 * B) + views,
             rootrot=2 + 1 + tail + cnt(9 * B) + views, keypoints_3d=7 + ch_j3 + tail + cnt(66 * B), pose=7 + 4 + tail + cnt(189 * B),
             shape=2 + 16 + 8 + cv + 8 + cnt(3 * B * V) + views + xs(X_VERTS), betas=3 + 1 + tail + cnt(10 * B) + views + xs(X_BETAS),
             cam=2 * (10 * smax + 2) + 1 + 1 + tail + cnt(B) + views)
    live = [k for k in t if not (k == "trans" and not c["trans"]) and not (k == "cam" and not c["cam"])]
    t["loss"] = max(t[k] for k in live) + 9
    rot = torch.full((1, 22, 1, 1), 7.0, dtype=torch.float64)
    rot[:, 0] = 3.0
    g = dict(trans=3, j2d=3, verts=5, betas=5, joints=7, rotmat=rot)
    return dict(terms=[t[n] for n in TERMS], grads=g)


def verify(c, ref, terms, grads, what, ratios=None, skip=()):
    """-> list of failures of (terms (9,), grads: per view dict of PRED or None entries) against ref's bars"""
    fails = []
    ratios = {} if ratios is None else ratios

    def one(name, got, want, bound):
        ok, ratio, nz, msg = evaluate(got, want, bound)
        ratios[name] = max(ratios.get(name, 0.0), ratio)
        if not ok:
            fails.append((what, name, msg))

    n = ref["n"]
    tb = torch.tensor([k * U32 for k in n["terms"]], dtype=torch.float64) * ref["terms"].abs()
    one("terms", terms, ref["terms"], tb)
    for v, gv in enumerate(grads):
        for name in PRED:
            if gv.get(name) is None or (v, name) in skip:
                continue
            A = ref["A"][v][name]
            if name == "cam":
                nn = 2 * (10 * c["pred"][v]["cam"][:, :1].double().abs() + 2) + 3
            else:
                nn = n["grads"][name]
            one("g_%s%d" % (name, v), gv[name], ref["grads"][v][name], nn * U32 * A)
    return fails


# ------------------------------------------------------------------------------------------------ fp32 emulation in the kernel's order
def _stream_sum(sq):
    """the vertex stream's sum of the flat squares: per workgroup 256 threads x (4 quads x 4) in order, tree; partials strided + tree"""
    n = sq.numel()
    nvb = -(-n // EPB)
    x = torch.zeros(nvb * EPB, dtype=sq.dtype)
    x[:n] = sq
    x = x.view(nvb, EPB // (LT * 4), LT, 4).permute(0, 2, 1, 3).reshape(nvb, LT, -1)
    acc = torch.zeros(nvb, LT, dtype=sq.dtype)
    for i in range(x.shape[2]):
        acc = acc + x[:, :, i]
    return _strided_sum(_tree(acc))


def _small_sum(per_body):
    """per_body (B, m): each small-term workgroup sums its 4 bodies' rows in loop order; partials strided + tree"""
    B = per_body.shape[0]
    parts = [_strided_sum(per_body[b:b + SB].reshape(-1)) for b in range(0, B, SB)]
    return _strided_sum(torch.stack(parts))


def emulate(c, mut=None, aliased=False):
    """fp32, the kernel's operations and order -> (terms (9,) fp32, grads per view)"""
    f = torch.float32
    w = c["w"].clone()
    nv, cross, B, V, J = c["nviews"], c["cross"], c["B"], c["V"], c["J"]
    if mut == "no_scale":
        w[10] = 1.0
    if mut == "dropped_cross":
        cross &= ~X_VERTS
    G = c["gt"]
    P = [c["pred"][0] if aliased else p for p in c["pred"]]
    two = nv == 2
    coef = lambda k, n: torch.tensor(float(w[10]) * float(w[k]) * 2.0 / n, dtype=torch.float64).to(f)
    sets3, setsp = ((LIMB1, LIMB2), (LIMB1, LIMB2))
    if mut == "limb_sets_shifted":
        sets3 = (tuple(j - 1 for j in LIMB1), tuple(j - 1 for j in LIMB2))
        setsp = (tuple(j + 1 for j in LIMB1[:-1]) + (20,), tuple(j + 1 for j in LIMB2[:-1]) + (21,))
    if mut == "dropped_limb_weight":
        sets3 = (LIMB1, ())
    grads = [dict.fromkeys(PRED) for _ in range(nv)]
    z = torch.zeros((), dtype=f)

    def plain(name, gname, k, n, rows=None):
        """per-view plain terms -> sum of the views' means"""
        tot = None
        for v in range(nv):
            a, g = P[v][name], G[gname][v]
            if rows is not None:
                a, g = a[:, :rows], g[:, :rows]
            d = a - g
            sq = torch.zeros(B, P[v][name][0].numel(), dtype=f)            # the loop runs over every row; rows >= 22 add nothing
            sq[:, :d[0].numel()] = (d * d).reshape(B, -1)
            m = _small_sum(sq) / torch.tensor(float(n), dtype=f)
            tot = m if tot is None else tot + m
            gr = torch.zeros_like(P[v][name])
            gr[:, :d.shape[1]] = coef(k, n) * d
            grads[v][name] = gr
        return tot

    def paired(a0, a1, g, cr, c_, lw):
        d0 = a0 - g
        e = d0 * d0
        dc = torch.zeros_like(d0)
        d1 = torch.zeros_like(d0)
        if two:
            d1 = a1 - g
            e = e + d1 * d1
            if cr:
                dc = a0 - a1
                e = e + dc * dc
        cl = c_ * lw
        return e * lw, cl * (d0 + dc), cl * (d1 - dc), (d0 * d0, d1 * d1, dc * dc)

    trans = plain("trans", "trans", 0, 3 * B) if c["trans"] else z
    kp = plain("j2d", "j2d", 1, 2 * (J if mut == "wrong_denominator" else NJ) * B, rows=NJ)
    # 3-D joints
    lw = limb_vec(NJ, 0, w[8], f, sets3)[None, :, None]
    e, g0, g1, _ = paired(P[0]["joints"][:, :NJ], P[-1]["joints"][:, :NJ], G["joints"][:, :NJ], cross & X_JOINTS, coef(2, 66 * B), lw)
    full = torch.zeros(B, J * 3, dtype=f)
    full[:, :NJ * 3] = e.reshape(B, -1)
    kp3d = _small_sum(full) / torch.tensor(66.0 * B, dtype=f)
    for v, gg in enumerate((g0, g1)[:nv]):
        gr = torch.zeros_like(P[v]["joints"])
        if mut == "joint_rows_nonzero":
            gr = coef(2, 66 * B) * (P[v]["joints"] - G["joints"][:, :1])
        gr[:, :NJ] = gg
        grads[v]["joints"] = gr
    # vertices
    _, g0, g1, sq = paired(P[0]["verts"], P[-1]["verts"], G["verts"], cross & X_VERTS, coef(3, 3 * B * V), torch.ones((), dtype=f))
    nsh = torch.tensor(3.0 * B * V, dtype=f)
    shape = _stream_sum(sq[0].reshape(-1)) / nsh
    if two:
        shape = (shape + _stream_sum(sq[1].reshape(-1)) / nsh) + _stream_sum(sq[2].reshape(-1)) / nsh
    for v, gg in enumerate((g0, g1)[:nv]):
        grads[v]["verts"] = gg
    # rotations
    root = None
    rg = []
    for v in range(nv):
        d = P[v]["rotmat"][:, :1] - G["root"][v]
        sq0 = torch.zeros(B, 22 * 9, dtype=f)
        sq0[:, :9] = (d * d).reshape(B, -1)
        m = _small_sum(sq0) / torch.tensor(9.0 * B, dtype=f)
        root = m if root is None else root + m
        rg.append(coef(4, 9 * B) * d)
    lw = limb_vec(21, 1, w[9], f, setsp)[None, :, None, None]
    e, g0, g1, _ = paired(P[0]["rotmat"][:, 1:], P[-1]["rotmat"][:, 1:], G["pose"], cross & X_POSE, coef(5, 189 * B), lw)
    full = torch.zeros(B, 22 * 9, dtype=f)
    full[:, 9:] = e.reshape(B, -1)
    pose = _small_sum(full) / torch.tensor(189.0 * B, dtype=f)
    for v, gg in enumerate((g0, g1)[:nv]):
        grads[v]["rotmat"] = torch.cat([rg[v], gg], 1)
    # betas
    _, g0, g1, sq = paired(P[0]["betas"], P[-1]["betas"], torch.zeros((), dtype=f), cross & X_BETAS, coef(6, 10 * B), torch.ones((), dtype=f))
    nb = torch.tensor(10.0 * B, dtype=f)
    betas = _small_sum(sq[0]) / nb
    if two:
        betas = (betas + _small_sum(sq[1]) / nb) + _small_sum(sq[2]) / nb
    for v, gg in enumerate((g0, g1)[:nv]):
        grads[v]["betas"] = gg
    cam = z
    if c["cam"]:
        cam = None
        cc = torch.tensor(float(w[10]) * float(w[7]) * -20.0 / B, dtype=torch.float64).to(f)
        for v in range(nv):
            ex = torch.exp(torch.tensor(-10.0, dtype=f) * P[v]["cam"][:, 0])
            q = ex * ex
            full = torch.zeros(B, 3, dtype=f)
            full[:, 0] = q
            m = _small_sum(full) / torch.tensor(float(B), dtype=f)
            cam = m if cam is None else cam + m
            gr = torch.zeros_like(P[v]["cam"])
            gr[:, 0] = cc * q
            grads[v]["cam"] = gr
    loss = w[0] * trans
    for k, t in ((1, kp), (2, kp3d), (3, shape), (4, root), (5, pose), (6, betas), (7, cam)):
        loss = loss + w[k] * t
    loss = loss * w[10]
    return torch.stack([loss, trans, kp, kp3d, shape, root, pose, betas, cam]), grads


SELF_CASES = [("twoview", 3, 24, 127, 144), ("twoview", 5, 1025, 23, 22), ("singleview", 2, 3, 23, 22), ("hmr", 5, 24, 22, 23),
              ("muhmr", 3, 24, 127, 22), ("twoview", 1, 1366, 22, 23)]


@pytest.mark.parametrize("kind,B,V,J,Jg", SELF_CASES)
def test_cpu_fp32_emulation_is_inside_every_bar(kind, B, V, J, Jg):
    c = make_case(kind, B, V, J, Jg)
    ref = reference(c)
    ratios = {}
    terms, grads = emulate(c)
    fails = verify(c, ref, terms, grads, "emulation", ratios)
    print("%s B %d V %d J %d: worst err / bound %s" % (kind, B, V, J, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fails, fails


@pytest.mark.parametrize("mut", MUTATIONS)
def test_cpu_mutations_are_rejected(mut):
    c = make_case("twoview", 3, 24, 127, 144, limbs=3.0)           # (the two-view default limbstheta = 1 would hide the pose sets)
    ref = reference(c)
    terms, grads = emulate(c, mut=mut)
    fails = verify(c, ref, terms, grads, mut)
    assert fails, "the bars accept the mutation %s" % mut
    names = {f[1] for f in fails}
    want = {"wrong_denominator": "g_j2d0", "dropped_limb_weight": "g_joints0", "limb_sets_shifted": "g_rotmat0", "dropped_cross": "g_verts0",
            "no_scale": "terms", "joint_rows_nonzero": "g_joints1"}[mut]
    assert want in names, (mut, sorted(names))


def test_cpu_aliased_views_have_no_cross_share():
    """pred0 is pred1: the restatement's cross terms vanish and the emulation's seeds are the single-view ones, exactly"""
    c = make_case("twoview", 3, 24, 23, 22)
    for v in ("root", "j2d", "trans"):
        c["gt"][v][1] = c["gt"][v][0]
    t2, g2 = emulate(c, aliased=True)
    c1 = dict(c, nviews=1, cross=0, pred=c["pred"][:1])
    t1, g1 = emulate(c1)
    assert torch.equal(t2, 2 * t1)
    for n in PRED:
        if g1[0][n] is not None:
            assert torch.equal(g2[0][n], g1[0][n]) and torch.equal(g2[1][n], g1[0][n]), n


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
def run(c, dev, want=None, voff=(0, 0, 0, 0, 0), aliased=False):
    """one apg_loss_fwd_bwd call -> (terms (9,) cpu, grads per view (cpu tensors / None)).  want: set of (view, name) gradients to ask
    for (None = all that exist; empty = the grads table itself NULL).  voff: float offsets of verts0, verts1, gt_verts, g_verts0,
    g_verts1."""
    from airpose_amd import _native_grad as G
    L = G.lib()
    nv, B, J, Jg, V = c["nviews"], c["B"], c["J"], c["Jg"], c["V"]
    every = {(v, n) for v in range(nv) for n in PRED if c["pred"][v][n] is not None}
    want = every if want is None else set(want)
    assert want <= every
    pred = []
    for v in range(nv):
        if aliased and v == 1:
            pred += pred[:len(PRED)]
            break
        pred += [_place(c["pred"][v][n], dev, voff[v] if n == "verts" else 0) for n in PRED]
    gt = [_place(c["gt"]["pose"], dev), _place(c["gt"]["joints"], dev), _place(c["gt"]["verts"], dev, voff[2])]
    for v in range(nv):
        gt += [_place(c["gt"]["root"][v], dev), _place(c["gt"]["j2d"][v], dev), _place(c["gt"]["trans"][v], dev)]
    outs = [Buf(dev, c["pred"][v][n].numel(), voff[3 + v] if n == "verts" else 0) if (v, n) in want else None
            for v in range(nv) for n in PRED]
    terms = Buf(dev, len(TERMS))
    nbytes = L.apg_loss_workspace_bytes(B, V)
    assert nbytes > 0
    ws = Buf(dev, nbytes // 4)
    w = (ctypes.c_float * 11)(*[float(x) for x in c["w"]])
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    table = G.ptrs([None if o is None else o.out for o in outs]) if want else None
    rc = L.apg_loss_fwd_bwd(nv, c["cross"], B, J, Jg, V, w, G.ptrs(pred), G.ptrs(gt), p(terms.out), table, p(ws.out), nbytes,
                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    G.check(rc, "apg_loss_fwd_bwd")
    torch.cuda.synchronize()
    lo = GUARD + nbytes // 4
    assert torch.isnan(ws.buf[:GUARD]).all() and torch.isnan(ws.buf[lo:]).all(), "the workspace's guard bands were written"
    grads = []
    for v in range(nv):
        grads.append({n: (None if outs[v * len(PRED) + k] is None else
                          outs[v * len(PRED) + k].values(c["pred"][v][n].shape, "g_%s%d" % (n, v))) for k, n in enumerate(PRED)})
    return terms.values((len(TERMS),), "terms"), grads


def run_twice_and_verify(c, dev, what, **kw):
    got = run_twice(lambda: run(c, dev, **kw), what)
    ref = reference(c)
    ratios = {}
    fails = verify(c, ref, got[0], got[1], what, ratios)
    print("%-44s worst err / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fails, fails
    return got, ref


GRID = [(1, 1, 22, 23), (2, 3, 23, 22), (3, 24, 127, 144), (5, 1025, 127, 22)]
EDGES = [("twoview", 3, 10475, 127, 144), ("twoview", 1, 10475, 22, 24), ("hmr", 2, 10475, 23, 22), ("twoview", 33, 24, 127, 22),
         ("hmr", 33, 3, 22, 23), ("muhmr", 33, 1, 23, 22), ("singleview", 33, 1025, 22, 23),
         ("twoview", 4, 24, 23, 22), ("twoview", 5, 24, 23, 22),                      # small-term workgroups: 1 | 2
         ("twoview", 1, 4, 22, 23),                                                   # N = 12: no partial quad
         ("twoview", 1, 1365, 22, 23), ("twoview", 1, 1366, 22, 23),                  # vertex workgroups: 1 | 2
         ("twoview", 33, 10591, 22, 23), ("twoview", 33, 10592, 22, 23),              # vertex partials: 256 | 257
         ("muhmr", 1024, 1, 22, 23), ("muhmr", 1025, 1, 22, 23)]                      # small partials: 256 | 257


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,V,J,Jg", [(k,) + s for k in KINDS for s in GRID] + EDGES)
def test_loss_and_seeds_against_fp64(dev, kind, B, V, J, Jg):
    run_twice_and_verify(make_case(kind, B, V, J, Jg), dev, "%s B %d V %d J %d Jg %d" % (kind, B, V, J, Jg))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["twoview", "muhmr"])
def test_each_gradient_pointer_null_in_turn_and_all_null(dev, kind):
    """which gradients are asked for changes neither the terms nor any other gradient, bit for bit"""
    c = make_case(kind, 3, 24, 23, 22)
    full, _ = run_twice_and_verify(c, dev, kind + " all gradients")
    every = [(v, n) for v in range(2) for n in PRED if c["pred"][v][n] is not None]
    for drop in every:
        got = run(c, dev, want=[e for e in every if e != drop])
        assert got[1][drop[0]][drop[1]] is None
        assert torch.equal(got[0].view(torch.int32), full[0].view(torch.int32)), drop
        for v, n in every:
            if (v, n) != drop:
                assert torch.equal(got[1][v][n].view(torch.int32), full[1][v][n].view(torch.int32)), (drop, v, n)
    fwd = run(c, dev, want=[])
    assert torch.equal(fwd[0].view(torch.int32), full[0].view(torch.int32))
    only = run(c, dev, want=[(1, "verts")])
    assert torch.equal(only[1][1]["verts"].view(torch.int32), full[1][1]["verts"].view(torch.int32))


@pytest.mark.gpu
def test_aliased_views_have_exactly_zero_cross_terms(dev):
    """pred0 is pred1 (the same pointers): every term is exactly twice the single-view one, both views' seeds are the single-view seeds"""
    c = make_case("twoview", 3, 1025, 23, 22)
    for k in ("root", "j2d", "trans"):
        c["gt"][k][1] = c["gt"][k][0]
    two = run(c, dev, aliased=True)
    c1 = dict(c, nviews=1, cross=0, pred=c["pred"][:1])
    one, ref1 = run_twice_and_verify(c1, dev, "single view of the aliased pair")
    assert torch.equal(two[0], 2 * one[0]), (two[0], one[0])
    for n in PRED:
        if one[1][0][n] is not None:
            assert torch.equal(two[1][0][n], one[1][0][n]) and torch.equal(two[1][1][n], one[1][0][n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("limbs", [1.0, 3.0, 0.0])
@pytest.mark.parametrize("kind", ["twoview", "hmr"])
def test_limb_weights(dev, kind, limbs):
    c = make_case(kind, 3, 24, 23, 22, limbs=limbs)
    got, _ = run_twice_and_verify(c, dev, "%s limbs %g" % (kind, limbs))
    if limbs == 0.0:
        for v in range(c["nviews"]):
            assert not got[1][v]["joints"][:, list(LIMB1 + LIMB2)].any()
            assert not got[1][v]["rotmat"][:, list(LIMB1 + LIMB2)].any()      # rotmat row j is pose rotation j - 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(8))
def test_a_zero_weight_gives_exactly_zero_seeds(dev, k):
    kind = "muhmr" if k == 7 else "twoview"
    w = list(WEIGHTS[kind])
    w[k] = 0.0
    c = make_case(kind, 3, 24, 23, 22, weights=w)
    got, _ = run_twice_and_verify(c, dev, "%s w_%s = 0" % (kind, W_NAMES[k]))
    for v in range(2):
        g = got[1][v]
        z = {0: g["trans"], 1: g["j2d"], 2: g["joints"], 3: g["verts"], 4: g["rotmat"][:, :1] if k == 4 else None,
             5: g["rotmat"][:, 1:] if k == 5 else None, 6: g["betas"], 7: g["cam"]}[k]
        assert z is not None and not z.any(), (W_NAMES[k], v)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_vertex_pointers_off_a_16_byte_boundary(dev, off):
    """each vertex pointer offset in turn, then all of them: the same bits as the aligned call (the partition does not move)"""
    c = make_case("twoview", 3, 1025, 23, 22)
    base, _ = run_twice_and_verify(c, dev, "aligned")
    for voff in [tuple(off if i == k else 0 for i in range(5)) for k in range(5)] + [(off,) * 5, (1, 2, 3, off, 0)]:
        got, _ = run_twice_and_verify(c, dev, "vertex offsets %s" % (voff,), voff=voff)
        assert bit_equal(got, base), voff
