"""Element-wise fp64 ground truth for apg_real_loss_fwd_bwd (airpose_amd/csrc/loss_real_grad.hip): the copenet_real trainers' get_loss
with the VPoser prior and its gradient seeds, through the C ABI of include/airpose_grad.h.  Companion of test_loss_fp64.py, whose
buffers, trees and evaluate() it shares.

Reference.  real_loss_util.loss_terms: get_loss restated in fp64 from torch ops on exactly the fp32 values the kernel receives, the
encoder as the literal unfolded layer chain, the axis-angle by oracle.geometry_ref.rotation_matrix_to_angle_axis; gradients by
autograd.  Terms: loss, vposer, pose, keypoints, betas, depth, in the kernel's order.

Bars (derived from the kernel, none measured).  u = 2^-24.
  Flat sums, |got - ref| <= n u A, A = the term itself (every summand is >= 0), n = the longest chain of roundings behind it:
    keypoints   d = a - b (1), d * d (2 + 1), wgt = conf * lw with lw = l * l (2), fmaf(d d, wgt, acc) (1): 6; a thread's chain
                ch = ceil(2 J / 256); the workgroup's tree of 8; the combine's cs = ceil(B / 256) strided additions and tree of 8;
                one division; one addition per further view (v):                     6 + ch + 8 + cs + 8 + 1 + v
    pose        dc (1 -> 2 in dc^2), fmaf (1); 9 per thread, 21 per row in order:     3 + 9 + 21 + cs + 8 + 1
    betas       x x or dc dc (3); 10 per row in order; the cross-view mean (x):       3 + 10 + cs + 8 + 1 + v + x
    depth       e = -g d moves the exponent by g |d| u, expf within 2 u, q = ex ex:   2 (g max|d| + 2) + 1 + cs + 8 + 1 + v
    loss        the weighted bounds of its terms, + 6 u (sum of |scale w_k term_k|) for w_k * term, four additions and the scale
  Flat gradients, A = the seed's expression on absolute values:
    g_j2d       c, l * l, conf * lw, c * wgt, d, the product: 6; A = |c| conf lw (|j2d| + |gt|); 0 on rows >= 22 and where conf = 0
    g_betas     dc, x +- dc, c, the product: 5 (as test_loss_fp64); A = |c| (|x| + |x0| + |x1|)
    g_depth     q as above, c, c * q: 2 (g |d| + 2) + 3 per element; 0 off the barrier's column
    g_rotmat    row 0: A = 0
  The encoder chain (the vposer term, rows 1 .. 21 of g_rotmat): grad_shapes_util.check at the project's TAU = REL_BAR = 1e-5, A
  propagated on absolute values through each stage (vposer_magnitudes): |J| |R| + |aa| through the conversion (J its fp64
  Jacobian), |W| A + |b| through the two affine maps, slope <= 1 through the LeakyReLU, A_mu + (sigmoid(s) A_s + softplus(s)) |eps|
  into z, 2 |z| A_z into z^2; and back: |c| A_z, |c| (A_z sigmoid(s) + |z| A_s / 4) |eps| for the seeds of mu and s, |W|^T A through
  the maps, |J|^T A into R, plus the pose share's |c| (|r0| + |r1|).  A covers the forward state's error in the seeds but not the
  Jacobian's own (a second-order, conditioning effect): where an element of g_rotmat fails check by that alone, the tensor is
  held to the SMPL-X files' rule instead (grad_shapes_util.check_slices per joint: four times the error of this same restatement
  evaluated in fp32 on the CPU, floor 1e-5) -- but only in a case listed in FALLBACK_ALLOWED, which is empty: every committed case
  must pass check itself, so nothing can pass under the looser bar unnoticed.
  Exact zeros where A = 0.

Shapes.  B in {1, 2, 3, 33}; the kernel gives every (view, body) row a workgroup of its own whatever B is, so its only partition
boundary is the combine's stride of 256 rows per view: B = 256 | 257.  J in {22, 25} with Jg != J; both nviews; both depth forms
((2, 1) and hmr's (0, 10)); l in {1, 1.5}; about a fifth of the confidences exactly 0; pointers offset by 1 to 3 floats.  Every
call runs twice into fresh NaN-filled, NaN-guarded buffers: bit-equal.

Inputs.  Rotations are rot6d_to_rotmat of seeded normal 6-vectors; real_loss_util.draw_rotations draws again (never leaves out)
any rotation within 1e-2 of a branch boundary of the conversion, with |w| < 1e-2 or with sin(theta / 2) < 5e-2, and every case
asserts in fp64 that all four quaternion branches are populated.

CPU self-check (no GPU): emulate(), an fp32 evaluation in the kernel's order (fmaf chains as mul + add in index order, the four
k segments, serial row sums, trees, strided combine), stays inside every bar; each of MUTATIONS is rejected.  The emulation does
NOT follow aa_bwd's own operation order: it takes the conversion's adjoint from fp32 autograd of geometry_ref, so that aa_bwd's
rounding fits the bars is shown by the GPU runs alone.
"""
import ctypes

import pytest
import torch

import grad_shapes_util as GS
from loss_util import GUARD, LT, U32, Buf, bit_equal, dev, run_twice  # noqa: F401  (dev is a fixture)
from loss_util import place as _place, strided_sum as _strided_sum
from real_loss_util import (FORMS, LIMB1, LIMB2, NJ, NR, NZ, PRED, SD, SD64, TERMS, X_BETAS, X_POSE, axis_angle, branch_of,
                            folded, limb_vec, loss_terms, make_case, packed)  # noqa: F401  (packed is a fixture)
from test_stem_pool_fp64 import evaluate

SEG = 128
MUTATIONS = ("dropped_confidence", "limb_sets_shifted", "softplus_as_exp", "eps_dropped", "bn_wrong_eps", "vposer_overwrites_pose",
             "bn_unfolded")
# cases allowed to leave grad_shapes_util.check for the per-joint rule on g_rotmat (an element that fails it by the conversion's
# conditioning alone): (form, B, J, Jg, limbs).  None needs it; a case that starts to need it fails until it is listed here with its reason
FALLBACK_ALLOWED = ()
_REF = {}


def case_key(c):
    """everything a case's reference depends on: a case is rebuilt from these by make_case"""
    return (c["form"], c["B"], c["J"], c["Jg"], c["seed"], tuple(float(x) for x in c["w"]))


def coefs(c):
    w = [float(x) for x in c["w"]]
    B = c["B"]
    return dict(kp=w[5] * w[0] * 2.0 / (44 * B), vp=w[5] * w[2] * 2.0 / (NZ * B), pose=w[5] * w[3] * 2.0 / (189 * B),
                beta=w[5] * w[1] * 2.0 / (10 * B), depth=w[5] * -2.0 * c["gain"] / B)


# ------------------------------------------------------------------------------------------------ the fp64 reference and its bars
def vposer_magnitudes(c, v):
    """-> (A of view v's vposer mean, A of the vposer share of g_rotmat[:, 1:]), by propagation on absolute values"""
    B = c["B"]
    R = c["pred"][v]["rotmat"][:, 1:].double().reshape(-1, 3, 3).requires_grad_()
    pad = torch.cat([R, torch.zeros(B * NR, 3, 1, dtype=torch.float64)], 2)
    from oracle import geometry_ref
    aa = geometry_ref.rotation_matrix_to_angle_axis(pad)
    Jabs = [torch.autograd.grad(aa[:, k].sum(), R, retain_graph=True)[0].abs() for k in range(3)]
    A_aa = torch.stack([(Jabs[k] * R.detach().abs()).sum((1, 2)) for k in range(3)], 1) + aa.detach().abs()
    W1, b1, W2, b2 = folded()
    x = aa.detach().reshape(B, 63)
    h = x @ W1.t() + b1
    A_h = A_aa.reshape(B, 63) @ W1.abs().t() + b1.abs()
    a = torch.nn.functional.leaky_relu(h, 0.01)
    out = a @ W2.t() + b2
    A_out = A_h @ W2.abs().t() + b2.abs()
    mu, s, A_mu, A_s = out[:, :NZ], out[:, NZ:], A_out[:, :NZ], A_out[:, NZ:]
    e = c["eps"][v].double().abs()
    sp, sg = torch.nn.functional.softplus(s), torch.sigmoid(s)
    z = mu + sp * c["eps"][v].double()
    A_z = A_mu + (sg * A_s + sp) * e
    A_term = float((2 * z.abs() * A_z).mean())
    cv = abs(coefs(c)["vp"])
    A_dout = torch.cat([cv * A_z, cv * (A_z * sg + z.abs() * A_s / 4) * e], 1)
    A_dh = (A_dout @ W2.abs()) * torch.where(h > 0, 1.0, 0.01)
    A_daa = (A_dh @ W1.abs()).reshape(-1, 3)
    A_R = sum(Jabs[k] * A_daa[:, k, None, None] for k in range(3))
    return A_term, A_R.reshape(B, NR, 3, 3)


def reference(c):
    """-> dict(terms (6,) fp64, grads per view, bound: per-term absolute bounds (vposer: None, it has A), A_vp, gA / gn per view)"""
    key = case_key(c)
    if key in _REF:
        return _REF[key]
    nv, B, J = c["nviews"], c["B"], c["J"]
    P = [{n: t.double().requires_grad_() for n, t in p.items()} for p in c["pred"]]
    terms = loss_terms(c, P, SD64)
    terms[0].backward()
    grads = [{n: (torch.zeros_like(t) if t.grad is None else t.grad) for n, t in p.items()} for p in P]
    t = torch.stack(terms).detach()
    w = [float(x) for x in c["w"]]
    k = coefs(c)
    views, cs, ch = nv - 1, -(-B // LT), -(-2 * J // LT)
    xb = 1 if c["cross"] & X_BETAS else 0
    dmax = max(float(p["depth"][:, c["col"]].abs().max()) for p in c["pred"])
    n = dict(keypoints=6 + ch + 8 + cs + 8 + 1 + views, pose=3 + 9 + 21 + cs + 8 + 1, betas=3 + 10 + cs + 8 + 1 + views + xb,
             depth=2 * (c["gain"] * dmax + 2) + 1 + cs + 8 + 1 + views)
    mags = [vposer_magnitudes(c, v) for v in range(nv)]
    A_vp = sum(m[0] for m in mags)
    bound = {name: n[name] * U32 * abs(float(t[TERMS.index(name)])) for name in n}
    tv = {name: float(t[TERMS.index(name)]) for name in TERMS}
    bound["loss"] = abs(w[5]) * (abs(w[0]) * bound["keypoints"] + abs(w[1]) * bound["betas"] + abs(w[2]) * GS.TAU * A_vp +
                                 abs(w[3]) * bound["pose"] + bound["depth"]) + \
        6 * U32 * abs(w[5]) * (abs(w[0] * tv["keypoints"]) + abs(w[1] * tv["betas"]) + abs(w[2] * tv["vposer"]) + abs(w[3] * tv["pose"]) +
                               abs(tv["depth"]))
    gA, gn = [], []
    lw = limb_vec(abs(w[4]), torch.float64)[None, :, None]
    for v in range(nv):
        p, o = c["pred"][v], c["pred"][1 - v] if nv == 2 else None
        a = lambda x: x.double().abs()
        A = {}
        A["j2d"] = torch.zeros(B, J, 2, dtype=torch.float64)
        g = c["gt"][v].double()
        A["j2d"][:, :NJ] = abs(k["kp"]) * g[:, :NJ, 2:] * lw * (a(p["j2d"])[:, :NJ] + g[:, :NJ, :2].abs())
        A["betas"] = abs(k["beta"]) * (a(p["betas"]) + ((a(p["betas"]) + a(o["betas"])) if xb else 0.0))
        A["depth"] = torch.zeros(B, 3, dtype=torch.float64)
        A["depth"][:, c["col"]] = abs(k["depth"]) * torch.exp(-2.0 * c["gain"] * p["depth"][:, c["col"]].double())
        A["rotmat"] = torch.zeros(B, NJ, 3, 3, dtype=torch.float64)
        A["rotmat"][:, 1:] = mags[v][1]
        if c["cross"] & X_POSE:
            A["rotmat"][:, 1:] += abs(k["pose"]) * (a(p["rotmat"])[:, 1:] + a(o["rotmat"])[:, 1:])
        gA.append(A)
        gn.append(dict(j2d=6.0, betas=5.0, depth=2 * (c["gain"] * p["depth"][:, c["col"]:c["col"] + 1].double().abs() + 2) + 3))
    _REF[key] = dict(terms=t, grads=grads, bound=bound, A_vp=A_vp, gA=gA, gn=gn)
    return _REF[key]


def cpu32(c):
    """the same restatement evaluated in fp32 on the CPU: the yardstick of the per-joint rule"""
    key = ("cpu32",) + case_key(c)
    if key not in _REF:
        P = [{n: t.clone().requires_grad_() for n, t in p.items()} for p in c["pred"]]
        loss_terms(c, P, SD)[0].backward()
        _REF[key] = [p["rotmat"].grad for p in P]
    return _REF[key]


def verify(c, ref, terms, grads, what, ratios=None):
    """-> list of failures of (terms (6,), grads: per view dict of PRED or None entries) against ref's bars"""
    fails = []
    ratios = {} if ratios is None else ratios

    def flat(name, got, want, bound):
        ok, ratio, nz, msg = evaluate(got, want, bound)
        ratios[name] = max(ratios.get(name, 0.0), ratio)
        if not ok:
            fails.append((what, name, msg))

    for name in ("loss", "pose", "keypoints", "betas", "depth"):
        i = TERMS.index(name)
        flat(name, terms[i:i + 1], ref["terms"][i:i + 1], torch.tensor([ref["bound"][name]], dtype=torch.float64))
    try:
        GS.check(what, "vposer", terms[1:2], ref["terms"][1:2], torch.tensor([ref["A_vp"]], dtype=torch.float64), ratios)
    except AssertionError as e:
        fails.append((what, "vposer", str(e)))
    for v, gv in enumerate(grads):
        for name in ("j2d", "betas", "depth"):
            if gv.get(name) is not None:
                flat("g_%s%d" % (name, v), gv[name], ref["grads"][v][name], ref["gn"][v][name] * U32 * ref["gA"][v][name])
        if gv.get("rotmat") is None:
            continue
        name = "g_rotmat%d" % v
        got, want, A = gv["rotmat"], ref["grads"][v]["rotmat"], ref["gA"][v]["rotmat"]
        if got[:, 0].abs().max() != 0:
            fails.append((what, name, "row 0 is not exactly zero"))
        try:
            GS.check(what, name, got, want, A, ratios)
            ratios[name + " bar"] = "tau A"
        except AssertionError as first:
            if (c["form"], c["B"], c["J"], c["Jg"], float(c["w"][4])) not in FALLBACK_ALLOWED:
                fails.append((what, name, "%s (and the case is not in FALLBACK_ALLOWED)" % first))
                continue
            try:
                GS.check_slices(what, name + " slices", got[:, 1:], want[:, 1:], cpu32(c)[v][:, 1:], 1, ratios)
                ratios[name + " bar"] = "4 x fp32 CPU per joint (tau A: %.2f)" % ratios.get(name, float("nan"))
            except AssertionError as second:
                fails.append((what, name, "%s; then %s" % (first, second)))
    return fails


def show(what, ratios):
    print("%-40s %s" % (what, "  ".join("%s %s" % (k, v if isinstance(v, str) else "%.3f" % v) for k, v in ratios.items())))


# ------------------------------------------------------------------------------------------------ fp32 emulation in the kernel's order
def _rows_sum(per_row):
    """the combine over one view's rows: thread t adds rows t, t + 256, .. in order, then the tree"""
    return _strided_sum(per_row)


def _serial(x):
    """sum over the last dimension in index order"""
    acc = torch.zeros_like(x[..., 0])
    for i in range(x.shape[-1]):
        acc = acc + x[..., i]
    return acc


def emulate(c, mut=None):
    """fp32, the kernel's operations and order -> (terms (6,) fp32, grads per view)"""
    f = torch.float32
    nv, B, J = c["nviews"], c["B"], c["J"]
    w = c["w"].clone()
    k = {n: torch.tensor(x, dtype=torch.float64).to(f) for n, x in coefs(c).items()}
    sd = SD
    if mut == "bn_unfolded":                                   # BatchNorm taken as the identity instead of being folded
        sd = dict(SD)
        for i, n in ((1, 63), (4, 512)):
            sd["encoder_net.%d.weight" % i], sd["encoder_net.%d.bias" % i] = torch.ones(n), torch.zeros(n)
            sd["encoder_net.%d.running_mean" % i], sd["encoder_net.%d.running_var" % i] = torch.zeros(n), torch.ones(n) - 1e-5
    W1, b1, W2, b2 = [t.to(f) for t in folded(sd, 1e-3 if mut == "bn_wrong_eps" else None)]
    sets = (LIMB1, LIMB2)
    if mut == "limb_sets_shifted":
        sets = (tuple(j - 1 for j in LIMB1), tuple(j - 1 for j in LIMB2))
    lw = limb_vec(w[4], f, sets=sets)[None, :, None]
    xp, xb = bool(c["cross"] & X_POSE), bool(c["cross"] & X_BETAS)
    P = c["pred"]
    S = {n: [] for n in ("kp", "vp", "pose", "bet", "betc", "depth")}
    grads = []
    for v in range(nv):
        p = P[v]
        R = p["rotmat"].clone().requires_grad_()
        aa = axis_angle(R)
        x = aa.detach()
        h = b1.expand(B, 512).clone()
        for j in range(63):
            h = h + W1[:, j] * x[:, j:j + 1]
        a = torch.where(h > 0, h, 0.01 * h)
        parts = []
        for s_ in range(4):
            acc = torch.zeros(B, 64, dtype=f)
            for i in range(s_ * SEG, (s_ + 1) * SEG):
                acc = acc + W2[:, i] * a[:, i:i + 1]
            parts.append(acc)
        out = ((parts[0] + parts[1]) + parts[2]) + parts[3] + b2
        mu, s = out[:, :NZ], out[:, NZ:]
        e = torch.ones_like(c["eps"][v]) if mut == "eps_dropped" else c["eps"][v]
        if mut == "softplus_as_exp":
            sp, dsp = torch.exp(s), torch.exp(s)
        else:
            sp, dsp = torch.where(s > 20, s, torch.log1p(torch.exp(s))), torch.where(s > 20, torch.ones_like(s), 1 / (1 + torch.exp(-s)))
        z = sp * e + mu
        S["vp"].append(_rows_sum(_serial(z * z)))
        dz = k["vp"] * z
        dout = torch.cat([dz, (dz * e) * dsp], 1)
        da = torch.zeros(B, 512, dtype=f)
        for o in range(64):
            da = da + W2[o] * dout[:, o:o + 1]
        dh = torch.where(h > 0, da, 0.01 * da)
        parts = []
        for s_ in range(4):
            acc = torch.zeros(B, 63, dtype=f)
            for i in range(s_ * SEG, (s_ + 1) * SEG):
                acc = acc + W1[i] * dh[:, i:i + 1]
            parts.append(acc)
        daa = ((parts[0] + parts[1]) + parts[2]) + parts[3]
        gvp, = torch.autograd.grad(aa, R, grad_outputs=daa)
        gR = torch.zeros(B, NJ, 3, 3, dtype=f)
        share = torch.zeros(B, NR, 3, 3, dtype=f)
        if xp:
            dc = P[0]["rotmat"][:, 1:] - P[1]["rotmat"][:, 1:]
            share = k["pose"] * dc
            if v == 1:
                share = -share
            if v == 0:
                S["pose"].append(_rows_sum(_serial(_serial((dc * dc).reshape(B, NR, 9)))))
        gR[:, 1:] = gvp[:, 1:] if mut == "vposer_overwrites_pose" else share + gvp[:, 1:]
        # keypoints
        g = c["gt"][v]
        d = p["j2d"][:, :NJ] - g[:, :NJ, :2]
        wgt = lw if mut == "dropped_confidence" else g[:, :NJ, 2:] * lw
        vals = torch.zeros(B, 2 * J, dtype=f)
        vals[:, :2 * NJ] = ((d * d) * wgt).reshape(B, -1)
        S["kp"].append(_rows_sum(torch.stack([_strided_sum(vals[b]) for b in range(B)])))
        gj = torch.zeros(B, J, 2, dtype=f)
        gj[:, :NJ] = (k["kp"] * wgt) * d
        # betas
        xb_ = p["betas"]
        dcb = (P[0]["betas"] - P[1]["betas"]) if xb else torch.zeros_like(xb_)
        S["bet"].append(_rows_sum(_serial(xb_ * xb_)))
        if xb and v == 0:
            S["betc"].append(_rows_sum(_serial(dcb * dcb)))
        gb = k["beta"] * (xb_ + dcb if v == 0 else xb_ - dcb)
        # depth
        ex = torch.exp(-torch.tensor(c["gain"], dtype=f) * p["depth"][:, c["col"]])
        q = ex * ex
        S["depth"].append(_rows_sum(q))
        gd = torch.zeros(B, 3, dtype=f)
        gd[:, c["col"]] = k["depth"] * q
        grads.append(dict(rotmat=gR, betas=gb, j2d=gj, depth=gd))
    n = lambda x: torch.tensor(float(x), dtype=f)
    two = nv == 2
    per = lambda name, den: S[name][0] / n(den) + (S[name][1] / n(den) if two else 0)
    kp, vp, depth = per("kp", 44 * B), per("vp", NZ * B), per("depth", B)
    pose = S["pose"][0] / n(189 * B) if xp else torch.zeros((), dtype=f)
    betas = per("bet", 10 * B)
    if two:
        betas = betas + (S["betc"][0] if xb else torch.zeros((), dtype=f)) / n(10 * B)
    loss = w[0] * kp
    loss = loss + w[1] * betas
    loss = loss + w[2] * vp
    loss = loss + w[3] * pose
    loss = (loss + depth) * w[5]
    return torch.stack([loss, vp, pose, kp, betas, depth]), grads


def assert_inputs(c):
    """in fp64 on the CPU: no rotation inside a band of the conversion, all four quaternion branches populated, some confidences 0"""
    from real_loss_util import too_close
    for v in range(c["nviews"]):
        R = c["pred"][v]["rotmat"][:, 1:].reshape(-1, 3, 3).double()
        assert not too_close(R).any()
        br = branch_of(R)
        assert sorted(set(br.tolist())) == [0, 1, 2, 3], ("branches", sorted(set(br.tolist())))
        conf = c["gt"][v][:, :NJ, 2]
        assert (conf == 0).any() and (conf > 0).any()


SELF_CASES = [("twoview", 1, 22, 25, 1.5), ("twoview", 3, 25, 22, 1.0), ("hmr", 2, 25, 22, 1.5), ("spin", 33, 22, 25, 1.5)]


@pytest.mark.parametrize("form,B,J,Jg,l", SELF_CASES)
def test_cpu_fp32_emulation_is_inside_every_bar(form, B, J, Jg, l):
    c = make_case(form, B, J, Jg, limbs=l)
    assert_inputs(c)
    ref = reference(c)
    ratios = {}
    terms, grads = emulate(c)
    fails = verify(c, ref, terms, grads, "emulation", ratios)
    show("%s B %d J %d (drawn again: %d)" % (form, B, J, c["redrawn"]), ratios)
    assert not fails, fails


@pytest.mark.parametrize("mut", MUTATIONS)
def test_cpu_mutations_are_rejected(mut):
    c = make_case("twoview", 3, 25, 22, limbs=1.5)
    ref = reference(c)
    terms, grads = emulate(c, mut=mut)
    fails = verify(c, ref, terms, grads, mut)
    assert fails, "the bars accept the mutation %s" % mut
    names = {f[1] for f in fails}
    want = {"dropped_confidence": "g_j2d0", "limb_sets_shifted": "g_j2d1", "softplus_as_exp": "vposer", "eps_dropped": "vposer",
            "bn_wrong_eps": "g_rotmat0", "vposer_overwrites_pose": "g_rotmat1", "bn_unfolded": "vposer"}[mut]
    assert want in names, (mut, sorted(names))


def test_redraws_happen_and_leave_nothing_out():
    c = make_case("twoview", 33, 22, 25)
    assert_inputs(c)
    assert c["pred"][0]["rotmat"].shape == (33, 22, 3, 3) and 0 < c["redrawn"] < 300


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
def run(c, dev, packed, want=None, off=0):
    """one apg_real_loss_fwd_bwd call -> (terms (6,) cpu, grads per view).  want: set of (view, name) gradients to ask for (None = all;
    empty = the grads table itself NULL).  off: every input and output pointer starts `off` floats past a 16-byte boundary"""
    from airpose_amd import _native_grad as G
    L = G.lib()
    nv, B, J, Jg = c["nviews"], c["B"], c["J"], c["Jg"]
    every = {(v, n) for v in range(nv) for n in PRED}
    want = every if want is None else set(want)
    pred = [_place(c["pred"][v][n], dev, off) for v in range(nv) for n in PRED]
    gt = []
    for v in range(nv):
        gt += [_place(c["gt"][v], dev, off), _place(c["eps"][v], dev, off)]
    outs = [Buf(dev, c["pred"][v][n].numel(), off) if (v, n) in want else None for v in range(nv) for n in PRED]
    terms = Buf(dev, len(TERMS), off)
    nbytes = L.apg_real_loss_workspace_bytes(B)
    assert nbytes > 0
    ws = Buf(dev, nbytes // 4)
    w = (ctypes.c_float * 6)(*[float(x) for x in c["w"]])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    table = G.ptrs([None if o is None else o.out for o in outs]) if want else None
    rc = L.apg_real_loss_fwd_bwd(nv, c["cross"], B, J, Jg, c["col"], c["gain"], w, p(packed), G.ptrs(pred), G.ptrs(gt), p(terms.out), table,
                                 p(ws.out), nbytes, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    G.check(rc, "apg_real_loss_fwd_bwd")
    torch.cuda.synchronize()
    lo = GUARD + nbytes // 4
    assert torch.isnan(ws.buf[:GUARD]).all() and torch.isnan(ws.buf[lo:]).all(), "the workspace's guard bands were written"
    grads = [{n: (None if outs[v * len(PRED) + k] is None else
                  outs[v * len(PRED) + k].values(c["pred"][v][n].shape, "g_%s%d" % (n, v))) for k, n in enumerate(PRED)} for v in range(nv)]
    return terms.values((len(TERMS),), "terms"), grads


def run_twice_and_verify(c, dev, packed, what, **kw):
    got = run_twice(lambda: run(c, dev, packed, **kw), what)
    ratios = {}
    fails = verify(c, reference(c), got[0], got[1], what, ratios)
    show(what, ratios)
    assert not fails, fails
    return got


GRID = [(form, B, J, Jg, l) for form in FORMS for (B, J, Jg, l) in ((1, 22, 25, 1.5), (2, 25, 22, 1.0), (3, 25, 24, 1.5), (33, 22, 25, 1.5))]
EDGES = [("spin", 256, 22, 25, 1.5), ("spin", 257, 22, 25, 1.5),           # the combine's stride: 256 | 257 rows of a view
         ("twoview", 256, 22, 25, 1.5), ("twoview", 257, 22, 25, 1.0), ("hmr", 33, 25, 22, 1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,B,J,Jg,l", GRID + EDGES)
def test_loss_and_seeds_against_fp64(dev, packed, form, B, J, Jg, l):
    c = make_case(form, B, J, Jg, limbs=l)
    assert_inputs(c)
    run_twice_and_verify(c, dev, packed, "%s B %d J %d Jg %d l %g" % (form, B, J, Jg, l))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["twoview", "hmr"])
def test_each_gradient_pointer_null_in_turn_and_all_null(dev, packed, form):
    """which gradients are asked for changes neither the terms nor any other gradient, bit for bit"""
    c = make_case(form, 3, 25, 22)
    full = run_twice_and_verify(c, dev, packed, form + " all gradients")
    every = [(v, n) for v in range(c["nviews"]) for n in PRED]
    for drop in every:
        got = run(c, dev, packed, want=[e for e in every if e != drop])
        assert got[1][drop[0]][drop[1]] is None
        assert torch.equal(got[0].view(torch.int32), full[0].view(torch.int32)), drop
        for v, n in every:
            if (v, n) != drop:
                assert torch.equal(got[1][v][n].view(torch.int32), full[1][v][n].view(torch.int32)), (drop, v, n)
    fwd = run(c, dev, packed, want=[])
    assert torch.equal(fwd[0].view(torch.int32), full[0].view(torch.int32))
    only = run(c, dev, packed, want=[(c["nviews"] - 1, "rotmat")])
    v = c["nviews"] - 1
    assert torch.equal(only[1][v]["rotmat"].view(torch.int32), full[1][v]["rotmat"].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_pointers_off_a_16_byte_boundary(dev, packed, off):
    c = make_case("twoview", 3, 25, 22)
    base = run(c, dev, packed)
    got = run_twice_and_verify(c, dev, packed, "every pointer offset by %d floats" % off, off=off)
    assert bit_equal(got, base), off


@pytest.mark.gpu
def test_zero_weights_give_exactly_zero_seeds(dev, packed):
    for k, name in ((0, "j2d"), (1, "betas")):
        w = [0.001, 1.0, 1.0, 1.0, 1.5, 60.0]
        w[k] = 0.0
        c = make_case("twoview", 3, 25, 22, weights=w)
        got = run(c, dev, packed)
        for v in range(2):
            assert not got[1][v][name].any(), (name, v)
    w = [0.001, 1.0, 0.0, 0.0, 1.5, 60.0]                                   # neither the prior nor the pose term: g_rotmat is zero
    got = run(make_case("twoview", 3, 25, 22, weights=w), dev, packed)
    for v in range(2):
        assert not got[1][v]["rotmat"].any()
        assert not got[1][v]["j2d"][:, NJ:].any() and not got[1][v]["depth"][:, :2].any()
