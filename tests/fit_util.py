"""Shared by tests/test_fit_fp64.py: the fp64 restatement of the AirPose+ fitting loop in the layout of ap_fit_run (per-frame loss
parts, packed gradient, plain Adam with the loop's two optimisers), the conditioned synthetic problems, the frame masks and the
per-element bar.  Everything here runs on the CPU; the reference's building blocks are oracle/fitting_ref.py's and
oracle/geometry_ref.py's."""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

from oracle import fitting_ref as Fr
from oracle import geometry_ref

KEYS = ("z", "phi0", "phi1", "tau0", "tau1", "beta")
NJ = Fr.NJ
DEFAULTS = dict(sigma=Fr.GM_SIGMA, w_vposer=Fr.W_VPOSER, w_temporal=Fr.W_TEMPORAL)
# deliberate errors of the reference (test_cpu_mutations_are_rejected)
MUTATIONS = ("extr_transposed", "extr_translation_dropped", "intr_swapped", "hip_weight_one_step_late", "pair_accounted_to_first_frame",
             "pairs_plus_one", "leaky_slope_zero_in_backward", "rodrigues_eps_dropped", "adam_counter_not_restarted", "prior_divided_by_L")


# ------------------------------------------------------------------------------------------------ the body model
@functools.lru_cache(maxsize=None)
def full_model():
    """the synthetic SMPL-X of the suite (conftest's smplx_model fixture builds the same)"""
    from airpose_amd import smplx_model
    return smplx_model.make_synthetic_model(4321)


@functools.lru_cache(maxsize=None)
def joint_model():
    """The body as the fitter's kernels receive it: ap_smplx_create forms the rest joints as an affine function of the shape,
    J = J_template + J_shapedirs beta, in fp64 and rounds both tables to fp32.  Written as a 55-"vertex" model with the identity as
    joint regressor, so that fitting_ref.body_joints evaluates exactly this on it."""
    m = full_model()
    Jr = torch.as_tensor(m["J_regressor"]).double()
    jt = (Jr @ torch.as_tensor(m["v_template"]).double()).float()
    jsd = torch.einsum("jv,vkl->jkl", Jr, torch.as_tensor(m["shapedirs"]).double()[:, :, :10]).float()
    return {"v_template": jt, "shapedirs": jsd, "J_regressor": torch.eye(jt.shape[0]), "parents": m["parents"]}


# ------------------------------------------------------------------------------------------------ mutations that reach into the oracle
@contextlib.contextmanager
def _patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


class _LeakyDeadBackward(torch.autograd.Function):
    """LeakyReLU(0.01) whose backward uses slope 0 on the negative side"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.where(x > 0, x, 0.01 * x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * (x > 0).to(g.dtype)


def _decode_with_dead_leaky_backward(vp, z):
    """fitting_ref.vposer_decode with _LeakyDeadBackward for its two activations"""
    h = _LeakyDeadBackward.apply(F.linear(z, vp["w1"], vp["b1"]))
    h = _LeakyDeadBackward.apply(F.linear(h, vp["w2"], vp["b2"]))
    o = F.linear(h, vp["w3"], vp["b3"]).view(-1, 3, 2)
    b1 = F.normalize(o[:, :, 0], dim=1)
    b2 = F.normalize(o[:, :, 1] - (b1 * o[:, :, 1]).sum(1, keepdim=True) * b1, dim=-1)
    R = torch.stack([b1, b2, torch.cross(b1, b2, dim=1)], dim=-1)
    aa = geometry_ref.rotation_matrix_to_angle_axis(F.pad(R, [0, 1]))
    return aa.view(z.shape[0], 21, 3), R.view(z.shape[0], 21, 3, 3)


def _rodrigues_without_eps(r):
    """lbs.batch_rodrigues with angle = |r| where r != 0 (a zero vector keeps the 1e-8: without it the matrix is 0 / 0)"""
    eps = 1e-8 * (r.abs().sum(1, keepdim=True) == 0).to(r.dtype)
    angle = torch.norm(r + eps, dim=1, keepdim=True)
    d = r / angle
    c, s = torch.cos(angle).unsqueeze(1), torch.sin(angle).unsqueeze(1)
    rx, ry, rz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    z = torch.zeros_like(rx)
    K = torch.cat([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1).view(-1, 3, 3)
    return torch.eye(3, dtype=r.dtype).unsqueeze(0) + s * K + (1 - c) * torch.bmm(K, K)


# ------------------------------------------------------------------------------------------------ the objective in the kernel's layout
def ref_terms(vp, model, prm, data, it, sigma=Fr.GM_SIGMA, w_vposer=Fr.W_VPOSER, w_temporal=Fr.W_TEMPORAL, mut=None):
    """One evaluation of the objective of fitting_ref.loss_terms at iteration `it` (0-based), in the dtype of prm, from the oracle's
    building blocks, with the hyper-parameters as arguments -> (parts (L,4), totals).

    parts is the layout of ap_fit_run's loss history: column 0 = the frame's share of the 2-D term, column 1 = the pose-temporal
    share of the pair (f-1, f), accounted to frame f, column 2 = the rigid-temporal share of the same pair, column 3 = 0.
    totals: loss_2d, loss_temporal_pose, loss_temporal_rigid, loss_vposer and total = parts.sum() + w_vposer loss_vposer.

    data["robust"] is the frame mask as the ABI takes it: ints, any non-zero value selects the frame.  The empty cases: without a
    selected pair of neighbours (n_pairs = 0) the temporal terms and their gradients are 0; without a selected frame (n_robust = 0)
    the 2-D term and its gradients are 0.  The reference script (and fitting_ref.loss_terms) takes the mean of an empty set there
    and produces NaN; the kernel's zero contribution is the contract, and this function pins it."""
    z = prm["z"]
    L, dt = z.shape[0], z.dtype
    rob = torch.as_tensor(data["robust"]) != 0
    pair = rob[:-1] & rob[1:]
    n_rob, n_pairs = int(rob.sum()), int(pair.sum())
    zero = torch.zeros(L, dtype=dt)
    aa, _ = (_decode_with_dead_leaky_backward if mut == "leaky_slope_zero_in_backward" else Fr.vposer_decode)(vp, z)
    pose_body = aa.reshape(L, 63)
    # (body_joints looks lbs_batch_rodrigues up in its module: the one mutation inside it is put there for the call)
    with _patched(Fr, "lbs_batch_rodrigues", _rodrigues_without_eps) if mut == "rodrigues_eps_dropped" else contextlib.nullcontext():
        Jtr = Fr.body_joints(model, pose_body, prm["beta"])
    hip = torch.ones(NJ, dtype=dt)
    hip[1] = hip[2] = 0.5 ** (it if mut == "hip_weight_one_step_late" else it + 1)
    l2d = zero
    if n_rob > 0:
        for v in (0, 1):
            Rv = Fr.rotation_6d_to_matrix(prm["phi%d" % v])
            tm = torch.cat([Rv, prm["tau%d" % v].unsqueeze(2)], 2)
            _, j3d = geometry_ref.transform_smpl(tm, Jtr, Jtr)
            E = data["extr"][v]
            ER = E[:, :3].t() if mut == "extr_transposed" else E[:, :3]
            Et = torch.zeros(3, dtype=dt) if mut == "extr_translation_dropped" else E[:, 3]
            fx, fy, cx, cy = [data["intr"][1 - v if mut == "intr_swapped" else v, i] for i in range(4)]
            uv = geometry_ref.perspective_projection(j3d[:, :NJ], ER.unsqueeze(0).expand(L, -1, -1), Et.expand(L, -1), [fx, fy],
                                                     torch.stack([cx, cy]))
            for det in (0, 1):
                gt = data["j2d"][v, :, det]
                conf = gt[:, :, 2:] * hip.view(1, NJ, 1)
                per_frame = (conf * Fr.gmcclure(uv, gt[:, :, :2], sigma)).sum((1, 2)) / (2 * NJ * n_rob)
                l2d = l2d + torch.where(rob, per_frame, zero)
    tpose, trigid = zero, zero
    if n_pairs > 0:
        div = n_pairs + 1 if mut == "pairs_plus_one" else n_pairs
        sq = lambda x: ((x[1:] - x[:-1]) ** 2).sum(1)
        none = torch.zeros(L - 1, dtype=dt)
        tp = torch.where(pair, 10 * w_temporal * sq(pose_body) / (63 * div), none)
        tr = sum(sq(prm["phi%d" % v]) / (6 * div) + sq(prm["tau%d" % v]) / (3 * div) for v in (0, 1))
        tr = torch.where(pair, 100 * w_temporal * tr, none)
        pad = torch.zeros(1, dtype=dt)
        first = mut == "pair_accounted_to_first_frame"
        tpose = torch.cat([tp, pad]) if first else torch.cat([pad, tp])
        trigid = torch.cat([tr, pad]) if first else torch.cat([pad, tr])
    prior = (z * z).sum() / L if mut == "prior_divided_by_L" else (z * z).mean()
    parts = torch.stack([l2d, tpose, trigid, zero], 1)
    total = parts.sum() + w_vposer * prior
    return parts, dict(total=total, loss_2d=l2d.sum(), loss_temporal_pose=tpose.sum(), loss_temporal_rigid=trigid.sum(), loss_vposer=prior)


def ref_grads(vp, model, prm, data, it, **kw):
    """ref_terms and the gradient of its total by autograd -> (parts, grads per KEYS (zeros where the total does not depend on one))"""
    p = {k: prm[k].detach().clone().requires_grad_(True) for k in KEYS}
    parts, tot = ref_terms(vp, model, p, data, it, **kw)
    tot["total"].backward()
    return parts.detach(), {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in KEYS}


def ref_fit(vp, model, prm0, data, first_iter, n_iters, switch_iter, lr=Fr.LR, sigma=Fr.GM_SIGMA, w_vposer=Fr.W_VPOSER,
            w_temporal=Fr.W_TEMPORAL, mut=None):
    """Iterations first_iter .. first_iter + n_iters - 1 of the loop with a plain Adam (betas 0.9 / 0.999, eps 1e-8): a fresh state
    (moments zero, step counter restarted) at first_iter and at switch_iter; phi, tau and beta are stepped from the start, z joins
    at switch_iter -> (state after, parts of every iteration (n_iters,L,4), gradients of the last iteration)."""
    p = {k: prm0[k].detach().clone() for k in KEYS}
    hist, g, t = [], None, 0
    for j in range(first_iter, first_iter + n_iters):
        if j == first_iter or j == switch_iter:
            m = {k: torch.zeros_like(p[k]) for k in KEYS}
            s = {k: torch.zeros_like(p[k]) for k in KEYS}
            if not (mut == "adam_counter_not_restarted" and j != first_iter):
                t = 0
        t += 1
        parts, g = ref_grads(vp, model, p, data, j, sigma=sigma, w_vposer=w_vposer, w_temporal=w_temporal, mut=mut)
        hist.append(parts)
        for k in KEYS:
            if k == "z" and j < switch_iter:
                continue
            m[k] = 0.9 * m[k] + 0.1 * g[k]
            s[k] = 0.999 * s[k] + 0.001 * g[k] * g[k]
            p[k] = p[k] - (lr / (1.0 - 0.9 ** t)) * m[k] / (s[k].sqrt() / math.sqrt(1.0 - 0.999 ** t) + 1e-8)
    return p, torch.stack(hist), g


# ------------------------------------------------------------------------------------------------ inputs
def rodrigues64(r):
    """exact Rodrigues formula, (N,3) -> (N,3,3), fp64 (the test's own rotations: no 1e-8)"""
    r = torch.as_tensor(r, dtype=torch.float64).view(-1, 3)
    th = r.norm(dim=1).clamp_min(1e-300).view(-1, 1, 1)
    d = r / th.view(-1, 1)
    z = torch.zeros(r.shape[0], dtype=torch.float64)
    K = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).view(-1, 3, 3)
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


def _extrinsic(r, t):
    return torch.cat([rodrigues64(r)[0], torch.tensor(t, dtype=torch.float64).view(3, 1)], 1)


# view 1 always has a proper rotation and a translation; view 0 is the identity ("id") or a second, different pose ("rot")
CAMS = {"id": (_extrinsic((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), _extrinsic((0.2, -0.3, 0.1), (0.3, -0.2, 0.5))),
        "rot": (_extrinsic((-0.05, 0.04, 0.08), (-0.1, 0.05, 0.2)), _extrinsic((0.2, -0.3, 0.1), (0.3, -0.2, 0.5)))}


def _decoder_targets(decoder, g):
    """the 21 rotations that the decoder's output sits around (its last bias is their 6-D form)"""
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if decoder == "body":
        return rodrigues64(0.5 * rnd(21, 3))
    assert decoder == "all-branch"
    aa = torch.zeros(21, 3, dtype=torch.float64)
    for j in range(21):
        if j % 4 < 3:                                        # 2.6 rad about an axis near x, y, z: branches 0, 1, 2 of matrot2aa
            axis = 0.1 * rnd(3)
            axis[j % 4] += 1.0
            angle = 2.6
        else:                                                # 0.6 .. 1.2 rad about a skew axis: branch 3
            axis = torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64) + 0.3 * rnd(3)
            angle = 0.6 + 0.6 * float(torch.rand(1, generator=g, dtype=torch.float64))
        aa[j] = angle * axis / axis.norm()
    return rodrigues64(aa)


def _project(vp, motion, intr, extr):
    """pixel positions (2 views, L, 24, 2) of a motion's first 24 chain joints, as synthetic_problem forms them, through extr"""
    with torch.no_grad():
        aa, _ = Fr.vposer_decode(vp, motion["z"])
        Jtr = Fr.body_joints(full_model(), aa.reshape(-1, 63), motion["beta"])[:, :NJ]
        uv = []
        for v in (0, 1):
            X = torch.einsum("lij,lkj->lki", Fr.rotation_6d_to_matrix(motion["phi%d" % v]), Jtr) + motion["tau%d" % v].unsqueeze(1)
            X = torch.einsum("ij,lkj->lki", extr[v][:, :3], X) + extr[v][:, 3]
            uv.append(torch.stack([intr[v, 0] * X[..., 0] / X[..., 2] + intr[v, 2], intr[v, 1] * X[..., 1] / X[..., 2] + intr[v, 3]], -1))
    return torch.stack(uv)


@functools.lru_cache(maxsize=None)
def make_problem(L, seed, decoder, cams):
    """fitting_ref.synthetic_problem(L, seed) for the state, the intrinsics and the detections' noise and confidences; the
    extrinsics of CAMS[cams]; the decoder's last layer scaled by 0.1 around seeded target rotations.  The detections are moved with
    the cameras and the decoder: synthetic_problem's own noise (3 px) and confidences around the projection of ITS ground-truth
    motion through THIS decoder and THESE extrinsics, so that both views' residuals are of the order of sigma (left where the
    identity camera and the random decoder put them, view 1's would be hundreds of pixels: the flat tail of Geman-McClure, where
    a wrong adjoint hardly shows) -> (vp, prm, data): fp64 tensors holding the fp32 values that the kernel receives
    (data["robust"] is synthetic_problem's; the tests pass their own masks)"""
    vp0, prm, data, motion = Fr.synthetic_problem(full_model(), L=L, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(1000003 * seed + 17)
    vp = dict(vp0)
    vp["w3"] = 0.1 * vp["w3"]
    vp["b3"] = _decoder_targets(decoder, g)[:, :, :2].reshape(126)
    data = dict(data)
    extr = torch.stack(CAMS[cams])
    noise = data["j2d"][..., :2] - _project(vp0, motion, data["intr"], data["extr"]).unsqueeze(2)
    j2d = data["j2d"].clone()
    j2d[..., :2] = _project(vp, motion, data["intr"], extr).unsqueeze(2) + noise
    data["j2d"], data["extr"] = j2d, extr
    r32 = lambda d: {k: (v.float().double() if v.is_floating_point() else v) for k, v in d.items()}
    return r32(vp), r32(prm), r32(data)


def branch_report(vp, z):
    """per (frame, joint) of the decoder's output: matrot2aa's branch, the chosen t = 4 q_max^2, and the distances of the two
    discriminants it passed (t22 against 1e-6; t00 against t11 or -t11) from their thresholds"""
    with torch.no_grad():
        aa, R = Fr.vposer_decode(vp, z)
    t00, t11, t22 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    low = t22 < 1e-6
    br = torch.where(low, torch.where(t00 > t11, 0, 1), torch.where(t00 < -t11, 2, 3))
    t = torch.stack([1 + t00 - t11 - t22, 1 - t00 + t11 - t22, 1 - t00 - t11 + t22, 1 + t00 + t11 + t22], -1).gather(-1, br.unsqueeze(-1))[..., 0]
    return dict(branch=br, t=t, d22=(t22 - 1e-6).abs(), d2=torch.where(low, (t00 - t11).abs(), (t00 + t11).abs()), angle=aa.norm(dim=-1))


def depths(prob):
    """camera-space depth of every projected joint, (2, L, 24)"""
    vp, prm, data = prob
    out = []
    with torch.no_grad():
        aa, _ = Fr.vposer_decode(vp, prm["z"])
        Jtr = Fr.body_joints(joint_model(), aa.reshape(-1, 63), prm["beta"])[:, :NJ]
        for v in (0, 1):
            X = torch.einsum("lij,lkj->lki", Fr.rotation_6d_to_matrix(prm["phi%d" % v]), Jtr) + prm["tau%d" % v].unsqueeze(1)
            E = data["extr"][v]
            out.append((torch.einsum("ij,lkj->lki", E[:, :3], X) + E[:, 3])[..., 2])
    return torch.stack(out)


def residuals(prob):
    """projection minus detection at the problem's initial state, pixels, (2 views, L, 2 detectors, 24, 2)"""
    vp, prm, data = prob
    with torch.no_grad():
        aa, _ = Fr.vposer_decode(vp, prm["z"])
        Jtr = Fr.body_joints(joint_model(), aa.reshape(-1, 63), prm["beta"])[:, :NJ]
        out = []
        for v in (0, 1):
            X = torch.einsum("lij,lkj->lki", Fr.rotation_6d_to_matrix(prm["phi%d" % v]), Jtr) + prm["tau%d" % v].unsqueeze(1)
            E, k = data["extr"][v], data["intr"][v]
            X = torch.einsum("ij,lkj->lki", E[:, :3], X) + E[:, 3]
            uv = torch.stack([k[0] * X[..., 0] / X[..., 2] + k[2], k[1] * X[..., 1] / X[..., 2] + k[3]], -1)
            out.append(uv.unsqueeze(1) - data["j2d"][v, ..., :2])
    return torch.stack(out)


def mask(name, L):
    """frame masks as the ABI takes them (int32, non-zero = selected)"""
    m = torch.ones(L, dtype=torch.int32)
    if name == "none":
        m[:] = 0
    elif name == "first_off":
        m[0] = 0
    elif name == "last_off":
        m[-1] = 0
    elif name == "interior_off":
        m[L // 2] = 0
    elif name == "alternating":                              # selected frames, but no pair of selected neighbours
        m[1::2] = 0
    elif name == "odd_values":                               # interior_off with 2 and -1 where it has 1
        m[L // 2] = 0
        m[m != 0] = torch.tensor([2, -1], dtype=torch.int32).repeat(L)[:int((m != 0).sum())]
    else:
        assert name == "all", name
    return m


# ------------------------------------------------------------------------------------------------ one call of ap_fit_run, restated
def pack_state(p):
    """KEYS dict -> the ABI's arrays z (L,32), phi (2,L,6), tau (2,L,3), beta (10,)"""
    return dict(z=p["z"], phi=torch.stack([p["phi0"], p["phi1"]]), tau=torch.stack([p["tau0"], p["tau1"]]), beta=p["beta"])


def ref_call(prob, robust, first_iter=0, n_iters=1, switch_iter=0, lr=0.0, dtype=torch.float64, mut=None, model=None, **hyper):
    """what one ap_fit_run call returns, from ref_fit in `dtype`: z, phi, tau, beta after the call, loss (n_iters,L,4), and the last
    gradient as dz (L,32), dphi (2,L,6), dtau (2,L,3), dbeta (10,) -- all as fp64"""
    vp, prm, data = prob
    cast = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    data = dict(cast(data), robust=torch.as_tensor(robust))
    h = dict(DEFAULTS, **hyper)
    p, hist, g = ref_fit(cast(vp), joint_model() if model is None else model, cast(prm), data, first_iter, n_iters, switch_iter, lr=lr,
                         mut=mut, **h)
    out = pack_state(p)
    out["loss"] = hist
    out.update({"d" + k: v for k, v in pack_state(g).items()})
    return {k: v.double() for k, v in out.items()}


KINDS = ("dz", "dphi", "dtau", "dbeta", "loss", "z", "phi", "tau", "beta")


def scale(ref):
    """|ref| + S per element, S = the largest |ref| of the element's row: one frame's 32, 6, 3 or 4 values, beta's whole vector"""
    a = ref.abs()
    return a + a.amax(-1, keepdim=True)


def ratios(got, ref):
    """worst |got - ref| / (|ref| + S) per output kind (an element whose |ref| + S is 0 counts 0 if it is exactly 0, else inf)"""
    out = {}
    for k in KINDS:
        err, sc = (got[k].double() - ref[k]).abs(), scale(ref[k])
        q = torch.where(sc > 0, err / torch.where(sc > 0, sc, torch.ones_like(sc)), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
        out[k] = float(q.max())
    return out
