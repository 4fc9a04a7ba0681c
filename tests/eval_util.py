"""Shared by test_eval_fp64.py and test_eval_module.py: the fp64 restatement of apg_eval_update (airpose_amd/csrc/eval_metrics.hip),
the fp32 emulation of the kernel's instruction sequence, the error bars counted from that sequence, the cases and the GPU call.
The derivation of the bars is in test_eval_fp64.py's docstring."""
import math

import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
NJ = 22
WAVE = 64                                # eval_metrics.hip: ET
ACC = 28                                 # include/airpose_grad.h: APG_EVAL_ACC_PER_VIEW
SINCOS_ULP = 2.0                         # allowed error of sinf / cosf in ulps of the result (HIP documents 1)
MUTATIONS = ("parent_off_by_one", "taylor_always", "eps_dropped", "rotation_transposed", "root_not_at_j0", "mean_over_21",
             "trans_err_squared", "gt_orient_views_swapped")


def spw(views):
    """eval_metrics.hip: samples per workgroup"""
    return 32 // views


# ------------------------------------------------------------------------------------------------ the computation, fp64 or emulated
def _fma(a, b, c, emu):
    if emu:                                              # the product of two floats is exact in fp64; one rounding to float
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _dot3(x0, y0, x1, y1, x2, y2, emu):
    if emu:
        return _fma(x2, y2, _fma(x1, y1, x0 * y0, emu), emu)
    return x0 * y0 + x1 * y1 + x2 * y2


def _norm3(d, emu):
    return torch.sqrt(_dot3(d[..., 0], d[..., 0], d[..., 1], d[..., 1], d[..., 2], d[..., 2], emu))


def aa_to_rotmat(r, emu=False, mutation=None):
    """tgm 0.1.2 angle_axis_to_rotation_matrix on (N, 3) -> (N, 3, 3) and the intermediates the bars need"""
    x, y, z = r.unbind(-1)
    t2 = _dot3(x, x, y, y, z, z, emu)
    eps = torch.tensor(1e-6, dtype=r.dtype)
    big = t2 > eps
    if mutation == "taylor_always":
        big = torch.zeros_like(big)
    th = torch.sqrt(torch.where(big, t2, torch.ones_like(t2)))
    d = th if mutation == "eps_dropped" else th + eps
    w = r / d[:, None]
    c, s = torch.cos(th), torch.sin(th)
    omc = 1 - c
    a = w * omc[:, None]
    sv = w * s[:, None]
    wx, wy = w[:, 0], w[:, 1]
    wz = w[:, 2]
    ax, ay, az = a.unbind(-1)
    sx, sy, sz = sv.unbind(-1)
    f = lambda p, q, t: _fma(p, q, t, emu)
    Rb = torch.stack([f(wx, ax, c), f(wx, ay, -sz), f(wx, az, sy), f(wx, ay, sz), f(wy, ay, c), f(wy, az, -sx),
                      f(wx, az, -sy), f(wy, az, sx), f(wz, az, c)], -1)
    one = torch.ones_like(x)
    Rs = torch.stack([one, -z, y, z, one, -x, -y, x, one], -1)
    R = torch.where(big[:, None], Rb, Rs).view(-1, 3, 3)
    return R, dict(big=big, th=th, w=w, c=c, s=s, omc=omc, a=a, sv=sv, R=R)


def chain(R, J, parents, emu=False, mutation=None):
    """lbs.batch_rigid_transform on joints 0 .. 21: R (N, 22, 3, 3), J (22, 3) -> G (N, 22, 3, 3), p (N, 22, 3)"""
    N = R.shape[0]
    G, p = [R[:, 0]], [torch.zeros(N, 3, dtype=R.dtype) if mutation == "root_not_at_j0" else J[0].expand(N, 3)]
    for j in range(1, NJ):
        P = parents[j]
        if mutation == "parent_off_by_one" and P >= 1:
            P -= 1
        Gp, pp, Rj = G[P], p[P], R[:, j]
        b = J[j] - J[P]
        Gj = torch.stack([torch.stack([_dot3(Gp[:, i, 0], Rj[:, 0, k], Gp[:, i, 1], Rj[:, 1, k], Gp[:, i, 2], Rj[:, 2, k], emu)
                                       for k in range(3)], -1) for i in range(3)], -2)
        pj = torch.stack([pp[:, i] + _dot3(Gp[:, i, 0], b[0], Gp[:, i, 1], b[1], Gp[:, i, 2], b[2], emu) for i in range(3)], -1)
        G.append(Gj)
        p.append(pj)
    return torch.stack(G, 1), torch.stack(p, 1)


def reference(case, emu=False, mutation=None, j_rest=None):
    """apg_eval_update's semantics on the case's fp32 values: in fp64 (emu = False), or in fp32 with the kernel's exact sequence
    (emu = True: emulate()).  j_rest overrides the case's rounded rest joints (test (a) feeds the unrounded product).
    -> joint_err (views, B, 22), trans_err (views, B) or None, angle_err (views, B, 22) or None, p_gt / p_pred (views, B, 22, 3) and
    what bars() needs"""
    dt = torch.float32 if emu else torch.float64
    J = (case["j_rest"] if j_rest is None else j_rest).to(dt)
    B, views = case["B"], case["views"]
    body = case["gt_body"].to(dt)
    out = dict(joint_err=[], trans_err=[], angle_err=[], p_gt=[], p_pred=[], G_gt=[], G_pred=[], R_gt=[], R_pred=[], conv=[])
    for v in range(views):
        d = case["view"][v]
        o = case["view"][1 - v]["gt_orient"] if (mutation == "gt_orient_views_swapped" and views == 2) else d["gt_orient"]
        Rg = torch.cat([o.to(dt), body], 1)
        if case["mode"] == "aa":
            Rp, conv = aa_to_rotmat(d["pred"].to(dt).reshape(-1, 3), emu, mutation)
            Rp = Rp.view(B, NJ, 3, 3)
        else:
            Rp, conv = d["pred"].to(dt), None
        if mutation == "rotation_transposed":
            Rp = Rp.transpose(-1, -2)
        Gg, pg = chain(Rg, J, case["parents"], emu, mutation)
        Gp, pp = chain(Rp, J, case["parents"], emu, mutation)
        out["joint_err"].append(_norm3(pp - pg, emu))
        if d["pred_trans"] is not None:
            t = _norm3(d["pred_trans"].to(dt) - d["gt_trans"].to(dt), emu)
            out["trans_err"].append(t * t if mutation == "trans_err_squared" else t)
        if d["gt_angles"] is not None:
            out["angle_err"].append(_norm3(d["pred"].to(dt) - d["gt_angles"].to(dt), emu))
        for k, t in (("p_gt", pg), ("p_pred", pp), ("G_gt", Gg), ("G_pred", Gp), ("R_gt", Rg), ("R_pred", Rp), ("conv", conv)):
            out[k].append(t)
    for k in ("joint_err", "trans_err", "angle_err", "p_gt", "p_pred"):
        out[k] = torch.stack(out[k]).double() if len(out[k]) == views else None
    return out


def emulate(case, mutation=None):
    return reference(case, emu=True, mutation=mutation)


# ------------------------------------------------------------------------------------------------ the bars
def _conv_bars(conv, B):
    """bound on each entry of the converted matrix (B, 22, 3, 3); zero in the first-order branch, which is exact"""
    th, w, c, s, omc, a, sv = (conv[k].abs() for k in ("th", "w", "c", "s", "omc", "a", "sv"))
    sc = 2 * SINCOS_ULP * U                              # an ulp of a float v is at most 2 u |v|
    dth = 2.5 * U * th
    dw = 5.5 * U * w
    dc = s * dth + sc * c
    ds = c * dth + sc * s
    domc = dc + U * omc
    da = w * domc[:, None] + omc[:, None] * dw + U * a
    dsv = w * ds[:, None] + s[:, None] * dw + U * sv
    Rabs = conv["R"].abs()

    # (i, k, m): R[i][k] = fmaf(w_i', a_k', +-s_m) with the operands the kernel uses
    spec = [(0, 0, None), (0, 1, 2), (0, 2, 1), (0, 1, 2), (1, 1, None), (1, 2, 0), (0, 2, 1), (1, 2, 0), (2, 2, None)]
    cols = []
    for e, (i, k, m) in enumerate(spec):
        last = dc if m is None else dsv[:, m]
        cols.append(w[:, i] * da[:, k] + a[:, k] * dw[:, i] + last + U * Rabs[:, e // 3, e % 3])
    dR = torch.stack(cols, -1).view(-1, 3, 3)
    dR = torch.where(conv["big"][:, None, None], dR, torch.zeros_like(dR))
    return dR.view(B, NJ, 3, 3)


def _chain_bars(R, dR, G, p, J, parents):
    """bounds on the entries of G (N, 22, 3, 3) and p (N, 22, 3) of the kernel's chain, given the bound dR on its rotations"""
    EG, Ep = [dR[:, 0]], [torch.zeros_like(p[:, 0])]
    for j in range(1, NJ):
        P = parents[j]
        aG = G[:, P].abs() + EG[P]
        aR = R[:, j].abs() + dR[:, j]
        EG.append(EG[P] @ aR + G[:, P].abs() @ dR[:, j] + 3 * U * (aG @ aR))
        b = (J[j] - J[P]).abs()
        eb = U * b
        ab = b + eb
        dot = aG @ ab
        Ep.append(Ep[P] + EG[P] @ ab + G[:, P].abs() @ eb + 3 * U * dot + U * (p[:, P].abs() + Ep[P] + dot))
    return torch.stack(EG, 1), torch.stack(Ep, 1)


def _norm_bar(e, Ed):
    """|sqrtf(fma chain of d'^2) - |d||: the norm moves by at most |Ed|_1, three roundings under the root and its own on top"""
    s = Ed.sum(-1)
    return s + 3 * U * (e + s)


def bars(case, ref):
    """per-sample bars for joint_err, trans_err, angle_err and the positions, from the fp64 reference's own magnitudes"""
    B, views = case["B"], case["views"]
    J = case["j_rest"].double()
    out = dict(joint_err=[], trans_err=[], angle_err=[], p_gt=[], p_pred=[])
    for v in range(views):
        d = case["view"][v]
        zero = torch.zeros(B, NJ, 3, 3, dtype=torch.float64)
        dRp = _conv_bars(ref["conv"][v], B) if case["mode"] == "aa" else zero
        _, Eg = _chain_bars(ref["R_gt"][v], zero, ref["G_gt"][v], ref["p_gt"][v], J, case["parents"])
        _, Epd = _chain_bars(ref["R_pred"][v], dRp, ref["G_pred"][v], ref["p_pred"][v], J, case["parents"])
        diff = (ref["p_pred"][v] - ref["p_gt"][v]).abs()
        Ed = Eg + Epd + U * (diff + Eg + Epd)
        out["joint_err"].append(_norm_bar(ref["joint_err"][v], Ed))
        out["p_gt"].append(Eg)
        out["p_pred"].append(Epd)
        if d["pred_trans"] is not None:
            dd = (d["pred_trans"].double() - d["gt_trans"].double()).abs()
            out["trans_err"].append(_norm_bar(ref["trans_err"][v], U * dd))
        if d["gt_angles"] is not None:
            dd = (d["pred"].double() - d["gt_angles"].double()).abs()
            out["angle_err"].append(_norm_bar(ref["angle_err"][v], U * dd))
    return {k: (torch.stack(x) if len(x) == views else None) for k, x in out.items()}


def accumulate(refs, bars_list, views):
    """the accumulator ((2, 28) fp64) of a sequence of updates and its bar: the elements' bars summed, plus one fp64 rounding per
    addition on the running sum (bounded by the number of terms times 2^-53 times the sum of the magnitudes)"""
    acc = torch.zeros(2, ACC, dtype=torch.float64)
    bar = torch.zeros(2, ACC, dtype=torch.float64)
    for ref, b in zip(refs, bars_list):
        for v in range(views):
            je, bj = ref["joint_err"][v], b["joint_err"][v]
            n = je.shape[0]
            acc[v, 0] += n
            terms = [(1, je.sum(), bj.sum(), je.numel())] + [(2 + j, je[:, j].sum(), bj[:, j].sum(), n) for j in range(NJ)]
            if ref["trans_err"] is not None:
                terms.append((24, ref["trans_err"][v].sum(), b["trans_err"][v].sum(), n))
                acc[v, 26] += n
            if ref["angle_err"] is not None:
                terms.append((25, ref["angle_err"][v].sum(), b["angle_err"][v].sum(), je.numel()))
                acc[v, 27] += n
            for k, s, bs, cnt in terms:
                acc[v, k] += s
                bar[v, k] += bs + (cnt + 2) * U64 * (s.abs() + acc[v, k].abs())
    return acc, bar


def summarise(acc, views, mutation=None):
    """the module's compute() from the raw sums"""
    out = {}
    for v in range(views):
        n = float(acc[v, 0])
        out["mpjpe%d" % v] = float(acc[v, 1]) / (n * (21 if mutation == "mean_over_21" else NJ))
        if float(acc[v, 26]):
            out["mpe%d" % v] = float(acc[v, 24]) / float(acc[v, 26])
        if float(acc[v, 27]):
            out["angle_err%d" % v] = float(acc[v, 25]) / (float(acc[v, 27]) * NJ)
    return out


# ------------------------------------------------------------------------------------------------ cases
def rodrigues64(r):
    """exact Rodrigues formula in fp64 (unit axis): the orthonormal ground-truth rotations"""
    th = r.norm(dim=-1, keepdim=True).clamp_min(1e-300)
    k = r / th
    K = torch.zeros(r.shape[0], 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    th = th[:, :, None]
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


def _axes(n, gen):
    a = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return a / a.norm(dim=-1, keepdim=True)


SPECIAL_NORMS = (0.0, 0.9e-3, 1.1e-3, math.pi - 5e-4, math.pi + 5e-4)


def make_case(model_j, parents, B, views, mode, extras, seed=0):
    """mode "aa" / "rotmat"; extras: translations and (aa mode) gt angles are given.  Ground-truth rotations exactly orthonormal in
    fp64, then rounded, angles spread over (0, pi]; predictions at angles in (0, pi) with SPECIAL_NORMS planted (aa mode): the zero
    vector, |r| on either side of sqrt(eps) = 1e-3 (t2 = 0.81e-6 and 1.21e-6: a margin of 19 % that fp32 cannot cross) and |r|
    within 1e-3 of pi on both sides"""
    gen = torch.Generator().manual_seed(1000 * seed + 100 * views + B + (7 if mode == "aa" else 0) + (3 if extras else 0))
    case = dict(B=B, views=views, mode=mode, j_rest=model_j.clone(), parents=list(parents), view=[])
    n = B * 21
    ang = math.pi * (torch.arange(n, dtype=torch.float64) + 1) / n                # (0, pi], the last one pi itself
    case["gt_body"] = rodrigues64(_axes(n, gen) * ang[torch.randperm(n, generator=gen)][:, None]).view(B, 21, 3, 3).float()
    for v in range(views):
        ango = math.pi * (torch.arange(B, dtype=torch.float64) + 1) / B
        d = {"gt_orient": rodrigues64(_axes(B, gen) * ango[:, None]).view(B, 1, 3, 3).float()}
        m = B * NJ
        r = _axes(m, gen) * (math.pi * torch.rand(m, 1, generator=gen, dtype=torch.float64)).clamp_min(0.05)
        if mode == "aa":
            for k, nrm in enumerate(SPECIAL_NORMS):
                i = (k * 7 + v) % m
                r[i] = r[i] / r[i].norm() * nrm
            d["pred"] = r.view(B, NJ, 3).float()
        else:
            d["pred"] = rodrigues64(r).view(B, NJ, 3, 3).float()
        if extras:
            d["gt_trans"] = (torch.randn(B, 3, generator=gen) + torch.tensor([0.0, 0.0, 10.0])).float()
            d["pred_trans"] = (d["gt_trans"] + 0.3 * torch.randn(B, 3, generator=gen)).float()
        else:
            d["gt_trans"] = d["pred_trans"] = None
        d["gt_angles"] = (r.view(B, NJ, 3) + 0.2 * torch.randn(B, NJ, 3, generator=gen, dtype=torch.float64)).float() \
            if (extras and mode == "aa") else None
        case["view"].append(d)
    return case


def batch_sizes(views):
    s = spw(views)
    return sorted(set([1, 2, WAVE - 1, WAVE, WAVE + 1, s - 1, s, s + 1, 2 * s + 1]))     # 2 spw + 1: three workgroups


def concat_cases(cases):
    out = dict(cases[0])
    out["B"] = sum(c["B"] for c in cases)
    out["gt_body"] = torch.cat([c["gt_body"] for c in cases])
    out["view"] = [{k: (None if cases[0]["view"][v][k] is None else torch.cat([c["view"][v][k] for c in cases]))
                    for k in cases[0]["view"][v]} for v in range(out["views"])]
    return out


# ------------------------------------------------------------------------------------------------ the GPU call
GUARD = 64


class Arena(object):
    """device tensors carved out of one NaN-filled buffer, GUARD floats of NaN between and around them"""

    def __init__(self, dev, floats):
        self.buf = torch.full((floats,), float("nan"), device=dev, dtype=torch.float32)
        self.used = GUARD
        self.mask = torch.ones(floats, dtype=torch.bool, device=dev)

    def take(self, shape, src=None, dtype=torch.float32):
        n = int(torch.Size(shape).numel()) * (2 if dtype == torch.float64 else 1)
        self.used = (self.used + 3) // 4 * 4                     # 16-byte boundaries (8-byte ones for the fp64 tensors)
        t = self.buf[self.used:self.used + n]
        self.mask[self.used:self.used + n] = False
        self.used += n + GUARD
        assert self.used <= self.buf.numel()
        t = t.view(dtype).view(shape) if dtype != torch.float32 else t.view(shape)
        if src is not None:
            t.copy_(src)
        return t

    def guards_intact(self):
        return bool(torch.isnan(self.buf[self.mask]).all())


class GuardedCall(object):
    """the scaffolding of ONE call of a metric entry point into fresh guarded buffers: the arena, the inputs put into it (tracked,
    so that the call is seen to leave them alone), the accumulator, a workspace of exactly the queried size, the call itself and
    what the arena looks like afterwards"""

    def __init__(self, dev, floats):
        self.dev, self.ar, self.ins = dev, Arena(dev, floats), []

    def put(self, t, skew=False):
        """host tensor (None stays None) -> its copy in the arena; skew: the copy starts one float past a 16-byte boundary"""
        if t is None:
            return None
        if skew:
            g = self.ar.take((t.numel() + 1,))
            self.ar.mask[g.data_ptr() // 4 - self.ar.buf.data_ptr() // 4] = True      # the skipped float stays a guard
            g = g[1:].view(t.shape)
            g.copy_(t)
        else:
            g = self.ar.take(t.shape, t)
        self.ins.append((g, t))
        return g

    def sums(self, per_view, acc_init, nbytes):
        """-> (the (2, per_view) accumulator holding acc_init (None: zeros), a workspace of exactly nbytes)"""
        init = torch.zeros(2, per_view, dtype=torch.float64) if acc_init is None else torch.as_tensor(acc_init)
        return self.ar.take((2, per_view), init, dtype=torch.float64), self.ar.take(((nbytes + 7) // 8,), dtype=torch.float64)

    def run(self, G, call, what, res):
        """call() (-> the entry point's status) on dev, checked and synchronised; res gains inputs_ok and guards_ok"""
        with torch.cuda.device(self.dev):
            G.check(call(), what)
            torch.cuda.synchronize(self.dev)
        res = res()
        res["inputs_ok"] = all(torch.equal(g.cpu(), t) for g, t in self.ins)
        res["guards_ok"] = self.ar.guards_intact()
        return res


def run_gpu(case, dev, acc_init=None, per_sample=True):
    """one apg_eval_update into fresh guarded buffers -> dict(joint_err, trans_err, angle_err, acc (2, 28), guards_ok, inputs_ok),
    everything on the host"""
    from airpose_amd import _native_grad as G
    L, vp = G.lib(), G.vp
    B, views = case["B"], case["views"]
    gc = GuardedCall(dev, 4096 + B * views * (NJ * 9 + 9 + 6 + 2 * NJ * 3 + 2 * NJ + 1 + 8 * GUARD) + B * 21 * 9 + 64 * 1024)
    j, body = gc.put(case["j_rest"]), gc.put(case["gt_body"])
    table = [gc.put(d[k]) for d in case["view"] for k in ("gt_orient", "pred", "gt_trans", "pred_trans", "gt_angles")]
    has_t = all(d["pred_trans"] is not None for d in case["view"])
    has_a = all(d["gt_angles"] is not None for d in case["view"])
    je = gc.ar.take((views, B, NJ)) if per_sample else None
    te = gc.ar.take((views, B)) if per_sample and has_t else None
    ae = gc.ar.take((views, B, NJ)) if per_sample and has_a else None
    nbytes = L.apg_eval_workspace_bytes(B, views)
    assert nbytes > 0
    acc, ws = gc.sums(ACC, acc_init, nbytes)
    host = lambda t: None if t is None else t.cpu().clone()
    return gc.run(G, lambda: L.apg_eval_update(B, views, 0 if case["mode"] == "aa" else 1, vp(j), G.ints(case["parents"]), G.ptrs(table),
                                               vp(body), vp(je), vp(te), vp(ae), vp(acc), vp(ws), nbytes, G.stream(dev)),
                  "apg_eval_update", lambda: dict(joint_err=host(je), trans_err=host(te), angle_err=host(ae), acc=host(acc)))
