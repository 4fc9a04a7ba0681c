"""What the gradient-norm tests share (test_gradnorm_abi.py, test_gradnorm_fp64.py, test_gradnorm_module.py): the cases, the fp64
reference and its bars, an emulation of the kernels' sequence (csrc/guard/grad_guard.hip: apg_grad_norm, apg_grad_scale, apg_adam_step_guarded)
with the mutations the bars must reject, and the runners that call the C ABI on the GPU.

Reference.  numpy / torch fp64 on exactly the fp32 values the kernels receive:
    S = sum g^2, norm = sqrt(S), coef = min(1, max_norm / (norm + 1e-6)), per_tensor[i] = sqrt(S_i)
Bars (counted, none measured), u = 2^-24, N the element count:
    norm        |got - ref| <= ref (u + (N + 2) 2^-53): a float squared is exact in fp64, the fp64 sum of N non-negative terms is off by at
                most (N - 1) 2^-53 relative in any order, one fp64 root, one rounding to float; all-zero gradients: exactly 0
    per_tensor  the same with the tensor's own count
    coef        |got - ref| <= u ref (the fp64 quotient's error is far below the one rounding to float); exactly 0 for max_norm = 0;
                exactly 1 where max_norm is clear of the norm: asserted for max_norm > 2 norm + 1e-5 (the cases use 4 x the norm and
                +inf).  Just above the norm the formula's eps still clips: max_norm / (norm + 1e-6) < 1 up to max_norm = norm + 1e-6
Non-finite: S is non-finite exactly when an element is NaN or +-Inf; then norm is non-finite, skip = skip_nonfinite, coef = 1 with skip
and NaN without.
"""
import ctypes
import math

import numpy as np
import torch

import test_optim_fp64 as F

U32 = 2.0 ** -24
C = F.C                                                  # adam_seq.inc: ADAM_CHUNK
T = 192                                                  # include/airpose_grad.h: APG_GRAD_NORM_BATCH
AT = 256                                                 # adam_seq.inc: threads of a chunk's workgroup
SIZES = (0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)
MIXED = (1, 3, 0, 4, 5, 64, 0, 257, 1023, C - 1, C, C + 1, 2048, 2 * C + 3, 37)
NORM_MUTATIONS = ("fp32_accumulation", "no_eps", "eps_inside_sqrt", "no_clamp", "sum_of_norms")
STEP_MUTATIONS = ("coef_after_weight_decay", "skip_updates_m")
GUARD = 64


# ------------------------------------------------------------------------------------------------ cases
def make_grads(sizes, seed=0):
    """|g| log-uniform in [1e-8, 1e-1] with a random sign and a tenth exact zeros: test_optim_fp64.make_tensor's gradients"""
    return [F.make_tensor(n, 9000 + 1000 * seed + i)["g"] if n else torch.zeros(0) for i, n in enumerate(sizes)]


def constant_grads(value, n=C + 1):
    """the two range cases: every |g| = value, signs alternating"""
    g = torch.full((n,), value, dtype=torch.float32)
    g[1::2] *= -1
    return [g]


def eps_case():
    """norm near 1e-5, to be clipped to max_norm = 1e-6: leaving eps out moves coef by 10 %"""
    g = torch.full((C + 1,), 1e-5 / math.sqrt(C + 1), dtype=torch.float32)
    g[::3] *= -1
    return [g], 1e-6


def mixed_sizes(n):
    return [MIXED[i % len(MIXED)] for i in range(n)]


# ------------------------------------------------------------------------------------------------ the fp64 reference and its bars
def reference(grads, max_norm):
    S_i = [float((g.double() ** 2).sum()) for g in grads]
    S = math.fsum(S_i)
    norm = math.sqrt(S) if S == S else float("nan")
    with np.errstate(all="ignore"):
        coef = float(np.minimum(1.0, np.float64(max_norm) / np.float64(norm + 1e-6)))
    return dict(S=S, norm=norm, coef=coef, per_tensor=[math.sqrt(s) if s == s else float("nan") for s in S_i],
                N=sum(g.numel() for g in grads), finite=math.isfinite(S))


def verify(got, grads, max_norm, skip_nonfinite=False):
    """got: dict(coef, norm, skip, per_tensor) as the record holds them (Python floats of the fp32 values) -> list of failures"""
    ref = reference(grads, max_norm)
    fails = []
    if not ref["finite"]:
        if math.isfinite(got["norm"]):
            fails.append(("norm", "finite %r for non-finite gradients" % got["norm"]))
        if got["skip"] != int(bool(skip_nonfinite)):
            fails.append(("skip", got["skip"]))
        if skip_nonfinite and got["coef"] != 1.0:
            fails.append(("coef", "%r with skip set" % got["coef"]))
        if not skip_nonfinite and got["coef"] == got["coef"]:
            fails.append(("coef", "%r, not NaN" % got["coef"]))
        return fails
    if got["skip"] != 0:
        fails.append(("skip", "set for finite gradients"))
    bar = ref["norm"] * (U32 + (ref["N"] + 2) * 2.0 ** -53)
    if not abs(got["norm"] - ref["norm"]) <= bar:
        fails.append(("norm", "got %r, reference %r, bar %.3e" % (got["norm"], ref["norm"], bar)))
    if ref["N"] == 0:
        want = 1.0
    else:
        want = ref["coef"]
    if max_norm > 2.0 * ref["norm"] + 1e-5 and got["coef"] != 1.0:
        fails.append(("coef", "%r, not exactly 1, for max_norm above the norm" % got["coef"]))
    if not abs(got["coef"] - want) <= U32 * want:
        fails.append(("coef", "got %r, reference %r" % (got["coef"], want)))
    if got.get("per_tensor") is not None:
        for i, (a, b, g) in enumerate(zip(got["per_tensor"], ref["per_tensor"], grads)):
            if not abs(a - b) <= b * (U32 + (g.numel() + 2) * 2.0 ** -53):
                fails.append(("per_tensor[%d]" % i, "got %r, reference %r" % (a, b)))
    return fails


# ------------------------------------------------------------------------------------------------ emulation of the kernels' sequence
def _chunk_partials(g, dtype):
    """one tensor's chunk partials in the kernel's order: a thread's (up to) 16 elements in element order, the 64 lanes of a wave
    folded 32, 16, .. 1, the four waves as ((w0 + w1) + w2) + w3.  (Zeros padded behind the tensor add nothing.)"""
    n = g.numel()
    nc = (n + C - 1) // C
    x = np.zeros(nc * C, dtype=dtype)
    x[:n] = g.numpy().astype(dtype)
    x = (x * x).reshape(nc, 4, AT, 4)                                     # [chunk][i][thread][k]: element (i * 256 + t) * 4 + k
    acc = np.zeros((nc, AT), dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(4):
            for k in range(4):
                acc = acc + x[:, i, :, k]
        w = acc.reshape(nc, 4, 64)
        off = 32
        while off:
            w = w[:, :, :off] + w[:, :, off:2 * off]
            off //= 2
        w = w[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _ordered(values, dtype):
    acc = dtype(0.0)
    with np.errstate(all="ignore"):
        for v in values:
            acc = dtype(acc + v)
    return acc


def emulate_norm(grads, max_norm, skip_nonfinite=False, mut=None):
    """the record and per_tensor apg_grad_norm writes, as Python floats of the fp32 values"""
    dtype = np.float32 if mut == "fp32_accumulation" else np.float64
    S_i = [_ordered(_chunk_partials(g, dtype), dtype) for g in grads]
    with np.errstate(all="ignore"):
        if mut == "sum_of_norms":
            nrm = np.float64(_ordered([np.sqrt(np.float64(s)) for s in S_i], np.float64))
            S = nrm * nrm
        else:
            S = np.float64(_ordered(S_i, dtype))
            nrm = np.sqrt(S)
        bad = not np.isfinite(S)
        if mut == "no_eps":
            c = np.float64(max_norm) / nrm if nrm else np.float64(np.inf)
        elif mut == "eps_inside_sqrt":
            c = np.float64(max_norm) / np.sqrt(S + 1e-6)
        else:
            c = np.float64(max_norm) / (nrm + 1e-6)
        coef = np.float32(c if (c < 1.0 or mut == "no_clamp") else 1.0)
        if bad:
            coef = np.float32("nan")
        skip = int(bad and bool(skip_nonfinite))
        if skip or sum(g.numel() for g in grads) == 0:
            coef = np.float32(1.0)
        return dict(coef=float(coef), norm=float(np.float32(nrm)), skip=skip,
                    per_tensor=[float(np.float32(np.sqrt(np.float64(s)))) for s in S_i])


def emulate_guarded(call, h, coef, skip, mut=None):
    """apg_adam_step_guarded on test_optim_fp64's emulation: g2 = coef * g (one rounding), then the sequence on g2; skip: nothing moves"""
    c = torch.tensor(coef, dtype=torch.float32)
    if skip:
        out = [{k: t[k].clone() for k in (F.OUTS if h["amsgrad"] else F.OUTS[:3])} for t in call]
        if mut == "skip_updates_m":
            for o, e in zip(out, F.emulate(call, h)):
                o["m"] = e["m"]
        return out
    if mut == "coef_after_weight_decay":
        wd = F._f32(h["wd"])
        return F.emulate([dict(t, g=c * F._fma(wd, t["p"], t["g"])) for t in call], dict(h, wd=0.0))
    return F.emulate([dict(t, g=c * t["g"]) for t in call], h)


def clipped_call(call, coef):
    """the call apg_adam_step must be given to reproduce a guarded step: g2 = float32(coef) * g, one rounded product per element"""
    c = torch.tensor(coef, dtype=torch.float32)
    return [dict(t, g=c * t["g"]) for t in call]


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
def _layout(tensors, off):
    """one NaN-filled fp32 buffer in which tensor i starts off (or off[i]) floats past a 16-byte boundary, GUARD or more NaNs around it"""
    cur, starts = 0, []
    for i, t in enumerate(tensors):
        o = off[i] if isinstance(off, (list, tuple)) else off
        cur = (cur + GUARD + 3) // 4 * 4 + o
        starts.append(cur)
        cur += t.numel()
    buf = torch.full((cur + GUARD + 4,), float("nan"), dtype=torch.float32)
    for s, t in zip(starts, tensors):
        buf[s:s + t.numel()] = t
    return buf, starts


def _table(devbuf, starts, tensors):
    n = len(tensors)
    return (ctypes.c_void_p * max(n, 1))(*[(devbuf.data_ptr() + 4 * s) if t.numel() else None for s, t in zip(starts, tensors)])


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def read_record(record):
    r = record.cpu()
    return dict(coef=float(r[0]), norm=float(r[1]), skip=int(r.view(torch.int32)[2]), reserved=int(r.view(torch.int32)[3]))


def run_norm(grads, max_norm, dev, skip_nonfinite=False, off=0, counters=None, scale=False, per_tensor=True):
    """one apg_grad_norm call (and one apg_grad_scale with scale=True) -> the record, per_tensor and, after a scale, the gradients.
    The gradients sit between NaN guard bands (a read outside a tensor would make the norm NaN), the workspace and per_tensor
    start as NaN with a band behind them, the record starts as garbage; `record` in the result is the device tensor."""
    from airpose_amd import _native_grad as G
    L = G.lib()
    n = len(grads)
    host, starts = _layout(grads, off)
    devb = host.to(dev)
    assert devb.data_ptr() % 16 == 0
    gtab = _table(devb, starts, grads)
    numel = (ctypes.c_int64 * max(n, 1))(*[g.numel() for g in grads])
    need = L.apg_grad_norm_workspace_bytes(n, numel)
    assert need >= 0 and need % 8 == 0
    ws = torch.full((need // 8 + 8,), float("nan"), dtype=torch.float64, device=dev)
    pt = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=dev)
    record = torch.full((4,), -7.0, dtype=torch.float32, device=dev)
    rc = L.apg_grad_norm(n, gtab, numel, max_norm, int(skip_nonfinite), ws.data_ptr(), need, record.data_ptr(),
                         pt.data_ptr() if per_tensor else None, None if counters is None else counters.data_ptr(), _stream(dev))
    G.check(rc, "apg_grad_norm")
    if scale:
        G.check(L.apg_grad_scale(n, gtab, numel, record.data_ptr(), _stream(dev)), "apg_grad_scale")
    torch.cuda.synchronize()
    out = read_record(record)
    assert out["reserved"] == 0
    assert torch.isnan(ws[need // 8:]).all(), "the workspace was written past its size"
    ptc = pt.cpu()
    if per_tensor:
        assert torch.isnan(ptc[n:]).all(), "per_tensor was written past its end"
        out["per_tensor"] = [float(x) for x in ptc[:n]]
    else:
        assert torch.isnan(ptc).all()
        out["per_tensor"] = None
    back = devb.cpu()
    inside = torch.zeros(back.numel(), dtype=torch.bool)
    for s, g in zip(starts, grads):
        inside[s:s + g.numel()] = True
    assert torch.isnan(back[~inside]).all(), "a guard band of the gradients was written"
    out["g"] = [back[s:s + g.numel()].clone() for s, g in zip(starts, grads)]
    if not scale:
        assert torch.equal(back.view(torch.int32), host.view(torch.int32)), "apg_grad_norm wrote a gradient"
    out["record"] = record
    return out


def same_record(a, b):
    eq = lambda x, y: x == y or (x != x and y != y)
    return eq(a["coef"], b["coef"]) and eq(a["norm"], b["norm"]) and a["skip"] == b["skip"] and \
        (a["per_tensor"] is None or all(eq(x, y) for x, y in zip(a["per_tensor"], b["per_tensor"])))


def run_guarded(call, h, dev, record):
    """one apg_adam_step_guarded call with the device record -> per tensor a dict of the new p, m, v (and vmax), cpu fp32; the layout
    and the guard bands are test_optim_fp64.run's (NaN bands; with skip set the outputs are the inputs, so no NaN check inside)"""
    from airpose_amd import _native_grad as G
    L = G.lib()
    n = len(call)
    arrays = F.NAMES if h["amsgrad"] else F.NAMES[:4]
    host, start, devb = {}, {}, {}
    for name in arrays:
        host[name], start[name] = _layout([t[name] for t in call], 0)
        devb[name] = host[name].to(dev)
    tab = {name: _table(devb[name], start[name], [t[name] for t in call]) for name in arrays}
    i64 = ctypes.c_int64 * n
    rc = L.apg_adam_step_guarded(n, tab["p"], tab["g"], tab["m"], tab["v"], tab.get("vmax"), i64(*[t["n"] for t in call]),
                                 i64(*[t["step"] for t in call]), h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], record.data_ptr(),
                                 _stream(dev))
    G.check(rc, "apg_adam_step_guarded")
    torch.cuda.synchronize()
    back = {name: devb[name].cpu() for name in arrays}
    assert torch.equal(back["g"].view(torch.int32), host["g"].view(torch.int32)), "g was written"
    out = [dict() for _ in call]
    for name in arrays:
        if name == "g":
            continue
        inside = torch.zeros(back[name].numel(), dtype=torch.bool)
        for i, (s, t) in enumerate(zip(start[name], call)):
            inside[s:s + t["n"]] = True
            out[i][name] = back[name][s:s + t["n"]].clone()
        assert torch.isnan(back[name][~inside]).all(), "%s: a guard band was written" % name
    return out


def inputs_of(call, h):
    return [{k: t[k].clone() for k in (F.OUTS if h["amsgrad"] else F.OUTS[:3])} for t in call]
