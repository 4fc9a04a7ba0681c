"""Element-wise fp64 ground truth for apg_adam_step (airpose_amd/csrc/optim.hip): the multi-tensor Adam / AMSGrad step, through the C
ABI of include/airpose_grad.h.  Companion of test_loss_fp64.py; evaluate() is test_stem_pool_fp64's.

Reference.  reference() below: torch's _single_tensor_adam (maximize = False, L2 weight decay) restated in fp64 on exactly the fp32
values the kernel receives, with the hyper-parameters as the doubles the caller passed:
    g' = g + wd p;  m' = m + (1 - b1)(g' - m);  v' = b2 v + (1 - b2) g'^2;  vmax' = max(vmax, v')  (amsgrad)
    den = sqrt(vmax' or v') / sqrt(1 - b2^step) + eps;  p' = p - (lr / (1 - b1^step)) m' / den

Bars (counted from the kernel's instruction sequence, none measured).  u = 2^-24, |got - ref| <= n u A; where A = 0 the output must
be exactly the reference.  The host rounds wd, 1 - b1, b2, 1 - b2, eps, ss = lr / (1 - b1^step) and rb = 1 / sqrt(1 - b2^step) to
float once each (one rounding apiece), and every fmaf, product, difference, square root and quotient of the sequence is one more.
  g'    = fmaf(wd, p, g)          wd's rounding and the fma's: n_g = 2 on A_g = |g| + wd |p|           (wd = 0: g' = g exactly, n_g = 0)
  m'    = fmaf(1 - b1, g' - m, m) n_g, the difference, (1 - b1)'s rounding, the fma's: n_m = n_g + 3
                                  on A_m = |m| + (1 - b1)(A_g + |m|)
  v'    = fmaf(1 - b2, g' * g', b2 * v)
                                  the g'^2 share carries 2 n_g + 1 (the product) + 1 ((1 - b2)'s rounding), the b2 v share 2 (b2's
                                  rounding, the product), then the fma's: n_v = max(2, 2 n_g + 2) + 1 = 2 n_g + 3
                                  on A_v = b2 v + (1 - b2) A_g^2
  vmax' = max(vmax, v')           exact, and |max(a, x) - max(a, y)| <= |x - y|: n_v on A_v
  p'    = fmaf(-ss, m' / den, p), den = fmaf(sqrt(vh), rb, eps), vh = vmax' or v'
                                  den: vh is off by at most n_v u A_v = n_v u r vh with r = A_v / vh (r <= 1 unless weight decay
                                  cancels g; with amsgrad vh >= v' makes it smaller still), the square root halves that and adds its
                                  own rounding, then rb's, eps's and the fma's: n_den = n_v r / 2 + 4 relative to den.
                                  The update ss m' / den: n_m (m', since |m'| <= A_m) + n_den + 1 (the quotient) + 1 (ss's rounding),
                                  and the last fma's rounding of p' itself:
                                  n_p = n_m + n_v r / 2 + 4 + 3 per element, on A_p = |p| + ss A_m / den
                                  (wd = 0 and r = 1: 11.5; wd > 0 and r = 1: 15.5)
bars(.., sequence="torch") counts torch's own unfused sequence the same way (test_optim_module.py compares against it): g' = add(g,
p, alpha = wd) 3; lerp 4 more; mul_(b2) 2 and addcmul_(g', g', value = 1 - b2) 2 n_g + 3, + 1: n_v = 2 n_g + 4; den = sqrt (1), the
division by a host scalar as a product with its float reciprocal (3), add(eps) (2): n_v r / 2 + 6; addcdiv_ 4:
n_p = n_m + n_v r / 2 + 6 + 4.

Exact zeros.  Where g = m = v = vmax = 0 and (wd = 0 or p = 0): p' is p bit for bit and m', v', vmax' are zero.

Inputs sit at the workload's scales: p = 0.05 N(0, 1); |g| log-uniform over [1e-8, 1e-1] with a random sign and a tenth exact zeros
(eps = 1e-8 is then sometimes the larger part of den); m and v from three emulated earlier steps; vmax = v / 2 or 2 v (so vmax >= v'
for some elements and vmax < v' for others); a twentieth of the elements dead (g = m = v = vmax = 0, half of them p = 0 as well).
step in {1, 2, 1000}, lr in {5e-5 (the reference trainers'), 1e-3}, wd in {0, 1e-4}, amsgrad on and off.

Shapes.  C = 4096 is the kernel's chunk, 64 tensors its batch: numel in {1, 3, 4, 5, C - 1, C, C + 1, 2 C + 3} in one call per
hyper-parameter set; calls of 1, 64 (one full batch) and 65 tensors; 401 tensors of mixed sizes, empty ones among them, with a step
count of their own each.  Every pointer offset by 1, 2 and 3 floats from a 16-byte boundary in turn: bit-equal to the aligned call.
Every call runs twice into fresh buffers whose tensors sit between NaN guard bands: bit-equal, guards untouched, g unchanged.

CPU self-check (no GPU): emulate(), an fp32 evaluation of the kernel's exact sequence (an fma is formed in fp64 -- the product of two
floats is exact there -- and rounded to float), stays inside every bar on the same cases; each of MUTATIONS is rejected.
"""
import ctypes
import itertools
import math

import pytest
import torch

from test_stem_pool_fp64 import evaluate

U32 = 2.0 ** -24
C, BATCH = 4096, 64                                      # optim.hip: ADAM_CHUNK, ADAM_BATCH
NAMES = ("p", "g", "m", "v", "vmax")
OUTS = ("p", "m", "v", "vmax")
SIZES = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)
MUTATIONS = ("no_bias_correction", "eps_inside_sqrt", "max_before_v", "no_weight_decay", "betas_swapped", "step_one_too_low")


def hyper(lr=5e-5, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, amsgrad=True):
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, amsgrad=amsgrad)


HYPERS = [(step, hyper(lr=lr, wd=wd, amsgrad=ams)) for step, lr, wd, ams in
          itertools.product((1, 2, 1000), (5e-5, 1e-3), (0.0, 1e-4), (True, False))]


_ID = lambda x: "step%d" % x if isinstance(x, int) else "lr%g-wd%g-%s" % (x["lr"], x["wd"], "ams" if x["amsgrad"] else "adam")


# ------------------------------------------------------------------------------------------------ cases
def make_tensor(n, seed, step=1):
    """one tensor's five fp32 arrays (and its step count) at the workload's scales"""
    gen = torch.Generator().manual_seed(7919 * seed + n)
    rand = lambda: torch.rand(n, generator=gen)

    def grad():
        g = 10.0 ** (rand() * 7 - 8) * torch.where(rand() < 0.5, -1.0, 1.0)
        return torch.where(rand() < 0.1, torch.zeros(n), g).float()
    p = (0.05 * torch.randn(n, generator=gen)).float()
    dead = rand() < 0.05
    m, v = torch.zeros(n), torch.zeros(n)
    for _ in range(3):
        g = grad()
        m = m + 0.1 * (g - m)
        v = 0.999 * v + 0.001 * g * g
    vmax = torch.where(rand() < 0.5, v * 0.5, v * 2.0)
    g = grad()
    z = torch.zeros(n)
    g, m, v, vmax = (torch.where(dead, z, t) for t in (g, m, v, vmax))
    p = torch.where(dead & (rand() < 0.5), z, p)
    return dict(p=p, g=g, m=m, v=v, vmax=vmax, step=step, n=n)


def make_call(sizes, steps, seed=0):
    return [make_tensor(n, seed * 1000 + i, s) for i, (n, s) in enumerate(zip(sizes, steps))]


# ------------------------------------------------------------------------------------------------ the fp64 restatement and its bars
def step_fp64(t, h, step=None):
    """one update of p, g, m, v, vmax (any float dtype, computed in fp64) -> dict of the new p, m, v, vmax and the intermediates"""
    step = t["step"] if step is None else step
    p, g, m, v, x = (t[k].double() for k in NAMES)
    b1, b2 = h["b1"], h["b2"]
    g1 = g + h["wd"] * p
    m1 = m + (1.0 - b1) * (g1 - m)
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    x1 = torch.maximum(x, v1) if h["amsgrad"] else x
    vh = x1 if h["amsgrad"] else v1
    ss = h["lr"] / (1.0 - b1 ** step)
    den = vh.sqrt() / math.sqrt(1.0 - b2 ** step) + h["eps"]
    return dict(p=p - ss * m1 / den, m=m1, v=v1, vmax=x1, vh=vh, den=den, ss=ss)


def bars(t, h, ref, sequence="kernel"):
    """n u A per output, as counted in the docstring.  p_own: the roundings of p' that are not inherited from m' and v' (den's four and
    the last three; torch: 6 + 4), for a caller that carries the errors of m' and v' through the step itself"""
    tq = sequence == "torch"
    p, g, m, v = (t[k].double().abs() for k in ("p", "g", "m", "v"))
    b1, b2, wd = h["b1"], h["b2"], h["wd"]
    n_g = 0 if wd == 0 else (3 if tq else 2)
    n_m = n_g + (4 if tq else 3)
    n_v = 2 * n_g + (4 if tq else 3)
    A_g = g + wd * p
    A_m = m + (1.0 - b1) * (A_g + m)
    A_v = b2 * v + (1.0 - b2) * A_g * A_g
    vh = ref["vh"]
    r = torch.where(vh > 0, A_v / torch.where(vh > 0, vh, torch.ones_like(vh)), torch.ones_like(vh))
    n_p = n_m + n_v * r / 2 + ((6 + 4) if tq else (4 + 3))
    A_p = p + ref["ss"] * A_m / ref["den"]
    out = dict(p=n_p * U32 * A_p, m=n_m * U32 * A_m, v=n_v * U32 * A_v, p_own=((6 + 4) if tq else (4 + 3)) * U32 * A_p)
    if h["amsgrad"]:
        out["vmax"] = n_v * U32 * A_v
    return out


def reference(t, h):
    ref = step_fp64(t, h)
    ref["bars"] = bars(t, h, ref)
    return ref


def dead_mask(t, h):
    z = (t["g"] == 0) & (t["m"] == 0) & (t["v"] == 0)
    if h["amsgrad"]:
        z &= t["vmax"] == 0
    return z & (t["p"] == 0) if h["wd"] != 0 else z


def verify(call, h, got, what, ratios=None):
    """got: per tensor a dict of the new p, m, v (and vmax) as fp32 -> list of failures against the bars and the exact-zero rule"""
    fails = []
    ratios = {} if ratios is None else ratios
    for i, (t, o) in enumerate(zip(call, got)):
        if t["n"] == 0:
            continue
        ref = reference(t, h)
        for name in OUTS:
            if name == "vmax" and not h["amsgrad"]:
                continue
            ok, ratio, nz, msg = evaluate(o[name], ref[name], ref["bars"][name])
            ratios[name] = max(ratios.get(name, 0.0), ratio)
            if not ok:
                fails.append((what, "tensor %d (numel %d, step %d)" % (i, t["n"], t["step"]), name, msg))
        z = dead_mask(t, h)
        if z.any():
            if not torch.equal(o["p"].view(torch.int32)[z], t["p"].view(torch.int32)[z]):
                fails.append((what, "tensor %d" % i, "p", "a dead element's p changed"))
            for name in OUTS[1:]:
                if (name != "vmax" or h["amsgrad"]) and o[name][z].view(torch.int32).any():
                    fails.append((what, "tensor %d" % i, name, "a dead element's %s is not +0" % name))
    return fails


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernel's sequence
def _fma(a, b, c):
    """fmaf on fp32 tensors (or Python floats already rounded to fp32): the product is exact in fp64, the sum is rounded there and to fp32"""
    d = lambda x: x.double() if torch.is_tensor(x) else x
    return (d(a) * d(b) + d(c)).float()


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).float())


def emulate(call, h, mut=None):
    out = []
    b1, b2 = (h["b2"], h["b1"]) if mut == "betas_swapped" else (h["b1"], h["b2"])
    wd = _f32(0.0 if mut == "no_weight_decay" else h["wd"])
    omb1, fb2, omb2, eps = _f32(1.0 - b1), _f32(b2), _f32(1.0 - b2), _f32(h["eps"])
    for t in call:
        step = t["step"] - 1 if mut == "step_one_too_low" else t["step"]
        if mut == "no_bias_correction":
            ss, rb = _f32(h["lr"]), 1.0
        else:
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            ss = _f32(h["lr"] / bc1) if bc1 else float("inf")
            rb = _f32(1.0 / math.sqrt(bc2)) if bc2 else float("inf")
        p, g, m, v, x = (t[k] for k in NAMES)
        g1 = _fma(wd, p, g)
        d = g1 - m
        m1 = _fma(omb1, d, m)
        tt = g1 * g1
        w = fb2 * v
        if mut == "max_before_v":
            x = torch.maximum(x, v)
        v1 = _fma(omb2, tt, w)
        vh = v1
        if h["amsgrad"]:
            if mut != "max_before_v":
                x = torch.maximum(x, v1)
            vh = x
        if mut == "eps_inside_sqrt":
            den = (_fma(vh, rb * rb, eps)).sqrt()
        else:
            den = _fma(vh.sqrt(), rb, eps)
        q = m1 / den
        o = dict(p=_fma(-ss, q, p), m=m1, v=v1)
        if h["amsgrad"]:
            o["vmax"] = x
        assert all(a.dtype == torch.float32 for a in o.values())
        out.append(o)
    return out


@pytest.mark.parametrize("step,h", HYPERS, ids=_ID)
def test_cpu_fp32_emulation_is_inside_every_bar(step, h):
    call = make_call(SIZES, [step] * len(SIZES))
    ratios = {}
    fails = verify(call, h, emulate(call, h), "emulation", ratios)
    print("step %d %s: worst err / bound %s" % (step, h, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fails, fails
    assert any(bool(dead_mask(t, h).any()) for t in call)                     # the exact-zero rule met elements
    for t in call[-2:]:                                                       # the inputs cover what the docstring promises
        v1 = step_fp64(t, h)["v"]
        assert (t["vmax"].double() >= v1).any() and (t["vmax"].double() < v1).any()
        if step == 1000:                                                      # (the steps whose bias correction leaves v's scale alone)
            small = step_fp64(t, h)["den"] < 2 * h["eps"]
            assert small.any() and (~small).any()                             # eps is the larger part of den for some elements


def _mutation_call():
    return make_call((5, C + 1, 259, 2 * C + 3), (2, 1000, 1, 2), seed=3)


@pytest.mark.parametrize("mut", MUTATIONS)
def test_cpu_mutations_are_rejected(mut):
    call, h = _mutation_call(), hyper(lr=5e-5, wd=1e-4, amsgrad=True)
    assert not verify(call, h, emulate(call, h), "unmutated")
    fails = verify(call, h, emulate(call, h, mut=mut), mut)
    assert fails, "the bars accept the mutation %s" % mut
    names = {f[2] for f in fails}
    want = dict(no_bias_correction="p", eps_inside_sqrt="p", max_before_v="vmax", no_weight_decay="m", betas_swapped="m",
                step_one_too_low="p")[mut]
    assert want in names, (mut, sorted(names))


def test_cpu_binding_has_the_entry():
    from airpose_amd import _native_grad as G
    assert "apg_adam_step" in G.SIGNATURES
    assert G.lib().apg_adam_step.restype is ctypes.c_int


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
GUARD = 64


def run(call, h, dev, offs=None):
    """one apg_adam_step call -> per tensor a dict of the new p, m, v (and vmax), cpu fp32.  Each of the five arrays is one NaN-filled
    device buffer in which tensor i's data starts offs[i][k] floats past a 16-byte boundary, GUARD or more NaNs on either side."""
    from airpose_amd import _native_grad as G
    L = G.lib()
    n = len(call)
    arrays = NAMES if h["amsgrad"] else NAMES[:4]
    offs = [(0,) * 5] * n if offs is None else offs
    host, start = {}, {}
    for k, name in enumerate(arrays):
        cur, st = 0, []
        for i, t in enumerate(call):
            cur = (cur + GUARD + 3) // 4 * 4 + offs[i][k]
            st.append(cur)
            cur += t["n"]
        buf = torch.full((cur + GUARD + 4,), float("nan"), dtype=torch.float32)
        for s, t in zip(st, call):
            buf[s:s + t["n"]] = t[name]
        host[name], start[name] = buf, st
    devb = {name: host[name].to(dev) for name in arrays}
    for name in arrays:
        assert devb[name].data_ptr() % 16 == 0
    vp, i64 = ctypes.c_void_p * n, ctypes.c_int64 * n
    # a tensor without elements gets a NULL pointer: the entry point must not look at it
    tab = {name: vp(*[(devb[name].data_ptr() + 4 * s) if t["n"] else None for s, t in zip(start[name], call)]) for name in arrays}
    rc = L.apg_adam_step(n, tab["p"], tab["g"], tab["m"], tab["v"], tab.get("vmax"), i64(*[t["n"] for t in call]),
                         i64(*[t["step"] for t in call]), h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    G.check(rc, "apg_adam_step")
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
        assert not torch.isnan(back[name][inside]).any(), "%s: NaN among the outputs" % name
    return out


def bit_equal(a, b):
    return all(x.keys() == y.keys() and all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in x) for x, y in zip(a, b))


def run_twice_and_verify(call, h, dev, what, **kw):
    got = run(call, h, dev, **kw)
    again = run(call, h, dev, **kw)
    assert bit_equal(got, again), (what, "two runs differ")
    ratios = {}
    fails = verify(call, h, got, what, ratios)
    print("%-50s worst err / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fails, fails[:5]
    return got


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("step,h", HYPERS, ids=_ID)
def test_every_size_against_fp64(dev, step, h):
    call = make_call(SIZES, [step] * len(SIZES))
    run_twice_and_verify(call, h, dev, "step %d lr %g wd %g amsgrad %d" % (step, h["lr"], h["wd"], h["amsgrad"]))


MIXED = (1, 3, 0, 4, 5, 64, 0, 257, 1023, C - 1, C, C + 1, 2048, 2 * C + 3, 37)


def _mixed_call(n, seed):
    sizes = [MIXED[i % len(MIXED)] for i in range(n)]
    steps = [(1, 2, 1000, 7)[(i // 3) % 4] for i in range(n)]
    return make_call(sizes, steps, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("ntensors", [1, BATCH, BATCH + 1, 401])
def test_tensor_counts_around_a_batch_against_fp64(dev, ntensors, amsgrad):
    """1 tensor; exactly one batch and one more (of tensors WITH elements: empty ones take no slot); 401 tensors of mixed sizes with empty
    ones among them and a step count per tensor -- a bias correction shared between tensors would miss the bars of most of them"""
    if ntensors == 1:
        call = make_call((2 * C + 3,), (2,), seed=5)
    elif ntensors == 401:
        call = _mixed_call(401, seed=6)
        assert sum(t["n"] == 0 for t in call) > 40 and len({t["step"] for t in call}) == 4
    else:
        live = [s for s in MIXED if s]
        call = make_call([live[i % len(live)] for i in range(ntensors)], [(1, 2, 1000)[i % 3] for i in range(ntensors)], seed=7)
    h = hyper(lr=5e-5, wd=1e-4, amsgrad=amsgrad)
    run_twice_and_verify(call, h, dev, "%d tensors amsgrad %d" % (ntensors, amsgrad))


def test_a_shared_bias_correction_would_be_caught():
    """the CPU side of the claim above: the 401-tensor call evaluated with tensor 0's step count for everyone misses the bars"""
    call, h = _mixed_call(401, seed=6), hyper(lr=5e-5, wd=1e-4)
    shared = [dict(t, step=call[0]["step"]) for t in call]
    assert verify(call, h, emulate(shared, h), "shared step")


@pytest.mark.gpu
@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_pointers_off_a_16_byte_boundary(dev, off, amsgrad):
    """each of the five pointers offset in turn (of one tensor, the others staying aligned), then all of them, then a mixture: the same
    bits as the aligned call"""
    call = make_call((5, C + 1, 2 * C + 3), (2, 1, 1000), seed=9)
    h = hyper(lr=1e-3, wd=1e-4, amsgrad=amsgrad)
    base = run_twice_and_verify(call, h, dev, "aligned")
    narr = 5 if amsgrad else 4
    one = lambda k: tuple(off if j == k else 0 for j in range(5))
    layouts = [[one(k)] * 3 for k in range(narr)]                             # array k of every tensor
    layouts += [[(0,) * 5, one(k), (0,) * 5] for k in range(narr)]            # array k of the middle tensor alone
    layouts += [[(off,) * 5] * 3, [(1, 2, 3, off, 0), (off, 0, 1, 2, 3), (0,) * 5]]
    for offs in layouts:
        got = run_twice_and_verify(call, h, dev, "offsets %s" % (offs,), offs=offs)
        assert bit_equal(got, base), offs
