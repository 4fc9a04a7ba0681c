"""airpose_amd.FusedAdam (airpose_amd/optim.py on apg_adam_step) as a torch.optim.Optimizer: trajectories against torch.optim.Adam and
against fp64, state_dict round trips in both directions, parameters without a gradient, param groups, the refusals, and the
train_reg_only fine-tune of copenet_sep with FusedAdam next to torch.optim.Adam.

Bars.  One step's bars are test_optim_fp64's (counted from the kernel's roundings; bars(.., sequence="torch") counts torch's unfused
sequence the same way).  Over several steps two runs drift apart, and Drift below carries an element-wise bound on that drift through
the exact update, with R_* the step's own roundings (of both runs where both are fp32) and E_g a difference of the gradients the runs
were given (0 when they are fed the same ones):
    E_g' = E_g + wd E_p
    E_m  <- b1 E_m + (1 - b1) E_g' + R_m                                   m' = b1 m + (1 - b1) g'
    E_v  <- b2 E_v + (1 - b2)(2 |g'| + E_g') E_g' + R_v                     |a^2 - b^2| = |a - b| |a + b|
    E_x  <- max(E_x, E_v)                                                  |max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|)
    E_s  =  min(E_vh / sqrt(vh), sqrt(E_vh)),  E_den = E_s / sqrt(1 - b2^t) |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= sqrt(|a - b|)
    E_q  =  E_m / den_lo + |m'| E_den / (den den_lo),  den_lo = max(den - E_den, eps)
    E_p  <- E_p + ss E_q + R_p_own                                         R_p_own: the roundings of p' not inherited from m', v'
evaluated at the reference run's state (the R_* at another state differ in second order).  Where a bound is 0 the runs must agree
exactly.

End to end.  Both trainings start from the same parameters and draw the same dropout seeds, so step 0's losses and gradients are
bit-equal.  From then on the parameters differ by at most E_p, and the gradients the two optimizers are given differ (the model's
answer to that difference): the measured |g_fused - g_torch| enters the recursion as E_g, so E_p stays a bound on what the two
OPTIMIZERS may legitimately make of their inputs, and a wrong update is caught at the first step it occurs, while E_g is still 0.
Loss bar at step t: sum_i |g_i| E_p,i (first order in the parameter difference; g = the reference run's gradient at that step, i.e.
the loss's exact derivative) + 2 N, N = the forward pass's own rounding noise, measured on the untrained reference model as the
largest change of the loss under four random +-1 ulp perturbations of the head parameters (a worst-case dot-product bound over the
2332 / 1024 / 1024-long reductions of three iterations is vacuous).
"""
import copy
import math

import pytest
import torch

import test_optim_fp64 as F
from conftest import MEAN_PARAMS
from test_stem_pool_fp64 import evaluate

pytestmark = pytest.mark.gpu
C = F.C
SIZES = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 64, 257, 2048, 37)
STEPS = 20
H = F.hyper(lr=5e-5, wd=0.0, amsgrad=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ drift bounds
class Drift(object):
    """element-wise bound on the difference of two runs of one tensor (see the module docstring); tensors of any one device"""

    def __init__(self, like):
        z = lambda: torch.zeros_like(like, dtype=torch.float64)
        self.p, self.m, self.v, self.x = z(), z(), z(), z()

    def step(self, state, g, h, step, seqs, E_g=None):
        """state: the reference run's p, m, v, vmax BEFORE the step; g: its gradient -> the exact fp64 step from that state"""
        t = dict(p=state["p"], g=g, m=state["m"], v=state["v"], vmax=state["vmax"], step=step)
        ref = F.step_fp64(t, h)
        R = None
        for s in seqs:
            b = F.bars(t, h, ref, sequence=s)
            R = b if R is None else {k: R[k] + b[k] for k in b}
        b1, b2, wd = h["b1"], h["b2"], h["wd"]
        E_g1 = (0.0 if E_g is None else E_g.double()) + wd * self.p
        g1 = (g.double() + wd * state["p"].double()).abs()
        self.m = b1 * self.m + (1.0 - b1) * E_g1 + R["m"]
        self.v = b2 * self.v + (1.0 - b2) * (2.0 * g1 + E_g1) * E_g1 + R["v"]
        if h["amsgrad"]:
            self.x = torch.maximum(self.x, self.v)
        E_vh = self.x if h["amsgrad"] else self.v
        vh = ref["vh"]
        lin = torch.where(vh > 0, E_vh / torch.where(vh > 0, vh, torch.ones_like(vh)).sqrt(), torch.full_like(vh, float("inf")))
        E_den = torch.minimum(lin, E_vh.sqrt()) / math.sqrt(1.0 - b2 ** step)
        den = ref["den"]
        den_lo = torch.clamp(den - E_den, min=h["eps"] * (1.0 - 2.0 ** -20))          # (eps itself is rounded to float once)
        E_q = self.m / den_lo + ref["m"].abs() * E_den / (den * den_lo)
        self.p = self.p + ref["ss"] * E_q + R["p_own"]
        return ref


def check(what, name, got, want, bound, ratios=None):
    ok, ratio, nz, msg = evaluate(got, want.double(), bound)
    if ratios is not None:
        ratios[name] = max(ratios.get(name, 0.0), ratio)
    assert ok, (what, name, msg)


# ------------------------------------------------------------------------------------------------ a small parameter set and its gradients
def start_values(seed=0):
    return [F.make_tensor(n, 100 * seed + i)["p"] for i, n in enumerate(SIZES)]


def gradient(i, n, step, seed=0):
    return F.make_tensor(n, 5000 + 100 * seed + 37 * step + i)["g"]


def params_on(dev, values):
    return [torch.nn.Parameter(v.clone().to(dev)) for v in values]


def feed(params, step, skip=(), seed=0):
    """.grad of every parameter for `step` (0-based); (index, step) in skip -> None"""
    for i, p in enumerate(params):
        p.grad = None if (i, step) in skip else gradient(i, p.numel(), step, seed).to(p.device)


def run_steps(opt, params, steps, skip=(), seed=0):
    for s in steps:
        feed(params, s, skip, seed)
        opt.step()
    torch.cuda.synchronize()


def snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append({k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()})
        out[-1]["p"] = p.detach().cpu().clone()
    return out


def bits_equal(a, b):
    for x, y in zip(a, b):
        assert x.keys() == y.keys(), (sorted(x), sorted(y))
        for k in x:
            if k == "step":
                assert float(x[k]) == float(y[k])
            else:
                assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), k
    return True


def fp64_trajectory(values, hs, nsteps, seqs, skip=(), seed=0):
    """fp64 Adam on CPU from the fp32 start values with the same gradients -> per step the states AFTER it and the drift bounds of a
    run (or two) of `seqs` around it: list over steps of list over tensors of (state, Drift snapshot)"""
    st = [dict(p=v.double(), m=torch.zeros_like(v, dtype=torch.float64), v=torch.zeros_like(v, dtype=torch.float64),
               vmax=torch.zeros_like(v, dtype=torch.float64), step=0) for v in values]
    dr = [Drift(v) for v in values]
    out = []
    for s in range(nsteps):
        for i, (t, d) in enumerate(zip(st, dr)):
            if (i, s) in skip:
                continue
            t["step"] += 1
            ref = d.step(t, gradient(i, values[i].numel(), s, seed).double(), hs[i], t["step"], seqs)
            t.update(p=ref["p"], m=ref["m"], v=ref["v"], vmax=ref["vmax"])
        out.append([(dict(t), dict(p=d.p.clone(), m=d.m.clone(), v=d.v.clone(), vmax=d.x.clone())) for t, d in zip(st, dr)])
    return out


def compare_to_trajectory(what, snap, traj_step, amsgrad=True, ratios=None):
    for i, (got, (want, E)) in enumerate(zip(snap, traj_step)):
        if want["step"] == 0:
            assert "step" not in got, (what, i, "a parameter that never had a gradient has state")
            assert torch.equal(got["p"].double(), want["p"]), (what, i)
            continue
        assert float(got["step"]) == want["step"], (what, i, float(got["step"]), want["step"])
        assert got["step"].device.type == "cpu" and got["step"].dtype == torch.float32
        for k, name in (("p", "p"), ("m", "exp_avg"), ("v", "exp_avg_sq")) + ((("vmax", "max_exp_avg_sq"),) if amsgrad else ()):
            check(what, "%s[%d]" % (name, i), got[name], want[k], E[k], ratios)
        assert amsgrad or "max_exp_avg_sq" not in got


def make_opts(dev, values, groups=None, **kw):
    """FusedAdam and torch.optim.Adam(foreach=False) over clones of the same values; groups: list of (indices, options)"""
    from airpose_amd import FusedAdam
    pf, pt = params_on(dev, values), params_on(dev, values)
    arg = lambda ps: ps if groups is None else [dict(params=[ps[i] for i in idx], **o) for idx, o in groups]
    return FusedAdam(arg(pf), **kw), pf, torch.optim.Adam(arg(pt), foreach=False, **kw), pt


KW = dict(lr=H["lr"], betas=(H["b1"], H["b2"]), eps=H["eps"], weight_decay=H["wd"], amsgrad=True)


# ------------------------------------------------------------------------------------------------ 1. trajectories
@pytest.mark.parametrize("amsgrad", [True, False])
def test_twenty_steps_against_torch_and_fp64(dev, amsgrad):
    values = start_values()
    h = dict(H, amsgrad=amsgrad)
    kw = dict(KW, amsgrad=amsgrad)
    fused, pf, ref, pt = make_opts(dev, values, **kw)
    hs = [h] * len(values)
    own = fp64_trajectory(values, hs, STEPS, ("kernel",))
    both = fp64_trajectory(values, hs, STEPS, ("kernel", "torch"))
    r64, rt = {}, {}
    for s in range(STEPS):
        run_steps(fused, pf, [s])
        run_steps(ref, pt, [s])
        sf, st = snapshot(fused, pf), snapshot(ref, pt)
        compare_to_trajectory("fused against fp64, step %d" % s, sf, own[s], amsgrad, r64)
        for i, (a, b) in enumerate(zip(sf, st)):                              # against torch: both drift from the fp64 run
            E = both[s][i][1]
            assert float(a["step"]) == float(b["step"]) == s + 1
            for k, name in (("p", "p"), ("m", "exp_avg"), ("v", "exp_avg_sq")) + ((("vmax", "max_exp_avg_sq"),) if amsgrad else ()):
                check("fused against torch, step %d" % s, "%s[%d]" % (name, i), a[name], b[name], E[k], rt)
    print("worst err / bound against fp64:", "  ".join("%s %.3f" % kv for kv in sorted(r64.items())[:4]), "...")
    print("worst ratio against fp64 %.3f, against torch %.3f" % (max(r64.values()), max(rt.values())))


def test_step_runs_on_the_current_stream_and_returns_the_closure_loss(dev):
    from airpose_amd import FusedAdam
    values = start_values(1)
    pa, pb = params_on(dev, values), params_on(dev, values)
    a, b = FusedAdam(pa, **KW), FusedAdam(pb, **KW)
    side = torch.cuda.Stream(dev)
    for s in range(3):
        feed(pa, s)
        feed(pb, s)
        assert a.step() is None
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            seen = []

            def closure():
                seen.append(torch.is_grad_enabled())
                return torch.tensor(3.5)
            assert float(b.step(closure)) == 3.5 and seen == [True]
        torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    assert bits_equal(snapshot(a, pa), snapshot(b, pb))


# ------------------------------------------------------------------------------------------------ 2. checkpoints
def _through(sd):
    """a state_dict as a checkpoint file would return it"""
    import io
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=False)


def test_state_dict_round_trips_in_both_directions(dev):
    from airpose_amd import FusedAdam
    values = start_values(2)
    half, total = 6, 12
    mk = {"fused": lambda ps: FusedAdam(ps, **KW), "torch": lambda ps: torch.optim.Adam(ps, foreach=False, **KW)}
    for first, other in (("fused", "torch"), ("torch", "fused")):
        # the uninterrupted run
        pu = params_on(dev, values)
        ou = mk[first](pu)
        run_steps(ou, pu, range(total))
        # the same class stopped in the middle, its state carried through the OTHER class and a file, and continued
        p1 = params_on(dev, values)
        o1 = mk[first](p1)
        run_steps(o1, p1, range(half))
        p2 = params_on(dev, [p.detach().cpu() for p in p1])
        o2 = mk[other](p2)
        o2.load_state_dict(_through(o1.state_dict()))
        assert bits_equal(snapshot(o1, p1), snapshot(o2, p2))
        assert o2.state_dict()["param_groups"][0].keys() == o1.state_dict()["param_groups"][0].keys()
        p3 = params_on(dev, [p.detach().cpu() for p in p2])
        o3 = mk[first](p3)
        o3.load_state_dict(_through(o2.state_dict()))
        run_steps(o3, p3, range(half, total))
        assert bits_equal(snapshot(ou, pu), snapshot(o3, p3)), "%s -> %s -> %s" % (first, other, first)
        # training continues in the other class too: its steps from the loaded state stay inside the drift bounds around the run above
        run_steps(o2, p2, range(half, total))
        traj = fp64_trajectory(values, [H] * len(values), total, ("kernel", "torch"))
        got, want = snapshot(o2, p2), snapshot(ou, pu)
        for i, (a, b) in enumerate(zip(got, want)):
            assert float(a["step"]) == float(b["step"]) == total and a["step"].device.type == "cpu"
            E = traj[-1][i][1]
            for k, name in (("p", "p"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")):
                check("%s continued by %s" % (first, other), "%s[%d]" % (name, i), a[name], b[name], E[k])


def test_a_fused_or_capturable_checkpoint_is_brought_to_the_host_and_unsupported_options_are_refused(dev):
    from airpose_amd import FusedAdam
    values = start_values(3)[:4]
    pt = params_on(dev, values)
    ot = torch.optim.Adam(pt, foreach=False, **KW)
    run_steps(ot, pt, range(2))
    sd = copy.deepcopy(ot.state_dict())
    for st in sd["state"].values():
        st["step"] = st["step"].to(dev)                                       # where torch's capturable / fused modes keep it
    sd["param_groups"][0]["foreach"] = True
    pf = params_on(dev, [p.detach().cpu() for p in pt])
    of = FusedAdam(pf, **KW)
    of.load_state_dict(sd)
    assert all(s["step"].device.type == "cpu" and float(s["step"]) == 2 for s in of.state.values())
    assert of.param_groups[0]["foreach"] is True                              # kept for the way back to torch, and ignored
    feed(pf, 2)
    feed(pt, 2)
    of.step()
    ot.step()
    torch.cuda.synchronize()
    assert all(s["step"].device.type == "cpu" and float(s["step"]) == 3 for s in of.state.values())
    for bad in ("maximize", "capturable", "differentiable", "decoupled_weight_decay"):
        sd2 = copy.deepcopy(ot.state_dict())
        sd2["param_groups"][0][bad] = True
        with pytest.raises(ValueError, match=bad):
            FusedAdam(params_on(dev, values), **KW).load_state_dict(sd2)


# ------------------------------------------------------------------------------------------------ 3. parameters without a gradient
def test_a_parameter_without_a_gradient_lags_exactly_as_in_torch(dev):
    values = start_values(4)
    skip = {(2, 3), (2, 4), (2, 9), (7, 0), (7, 1), (5, 6)} | {(11, s) for s in range(STEPS)}
    fused, pf, ref, pt = make_opts(dev, values, **KW)
    traj = fp64_trajectory(values, [H] * len(values), STEPS, ("kernel",), skip=skip)
    for s in range(STEPS):
        before = snapshot(fused, pf)
        run_steps(fused, pf, [s], skip=skip)
        run_steps(ref, pt, [s], skip=skip)
        sf, st = snapshot(fused, pf), snapshot(ref, pt)
        for i in range(len(values)):
            assert sf[i].keys() == st[i].keys(), (s, i)
            assert float(sf[i].get("step", 0)) == float(st[i].get("step", 0)), (s, i)
            if (i, s) in skip:
                assert bits_equal([before[i]], [sf[i]]), (s, i)
        compare_to_trajectory("with skipped steps, step %d" % s, sf, traj[s])
    assert float(sf[2]["step"]) == STEPS - 3 and float(sf[7]["step"]) == STEPS - 2 and "step" not in sf[11]


# ------------------------------------------------------------------------------------------------ 4. param groups
def test_two_param_groups_with_their_own_lr_and_weight_decay(dev):
    values = start_values(5)
    n = len(values)
    g0, g1 = dict(lr=5e-5, weight_decay=0.0), dict(lr=1e-3, weight_decay=1e-4)
    groups = [(list(range(0, n, 2)), g0), (list(range(1, n, 2)), g1)]
    fused, pf, ref, pt = make_opts(dev, values, groups=groups, betas=(H["b1"], H["b2"]), eps=H["eps"], amsgrad=True)
    hs = [dict(H, lr=(g0, g1)[i % 2]["lr"], wd=(g0, g1)[i % 2]["weight_decay"]) for i in range(n)]
    own = fp64_trajectory(values, hs, 8, ("kernel",))
    both = fp64_trajectory(values, hs, 8, ("kernel", "torch"))
    run_steps(fused, pf, range(8))
    run_steps(ref, pt, range(8))
    # (make_opts lists the parameters group by group: snapshot them in their original order)
    sf, st = snapshot(fused, pf), snapshot(ref, pt)
    compare_to_trajectory("two groups against fp64", sf, own[-1])
    for i, (a, b) in enumerate(zip(sf, st)):
        for k, name in (("p", "p"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")):
            check("two groups against torch", "%s[%d]" % (name, i), a[name], b[name], both[-1][i][1][k])
    # a scheduler's write to param_groups is honoured at the next step
    fused.param_groups[0]["lr"] = 0.0
    before = snapshot(fused, pf)
    run_steps(fused, pf, [8])
    after = snapshot(fused, pf)
    for i in range(n):
        same = torch.equal(before[i]["p"], after[i]["p"])
        assert same == (i % 2 == 0), i


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(dev):
    from airpose_amd import FusedAdam
    ok = torch.nn.Parameter(torch.randn(8, 6, device=dev))
    with pytest.raises(ValueError, match="cpu"):
        FusedAdam([torch.nn.Parameter(torch.randn(4))])
    with pytest.raises(TypeError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.randn(4, device=dev, dtype=torch.float16))])
    with pytest.raises(TypeError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.randn(4, device=dev, dtype=torch.float64))])
    with pytest.raises(ValueError, match="not contiguous"):
        FusedAdam([torch.nn.Parameter(torch.randn(8, 6, device=dev).t())])
    with pytest.raises(ValueError, match="cpu"):
        FusedAdam([ok]).add_param_group(dict(params=[torch.nn.Parameter(torch.randn(4))]))
    for opt in ("maximize", "capturable", "differentiable", "foreach", "fused"):
        with pytest.raises(TypeError, match=opt):
            FusedAdam([ok], **{opt: True})
    for kw, word in ((dict(lr=-1.0), "learning rate"), (dict(eps=-1.0), "epsilon"), (dict(betas=(1.0, 0.999)), "index 0"),
                     (dict(betas=(0.9, -0.1)), "index 1"), (dict(weight_decay=-1e-4), "weight_decay")):
        with pytest.raises(ValueError, match=word):
            FusedAdam([ok], **kw)
    with pytest.raises(TypeError, match="tensor"):
        FusedAdam([ok], lr=torch.tensor(1e-3))

    # at step: a refused gradient leaves every parameter, every state and every step count of the group as it was
    a, b = torch.nn.Parameter(torch.randn(8, 6, device=dev)), torch.nn.Parameter(torch.randn(5, device=dev))
    opt = FusedAdam([a, b], amsgrad=True)
    a.grad, b.grad = torch.randn(8, 6, device=dev), torch.randn(5, device=dev)
    opt.step()
    keep = snapshot(opt, [a, b])
    for bad, exc, word in ((torch.randn(6, 8, device=dev).t(), ValueError, "not contiguous"),
                           (torch.randn(8, 6, device=dev).to_sparse(), ValueError, "sparse"),
                           (torch.randn(8, 6, device=dev, dtype=torch.float64), TypeError, "float64"),
                           (torch.randn(8, 6), TypeError, "cpu")):
        b.grad = torch.randn(5, device=dev)
        a.grad = None
        try:
            a.grad = bad
        except (RuntimeError, TypeError):                                     # torch itself refuses to attach such a gradient
            continue
        with pytest.raises(exc, match=word):
            opt.step()
        torch.cuda.synchronize()
        assert bits_equal(keep, snapshot(opt, [a, b])), word
    opt.param_groups[0]["maximize"] = True
    a.grad = torch.randn(8, 6, device=dev)
    with pytest.raises(ValueError, match="maximize"):
        opt.step()


# ------------------------------------------------------------------------------------------------ 6. end to end: train_reg_only fine-tune
HEAD2 = ("fc1", "fc2", "decpose", "decshape")


def _sep(sds, dev, on=True):
    from airpose_amd import copenet_sep_model
    sep = copenet_sep_model.getcopenet_sep(MEAN_PARAMS, precision="fp32")
    sep.copenet0.load_state_dict(sds["copenet"])
    sep.copenet1.load_state_dict(sds["copenet_b"])
    sep = sep.to(dev).eval()
    return sep.set_trainable(True) if on else sep


def _two_view_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"xf0": torch.relu(torch.randn(B, 2048, generator=g)), "xf1": torch.relu(torch.randn(B, 2048, generator=g))}
    for v in "01":
        d["bb" + v] = torch.rand(B, 3, generator=g) + 0.2
        d["pos" + v] = torch.randn(B, 3, generator=g) * 0.3 + torch.tensor([0., 0., 10.])
    return d


def test_sep_train_reg_only_fine_tune_next_to_torch_adam(dev):
    from airpose_amd import FusedAdam
    from airpose_amd import weights as W
    sds = {"copenet": W.to_torch(W.copenet_state_dict(20240901, MEAN_PARAMS, variant="copenet")),
           "copenet_b": W.to_torch(W.copenet_state_dict(777, MEAN_PARAMS, variant="copenet"))}
    B, lr, steps = 8, 1e-6, 20                                                # (test_head_local_grad.py explains the learning rate)
    h = F.hyper(lr=lr, wd=0.0, amsgrad=True)
    d = {k: t.to(dev) for k, t in _two_view_inputs(B, 400).items()}
    args = [d[k] for k in ("xf0", "xf1", "bb0", "bb1", "pos0", "pos1")]       # trunks frozen: the features are the inputs
    tgt_net = _sep(sds, dev, on=False)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for c in (tgt_net.copenet0, tgt_net.copenet1):
            c.decpose.bias.add_(0.05 * torch.randn(135, generator=g).to(dev))
            c.decshape.bias.add_(0.05 * torch.randn(10, generator=g).to(dev))
        target = tgt_net.forward_ief(*args, iters=3)

    def loss_of(sep, seed):
        torch.manual_seed(seed)                                               # the dropout seeds of this forward: the same for both runs
        out = sep.forward_ief(*args, iters=3)
        return sum(((o - t) ** 2).mean() for o, t in zip(out, target))

    runs = {}
    for name in ("torch", "fused"):
        sep = _sep(sds, dev).train()                                          # dropout on, with the seeds of loss_of
        head = [p for c in (sep.copenet0, sep.copenet1) for m in HEAD2 for p in getattr(c, m).parameters()]
        ids = {id(p) for p in head}
        frozen = {k: p.detach().clone() for k, p in sep.named_parameters() if id(p) not in ids}
        opt = FusedAdam(head, lr=lr, weight_decay=0, amsgrad=True) if name == "fused" else \
            torch.optim.Adam(head, lr=lr, weight_decay=0, amsgrad=True)
        runs[name] = dict(sep=sep, head=head, opt=opt, frozen=frozen, losses=[])
    T, Fu = runs["torch"], runs["fused"]

    # N: the forward's own rounding noise, on the reference model before any step
    base = float(loss_of(T["sep"], 1000).detach().double())
    keep = [p.detach().clone() for p in T["head"]]
    noise = 0.0
    gen = torch.Generator(device=dev).manual_seed(5)
    for _ in range(4):
        with torch.no_grad():
            for p, k in zip(T["head"], keep):                                 # +-1 in the float's integer image: one ulp of magnitude
                one = torch.where(torch.rand(k.shape, generator=gen, device=dev) < 0.5, 1, -1).to(torch.int32)
                p.copy_(torch.where(k == 0, k, (k.view(torch.int32) + one).view(torch.float32)))
        noise = max(noise, abs(float(loss_of(T["sep"], 1000).detach().double()) - base))
    with torch.no_grad():
        for p, k in zip(T["head"], keep):
            p.copy_(k)
    drift = [Drift(p) for p in T["head"]]
    zero = lambda p: torch.zeros_like(p, dtype=torch.float64)
    worst_p = worst_l = 0.0
    for s in range(steps):
        for r in (T, Fu):
            r["opt"].zero_grad()
            loss = loss_of(r["sep"], 1000)                                    # one set of masks: a fixed objective, as in the original
            loss.backward()
            r["losses"].append(float(loss.detach().double()))
        first = sum(float((pt.grad.double().abs() * dr.p).sum()) for pt, dr in zip(T["head"], drift))
        bar = first + 2.0 * noise
        diff = abs(Fu["losses"][-1] - T["losses"][-1])
        worst_l = max(worst_l, diff / bar if bar else (0.0 if diff == 0 else float("inf")))
        assert diff <= bar, "step %d: losses %.9g (fused) and %.9g (torch) differ by %.3e, bar %.3e = %.3e + 2 * %.3e" % (
            s, Fu["losses"][-1], T["losses"][-1], diff, bar, first, noise)
        if s == 0:
            assert Fu["losses"][0] == T["losses"][0]
            assert all(torch.equal(a.grad, b.grad) for a, b in zip(Fu["head"], T["head"]))
        for pt, pf, dr in zip(T["head"], Fu["head"], drift):
            st = T["opt"].state.get(pt, {})
            state = dict(p=pt.detach().double(), m=st["exp_avg"].double() if st else zero(pt),
                         v=st["exp_avg_sq"].double() if st else zero(pt), vmax=st["max_exp_avg_sq"].double() if st else zero(pt))
            dr.step(state, pt.grad.double(), h, s + 1, ("kernel", "torch"), E_g=(pf.grad - pt.grad).abs())
        T["opt"].step()
        Fu["opt"].step()
        for i, (pt, pf, dr) in enumerate(zip(T["head"], Fu["head"], drift)):
            ok, ratio, nz, msg = evaluate(pf.detach(), pt.detach().double(), dr.p)
            worst_p = max(worst_p, ratio)
            assert ok, ("step %d, head parameter %d" % (s, i), msg)
    print("sep fine-tune: torch losses", ["%.4e" % x for x in T["losses"]])
    print("               fused losses", ["%.4e" % x for x in Fu["losses"]])
    print("               forward noise N %.3e; worst |dL| / bar %.3f, worst |dp| / bound %.3f" % (noise, worst_l, worst_p))
    assert T["losses"][-1] < T["losses"][0] and Fu["losses"][-1] < Fu["losses"][0]
    for r in (T, Fu):
        now = dict(r["sep"].named_parameters())
        for k, t in r["frozen"].items():
            assert torch.equal(t, now[k].detach()) and now[k].grad is None, k
        assert all(float(r["opt"].state[p]["step"]) == steps for p in r["head"])
