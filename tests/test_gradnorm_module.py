"""airpose_amd.clip_grad_norm_ and FusedAdam(max_grad_norm=, skip_nonfinite=) (airpose_amd/optim.py on apg_grad_norm, apg_grad_scale and
apg_adam_step_guarded) as torch sees them.

  * clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ on a CPU copy of the same gradients (a small stack of Linear layers, about
    26 000 parameters).  Bar: K u relative in the norm and in every scaled gradient, K the total element count and u = 2^-24 -- the
    worst case of ANY fp32 summation order, so a check of the formula, not of precision (test_gradnorm_fp64.py holds the precision);
    the cases are chosen so that a wrong formula (no eps, no clamp, a sum of the per-tensor norms) moves the result by more than 5 %.
  * FusedAdam(max_grad_norm=c) over 20 steps against clip_grad_norm_ + plain FusedAdam on the same gradients: bit-equal in p and the
    moments after every step -- fusing changes nothing but which pass applies the product.
  * Against torch's clip + torch.optim.Adam by test_optim_module's method: the measured difference of the two runs' CLIPPED gradients
    enters Drift as E_g, everything else is its counted bounds.
  * An Inf injected at step 7 with skip_nonfinite=True and without, state dicts to and from torch.optim.Adam with the options set, two
    param groups under one global norm, a parameter without a gradient.
"""
import copy
import math

import pytest
import torch

import test_optim_module as M

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
STEPS = 20
KW = M.KW
CLIP = 0.5                                                # the gradients of M.feed have a norm of 2 to 3: every step clips


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _mlp(dev, seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.Tanh(), torch.nn.Linear(128, 128), torch.nn.Tanh(), torch.nn.Linear(128, 10))
    return net.to(dev)


def _backward(net, dev, seed=1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(32, 64, generator=g).to(dev), torch.randn(32, 10, generator=g).to(dev)
    net.zero_grad()
    loss = scale * ((net(x) - y) ** 2).mean()
    loss.backward()
    return loss


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


@pytest.mark.parametrize("case", ["clipped", "not-clipped", "eps"])
def test_clip_grad_norm_against_torch(dev, case):
    import airpose_amd
    net = _mlp(dev)
    _backward(net, dev)
    params = list(net.parameters())
    if case == "eps":                                                         # a norm of 5e-6, where torch's 1e-6 is a fifth of it
        _backward(net, dev, scale=5e-6 / _norm64([p.grad.detach().cpu() for p in params]))
    K = sum(p.numel() for p in params)
    assert 20000 < K < 40000
    raw = [p.grad.detach().cpu().clone() for p in params]
    n64 = _norm64(raw)
    max_norm = 2.0 * n64 if case == "not-clipped" else 0.5 * n64
    if case == "eps":
        assert 4e-6 < n64 < 6e-6, n64
    cpu = [torch.nn.Parameter(torch.zeros_like(g)) for g in raw]
    for c, g in zip(cpu, raw):
        c.grad = g.clone()
    want = torch.nn.utils.clip_grad_norm_(cpu, max_norm)
    got = airpose_amd.clip_grad_norm_(params, max_norm)
    assert torch.is_tensor(got) and got.dim() == 0 and got.dtype == torch.float32 and got.device == params[0].device
    assert abs(float(got) - float(want)) <= K * U32 * float(want), (float(got), float(want))
    assert abs(float(got) - n64) <= 2 * U32 * n64                             # and it IS the norm
    coef = min(1.0, max_norm / (n64 + 1e-6))
    assert (coef == 1.0) == (case == "not-clipped") and (case != "eps" or coef < 0.48), coef
    for p, c, g in zip(params, cpu, raw):
        a, b = p.grad.detach().cpu().double(), c.grad.double()
        assert bool(((a - b).abs() <= K * U32 * b.abs()).all()), case
        if case == "not-clipped":
            assert torch.equal(p.grad.detach().cpu().view(torch.int32), g.view(torch.int32))      # untouched
    # the generator form and a single tensor, as torch takes them
    assert float(airpose_amd.clip_grad_norm_(iter(params), float("inf"))) > 0
    one = airpose_amd.clip_grad_norm_(params[0], float("inf"))
    assert abs(float(one) - _norm64([params[0].grad.cpu()])) <= 2 * U32 * float(one)


def test_clip_grad_norm_nonfinite_empty_and_refusals(dev):
    import airpose_amd
    clip = airpose_amd.clip_grad_norm_
    net = _mlp(dev)
    _backward(net, dev)
    params = list(net.parameters())
    keep = [p.grad.clone() for p in params]
    params[2].grad[5, 7] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip(params, 1.0, error_if_nonfinite=True)
    for p, k in zip(params, keep):                                            # raised before the gradients were touched
        if p is not params[2]:
            assert torch.equal(p.grad, k)
    total = clip(params, 1.0)                                                 # without the flag: no error, no synchronisation, NaN gradients
    assert not math.isfinite(float(total)) and all(bool(torch.isnan(p.grad).all()) for p in params)
    for p, k in zip(params, keep):
        p.grad = k.clone()
    assert math.isfinite(float(clip(params, 1.0, error_if_nonfinite=True)))
    # empty lists, and parameters without a gradient
    assert float(clip([], 1.0)) == 0.0
    nog = [torch.nn.Parameter(torch.randn(3, device=dev))]
    assert float(clip(nog, 1.0)) == 0.0
    some = [nog[0], params[0]]
    assert abs(float(clip(some, float("inf"))) - _norm64([params[0].grad.cpu()])) <= 1e-6 * float(params[0].grad.norm())
    with pytest.raises(ValueError, match="norm_type"):
        clip(params, 1.0, norm_type=1.0)
    bad = torch.nn.Parameter(torch.randn(6, 4, device=dev))
    bad.grad = torch.randn(4, 6, device=dev).t()
    with pytest.raises(ValueError, match="not contiguous"):
        clip([bad], 1.0)
    half = torch.nn.Parameter(torch.randn(6, device=dev, dtype=torch.float16))
    half.grad = torch.randn(6, device=dev, dtype=torch.float16)
    with pytest.raises(TypeError, match="float16"):
        clip([half], 1.0)


def _pair(dev, values, guarded_kw, plain_kw=None, groups=None):
    """FusedAdam with the options and a plain FusedAdam over clones of the same values"""
    from airpose_amd import FusedAdam
    pa, pb = M.params_on(dev, values), M.params_on(dev, values)
    arg = lambda ps: ps if groups is None else [dict(params=[ps[i] for i in idx], **o) for idx, o in groups]
    kw = KW if groups is None else {k: v for k, v in KW.items() if k not in ("lr", "weight_decay")}
    return FusedAdam(arg(pa), **dict(kw, **guarded_kw)), pa, FusedAdam(arg(pb), **dict(kw, **(plain_kw or {}))), pb


def test_fused_clip_over_twenty_steps_is_clip_then_step_bit_for_bit(dev):
    import airpose_amd
    values = M.start_values()
    a, pa, b, pb = _pair(dev, values, dict(max_grad_norm=CLIP))
    assert a.grad_norm is None
    for s in range(STEPS):
        M.feed(pa, s)
        M.feed(pb, s)
        raw = [p.grad.clone() for p in pa]
        a.step()
        total = airpose_amd.clip_grad_norm_(pb, CLIP)
        b.step()
        torch.cuda.synchronize()
        assert all(torch.equal(p.grad, g) for p, g in zip(pa, raw)), "the fused step rewrote a gradient"
        assert float(total) > 2 * CLIP and float(a.grad_norm) == float(total)
        assert M.bits_equal(M.snapshot(a, pa), M.snapshot(b, pb)), s
    assert a.skipped_steps() == 0 and a.grad_norm.device == pa[0].device and a.grad_norm.dim() == 0


def test_fused_clip_against_torch_clip_and_torch_adam(dev):
    import airpose_amd
    from airpose_amd import FusedAdam
    values = M.start_values()
    pf, pt = M.params_on(dev, values), M.params_on(dev, values)
    fused = FusedAdam(pf, max_grad_norm=CLIP, **KW)
    ref = torch.optim.Adam(pt, foreach=False, **KW)
    drift = [M.Drift(p) for p in pt]
    zero = lambda p: torch.zeros_like(p, dtype=torch.float64)
    worst = 0.0
    for s in range(STEPS):
        M.feed(pf, s)
        M.feed(pt, s)
        shadow = [torch.nn.Parameter(p.detach().clone()) for p in pf]        # the fused run's clipped gradients, made visible
        for q, p in zip(shadow, pf):
            q.grad = p.grad.clone()
        airpose_amd.clip_grad_norm_(shadow, CLIP)
        torch.nn.utils.clip_grad_norm_(pt, CLIP, foreach=False)
        for p, q, d in zip(pt, shadow, drift):
            st = ref.state.get(p, {})
            state = dict(p=p.detach().double(), m=st["exp_avg"].double() if st else zero(p), v=st["exp_avg_sq"].double() if st else zero(p),
                         vmax=st["max_exp_avg_sq"].double() if st else zero(p))
            d.step(state, p.grad.double(), M.H, s + 1, ("kernel", "torch"), E_g=(q.grad - p.grad).abs())
        fused.step()
        ref.step()
        for i, (p, q, d) in enumerate(zip(pt, pf, drift)):
            st, sf = ref.state[p], fused.state[q]
            for name, got, want, bound in (("p", q, p, d.p), ("exp_avg", sf["exp_avg"], st["exp_avg"], d.m),
                                           ("exp_avg_sq", sf["exp_avg_sq"], st["exp_avg_sq"], d.v),
                                           ("max_exp_avg_sq", sf["max_exp_avg_sq"], st["max_exp_avg_sq"], d.x)):
                ok, ratio, nz, msg = M.evaluate(got.detach(), want.detach().double(), bound)
                worst = max(worst, ratio)
                assert ok, ("step %d, tensor %d, %s" % (s, i, name), msg)
    print("fused clip against torch clip + torch.optim.Adam: worst |d| / bound %.3f" % worst)


@pytest.mark.parametrize("skip", [True, False])
def test_an_inf_at_step_seven(dev, skip):
    from airpose_amd import FusedAdam
    net = _mlp(dev, seed=3)
    params = list(net.parameters())
    opt = FusedAdam(params, lr=1e-3, amsgrad=True, max_grad_norm=1.0, skip_nonfinite=skip)
    snaps = []
    for s in range(STEPS):
        _backward(net, dev, seed=100 + s)
        if s == 7:
            params[0].grad[3, 3] = float("inf")
        opt.step()
        snaps.append(M.snapshot(opt, params))
        if s == 7:
            assert not math.isfinite(float(opt.grad_norm))
    assert all(float(st["step"]) == STEPS for st in opt.state.values())      # the host's count advances on a skipped step too
    final = snaps[-1]
    if skip:
        for a, b in zip(snaps[6], snaps[7]):                                  # step 7 changed nothing but the count
            for k in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
            assert float(a["step"]) == 7 and float(b["step"]) == 8
        assert all(bool(torch.isfinite(t[k]).all()) for t in final for k in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
        assert any(not torch.equal(a["p"], b["p"]) for a, b in zip(snaps[7], final)), "training went on"
        assert opt.skipped_steps() == 1
        assert math.isfinite(float(opt.grad_norm))
    else:
        assert all(bool(torch.isnan(t["p"]).any()) for t in final)            # torch's behaviour: the run is lost
        assert opt.skipped_steps() == 0


def test_state_dicts_round_trip_with_the_options_set(dev):
    from airpose_amd import FusedAdam
    values = M.start_values(2)
    half, total = 6, 12
    opts = dict(max_grad_norm=CLIP, skip_nonfinite=True)
    pu = M.params_on(dev, values)
    ou = FusedAdam(pu, **dict(KW, **opts))
    M.run_steps(ou, pu, range(total))
    p1 = M.params_on(dev, values)
    o1 = FusedAdam(p1, **dict(KW, **opts))
    M.run_steps(o1, p1, range(half))
    sd = o1.state_dict()
    p2 = M.params_on(dev, [p.detach().cpu() for p in p1])
    o2 = torch.optim.Adam(p2, foreach=False, **KW)
    o2.load_state_dict(M._through(sd))                                        # into torch ...
    assert M.bits_equal(M.snapshot(o1, p1), M.snapshot(o2, p2))
    assert o2.state_dict()["param_groups"][0].keys() == sd["param_groups"][0].keys()
    assert not any("max_grad_norm" in g or "skip_nonfinite" in g for g in sd["param_groups"])
    p3 = M.params_on(dev, [p.detach().cpu() for p in p2])
    o3 = FusedAdam(p3, **dict(KW, **opts))
    o3.load_state_dict(M._through(o2.state_dict()))                           # ... and back: the options are the constructor's
    assert o3.max_grad_norm == CLIP and o3.skip_nonfinite is True
    M.run_steps(o3, p3, range(half, total))
    assert M.bits_equal(M.snapshot(ou, pu), M.snapshot(o3, p3))
    o4 = copy.deepcopy(o3)                                                    # (a pickled optimizer keeps or regains the attributes)
    assert o4.max_grad_norm == CLIP and o4.skip_nonfinite is True


def test_two_param_groups_share_one_global_norm(dev):
    import airpose_amd
    values = M.start_values(5)
    n = len(values)
    groups = [(list(range(0, n, 2)), dict(lr=5e-5, weight_decay=0.0)), (list(range(1, n, 2)), dict(lr=1e-3, weight_decay=1e-4))]
    a, pa, b, pb = _pair(dev, values, dict(max_grad_norm=CLIP), groups=groups)
    for s in range(4):
        M.feed(pa, s)
        M.feed(pb, s)
        everything = _norm64([p.grad.cpu() for p in pa])
        first = _norm64([pa[i].grad.cpu() for i in groups[0][0]])
        a.step()
        # clip_grad_norm_ over the parameters in the optimizer's own order: group 0's, then group 1's
        order = [p for g in b.param_groups for p in g["params"]]
        airpose_amd.clip_grad_norm_(order, CLIP)
        b.step()
        torch.cuda.synchronize()
        assert abs(float(a.grad_norm) - everything) <= 2 * U32 * everything and first < 0.9 * everything
        assert M.bits_equal(M.snapshot(a, pa), M.snapshot(b, pb)), s


def test_a_parameter_without_a_gradient_is_left_out_of_norm_and_step(dev):
    import airpose_amd
    values = M.start_values(4)
    skip = {(2, 1), (2, 2), (7, 0), (5, 3)} | {(11, s) for s in range(5)}
    a, pa, b, pb = _pair(dev, values, dict(max_grad_norm=CLIP, skip_nonfinite=True))
    for s in range(5):
        M.feed(pa, s, skip)
        M.feed(pb, s, skip)
        before = M.snapshot(a, pa)
        have = _norm64([p.grad.cpu() for p in pa if p.grad is not None])
        a.step()
        airpose_amd.clip_grad_norm_(pb, CLIP)
        b.step()
        torch.cuda.synchronize()
        after = M.snapshot(a, pa)
        assert abs(float(a.grad_norm) - have) <= 2 * U32 * have
        assert M.bits_equal(after, M.snapshot(b, pb)), s
        for i in range(len(values)):
            if (i, s) in skip:
                assert M.bits_equal([before[i]], [after[i]]), (s, i)
    assert "step" not in after[11] and float(after[2]["step"]) == 3 and a.skipped_steps() == 0
