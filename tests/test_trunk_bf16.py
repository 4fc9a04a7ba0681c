"""The bf16 training mode of the trunk (copenet.set_trunk_trainable(True, precision="bf16"); trunk_grad_bf16.hip) as a whole.

1. Against an fp64 emulation of the numerics contract, written here: the walk of oracle.copenet_ref's trunk with a
   round-to-nearest-even to bf16 at exactly the stores of the contract, forward (crops, weights, conv output, BatchNorm output) and
   backward (every activation gradient a kernel stores: BatchNorm's gx, a data gradient with its fused add, the pools' gradients).
   A rounding decision can flip between fp32 and fp64 accumulation and a flip propagates, so the bar is measured against something
   that is not the code under test: the same emulation run with fp32 accumulation on the CPU gives E_cpu per tensor (rel_err of
   tests/conftest.py against the fp64 emulation), and the GPU must be within max(4 E_cpu, 2^-7) (2^-7: one bf16 ulp, one flip).
2. One SGD step along the bf16 gradients lowers a fixed loss evaluated by the fp32 path.
3. The contract behaviour the fp32 path has; 4. precision="fp32" is the default path bit for bit; 5. no torch conv / BN / pool."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, rel_err

pytestmark = pytest.mark.gpu
MOM, EPS = 0.1, 1e-5
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _net(sd, dev, precision="bf16", trainable=True):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32")
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    if trainable:
        if precision is None:
            net.set_trunk_trainable(True)
        else:
            net.set_trunk_trainable(True, precision=precision)
    return net


def _trunk_keys(net):
    from airpose_amd import trunk_grad
    names = {id(m): n for n, m in net.named_modules()}
    out = []
    for conv, bn in trunk_grad.conv_bn_pairs(net):
        out += [names[id(conv)] + ".weight", names[id(bn)] + ".weight", names[id(bn)] + ".bias"]
    return out, [names[id(bn)] for _, bn in trunk_grad.conv_bn_pairs(net)]


def _images(n, seed):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the emulation of the contract
def _rne(t):
    return t.to(BF).to(t.dtype)


class _Q(torch.autograd.Function):
    """y = rne(x) when fwd, g_x = rne(g_y) when bwd (else the identity in that direction)"""
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return _rne(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_rne(g) if ctx.bwd else g), None, None


class _Fork(torch.autograd.Function):
    """A block input read by conv1 and by the residual / downsample branch: the two gradients are added in the working precision
    and rounded once (the data gradient of conv1 with its fused add)"""
    @staticmethod
    def forward(ctx, x, quant):
        ctx.quant = quant
        return x.clone(), x.clone()

    @staticmethod
    def backward(ctx, g1, g2):
        s = g1 + g2
        return (_rne(s) if ctx.quant else s), None


def _emulate(sd, x, train, quant):
    """forward_feat_ext on the state dict sd (its dtype is the working precision); quant = False is the plain graph"""
    qf = lambda t: _Q.apply(t, quant, False)                          # a stored forward value
    qb = lambda t: _Q.apply(t, False, quant)                          # a stored activation gradient
    qfb = lambda t: _Q.apply(t, quant, quant)

    def conv_bn(x, p_conv, p_bn, stride, pad, res=None, relu=True, round_dgrad=True):
        # weights: bf16 copy of the fp32 master, gradient straight to the master; conv output stored in bf16; its gradient
        # (BatchNorm's gx) stored in bf16; the data gradient stored in bf16 (round_dgrad False: left to the caller's fused add, or fp32)
        z = qfb(F.conv2d(qb(x) if round_dgrad else x, qf(sd[p_conv + ".weight"]), stride=stride, padding=pad))
        y = F.batch_norm(z, sd[p_bn + ".running_mean"], sd[p_bn + ".running_var"], sd[p_bn + ".weight"], sd[p_bn + ".bias"], train,
                         MOM, EPS)
        if res is not None:
            y = y + res
        if relu:
            y = F.relu(y)
        return qf(y)

    x = qf(x)
    x = conv_bn(x, "conv1", "bn1", 2, 3, round_dgrad=False)           # the crop gradient stays fp32
    x = F.max_pool2d(qb(x), 3, 2, 1)
    for li, nblocks in enumerate((3, 4, 6, 3), start=1):
        for bi in range(nblocks):
            p = "layer%d.%d" % (li, bi)
            stride = 2 if (bi == 0 and li > 1) else 1
            x1, x2 = _Fork.apply(x, quant)
            out = conv_bn(x1, p + ".conv1", p + ".bn1", 1, 0, round_dgrad=False)
            out = conv_bn(out, p + ".conv2", p + ".bn2", stride, 1)
            # the downsample's data gradient stays fp32 and enters the fork's sum unrounded: one rounding per block input
            res = conv_bn(x2, p + ".downsample.0", p + ".downsample.1", stride, 0, relu=False, round_dgrad=False) if bi == 0 else x2
            x = conv_bn(out, p + ".conv3", p + ".bn3", 1, 0, res=res)
    return F.avg_pool2d(qb(x), 7, stride=1).flatten(1)


def _run_emulation(net, x, Wt, dtype, train, quant=True):
    keys, _ = _trunk_keys(net)
    sd = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in net.state_dict().items()}
    for k in keys:
        sd[k].requires_grad_(True)
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    xf = _emulate(sd, xr, train, quant)
    (xf * Wt.to(dtype)).sum().backward()
    return xf.detach(), sd, xr


def test_the_emulation_without_rounding_is_the_oracle(copenet_sd):
    from oracle import copenet_ref
    sd = {k: v.double() for k, v in copenet_sd.items() if v.is_floating_point()}
    x = _images(1, 3).double()
    with torch.no_grad():
        assert torch.equal(_emulate(sd, x, False, False), copenet_ref.forward_feat_ext(x, sd))


# ------------------------------------------------------------------------------------------------ 1. against the emulation
@pytest.mark.parametrize("train,n", [pytest.param(True, 4, id="train"), pytest.param(False, 4, id="eval"),
                                     pytest.param(True, 1, id="train-n1")])
def test_whole_trunk_matches_fp64_emulation_of_the_contract(copenet_sd, dev, train, n):
    """Measured gpu_err / bar per tensor class: see DESIGN 4.3.4 (the test prints the worst ratio of each class)."""
    net = _net(copenet_sd, dev).train(train)
    keys, bns = _trunk_keys(net)
    x = _images(n, 21)
    Wt = torch.randn(n, 2048, generator=torch.Generator().manual_seed(22))
    before = {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    xf64, sd64, x64 = _run_emulation(net, x, Wt, torch.float64, train)
    xf32, sd32, x32 = _run_emulation(net, x, Wt, torch.float32, train)
    xg = x.to(dev).requires_grad_(True)
    xf = net.forward_feat_ext(xg)
    assert xf.grad_fn is not None and xf.dtype == torch.float32
    (xf * Wt.to(dev)).sum().backward()
    worst, fails = {}, []

    def check(cls, name, got, want, cpu):
        e, ecpu = rel_err(got.detach().cpu().numpy(), want.detach().numpy()), rel_err(cpu.detach().numpy(), want.detach().numpy())
        bar = max(4 * ecpu, 2.0 ** -7)
        print("%-34s gpu %.3e  cpu-fp32 %.3e  bar %.3e  ratio %.3f" % (name, e, ecpu, bar, e / bar))
        worst[cls] = max(worst.get(cls, 0.0), e / bar)
        if not e <= bar:
            fails.append((name, e, bar))

    check("xf", "xf", xf, xf64, xf32)
    params = dict(net.named_parameters())
    for k in keys:
        assert params[k].grad is not None and params[k].grad.dtype == torch.float32, k
        cls = "gW" if params[k].dim() == 4 else ("g_gamma" if k.endswith("weight") else "g_beta")
        check(cls, k, params[k].grad, sd64[k].grad, sd32[k].grad)
    assert xg.grad.dtype == torch.float32
    check("g_x", "g_x", xg.grad, x64.grad, x32.grad)
    after = net.state_dict()
    for p in bns:
        if train:
            for b in ("running_mean", "running_var"):
                check(b, p + "." + b, after[p + "." + b], sd64[p + "." + b], sd32[p + "." + b])
            assert int(after[p + ".num_batches_tracked"]) == int(before[p + ".num_batches_tracked"]) + 1
        else:
            for b in ("running_mean", "running_var", "num_batches_tracked"):
                assert torch.equal(after[p + "." + b], before[p + "." + b]), (p, b)
    print("train=%s n=%d worst gpu_err / bar per class: %s" % (train, n, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert not fails, fails


def _saved_layers(ws, n):
    """(name, input, z, mean, invstd) of the 53 conv + BN pairs read back from a save = 1 workspace of apg_trunk_fwd_p: the
    buffer list of DESIGN 4.3.4 in order (every buffer on a 256-byte boundary): the 8-channel crops; per layer wf, wd, z, a, mean,
    invstd; the max-pool output after the stem."""
    off = [0]

    def take(nbytes, dtype, shape):
        t = ws[off[0]:off[0] + nbytes].view(dtype).view(shape)
        off[0] += (nbytes + 255) // 256 * 256
        return t

    out = []

    def layer(name, x, H, C, K, R, st, pad):
        Cp, Ho = (C + 7) // 8 * 8, (H + 2 * pad - R) // st + 1
        for _ in range(2):
            take(K * R * R * Cp * 2, BF, (K, R, R, Cp))
        z = take(n * Ho * Ho * K * 2, BF, (n, Ho, Ho, K))
        a = take(n * Ho * Ho * K * 2, BF, (n, Ho, Ho, K))
        mean, invstd = take(K * 4, torch.float32, (K,)), take(K * 4, torch.float32, (K,))
        out.append((name, x, z, mean, invstd, st, pad))
        return a

    x = take(n * 224 * 224 * 8 * 2, BF, (n, 224, 224, 8))
    layer("conv1", x, 224, 3, 64, 7, 2, 3)
    x = take(n * 56 * 56 * 64 * 2, BF, (n, 56, 56, 64))
    H, C = 56, 64
    for li, (nb, p) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512)), start=1):
        for b in range(nb):
            st, nm = (2 if (b == 0 and li > 1) else 1), "layer%d.%d." % (li, b)
            a1 = layer(nm + "conv1", x, H, C, p, 1, 1, 0)
            a2 = layer(nm + "conv2", a1, H, p, p, 3, st, 1)
            Ho = a2.shape[1]
            a3 = layer(nm + "conv3", a2, Ho, p, 4 * p, 1, 1, 0)
            if b == 0:
                layer(nm + "downsample.0", x, H, C, 4 * p, 1, st, 0)
            x, H, C = a3, Ho, 4 * p
    assert len(out) == 53
    return out


@pytest.mark.parametrize("n", [1, 2])
def test_walker_statistics_come_from_the_stored_bf16_conv_output(copenet_sd, dev, n):
    """The contract row 'BatchNorm statistics: from the stored (bf16-rounded) conv output'.  The walker's saved workspace holds
    every layer's stored conv output z and the save_mean / save_invstd its BatchNorm used: they must be the fp64 statistics of
    that stored z to 1e-5 (the fp32 bar of the statistics).  That the check can tell the two apart is asserted too: on a layer4
    conv at n = 1 (49 rows per channel) the statistics of the UNROUNDED product -- fp64 conv of the stored bf16 input and the
    RNE'd weights -- must differ from those of the stored z by more than 1e-5, so a build that feeds the accumulator to the
    statistics fails here."""
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    from airpose_amd import trunk_grad
    net = _net(copenet_sd, dev).train()
    pairs = trunk_grad.conv_bn_pairs(net)
    params, bufs = trunk_grad._tables(pairs, dev)
    x = _images(n, 17).to(dev)
    L = G.lib()
    nbytes = L.apg_trunk_workspace_bytes_p(n, 1, 1)
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    xf = torch.empty(n, 2048, device=dev)
    G.check(L.apg_trunk_fwd_p(1, n, N.dptr(x), trunk_grad._table_ptrs(params, bufs), 1, MOM, EPS, N.dptr(xf), 1, ws.data_ptr(), nbytes,
                              N.stream_ptr(dev)), "apg_trunk_fwd_p")
    torch.cuda.synchronize()
    layers = _saved_layers(ws.cpu(), n)
    names = {id(m): k for k, m in net.named_modules()}
    assert [names[id(c)] for c, _ in pairs] == [l[0] for l in layers]
    worst = 0.0
    for name, xin, z, mean, invstd, st, pad in layers:
        z64 = z.double().flatten(0, 2)
        assert torch.isfinite(z64).all() and z64.abs().max() > 0, name
        mu, var = z64.mean(0), z64.var(0, unbiased=False)
        e = max(rel_err(mean.numpy(), mu.numpy()), rel_err(invstd.numpy(), (1 / torch.sqrt(var + EPS)).numpy()))
        worst = max(worst, e)
        assert e <= 1e-5, (name, e)
    print("n=%d: worst statistics error against the stored conv output %.2e" % (n, worst))
    if n == 1:
        (name, xin, z, mean, invstd, st, pad), conv = layers[-3], pairs[-3][0]
        assert name == "layer4.2.conv1"
        w = conv.weight.detach().cpu().to(BF).double()
        raw = F.conv2d(xin.double().permute(0, 3, 1, 2), w, stride=st, padding=pad).permute(0, 2, 3, 1).flatten(0, 2)
        assert torch.equal(raw.to(BF).view(torch.int16), z.flatten(0, 2).view(torch.int16)) or \
            (raw.to(BF).float() - z.flatten(0, 2).float()).abs().max() <= 2.0 ** -7 * raw.abs().max()   # z is the rounded product
        mu_raw, istd_raw = raw.mean(0), 1 / torch.sqrt(raw.var(0, unbiased=False) + EPS)
        gap = max(rel_err(mean.numpy(), mu_raw.numpy()), rel_err(invstd.numpy(), istd_raw.numpy()))
        print("layer4.2.conv1: statistics of the unrounded product are %.2e away" % gap)
        assert gap > 1e-5, gap


# ------------------------------------------------------------------------------------------------ 2. descent direction
def test_one_sgd_step_along_the_bf16_gradients_lowers_the_loss(copenet_sd, dev):
    """Loss = mean(xf^2) of a fixed batch in train mode.  The learning rate is not tuned: lr = 0.01 L / |g|^2 with the fp32
    path's own gradient g, the step whose first-order decrease is 1 % of the loss; the test first shows that the fp32 gradients
    lower the loss at that rate, then takes the same step along the bf16 gradients.  Both losses are evaluated by the fp32 path."""
    x = _images(4, 31).to(dev)

    def loss32(sd):
        with torch.no_grad():
            return float(_net(sd, dev, "fp32").train().forward_feat_ext(x).square().mean())

    def grads(precision):
        net = _net(copenet_sd, dev, precision).train()
        net.forward_feat_ext(x).square().mean().backward()
        keys, _ = _trunk_keys(net)
        params = dict(net.named_parameters())
        return {k: params[k].grad.clone() for k in keys}

    def stepped(g, lr):
        sd = {k: v.clone() for k, v in copenet_sd.items()}
        for k, gk in g.items():
            sd[k] = sd[k] - lr * gk.cpu()
        return sd

    L0 = loss32(copenet_sd)
    g32, g16 = grads("fp32"), grads("bf16")
    lr = 0.01 * L0 / float(sum(g.double().square().sum() for g in g32.values()))
    L32, L16 = loss32(stepped(g32, lr)), loss32(stepped(g16, lr))
    print("loss %.6e -> fp32 step %.6e, bf16 step %.6e (lr %.3e)" % (L0, L32, L16, lr))
    assert L32 < L0, "the learning rate does not lower the loss along the fp32 gradients"
    assert L16 < L0


# ------------------------------------------------------------------------------------------------ 3. contract behaviour
def _pair_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"x0": torch.randn(B, 3, 224, 224, generator=g), "x1": torch.randn(B, 3, 224, 224, generator=g)}
    for v in "01":
        d["bb" + v] = torch.rand(B, 3, generator=g) + 0.2
        d["pos" + v] = torch.randn(B, 3, generator=g) * 0.3 + torch.tensor([0., 0., 10.])
    return d


def _fwd_args(d, dev):
    return [d[k].to(dev) for k in ("x0", "x1", "bb0", "bb1", "pos0", "pos1")]


def test_steps_are_bit_reproducible_and_outputs_are_fp32(copenet_sd, dev):
    net = _net(copenet_sd, dev).train()
    d = _pair_inputs(3, 41)
    start = {k: v.clone() for k, v in net.state_dict().items() if "running" in k}

    def step():
        with torch.no_grad():
            for k, v in start.items():
                net.state_dict()[k].copy_(v)
        for p in net.parameters():
            p.grad = None
        x0 = d["x0"].to(dev).requires_grad_(True)
        torch.manual_seed(7)
        outs = net(x0, *_fwd_args(d, dev)[1:])
        sum(o.square().sum() for o in outs).backward()
        return ([o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None},
                x0.grad.clone(), {k: v.clone() for k, v in net.state_dict().items() if "running" in k})

    o1, g1, x1, s1 = step()
    o2, g2, x2, s2 = step()
    keys, _ = _trunk_keys(net)
    assert set(keys) <= set(g1) and set(g1) == set(g2)
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert torch.equal(x1, x2)
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    assert all(g.dtype == torch.float32 for g in g1.values()) and x1.dtype == torch.float32
    assert net.conv1.weight.grad is not None and net.conv1.weight.grad.abs().max() > 0       # forward: trunk bf16, head fp32
    xf = net.forward_feat_ext(d["x0"].to(dev))
    assert xf.dtype == torch.float32 and xf.grad_fn is not None


def test_running_statistics_update_per_call_and_per_view(copenet_sd, dev):
    net, twin = _net(copenet_sd, dev).train(), _net(copenet_sd, dev).train()
    _, bns = _trunk_keys(net)
    args = _fwd_args(_pair_inputs(2, 51), dev)
    v = net.bn1.running_mean._version
    with torch.no_grad():
        net(*args)                                                   # view 0's trunk, then view 1's
        twin.forward_feat_ext(args[0])
        one = {k: t.clone() for k, t in twin.state_dict().items() if "running" in k}
        twin.forward_feat_ext(args[1])
    assert net.bn1.running_mean._version > v
    a, b = net.state_dict(), twin.state_dict()
    for p in bns:
        for s in ("running_mean", "running_var"):
            assert torch.equal(a[p + "." + s], b[p + "." + s]), (p, s)
            assert not torch.equal(a[p + "." + s], one[p + "." + s]), (p, s)
        assert int(a[p + ".num_batches_tracked"]) == int(copenet_sd[p + ".num_batches_tracked"]) + 2


def test_an_optimizer_step_takes_effect_on_the_next_call(copenet_sd, dev):
    """no stale bf16 weight copy: after an in-place update the next call equals a fresh net on the updated state"""
    net = _net(copenet_sd, dev).train()
    x = _images(2, 61).to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    xf1 = net.forward_feat_ext(x)
    xf1.square().mean().backward()
    opt.step()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    xf2 = net.forward_feat_ext(x)
    assert not torch.equal(xf1, xf2)
    fresh = _net(sd, dev).train()
    assert torch.equal(fresh.forward_feat_ext(x), xf2)


def test_eval_no_grad_after_bf16_training_repacks_the_inference_path(copenet_sd, dev):
    net = _net(copenet_sd, dev)
    args = _fwd_args(_pair_inputs(2, 71), dev)
    with torch.no_grad():
        net(*args)                                                   # the inference handle now holds the initial weights
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad()
        sum(o.square().mean() for o in net(*args)).backward()
        opt.step()
    net.eval()
    with torch.no_grad():
        got = net(*args)
        fresh = _net(net.state_dict(), dev, trainable=False)
        want = fresh(*args)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(net.forward_feat_ext(args[0]), fresh.forward_feat_ext(args[0]))


def test_train_mode_under_no_grad_records_nothing_and_uses_the_small_workspace(copenet_sd, dev, monkeypatch):
    from airpose_amd import trunk_grad
    net = _net(copenet_sd, dev).train()
    x = _images(2, 81).to(dev)
    seen = []
    real = trunk_grad._run_fwd_p

    def spy(L, prec, n, x_, params, bufs, train, momentum, eps, save, dev_):
        seen.append((prec, bool(save), L.apg_trunk_workspace_bytes_p(n, int(save), prec)))
        return real(L, prec, n, x_, params, bufs, train, momentum, eps, save, dev_)
    monkeypatch.setattr(trunk_grad, "_run_fwd_p", spy)
    with torch.no_grad():
        xf = net.forward_feat_ext(x)
    assert xf.grad_fn is None and not xf.requires_grad
    assert int(net.bn1.num_batches_tracked) == int(copenet_sd["bn1.num_batches_tracked"]) + 1
    xg = net.forward_feat_ext(x)
    assert xg.grad_fn is not None
    assert [s[:2] for s in seen] == [(1, False), (1, True)] and seen[0][2] < seen[1][2], seen
    assert torch.equal(xf, xg)                                       # the same forward arithmetic with and without the saved buffers


# ------------------------------------------------------------------------------------------------ 4. nothing else moved
def test_explicit_fp32_is_the_default_path_bit_for_bit(copenet_sd, dev):
    x = _images(2, 91)
    outs = []
    for precision in (None, "fp32"):
        net = _net(copenet_sd, dev, precision).train()
        assert net.trunk_precision == "fp32"
        xg = x.to(dev).requires_grad_(True)
        xf = net.forward_feat_ext(xg)
        xf.square().sum().backward()
        keys, _ = _trunk_keys(net)
        params = dict(net.named_parameters())
        outs.append([xf.detach(), xg.grad] + [params[k].grad for k in keys] + [net.bn1.running_var.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    bf = _net(copenet_sd, dev, "bf16").train()
    assert not torch.equal(bf.forward_feat_ext(x.to(dev)).detach(), outs[0][0])      # and the switch does switch


# ------------------------------------------------------------------------------------------------ 5. no foreign kernels on the path
def test_bf16_trunk_path_calls_no_torch_conv_bn_or_pool(copenet_sd, dev, monkeypatch):
    net = _net(copenet_sd, dev).train()
    x = _images(2, 95).to(dev).requires_grad_(True)

    def boom(*a, **k):
        raise AssertionError("torch compute on the trainable trunk")
    for mod, name in ((F, "conv2d"), (torch, "conv2d"), (F, "batch_norm"), (torch, "batch_norm"), (F, "max_pool2d"),
                      (F, "avg_pool2d")):
        monkeypatch.setattr(mod, name, boom)
    xf = net.forward_feat_ext(x)
    xf.square().sum().backward()
    assert x.grad is not None and net.conv1.weight.grad is not None and net.layer1[0].downsample[1].bias.grad is not None
    assert np.isfinite(xf.detach().cpu().numpy()).all()
