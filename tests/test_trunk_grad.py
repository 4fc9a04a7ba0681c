"""Trainable ResNet-50 trunk (libairpose_grad.so: trunk_grad.hip, airpose_amd/trunk_grad.py) against fp64 autograd: the layer
primitives, the whole trunk in train- and eval-mode BatchNorm, copenet.forward in train mode with per-view statistics,
determinism, the reference's training step with Adam, and unchanged inference behaviour.

The fp64 reference is oracle.copenet_ref.forward_feat_ext with its eval-mode _bn replaced, in this file only, by train-mode
F.batch_norm on fp64 copies of the running buffers.  For the 53-layer chain a gradient's bar is max(4 x the error of the same
restatement run in fp32 on the CPU, 1e-5).  That fp32 yardstick is the worse of two equally valid fp32 CPU runs, NCHW and
channels_last: the eval-mode chain of the test checkpoint is ill-conditioned enough that they differ by up to 6x on one tensor
(layer1.0.bn2.weight: 1.3e-4 and 7.3e-4 against fp64), and either alone would make the bar a coin toss."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, pose_rel_errs, rel_err

pytestmark = pytest.mark.gpu
MOM, EPS = 0.1, 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _net(sd, dev, trainable=True):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32")
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    if trainable:
        net.set_trunk_trainable(True)
    return net


def _trunk_keys(net):
    from airpose_amd import trunk_grad
    names = {id(m): n for n, m in net.named_modules()}
    out = []
    for conv, bn in trunk_grad.conv_bn_pairs(net):
        out += [names[id(conv)] + ".weight", names[id(bn)] + ".weight", names[id(bn)] + ".bias"]
    return out, [names[id(bn)] for _, bn in trunk_grad.conv_bn_pairs(net)]


def _images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 224, 224, generator=g)


def _restate(net, dtype, train, grad_keys, extra_grad=()):
    """CPU copy of the net's state in `dtype` (grad on grad_keys) and a _bn for the oracle: train mode updates copies of the
    running buffers, eval mode reads them."""
    sd = {k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu() for k, v in net.state_dict().items()}
    for k in list(grad_keys) + list(extra_grad):
        sd[k].requires_grad_(True)

    def bn(x, sd_, p):
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], train, MOM, EPS)
    return sd, bn


def _cl(t, on):
    return t.contiguous(memory_format=torch.channels_last) if on else t


def _ref_trunk(monkeypatch, net, x, Wt, dtype, train, with_x, cl=False):
    from oracle import copenet_ref
    keys, _ = _trunk_keys(net)
    sd, bn = _restate(net, dtype, train, keys)
    monkeypatch.setattr(copenet_ref, "_bn", bn)
    xr = x.detach().to(dtype).clone().requires_grad_(with_x)
    xf = copenet_ref.forward_feat_ext(_cl(xr, cl), sd)
    (xf * Wt.to(dtype)).sum().backward()
    monkeypatch.undo()
    return xf.detach(), sd, xr


def _bar(want, fp32_runs, floor=1e-5):
    return max(4 * max(rel_err(t.grad.numpy(), want.grad.numpy()) for t in fp32_runs), floor)


def _check_trunk_grads(net, x_gpu, sd64, x64, sd32s, x32s, what, floor=1e-5):
    """sd32s / x32s: the fp32 CPU restatements (NCHW, channels_last)"""
    keys, _ = _trunk_keys(net)
    params = dict(net.named_parameters())
    worst = 0.0
    for k in keys:
        got = params[k].grad
        assert got is not None, k
        e = rel_err(got.cpu().numpy(), sd64[k].grad.numpy())
        bar = _bar(sd64[k], [sd[k] for sd in sd32s], floor)
        worst = max(worst, e / bar)
        assert e <= bar, (what, k, e, bar)
    if x_gpu is not None:
        e = rel_err(x_gpu.grad.cpu().numpy(), x64.grad.numpy())
        bar = _bar(x64, x32s, floor)
        assert e <= bar, (what, "x", e, bar)
    print("%s: worst gradient error / bar %.3f" % (what, worst))


# ------------------------------------------------------------------------------------------------ 1. primitives
GEOMS = [  # (n, H, C, K, R, stride, pad)
    (2, 32, 3, 64, 7, 2, 3),             # the stem
    (2, 14, 64, 128, 1, 1, 0),           # 1 x 1 / s1
    (2, 14, 64, 64, 3, 1, 1),            # 3 x 3 / s1 / p1
    (2, 15, 64, 128, 3, 2, 1),           # 3 x 3 / s2 / p1 (odd size: the last row / column has no partner)
    (2, 14, 128, 256, 1, 2, 0),          # 1 x 1 / s2 (downsample)
]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("geom", GEOMS, ids=["stem7x7s2", "1x1s1", "3x3s1", "3x3s2", "1x1s2"])
def test_conv_primitives_match_fp64(dev, geom):
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, H, C, K, R, st, pad = geom
    g = torch.Generator().manual_seed(sum(geom))
    x = torch.randn(n, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, R, R, generator=g, dtype=torch.float64) * (2.0 / (C * R * R)) ** 0.5
    x.requires_grad_(True)
    w.requires_grad_(True)
    y = F.conv2d(x, w, stride=st, padding=pad)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * gy).sum().backward()
    Ho = y.shape[2]
    L = G.lib()
    xd, wd, gyd = _nhwc(x.detach()).float().to(dev), w.detach().float().to(dev), _nhwc(gy).float().to(dev)
    yd = torch.empty(n, Ho, Ho, K, device=dev)
    gxd = torch.empty(n, H, H, C, device=dev)
    gwd = torch.empty(K, C, R, R, device=dev)
    nb = L.apg_conv_bwd_workspace_bytes(n, H, H, C, K, R, R, st, pad)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    s = N.stream_ptr(dev)
    G.check(L.apg_conv_fwd(N.dptr(xd), n, H, H, C, N.dptr(wd), K, R, R, st, pad, N.dptr(yd), s), "apg_conv_fwd")
    G.check(L.apg_conv_bwd(N.dptr(xd), n, H, H, C, N.dptr(wd), K, R, R, st, pad, N.dptr(gyd), N.dptr(gxd), N.dptr(gwd),
                           ws.data_ptr(), nb, s), "apg_conv_bwd")
    gw_only = torch.empty_like(gwd)                                  # each output on its own
    G.check(L.apg_conv_bwd(N.dptr(xd), n, H, H, C, None, K, R, R, st, pad, N.dptr(gyd), None, N.dptr(gw_only), ws.data_ptr(), nb, s),
            "apg_conv_bwd")
    torch.cuda.synchronize()
    errs = {"y": rel_err(yd.cpu().numpy(), _nhwc(y.detach()).numpy()),
            "gx": rel_err(gxd.cpu().numpy(), _nhwc(x.grad).numpy()),
            "gw": rel_err(gwd.cpu().numpy(), w.grad.numpy())}
    print(geom, errs)
    assert all(e <= 1e-5 for e in errs.values()), errs
    assert torch.equal(gw_only, gwd)


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, True)], ids=["plain", "relu", "res+relu"])
def test_batchnorm_primitives_match_fp64(dev, train, res, relu):
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, H, C = 4, 20, 96                                              # 1600 rows: several partial tiles; 96: a partial channel block
    g = torch.Generator().manual_seed(11 + train + 2 * res + 4 * relu)
    x = (torch.randn(n, C, H, H, generator=g, dtype=torch.float64) * 3 + 5).requires_grad_(True)   # offset: cancellation-prone
    gam = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    bet = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    r = torch.randn(n, C, H, H, generator=g, dtype=torch.float64).requires_grad_(True)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rm64, rv64 = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm64, rv64, gam, bet, bool(train), MOM, EPS)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * gy).sum().backward()
    M = n * H * H
    f = lambda t: _nhwc(t.detach()).float().to(dev).reshape(M, C)
    xd, rd, gyd = f(x), f(r), f(gy)
    gd, bd, rmd, rvd = (t.detach().float().to(dev) for t in (gam, bet, rm, rv))
    yd, mean, invstd = torch.empty(M, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    L = G.lib()
    nb = L.apg_bn_workspace_bytes(M, C)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    s = N.stream_ptr(dev)
    G.check(L.apg_bn_fwd(N.dptr(xd), M, C, N.dptr(gd), N.dptr(bd), N.dptr(rmd), N.dptr(rvd), train, MOM, EPS,
                         N.dptr(rd) if res else None, int(relu), N.dptr(yd), N.dptr(mean), N.dptr(invstd), ws.data_ptr(), nb, s),
            "apg_bn_fwd")
    gx, gres, gg, gb = torch.empty(M, C, device=dev), torch.empty(M, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    G.check(L.apg_bn_bwd(N.dptr(gyd), N.dptr(yd) if relu else None, N.dptr(xd), M, C, N.dptr(gd), N.dptr(mean), N.dptr(invstd), train,
                         N.dptr(gx), N.dptr(gres), N.dptr(gg), N.dptr(gb), ws.data_ptr(), nb, s), "apg_bn_bwd")
    torch.cuda.synchronize()
    errs = {"y": rel_err(yd.cpu().numpy(), f(y).cpu().numpy()), "gx": rel_err(gx.cpu().numpy(), f(x.grad).cpu().numpy()),
            "ggamma": rel_err(gg.cpu().numpy(), gam.grad.numpy()), "gbeta": rel_err(gb.cpu().numpy(), bet.grad.numpy()),
            "running_mean": rel_err(rmd.cpu().numpy(), rm64.numpy()), "running_var": rel_err(rvd.cpu().numpy(), rv64.numpy())}
    if res:
        errs["gres"] = rel_err(gres.cpu().numpy(), f(r.grad).cpu().numpy())
    print(train, res, relu, errs)
    assert all(e <= 1e-5 for e in errs.values()), errs
    if not train:
        assert torch.equal(rmd.cpu(), rm.float()) and torch.equal(rvd.cpu(), rv.float())


def test_pools_match_torch_with_exact_ties(dev):
    from airpose_amd import _native as N
    from airpose_amd import _native_grad as G
    n, H, C = 2, 17, 64
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randint(-2, 3, (n, C, H, H), generator=g).double()).requires_grad_(True)    # ~60 % zeros: all-tie windows
    y = F.max_pool2d(x, 3, 2, 1)
    gy = torch.randint(-4, 5, y.shape, generator=g).double()                                            # integer sums are exact
    (y * gy).sum().backward()
    Ho = y.shape[2]
    L = G.lib()
    s = N.stream_ptr(dev)
    xd, gyd = _nhwc(x.detach()).float().to(dev), _nhwc(gy).float().to(dev)
    yd, gxd = torch.empty(n, Ho, Ho, C, device=dev), torch.empty(n, H, H, C, device=dev)
    G.check(L.apg_maxpool_fwd(N.dptr(xd), n, H, H, C, N.dptr(yd), s), "apg_maxpool_fwd")
    G.check(L.apg_maxpool_bwd(N.dptr(xd), n, H, H, C, N.dptr(gyd), N.dptr(gxd), s), "apg_maxpool_bwd")
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), _nhwc(y.detach()).float())
    assert torch.equal(gxd.cpu(), _nhwc(x.grad).float())
    # avg-pool 7 x 7
    a = torch.randn(n, 256, 7, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    ya = F.avg_pool2d(a, 7, stride=1).flatten(1)
    ga = torch.randn(ya.shape, generator=g, dtype=torch.float64)
    (ya * ga).sum().backward()
    ad, gad = _nhwc(a.detach()).float().to(dev), ga.float().to(dev)
    yad, gxa = torch.empty(n, 256, device=dev), torch.empty(n, 7, 7, 256, device=dev)
    G.check(L.apg_avgpool_fwd(N.dptr(ad), n, 256, N.dptr(yad), s), "apg_avgpool_fwd")
    G.check(L.apg_avgpool_bwd(N.dptr(gad), n, 256, N.dptr(gxa), s), "apg_avgpool_bwd")
    torch.cuda.synchronize()
    assert rel_err(yad.cpu().numpy(), ya.detach().numpy()) <= 1e-6
    assert rel_err(gxa.cpu().numpy(), _nhwc(a.grad).numpy()) <= 1e-6


# ------------------------------------------------------------------------------------------------ 2. / 3. the whole trunk
# n = 1: every layer4 GEMM and BatchNorm below one tile (M = 49); n = 6: the stem's BatchNorm in the capped-tile regime (M = 75 264
# rows > 65 536: 296-row tiles, 255 of them, the last ragged) and layer1's above 64 tiles
@pytest.mark.parametrize("train,n", [pytest.param(True, 4, id="train"), pytest.param(False, 4, id="eval"),
                                     pytest.param(True, 1, id="train-n1"), pytest.param(True, 6, id="train-n6")])
def test_whole_trunk_matches_fp64(copenet_sd, dev, monkeypatch, train, n):
    from oracle import copenet_ref
    net = _net(copenet_sd, dev).train(train)
    _, bns = _trunk_keys(net)
    x = _images(n, 21)
    Wt = torch.randn(n, 2048, generator=torch.Generator().manual_seed(22))
    before = {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    xf64, sd64, x64 = _ref_trunk(monkeypatch, net, x.double(), Wt, torch.float64, train, True)
    runs32 = [_ref_trunk(monkeypatch, net, x.float(), Wt, torch.float32, train, True, cl) for cl in (False, True)]
    xg = x.to(dev).requires_grad_(True)
    xf = net.forward_feat_ext(xg)
    assert xf.grad_fn is not None
    (xf * Wt.to(dev)).sum().backward()
    e = rel_err(xf.detach().cpu().numpy(), xf64.numpy())
    print("xf rel err %.3e" % e)
    assert e <= 1e-4
    if not train:                                                      # the unpatched oracle: eval-mode BatchNorm
        with torch.no_grad():
            ref = copenet_ref.forward_feat_ext(x.double(), {k: v.detach().cpu().double() for k, v in copenet_sd.items()
                                                            if v.is_floating_point()})
        assert rel_err(xf.detach().cpu().numpy(), ref.numpy()) <= 1e-4
    # eval mode: nothing re-centres the activations, and this batch's layer4 pre-ReLU maps hold values within 1e-7 .. 1e-6 of
    # zero relative to their maximum -- inside fp32's accumulated forward error, so whether a ReLU mask entry flips against fp64
    # is chance for any fp32 order: flips in layer4.1 moved its conv1 / bn1 / bn3 gradients by 5e-5 / 1.2e-4 / 6.5e-4 while every
    # tensor before them stayed under 1e-4.  The floor is 1e-3 there; the layer primitives hold 1e-5 in eval mode on their own.
    _check_trunk_grads(net, xg, sd64, x64, [r[1] for r in runs32], [r[2] for r in runs32], "trunk train=%s n=%d" % (train, n),
                       1e-5 if train else 1e-3)
    after = net.state_dict()
    for p in bns:
        if train:
            for b in ("running_mean", "running_var"):
                k = p + "." + b
                e = rel_err(after[k].cpu().numpy(), sd64[k].numpy())
                # n = 1: a layer4 statistic over 49 rows averages away little of the fp32 error that the 50 layers before it
                # carry, and a correct fp32 evaluation misses 1e-5 there: torch's own fp32 CPU restatements of this batch land at
                # 1.0e-5 (NCHW) and 1.3e-5 (the worse of the two) on layer4.2.bn1.running_var, this kernel at 1.1e-5, while the
                # BatchNorm primitive at M = 49 holds 1e-7 on its own (test_trunk_grad_shapes.py).  At n = 1 the bar is therefore
                # the gradients' rule, max(4 x fp32-CPU, 1e-5) (5.3e-5 on that buffer); at n = 4 and 6 the fixed 1e-5 holds.
                bar = 1e-5 if n > 1 else max(1e-5, 4 * max(rel_err(r[1][k].detach().numpy(), sd64[k].numpy()) for r in runs32))
                if e > 1e-5:
                    print("%s: %.3e against the bar %.3e" % (k, e, bar))
                assert e <= bar, (p, b, e, bar)
            assert int(after[p + ".num_batches_tracked"]) == int(before[p + ".num_batches_tracked"]) + 1
        else:
            for b in ("running_mean", "running_var", "num_batches_tracked"):
                assert torch.equal(after[p + "." + b], before[p + "." + b]), (p, b)


# ------------------------------------------------------------------------------------------------ 4. copenet.forward, train mode
def _pair_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"x0": torch.randn(B, 3, 224, 224, generator=g), "x1": torch.randn(B, 3, 224, 224, generator=g)}
    for v in "01":
        d["bb" + v] = torch.rand(B, 3, generator=g) + 0.2
        d["pos" + v] = torch.randn(B, 3, generator=g) * 0.3 + torch.tensor([0., 0., 10.])
    return d


def _fwd_args(d, dev=None, dtype=None):
    f = (lambda t: t.to(dev)) if dev is not None else (lambda t: t.to(dtype))
    return [f(d[k]) for k in ("x0", "x1", "bb0", "bb1", "pos0", "pos1")]


HEAD = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "decpose.weight", "decpose.bias", "decshape.weight", "decshape.bias")


def test_forward_train_mode_per_view_statistics_match_fp64(copenet_sd, dev, monkeypatch):
    from oracle import copenet_ref
    B = 2
    net = _net(copenet_sd, dev).train()
    net.drop1.eval()
    net.drop2.eval()
    keys, bns = _trunk_keys(net)
    d = _pair_inputs(B, 31)
    g = torch.Generator().manual_seed(32)
    Wl = [torch.randn(B, 135, generator=g), torch.randn(B, 10, generator=g), torch.randn(B, 135, generator=g),
          torch.randn(B, 10, generator=g)]
    ref = {}
    for dt, cl in ((torch.float64, False), (torch.float32, False), (torch.float32, True)):
        sd, bn = _restate(net, dt, True, keys, HEAD)
        monkeypatch.setattr(copenet_ref, "_bn", bn)
        a = _fwd_args(d, dtype=dt)
        outs = copenet_ref.copenet_forward(sd, _cl(a[0], cl), _cl(a[1], cl), *a[2:])   # view 0's trunk, then view 1's
        sum((o * w.to(dt)).sum() for o, w in zip(outs, Wl)).backward()
        monkeypatch.undo()
        ref[dt, cl] = (outs, sd)
    outs = net(*_fwd_args(d, dev))
    sum((o * w.to(dev)).sum() for o, w in zip(outs, Wl)).backward()
    outs64, sd64 = ref[torch.float64, False]
    sd32s = [ref[torch.float32, False][1], ref[torch.float32, True][1]]
    for a, b in zip(outs, outs64):
        a, b = a.detach().cpu().numpy(), b.detach().numpy()
        errs = pose_rel_errs(a, b) if a.shape[1] == 135 else {"betas": rel_err(a, b)}
        assert all(e <= 1e-4 for e in errs.values()), errs
    _check_trunk_grads(net, None, sd64, None, sd32s, None, "forward")
    params = dict(net.named_parameters())
    for k in HEAD:
        e = rel_err(params[k].grad.cpu().numpy(), sd64[k].grad.numpy())
        bar = _bar(sd64[k], [sd[k] for sd in sd32s])
        assert e <= bar, (k, e, bar)
    after = net.state_dict()
    for p in bns:
        for b in ("running_mean", "running_var"):
            e = rel_err(after[p + "." + b].cpu().numpy(), sd64[p + "." + b].numpy())
            assert e <= 1e-5, (p, b, e)
        assert int(after[p + ".num_batches_tracked"]) == int(copenet_sd[p + ".num_batches_tracked"]) + 2


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_steps_are_bit_reproducible(copenet_sd, dev):
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


# ------------------------------------------------------------------------------------------------ 6. the reference's training step
def test_reference_training_step_with_adam_then_eval_repacks(copenet_sd, smplx_model, dev):
    from airpose_amd import geometry, smplx, utils
    from test_head_grad import _caller_loss
    B = 2
    net = _net(copenet_sd, dev)
    body = smplx.SMPLX(model_data=smplx_model)
    d = _pair_inputs(B, 51)
    g = torch.Generator().manual_seed(52)
    tgt = {"j2d": torch.randn(B, 22, 2, generator=g) * 100 + 500, "j3d": torch.randn(B, 22, 3, generator=g),
           "rot": torch.eye(3).expand(B, 21, 3, 3), "root": torch.eye(3).expand(B, 1, 3, 3),
           "trans": torch.randn(B, 3, generator=g) + torch.tensor([0., 0., 200.]),
           "cc0": torch.full((1, B, 2), 500.), "cc1": torch.full((1, B, 2), 520.)}
    eye = torch.eye(3, device=dev).expand(B, 1, 3, 3)
    mods = (geometry.rot6d_to_rotmat,
            lambda be, bp: (lambda o: (o.vertices, o.joints))(body.forward(betas=be, body_pose=bp, global_orient=eye,
                                                                            transl=torch.zeros(B, 3, device=dev), pose2rot=False)),
            lambda M, v, j: utils.transform_smpl(M, v, j)[:2],
            lambda j, cc: geometry.perspective_projection(j, None, None, (5000., 5000.), cc.to(dev)))
    args = _fwd_args(d, dev)
    with torch.no_grad():
        net(*args)                                                   # the inference handle now holds the initial weights
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, amsgrad=True)
    losses = []
    for it in range(5):
        opt.zero_grad()
        torch.manual_seed(100 + it)
        pos0, pos1 = args[4].clone(), args[5].clone()
        p0, b0, p1, b1 = net(args[0], args[1], args[2], args[3], pos0, pos1)
        loss = _caller_loss(mods, p0, b0, p1, b1, pos0, pos1, tgt, torch.float32)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("training-step losses", ["%.4e" % v for v in losses])
    assert losses[-1] < losses[0], losses
    assert net.conv1.weight.grad is not None and net.layer4[2].bn3.weight.grad is not None
    net.eval()
    with torch.no_grad():
        got = net(*args)
        fresh = _net(net.state_dict(), dev, trainable=False)
        want = fresh(*args)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(net.forward_feat_ext(args[0]), fresh.forward_feat_ext(args[0]))


def test_running_stat_writes_are_seen_by_the_inference_handle(copenet_sd, dev):
    net = _net(copenet_sd, dev)
    x = _images(2, 61).to(dev)
    with torch.no_grad():
        net.forward_feat_ext(x)                                      # packs the handle
        sig = net._signature()
        v = net.bn1.running_mean._version
        net.train()
        net.forward_feat_ext(x)                                      # train mode, no graph: running statistics only
        assert net.bn1.running_mean._version > v and net._signature() != sig
        net.eval()
        got = net.forward_feat_ext(x)
        want = _net(net.state_dict(), dev, trainable=False).forward_feat_ext(x)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 7. unchanged behaviour
def test_switch_on_eval_no_grad_is_the_inference_path(copenet_sd, dev):
    on, off = _net(copenet_sd, dev), _net(copenet_sd, dev, trainable=False)
    args = _fwd_args(_pair_inputs(2, 71), dev)
    with torch.no_grad():
        a, b = on(*args), off(*args)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(on.forward_feat_ext(args[0]), off.forward_feat_ext(args[0]))
    assert int(on.bn1.num_batches_tracked) == int(copenet_sd["bn1.num_batches_tracked"])


def test_switch_off_train_mode_still_raises(copenet_sd, dev):
    net = _net(copenet_sd, dev, trainable=False).train()
    x = torch.zeros(1, 3, 224, 224, device=dev)
    z = torch.zeros(1, 3, device=dev)
    with pytest.raises(RuntimeError, match="inference path only"):
        net(x, x, z, z, z, z)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.forward_feat_ext(x)
    net.set_trunk_trainable(True).set_trunk_trainable(False)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.forward_feat_ext(x)


def test_errors_are_named(copenet_sd, dev):
    from airpose_amd import hmr_model
    net = _net(copenet_sd, dev).train()
    x = _images(1, 81).to(dev)
    xf = net.forward_feat_ext(x.clone().requires_grad_(True))
    g, = torch.autograd.grad(xf.sum(), net.conv1.weight, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()                                           # first derivatives only
    net.layer2[1].bn2.momentum = None
    with pytest.raises(RuntimeError, match="momentum=None"):
        net.forward_feat_ext(x)
    net.layer2[1].bn2.momentum = 0.2
    with pytest.raises(RuntimeError, match="one momentum"):
        net.forward_feat_ext(x)
    cpu_net = _net(copenet_sd, torch.device("cpu")).train()
    with pytest.raises(RuntimeError, match=r"net\.to\(dev\)"):
        cpu_net.forward_feat_ext(x)
    with pytest.raises(RuntimeError, match="CUDA"):
        _net(copenet_sd, dev).train().forward_feat_ext(x.cpu())
    with pytest.raises(RuntimeError, match="two-view"):
        hmr_model.getcopenet(MEAN_PARAMS).set_trunk_trainable(True)


# ------------------------------------------------------------------------------------------------ 8. no torch compute on the path
def test_trunk_path_calls_no_torch_conv_bn_or_pool(copenet_sd, dev, monkeypatch):
    net = _net(copenet_sd, dev).train()
    x = _images(2, 91).to(dev).requires_grad_(True)

    def boom(*a, **k):
        raise AssertionError("torch compute on the trainable trunk")
    for mod, name in ((F, "conv2d"), (torch, "conv2d"), (F, "batch_norm"), (torch, "batch_norm"), (F, "max_pool2d"),
                      (F, "avg_pool2d")):
        monkeypatch.setattr(mod, name, boom)
    xf = net.forward_feat_ext(x)
    xf.square().sum().backward()
    assert x.grad is not None and net.conv1.weight.grad is not None and net.layer1[0].downsample[1].bias.grad is not None
    assert np.isfinite(xf.detach().cpu().numpy()).all()
