"""Trainable view-local and baseline heads behind net.set_trainable(True) (head_local_grad.py on apg_head_local_fwd / _bwd):
copenet.regressor_step against the merged two-view head bit for bit, copenet_sep / hmr / muhmr / copenet_singleview against fp64
autograd through the oracle (oracle/copenet_ref.py) or, with dropout, an fp64 restatement that applies the masks of
apg_dropout_mask; one end-to-end step with a trainable trunk, a train_reg_only fine-tune of copenet_sep, and unchanged behaviour
with the switch off.  Bars: rel_err <= 1e-5 on outputs, <= 1e-4 on gradients (tests/test_head_grad.py)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, rel_err

TOL_OUT, TOL_GRAD = 1e-5, 1e-4
pytestmark = pytest.mark.gpu
HEAD2 = ("fc1", "fc2", "decpose", "decshape")
HEAD3 = HEAD2 + ("deccam",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sds():
    from airpose_amd import weights as W
    sd = {v: W.to_torch(W.copenet_state_dict(20240901 + i, MEAN_PARAMS, variant=v)) for i, v in
          enumerate(("copenet", "hmr", "singleview", "muhmr"))}
    sd["copenet_b"] = W.to_torch(W.copenet_state_dict(777, MEAN_PARAMS, variant="copenet"))
    return sd


def _net(variant, sd, dev, on=True, trunk=None):
    from airpose_amd import copenet_model, copenet_singleview_model, hmr_model, muhmr_model
    mod = {"copenet": copenet_model, "hmr": hmr_model, "singleview": copenet_singleview_model, "muhmr": muhmr_model}[variant]
    net = mod.getcopenet(MEAN_PARAMS, precision="fp32")
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    return net.set_trainable(True, trunk=trunk) if on else net


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
        d["orient" + v] = torch.randn(B, 6, generator=g)
        d["art" + v] = torch.randn(B, 126, generator=g)
        d["shape" + v] = torch.randn(B, 10, generator=g) * 0.5
    return d


ORDER = ("xf0", "xf1", "bb0", "bb1", "pos0", "pos1", "orient0", "orient1", "art0", "art1", "shape0", "shape1")


def _weights(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in shapes]


def _wloss(outs, W):
    return sum((o * w.to(o)).sum() for o, w in zip(outs, W))


def _sd64(net, names):
    return {k: v.detach().cpu().double().requires_grad_(k.split(".")[0] in names) for k, v in net.state_dict().items()}


def _cmp(got, want, tol, what):
    """one rel_err per semantic slice: a (.., 135) pose holds a translation (z ~ 10) in front of the 6-D rotations"""
    got, want = got.detach().cpu().numpy(), want.detach().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    parts = [(got[..., :3], want[..., :3]), (got[..., 3:], want[..., 3:])] if got.shape[-1] == 135 and got.ndim == 2 else [(got, want)]
    for a, b in parts:
        e = rel_err(a, b)
        print("%-40s rel err %.3e" % (what, e))
        assert e < tol, (what, e)


def _check_param_grads(net, sd64, names, what, prefix=""):
    for m in names:
        for attr in ("weight", "bias"):
            got = getattr(getattr(net, m), attr).grad
            assert got is not None, (what, m, attr)
            _cmp(got, sd64["%s.%s" % (m, attr)].grad, TOL_GRAD, "%s grad %s%s.%s" % (what, prefix, m, attr))
    assert net.conv1.weight.grad is None


def _check_leaf_grads(leaves, l64, what):
    for k, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape, (what, k)
        _cmp(t.grad, l64[k].grad, TOL_GRAD, "%s grad %s" % (what, k))


# ------------------------------------------------------------------------------------------------ 1. the merged head, bit for bit
@pytest.mark.parametrize("view", [0, 1])
def test_regressor_step_equals_the_two_view_head_bitwise(sds, dev, view):
    B = 5
    net = _net("copenet", sds["copenet"], dev)
    d = _two_view_inputs(B, 100)
    W = _weights([(B, 135), (B, 10)], 7)
    v, o = str(view), str(1 - view)
    # the two-view path, loss on this view alone
    lv = {k: t.to(dev).requires_grad_(True) for k, t in d.items()}
    outs = net.forward_reg(*[lv[k] for k in ORDER])
    _wloss(outs[2 * view:2 * view + 2], W).backward()
    gpar2 = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    net.zero_grad(set_to_none=True)
    # the view-local step with the partner's state supplied
    xf, bb = d["xf" + v].to(dev).requires_grad_(True), d["bb" + v].to(dev).requires_grad_(True)
    pose = torch.cat([d["pos" + v], d["orient" + v], d["art" + v]], 1).to(dev).requires_grad_(True)
    betas = d["shape" + v].to(dev).requires_grad_(True)
    partner = torch.cat([d["art" + o], d["shape" + o]], 1).to(dev).requires_grad_(True)
    p, b = net.regressor_step(xf, bb, pose, betas, partner)
    assert p.grad_fn is not None and b.grad_fn is not None
    assert torch.equal(p, outs[2 * view]) and torch.equal(b, outs[2 * view + 1])
    _wloss((p, b), W).backward()
    assert torch.equal(xf.grad, lv["xf" + v].grad) and torch.equal(bb.grad, lv["bb" + v].grad)
    assert torch.equal(pose.grad, torch.cat([lv["pos" + v].grad, lv["orient" + v].grad, lv["art" + v].grad], 1))
    assert torch.equal(betas.grad, lv["shape" + v].grad)
    # the partner's gradient is what the two-view path adds into the other view's art / shape
    assert torch.equal(partner.grad, torch.cat([lv["art" + o].grad, lv["shape" + o].grad], 1))
    for k in ("decpose.bias", "decshape.bias"):               # column sums over the rows with a gradient: the same rows, the same order
        if view == 0:
            assert torch.equal(dict(net.named_parameters())[k].grad, gpar2[k]), k
    with torch.no_grad():                                     # and the inference kernel agrees (1e-4: test_head_grad's bar between the paths)
        pi, bi = net.regressor_step(xf, bb, pose, betas, partner)
    assert pi.grad_fn is None
    _cmp(p, pi.cpu().double(), 1e-4, "step vs inference pose")
    _cmp(b, bi.cpu().double(), 1e-4, "step vs inference betas")


def test_train_mode_view0_rows_equal_the_two_view_call_with_the_same_seed(sds, dev):
    from airpose_amd import head_grad
    B = 5
    net = _net("copenet", sds["copenet"], dev).train()
    d = {k: t.to(dev) for k, t in _two_view_inputs(B, 101).items()}
    seed = 123456789
    outs = head_grad.forward_reg(net, *[d[k] for k in ORDER], seed=seed)
    pose = torch.cat([d["pos0"], d["orient0"], d["art0"]], 1)
    p, b = net.regressor_step(d["xf0"], d["bb0"], pose, d["shape0"], torch.cat([d["art1"], d["shape1"]], 1), seed=seed)
    assert net.last_dropout_seed == seed
    assert torch.equal(p, outs[0]) and torch.equal(b, outs[1])             # rows [0, B) share their index: the same masks
    p2, _ = net.regressor_step(d["xf0"], d["bb0"], pose, d["shape0"], torch.cat([d["art1"], d["shape1"]], 1))
    assert net.last_dropout_seed != seed and not torch.equal(p2, p)        # a fresh seed per call


# ------------------------------------------------------------------------------------------------ 2. copenet_sep
def _sep_param_check(sep, sd0, sd1, what):
    _check_param_grads(sep.copenet0, sd0, HEAD2, what, "copenet0.")
    _check_param_grads(sep.copenet1, sd1, HEAD2, what, "copenet1.")


@pytest.mark.parametrize("B", [1, 5])
def test_sep_forward_reg_matches_oracle(sds, dev, B):
    from oracle import copenet_ref
    sep = _sep(sds, dev)
    d = _two_view_inputs(B, 200 + B)
    W = _weights([(B, 135), (B, 10), (B, 135), (B, 10)], 8)
    lv = {k: t.to(dev).requires_grad_(True) for k, t in d.items()}
    outs = sep.forward_reg(*[lv[k] for k in ORDER])
    assert all(o.grad_fn is not None for o in outs)
    _wloss(outs, W).backward()
    sd0, sd1 = _sd64(sep.copenet0, HEAD2), _sd64(sep.copenet1, HEAD2)
    l64 = {k: t.double().requires_grad_(True) for k, t in d.items()}
    want = copenet_ref.sep_forward_reg(sd0, sd1, *[l64[k] for k in ORDER])
    for i, (a, b) in enumerate(zip(outs, want)):
        _cmp(a, b, TOL_OUT, "sep reg B=%d out%d" % (B, i))
    _wloss(want, [w.double() for w in W]).backward()
    _sep_param_check(sep, sd0, sd1, "sep reg B=%d" % B)
    _check_leaf_grads(lv, l64, "sep reg B=%d" % B)


@pytest.mark.parametrize("B", [1, 5])
def test_sep_forward_ief_matches_oracle(sds, dev, B):
    from oracle import copenet_ref
    sep = _sep(sds, dev)
    d = _two_view_inputs(B, 210 + B)
    W = _weights([(B, 135), (B, 10), (B, 135), (B, 10)], 9)
    names = ("xf0", "xf1", "bb0", "bb1", "pos0", "pos1")
    lv = {k: d[k].to(dev).requires_grad_(True) for k in names}
    outs = sep.forward_ief(*[lv[k] for k in names], iters=3)
    _wloss(outs, W).backward()
    sd0, sd1 = _sd64(sep.copenet0, HEAD2), _sd64(sep.copenet1, HEAD2)
    l64 = {k: d[k].double().requires_grad_(True) for k in names}
    want = copenet_ref.sep_ief(sd0, sd1, *[l64[k] for k in names], iters=3)
    for i, (a, b) in enumerate(zip(outs, want)):
        _cmp(a, b, TOL_OUT, "sep ief B=%d out%d" % (B, i))
    _wloss(want, [w.double() for w in W]).backward()
    _sep_param_check(sep, sd0, sd1, "sep ief B=%d" % B)
    _check_leaf_grads(lv, l64, "sep ief B=%d" % B)


def test_sep_loss_on_view1_reaches_copenet0_through_the_partner(sds, dev):
    from oracle import copenet_ref
    B = 5
    sep = _sep(sds, dev)
    d = _two_view_inputs(B, 220)
    W = _weights([(B, 135), (B, 10)], 10)
    outs = sep.forward_reg(*[d[k].to(dev) for k in ORDER])
    _wloss(outs[2:], W).backward()
    sd0, sd1 = _sd64(sep.copenet0, HEAD2), _sd64(sep.copenet1, HEAD2)
    want = copenet_ref.sep_forward_reg(sd0, sd1, *[d[k].double() for k in ORDER])
    _wloss(want[2:], [w.double() for w in W]).backward()
    for k in ("decshape.weight", "decshape.bias", "fc1.weight", "fc1.bias", "fc2.weight"):
        m, a = k.split(".")
        got = getattr(getattr(sep.copenet0, m), a).grad
        assert got is not None and float(got.abs().max()) > 0, k
        _cmp(got, sd0[k].grad, TOL_GRAD, "view-1 loss, copenet0." + k)
    # view 1 reads view 0's OLD articulated pose: decpose of copenet0 gets exactly nothing
    assert sep.copenet0.decpose.weight.grad is None or float(sep.copenet0.decpose.weight.grad.abs().max()) == 0.0
    assert float(sd0["decpose.weight"].grad.abs().max() if sd0["decpose.weight"].grad is not None else 0.0) == 0.0
    _check_param_grads(sep.copenet1, sd1, HEAD2, "view-1 loss", "copenet1.")


# ------------------------------------------------------------------------------------------------ 3. hmr / muhmr / single-view
def _masks(net, seed, R, dev):
    from airpose_amd import _native_grad as G
    return [G.dropout_mask(seed, layer, R, 1024, drop.p, dev).cpu().double() / (1.0 - drop.p) if drop.training else None
            for layer, drop in ((1, net.drop1), (2, net.drop2))]


def _restate(sd, xc, residuals, decs, masks=None):
    """fp64 restatement of one head evaluation on the rows of xc with explicit (already scaled) dropout masks"""
    lin = lambda x, p: F.linear(x, sd[p + ".weight"], sd[p + ".bias"])
    h = lin(xc, "fc1")
    if masks is not None and masks[0] is not None:
        h = h * masks[0]
    h = lin(h, "fc2")
    if masks is not None and masks[1] is not None:
        h = h * masks[1]
    return [lin(h, dname) + r for dname, r in zip(decs, residuals)]


def _baseline_case(variant, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    if variant == "hmr":
        return {"xf": torch.relu(r(B, 2048)), "pose": r(B, 132), "shape": r(B, 10) * 0.5, "cam": r(B, 3)}
    if variant == "singleview":
        return {"xf": torch.relu(r(B, 2048)), "bb": torch.rand(B, 3, generator=g) + 0.2,
                "pose": torch.cat([r(B, 3) * 0.3 + torch.tensor([0., 0., 10.]), r(B, 132)], 1), "shape": r(B, 10) * 0.5}
    d = {}
    for v in "01":
        d.update({"xf" + v: torch.relu(r(B, 2048)), "orient" + v: r(B, 6), "art" + v: r(B, 126), "shape" + v: r(B, 10) * 0.5,
                  "cam" + v: r(B, 3)})
    return d


def _baseline_call(variant, net, L):
    if variant == "hmr":
        return net.forward_reg(L["xf"], L["pose"], L["shape"], L["cam"])
    if variant == "singleview":
        return net.forward_reg(L["xf"], L["bb"], L["pose"], L["shape"])
    return net.forward_reg(L["xf0"], L["xf1"], L["orient0"], L["orient1"], L["art0"], L["art1"], L["shape0"], L["shape1"],
                           L["cam0"], L["cam1"])


def _baseline_ref(variant, sd, L, masks=None):
    """the reference's forward_reg in fp64; muhmr: rows view 0 then view 1, as the kernels number them"""
    from oracle import copenet_ref
    if variant == "hmr":
        out = _restate(sd, torch.cat([L["xf"], L["pose"], L["shape"], L["cam"]], 1), (L["pose"], L["shape"], L["cam"]), HEAD3[2:], masks)
        if masks is None:                                    # the oracle's own statement
            for a, b in zip(out, copenet_ref.hmr_forward_reg(sd, L["xf"], L["pose"], L["shape"], L["cam"])):
                assert torch.equal(a, b)
        return out
    if variant == "singleview":                              # oracle singleview_forward's loop body
        return _restate(sd, torch.cat([L["xf"], L["bb"], L["pose"], L["shape"]], 1), (L["pose"], L["shape"]), HEAD2[2:], masks)
    B = L["xf0"].shape[0]                                    # oracle muhmr_forward's loop body
    pose = [torch.cat([L["orient" + v], L["art" + v]], 1) for v in "01"]
    xc = torch.cat([torch.cat([L["xf%d" % v], L["cam%d" % v], pose[v], L["shape%d" % v], pose[1 - v][:, 6:], L["shape%d" % (1 - v)]], 1)
                    for v in (0, 1)], 0)
    p, s, c = _restate(sd, xc, (torch.cat(pose, 0), torch.cat([L["shape0"], L["shape1"]], 0), torch.cat([L["cam0"], L["cam1"]], 0)),
                       HEAD3[2:], masks)
    return p[:B], s[:B], c[:B], p[B:], s[B:], c[B:]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("variant", ["hmr", "muhmr", "singleview"])
def test_baseline_forward_reg_matches_fp64(sds, dev, variant, B, train):
    net = _net(variant, sds[variant], dev)
    names = HEAD2 if variant == "singleview" else HEAD3
    if train:
        net.train()
    d = _baseline_case(variant, B, 300 + B)
    lv = {k: t.to(dev).requires_grad_(True) for k, t in d.items()}
    outs = _baseline_call(variant, net, lv)
    assert all(o.grad_fn is not None for o in outs)
    W = _weights([tuple(o.shape) for o in outs], 11)
    _wloss(outs, W).backward()
    R = 2 * B if variant == "muhmr" else B
    masks = _masks(net, net.last_dropout_seed, R, dev) if train else None
    sd64 = _sd64(net, names)
    l64 = {k: t.double().requires_grad_(True) for k, t in d.items()}
    want = _baseline_ref(variant, sd64, l64, masks)
    what = "%s B=%d %s" % (variant, B, "train" if train else "eval")
    for i, (a, b) in enumerate(zip(outs, want)):
        _cmp(a, b, TOL_OUT, "%s out%d" % (what, i))
    _wloss(want, [w.double() for w in W]).backward()
    _check_param_grads(net, sd64, names, what)
    _check_leaf_grads(lv, l64, what)
    if variant == "singleview":
        assert not hasattr(net, "init_cam") and net.deccam.weight.grad is None


def test_hmr_forward_reg_through_rot6d_to_rotmat(sds, dev):
    from airpose_amd import geometry
    from oracle import geometry_ref
    B = 5
    net = _net("hmr", sds["hmr"], dev)
    d = _baseline_case("hmr", B, 320)
    lv = {k: t.to(dev).requires_grad_(True) for k, t in d.items()}
    pose, shape, cam = _baseline_call("hmr", net, lv)
    rot = geometry.rot6d_to_rotmat(pose).view(B, 22, 3, 3)
    W = _weights([(B, 22, 3, 3), (B, 10), (B, 3)], 12)
    _wloss((rot, shape, cam), W).backward()
    sd64 = _sd64(net, HEAD3)
    l64 = {k: t.double().requires_grad_(True) for k, t in d.items()}
    p64, s64, c64 = _baseline_ref("hmr", sd64, l64)
    r64 = geometry_ref.rot6d_to_rotmat(p64).view(B, 22, 3, 3)
    _cmp(rot, r64, TOL_OUT, "hmr rotmat")
    _wloss((r64, s64, c64), [w.double() for w in W]).backward()
    _check_param_grads(net, sd64, HEAD3, "hmr rotmat chain")
    _check_leaf_grads(lv, l64, "hmr rotmat chain")


# ------------------------------------------------------------------------------------------------ 4. one step with a trainable trunk
def test_hmr_end_to_end_step_with_a_trainable_trunk(sds, dev):
    from airpose_amd import weights as Wt
    n = 2
    x = torch.from_numpy(Wt.synthetic_inputs(55, n)["im0"]).to(dev)
    W = _weights([(n, 22, 3, 3), (n, 10), (n, 3)], 13)

    def step():
        net = _net("hmr", sds["hmr"], dev, trunk="fp32").train()
        before = net.bn1.running_mean.clone(), net.layer4[2].bn3.running_var.clone()
        torch.manual_seed(99)
        outs = net(x)
        assert tuple(outs[0].shape) == (n, 22, 3, 3) and all(o.grad_fn is not None for o in outs)
        _wloss(outs, W).backward()
        assert not torch.equal(net.bn1.running_mean, before[0]) and not torch.equal(net.layer4[2].bn3.running_var, before[1])
        assert int(net.bn1.num_batches_tracked) == 1
        return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, [o.detach() for o in outs], net

    g1, o1, net = step()
    for k in ("conv1.weight", "deccam.weight", "decpose.bias", "fc1.weight", "layer3.2.bn2.weight"):
        assert k in g1 and torch.isfinite(g1[k]).all() and float(g1[k].abs().max()) > 0, k
    g2, o2, _ = step()
    assert set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    # without a trunk precision the trunk stays the inference path
    net.set_trainable(True, trunk=None)
    with pytest.raises(RuntimeError, match="inference path only"):
        net(x)


# ------------------------------------------------------------------------------------------------ 5. train_reg_only fine-tune
def test_sep_train_reg_only_fine_tune_with_amsgrad(sds, dev):
    B = 8
    sep = _sep(sds, dev)
    d = {k: t.to(dev) for k, t in _two_view_inputs(B, 400).items()}
    args = [d[k] for k in ("xf0", "xf1", "bb0", "bb1", "pos0", "pos1")]    # trunks frozen: the features are the inputs
    tgt_net = _sep(sds, dev, on=False)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for c in (tgt_net.copenet0, tgt_net.copenet1):
            c.decpose.bias.add_(0.05 * torch.randn(135, generator=g).to(dev))
            c.decshape.bias.add_(0.05 * torch.randn(10, generator=g).to(dev))
        target = tgt_net.forward_ief(*args, iters=3)
    sep.train()
    for c in (sep.copenet0, sep.copenet1):                    # a fixed target and a monotone loss: no masks
        c.drop1.eval()
        c.drop2.eval()
    head = [p for c in (sep.copenet0, sep.copenet1) for m in HEAD2 for p in getattr(c, m).parameters()]
    head_ids = {id(p) for p in head}
    frozen = {k: p.detach().clone() for k, p in sep.named_parameters() if id(p) not in head_ids}
    frozen.update({"buf." + k: b.detach().clone() for k, b in sep.named_buffers()})
    start = [p.detach().clone() for p in head]
    # The learning rate is set so that 20 full-batch steps stay in the regime where descent is monotone.  Adam's first steps move
    # EVERY parameter by about lr (m / sqrt(v) ~ sign(g)), and the moves of one fc row add up coherently: a hidden unit shifts by up
    # to lr * |xc|_1 ~ lr * 1e3 per step (2048 relu(randn) features at mean 0.4, 284 O(1) state columns), the outputs by about as
    # much per layer.  The distance to the target is the 0.05 bias perturbation carried through three iterations, ~0.1.  A step of
    # about 1 % of that, lr * 1e3 <= 1e-3, gives lr = 1e-6; the reference's 5e-5 (copenet_twoview_sep.py:638) is for noisy
    # mini-batches over epochs and overshoots this noiseless 8-sample problem within a few steps.
    opt = torch.optim.Adam(head, lr=1e-6, weight_decay=0, amsgrad=True)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        out = sep.forward_ief(*args, iters=3)
        loss = sum(((o - t) ** 2).mean() for o, t in zip(out, target))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("sep fine-tune losses", ["%.3e" % x for x in losses])
    assert all(b < a for a, b in zip(losses[-11:-1], losses[-10:])), losses
    assert losses[-1] < losses[0]
    assert all(not torch.equal(a, p.detach()) for a, p in zip(start, head))
    now = dict(sep.named_parameters())
    bufs = dict(sep.named_buffers())
    for k, t in frozen.items():
        cur = bufs[k[4:]] if k.startswith("buf.") else now[k]
        assert torch.equal(t, cur.detach()), k
        assert k.startswith("buf.") or cur.grad is None, k


# ------------------------------------------------------------------------------------------------ 6. unchanged behaviour
def test_switch_off_raises_as_before(sds, dev):
    from airpose_amd import copenet_sep_model, hmr_model
    net = _net("copenet", sds["copenet"], dev, on=False).train()
    x = torch.zeros(1, 3, 224, 224, device=dev)
    z = torch.zeros(1, 3, device=dev)
    step_args = (torch.zeros(1, 2048, device=dev), z, torch.zeros(1, 135, device=dev), torch.zeros(1, 10, device=dev),
                 torch.zeros(1, 136, device=dev))
    with pytest.raises(RuntimeError, match="inference path only"):
        net(x, x, z, z, z, z)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.forward_feat_ext(x)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.regressor_step(*step_args)
    hmr = hmr_model.getcopenet(MEAN_PARAMS).to(dev).train()
    with pytest.raises(RuntimeError, match="inference path only"):
        hmr(x)
    with pytest.raises(RuntimeError, match="inference path only"):
        hmr.forward_reg(torch.zeros(1, 2048, device=dev), torch.zeros(1, 132, device=dev), torch.zeros(1, 10, device=dev), z)
    with pytest.raises(RuntimeError, match="two-view"):
        hmr.set_trunk_trainable(True)
    with pytest.raises(RuntimeError, match="two-view"):
        hmr.set_trainable(True, trunk="fp32").set_trunk_trainable(True)        # the variant check is not loosened
    sep = copenet_sep_model.getcopenet_sep(MEAN_PARAMS).to(dev).train()
    with pytest.raises(RuntimeError, match="inference path only"):
        sep.forward_ief(torch.zeros(1, 2048, device=dev), torch.zeros(1, 2048, device=dev), z, z, z, z)
    # switched on and off again: as before
    net.set_trainable(True).set_trainable(False)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.regressor_step(*step_args)
    with pytest.raises(RuntimeError, match="trunk"):
        net.set_trainable(True, trunk="fp16")
    assert "_trainable" not in net.state_dict() and len(net.state_dict()) == len(sds["copenet"])


def test_switch_on_eval_no_grad_keeps_the_inference_bits(sds, dev):
    B = 3
    d = {k: t.to(dev) for k, t in _two_view_inputs(B, 600).items()}
    pose = torch.cat([d["pos0"], d["orient0"], d["art0"]], 1)
    partner = torch.cat([d["art1"], d["shape1"]], 1)
    on, fresh = _net("copenet", sds["copenet"], dev), _net("copenet", sds["copenet"], dev, on=False)
    sep_on, sep_fresh = _sep(sds, dev), _sep(sds, dev, on=False)
    with torch.no_grad():
        pairs = [(on.regressor_step(d["xf0"], d["bb0"], pose, d["shape0"], partner),
                  fresh.regressor_step(d["xf0"], d["bb0"], pose, d["shape0"], partner)),
                 (sep_on.forward_ief(d["xf0"], d["xf1"], d["bb0"], d["bb1"], d["pos0"], d["pos1"]),
                  sep_fresh.forward_ief(d["xf0"], d["xf1"], d["bb0"], d["bb1"], d["pos0"], d["pos1"]))]
        for variant in ("hmr", "muhmr", "singleview"):
            c = {k: t.to(dev) for k, t in _baseline_case(variant, B, 610).items()}
            pairs.append((_baseline_call(variant, _net(variant, sds[variant], dev), c),
                          _baseline_call(variant, _net(variant, sds[variant], dev, on=False), c)))
    for a, b in pairs:
        for x, y in zip(a, b):
            assert x.grad_fn is None and torch.equal(x, y)


def test_local_grad_path_calls_no_torch_matmul(sds, dev, monkeypatch):
    sep = _sep(sds, dev).train()
    nets = {v: _net(v, sds[v], dev).train() for v in ("hmr", "muhmr", "singleview")}
    d = {k: t.to(dev).requires_grad_(True) for k, t in _two_view_inputs(4, 700).items()}
    cases = {v: {k: t.to(dev).requires_grad_(True) for k, t in _baseline_case(v, 4, 710).items()} for v in nets}

    def boom(*a, **k):
        raise AssertionError("torch matrix product on the head's training path")
    for mod, name in ((F, "linear"), (torch, "matmul"), (torch, "mm"), (torch, "addmm"), (torch, "bmm"),
                      (torch.Tensor, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "addmm"), (torch.Tensor, "bmm"),
                      (torch.Tensor, "__matmul__")):
        monkeypatch.setattr(mod, name, boom)
    outs = sep.forward_ief(d["xf0"], d["xf1"], d["bb0"], d["bb1"], d["pos0"], d["pos1"], iters=2)
    sum(o.sum() for o in outs).backward()
    assert sep.copenet0.fc1.weight.grad is not None and d["xf1"].grad is not None
    for v, net in nets.items():
        sum(o.sum() for o in _baseline_call(v, net, cases[v])).backward()
        assert net.fc1.weight.grad is not None and net.decshape.bias.grad is not None
