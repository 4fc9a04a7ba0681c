"""Trainable IEF regressor head: copenet.forward_reg / forward_ief on libairpose_grad.so (apg_head_fwd / apg_head_bwd) against fp64
autograd through the oracle (oracle/copenet_ref.py) or an fp64 restatement that applies the same dropout masks
(apg_dropout_mask); determinism, batch invariance, the reference caller's loss chain, an Adam fine-tune, and unchanged
inference behaviour."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, pose_rel_errs, rel_err

TOL_OUT, TOL_GRAD = 1e-5, 1e-4
pytestmark = pytest.mark.gpu
PNAMES = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "decpose.weight", "decpose.bias", "decshape.weight", "decshape.bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _net(sd, dev, precision="fp32"):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision=precision)
    net.load_state_dict(sd)
    return net.to(dev).eval()


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"xf0": torch.relu(torch.randn(B, 2048, generator=g)), "xf1": torch.relu(torch.randn(B, 2048, generator=g))}
    for v in "01":
        d["bb" + v] = torch.rand(B, 3, generator=g) + 0.2
        d["pos" + v] = torch.randn(B, 3, generator=g) * 0.3 + torch.tensor([0., 0., 10.])
        d["orient" + v] = torch.randn(B, 6, generator=g)
        d["art" + v] = torch.randn(B, 126, generator=g)
        d["shape" + v] = torch.randn(B, 10, generator=g) * 0.5
    return d


def _order(d):
    return [d[k] for k in ("xf0", "xf1", "bb0", "bb1", "pos0", "pos1", "orient0", "orient1", "art0", "art1", "shape0", "shape1")]


def _ref_reg(sd, xf0, xf1, bb0, bb1, pos0, pos1, or0, or1, art0, art1, sh0, sh1, masks=None, scale=2.0):
    """fp64 restatement of forward_reg with explicit dropout masks (m1, m2: (2B, 1024), rows = view * B + sample)."""
    B = xf0.shape[0]
    lin = lambda x, p: F.linear(x, sd[p + ".weight"], sd[p + ".bias"])
    out = []
    for v, (xf, bb, pos, o, a, s, pa, ps) in enumerate(((xf0, bb0, pos0, or0, art0, sh0, art1, sh1),
                                                         (xf1, bb1, pos1, or1, art1, sh1, art0, sh0))):
        h = lin(torch.cat([xf, bb, pos, o, a, s, pa, ps], 1), "fc1")
        if masks is not None and masks[0] is not None:
            h = h * masks[0][v * B:(v + 1) * B] * scale
        h = lin(h, "fc2")
        if masks is not None and masks[1] is not None:
            h = h * masks[1][v * B:(v + 1) * B] * scale
        out += [torch.cat([pos, o, a], 1) + lin(h, "decpose"), s + lin(h, "decshape")]
    return out[0], out[1], out[2], out[3]


def _loss_weights(B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 135, generator=g), torch.randn(B, 10, generator=g), torch.randn(B, 135, generator=g),
            torch.randn(B, 10, generator=g)]


def _wloss(outs, W):
    return sum((o * w.to(o)).sum() for o, w in zip(outs, W))


def _sd64(net):
    return {k: v.detach().cpu().double().requires_grad_(k in PNAMES) for k, v in net.state_dict().items()}


def _check_grads(net, leaves, sd64, leaves64, what):
    for k in PNAMES:
        mod, attr = k.split(".")
        got = getattr(getattr(net, mod), attr).grad
        assert got is not None, k
        e = rel_err(got.cpu().numpy(), sd64[k].grad.numpy())
        print("%s grad %-16s rel err %.3e" % (what, k, e))
        assert e < TOL_GRAD, (what, k, e)
    for k, t in leaves.items():
        if not t.requires_grad:
            continue
        assert t.grad is not None and t.grad.shape == t.shape, k
        e = rel_err(t.grad.cpu().numpy(), leaves64[k].grad.numpy())
        print("%s grad %-16s rel err %.3e" % (what, k, e))
        assert e < TOL_GRAD, (what, k, e)
    for m in ("deccam",):
        assert getattr(net, m).weight.grad is None and getattr(net, m).bias.grad is None
    assert net.conv1.weight.grad is None


def _check_outs(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.detach().cpu().numpy(), b.detach().numpy()
        errs = pose_rel_errs(a, b) if a.shape[1] == 135 else {"betas": rel_err(a, b)}
        for k, e in errs.items():
            assert e < TOL_OUT, (what, i, k, e)


def _zero(net):
    for p in net.parameters():
        p.grad = None


# ------------------------------------------------------------------------------------------------ 1. eval mode
@pytest.mark.parametrize("B", [1, 5, 64])
def test_eval_forward_reg_outputs_and_grads_match_oracle(copenet_sd, dev, B):
    from oracle import copenet_ref
    net = _net(copenet_sd, dev)
    d = _inputs(B, 100 + B)
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in d.items()}
    W = _loss_weights(B, 7)
    outs = net.forward_reg(*_order(leaves))
    assert all(o.grad_fn is not None for o in outs)
    _wloss(outs, W).backward()
    sd64 = _sd64(net)
    l64 = {k: v.double().requires_grad_(True) for k, v in d.items()}
    want = copenet_ref.forward_reg(sd64, *_order(l64))
    _check_outs(outs, want, "eval B=%d" % B)
    _wloss(want, [w.double() for w in W]).backward()
    _check_grads(net, leaves, sd64, l64, "eval B=%d" % B)


def test_eval_forward_ief_broadcast_init_theta(copenet_sd, dev):
    """forward_ief with a (1,144) init_theta and (1,10) init_shape that require grad: the gradient is the batch sum, and the
    columns past 132 get zero."""
    from oracle import copenet_ref
    B = 5
    net = _net(copenet_sd, dev)
    d = _inputs(B, 3)
    g = torch.Generator().manual_seed(4)
    th = (net.init_pose.cpu() + 0.1 * torch.randn(1, 144, generator=g))
    sh = torch.randn(1, 10, generator=g) * 0.3
    leaves = {"xf0": d["xf0"].to(dev).requires_grad_(True), "xf1": d["xf1"].to(dev), "th": th.to(dev).requires_grad_(True),
              "sh": sh.to(dev).requires_grad_(True)}
    W = _loss_weights(B, 8)
    outs = net.forward_ief(leaves["xf0"], leaves["xf1"], d["bb0"].to(dev), d["bb1"].to(dev), d["pos0"].to(dev),
                           d["pos1"].to(dev), leaves["th"], leaves["th"], leaves["sh"], None, iters=3)
    _wloss(outs, W).backward()
    sd64 = _sd64(net)
    l64 = {"xf0": d["xf0"].double().requires_grad_(True), "xf1": d["xf1"].double(), "th": th.double().requires_grad_(True),
           "sh": sh.double().requires_grad_(True)}
    want = copenet_ref.ief(sd64, l64["xf0"], l64["xf1"], d["bb0"].double(), d["bb1"].double(), d["pos0"].double(),
                           d["pos1"].double(), l64["th"], l64["th"], l64["sh"].expand(B, -1), None, iters=3)
    _check_outs(outs, want, "ief broadcast")
    _wloss(want, [w.double() for w in W]).backward()
    assert leaves["th"].grad.shape == (1, 144) and float(leaves["th"].grad[:, 132:].abs().max()) == 0.0
    _check_grads(net, leaves, sd64, l64, "ief broadcast")


# ------------------------------------------------------------------------------------------------ 2. train mode, masks
def _masks(net, seed, B, dev):
    from airpose_amd import _native_grad as G
    m = []
    for layer, drop in ((1, net.drop1), (2, net.drop2)):
        m.append(G.dropout_mask(seed, layer, 2 * B, 1024, drop.p, dev).cpu().double() if drop.training else None)
    return m


@pytest.mark.parametrize("B", [1, 5, 64])
def test_train_forward_reg_with_dropout_matches_restatement(copenet_sd, dev, B):
    net = _net(copenet_sd, dev).train()
    d = _inputs(B, 200 + B)
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in d.items()}
    W = _loss_weights(B, 9)
    torch.manual_seed(1234)
    outs = net.forward_reg(*_order(leaves))
    seed = net.last_dropout_seed
    _wloss(outs, W).backward()
    masks = _masks(net, seed, B, dev)
    sd64 = _sd64(net)
    l64 = {k: v.double().requires_grad_(True) for k, v in d.items()}
    want = _ref_reg(sd64, *_order(l64), masks=masks)
    _check_outs(outs, want, "train B=%d" % B)
    _wloss(want, [w.double() for w in W]).backward()
    _check_grads(net, leaves, sd64, l64, "train B=%d" % B)
    # torch.manual_seed reproduces the seed
    torch.manual_seed(1234)
    again = net.forward_reg(*_order({k: v.detach() for k, v in leaves.items()}))
    assert net.last_dropout_seed == seed and all(torch.equal(a, b) for a, b in zip(outs, again))


def test_dropout_mask_statistics_and_scale(copenet_sd, dev):
    from airpose_amd import _native_grad as G
    m = G.dropout_mask(987654321, 1, 256, 1024, 0.5, dev).cpu().numpy()
    assert m.size >= 10 ** 5 and set(np.unique(m)) <= {0, 1}
    assert abs(m.mean() - 0.5) < 0.01
    m2 = G.dropout_mask(987654321, 2, 256, 1024, 0.5, dev).cpu().numpy()
    assert (m != m2).mean() > 0.4                               # layers draw independent masks
    assert G.dropout_mask(5, 1, 4, 1024, 0.0, dev).all()        # p = 0: the identity
    # kept values are scaled by exactly 2: one fc1 row through the head with drop2 off, fc2 = identity, decoders read h1 directly
    net = _net(copenet_sd, dev).train()
    net.drop2.eval()
    with torch.no_grad():
        net.fc2.weight.copy_(torch.eye(1024))
        net.fc2.bias.zero_()
        net.decpose.weight.zero_()
        net.decpose.weight[:135, :135].copy_(torch.eye(135))
        net.decpose.bias.zero_()
    B = 4
    d = {k: v.to(dev) for k, v in _inputs(B, 11).items()}
    for k in ("pos0", "orient0", "art0"):
        d[k].zero_()                                             # pose0 = delta exactly
    pose0 = net.forward_reg(*_order(d))[0]
    seed = net.last_dropout_seed
    net.eval()
    with torch.enable_grad():
        ref0 = net.forward_reg(*_order({k: (v.requires_grad_(True) if k == "xf0" else v) for k, v in d.items()}))[0]
    m1 = G.dropout_mask(seed, 1, 2 * B, 1024, 0.5, dev)[:B, :135].bool()
    kept, full = pose0.detach()[m1], ref0.detach()[m1]
    assert kept.numel() > 0 and torch.equal(kept, 2 * full) and float(full.abs().min()) > 0
    assert float(pose0.detach()[~m1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. forward_ief, train mode
@pytest.mark.parametrize("iters", [1, 2, 3, 5])
def test_train_forward_ief_matches_unrolled_restatement(copenet_sd, dev, iters):
    from airpose_amd import head_grad
    B = 6
    net = _net(copenet_sd, dev).train()
    d = _inputs(B, 300 + iters)
    leaves = {k: v.to(dev).requires_grad_(k.startswith(("xf", "pos", "bb"))) for k, v in d.items()}
    W = _loss_weights(B, 10)
    torch.manual_seed(77)
    outs = net.forward_ief(leaves["xf0"], leaves["xf1"], leaves["bb0"], leaves["bb1"], leaves["pos0"], leaves["pos1"], iters=iters)
    _wloss(outs, W).backward()
    torch.manual_seed(77)
    seeds = [head_grad.new_seed() for _ in range(iters)]
    sd64 = _sd64(net)
    l64 = {k: v.double().requires_grad_(k.startswith(("xf", "pos", "bb"))) for k, v in d.items()}
    ip = sd64["init_pose"]
    o0 = o1 = ip[:, :6].expand(B, -1)
    a0 = a1 = ip[:, 6:132].expand(B, -1)
    s0 = s1 = sd64["init_shape"].expand(B, -1)
    p0, p1 = l64["pos0"], l64["pos1"]
    for it in range(iters):
        masks = _masks(net, seeds[it], B, dev)
        q0, b0, q1, b1 = _ref_reg(sd64, l64["xf0"], l64["xf1"], l64["bb0"], l64["bb1"], p0, p1, o0, o1, a0, a1, s0, s1, masks)
        p0, p1, o0, o1, a0, a1, s0, s1 = q0[:, :3], q1[:, :3], q0[:, 3:9], q1[:, 3:9], q0[:, 9:], q1[:, 9:], b0, b1
    want = (q0, b0, q1, b1)
    _check_outs(outs, want, "ief iters=%d" % iters)
    _wloss(want, [w.double() for w in W]).backward()
    _check_grads(net, {k: v for k, v in leaves.items() if v.requires_grad}, sd64, l64, "ief iters=%d" % iters)


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_gradients_are_bit_reproducible_and_batch_invariant(copenet_sd, dev):
    net = _net(copenet_sd, dev).train()
    d = _inputs(64, 400)
    W = _loss_weights(64, 11)

    def run(dd, WW, seed):
        _zero(net)
        lv = {k: v.to(dev).requires_grad_(True) for k, v in dd.items()}
        torch.manual_seed(seed)
        _wloss(net.forward_ief(lv["xf0"], lv["xf1"], lv["bb0"], lv["bb1"], lv["pos0"], lv["pos1"], iters=3), WW).backward()
        return {k: v.grad.clone() for k, v in lv.items() if v.grad is not None}, \
            {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    gi1, gp1 = run(d, W, 5)
    gi2, gp2 = run(d, W, 5)
    assert set(gp1) == {"fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "decpose.weight", "decpose.bias",
                        "decshape.weight", "decshape.bias"}
    for k in gp1:
        assert torch.equal(gp1[k], gp2[k]), k
    for k in gi1:
        assert torch.equal(gi1[k], gi2[k]), k
    # eval mode: a sample's input gradients do not depend on the batch size or its position
    net.eval()
    idx = [10, 3, 40]
    small = {k: v[idx] for k, v in d.items()}
    Ws = [w[idx] for w in W]
    gi64, _ = run(d, W, 0)
    gi3, _ = run(small, Ws, 0)
    for k in gi3:
        assert torch.equal(gi3[k], gi64[k][idx]), k


# ------------------------------------------------------------------------------------------------ 5. the reference caller's loss
def _caller_loss(mods, pose0, b0, pose1, b1, pos0, pos1, tgt, dtype):
    """copenet_twoview.py:212-317 + get_loss (:83-161): trans scaling in place, rot6d, SMPL-X, transform_smpl, projection,
    the 2-D keypoint / 3-D joint / rotmat / betas terms."""
    rot6d, smplx_fwd, transform, project = mods
    B = pose0.shape[0]
    t0, t1 = pose0[:, :3], pose1[:, :3]
    t0 /= 0.05
    t1 /= 0.05
    pos0 /= 0.05
    pos1 /= 0.05
    loss = 0.
    j3 = []
    for v, (pose, betas, t) in enumerate(((pose0, b0, t0), (pose1, b1, t1))):
        rotmat = rot6d(pose[:, 3:]).view(B, 22, 3, 3)
        verts, joints = smplx_fwd(betas, rotmat[:, 1:])
        M = torch.cat([rotmat[:, :1].squeeze(1), t.unsqueeze(2)], dim=2)
        vc, jc = transform(M, verts, joints)
        j2d = project(jc, tgt["cc%d" % v])
        loss = loss + ((j2d[:, :22] - tgt["j2d"].to(j2d)) ** 2).mean() * 1e-4
        loss = loss + ((jc[:, :22] - tgt["j3d"].to(jc)) ** 2).mean()
        loss = loss + ((rotmat[:, 1:] - tgt["rot"].to(rotmat)) ** 2).mean() + ((rotmat[:, :1] - tgt["root"].to(rotmat)) ** 2).mean()
        loss = loss + ((t - tgt["trans"].to(t)) ** 2).mean() + (betas * betas).mean() * 0.01
        j3.append(jc[:, :22])
    return loss + ((j3[0] - j3[1]) ** 2).mean()


def test_reference_caller_chain_matches_fp64(copenet_sd, smplx_model, dev):
    from airpose_amd import geometry, smplx, utils
    from oracle import copenet_ref, geometry_ref, smplx_ref
    B = 4
    net = _net(copenet_sd, dev).train()
    net.drop1.eval()
    net.drop2.eval()                                             # dropout off: the fp64 chain has no masks
    body = smplx.SMPLX(model_data=smplx_model)
    d = _inputs(B, 500)
    g = torch.Generator().manual_seed(5)
    tgt = {"j2d": torch.randn(B, 22, 2, generator=g) * 100 + 500, "j3d": torch.randn(B, 22, 3, generator=g),
           "rot": torch.eye(3).expand(B, 21, 3, 3), "root": torch.eye(3).expand(B, 1, 3, 3),
           "trans": torch.randn(B, 3, generator=g) + torch.tensor([0., 0., 200.]),
           "cc0": torch.full((1, B, 2), 500.), "cc1": torch.full((1, B, 2), 520.)}
    eye = lambda dt, dv: torch.eye(3, dtype=dt, device=dv).expand(B, 1, 3, 3)
    pos0, pos1 = d["pos0"].clone().to(dev), d["pos1"].clone().to(dev)
    xf0, xf1 = d["xf0"].to(dev), d["xf1"].to(dev)
    p0, b0, p1, b1 = net.forward_ief(xf0, xf1, d["bb0"].to(dev), d["bb1"].to(dev), pos0, pos1, iters=3)
    gpu = (geometry.rot6d_to_rotmat,
           lambda be, bp: (lambda o: (o.vertices, o.joints))(body.forward(betas=be, body_pose=bp, global_orient=eye(torch.float32, dev),
                                                                           transl=torch.zeros(B, 3, device=dev), pose2rot=False)),
           lambda M, v, j: utils.transform_smpl(M, v, j)[:2],
           lambda j, cc: geometry.perspective_projection(j, None, None, (5000., 5000.), cc.to(dev)))
    _caller_loss(gpu, p0, b0, p1, b1, pos0, pos1, tgt, torch.float32).backward()
    sd64 = _sd64(net)
    q0, c0, q1, c1 = copenet_ref.ief(sd64, d["xf0"].double(), d["xf1"].double(), d["bb0"].double(), d["bb1"].double(),
                                     d["pos0"].double(), d["pos1"].double(), iters=3)
    ref = (geometry_ref.rot6d_to_rotmat,
           lambda be, bp: smplx_ref.smplx_forward(smplx_model, betas=be, body_pose=bp, global_orient=eye(torch.float64, "cpu"),
                                                  transl=torch.zeros(B, 3, dtype=torch.float64), dtype=torch.float64),
           lambda M, v, j: geometry_ref.transform_smpl(M, v, j),
           lambda j, cc: geometry_ref.perspective_projection(j, torch.eye(3, dtype=torch.float64).expand(B, 3, 3),
                                                             torch.zeros(B, 3, dtype=torch.float64), (5000., 5000.),
                                                             cc.double().reshape(-1, 2)))
    _caller_loss(ref, q0, c0, q1, c1, d["pos0"].double().clone(), d["pos1"].double().clone(), tgt, torch.float64).backward()
    for k in PNAMES:
        mod, attr = k.split(".")
        e = rel_err(getattr(getattr(net, mod), attr).grad.cpu().numpy(), sd64[k].grad.numpy())
        print("caller chain grad %-16s rel err %.3e" % (k, e))
        assert e < TOL_GRAD, (k, e)


# ------------------------------------------------------------------------------------------------ 6. fine-tune
def test_adam_fine_tune_of_the_head_then_eval_repacks(copenet_sd, dev):
    from airpose_amd import weights as W
    B = 8
    net = _net(copenet_sd, dev)
    inp = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(99, B).items()}
    with torch.no_grad():
        xf0, xf1 = net.forward_feat_ext(inp["im0"]), net.forward_feat_ext(inp["im1"])     # the trunk, once
    bb0, bb1 = inp["bb0"], inp["bb1"]
    pos = torch.tensor([[0., 0., 10.]], device=dev).expand(B, 3).contiguous()
    target_net = _net(copenet_sd, dev)
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(3)
        target_net.decpose.bias.add_(0.05 * torch.randn(135, generator=g).to(dev))
        target_net.decshape.bias.add_(0.05 * torch.randn(10, generator=g).to(dev))
        target = target_net.forward_ief(xf0, xf1, bb0, bb1, pos, pos, iters=3)
    net.train()
    net.drop1.eval()
    net.drop2.eval()
    params = [p for m in ("fc1", "fc2", "decpose", "decshape") for p in getattr(net, m).parameters()]
    opt = torch.optim.Adam(params, lr=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, 100, 0.3)
    losses = []
    for _ in range(300):
        opt.zero_grad()
        out = net.forward_ief(xf0, xf1, bb0, bb1, pos, pos, iters=3)
        loss = sum(((o - t) ** 2).mean() for o, t in zip(out, target))
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    print("fine-tune losses", ["%.2e" % x for x in losses[::30]])
    print("fine-tune loss %.3e -> %.3e" % (losses[0], losses[-1]))
    assert losses[-1] * 100 <= losses[0], losses[::30]
    net.eval()
    with torch.no_grad():
        inf = net.forward_ief(xf0, xf1, bb0, bb1, pos, pos, iters=3)           # the inference path: must repack
    grad_path = net.forward_ief(xf0.clone().requires_grad_(True), xf1, bb0, bb1, pos, pos, iters=3)
    assert grad_path[0].grad_fn is not None and inf[0].grad_fn is None
    for a, b in zip(inf, grad_path):
        a, b = a.cpu().numpy(), b.detach().cpu().numpy()
        errs = pose_rel_errs(a, b) if a.shape[1] == 135 else {"betas": rel_err(a, b)}
        for k, e in errs.items():
            assert e < 1e-4, (k, e)


# ------------------------------------------------------------------------------------------------ 7. unchanged behaviour
def test_eval_without_grad_inputs_takes_the_inference_path(copenet_sd, dev):
    d = {k: v.to(dev) for k, v in _inputs(3, 600).items()}
    net = _net(copenet_sd, dev)
    fresh = _net(copenet_sd, dev)
    a = net.forward_ief(d["xf0"], d["xf1"], d["bb0"], d["bb1"], d["pos0"], d["pos1"], iters=3)
    b = fresh.forward_ief(d["xf0"], d["xf1"], d["bb0"], d["bb1"], d["pos0"], d["pos1"], iters=3)
    for x, y in zip(a, b):
        assert x.grad_fn is None and torch.equal(x, y)
    r = net.forward_reg(*_order(d))
    assert all(t.grad_fn is None for t in r)


def test_forward_and_other_heads_still_raise_in_train_mode(copenet_sd, dev):
    from airpose_amd import copenet_sep_model, hmr_model
    net = _net(copenet_sd, dev).train()
    x = torch.zeros(1, 3, 224, 224, device=dev)
    z = torch.zeros(1, 3, device=dev)
    with pytest.raises(RuntimeError, match="inference path only"):
        net(x, x, z, z, z, z)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.forward_feat_ext(x)
    with pytest.raises(RuntimeError, match="inference path only"):
        net.regressor_step(torch.zeros(1, 2048, device=dev), z, torch.zeros(1, 135, device=dev), torch.zeros(1, 10, device=dev),
                           torch.zeros(1, 136, device=dev))
    hmr = hmr_model.getcopenet(MEAN_PARAMS).to(dev).train()
    with pytest.raises(RuntimeError, match="inference path only"):
        hmr(x)
    sep = copenet_sep_model.getcopenet_sep(MEAN_PARAMS).to(dev).train()
    with pytest.raises(RuntimeError):
        sep.forward_ief(torch.zeros(1, 2048, device=dev), torch.zeros(1, 2048, device=dev), z, z, z, z)


def test_grad_path_calls_no_torch_matmul(copenet_sd, dev, monkeypatch):
    net = _net(copenet_sd, dev).train()
    d = {k: v.to(dev).requires_grad_(True) for k, v in _inputs(4, 700).items()}

    def boom(*a, **k):
        raise AssertionError("torch matrix product on the head's training path")
    for mod, name in ((F, "linear"), (torch, "matmul"), (torch, "mm"), (torch, "addmm"), (torch, "bmm"),
                      (torch.Tensor, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "addmm"), (torch.Tensor, "bmm"),
                      (torch.Tensor, "__matmul__")):
        monkeypatch.setattr(mod, name, boom)
    outs = net.forward_ief(d["xf0"], d["xf1"], d["bb0"], d["bb1"], d["pos0"], d["pos1"], iters=2)
    sum(o.sum() for o in outs).backward()
    assert net.fc1.weight.grad is not None and d["xf0"].grad is not None


def test_double_backward_raises_and_wrong_device_is_named(copenet_sd, dev):
    net = _net(copenet_sd, dev)
    d = {k: v.to(dev) for k, v in _inputs(2, 800).items()}
    x = d["xf0"].clone().requires_grad_(True)
    outs = net.forward_reg(x, *_order(d)[1:])
    g, = torch.autograd.grad(outs[0].sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    cpu_net = _net(copenet_sd, torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"net\.to\(dev\)"):
        cpu_net.forward_reg(x, *_order(d)[1:])
