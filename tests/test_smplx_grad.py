"""Differentiable SMPLX.forward: the hand-written adjoint (ap_smplx_bwd, ap_batch_rodrigues_bwd) against torch autograd through
the CPU oracle (oracle/smplx_ref.py, float64), plus the properties the backward promises: bit-identical forward under grad,
deterministic and batch-invariant gradients, no shared workspace with the forward."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err

TOL32 = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def body(smplx_model, dev):
    from airpose_amd import smplx
    return smplx.SMPLX(model_data=smplx_model)


def _rot(n, gen, scale=0.7):
    from oracle import smplx_ref
    return smplx_ref.batch_rodrigues(torch.randn(n, 3, generator=gen, dtype=torch.float64) * scale).float()


def _weights(B, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 10475, 3, generator=gen), torch.randn(B, 127, 3, generator=gen)


def _loss(v, j, Wv, Wj, use_v=True, use_j=True):
    out = 0.
    if use_v:
        out = out + (v * Wv.to(v)).sum()
    if use_j:
        out = out + (j * Wj.to(j)).sum()
    return out


def _gpu_grads(body, dev, inputs, want, Wv, Wj, use_v=True, use_j=True, **kw):
    leaves = {k: (v.to(dev).clone().requires_grad_(k in want) if v is not None else None) for k, v in inputs.items()}
    out = body.forward(**leaves, **kw)
    _loss(out.vertices if use_v else None, out.joints, Wv, Wj, use_v, use_j).backward()
    return {k: leaves[k].grad for k in want}, leaves, out


def _ref_grads(fn, inputs, want, Wv, Wj, use_v=True, use_j=True, **kw):
    leaves = {k: (v.double().clone().requires_grad_(k in want) if v is not None else None) for k, v in inputs.items()}
    v, j = fn(**leaves, dtype=torch.float64, **kw)
    _loss(v, j, Wv.double(), Wj.double(), use_v, use_j).backward()
    return {k: leaves[k].grad for k in want}


def _check(got, want, what=""):
    for k in want:
        assert got[k] is not None, k
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        e = rel_err(got[k].cpu().numpy(), want[k].numpy())
        print("%s grad %-16s rel err %.3e" % (what, k, e))
        assert np.isfinite(got[k].cpu().numpy()).all(), k
        assert e < TOL32, (k, e)


def _rotmat_inputs(B, seed, extra=False):
    gen = torch.Generator().manual_seed(seed)
    d = dict(betas=torch.randn(B, 10, generator=gen), expression=torch.randn(B, 10, generator=gen) * 0.5,
             global_orient=_rot(B, gen).view(B, 1, 3, 3), body_pose=_rot(B * 21, gen).view(B, 21, 3, 3),
             transl=torch.randn(B, 3, generator=gen))
    if extra:
        d.update(jaw_pose=_rot(B, gen, 0.3).view(B, 1, 3, 3), leye_pose=_rot(B, gen, 0.2).view(B, 1, 3, 3),
                 reye_pose=_rot(B, gen, 0.2).view(B, 1, 3, 3), left_hand_pose=_rot(B * 15, gen, 0.4).view(B, 15, 3, 3),
                 right_hand_pose=_rot(B * 15, gen, 0.4).view(B, 15, 3, 3))
    return d


def _oracle_rotmat(model):
    from oracle import smplx_ref
    return lambda dtype, **kw: smplx_ref.smplx_forward(model, **kw, dtype=dtype)


# ------------------------------------------------------------------------------------------------ CPU
def test_binding_exposes_the_backward_entry_points():
    from airpose_amd import _native
    assert _native.ABI_VERSION == 13                                # (the backward entry points came with 10; 11: the stem / pool operators; 12: the range hook; 13: the trunk-form operators)
    for name in ("ap_smplx_bwd", "ap_batch_rodrigues_bwd"):
        assert name in _native.SIGNATURES
    res, args = _native.SIGNATURES["ap_smplx_bwd"]
    assert res is ctypes.c_int and len(args) == 17
    res, args = _native.SIGNATURES["ap_batch_rodrigues_bwd"]
    assert res is ctypes.c_int and len(args) == 5
    L = _native.lib()
    assert L.ap_smplx_bwd.argtypes is not None and L.ap_batch_rodrigues_bwd.argtypes is not None


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5])
def test_grad_rotmat_body_matches_oracle(body, smplx_model, dev, B):
    inp = _rotmat_inputs(B, 100 + B)
    want = ("betas", "expression", "global_orient", "body_pose", "transl")
    Wv, Wj = _weights(B, 7)
    got, _, out = _gpu_grads(body, dev, inp, want, Wv, Wj, pose2rot=False)
    assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
    _check(got, _ref_grads(_oracle_rotmat(smplx_model), inp, want, Wv, Wj), "body B=%d" % B)


@pytest.mark.gpu
def test_grad_rotmat_hands_face_matches_oracle(body, smplx_model, dev):
    B = 3
    inp = _rotmat_inputs(B, 200, extra=True)
    want = tuple(inp)
    Wv, Wj = _weights(B, 8)
    got, _, _ = _gpu_grads(body, dev, inp, want, Wv, Wj, pose2rot=False)
    _check(got, _ref_grads(_oracle_rotmat(smplx_model), inp, want, Wv, Wj), "hands/face")


@pytest.mark.gpu
def test_grad_axis_angle_pca_hands_matches_oracle(body, smplx_model, dev):
    from oracle import smplx_ref
    B = 3
    gen = torch.Generator().manual_seed(300)
    inp = dict(betas=torch.randn(B, 10, generator=gen), global_orient=torch.randn(B, 3, generator=gen),
               body_pose=torch.randn(B, 63, generator=gen) * 0.5, jaw_pose=torch.randn(B, 3, generator=gen) * 0.2,
               left_hand_pose=torch.randn(B, 6, generator=gen) * 0.5, right_hand_pose=torch.randn(B, 6, generator=gen) * 0.5,
               transl=torch.randn(B, 3, generator=gen))
    inp["body_pose"][1] = 0.                                  # a body at zero axis-angle: the epsilon path of batch_rodrigues
    inp["global_orient"][1] = 0.
    want = tuple(inp)
    Wv, Wj = _weights(B, 9)
    old = (body.use_pca, body.flat_hand_mean, body.num_pca_comps)
    body.use_pca, body.flat_hand_mean, body.num_pca_comps = True, False, 6
    try:
        got, _, _ = _gpu_grads(body, dev, inp, want, Wv, Wj, pose2rot=True)
    finally:
        body.use_pca, body.flat_hand_mean, body.num_pca_comps = old
    fn = lambda dtype, **kw: smplx_ref.smplx_forward_axis_angle(smplx_model, **kw, use_pca=True, num_pca_comps=6,
                                                                flat_hand_mean=False, dtype=dtype)
    _check(got, _ref_grads(fn, inp, want, Wv, Wj), "axis-angle")


@pytest.mark.gpu
def test_batch_rodrigues_grad_matches_oracle(dev):
    from airpose_amd import lbs
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(31)
    aa = torch.randn(64, 3, generator=gen) * 1.5
    aa[0] = 0.
    W = torch.randn(64, 3, 3, generator=gen)
    x = aa.to(dev).requires_grad_(True)
    (lbs.batch_rodrigues(x) * W.to(dev)).sum().backward()
    y = aa.double().requires_grad_(True)
    (smplx_ref.batch_rodrigues(y) * W.double()).sum().backward()
    assert rel_err(x.grad.cpu().numpy(), y.grad.numpy()) < TOL32


@pytest.mark.gpu
def test_grad_joints_only_vertices_only_and_betas_only(body, smplx_model, dev):
    B = 2
    inp = _rotmat_inputs(B, 400)
    want = ("betas", "global_orient", "body_pose", "transl")
    Wv, Wj = _weights(B, 10)
    ref = _oracle_rotmat(smplx_model)
    got, _, out = _gpu_grads(body, dev, inp, want, Wv, Wj, use_v=False, pose2rot=False, return_verts=False)
    assert out.vertices is None
    _check(got, _ref_grads(ref, inp, want, Wv, Wj, use_v=False), "joints-only")
    got, _, _ = _gpu_grads(body, dev, inp, want, Wv, Wj, use_j=False, pose2rot=False)
    _check(got, _ref_grads(ref, inp, want, Wv, Wj, use_j=False), "vertices-only")
    got, leaves, _ = _gpu_grads(body, dev, inp, ("betas",), Wv, Wj, pose2rot=False)
    for k in ("expression", "global_orient", "body_pose", "transl"):
        assert leaves[k].grad is None, k
    assert torch.isfinite(got["betas"]).all()
    _check(got, _ref_grads(ref, inp, ("betas",), Wv, Wj), "betas-only")


@pytest.mark.gpu
def test_grad_broadcast_betas(body, smplx_model, dev):
    B = 4
    inp = _rotmat_inputs(B, 500)
    inp["betas"] = inp["betas"][:1]
    Wv, Wj = _weights(B, 11)
    got, _, _ = _gpu_grads(body, dev, inp, ("betas", "body_pose"), Wv, Wj, pose2rot=False)
    assert got["betas"].shape == (1, 10)
    ref_inp = dict(inp, betas=inp["betas"].expand(B, 10))
    leaves = {k: v.double() for k, v in ref_inp.items()}
    leaves["betas"] = inp["betas"].double().requires_grad_(True)
    from oracle import smplx_ref
    v, j = smplx_ref.smplx_forward(smplx_model, **dict(leaves, betas=leaves["betas"].expand(B, 10)), dtype=torch.float64)
    _loss(v, j, Wv.double(), Wj.double()).backward()
    assert rel_err(got["betas"].cpu().numpy(), leaves["betas"].grad.numpy()) < TOL32


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [False, True])
def test_forward_under_grad_is_bit_identical(body, dev, extra):
    inp = {k: v.to(dev) for k, v in _rotmat_inputs(6, 600, extra).items()}
    with torch.no_grad():
        ref = body.forward(**inp, pose2rot=False)
    leaves = {k: v.clone().requires_grad_(True) for k, v in inp.items()}
    out = body.forward(**leaves, pose2rot=False)
    assert out.vertices.requires_grad
    assert torch.equal(out.vertices.detach(), ref.vertices) and torch.equal(out.joints.detach(), ref.joints)


def _body_grads(body, dev, inp, Wv, Wj, want):
    got, _, _ = _gpu_grads(body, dev, inp, want, Wv, Wj, pose2rot=False)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [False, True])
def test_backward_is_deterministic_and_batch_invariant(body, dev, extra):
    B = 77
    inp = _rotmat_inputs(B, 700, extra)
    want = tuple(inp)
    Wv, Wj = _weights(B, 12)
    g1 = _body_grads(body, dev, inp, Wv, Wj, want)
    g2 = _body_grads(body, dev, inp, Wv, Wj, want)
    for k in want:
        assert torch.equal(g1[k], g2[k]), k
    pick = lambda d, idx: {k: v[idx] for k, v in d.items()}
    for idx in ([0], [40], [76], [76, 5, 40]):
        gs = _body_grads(body, dev, pick(inp, idx), Wv[idx], Wj[idx], want)
        for k in want:
            assert torch.equal(gs[k], g1[k][idx]), (k, idx)


@pytest.mark.gpu
def test_backward_leaves_the_forward_workspaces_alone(body, dev):
    inp = {k: v.to(dev) for k, v in _rotmat_inputs(9, 800, True).items()}
    with torch.no_grad():
        before = body.forward(**inp, pose2rot=False)
        before_body = body.forward(betas=inp["betas"], body_pose=inp["body_pose"], pose2rot=False)
    other = {k: v.to(dev).requires_grad_(True) for k, v in _rotmat_inputs(13, 801, True).items()}
    out = body.forward(**other, pose2rot=False)
    (out.vertices.sum() + out.joints.sum()).backward()
    with torch.no_grad():
        after = body.forward(**inp, pose2rot=False)
        after_body = body.forward(betas=inp["betas"], body_pose=inp["body_pose"], pose2rot=False)
    assert torch.equal(before.vertices, after.vertices) and torch.equal(before.joints, after.joints)
    assert torch.equal(before_body.vertices, after_body.vertices) and torch.equal(before_body.joints, after_body.joints)


@pytest.mark.gpu
def test_double_backward_raises(body, dev):
    inp = {k: v.to(dev) for k, v in _rotmat_inputs(2, 900).items()}
    b = inp["betas"].clone().requires_grad_(True)
    out = body.forward(betas=b, body_pose=inp["body_pose"], pose2rot=False)
    g, = torch.autograd.grad(out.vertices.pow(2).sum(), b, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.gpu
def test_adam_fit_of_a_target_body(body, dev):
    gen = torch.Generator().manual_seed(1000)
    B = 2
    tb, tp, tt = torch.randn(B, 10, generator=gen) * 0.5, torch.randn(B, 63, generator=gen) * 0.05, torch.randn(B, 3, generator=gen) * 0.2
    with torch.no_grad():
        target = body.forward(betas=tb.to(dev), body_pose=tp.to(dev), transl=tt.to(dev), pose2rot=True).vertices
    betas = torch.zeros(B, 10, device=dev, requires_grad=True)
    pose = torch.zeros(B, 63, device=dev, requires_grad=True)
    transl = torch.zeros(B, 3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([betas, pose, transl], lr=0.08)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        v = body.forward(betas=betas, body_pose=pose, transl=transl, pose2rot=True).vertices
        loss = (v - target).pow(2).sum(-1).mean()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.item())
    print("adam fit: loss %.3e -> %.3e" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all()
    assert losses[-1] < 1e-3 * losses[0]
