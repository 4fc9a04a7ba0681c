"""Differentiable geometry helpers (geometry.rot6d_to_rotmat, geometry.perspective_projection, utils.transform_smpl): the HIP
adjoints of libairpose_grad.so against fp64 autograd through oracle/geometry_ref.py, plus bit-identical forwards under grad,
deterministic gradients and no grad_fn on no-grad calls."""
import numpy as np
import pytest
import torch

from conftest import rel_err

TOL = 1e-4
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _grads(fn, inputs, W, dev=None):
    leaves = [(t.to(dev) if dev is not None else t.double()).clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    outs = out if isinstance(out, (tuple, list)) else (out,)
    loss = sum((o * w.to(o)).sum() for o, w in zip(outs, W) if o is not None)
    loss.backward()
    return [l.grad for l in leaves], outs


def _x6(n, gen, n_eps=0):
    x = torch.randn(n, 6, generator=gen)
    x[:n_eps, 0::2] *= 1e-14                                   # a1 below F.normalize's clamp: the eps branch
    return x


def test_rot6d_grad_matches_oracle(dev):
    from airpose_amd import geometry
    from oracle import geometry_ref
    gen = torch.Generator().manual_seed(1)
    n, n_eps = 300, 4
    x = _x6(n, gen, n_eps)
    W = [torch.randn(n, 3, 3, generator=gen)]
    (g,), (out,) = _grads(geometry.rot6d_to_rotmat, [x], W, dev)
    (r,), _ = _grads(geometry_ref.rot6d_to_rotmat, [x], W)
    assert out.grad_fn is not None and g.shape == x.shape
    g = g.cpu().numpy()
    assert np.isfinite(g).all()
    e_norm, e_eps = rel_err(g[n_eps:], r[n_eps:].numpy()), rel_err(g[:n_eps], r[:n_eps].numpy())
    print("rot6d grad rel err %.3e, eps branch %.3e" % (e_norm, e_eps))
    assert e_norm < TOL and e_eps < TOL
    assert np.abs(g[:n_eps]).max() > 1e6                       # the eps branch really was taken (g / 1e-12)


def _proj_inputs(B, P, gen):
    from oracle import smplx_ref
    pts = torch.randn(B, P, 3, generator=gen)
    rot = smplx_ref.batch_rodrigues(torch.randn(B, 3, generator=gen, dtype=torch.float64) * 0.3).float()
    tr = torch.randn(B, 3, generator=gen) * 0.2 + torch.tensor([0., 0., 10.])
    cc = torch.randn(1, B, 2, generator=gen) * 10 + 500.
    return pts, rot, tr, cc


@pytest.mark.parametrize("B,P", [(1, 7), (5, 127), (3, 600)])
def test_perspective_projection_grad_matches_oracle(dev, B, P):
    from airpose_amd import geometry
    from oracle import geometry_ref
    gen = torch.Generator().manual_seed(10 + B)
    inp = _proj_inputs(B, P, gen)
    W = [torch.randn(B, P, 2, generator=gen)]
    f = (5000., 4000.)
    got, (out,) = _grads(lambda p, r, t, c: geometry.perspective_projection(p, r, t, f, c), inp, W, dev)
    want, _ = _grads(lambda p, r, t, c: geometry_ref.perspective_projection(p, r, t, f, c.reshape(-1, 2)), inp, W)
    assert out.grad_fn is not None
    for name, a, b, x in zip(("points", "rotation", "translation", "camera_center"), got, want, inp):
        assert a.shape == x.shape, name                        # the caller's shapes: (1,B,2) centre included
        e = rel_err(a.cpu().numpy(), b.numpy())
        print("projection B=%d P=%d grad %-14s rel err %.3e" % (B, P, name, e))
        assert e < TOL, name


def test_focal_length_is_not_differentiable(dev):
    from airpose_amd import geometry
    gen = torch.Generator().manual_seed(3)
    pts, rot, tr, cc = (t.to(dev) for t in _proj_inputs(2, 5, gen))
    f = torch.tensor([5000., 5000.], device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="focal_length"):
        geometry.perspective_projection(pts.requires_grad_(True), rot, tr, f, cc)


def _transform_ref(M, v, j, o, t):
    R, tt = M[:, :3, :3], M[:, :3, 3]
    from oracle import geometry_ref
    vv, jj = geometry_ref.transform_smpl(M, v, j)
    return vv, jj, R @ o, (R @ t.unsqueeze(2)).squeeze(2) + tt


@pytest.mark.parametrize("B", [1, 4])
def test_transform_smpl_grad_matches_oracle(dev, B):
    from airpose_amd import utils
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(20 + B)
    M = torch.zeros(B, 4, 4)
    M[:, :3, :3] = smplx_ref.batch_rodrigues(torch.randn(B, 3, generator=gen, dtype=torch.float64)).float()
    M[:, :3, 3] = torch.randn(B, 3, generator=gen)
    M[:, 3, 3] = 1.
    inp = [M, torch.randn(B, 500, 3, generator=gen), torch.randn(B, 127, 3, generator=gen),
           smplx_ref.batch_rodrigues(torch.randn(B, 3, generator=gen, dtype=torch.float64)).float(), torch.randn(B, 3, generator=gen)]
    W = [torch.randn(B, 500, 3, generator=gen), torch.randn(B, 127, 3, generator=gen), torch.randn(B, 3, 3, generator=gen),
         torch.randn(B, 3, generator=gen)]
    got, outs = _grads(lambda m, v, j, o, t: utils.transform_smpl(m, v, j, o, t), inp, W, dev)
    want, _ = _grads(_transform_ref, inp, W)
    assert all(o.grad_fn is not None for o in outs)
    assert got[0].shape == (B, 4, 4) and float(got[0][:, 3].abs().max()) == 0.0     # row 3 of trans_mat gets zero
    for name, a, b in zip(("trans_mat", "vertices", "joints", "orientation", "smpltrans"), got, want):
        e = rel_err(a.cpu().numpy(), b.numpy())
        print("transform_smpl B=%d grad %-12s rel err %.3e" % (B, name, e))
        assert e < TOL, name


def test_forward_under_grad_is_bit_identical_and_no_grad_has_no_grad_fn(dev):
    from airpose_amd import geometry, utils
    gen = torch.Generator().manual_seed(5)
    x = _x6(64, gen, 2).to(dev)
    pts, rot, tr, cc = (t.to(dev) for t in _proj_inputs(3, 50, gen))
    M = torch.cat([rot, tr.unsqueeze(2)], 2)
    a = geometry.rot6d_to_rotmat(x)
    b = geometry.rot6d_to_rotmat(x.clone().requires_grad_(True))
    assert a.grad_fn is None and b.grad_fn is not None and torch.equal(a, b.detach())
    a = geometry.perspective_projection(pts, rot, tr, (5000., 5000.), cc)
    b = geometry.perspective_projection(pts, rot, tr, (5000., 5000.), cc.clone().requires_grad_(True))
    assert a.grad_fn is None and b.grad_fn is not None and torch.equal(a, b.detach())
    a = utils.transform_smpl(M, pts, pts[:, :10], rot, tr)
    b = utils.transform_smpl(M.clone().requires_grad_(True), pts, pts[:, :10], rot, tr)
    for u, v in zip(a, b):
        assert u.grad_fn is None and v.grad_fn is not None and torch.equal(u, v.detach())
    with torch.no_grad():
        assert geometry.rot6d_to_rotmat(x.clone().requires_grad_(True)).grad_fn is None


def test_gradients_are_deterministic(dev):
    from airpose_amd import geometry, utils
    gen = torch.Generator().manual_seed(6)
    pts, rot, tr, cc = _proj_inputs(4, 2000, gen)
    W = [torch.randn(4, 2000, 2, generator=gen)]
    fn = lambda p, r, t, c: geometry.perspective_projection(utils.transform_smpl(torch.cat([r, t.unsqueeze(2)], 2), p)[0],
                                                            None, None, (5000., 5000.), c)
    inp = [pts, rot, tr + torch.tensor([0., 0., 10.]), cc]
    g1, _ = _grads(fn, inp, W, dev)
    g2, _ = _grads(fn, inp, W, dev)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    x = _x6(500, gen)
    W = [torch.randn(500, 3, 3, generator=gen)]
    (a,), _ = _grads(geometry.rot6d_to_rotmat, [x], W, dev)
    (b,), _ = _grads(geometry.rot6d_to_rotmat, [x], W, dev)
    assert torch.equal(a, b)
