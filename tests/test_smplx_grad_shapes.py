"""The SMPL-X adjoint (ap_smplx_bwd: smplx_bwd.hip and its driver) and ap_batch_rodrigues_bwd through SMPLX.forward autograd
and lbs.batch_rodrigues, against fp64 autograd through oracle/smplx_ref.py, slice by slice, at the batch sizes, gradient
subsets, blend precisions, bone counts and vertex counts that tests/test_smplx_grad.py (one number per tensor, 1e-4, B <= 5, the
10475-vertex 4-bone model, bf16x2) does not reach.

The adjoint is not linear in its inputs, so there is no clean magnitude bound; the bar is per slice instead.  A slice is one
joint's 3 x 3 block of a pose gradient (over the batch), one column of betas, expression or transl, or one row of a
batch_rodrigues gradient; its error is max |got - fp64| / max |fp64| over the slice.  Bar of a slice: four times the error of the
fp32 CPU oracle (the same oracle, run in fp32 on the same inputs) on that slice, with a floor of 1e-5 -- the rule of
tests/test_trunk_grad.py's n = 1 statistics.  The fp32 CPU oracle's own worst slice is 2.6e-6 at B = 3, so the floor is what
binds almost everywhere and the fp64 reference sits well inside it.  The whole-tensor 1e-4 of the existing file stays as an
outer cap.  Every GPU call runs twice and the two results must be equal bit for bit.

Cases: B in {1, 5, 64, 65, 77} with hands and face and body-only; global_orient only (no coefficient kernel), transl only,
expression only, body_pose only with joints-only upstream, vertices-only upstream; both blend precisions; models with up to 6
and 9 bones per vertex; models of 1024, 1025, 2731 and 5000 vertices (one vertex range, a range of one vertex, 3V off a multiple
of 16); batch_rodrigues at n in {1, 256, 257, 55 x 40} with angles from {0, 1e-6, 1e-3, 1, 3.1}.  Nothing of the issue's list
was trimmed; the forward accepts every vertex count (each such case first holds the forward against the oracle)."""
import pytest
import torch

from conftest import rel_err
from grad_shapes_util import check_slices
from test_smplx_grad import TOL32, _gpu_grads, _loss, _rotmat_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def body(smplx_model, dev):
    from airpose_amd import smplx
    return smplx.SMPLX(model_data=smplx_model)


def _weights(B, V, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, V, 3, generator=gen), torch.randn(B, 127, 3, generator=gen)


def _cpu_grads(model, inp, want, Wv, Wj, use_v, use_j, dtype):
    from oracle import smplx_ref
    leaves = {k: v.to(dtype).clone().requires_grad_(k in want) for k, v in inp.items()}
    v, j = smplx_ref.smplx_forward(model, **leaves, dtype=dtype)
    _loss(v, j, Wv.to(dtype), Wj.to(dtype), use_v, use_j).backward()
    return {k: leaves[k].grad for k in want}, v.detach(), j.detach()


def _run(body, model, dev, inp, want, seed, what, use_v=True, use_j=True, check_forward=False):
    """GPU gradients (twice), the oracle's in fp64 and in fp32, the per-slice bar and the whole-tensor cap"""
    B, V = inp["betas"].shape[0], model["v_template"].shape[0]
    Wv, Wj = _weights(B, V, seed)
    kw = dict(pose2rot=False) if use_v else dict(pose2rot=False, return_verts=False)
    got, leaves, out = _gpu_grads(body, dev, inp, want, Wv, Wj, use_v, use_j, **kw)
    again, _, _ = _gpu_grads(body, dev, inp, want, Wv, Wj, use_v, use_j, **kw)
    torch.cuda.synchronize()
    r64, v64, j64 = _cpu_grads(model, inp, want, Wv, Wj, use_v, use_j, torch.float64)
    r32, _, _ = _cpu_grads(model, inp, want, Wv, Wj, use_v, use_j, torch.float32)
    if check_forward:
        ev, ej = rel_err(out.vertices.detach().cpu().numpy(), v64.numpy()), rel_err(out.joints.detach().cpu().numpy(), j64.numpy())
        print("%-40s forward rel err verts %.3e joints %.3e" % (what, ev, ej))
        assert ev < TOL32 and ej < TOL32, (what, "the forward itself is off", ev, ej)
    for k in inp:
        if k not in want:
            assert leaves[k].grad is None, (what, k, "a gradient nobody asked for")
    ratios = {}
    for k in want:
        assert got[k] is not None and got[k].shape == r64[k].shape, (what, k)
        assert torch.equal(got[k], again[k]), (what, k, "two identical calls differ")
        e = rel_err(got[k].cpu().numpy(), r64[k].numpy())
        assert e < TOL32, (what, k, "whole-tensor rel err %.3e" % e)
        check_slices(what, k, got[k], r64[k], r32[k], 1, ratios)
    print("%-40s worst slice err/bar: %s | worst slice err: %s" % (
        what, "  ".join("%s %.3f" % (k, ratios[k]) for k in want), "  ".join("%s %.2e" % (k, ratios[k + " err"]) for k in want)))
    return ratios


# ------------------------------------------------------------------------------------------------ batch size
@pytest.mark.parametrize("extra", [True, False], ids=["hands-face", "body"])
@pytest.mark.parametrize("B", [1, 5, 64, 65, 77])
def test_batch_sizes(body, smplx_model, dev, B, extra):
    """accuracy, not only invariance: B = 64 fills the coefficient kernel's body tile, 65 starts a second one"""
    inp = _rotmat_inputs(B, 2000 + B, extra)
    _run(body, smplx_model, dev, inp, tuple(inp), 21 + B, "B=%d %s" % (B, "hands/face" if extra else "body"))


# ------------------------------------------------------------------------------------------------ gradient subsets
@pytest.mark.parametrize("extra", [True, False], ids=["hands-face", "body"])
def test_gradient_subsets(body, smplx_model, dev, extra):
    B = 3
    inp = _rotmat_inputs(B, 2100 + int(extra), extra)
    tag = "hands/face" if extra else "body"
    _run(body, smplx_model, dev, inp, ("global_orient",), 31, "global_orient only (nsplit = 0) " + tag)
    _run(body, smplx_model, dev, inp, ("transl",), 32, "transl only " + tag)
    _run(body, smplx_model, dev, inp, ("expression",), 33, "expression only " + tag)
    _run(body, smplx_model, dev, inp, ("body_pose",), 34, "body_pose only, joints upstream " + tag, use_v=False)
    _run(body, smplx_model, dev, inp, tuple(inp), 35, "vertices upstream only " + tag, use_j=False)
    _run(body, smplx_model, dev, inp, ("global_orient",), 36, "global_orient only, joints upstream " + tag, use_v=False)


# ------------------------------------------------------------------------------------------------ blend precision
@pytest.mark.parametrize("precision", ["fp32", "bf16x2"])
def test_blend_precisions(body, smplx_model, dev, precision):
    """the backward recomputes v_posed through the forward's blend GEMM in the handle's precision"""
    inp = _rotmat_inputs(5, 2200, True)
    body.set_blend_precision(precision)
    try:
        _run(body, smplx_model, dev, inp, tuple(inp), 41, "blend %s B=5" % precision, check_forward=True)
    finally:
        body.set_blend_precision("bf16x2")


# ------------------------------------------------------------------------------------------------ bones per vertex
@pytest.mark.parametrize("max_bones", [6, 9])
def test_more_than_four_bones_per_vertex(dev, max_bones):
    from airpose_amd import smplx
    from airpose_amd import smplx_model as SM
    md = SM.make_synthetic_model(4321, max_bones=max_bones)
    assert (md["lbs_weights"] != 0).sum(1).max() == max_bones
    b = smplx.SMPLX(model_data=md)
    for extra in (True, False):
        inp = _rotmat_inputs(3, 2300 + max_bones, extra)
        _run(b, md, dev, inp, tuple(inp), 51, "max_bones=%d %s" % (max_bones, "hands/face" if extra else "body"), check_forward=True)


# ------------------------------------------------------------------------------------------------ vertex counts
@pytest.mark.parametrize("V", [1024, 1025, 2731, 5000])
def test_vertex_counts(dev, V):
    """1024: one vertex range and 3V = 3 reduction splits exactly; 1025: a second range of one vertex; 2731: 3V = 8193, a last
    reduction split of one row inside a 16-row pad; 5000: 3V = 15000 = 16 x 937 + 8"""
    from airpose_amd import smplx
    from airpose_amd import smplx_model as SM
    md = SM.make_synthetic_model(4321, num_verts=V)
    b = smplx.SMPLX(model_data=md)
    for B, extra in ((3, True), (3, False), (65, True)):
        inp = _rotmat_inputs(B, 2400 + V % 97 + B, extra)
        _run(b, md, dev, inp, tuple(inp), 61, "V=%d B=%d %s" % (V, B, "hands/face" if extra else "body"), check_forward=True)
    _run(b, md, dev, _rotmat_inputs(2, 2500, False), ("global_orient", "transl"), 62, "V=%d global_orient + transl" % V)


# ------------------------------------------------------------------------------------------------ batch_rodrigues
@pytest.mark.parametrize("n", [1, 256, 257, 55 * 40])
def test_batch_rodrigues_backward(dev, n):
    from airpose_amd import lbs
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(700 + n)
    angles = torch.tensor([0.0, 1e-6, 1e-3, 1.0, 3.1])
    worst = {}
    for first in range(5 if n == 1 else 1):                  # n = 1: each angle on its own
        ang = angles[(torch.arange(n) + first) % 5]
        ang = ang[torch.randperm(n, generator=gen)] if n > 5 else ang
        d = torch.randn(n, 3, generator=gen)
        aa = d / d.norm(dim=1, keepdim=True) * ang.unsqueeze(1)
        W = torch.randn(n, 3, 3, generator=gen)
        got = []
        for _ in range(2):
            x = aa.to(dev).requires_grad_(True)
            (lbs.batch_rodrigues(x) * W.to(dev)).sum().backward()
            got.append(x.grad)
        torch.cuda.synchronize()
        assert torch.equal(got[0], got[1]), (n, "two identical calls differ")
        refs = []
        for dt in (torch.float64, torch.float32):
            y = aa.to(dt).requires_grad_(True)
            (smplx_ref.batch_rodrigues(y) * W.to(dt)).sum().backward()
            refs.append(y.grad)
        assert rel_err(got[0].cpu().numpy(), refs[0].numpy()) < TOL32
        for a in angles.tolist():                            # rows are the slices, reported per angle
            idx = (ang == a).nonzero().flatten()
            if idx.numel():
                check_slices((n, a), "angle %g" % a, got[0].cpu()[idx], refs[0][idx], refs[1][idx], 0, worst)
    print("batch_rodrigues n=%d worst row err/bar: %s | worst row err: %s" % (
        n, "  ".join("%s %.3f" % kv for kv in worst.items() if not kv[0].endswith(" err")),
        "  ".join("%s %.2e" % (k[:-4], v) for k, v in worst.items() if k.endswith(" err"))))
