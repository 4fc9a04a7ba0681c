"""airpose_amd.TrainingLoss on the GPU: the module's plumbing (the reference's argument orders and input_batch keys, which gradients
are asked for, grad_output, no_grad, double backward, the one host copy of the terms) against test_loss_fp64's fp64 restatement and
C-ABI runs, and the whole training chain (head -> rot6d -> SMPL-X -> transform_smpl -> projection -> the real two-view loss)
against the fp64 oracle chain.

End-to-end bar: every head-parameter gradient within test_head_grad.TOL_GRAD (1e-4, max-norm relative) of the fp64 chain.  Measured
on an MI355X: 1.1e-6 .. 1.6e-6 over the eight parameters, so the bar stands as it is and no eager-torch fallback bar is needed.
"""
import types

import pytest
import torch

from conftest import rel_err
from loss_util import dev  # noqa: F401  (a fixture)
from test_head_grad import PNAMES, TOL_GRAD, _inputs, _net, _sd64
from test_loss_fp64 import KINDS, PRED, WEIGHTS, loss_terms, make_case, reference, run, verify

pytestmark = pytest.mark.gpu
KIND_NAMES = sorted(KINDS)


def _batch(c, dev):
    """the reference's input_batch: meshes, joints and 2-D joints carry the dataloader's singleton dimension"""
    crop = "" if c["trans"] else "_crop"
    G = c["gt"]
    b = {"smplpose_rotmat": G["pose"], "smpl_vertices": G["verts"].unsqueeze(1), "smpl_joints": G["joints"].unsqueeze(1)}
    for v in range(c["nviews"]):
        b["smplorient_rel%d" % v] = G["root"][v]
        b["smpl_joints_2d%s%d" % (crop, v)] = G["j2d"][v].unsqueeze(1)
        if c["trans"]:
            b["smpltrans_rel%d" % v] = G["trans"][v]
    return {k: t.to(dev) for k, t in b.items()}


def _leaves(c, dev, requires_grad=True):
    return [{n: (None if t is None else t.to(dev).requires_grad_(requires_grad)) for n, t in p.items()} for p in c["pred"]]


def _args(c, P, pair=False):
    """the positional arguments of the kind's get_loss after input_batch"""
    out = [(p["joints"], p["verts"]) if pair else types.SimpleNamespace(joints=p["joints"], vertices=p["verts"]) for p in P]
    k = c["kind"]
    if k == "twoview":
        return (P[0]["trans"], P[1]["trans"], P[0]["rotmat"], P[1]["rotmat"], P[0]["betas"], P[1]["betas"], out[0], out[1], P[0]["j2d"], P[1]["j2d"])
    if k == "singleview":
        return (P[0]["trans"], P[0]["rotmat"], P[0]["betas"], out[0], P[0]["j2d"])
    if k == "hmr":
        return (P[0]["cam"], P[0]["rotmat"], P[0]["betas"], out[0], P[0]["j2d"])
    return (P[0]["rotmat"], P[0]["betas"], out[0], P[0]["j2d"], P[0]["cam"], P[1]["rotmat"], P[1]["betas"], out[1], P[1]["j2d"], P[1]["cam"])


def _grads(P):
    return [{n: (None if t is None or t.grad is None else t.grad.cpu()) for n, t in p.items()} for p in P]


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_module_matches_fp64_and_the_c_abi_seeds(dev, kind):
    from airpose_amd import TrainingLoss
    c = make_case(kind, 3, 24, 127, 144)
    P = _leaves(c, dev)
    m = TrainingLoss(kind)
    assert [float(x) for x in c["w"]] == [float(torch.tensor(x, dtype=torch.float32)) for x in m.weight_vector()]
    loss, terms = m(_batch(c, dev), *_args(c, P))
    assert loss.dim() == 0 and loss.requires_grad and terms.shape == (9,) and not terms.requires_grad and terms.is_cuda
    loss.backward()
    ref = reference(c)
    got = _grads(P)
    fails = verify(c, ref, terms.cpu(), got, kind)
    assert not fails, fails
    assert float(loss.detach()) == float(terms[0])
    assert loss.untyped_storage().data_ptr() != terms.untyped_storage().data_ptr()       # in-place work on terms cannot reach the loss
    abi_terms, abi_grads = run(c, dev)
    assert torch.equal(terms.cpu(), abi_terms)
    for v in range(c["nviews"]):
        for n in PRED:
            if abi_grads[v][n] is not None:
                assert torch.equal(got[v][n], abi_grads[v][n]), (v, n)
    # the (joints, vertices) pair in place of the SMPL-X output object
    loss2, terms2 = m(_batch(c, dev), *_args(c, _leaves(c, dev), pair=True))
    assert torch.equal(terms2, terms)


def test_grad_output_scales_the_seeds(dev):
    from airpose_amd import TrainingLoss
    c = make_case("twoview", 3, 24, 23, 22)
    P = _leaves(c, dev)
    loss, _ = TrainingLoss("twoview")(_batch(c, dev), *_args(c, P))
    (2.5 * loss).backward()
    _, seeds = run(c, dev)
    for v in range(2):
        for n in PRED:
            if seeds[v][n] is not None:
                assert torch.equal(P[v][n].grad.cpu(), seeds[v][n] * 2.5), (v, n)


class _Spy(object):
    """the gradient library with apg_loss_fwd_bwd's pointer tables recorded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "apg_loss_fwd_bwd":
            return fn

        def spy(*a):
            grads = a[10]
            self.calls.append(None if grads is None else [grads[i] for i in range(len(grads))])
            return fn(*a)
        return spy


def test_only_inputs_that_require_grad_get_a_gradient(dev, monkeypatch):
    from airpose_amd import TrainingLoss
    from airpose_amd import _native_grad as G
    spy = _Spy(G.lib())
    monkeypatch.setattr(G, "lib", lambda: spy)
    c = make_case("twoview", 3, 24, 23, 22)
    P = _leaves(c, dev, requires_grad=False)
    P[0]["verts"].requires_grad_(True)
    P[1]["betas"].requires_grad_(True)
    m = TrainingLoss("twoview")
    loss, _ = m(_batch(c, dev), *_args(c, P))
    table = spy.calls[-1]
    assert len(table) == 14
    assert [i for i, p in enumerate(table) if p] == [PRED.index("verts"), 7 + PRED.index("betas")]
    loss.backward()
    assert P[0]["verts"].grad is not None and P[1]["betas"].grad is not None and P[0]["betas"].grad is None
    with torch.no_grad():
        P = _leaves(c, dev)
        loss, terms = m(_batch(c, dev), *_args(c, P))
    assert spy.calls[-1] is None and not loss.requires_grad                # forward only: the grads table itself is NULL
    P = _leaves(c, dev, requires_grad=False)
    loss2, terms2 = m(_batch(c, dev), *_args(c, P))
    assert spy.calls[-1] is None and not loss2.requires_grad and torch.equal(terms2, terms)


def test_double_backward_raises(dev):
    from airpose_amd import TrainingLoss
    c = make_case("hmr", 3, 24, 23, 22)
    P = _leaves(c, dev)
    loss, _ = TrainingLoss("hmr")(_batch(c, dev), *_args(c, P))
    g, = torch.autograd.grad(loss, P[0]["verts"], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_bad_inputs_are_made_contiguous_or_refused_by_name(dev):
    from airpose_amd import TrainingLoss
    c = make_case("singleview", 3, 24, 23, 22)
    m = TrainingLoss("singleview")
    P = _leaves(c, dev, requires_grad=False)
    _, want = m(_batch(c, dev), *_args(c, P))
    Q = [dict(P[0])]
    Q[0]["verts"] = P[0]["verts"].transpose(1, 2).contiguous().transpose(1, 2)          # non-contiguous
    Q[0]["betas"] = P[0]["betas"].double()                                               # not fp32 (exactly representable)
    _, got = m(_batch(c, dev), *_args(c, Q))
    assert torch.equal(got, want)
    Q = [dict(P[0], j2d=P[0]["j2d"].cpu())]
    with pytest.raises(RuntimeError, match="j2d of view 0"):
        m(_batch(c, dev), *_args(c, Q))
    Q = [dict(P[0], rotmat=P[0]["rotmat"][:, :21])]
    with pytest.raises(RuntimeError, match="rotmat of view 0"):
        m(_batch(c, dev), *_args(c, Q))
    b = _batch(c, dev)
    del b["smpl_joints_2d0"]
    with pytest.raises(RuntimeError, match="smpl_joints_2d0"):
        m(b, *_args(c, P))


def test_losses_dict_is_one_host_copy(dev, monkeypatch):
    from airpose_amd import TrainingLoss
    counts = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy", "to", "__float__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                counts["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    for kind in KIND_NAMES:
        c = make_case(kind, 3, 24, 23, 22)
        m = TrainingLoss(kind)
        P = _leaves(c, dev, requires_grad=False)
        batch, args = _batch(c, dev), _args(c, P)
        counts["n"] = 0
        _, terms = m(batch, *args)
        assert counts["n"] == 0, "forward synchronised with the host"
        d = m.losses(terms)
        assert counts["n"] == 1
        keys = ["loss", "loss_regr_trans", "loss_keypoints", "loss_keypoints_3d", "loss_regr_shape", "loss_rootrot", "loss_regr_pose",
                "loss_regul_betas"]
        if not c["trans"]:
            keys.remove("loss_regr_trans")
        assert list(d) == keys and all(isinstance(v, float) for v in d.values())
        host = terms.cpu()
        assert d["loss"] == float(host[0]) and d["loss_regul_betas"] == float(host[7])


# ------------------------------------------------------------------------------------------------ the whole training chain
def _chain(mods, pose0, b0, pose1, b1, pos0, pos1, cc, loss_fn):
    """copenet_twoview.py:212-317: trans un-scaling in place, rot6d, SMPL-X, transform_smpl, projection; then get_loss"""
    rot6d, smplx_fwd, transform, project = mods
    B = pose0.shape[0]
    t0, t1 = pose0[:, :3], pose1[:, :3]
    t0 /= 0.05
    t1 /= 0.05
    pos0 /= 0.05
    pos1 /= 0.05
    P = []
    for v, (pose, betas, t) in enumerate(((pose0, b0, t0), (pose1, b1, t1))):
        rotmat = rot6d(pose[:, 3:]).view(B, 22, 3, 3)
        verts, joints = smplx_fwd(betas, rotmat[:, 1:])
        M = torch.cat([rotmat[:, :1].squeeze(1), t.unsqueeze(2)], dim=2)
        _, jc = transform(M, verts, joints)
        P.append(dict(trans=t, rotmat=rotmat, betas=betas, joints=joints, verts=verts, j2d=project(jc, cc[v]), cam=None))
    return loss_fn(P)


def test_training_chain_with_the_real_loss_matches_fp64(copenet_sd, smplx_model, dev):
    from airpose_amd import TrainingLoss, geometry, smplx, utils
    from oracle import copenet_ref, geometry_ref, smplx_ref
    B = 4
    net = _net(copenet_sd, dev).train()
    net.drop1.eval()
    net.drop2.eval()                                             # dropout off: the fp64 chain has no masks
    body = smplx.SMPLX(model_data=smplx_model)
    d = _inputs(B, 500)
    g = torch.Generator().manual_seed(6)
    eye = lambda dt, dv: torch.eye(3, dtype=dt, device=dv).expand(B, 1, 3, 3)
    cc = [torch.full((1, B, 2), 500.), torch.full((1, B, 2), 520.)]
    gpu = (geometry.rot6d_to_rotmat,
           lambda be, bp: (lambda o: (o.vertices, o.joints))(body.forward(betas=be, body_pose=bp, global_orient=eye(torch.float32, dev),
                                                                           transl=torch.zeros(B, 3, device=dev), pose2rot=False)),
           lambda M, v, j: utils.transform_smpl(M, v, j)[:2],
           lambda j, c_: geometry.perspective_projection(j, None, None, (5000., 5000.), c_.to(dev)))
    ref = (geometry_ref.rot6d_to_rotmat,
           lambda be, bp: smplx_ref.smplx_forward(smplx_model, betas=be, body_pose=bp, global_orient=eye(torch.float64, "cpu"),
                                                  transl=torch.zeros(B, 3, dtype=torch.float64), dtype=torch.float64),
           lambda M, v, j: geometry_ref.transform_smpl(M, v, j),
           lambda j, c_: geometry_ref.perspective_projection(j, torch.eye(3, dtype=torch.float64).expand(B, 3, 3),
                                                             torch.zeros(B, 3, dtype=torch.float64), (5000., 5000.),
                                                             c_.double().reshape(-1, 2)))
    # the fp64 chain first: it fixes the shapes of the ground truth
    sd64 = _sd64(net)
    q0, c0, q1, c1 = copenet_ref.ief(sd64, d["xf0"].double(), d["xf1"].double(), d["bb0"].double(), d["bb1"].double(),
                                     d["pos0"].double(), d["pos1"].double(), iters=3)
    case = dict(KINDS["twoview"], kind="twoview", w=torch.tensor(WEIGHTS["twoview"], dtype=torch.float32))
    holder = {}

    def ref_loss(P):
        V, J = P[0]["verts"].shape[1], P[0]["joints"].shape[1]
        r = lambda *s: torch.randn(*s, generator=g)
        holder["gt"] = dict(pose=torch.eye(3).expand(B, 21, 3, 3).contiguous(), joints=P[0]["joints"].detach().float() + r(B, J, 3) * 0.05,
                            verts=P[0]["verts"].detach().float() + r(B, V, 3) * 0.05,
                            root=[torch.eye(3).expand(B, 1, 3, 3).contiguous()] * 2,
                            j2d=[r(B, J, 2) * 100 + 500, r(B, J, 2) * 100 + 500],
                            trans=[r(B, 3) + torch.tensor([0., 0., 200.])] * 2)
        return loss_terms(case, P, holder["gt"])[0]
    want = _chain(ref, q0, c0, q1, c1, d["pos0"].double().clone(), d["pos1"].double().clone(), cc, ref_loss)
    want.backward()
    c = dict(case, gt=holder["gt"])
    batch = _batch(c, dev)
    m = TrainingLoss("twoview")
    pos0, pos1 = d["pos0"].clone().to(dev), d["pos1"].clone().to(dev)
    p0, b0, p1, b1 = net.forward_ief(d["xf0"].to(dev), d["xf1"].to(dev), d["bb0"].to(dev), d["bb1"].to(dev), pos0, pos1, iters=3)
    got = _chain(gpu, p0, b0, p1, b1, pos0, pos1, cc, lambda P: m(batch, *_args(c, P))[0])
    got.backward()
    print("chain loss %.6f against fp64 %.6f" % (float(got), float(want)))
    errs = {}
    for k in PNAMES:
        mod, attr = k.split(".")
        errs[k] = rel_err(getattr(getattr(net, mod), attr).grad.cpu().numpy(), sd64[k].grad.numpy())
        print("chain + TrainingLoss grad %-16s rel err %.3e" % (k, errs[k]))
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)
