"""airpose_amd.RealDataLoss on the GPU: the module's plumbing (each trainer's argument order and input_batch keys, the draw of eps,
which gradients are asked for, grad_output, no_grad, the one host copy of the terms) against test_real_loss_fp64's fp64 restatement
and C-ABI runs; the whole fine-tune chain (rot6d pose, betas and translation leaves -> rot6d_to_rotmat -> SMPL-X -> transform_smpl
-> projection -> RealDataLoss("twoview") -> backward) against the same chain in eager torch (the oracle's functions, fp64); and three
FusedAdam steps of that chain next to torch.optim.Adam(amsgrad=True) on the eager chain.

Bars.  Value and seeds of every kind: test_real_loss_fp64.verify.  The chain's leaf gradients: test_head_grad.TOL_GRAD (1e-4, max-norm
relative), as it stands.  The three optimizer steps: test_optim_module's trajectory bar -- its Drift recursion carried through the
exact update at the eager run's state, the measured difference of the two chains' gradients entering as E_g -- on every leaf.
"""
import pytest
import torch

from conftest import rel_err
from loss_util import dev  # noqa: F401  (a fixture)
from real_loss_util import NJ, NZ, PRED, SD, SD64, WEIGHTS, draw_rot6d, loss_terms, make_case, packed  # noqa: F401  (packed: a fixture)
from test_head_grad import TOL_GRAD
from test_optim_module import Drift
from test_real_loss_fp64 import reference, run, verify
from test_stem_pool_fp64 import evaluate

pytestmark = pytest.mark.gpu
# kind -> (the form of test_real_loss_fp64's cases, limbs2d, the weights its trainer declares no default for)
UNDECLARED = dict(limbs2d_loss_weight=1.5, vposer_loss_weight=1.0)
KINDS = {"twoview": ("twoview", 1.5, {}), "twoview_sep": ("twoview", 1.0, {}), "hmr": ("hmr", 1.5, UNDECLARED),
         "hmr_camswap": ("spin", 1.5, UNDECLARED), "spin": ("spin", 1.5, UNDECLARED)}


def _case(kind, B=3, J=25, Jg=24):
    form, l, _ = KINDS[kind]
    w = list(WEIGHTS)
    if form != "twoview":
        w[3] = 0.0                                                          # no pose term with one view: the module passes weight 0
    return make_case(form, B, J, Jg, limbs=l, weights=w)


def _batch(c, dev):
    """the reference's input_batch: the 2-D joints carry the dataloader's singleton dimension"""
    if c["nviews"] == 2:
        return {"smpl_joints_2d%d" % v: c["gt"][v].unsqueeze(1).to(dev) for v in range(2)}
    return {"smpl_joints_2d_crop0": c["gt"][0].unsqueeze(1).to(dev)}


def _leaves(c, dev, requires_grad=True):
    return [{n: t.to(dev).requires_grad_(requires_grad) for n, t in p.items()} for p in c["pred"]]


def _args(c, P):
    """the positional arguments of the kind's get_loss after input_batch (pred_output_cam is not read: None)"""
    if c["nviews"] == 2:
        return (P[0]["depth"], P[1]["depth"], P[0]["rotmat"], P[1]["rotmat"], P[0]["betas"], P[1]["betas"], None, None, P[0]["j2d"], P[1]["j2d"])
    return (P[0]["depth"], P[0]["rotmat"], P[0]["betas"], None, P[0]["j2d"])


def _eps(c, dev):
    return [e.to(dev) for e in c["eps"]]


def _grads(P):
    return [{n: (None if t.grad is None else t.grad.cpu()) for n, t in p.items()} for p in P]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_module_matches_fp64_and_the_c_abi_seeds(dev, packed, kind):
    from airpose_amd import RealDataLoss
    c = _case(kind)
    P = _leaves(c, dev)
    m = RealDataLoss(kind, {"vp_model." + k: v for k, v in SD.items()}, **KINDS[kind][2])
    assert [float(x) for x in c["w"]] == [float(torch.tensor(x, dtype=torch.float32)) for x in m.weight_vector()]
    loss, terms = m(_batch(c, dev), *_args(c, P), eps=_eps(c, dev))
    assert loss.dim() == 0 and loss.requires_grad and terms.shape == (6,) and not terms.requires_grad and terms.is_cuda
    loss.backward()
    got = _grads(P)
    ratios = {}
    fails = verify(c, reference(c), terms.cpu(), got, kind, ratios)
    assert not fails, fails
    assert float(loss.detach()) == float(terms[0])
    assert loss.untyped_storage().data_ptr() != terms.untyped_storage().data_ptr()       # in-place work on terms cannot reach the loss
    abi_terms, abi_grads = run(c, dev, packed)
    assert torch.equal(terms.cpu(), abi_terms)
    for v in range(c["nviews"]):
        for n in PRED:
            assert torch.equal(got[v][n], abi_grads[v][n]), (v, n)
    d = m.losses(terms)
    keys = ["loss", "loss_regul_vposer", "loss_regr_pose", "loss_keypoints", "loss_regul_betas"]
    if c["nviews"] == 1:
        keys.remove("loss_regr_pose")
    assert list(d) == keys and d["loss"] == float(terms[0]) and d["loss_regul_betas"] == float(terms[4])


def test_eps_drawn_from_a_seeded_generator_is_torch_randn_view_0_then_view_1(dev):
    from airpose_amd import RealDataLoss
    c = _case("twoview")
    m = RealDataLoss("twoview", SD)
    g1, g2 = torch.Generator(device=dev).manual_seed(77), torch.Generator(device=dev).manual_seed(77)
    P = _leaves(c, dev)
    loss, terms = m(_batch(c, dev), *_args(c, P), generator=g1)
    loss.backward()
    eps = [torch.randn((c["B"], NZ), device=dev, generator=g2) for _ in range(2)]
    Q = _leaves(c, dev)
    loss2, terms2 = m(_batch(c, dev), *_args(c, Q), eps=eps)
    loss2.backward()
    assert torch.equal(terms.view(torch.int32), terms2.view(torch.int32))
    for a, b in zip(_grads(P), _grads(Q)):
        for n in PRED:
            assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    # the default generator, likewise; and another draw gives another prior term
    torch.manual_seed(5)
    _, t3 = m(_batch(c, dev), *_args(c, Q))
    torch.manual_seed(5)
    eps = [torch.randn((c["B"], NZ), device=dev) for _ in range(2)]
    _, t4 = m(_batch(c, dev), *_args(c, Q), eps=eps)
    assert torch.equal(t3, t4) and float(t3[1]) != float(terms[1])
    with pytest.raises(RuntimeError, match="not both"):
        m(_batch(c, dev), *_args(c, Q), eps=eps, generator=g1)


class _Spy(object):
    """the gradient library with apg_real_loss_fwd_bwd's grads tables recorded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "apg_real_loss_fwd_bwd":
            return fn

        def spy(*a):
            grads = a[12]
            self.calls.append(None if grads is None else [grads[i] for i in range(len(grads))])
            return fn(*a)
        return spy


def test_only_inputs_that_require_grad_get_a_gradient_and_no_grad_allocates_no_seeds(dev, monkeypatch):
    from airpose_amd import RealDataLoss
    from airpose_amd import _native_grad as G
    spy = _Spy(G.lib())
    monkeypatch.setattr(G, "lib", lambda: spy)
    c = _case("twoview")
    m = RealDataLoss("twoview", SD)
    P = _leaves(c, dev, requires_grad=False)
    P[0]["j2d"].requires_grad_(True)
    P[1]["rotmat"].requires_grad_(True)
    loss, _ = m(_batch(c, dev), *_args(c, P), eps=_eps(c, dev))
    table = spy.calls[-1]
    assert len(table) == 8 and [i for i, p in enumerate(table) if p] == [PRED.index("j2d"), 4 + PRED.index("rotmat")]
    loss.backward()
    assert P[0]["j2d"].grad is not None and P[1]["rotmat"].grad is not None and P[0]["rotmat"].grad is None
    with torch.no_grad():
        Q = _leaves(c, dev)
        loss, terms = m(_batch(c, dev), *_args(c, Q), eps=_eps(c, dev))
    assert spy.calls[-1] is None and not loss.requires_grad                # forward only: the grads table itself is NULL
    Q = _leaves(c, dev, requires_grad=False)
    loss2, terms2 = m(_batch(c, dev), *_args(c, Q), eps=_eps(c, dev))
    assert spy.calls[-1] is None and not loss2.requires_grad and torch.equal(terms2, terms)


def test_grad_output_scales_the_seeds(dev, packed):
    from airpose_amd import RealDataLoss
    c = _case("twoview")
    P = _leaves(c, dev)
    loss, _ = RealDataLoss("twoview", SD)(_batch(c, dev), *_args(c, P), eps=_eps(c, dev))
    (2.5 * loss).backward()
    _, seeds = run(c, dev, packed)
    for v in range(2):
        for n in PRED:
            assert torch.equal(P[v][n].grad.cpu(), seeds[v][n] * 2.5), (v, n)


def test_bad_inputs_are_refused_by_name(dev):
    from airpose_amd import RealDataLoss
    c = _case("spin")
    m = RealDataLoss("spin", SD, **UNDECLARED)
    P = _leaves(c, dev, requires_grad=False)
    eps = _eps(c, dev)
    _, want = m(_batch(c, dev), *_args(c, P), eps=eps)
    Q = [dict(P[0], j2d=P[0]["j2d"].transpose(1, 2).contiguous().transpose(1, 2))]       # non-contiguous: made contiguous
    _, got = m(_batch(c, dev), *_args(c, Q), eps=eps[0])
    assert torch.equal(got, want)
    for bad, word in ((dict(j2d=P[0]["j2d"].cpu()), "j2d of view 0"), (dict(rotmat=P[0]["rotmat"][:, :21]), "rotmat of view 0"),
                      (dict(betas=P[0]["betas"].double()), "betas of view 0"), (dict(depth=P[0]["depth"][:, :2]), "depth of view 0")):
        with pytest.raises(RuntimeError, match=word):
            m(_batch(c, dev), *_args(c, [dict(P[0], **bad)]), eps=eps)
    with pytest.raises(RuntimeError, match="smpl_joints_2d_crop0"):
        m({}, *_args(c, P), eps=eps)
    with pytest.raises(RuntimeError, match="eps of view 0"):
        m(_batch(c, dev), *_args(c, P), eps=[eps[0][:, :31]])


def test_losses_dict_is_one_host_copy(dev, monkeypatch):
    from airpose_amd import RealDataLoss
    c = _case("twoview")
    m = RealDataLoss("twoview", SD)
    P = _leaves(c, dev, requires_grad=False)
    batch, args, eps = _batch(c, dev), _args(c, P), _eps(c, dev)
    m(batch, *args, eps=eps)                                               # the encoder is packed on first use
    counts = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy", "to", "__float__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                counts["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    _, terms = m(batch, *args, eps=eps)
    assert counts["n"] == 0, "forward synchronised with the host"
    d = m.losses(terms)
    assert counts["n"] == 1 and all(isinstance(v, float) for v in d.values())


# ------------------------------------------------------------------------------------------------ the whole fine-tune chain
B_CHAIN = 2
CC = [torch.full((1, B_CHAIN, 2), 500.), torch.full((1, B_CHAIN, 2), 520.)]


def _chain(mods, leaves, loss_fn):
    """per view (pose6 (B, 132), betas (B, 10), trans (B, 3)): rot6d, SMPL-X, transform_smpl, projection; then get_loss"""
    rot6d, smplx_fwd, transform, project = mods
    P = []
    for v, (pose6, betas, t) in enumerate(leaves):
        rotmat = rot6d(pose6).view(B_CHAIN, NJ, 3, 3)
        verts, joints = smplx_fwd(betas, rotmat[:, 1:])
        M = torch.cat([rotmat[:, 0], t.unsqueeze(2)], dim=2)
        _, jc = transform(M, verts, joints)
        P.append(dict(depth=t, rotmat=rotmat, betas=betas, j2d=project(jc, CC[v])))
    return loss_fn(P)


def _chain_setup(smplx_model, dev):
    from airpose_amd import geometry, smplx, utils
    from oracle import geometry_ref, smplx_ref
    B = B_CHAIN
    body = smplx.SMPLX(model_data=smplx_model)
    eye = lambda dt, dv: torch.eye(3, dtype=dt, device=dv).expand(B, 1, 3, 3)
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
    g = torch.Generator().manual_seed(31)
    start = []
    for v in range(2):
        x6, _, _ = draw_rot6d(B * NJ, g)
        start.append((x6.reshape(B, NJ * 6).contiguous(), torch.randn(B, 10, generator=g) * 0.5,
                      torch.randn(B, 3, generator=g) * 0.3 + torch.tensor([0., 0., 6.])))
    # the ground truth sits around the start's own projection, with detector confidences (some exactly 0)
    with torch.no_grad():
        proj = _chain(ref, [tuple(t.double() for t in lv) for lv in start], lambda P: [p["j2d"] for p in P])
    J = proj[0].shape[1]
    conf = [torch.rand(B, J, 1, generator=g) for _ in range(2)]
    for cf in conf:
        cf[torch.rand(B, J, 1, generator=g) < 0.2] = 0.0
    gt = [torch.cat([proj[v].float() + torch.randn(B, J, 2, generator=g) * 5, conf[v]], 2).contiguous() for v in range(2)]
    eps = [torch.randn(B, NZ, generator=g) for _ in range(2)]
    c = dict(make_case("twoview", B, J, J), gt=gt, eps=eps)
    return gpu, ref, start, c


def _eager(ref, c, leaves32):
    """the eager chain in fp64 on the leaves' fp32 values -> (loss, gradients cast to fp32)"""
    lv = [tuple(t.detach().double().requires_grad_() for t in view) for view in leaves32]
    loss = _chain(ref, lv, lambda P: loss_terms(c, P, SD64)[0])
    loss.backward()
    return loss.detach(), [tuple(t.grad for t in view) for view in lv]


def test_fine_tune_chain_matches_the_eager_chain(smplx_model, dev):
    from airpose_amd import RealDataLoss
    gpu, ref, start, c = _chain_setup(smplx_model, dev)
    want, gwant = _eager(ref, c, start)
    m = RealDataLoss("twoview", SD)
    batch = {"smpl_joints_2d%d" % v: c["gt"][v].unsqueeze(1).to(dev) for v in range(2)}
    lv = [tuple(t.clone().to(dev).requires_grad_() for t in view) for view in start]
    got = _chain(gpu, lv, lambda P: m(batch, P[0]["depth"], P[1]["depth"], P[0]["rotmat"], P[1]["rotmat"], P[0]["betas"], P[1]["betas"],
                                      None, None, P[0]["j2d"], P[1]["j2d"], eps=[e.to(dev) for e in c["eps"]])[0])
    got.backward()
    print("chain loss %.6f against fp64 %.6f" % (float(got.detach()), float(want)))
    assert abs(float(got.detach()) - float(want)) <= 1e-5 * abs(float(want))
    for v in range(2):
        for k, name in enumerate(("pose6", "betas", "trans")):
            e = rel_err(lv[v][k].grad.cpu().numpy(), gwant[v][k].numpy())
            print("chain + RealDataLoss grad %-6s view %d rel err %.3e" % (name, v, e))
            assert e < TOL_GRAD, (name, v, e)


def test_three_fused_adam_steps_next_to_torch_adam_on_the_eager_chain(smplx_model, dev):
    import test_optim_fp64 as F
    from airpose_amd import FusedAdam, RealDataLoss
    gpu, ref, start, c = _chain_setup(smplx_model, dev)
    lr = 1e-3
    h = F.hyper(lr=lr, wd=0.0, amsgrad=True)
    m = RealDataLoss("twoview", SD)
    batch = {"smpl_joints_2d%d" % v: c["gt"][v].unsqueeze(1).to(dev) for v in range(2)}
    eps = [e.to(dev) for e in c["eps"]]
    pf = [tuple(torch.nn.Parameter(t.clone().to(dev)) for t in view) for view in start]
    pt = [tuple(torch.nn.Parameter(t.clone()) for t in view) for view in start]
    flat = lambda ps: [p for view in ps for p in view]
    of = FusedAdam(flat(pf), lr=lr, weight_decay=0, amsgrad=True)
    ot = torch.optim.Adam(flat(pt), lr=lr, weight_decay=0, amsgrad=True, foreach=False)
    drift = [Drift(p) for p in flat(pt)]
    zero = lambda p: torch.zeros_like(p, dtype=torch.float64)
    worst = 0.0
    for s in range(3):
        of.zero_grad()
        loss = _chain(gpu, pf, lambda P: m(batch, P[0]["depth"], P[1]["depth"], P[0]["rotmat"], P[1]["rotmat"], P[0]["betas"], P[1]["betas"],
                                           None, None, P[0]["j2d"], P[1]["j2d"], eps=eps)[0])
        loss.backward()
        _, gw = _eager(ref, c, pt)
        for p, g in zip(flat(pt), [g for view in gw for g in view]):
            p.grad = g.float()
        for a, b, dr in zip(flat(pt), flat(pf), drift):
            st = ot.state.get(a, {})
            state = dict(p=a.detach().double(), m=st["exp_avg"].double() if st else zero(a), v=st["exp_avg_sq"].double() if st else zero(a),
                         vmax=st["max_exp_avg_sq"].double() if st else zero(a))
            dr.step(state, a.grad.double(), h, s + 1, ("kernel", "torch"), E_g=(b.grad.cpu() - a.grad).abs())
        ot.step()
        of.step()
        torch.cuda.synchronize()
        for i, (a, b, dr) in enumerate(zip(flat(pt), flat(pf), drift)):
            ok, ratio, nz, msg = evaluate(b.detach().cpu(), a.detach().double(), dr.p)
            worst = max(worst, ratio)
            assert ok, ("step %d, leaf %d" % (s, i), msg)
    print("three steps: worst |dp| / bound %.3f" % worst)
    assert not torch.equal(pf[0][0].detach().cpu(), start[0][0])
