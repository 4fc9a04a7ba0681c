"""airpose_amd.EvalMetrics (airpose_amd/eval_metrics.py) and its driver evaluate(): the dict handling of the four trainers' test_step
outputs, the refusals by name and the state round trip on the CPU; update / compute / reset, the ground truth taken from `batch`,
the streams and the driver on the GPU.  The kernel's arithmetic is test_eval_fp64.py's subject; the reference, bars and cases are
eval_util.py's."""
import pytest
import torch

import eval_util as E
from conftest import MEAN_PARAMS
from test_stem_pool_fp64 import evaluate

KINDS = {"twoview": 2, "singleview": 1, "hmr": 1, "muhmr": 2}


@pytest.fixture(scope="module")
def rest(smplx_model):
    from airpose_amd.eval_metrics import rest_joints
    return rest_joints(smplx_model)


def dicts(case, kind, split=False, to=None):
    """the reference's test_step output dict of `kind` from an eval_util case; split: the ground truth goes into a batch dict under
    the batch's names (smpltrans_rel*), as with our TwoViewInference"""
    two = KINDS[kind] == 2
    mv = (lambda t: t) if to is None else (lambda t: t.to(to))
    out, gt = {}, {}
    gt["smplpose_rotmat"] = mv(case["gt_body"])
    for v, d in enumerate(case["view"]):
        s = str(v) if two else ""
        out[("pred_angles" if case["mode"] == "aa" else "pred_rotmat") + s] = mv(d["pred"])
        gt["smplorient_rel" + (s if two else ("0" if kind == "singleview" else ""))] = mv(d["gt_orient"])
        if d["pred_trans"] is not None:
            out["pred_smpltrans" + s] = mv(d["pred_trans"])
            gt[("smpltrans_rel" + (s or "0")) if split else ("gt_smpltrans" + s)] = mv(d["gt_trans"])
        if d["gt_angles"] is not None:
            gt["gt_angles" + s] = mv(d["gt_angles"])
    if split:
        return out, gt
    out.update(gt)
    return out, None


# ------------------------------------------------------------------------------------------------ CPU
def test_exported_and_constructed_without_a_gpu(smplx_model, rest):
    import airpose_amd
    from airpose_amd import eval_metrics
    assert airpose_amd.EvalMetrics is eval_metrics.EvalMetrics
    m = airpose_amd.EvalMetrics(smplx_model, kind="muhmr", device="cuda:0")
    assert m.views == 2 and m.parents == rest[1] and m.parents[0] == -1
    j64 = (torch.as_tensor(smplx_model["J_regressor"]).double() @ torch.as_tensor(smplx_model["v_template"]).double())[:22]
    assert torch.equal(m._j_host, j64.float())
    with pytest.raises(ValueError, match="kind"):
        airpose_amd.EvalMetrics(smplx_model, kind="spin")
    with pytest.raises(RuntimeError, match="no CPU path"):
        airpose_amd.EvalMetrics(smplx_model, device="cpu")
    with pytest.raises(RuntimeError, match="J_regressor"):
        airpose_amd.EvalMetrics({"v_template": smplx_model["v_template"]})


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("mode", ("aa", "rotmat"))
def test_keys_of_the_four_kinds(smplx_model, rest, kind, mode):
    from airpose_amd import EvalMetrics
    from airpose_amd.eval_metrics import ANGLE_AXIS, ROTMAT
    views = KINDS[kind]
    case = E.make_case(rest[0], rest[1], 2, views, mode, True)
    m = EvalMetrics(smplx_model, kind=kind, device="cuda:0")
    for split in (False, True):
        out, batch = dicts(case, kind, split)
        got_mode, body, per_view = m.gather(out, batch)
        assert got_mode == (ANGLE_AXIS if mode == "aa" else ROTMAT)
        assert body[0] == "smplpose_rotmat" and body[1] is case["gt_body"]
        for v, d in enumerate(per_view):
            c = case["view"][v]
            assert d["pred_rot"][1] is c["pred"] and d["gt_orient"][1] is c["gt_orient"]
            assert d["pred_trans"][1] is c["pred_trans"] and d["gt_trans"][1] is c["gt_trans"]
            assert d["gt_trans"][0].startswith("smpltrans_rel" if split else "gt_smpltrans")
            assert (d["gt_angles"] is None) if mode == "rotmat" else (d["gt_angles"][1] is c["gt_angles"])
    # `output` wins over `batch`; without translations and angles nothing optional is picked up
    out, _ = dicts(case, kind)
    other = {k: torch.zeros_like(t) for k, t in out.items()}
    assert all(d["pred_rot"][1] is case["view"][v]["pred"] for v, d in enumerate(m.gather(out, other)[2]))
    bare, _ = dicts(E.make_case(rest[0], rest[1], 2, views, mode, False), kind)
    assert all(d["pred_trans"] is None and d["gt_trans"] is None and d["gt_angles"] is None for d in m.gather(bare)[2])


def test_refusals_by_name(smplx_model, rest):
    from airpose_amd import EvalMetrics
    m = EvalMetrics(smplx_model, kind="twoview", device="cuda:0")
    case = E.make_case(rest[0], rest[1], 3, 2, "aa", True)
    out, _ = dicts(case, "twoview")

    def without(*keys, **repl):
        d = {k: t for k, t in out.items() if k not in keys}
        d.update(repl)
        return d
    with pytest.raises(RuntimeError, match="smplpose_rotmat"):
        m.update(without("smplpose_rotmat"))
    with pytest.raises(RuntimeError, match="smplorient_rel1"):
        m.update(without("smplorient_rel1"))
    with pytest.raises(RuntimeError, match="pred_angles1 or pred_rotmat1"):
        m.update(without("pred_angles1"))
    with pytest.raises(RuntimeError, match="pred_smpltrans0 is given without gt_smpltrans0 / smpltrans_rel0"):
        m.update(without("gt_smpltrans0"))
    with pytest.raises(RuntimeError, match="pred_rotmat1 is given where view 0"):
        m.update(without("pred_angles1", pred_rotmat1=torch.zeros(3, 22, 3, 3)))
    with pytest.raises(RuntimeError, match=r"pred_angles0 must be a tensor"):
        m.update(without(pred_angles0=[1.0]))
    with pytest.raises(RuntimeError, match=r"gt_angles1 must be \(3, 22, 3\), got \(3, 21, 3\)"):
        m.update(without(gt_angles1=torch.zeros(3, 21, 3)))
    with pytest.raises(RuntimeError, match=r"smplorient_rel0 must be \(3, 1, 3, 3\)"):
        m.update(without(smplorient_rel0=torch.zeros(3, 3, 3)))
    with pytest.raises(RuntimeError, match="pred_smpltrans1 must be a floating-point tensor, got torch.int64"):
        m.update(without(pred_smpltrans1=torch.zeros(3, 3, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="smplorient_rel0 lives on cpu"):                  # the first tensor looked at
        m.update(out)
    # single-view kinds read the names without an index
    s = EvalMetrics(smplx_model, kind="hmr", device="cuda:0")
    with pytest.raises(RuntimeError, match="pred_angles / pred_angles0 or pred_rotmat / pred_rotmat0"):
        s.update({"smplpose_rotmat": case["gt_body"], "smplorient_rel": case["view"][0]["gt_orient"]})


def test_state_round_trip_on_the_host(smplx_model):
    from airpose_amd import EvalMetrics
    m = EvalMetrics(smplx_model, kind="twoview", device="cuda:0")
    st = m.state()
    assert st["kind"] == "twoview" and st["acc"].shape == (2, 28) and st["acc"].dtype == torch.float64 and float(st["acc"].abs().max()) == 0
    acc = torch.arange(56, dtype=torch.float64).view(2, 28) / 7
    acc[:, 0], acc[:, 26], acc[:, 27] = 5, 5, 0
    m.load_state({"kind": "twoview", "acc": acc})
    acc2 = m.state()["acc"]
    assert torch.equal(acc2, acc) and acc2 is not acc
    got = m.compute()
    assert got["count"] == 5 and got["mpjpe1"] == float(acc[1, 1]) / (5 * 22) and got["mpe0"] == float(acc[0, 24]) / 5
    assert got["per_joint0"] == [float(x) / 5 for x in acc[0, 2:24]] and len(got["per_joint1"]) == 22
    assert "angle_err0" not in got and "angle_err1" not in got
    # two shards add: the sums are raw
    n = EvalMetrics(smplx_model, kind="twoview", device="cuda:0")
    n.load_state({"acc": acc + m.state()["acc"]})
    assert n.compute()["count"] == 10 and n.compute()["mpjpe0"] == got["mpjpe0"]
    m.reset()
    assert float(m.state()["acc"].abs().max()) == 0 and m.compute()["count"] == 0
    with pytest.raises(RuntimeError, match="kind"):
        m.load_state({"kind": "hmr", "acc": acc})
    with pytest.raises(RuntimeError, match="float64"):
        m.load_state({"acc": acc.float()})
    one = EvalMetrics(smplx_model, kind="singleview", device="cuda:0")
    one.load_state({"acc": acc})
    assert "mpjpe0" in one.compute() and "mpjpe1" not in one.compute()


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda", 0)


def _expected(cases, views):
    refs = [E.reference(c) for c in cases]
    bars = [E.bars(c, r) for c, r in zip(cases, refs)]
    return E.accumulate(refs, bars, views)


def _check_compute(got, acc, abar, views, angles):
    want = E.summarise(acc, views)
    assert got["count"] == int(acc[0, 0])
    for v in range(views):
        n = float(acc[v, 0])
        assert abs(got["mpjpe%d" % v] - want["mpjpe%d" % v]) <= float(abar[v, 1]) / (n * 22)
        assert abs(got["mpe%d" % v] - want["mpe%d" % v]) <= float(abar[v, 24]) / n
        for j in range(22):
            assert abs(got["per_joint%d" % v][j] - float(acc[v, 2 + j]) / n) <= float(abar[v, 2 + j]) / n
        if angles:
            assert abs(got["angle_err%d" % v] - want["angle_err%d" % v]) <= float(abar[v, 25]) / (n * 22)
        else:
            assert "angle_err%d" % v not in got
    if views == 1:
        assert not any(k.endswith("1") for k in got)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode,split", [("twoview", "aa", False), ("twoview", "rotmat", True), ("muhmr", "aa", True),
                                             ("singleview", "aa", True), ("hmr", "aa", False), ("hmr", "rotmat", False)])
def test_update_compute_reset(smplx_model, rest, kind, mode, split):
    """batches of B = 3, 1 and 5 on the reference's keys (ground truth in `output`, or in `batch` under the batch's names)"""
    from airpose_amd import EvalMetrics, smplx
    views = KINDS[kind]
    cases = [E.make_case(rest[0], rest[1], B, views, mode, True, seed=20 + i) for i, B in enumerate((3, 1, 5))]
    acc, abar = _expected(cases, views)
    model = smplx.SMPLX(model_data=smplx_model) if kind == "twoview" else smplx_model       # either form of the model
    m = EvalMetrics(model, kind=kind, device=_dev())
    for c in cases:
        assert m.update(*dicts(c, kind, split, to=_dev())) is None
    got = m.compute()
    _check_compute(got, acc, abar, views, angles=mode == "aa")
    st = m.state()["acc"]
    ok, _, _, msg = evaluate(st, acc, abar)
    assert ok, msg
    m.reset()
    assert m.compute()["count"] == 0 and float(m.state()["acc"].abs().max()) == 0
    for c in cases:                                               # after a reset the same stream gives the same bits
        m.update(*dicts(c, kind, split, to=_dev()))
    assert torch.equal(m.state()["acc"].view(torch.int64), st.view(torch.int64))
    # shards: the first batch here, the other two there, sums added on the host
    a, b = EvalMetrics(smplx_model, kind=kind, device=_dev()), EvalMetrics(smplx_model, kind=kind, device=_dev())
    a.update(*dicts(cases[0], kind, split, to=_dev()))
    for c in cases[1:]:
        b.update(*dicts(c, kind, split, to=_dev()))
    a.load_state({"kind": kind, "acc": a.state()["acc"] + b.state()["acc"]})
    _check_compute(a.compute(), acc, abar, views, angles=mode == "aa")


@pytest.mark.gpu
def test_per_sample_outputs_dtypes_and_device_refusals(smplx_model, rest):
    from airpose_amd import EvalMetrics
    case = E.make_case(rest[0], rest[1], 5, 2, "aa", True, seed=31)
    ref = E.reference(case)
    bar = E.bars(case, ref)
    m = EvalMetrics(smplx_model, kind="twoview", device=_dev(), per_sample=True)
    out, _ = dicts(case, "twoview", to=_dev())
    je, te, ae = m.update(out)
    for got, n in ((je, "joint_err"), (te, "trans_err"), (ae, "angle_err")):
        ok, _, _, msg = evaluate(got.cpu(), ref[n], bar[n])
        assert ok, (n, msg)
    # an fp64 tensor is converted (exactly: it holds fp32 values), a strided view is made contiguous
    wide = dict(out)
    wide["pred_angles0"] = out["pred_angles0"].double()
    padded = torch.zeros(5, 7, device=_dev())
    padded[:, :3] = out["pred_smpltrans1"]
    wide["pred_smpltrans1"] = padded[:, :3]
    je2, te2, ae2 = m.update(wide)
    assert torch.equal(je2, je) and torch.equal(te2, te) and torch.equal(ae2, ae)
    assert m.compute()["count"] == 10
    bare, _ = dicts(E.make_case(rest[0], rest[1], 2, 2, "rotmat", False), "twoview", to=_dev())
    je3, te3, ae3 = EvalMetrics(smplx_model, kind="twoview", device=_dev(), per_sample=True).update(bare)
    assert je3.shape == (2, 2, 22) and te3 is None and ae3 is None
    cpu = dict(out)
    cpu["gt_angles1"] = out["gt_angles1"].cpu()
    with pytest.raises(RuntimeError, match="gt_angles1 lives on cpu"):
        m.update(cpu)
    if torch.cuda.device_count() > 1:
        far = dict(out)
        far["smplpose_rotmat"] = out["smplpose_rotmat"].to("cuda:1")
        with pytest.raises(RuntimeError, match="smplpose_rotmat lives on cuda:1"):
            m.update(far)


@pytest.mark.gpu
def test_side_stream_gives_the_default_streams_bits(smplx_model, rest):
    from airpose_amd import EvalMetrics
    cases = [E.make_case(rest[0], rest[1], B, 2, "aa", True, seed=40 + i) for i, B in enumerate((4, 17))]
    feeds = [dicts(c, "twoview", True, to=_dev()) for c in cases]
    torch.cuda.synchronize()
    a = EvalMetrics(smplx_model, kind="twoview", device=_dev(), per_sample=True)
    outs_a = [a.update(*f) for f in feeds]
    b = EvalMetrics(smplx_model, kind="twoview", device=_dev(), per_sample=True)
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        outs_b = [b.update(*f) for f in feeds]
    side.synchronize()
    assert torch.equal(a.state()["acc"].view(torch.int64), b.state()["acc"].view(torch.int64))
    for x, y in zip(outs_a, outs_b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)


@pytest.mark.gpu
def test_evaluate_equals_update_on_the_materialised_outputs(smplx_model, copenet_sd, rest):
    """three B = 2 batches of the golden synthetic checkpoint behind TwoViewInference.submit: the same numbers, bit for bit, as update
    fed the outputs of pipe(batch, want_angles=True)"""
    from airpose_amd import EvalMetrics, copenet_model, pipeline, smplx
    from airpose_amd import weights as W
    from airpose_amd.eval_metrics import evaluate as run
    dev = _dev()
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    body = smplx.SMPLX(model_data=smplx_model)
    pipe = pipeline.TwoViewInference(net, body)
    batches = []
    for i in range(3):
        b = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(600 + i, 2).items()}
        c = E.make_case(rest[0], rest[1], 2, 2, "aa", True, seed=50 + i)
        b["smplpose_rotmat"] = c["gt_body"].to(dev)
        for v in (0, 1):
            b["smplorient_rel%d" % v] = c["view"][v]["gt_orient"].to(dev)
            b["smpltrans_rel%d" % v] = c["view"][v]["gt_trans"].to(dev)
        batches.append(b)
    direct = EvalMetrics(body, kind="twoview", device=dev)
    for b in batches:
        out = pipe(b, want_angles=True)
        torch.cuda.synchronize()
        assert out["pred_angles0"].shape == (2, 22, 3)
        direct.update({k: (t.clone() if torch.is_tensor(t) else t) for k, t in out.items()}, b)
    want = direct.compute()
    m = EvalMetrics(body, kind="twoview", device=dev)
    got = run(pipe, iter(batches), m)
    assert got == want and got["count"] == 6
    assert all(k in got for k in ("mpjpe0", "mpjpe1", "mpe0", "mpe1", "per_joint0", "per_joint1"))
    assert got["mpjpe0"] > 0 and got["mpe1"] > 0 and "angle_err0" not in got
    assert torch.equal(m.state()["acc"].view(torch.int64), direct.state()["acc"].view(torch.int64))
