"""airpose_amd.MeshMetrics (airpose_amd/mesh_metrics.py) and its driver evaluate() on the GPU: update / compute / reset on a synthetic
TwoViewInference-shaped output and batch against align_util.reference()'s batch means, the state round trip, shards, per-sample
outputs, and EvalMetrics and MeshMetrics scoring one pass.  The kernel's arithmetic is test_align_fp64.py's subject, the dict handling
and the refusals without a GPU test_align_abi.py's; the reference, bars and cases are align_util.py's."""
import numpy as np
import pytest
import torch

import align_util as A
from conftest import MEAN_PARAMS

VIEWS = {"twoview": 2, "singleview": 1, "hmr": 1, "muhmr": 2}
NJ, J_PRED = 22, 25                                      # joints compared; joints the prediction carries


def _dev():
    return torch.device("cuda", 0)


def make_pair(views, B, V, seed):
    """(joint case, vertex case) of align_util: the vertex case's roots are joint 0 of the joint sets, as MeshMetrics passes them;
    the joint case's own roots are its joint 0 too"""
    cj = A.make_case(views, B, NJ, False, seed=seed)
    cv = A.make_case(views, B, V, False, seed=seed + 1000)
    for v in range(views):
        for c in (cj, cv):
            c["view"][v]["pred_root"] = cj["view"][v]["pred"][:, :3].copy()
            c["view"][v]["gt_root"] = cj["view"][v]["gt"][:, :3].copy()
    return cj, cv


def dicts(cj, cv, kind, to, verts=True):
    """output as TwoViewInference emits it (pred_j3d_cam* with J_PRED joints, pred_vertices_cam*) and the batch as the dataset
    carries it ((B, 1, ., 3))"""
    two = VIEWS[kind] == 2
    B, V = cj["B"], cv["N"]
    out, batch = {}, {}
    for v in range(cj["views"]):
        s = str(v) if two else ""
        pj = np.full((B, J_PRED, 3), A.PAD, np.float32)
        pj[:, :NJ] = A.points(cj, v, "pred")
        out["pred_j3d_cam" + s] = torch.from_numpy(pj).to(to)
        batch["smpl_joints_rel" + (s or "0")] = torch.from_numpy(A.points(cj, v, "gt").reshape(B, 1, NJ, 3).copy()).to(to)
        if verts:
            out["pred_vertices_cam" + s] = torch.from_numpy(A.points(cv, v, "pred").copy()).to(to)
            batch["smpl_vertices_rel" + (s or "0")] = torch.from_numpy(A.points(cv, v, "gt").reshape(B, 1, V, 3).copy()).to(to)
    return out, batch


def expected(pairs, views):
    """per point set (accumulator, its bar) of a sequence of (joint case, vertex case)"""
    res = []
    for k in (0, 1):
        refs = [A.reference(p[k]) for p in pairs]
        bars = [A.bars(p[k], r) for p, r in zip(pairs, refs)]
        res.append(A.accumulate(refs, bars, [(True, True)] * len(pairs), views) + (refs, bars))
    return res


def check_compute(got, exp, views, verts=True):
    labels = (("mpjpe_abs", "mpjpe_root", "pa_mpjpe"), ("pve_abs", "pve_root", "pa_pve"))
    assert got["count"] == int(exp[0][0][0, 0])
    for k in (0, 1):
        acc, bar = exp[k][0], exp[k][1]
        for v in range(views):
            n = acc[v, 0]
            for i, name in enumerate(labels[k]):
                key = "%s%d" % (name, v)
                if k == 1 and not verts:
                    assert key not in got
                    continue
                assert np.isfinite(bar[v, 1 + i]), "a collinear sample's pa has no bar: pick another seed"
                assert abs(got[key] - acc[v, 1 + i] / n) <= bar[v, 1 + i] / n, (key, got[key], acc[v, 1 + i] / n, bar[v, 1 + i] / n)
    if views == 1:
        assert not any(k.endswith("1") for k in got)


def regular_pairs(views, V, sizes, seed):
    """pairs whose samples all carry a pa bar (no collinear kind): the batch means are then pinned on every column"""
    kinds = [k for k in A.KINDS if k != "collinear"]
    pairs = []
    for i, B in enumerate(sizes):
        ks = [[kinds[(b + 2 * v + i) % len(kinds)] for b in range(B)] for v in range(views)]
        cj = A.make_case(views, B, NJ, False, seed=seed + i, kinds=ks)
        cv = A.make_case(views, B, V, False, seed=seed + 100 + i, kinds=ks)
        for v in range(views):
            for c in (cj, cv):
                c["view"][v]["pred_root"] = cj["view"][v]["pred"][:, :3].copy()
                c["view"][v]["gt_root"] = cj["view"][v]["gt"][:, :3].copy()
        pairs.append((cj, cv))
    return pairs


@pytest.fixture(scope="module")
def n_vertices(smplx_model):
    return int(torch.as_tensor(smplx_model["v_template"]).shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("twoview", "muhmr", "singleview", "hmr"))
def test_update_compute_reset_state_and_shards(n_vertices, kind):
    """batches of B = 3, 1 and 5 against the reference's batch means; reset; state -> load_state -> compute; two shards added"""
    from airpose_amd import MeshMetrics
    views = VIEWS[kind]
    pairs = regular_pairs(views, n_vertices, (3, 1, 5), seed=20)
    exp = expected(pairs, views)
    m = MeshMetrics(kind=kind, device=_dev())
    feeds = [dicts(cj, cv, kind, _dev()) for cj, cv in pairs]
    for f in feeds:
        assert m.update(*f) is None
    got = m.compute()
    check_compute(got, exp, views)
    st = m.state()
    assert st["kind"] == kind and st["n_joints"] == NJ and st["acc"].shape == (2, 2, 5) and st["acc"].dtype == torch.float64
    for k in (0, 1):
        A.check(st["acc"][k].numpy(), exp[k][0], exp[k][1], "state of set %d" % k)
    fresh = MeshMetrics(kind=kind, device=_dev())
    fresh.load_state(st)
    assert fresh.compute() == got
    fresh.update(*feeds[1])                                       # a loaded state goes on accumulating on the device
    assert fresh.compute()["count"] == got["count"] + 1
    m.reset()
    assert m.compute()["count"] == 0 and float(m.state()["acc"].abs().max()) == 0
    for f in feeds:                                               # after a reset the same stream gives the same bits
        m.update(*f)
    assert torch.equal(m.state()["acc"].view(torch.int64), st["acc"].view(torch.int64))
    a, b = MeshMetrics(kind=kind, device=_dev()), MeshMetrics(kind=kind, device=_dev())
    a.update(*feeds[0])
    for f in feeds[1:]:
        b.update(*f)
    a.load_state({"kind": kind, "acc": a.state()["acc"] + b.state()["acc"]})
    check_compute(a.compute(), exp, views)


@pytest.mark.gpu
def test_joints_alone_and_the_ground_truth_in_output(n_vertices):
    from airpose_amd import MeshMetrics
    pairs = regular_pairs(2, n_vertices, (4,), seed=30)
    exp = expected(pairs, 2)
    out, batch = dicts(pairs[0][0], pairs[0][1], "twoview", _dev(), verts=False)
    out.update(batch)
    m = MeshMetrics(kind="twoview", device=_dev())
    m.update(out)
    check_compute(m.compute(), exp, 2, verts=False)
    assert float(m.state()["acc"][1].abs().max()) == 0


@pytest.mark.gpu
def test_per_sample_outputs_dtypes_and_device_refusals(n_vertices):
    from airpose_amd import MeshMetrics
    cj, cv = make_pair(2, 6, n_vertices, seed=31)                # every kind, the collinear one included
    refs = [A.reference(c) for c in (cj, cv)]
    bars = [A.bars(c, r) for c, r in zip((cj, cv), refs)]
    m = MeshMetrics(kind="twoview", device=_dev(), per_sample=True)
    out, batch = dicts(cj, cv, "twoview", _dev())
    je, ve, tr = m.update(out, batch)
    assert je.shape == (2, 6, 3) and ve.shape == (2, 6, 3) and tr.shape == (2, 6, 13) and je.dtype == torch.float32
    A.check(je.cpu().numpy(), refs[0]["err"], bars[0]["err"], "joint_err")
    A.check(ve.cpu().numpy(), refs[1]["err"], bars[1]["err"], "vertex_err")
    A.check(tr.cpu().numpy(), refs[0]["transform"], bars[0]["transform"], "transform")
    A.check_rotations(tr.cpu().numpy(), bars[0]["cls"], "transform")
    # an fp64 tensor is converted (exactly: it holds fp32 values), a strided view is made contiguous
    wide = dict(out)
    wide["pred_vertices_cam0"] = out["pred_vertices_cam0"].double()
    big = torch.zeros(6, J_PRED + 3, 3, device=_dev())
    big[:, :J_PRED] = out["pred_j3d_cam1"]
    wide["pred_j3d_cam1"] = big[:, :J_PRED]
    je2, ve2, tr2 = m.update(wide, batch)
    assert torch.equal(je2, je) and torch.equal(ve2, ve) and torch.equal(tr2, tr)
    assert m.compute()["count"] == 12
    je3, ve3, tr3 = MeshMetrics(kind="twoview", device=_dev(), per_sample=True).update(
        {k: t for k, t in out.items() if "vertices" not in k}, {k: t for k, t in batch.items() if "vertices" not in k})
    assert torch.equal(je3, je) and ve3 is None and torch.equal(tr3, tr)
    cpu = dict(batch)
    cpu["smpl_vertices_rel1"] = batch["smpl_vertices_rel1"].cpu()
    with pytest.raises(RuntimeError, match="smpl_vertices_rel1 lives on cpu"):
        m.update(out, cpu)
    assert m.compute()["count"] == 12                             # a refused update adds nothing
    if torch.cuda.device_count() > 1:
        far = dict(out)
        far["pred_j3d_cam0"] = out["pred_j3d_cam0"].to("cuda:1")
        with pytest.raises(RuntimeError, match="pred_j3d_cam0 lives on cuda:1"):
            m.update(far, batch)


@pytest.mark.gpu
def test_side_stream_gives_the_default_streams_bits(n_vertices):
    from airpose_amd import MeshMetrics
    feeds = [dicts(*make_pair(2, B, n_vertices, seed=40 + i), "twoview", _dev()) for i, B in enumerate((4, 7))]
    torch.cuda.synchronize()
    a = MeshMetrics(kind="twoview", device=_dev(), per_sample=True)
    outs_a = [a.update(*f) for f in feeds]
    b = MeshMetrics(kind="twoview", device=_dev(), per_sample=True)
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        outs_b = [b.update(*f) for f in feeds]
    side.synchronize()
    assert torch.equal(a.state()["acc"].view(torch.int64), b.state()["acc"].view(torch.int64))
    for x, y in zip(outs_a, outs_b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)


@pytest.mark.gpu
def test_evaluate_scores_one_pass_for_both_metric_classes(smplx_model, copenet_sd):
    """three B = 2 batches of the golden synthetic checkpoint behind TwoViewInference.submit: mesh_metrics.evaluate with an
    EvalMetrics and a MeshMetrics gives each the numbers it gets alone (EvalMetrics through its own evaluate, MeshMetrics through
    update on the materialised outputs), bit for bit"""
    import eval_util as E
    from airpose_amd import EvalMetrics, MeshMetrics, copenet_model, pipeline, smplx
    from airpose_amd import weights as W
    from airpose_amd.eval_metrics import evaluate as run_one, rest_joints
    from airpose_amd.mesh_metrics import evaluate as run_many
    dev = _dev()
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    body = smplx.SMPLX(model_data=smplx_model)
    pipe = pipeline.TwoViewInference(net, body)
    rest = rest_joints(smplx_model)
    gen = torch.Generator().manual_seed(7)
    batches = []
    for i in range(3):
        b = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(700 + i, 2).items()}
        c = E.make_case(rest[0], rest[1], 2, 2, "aa", True, seed=60 + i)
        b["smplpose_rotmat"] = c["gt_body"].to(dev)
        out = pipe(b, want_angles=True)
        torch.cuda.synchronize()
        for v in (0, 1):
            b["smplorient_rel%d" % v] = c["view"][v]["gt_orient"].to(dev)
            b["smpltrans_rel%d" % v] = c["view"][v]["gt_trans"].to(dev)
            for src, dst in (("pred_j3d_cam%d", "smpl_joints_rel%d"), ("pred_vertices_cam%d", "smpl_vertices_rel%d")):
                p = out[src % v].detach().cpu()
                b[dst % v] = (p + 0.02 * torch.randn(p.shape, generator=gen)).unsqueeze(1).to(dev)
        batches.append(b)
    alone_mesh = MeshMetrics(kind="twoview", device=dev)
    for b in batches:
        out = pipe(b, want_angles=True)
        torch.cuda.synchronize()
        alone_mesh.update({k: (t.clone() if torch.is_tensor(t) else t) for k, t in out.items()}, b)
    want_mesh = alone_mesh.compute()
    want_eval = run_one(pipe, iter(batches), EvalMetrics(body, kind="twoview", device=dev))
    em, mm = EvalMetrics(body, kind="twoview", device=dev), MeshMetrics(kind="twoview", device=dev)
    got_eval, got_mesh = run_many(pipe, iter(batches), [em, mm])
    assert got_eval == want_eval and got_mesh == want_mesh
    assert got_mesh["count"] == 6 and got_eval["count"] == 6
    assert torch.equal(mm.state()["acc"].view(torch.int64), alone_mesh.state()["acc"].view(torch.int64))
    for k in ("mpjpe_abs0", "mpjpe_root1", "pa_mpjpe0", "pve_abs1", "pve_root0", "pa_pve1"):
        assert 0 < got_mesh[k] < 0.1, (k, got_mesh[k])            # 2 cm of noise per coordinate
