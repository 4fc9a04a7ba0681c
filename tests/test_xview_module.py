"""airpose_amd.CrossViewMetrics (airpose_amd/cross_view_metrics.py) and geometry.lstsq_triangulation.  CPU part: the export, the
constructor, every refusal by name, the state round trip and summarise on hand-made sums, without a GPU.  GPU part: the class against
xview_util.reference() through update / compute, the same through _stream_metric.evaluate next to a MeshMetrics on one submit stream,
the class on an AirPosePlusSequence.export-shaped dict, and geometry.lstsq_triangulation against the reference function's arithmetic.
The reference and the bars are test_xview_fp64.py's."""
import numpy as np
import pytest
import torch

import xview_util as X
from conftest import MEAN_PARAMS


def _dev():
    return torch.device("cuda", 0)


def _case(B=3, V=40, rot="rotmat", seed=3):
    return X.make_case(B, 22, 25, V, False, rot, "trans", seed=seed, kinds=(["consistent", "shifted", "zero_conf", "narrow", "nonortho"] * 2)[:B])


# ------------------------------------------------------------------------------------------------ CPU
def test_class_is_exported_and_constructed_without_a_gpu():
    import airpose_amd
    from airpose_amd import cross_view_metrics
    assert airpose_amd.CrossViewMetrics is cross_view_metrics.CrossViewMetrics
    m = airpose_amd.CrossViewMetrics(device="cuda:0")
    assert m.views == 2 and m.n_joints == 22 and m.root == "trans" and m.min_ray_angle_deg == 1.0
    assert abs(m.min_sin2 - X.MIN_SIN2) < 1e-18
    assert airpose_amd.CrossViewMetrics(n_joints=14, root="joint0", min_ray_angle_deg=0, device="cuda:0").min_sin2 == 0.0
    with pytest.raises(ValueError, match="n_joints"):
        airpose_amd.CrossViewMetrics(n_joints=0)
    with pytest.raises(ValueError, match="root"):
        airpose_amd.CrossViewMetrics(root="pelvis")
    with pytest.raises(ValueError, match="min_ray_angle_deg"):
        airpose_amd.CrossViewMetrics(min_ray_angle_deg=-1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        airpose_amd.CrossViewMetrics(device="cpu")
    got = m.compute()
    assert got == {"count": 0, "skipped": 0}
    assert "1 degree" in cross_view_metrics.CrossViewMetrics.__doc__ and "0.4 m" in cross_view_metrics.CrossViewMetrics.__doc__
    assert "cam1_wrt_cam0" in cross_view_metrics.CrossViewMetrics.__doc__


def test_class_refuses_by_name():
    from airpose_amd import CrossViewMetrics
    m = CrossViewMetrics(device="cuda:0")
    out, batch = X.dicts_of(_case())

    def without(*keys, **repl):
        d = {k: t for k, t in list(out.items()) + list(batch.items()) if k not in keys}
        d.update(repl)
        return d
    got = m.gather(out, batch)
    assert got["vertices"][1][1] is out["pred_vertices_cam1"] and got["extr"][0][1] is batch["extr0"] and got["rot_kind"] == "rotmat"
    assert m.gather(without("pred_vertices_cam0", "pred_vertices_cam1"))["vertices"] is None
    with pytest.raises(RuntimeError, match=r"CrossViewMetrics\(twoview\): neither output nor batch has pred_j3d_cam1 \(the predicted joints\)"):
        m.update(without("pred_j3d_cam1"))
    with pytest.raises(RuntimeError, match="neither output nor batch has extr0"):
        m.update(out, {k: t for k, t in batch.items() if k != "extr0"})
    for gone, other in (("pred_vertices_cam1", "pred_vertices_cam0"), ("pred_smpltrans0", "pred_smpltrans1"), ("pred_rotmat1", "pred_rotmat0"),
                        ("pred_j2d_cam0", "pred_j2d_cam1"), ("smpl_joints_2d1", "smpl_joints_2d0"), ("intr0", "intr1")):
        with pytest.raises(RuntimeError, match=r"%s is given for one view only .%s is missing" % (other, gone)):
            m.update(without(gone))
    with pytest.raises(RuntimeError, match='neither output nor batch has pred_smpltrans0 .the roots of root="trans"'):
        m.update(without("pred_smpltrans0", "pred_smpltrans1"))
    CrossViewMetrics(root="joint0", device="cuda:0").gather(without("pred_smpltrans0", "pred_smpltrans1"))
    with pytest.raises(RuntimeError, match="pred_j2d_cam0 is given without smpl_joints_2d0"):
        m.update(without("smpl_joints_2d0", "smpl_joints_2d1"))
    with pytest.raises(RuntimeError, match="pred_j3d_cam0 must be a tensor"):
        m.update(without(pred_j3d_cam0=[1.0]))
    with pytest.raises(RuntimeError, match=r"pred_j3d_cam1 must be \(3, at least 22, 3\), got \(3, 21, 3\)"):
        m.update(without(pred_j3d_cam1=torch.zeros(3, 21, 3)))
    with pytest.raises(RuntimeError, match=r"extr1 must be \(3, 4, 4\) or \(3, 3, 4\), got \(3, 4, 3\)"):
        m.update(without(extr1=torch.zeros(3, 4, 3)))
    with pytest.raises(RuntimeError, match=r"pred_vertices_cam1 must be \(3, at least 1, 3\), got \(3, 40, 2\)"):
        m.update(without(pred_vertices_cam1=torch.zeros(3, 40, 2)))
    with pytest.raises(RuntimeError, match=r"pred_smpltrans0 must be \(3, 3\), got \(3, 4\)"):
        m.update(without(pred_smpltrans0=torch.zeros(3, 4)))
    with pytest.raises(RuntimeError, match=r"pred_rotmat0 must be \(3, 22, 3, 3\), got \(3, 21, 3, 3\)"):
        m.update(without(pred_rotmat0=torch.zeros(3, 21, 3, 3)))
    with pytest.raises(RuntimeError, match=r"pred_angles1 must be \(3, 22, 3\), got \(3, 22, 4\)"):
        m.update(without("pred_rotmat0", "pred_rotmat1", pred_angles0=torch.zeros(3, 22, 3), pred_angles1=torch.zeros(3, 22, 4)))
    with pytest.raises(RuntimeError, match=r"pred_j2d_cam0 must be \(3, at least 22, 2\), got \(3, 25, 3\)"):
        m.update(without(pred_j2d_cam0=torch.zeros(3, 25, 3)))
    with pytest.raises(RuntimeError, match=r"smpl_joints_2d1 must be \(3, 2, 24, 3\) .row 0 = OpenPose. or \(3, at least 22, 3\), got \(3, 21, 3\)"):
        m.update(without(smpl_joints_2d1=torch.zeros(3, 21, 3)))
    with pytest.raises(RuntimeError, match=r"intr0 must be \(3, 3, 3\), got \(3, 3, 4\)"):
        m.update(without(intr0=torch.zeros(3, 3, 4)))
    with pytest.raises(RuntimeError, match="extr0 must be a floating-point tensor, got torch.int32"):
        m.update(without(extr0=torch.zeros(3, 4, 4, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="pred_j3d_cam0 lives on cpu"):                    # the first tensor looked at
        m.update(out, batch)


def test_state_round_trip_and_summarise_without_a_gpu():
    from airpose_amd import CrossViewMetrics
    from airpose_amd import cross_view_metrics as C
    m = CrossViewMetrics(device="cuda:0")
    acc = torch.zeros(2, 13, dtype=torch.float64)
    flat = acc.view(-1)
    flat[C.A_SEEN], flat[C.A_SKIPPED] = 10, 2
    flat[C.A_JW], flat[C.A_JR], flat[C.A_NROOT] = 0.8, 0.4, 8
    flat[C.A_TRANS], flat[C.A_NTRANS] = 1.6, 4
    flat[C.A_ORIENT], flat[C.A_POSE], flat[C.A_NROT] = 40.0, 16.0, 8
    flat[C.A_RP0], flat[C.A_RP1], flat[C.A_RS0], flat[C.A_RS1], flat[C.A_RN0], flat[C.A_RN1], flat[C.A_NRP] = 35.0, 0.0, 7, 0, 150, 0, 8
    flat[C.A_TRI0], flat[C.A_TRI1], flat[C.A_TRIN], flat[C.A_NTRI] = 3.0, 6.0, 120, 8
    m.load_state({"kind": "twoview", "n_joints": 22, "root": "trans", "min_ray_angle_deg": 1.0, "acc": acc})
    got = m.compute()
    drop_nan = lambda d: {k: v for k, v in d.items() if v == v}
    assert drop_nan(got) == drop_nan(C.summarise(acc)) and set(got) == set(C.summarise(acc)) and got["count"] == 8 and got["skipped"] == 2
    assert got["joint_gap_world"] == 0.8 / 8 and got["joint_gap_root"] == 0.4 / 8 and got["trans_gap"] == 1.6 / 4
    assert "vertex_gap_world" not in got and "vertex_gap_root" not in got                     # no vertices were fed
    assert got["orient_gap_deg"] == 5.0 and got["pose_gap_deg"] == 2.0
    assert got["reproj_px0"] == 5.0 and got["reproj_n0"] == 150 and got["reproj_n1"] == 0
    assert got["reproj_px1"] != got["reproj_px1"]                                             # fed, and no keypoint ever counted: NaN
    assert got["tri_mpjpe0"] == 3.0 / 120 and got["tri_mpjpe1"] == 6.0 / 120 and got["tri_n"] == 120
    assert all(isinstance(v, (int, float)) for v in got.values())
    assert torch.equal(m.state()["acc"], acc)
    assert m.state()["root"] == "trans" and m.state()["n_joints"] == 22 and m.state()["min_ray_angle_deg"] == 1.0
    with pytest.raises(RuntimeError, match="kind"):
        m.load_state({"kind": "hmr", "acc": acc})
    with pytest.raises(RuntimeError, match="joints"):
        m.load_state({"kind": "twoview", "n_joints": 14, "acc": acc})
    with pytest.raises(RuntimeError, match="root"):
        m.load_state({"root": "joint0", "acc": acc})
    with pytest.raises(RuntimeError, match="min_ray_angle_deg"):
        m.load_state({"min_ray_angle_deg": 2.0, "acc": acc})
    with pytest.raises(RuntimeError, match=r"\(2, 13\) float64"):
        m.load_state({"acc": acc.float()})
    m.reset()
    assert m.compute() == {"count": 0, "skipped": 0}


# ------------------------------------------------------------------------------------------------ GPU
def _check_state(m, refs, bars_list, what):
    acc = m.state()["acc"].numpy().reshape(-1)
    racc, abar = X.accumulate(refs, bars_list)
    X.check(acc, racc, abar, what + " accumulator")
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("rot", ["rotmat", "aa"])
def test_update_and_compute_against_the_reference(rot):
    from airpose_amd import CrossViewMetrics
    from airpose_amd.cross_view_metrics import summarise
    dev = _dev()
    m = CrossViewMetrics(device=dev, per_sample=True)
    refs, bars_list = [], []
    for i, B in enumerate((3, 5)):
        case = _case(B, 40, rot, seed=20 + i)
        ref = X.reference(case)
        bar = X.bars(case, ref)
        out, batch = X.dicts_of(case, dev)
        ps, tri = m.update(out, batch)
        assert ps.shape == (B, 16) and tri.shape == (B, 22, 4) and ps.device == dev and ps.dtype == torch.float32
        X.check(ps.cpu().numpy(), ref["ps"], bar["ps"], "per-sample values")
        X.check(tri.cpu().numpy(), ref["tri"], bar["tri"], "tri")
        refs.append(ref), bars_list.append(bar)
    acc = _check_state(m, refs, bars_list, "two updates")
    got = m.compute()
    assert got == summarise(acc) and got["count"] == 7 and got["skipped"] == 1
    want = summarise(X.accumulate(refs, bars_list)[0])
    assert set(got) == set(want) == {"count", "skipped", "joint_gap_world", "joint_gap_root", "vertex_gap_world", "vertex_gap_root",
                                     "trans_gap", "orient_gap_deg", "pose_gap_deg", "reproj_px0", "reproj_px1", "reproj_n0", "reproj_n1",
                                     "tri_mpjpe0", "tri_mpjpe1", "tri_n"}
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-7, (k, got[k], want[k])
    # joint0 as the root, no translations, no per-sample outputs, (B, 3, 4) extrinsics and flat keypoints
    case = _case(3, 0, rot, seed=31)
    out, batch = X.dicts_of(case, dev)
    j0 = CrossViewMetrics(root="joint0", device=dev)
    lean = {k: t for k, t in out.items() if not k.startswith("pred_smpltrans")}
    lean.update({k: (t[:, :3].contiguous() if k.startswith("extr") else t[:, 0, :23].contiguous() if k.startswith("smpl_joints_2d") else t)
                 for k, t in batch.items()})
    assert j0.update(lean) is None
    c2 = dict(case, root="joint0", feed={"rot", "reproj", "tri"})
    c2["size"] = dict(case["size"], root=3)
    c2["stride"] = dict(case["stride"], root=case["stride"]["joints"])
    c2["view"] = [dict(d, root=d["joints"]) for d in case["view"]]
    ref = X.reference(c2)
    _check_state(j0, [ref], [X.bars(c2, ref)], "joint0")
    assert "trans_gap" not in j0.compute() and "joint_gap_root" in j0.compute()
    m.reset()
    assert m.compute() == {"count": 0, "skipped": 0}


@pytest.mark.gpu
def test_evaluate_scores_the_pass_next_to_mesh_metrics(smplx_model, copenet_sd):
    """two B = 2 batches of the golden synthetic checkpoint behind TwoViewInference.submit: _stream_metric.evaluate with a
    MeshMetrics and a CrossViewMetrics gives the CrossViewMetrics the sums it gets alone from the materialised outputs, bit for bit,
    and those are the reference's"""
    from airpose_amd import CrossViewMetrics, MeshMetrics, copenet_model, pipeline, smplx
    from airpose_amd import weights as W
    from airpose_amd._stream_metric import evaluate
    dev = _dev()
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    pipe = pipeline.TwoViewInference(net, smplx.SMPLX(model_data=smplx_model))
    rng = np.random.default_rng(5)
    batches, outs = [], []
    for i in range(2):
        b = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(800 + i, 2).items()}
        out = {k: (t.clone() if torch.is_tensor(t) else t) for k, t in pipe(b, want_angles=True).items()}
        torch.cuda.synchronize()
        for v in (0, 1):
            cams = [X._look_at(rng.uniform(6, 10) * d / np.linalg.norm(d), np.zeros(3), rng) for d in rng.standard_normal((2, 3))]
            e = np.stack([np.vstack([np.concatenate([R, t[:, None]], 1), [0, 0, 0, 1]]) for R, t in cams]).astype(np.float32)
            b["extr%d" % v] = torch.from_numpy(e).to(dev)
            kp = np.concatenate([out["pred_j2d_cam%d" % v][:, :24].cpu().numpy() + rng.uniform(-4, 4, (2, 24, 2)), rng.uniform(0.2, 1, (2, 24, 1))], 2)
            b["smpl_joints_2d%d" % v] = torch.from_numpy(np.stack([kp, rng.uniform(0, 1000, kp.shape)], 1).astype(np.float32)).to(dev)
            for src, dst in (("pred_j3d_cam%d", "smpl_joints_rel%d"), ("pred_vertices_cam%d", "smpl_vertices_rel%d")):
                b[dst % v] = (out[src % v] + 0.01).unsqueeze(1)
        batches.append(b), outs.append(out)
    alone = CrossViewMetrics(min_ray_angle_deg=0.0, device=dev)
    refs, bars_list = [], []
    for b, out in zip(batches, outs):
        alone.update(out, b)
        case = X.case_of(out, b)
        ref = X.reference(case, min_sin2=0.0)
        refs.append(ref), bars_list.append(X.bars(case, ref))
    mm, cv = MeshMetrics(kind="twoview", device=dev), CrossViewMetrics(min_ray_angle_deg=0.0, device=dev)
    got_mesh, got_cv = evaluate(pipe, iter(batches), [mm, cv])
    assert got_mesh["count"] == 4 and got_cv["count"] == 4 and got_cv["skipped"] == 0
    assert torch.equal(cv.state()["acc"].view(torch.int64), alone.state()["acc"].view(torch.int64))
    assert got_cv == alone.compute()
    assert got_cv["reproj_n0"] == 88 and got_cv["orient_gap_deg"] > 0 and got_cv["vertex_gap_world"] > 0 and "tri_n" in got_cv
    _check_state(cv, refs, bars_list, "evaluate")


@pytest.mark.gpu
def test_an_export_shaped_dict_is_scored_with_one_camera_as_the_world():
    """what AirPosePlusSequence.export returns for a body both cameras agree on: smpl_wrt_cam0/1 carry one body into the two cameras,
    cam1_wrt_cam0 = smpl_wrt_cam0 smpl_wrt_cam1^-1 is extr0 with world = camera 1 -- the gaps are the floats' rounding; taken the
    other way round they are metres"""
    from airpose_amd import CrossViewMetrics
    dev = _dev()
    rng = np.random.default_rng(9)
    n, V = 4, 300
    T = []
    for v in range(2):
        R, t = zip(*[(X._rot(rng), rng.uniform(-1, 1, 3) + [0, 0, 8.0]) for _ in range(n)])
        T.append(np.stack([np.vstack([np.concatenate([Rv, tv[:, None]], 1), [0, 0, 0, 1]]) for Rv, tv in zip(R, t)]))
    body, verts, root = rng.uniform(-0.5, 0.5, (n, 127, 3)), rng.uniform(-0.5, 0.5, (n, V, 3)), rng.uniform(-0.1, 0.1, (n, 3))
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
    export = {"cam1_wrt_cam0": f(T[0] @ np.linalg.inv(T[1])), "frames": slice(0, n)}
    for v in range(2):
        carry = lambda P: np.einsum("nij,nkj->nki", T[v][:, :3, :3], P) + T[v][:, None, :3, 3]
        export["smpl_wrt_cam%d" % v] = f(T[v])
        export["pred_j3d_cam%d" % v], export["pred_vertices_cam%d" % v] = f(carry(body)), f(carry(verts))
        export["trans%d" % v] = f(carry(root[:, None])[:, 0])
    eye = torch.eye(4, device=dev).expand(n, 4, 4).contiguous()
    extra = {"pred_smpltrans0": export["trans0"], "pred_smpltrans1": export["trans1"]}
    m = CrossViewMetrics(device=dev)
    m.update(export, dict(extra, extr0=export["cam1_wrt_cam0"], extr1=eye))
    got = m.compute()
    assert got["count"] == n and got["skipped"] == 0
    assert set(got) == {"count", "skipped", "joint_gap_world", "joint_gap_root", "vertex_gap_world", "vertex_gap_root", "trans_gap"}
    for k in ("joint_gap_world", "joint_gap_root", "vertex_gap_world", "vertex_gap_root", "trans_gap"):
        assert got[k] < 2e-5, (k, got[k])                    # 8 m away in floats: 24 u |p| is 1.2e-5
    wrong = CrossViewMetrics(device=dev)
    wrong.update(export, dict(extra, extr0=eye, extr1=export["cam1_wrt_cam0"]))
    assert wrong.compute()["joint_gap_world"] > 0.1


@pytest.mark.gpu
def test_lstsq_triangulation_against_the_reference_function():
    from airpose_amd import geometry
    dev = _dev()
    case = X.make_case(6, 22, 22, 0, False, seed=40, kinds=["consistent", "shifted", "zero_conf", "nan_kp", "narrow", "nonortho"])
    ref = X.reference(case)
    bar = X.bars(case, ref)
    out, batch = X.dicts_of(case, dev)
    K = torch.stack([batch["intr0"], batch["intr1"]], 1)
    Ex = torch.stack([batch["extr0"], batch["extr1"]], 1)
    kp = torch.stack([batch["smpl_joints_2d0"][:, 0, :22], batch["smpl_joints_2d1"][:, 0, :22]], 1)
    pts, valid = geometry.lstsq_triangulation(K, Ex, kp, min_ray_angle_deg=X.MIN_ANGLE_DEG)
    assert pts.shape == (6, 22, 3) and valid.shape == (6, 22) and valid.dtype == torch.bool
    assert np.array_equal(valid.cpu().numpy(), ref["tri"][..., 3] > 0)
    X.check(pts.cpu().numpy(), ref["tri"][..., :3], bar["tri"][..., :3], "lstsq_triangulation")
    assert not valid[4].any() and not valid[5].any() and valid[0].all()
    # (B, 2, 3, 4) extrinsics, points without a confidence, no gate: the reference function on every joint of the first two samples
    pts2, valid2 = geometry.lstsq_triangulation(K[:2], Ex[:2, :, :3], kp[:2, :, :, :2])
    assert valid2.all()
    for b in range(2):
        for j in range(22):
            one = np.append(kp[b, :, j, :2].cpu().numpy().astype(np.float64), [[1.0], [1.0]], 1)
            T, ok, sv, nb = X.tri_reference(X.view(case, 0, "extr")[b][:12], X.view(case, 1, "extr")[b][:12], X.view(case, 0, "intr")[b],
                                            X.view(case, 1, "intr")[b], one[0], one[1], 0.0)
            tol = X.U * np.abs(T) + 64 * X.U64 * (sv[0] / sv[2]) ** 2 * (np.linalg.norm(T) + nb / sv[0])
            assert ok and (np.abs(pts2[b, j].cpu().numpy() - T) <= tol).all(), (b, j)
    with pytest.raises(RuntimeError, match="points_2d must be"):
        geometry.lstsq_triangulation(K, Ex, kp[:, 0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.lstsq_triangulation(K.cpu(), Ex.cpu(), kp.cpu())
