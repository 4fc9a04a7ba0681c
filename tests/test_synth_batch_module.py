"""airpose_amd.SyntheticBatches (airpose_amd/synth_batches.py): the refusals by name without a GPU, and on the GPU the dict's keys and
shapes against the return statement of aerialpeople_crop.__getitem__ (aerialpeople.py:212-226, collated over the batch), the kernel
outputs against the direct C ABI calls of test_synth_batch_fp64.py, the canonical body of every row against a direct SMPLX.forward of
that row's gender, no host synchronisation (by counting, as tests/test_real_batch_module.py does), and the dict unchanged in its
consumers: TwoViewInference, TrainingLoss("twoview"), EvalMetrics and MeshMetrics.  The body models are conftest's synthetic one,
built with a seed per gender."""
import numpy as np
import pytest
import torch

import synth_batch_util as U
from conftest import MEAN_PARAMS
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)

N = 5
GENDERS = ["male", "FEMALE", "neutral", "Female", "robot"]    # the reference's rule: any case; what is neither is neutral
ROWS = {"male": [0], "female": [1, 3], "neutral": [2, 4]}


@pytest.fixture(scope="module")
def models(smplx_model):
    from airpose_amd import smplx, smplx_model as SM
    return {"neutral": smplx.SMPLX(model_data=smplx_model), "male": smplx.SMPLX(model_data=SM.make_synthetic_model(4322)),
            "female": smplx.SMPLX(model_data=SM.make_synthetic_model(4323))}


def _records(V, J, device=None):
    rec, index = U.case(N, V, J)
    t = {k: torch.from_numpy(v.copy()) for k, v in rec.items()}
    index = torch.from_numpy(index.copy())
    if device is not None:
        t, index = {k: v.to(device) for k, v in t.items()}, index.to(device)
    t["smplgender"] = list(GENDERS)
    return t, index


def _frames(device=None):
    g = torch.Generator().manual_seed(4400 + N)              # (test_synth_batch_fp64.frames_for's)
    f = torch.randint(0, 256, (2, N, U.HC, U.WC, 3), generator=g, dtype=torch.uint8)
    return f if device is None else f.to(device)


def _make(models, **kw):
    from airpose_amd import SyntheticBatches
    args = dict(device="cuda:0", frame_size=(U.H, U.W), margin=U.MARGIN, focal_length=U.FOCAL, seed=U.SEED)
    args.update(kw)
    return SyntheticBatches(models, **args)


# ------------------------------------------------------------------------------------------------ no GPU
def test_class_is_exported_and_refuses_by_name_without_a_gpu(models):
    import airpose_amd
    from airpose_amd import synth_batches
    assert airpose_amd.SyntheticBatches is synth_batches.SyntheticBatches
    S = airpose_amd.SyntheticBatches
    with pytest.raises(RuntimeError, match="device must be a CUDA .* there is no CPU path"):
        S(models, device="cpu")
    with pytest.raises(TypeError, match="smplx_models must be a non-empty dict"):
        S({}, device="cuda:0")
    with pytest.raises(ValueError, match="smplx_models has the key 'other'"):
        S({"other": models["male"]}, device="cuda:0")
    with pytest.raises(TypeError, match=r"smplx_models\['male'\] must be an airpose_amd.SMPLX, got dict"):
        S({"male": {}}, device="cuda:0")
    with pytest.raises(ValueError, match="margin must be a whole number in 0 .. 1048576, got -1"):
        S(models, device="cuda:0", margin=-1)
    with pytest.raises(ValueError, match=r"frame_size\[1\] must be a whole number"):
        S(models, device="cuda:0", frame_size=(1080, 0))
    with pytest.raises(ValueError, match="frame_size must be"):
        S(models, device="cuda:0", frame_size=1080)
    with pytest.raises(ValueError, match="seed must be a whole number"):
        S(models, device="cuda:0", seed=-3)
    with pytest.raises(ValueError, match="focal_length must be"):
        S(models, device="cuda:0", focal_length=(1.0, float("nan")))
    s = S({"male": models["male"]}, device=torch.device("cuda", 0))          # a subset is allowed
    assert s.frame_size == (1080, 1920) and s.margin == 200 and s.focal_length == (1475.0, 1475.0) and s.jitter and s.shuffle


def test_batch_refuses_its_arguments_by_name(models):
    """types and shapes first, then the genders, the devices last: all reachable with CPU tensors"""
    s = _make(models)
    rec, index = _records(67, 22)
    frames = _frames()
    bad = lambda **kw: dict(rec, **kw)
    with pytest.raises(RuntimeError, match="records must be a dict"):
        s.batch([rec], frames, index)
    with pytest.raises(RuntimeError, match="records has no 'smpltrans'"):
        s.batch({k: v for k, v in rec.items() if k != "smpltrans"}, frames, index)
    with pytest.raises(RuntimeError, match=r"records\['extr'\] must be a tensor, got ndarray"):
        s.batch(bad(extr=rec["extr"].numpy()), frames, index)
    with pytest.raises(RuntimeError, match=r"records\['bb'\] must be int32 .* got torch.int64"):
        s.batch(bad(bb=rec["bb"].long()), frames, index)
    with pytest.raises(RuntimeError, match=r"records\['smpl_vertices_wrt_origin'\] must be float32 .* got torch.float64"):
        s.batch(bad(smpl_vertices_wrt_origin=rec["smpl_vertices_wrt_origin"].double()), frames, index)
    with pytest.raises(RuntimeError, match="frames must be uint8"):
        s.batch(rec, frames.float(), index)
    with pytest.raises(RuntimeError, match="index must be int32"):
        s.batch(rec, frames, index.long())
    with pytest.raises(RuntimeError, match=r"records\['smplpose'\] must be \(n, 63\) with n = 5, got \(5, 66\)"):
        s.batch(bad(smplpose=torch.zeros(N, 66)), frames, index)
    with pytest.raises(RuntimeError, match=r"records\['intr'\] must be \(n, 2, 3, 3\) with n = 5, got \(4, 2, 3, 3\)"):
        s.batch(bad(intr=rec["intr"][:4]), frames, index)
    with pytest.raises(RuntimeError, match=r"records\['smpl_joints_wrt_origin'\] must be \(n, 1, J, 3\)"):
        s.batch(bad(smpl_joints_wrt_origin=rec["smpl_joints_wrt_origin"][:, 0]), frames, index)
    with pytest.raises(RuntimeError, match=r"frames must be \(2, n, Hc, Wc, 3\) with n = 5, got \(2, 4, 96, 128, 3\)"):
        s.batch(rec, frames[:, :4], index)
    with pytest.raises(RuntimeError, match=r"index must be \(n,\) with n = 5, got \(4,\)"):
        s.batch(rec, frames, index[:4])
    with pytest.raises(RuntimeError, match="smplgender'\\] must be a host list of n = 5 strings"):
        s.batch(bad(smplgender=GENDERS[:4]), frames, index)
    with pytest.raises(RuntimeError, match="epoch must be an integer, got float"):
        s.batch(rec, frames, index, epoch=1.5)
    with pytest.raises(RuntimeError, match="epoch must be in"):
        s.batch(rec, frames, index, epoch=-1)
    with pytest.raises(RuntimeError, match="origin must be 'region' or 'frame', got 'canvas'"):
        s.batch(rec, frames, index, origin="canvas")
    with pytest.raises(RuntimeError, match="sample 1 is female and smplx_models has no 'female' model"):
        _make({k: models[k] for k in ("male", "neutral")}).batch(rec, frames, index)
    with pytest.raises(RuntimeError, match=r"records\['bb'\] lives on cpu; it must be a CUDA .* there is no CPU path"):
        s.batch(rec, frames, index)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def sizes(dev, models):
    """(V, J) of the body models: the records carry the same counts, as the dataset's do"""
    body = models["neutral"]
    out = body.forward(betas=torch.zeros(1, 10, device=dev), body_pose=torch.eye(3, device=dev).expand(1, 21, 3, 3).contiguous(),
                       global_orient=torch.eye(3, device=dev).reshape(1, 1, 3, 3), transl=torch.zeros(1, 3, device=dev), pose2rot=False)
    return int(out.vertices.shape[1]), int(out.joints.shape[1])


@pytest.fixture(scope="module")
def made(dev, models, sizes):
    s = _make(models, device=dev)
    rec, index = _records(*sizes, device=dev)
    frames = _frames(dev)
    return s, rec, index, frames, s.batch(rec, frames, index, epoch=2)


@pytest.mark.gpu
def test_keys_and_shapes_are_the_reference_s(made, sizes):
    s, rec, index, frames, b = made
    V, J = sizes
    want = {"smplbetas": (N, 10), "smplpose_rotmat": (N, 21, 3, 3), "focal_length": (N, 2), "img_size": (N, 2), "smpl_vertices": (N, 1, V, 3),
            "smpl_joints": (N, 1, J, 3), "cam0": (N,)}
    per_view = {"im": (N, 3, 224, 224), "intr": (N, 3, 3), "extr": (N, 1, 4, 4), "bb": (N, 3), "crop_info": (N, 2, 2), "smpltrans_rel": (N, 3),
                "smplorient_rel": (N, 1, 3, 3), "smpl_vertices_rel": (N, 1, V, 3), "smpl_joints_rel": (N, 1, J, 3), "smpl_joints_2d": (N, 1, J, 2),
                "smpl_joints_2d_crop": (N, J, 2), "crops": (N, 4), "scale": (N,), "pad": (N, 2), "status": (N,)}
    want.update({"%s%d" % (k, v): shape for k, shape in per_view.items() for v in (0, 1)})
    assert sorted(b) == sorted(list(want) + ["smpl_gender"]) and b["smpl_gender"] == GENDERS
    for k, shape in want.items():
        assert tuple(b[k].shape) == shape and b[k].device == s.device, k
        assert b[k].dtype == (torch.int32 if k[:-1] in ("crop_info", "crops", "pad", "status") or k == "cam0" else torch.float32), k
    # every key of the reference's return statement but the two image paths, which stay with the caller
    reference = ["im", "intr", "extr", "bb", "crop_info", "smpltrans_rel", "smplorient_rel", "smpl_vertices_rel", "smpl_joints_rel",
                 "smpl_joints_2d", "smpl_joints_2d_crop"]
    for k in [r + str(v) for r in reference for v in (0, 1)] + ["smplbetas", "smplpose_rotmat", "focal_length", "img_size", "smpl_vertices",
                                                              "smpl_joints", "smpl_gender"]:
        assert k in b, k
    assert torch.equal(b["focal_length"].cpu(), torch.tensor(U.FOCAL).expand(N, 2)) and torch.equal(b["img_size"].cpu(), torch.tensor([float(U.W), float(U.H)]).expand(N, 2))
    assert torch.equal(b["smplbetas"], rec["smplshape"])


@pytest.mark.gpu
def test_batch_is_the_two_entry_points(dev, made, sizes):
    from test_synth_batch_fp64 import run_batch, run_crops
    s, rec, index, frames, b = made
    rn, idx = U.case(N, *sizes)
    o = run_batch(dev, rn, idx, epoch=2)
    o.update(run_crops(dev, frames, o))
    names = {"crops": "crops", "crop_info": "crop_info", "status": "status", "bb": "bb", "intr": "intr", "extr": "extr",
             "verts_rel": "smpl_vertices_rel", "joints_rel": "smpl_joints_rel", "orient_rel": "smplorient_rel", "trans_rel": "smpltrans_rel",
             "j2d": "smpl_joints_2d", "j2d_crop": "smpl_joints_2d_crop", "im": "im", "scale": "scale", "pad": "pad"}
    for k, name in names.items():
        for v in (0, 1):
            got = b["%s%d" % (name, v)]
            assert torch.equal(got.reshape(o[k][v].shape), o[k][v]), (k, v)
    assert torch.equal(b["cam0"], o["flip"]) and torch.equal(b["smplpose_rotmat"], o["pose_rotmat"])
    ref = U.ref_batch(rn, idx, epoch=2, boxes_only=True)
    assert np.array_equal(b["cam0"].cpu().numpy(), ref["flip"]) and np.array_equal(b["crops0"].cpu().numpy(), ref["crops"][0])
    # bgr and the epoch matter; the origin "frame" takes the whole frame as its canvas
    assert not torch.equal(s.batch(rec, frames, index, epoch=2, bgr=False)["im0"], b["im0"])
    assert not torch.equal(s.batch(rec, frames, index, epoch=3)["crops0"], b["crops0"])
    g = torch.Generator().manual_seed(1)
    whole = torch.randint(0, 256, (2, N, U.H, U.W, 3), generator=g, dtype=torch.uint8).to(dev)
    f = s.batch(rec, whole, index, epoch=2, origin="frame")
    assert np.array_equal(f["crops1"].cpu().numpy(), U.ref_batch(rn, idx, epoch=2, origin="frame", boxes_only=True)["crops"][1])
    plain = _make(s.models, device=dev, jitter=False, shuffle=False).batch(rec, frames, index)
    assert not bool(plain["cam0"].any()) and int(plain["status0"][3]) == U.OUTSIDE


@pytest.mark.gpu
def test_canonical_body_rows_are_a_direct_forward_of_their_gender(dev, made, models):
    s, rec, index, frames, b = made
    eye, zero = torch.eye(3, device=dev).reshape(1, 1, 3, 3), torch.zeros(1, 3, device=dev)
    seen = 0
    for g, rows in ROWS.items():
        for i in rows:
            out = models[g].forward(betas=rec["smplshape"][i:i + 1], body_pose=b["smplpose_rotmat"][i:i + 1].contiguous(), global_orient=eye,
                                    transl=zero, pose2rot=False)
            assert torch.equal(b["smpl_vertices"][i], out.vertices) and torch.equal(b["smpl_joints"][i], out.joints), (g, i)
            seen += 1
    assert seen == N
    assert not torch.equal(b["smpl_vertices"][1], b["smpl_vertices"][3])                   # (two women, two bodies)
    # one gender for the whole batch takes the path without a gather
    rec1 = dict(rec, smplgender=["male"] * N)
    one = s.batch(rec1, frames, index, epoch=2)
    out = models["male"].forward(betas=rec["smplshape"], body_pose=b["smplpose_rotmat"], global_orient=eye.expand(N, 1, 3, 3),
                                 transl=zero.expand(N, 3), pose2rot=False)
    assert torch.equal(one["smpl_vertices"][:, 0], out.vertices) and torch.equal(one["smpl_joints"][:, 0], out.joints)
    assert torch.equal(one["smpl_vertices"][0], b["smpl_vertices"][0])


@pytest.mark.gpu
def test_batch_does_not_synchronise(made, monkeypatch):
    s, rec, index, frames, _ = made
    counts = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy", "to", "__float__", "__bool__", "__int__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                counts["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    b = s.batch(rec, frames, index)
    assert counts["n"] == 0, "batch() copied to the host"
    b["status0"].cpu()
    assert counts["n"] == 1                                  # (the count does see a copy)


@pytest.mark.gpu
def test_the_dict_feeds_its_consumers_unchanged(dev, made, models, copenet_sd, smplx_model):
    from airpose_amd import EvalMetrics, MeshMetrics, TrainingLoss, copenet_model, pipeline
    s, rec, index, frames, b = made
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    out = pipeline.TwoViewInference(net, models["neutral"])(b, want_angles=True)
    leaf = lambda k: out[k].detach().clone().contiguous().requires_grad_()
    P = [leaf(k + str(v)) for k in ("pred_smpltrans", "pred_rotmat", "pred_betas") for v in (0, 1)]
    O = [(leaf("pred_j3d_cam%d" % v), leaf("pred_vertices_cam%d" % v)) for v in (0, 1)]
    J2 = [leaf("pred_j2d_cam%d" % v) for v in (0, 1)]
    loss, terms = TrainingLoss("twoview")(b, *P, *O, *J2)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(terms).all()) and float(loss.detach()) > 0
    grads = P + [t for o in O for t in o] + J2
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in grads) and bool(J2[0].grad.abs().sum() > 0)
    held = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}                     # (the pipeline reuses its workspaces)
    ev = EvalMetrics(smplx_model, kind="twoview", device=dev)
    ev.update(held, b)
    res = ev.compute()
    assert res["count"] == N and all(np.isfinite(res[k]) for k in ("mpjpe0", "mpjpe1", "mpe0", "mpe1"))
    mm = MeshMetrics(kind="twoview", device=dev)
    mm.update(held, b)
    res = mm.compute()
    assert res["count"] == N and all(np.isfinite(res[k]) and res[k] > 0 for k in ("mpjpe_abs0", "pa_mpjpe1", "pve_abs0", "pa_pve1"))
