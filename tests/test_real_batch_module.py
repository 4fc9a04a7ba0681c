"""airpose_amd.RealSequenceBatches (airpose_amd/real_batches.py) on the GPU: batch() against utils.preprocess_crops bit for bit,
the camera swap, the filtered detections against AirPosePlusSequence.prepare's, no host synchronisation, predict against direct
pipeline calls, and the dict in its three consumers (TwoViewInference, AirPosePlusSequence, RealDataLoss).  The kernel's own checks
are in test_real_batch_fp64.py; the inputs (frames of 120 x 160 and 90 x 200, the planted detections) are real_batch_util's.

No synchronisation is shown by COUNTING, as tests/test_real_loss_module.py does: every torch.Tensor method that copies to the host
(cpu, item, tolist, numpy, to, __float__, __bool__, __int__) is patched to count its calls on CUDA tensors, and batch() must make none.
(torch.cuda.set_sync_debug_mode sees only torch's own operators; the count also covers what the module itself might call.)"""
import numpy as np
import pytest
import torch

import real_batch_util as U
import seq_util as SU
from conftest import MEAN_PARAMS
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)
from test_real_batch_fp64 import run

BORDER = 50
LP = 5                                                       # predict: batches of 2, 2, 1


def _intr():
    K = torch.zeros(2, 3, 3)
    for v, (cx, cy) in enumerate(U.PRINCIPAL):
        K[v] = torch.tensor([[300.0 + 10 * v, 0.0, cx], [0.0, 310.0 + 10 * v, cy], [0.0, 0.0, 1.0]])
    return K


@pytest.fixture(scope="module")
def frames(dev):
    g = torch.Generator().manual_seed(77)
    return [torch.randint(0, 256, (U.L, H, W, 3), generator=g, dtype=torch.uint8).to(dev) for H, W in U.SIZES]


@pytest.fixture(scope="module")
def batches(dev):
    from airpose_amd import RealSequenceBatches
    return RealSequenceBatches(U.case(BORDER).to(dev), _intr(), device=dev, border=BORDER)


@pytest.fixture(scope="module")
def body(dev, smplx_model):
    from airpose_amd import smplx
    return smplx.SMPLX(model_data=smplx_model)


@pytest.fixture(scope="module")
def pipe(dev, body, copenet_sd):
    from airpose_amd import copenet_model, pipeline
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    return pipeline.TwoViewInference(net, body)


@pytest.fixture(scope="module")
def vposer():
    return SU.state_dict(SU.export_case(3, "body")[0])


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("start,n", [(0, U.L), (2, 3)])
def test_batch_is_preprocess_crops_on_the_kernel_s_boxes(dev, batches, frames, bgr, start, n):
    from airpose_amd import utils
    f = [t[start:start + n] for t in frames]
    b = batches.batch(f[0], f[1], start, bgr=bgr)
    ref = U.ref_batch(U.case(BORDER), start, n, BORDER)
    assert b["cam"] == 0
    for v in (0, 1):
        crops = b["crops%d" % v]
        assert np.array_equal(crops.cpu().numpy(), ref["crops"][v])                       # (the boxes are valid before anything reads through them again)
        assert torch.equal(b["crop_info%d" % v].cpu(), torch.from_numpy(ref["crop_info"][v]))
        im, scale, pad = utils.preprocess_crops(f[v], crops, bgr=bgr)
        assert tuple(b["im%d" % v].shape) == (n, 3, 224, 224) and _eq(b["im%d" % v], im)
        assert _eq(b["scale%d" % v], scale) and torch.equal(b["pad%d" % v], pad) and _eq(b["bb%d" % v][:, 2], scale)
        assert tuple(b["bb%d" % v].shape) == (n, 3) and tuple(b["intr%d" % v].shape) == (n, 3, 3)
        assert torch.equal(b["intr%d" % v].cpu(), _intr()[v].expand(n, 3, 3))
        assert tuple(b["smpl_joints_2d%d" % v].shape) == tuple(b["smpl_joints_2d_crop%d" % v].shape) == (n, 2, 24, 3)
        assert np.array_equal(b["status%d" % v].cpu().numpy(), ref["status"][v])
    other = batches.batch(f[0], f[1], start, bgr=not bgr)
    assert not _eq(other["im0"], b["im0"])                   # the channel order matters
    assert torch.equal(batches.intr_fit.cpu(), torch.tensor([[300.0, 310.0, *U.PRINCIPAL[0]], [310.0, 320.0, *U.PRINCIPAL[1]]]))


@pytest.mark.gpu
def test_first_cam_swaps_by_naming(dev, batches, frames):
    from airpose_amd import RealSequenceBatches
    swapped = RealSequenceBatches(U.case(BORDER).to(dev), _intr().to(dev), device=dev, first_cam=1, border=BORDER)
    a, b = batches.batch(frames[0], frames[1], 0), swapped.batch(frames[0], frames[1], 0)
    assert a["cam"] == 0 and b["cam"] == 1
    keys = sorted(k[:-1] for k in a if k.endswith("0"))
    assert keys == sorted(["im", "bb", "intr", "crop_info", "smpl_joints_2d", "smpl_joints_2d_crop", "crops", "scale", "pad", "status"])
    assert sorted(a) == sorted(b)
    for k in keys:
        for s in (0, 1):
            x, y = a["%s%d" % (k, s)], b["%s%d" % (k, 1 - s)]
            assert x.shape == y.shape and torch.equal(x, y), (k, s)
    assert not torch.equal(a["bb0"], a["bb1"])


@pytest.mark.gpu
def test_filtered_detections_are_prepare_s(dev, batches, frames, body, vposer):
    """smpl_joints_2d* against AirPosePlusSequence.prepare's j2d, torch.equal: on the planted detections through batch(), and -- the
    kernel alone, no frame is read -- on 64 frames of detector pairs whose distance is 100 px to within a few fp32 roundings, where a
    comparison formed in another order (a fused against an unfused sum of squares) would decide differently"""
    from airpose_amd import AirPosePlusSequence
    seq = AirPosePlusSequence(vposer, body, device=dev)
    pred = lambda L: {"pred_angles0": torch.zeros(L, 22, 3, device=dev), "pred_angles1": torch.full((L, 22, 3), 0.1, device=dev),
                      "pred_smpltrans0": torch.ones(L, 3, device=dev), "pred_smpltrans1": torch.ones(L, 3, device=dev)}
    det = U.case(BORDER).to(dev)
    want = seq.prepare(pred(U.L), det)[1]["j2d"]
    for start, n in ((0, U.L), (2, 3)):
        b = batches.batch(frames[0][start:start + n], frames[1][start:start + n], start)
        got = torch.stack([b["smpl_joints_2d0"], b["smpl_joints_2d1"]])
        assert torch.equal(got, want[:, start:start + n])
    assert bool((want[..., 2] == 0).any()) and not torch.equal(want, det)
    L = 64
    g = torch.Generator().manual_seed(91)
    edge = torch.zeros(2, L, 2, 24, 3)
    pos = 40.0 + 100.0 * torch.rand(2, L, 24, 2, generator=g)
    ang = 6.2831853 * torch.rand(2, L, 24, generator=g)
    far = 100.0 * (1.0 + 2e-7 * torch.randint(-3, 4, (2, L, 24), generator=g).float())
    edge[:, :, 0, :, :2], edge[:, :, 1, :, :2] = pos, pos + far.unsqueeze(-1) * torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    edge[..., 2] = 0.25 + 0.5 * torch.rand(2, L, 2, 24, generator=g)
    want = seq.prepare(pred(L), edge.to(dev))[1]["j2d"]
    got = run(dev, edge, 0, L, BORDER)["j2d"]
    dropped = float((want[..., 2] == 0).float().mean())
    print("pairs at the threshold: %.0f %% dropped" % (100 * dropped))
    assert 0.2 < dropped < 0.8 and torch.equal(got, want)


@pytest.mark.gpu
def test_batch_does_not_synchronise(dev, batches, frames, monkeypatch):
    batches.batch(frames[0], frames[1], 0)                   # (the libraries are loaded by now)
    counts = {"n": 0}
    for name in ("cpu", "item", "tolist", "numpy", "to", "__float__", "__bool__", "__int__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                counts["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    b = batches.batch(frames[0], frames[1], 0)
    assert counts["n"] == 0, "batch() copied to the host"
    b["status0"].cpu()
    assert counts["n"] == 1                                  # (the count does see a copy)


def _source(frames):
    return lambda a, b: (frames[0][a:b], frames[1][a:b])


@pytest.mark.gpu
def test_predict_equals_direct_calls_read_one_at_a_time(dev, frames, pipe):
    from airpose_amd import RealSequenceBatches
    rb = RealSequenceBatches(U.case(BORDER)[:, :LP].to(dev), _intr(), device=dev, border=BORDER)
    got = rb.predict(pipe, _source(frames), batch_size=2)
    keys = ("pred_angles0", "pred_angles1", "pred_smpltrans0", "pred_smpltrans1")
    assert sorted(got) == sorted(keys + ("status",))
    want = {k: [] for k in keys}
    for a, b in ((0, 2), (2, 4), (4, 5)):
        out = pipe(rb.batch(frames[0][a:b], frames[1][a:b], a), want_angles=True)
        for k in keys:
            want[k].append(out[k].cpu())                     # read before the next call reuses the workspaces
    for k in keys:
        w = torch.cat(want[k])
        assert tuple(got[k].shape) == (LP,) + tuple(w.shape[1:]) and bool(torch.isfinite(w).all())
        assert torch.equal(got[k].cpu().view(torch.int32), w.contiguous().view(torch.int32)), k
    assert not torch.equal(got["pred_angles0"][0], got["pred_angles0"][2])
    assert np.array_equal(got["status"].cpu().numpy(), U.ref_batch(U.case(BORDER), 0, LP, BORDER)["status"])
    # the cameras keep their index whichever comes first
    sw = RealSequenceBatches(U.case(BORDER)[:, :LP].to(dev), _intr(), device=dev, first_cam=1, border=BORDER)
    out = pipe(sw.batch(frames[0][:2], frames[1][:2], 0), want_angles=True)
    first = {k: out[k].cpu() for k in keys}
    got1 = sw.predict(pipe, _source(frames), batch_size=2)
    assert torch.equal(got1["pred_angles1"][:2].cpu(), first["pred_angles0"]) and torch.equal(got1["pred_smpltrans0"][:2].cpu(), first["pred_smpltrans1"])
    assert torch.equal(got1["status"], got["status"])


@pytest.mark.gpu
def test_frames_to_fitted_bodies(dev, frames, pipe, body, vposer):
    from airpose_amd import AirPosePlusSequence, RealSequenceBatches
    det = U.case(BORDER)[:, :LP].to(dev)
    rb = RealSequenceBatches(det, _intr(), device=dev, border=BORDER)
    pred = rb.predict(pipe, _source(frames), batch_size=2)
    out = AirPosePlusSequence(vposer, body, device=dev)(pred, det, rb.intr_fit, n_iters=3, frames=slice(0, 2))
    V = body.num_verts
    for k, shape in (("thetas", (LP, 63)), ("trans0", (LP, 3)), ("trans1", (LP, 3)), ("pred_vertices_cam0", (2, V, 3)),
                     ("pred_vertices_cam1", (2, V, 3))):
        assert tuple(out[k].shape) == shape and bool(torch.isfinite(out[k]).all()), k


@pytest.mark.gpu
def test_batch_feeds_the_fine_tune_loss(dev, batches, frames, pipe, vposer):
    from airpose_amd import RealDataLoss
    batch = batches.batch(frames[0][:3], frames[1][:3], 0)
    out = pipe(batch)
    leaf = lambda k: out[k].detach().clone().contiguous().requires_grad_()
    P = [leaf(k + str(v)) for k in ("pred_smpltrans", "pred_rotmat", "pred_betas") for v in (0, 1)]
    J = [leaf("pred_j2d_cam%d" % v) for v in (0, 1)]
    loss, terms = RealDataLoss("twoview", vposer)(batch, *P, None, None, *J)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(terms).all()) and float(loss.detach()) > 0
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in P + J) and bool(J[0].grad.abs().sum() > 0)
