"""airpose_amd.CameraRoll (airpose_amd/roll.py): the refusals by name without a GPU; on the GPU a SyntheticBatches dict (n = 4, frames
of 120 x 160, V = 67, J = 22, shuffle = True, fx != fy) and a RealSequenceBatches dict (n = 2) through apply with planted angles.

The rolled labels must still BE the geometry of one camera.  Each identity below is evaluated in fp64 from the fp32 tensors of the
rolled dict and held to N ulps of the largest magnitude M of its chain, an ulp being 2^-23 M; a fp32 rounding costs at most half of
one.  N is counted from the chains of include/airpose_grad.h (|c| + |t| <= 1.42 for the 2 x 2 mixes), not taken from a run:
  projection   fx x' / z + cx == j2d'.  j2d: /, *, + (3 roundings); the roll of it: x - cx (1), both components mixed (4 * 1.42 = 5.7),
               t = sn * (fx / fy) and its product (3), c * dx (1), the sum (1), cx + (1): 11.7.  joints': two products and a sum on
               each of x and y, scaled to pixels: 2.4.  14.1 roundings = 7.1 ulps -> N = 8, M = max |pixel coordinate|.
  crop         scale (j2d' - (bb' + 1) c) == j2d_crop'.  j2d_crop: bb (/ and -: 2 that matter), bb + 1, * c, the difference, * scale
               (6), mixed (8.5), t and the sums (5): 13.5.  The left side: j2d' (11.7), bb' from bb (2 * 1.42), bb * c (1), the mix
               (5), / c (1): 9.8, all times scale.  35 roundings = 17.5 ulps -> N = 20, M = scale * max |pixel coordinate|.
  extrinsics   extr' (wrt_origin, 1) == the rolled *_rel.  *_rel: 3 products and 3 sums (6), mixed (8.5), the roll's products and
               sum (3); extr': 3 roundings per entry on 1.42 of the chain's magnitude (4.3): 15.8 roundings = 7.9 ulps -> N = 8,
               M = max over rows of sum |E_rk| |x_k| + |t_r|.
  orthonormal  R'^T R' == I.  An entry of R' carries the 11.5 roundings above and the fp32 rounding of the two rotations it is built
               from (2); a column product sums 2 sqrt(3) of that: 47 roundings = 23.4 ulps -> N = 24, M = 1.
The end-to-end check paints a Gaussian blob into the frame at one joint's projection: its intensity centroid in the rolled crop lies
at smpl_joints_2d_crop' + 112 within what the SAME statistic gives on the un-rolled batch (the reference's half-pixel conventions)
plus 0.5 pixel for the second resampling, at 25 and at -140 degrees."""
import numpy as np
import pytest
import torch

import real_batch_util as RU
import roll_util as U
from conftest import MEAN_PARAMS
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)

N, V, J = 4, 67, 22
H, W = 120, 160
FOCAL = (1475.0, 1460.0)
MARGIN = 6
ULP = 2.0 ** -23
INDEX = (7, 123456, 3, 2 ** 31 - 1)


def _rotation(g):
    q, r = np.linalg.qr(g.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _records():
    """AerialPeople-shaped records whose bodies DO project into their boxes: the box centres lie within 35 pixels of the principal
    point, the world origin projects to the box centre, the joints within 9 pixels of it and joint 0 within 3"""
    g = np.random.default_rng(9100)
    bb = np.zeros((N, 2, 2, 2), np.int32)
    intr = np.zeros((N, 2, 3, 3), np.float32)
    extr = np.zeros((N, 2, 4, 4), np.float32)
    for i in range(N):
        for c in (0, 1):
            cx, cy = 80.25 + i - c, 59.25 - i + 2 * c
            intr[i, c] = [[FOCAL[0], 0, cx], [0, FOCAL[1], cy], [0, 0, 1]]
            h, w = int(g.integers(50, 64)), int(g.integers(50, 72))
            mx, my = int(cx + g.integers(-30, 31)), int(cy + g.integers(-18, 19))
            x0, y0 = mx - w // 2, my - h // 2
            bb[i, c] = ((x0, y0), (x0 + w, y0 + h))
            Z = float(g.uniform(4.5, 5.5))
            extr[i, c, :3, :3] = _rotation(g)
            extr[i, c, :3, 3] = [Z * ((x0 + w / 2) - cx) / FOCAL[0], Z * ((y0 + h / 2) - cy) / FOCAL[1], Z]
            extr[i, c, 3] = [0, 0, 0, 1]
    joints = g.uniform(-0.03, 0.03, (N, 1, J, 3))
    joints[:, 0, 0] = g.uniform(-0.01, 0.01, (N, 3))
    rec = dict(bb=bb, intr=intr, extr=extr, smplpose=(0.4 * g.standard_normal((N, 63))).astype(np.float32),
               smplshape=g.standard_normal((N, 10)).astype(np.float32),
               smpl_vertices_wrt_origin=g.uniform(-0.05, 0.05, (N, 1, V, 3)).astype(np.float32),
               smpl_joints_wrt_origin=joints.astype(np.float32),
               smplorient_rotmat_wrt_origin=np.stack([_rotation(g) for _ in range(N)])[:, None].astype(np.float32),
               smpltrans=g.uniform(-0.05, 0.05, (N, 3)).astype(np.float32))
    return rec


def _rot(deg0, deg1, dev):
    """(2, N, 2): every sample of suffix 0 by deg0, of suffix 1 by deg1"""
    a = np.deg2rad(np.asarray([[deg0] * N, [deg1] * N], np.float64))
    return torch.from_numpy(np.stack([np.cos(a), np.sin(a)], -1).astype(np.float32)).to(dev)


@pytest.fixture(scope="module")
def synth(dev, smplx_model):
    """the un-rolled batch, once: records, frames with a blob at joint 0's projection in each (sample, view), the dict"""
    from airpose_amd import SyntheticBatches, smplx
    models = {"neutral": smplx.SMPLX(model_data=smplx_model)}
    sb = SyntheticBatches(models, device=dev, frame_size=(H, W), margin=MARGIN, focal_length=FOCAL, seed=U.SEED, jitter=True, shuffle=True)
    rec = _records()
    t = {k: torch.from_numpy(v).to(dev) for k, v in rec.items()}
    t["smplgender"] = ["neutral"] * N
    index = torch.tensor(INDEX, dtype=torch.int32, device=dev)
    blank = torch.zeros(2, N, H, W, 3, dtype=torch.uint8, device=dev)
    first = sb.batch(t, blank, index, epoch=1, origin="frame")                 # the labels do not depend on the pixels
    cam0 = first["cam0"].cpu().numpy()
    assert set(cam0.tolist()) == {0, 1}                      # the shuffle did shuffle
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.zeros((2, N, H, W, 3), np.uint8)
    for s in (0, 1):
        p = first["smpl_joints_2d%d" % s].cpu().numpy()[:, 0, 0]
        for i in range(N):
            blob = 250.0 * np.exp(-((xx - p[i, 0]) ** 2 + (yy - p[i, 1]) ** 2) / (2 * 2.0 ** 2))
            frames[int(cam0[i]) ^ s, i] = np.round(blob)[..., None]
    frames = torch.from_numpy(frames).to(dev)
    batch = sb.batch(t, frames, index, epoch=1, origin="frame")
    return rec, frames, index, batch


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _centroid_error(batch):
    """per (suffix, sample): |intensity centroid of the crop - (smpl_joints_2d_crop[joint 0] + 112)| in crop pixels"""
    yy, xx = np.mgrid[0:224, 0:224]
    err = np.zeros((2, N))
    for s in (0, 1):
        im = _np(batch["im%d" % s]) * U.STD[None, :, None, None].astype(np.float64) + U.MEAN[None, :, None, None].astype(np.float64)
        want = _np(batch["smpl_joints_2d_crop%d" % s])[:, 0] + 112.0
        for i in range(N):
            inten = np.clip(im[i].sum(0), 0, None)
            inten[inten < 1e-3] = 0                          # the normalisation's own rounding on the black background
            assert inten.sum() > 10
            cx, cy = (inten * xx).sum() / inten.sum(), (inten * yy).sum() / inten.sum()
            err[s, i] = np.hypot(cx - want[i, 0], cy - want[i, 1])
    return err


def _check_geometry(rec, batch, new):
    cam0 = batch["cam0"].cpu().numpy()
    worst = {}
    for s in (0, 1):
        K = _np(new["intr%d" % s])
        c = K[:, :2, 2]
        jr, j2, jc, bb = _np(new["smpl_joints_rel%d" % s])[:, 0], _np(new["smpl_joints_2d%d" % s])[:, 0], \
            _np(new["smpl_joints_2d_crop%d" % s]), _np(new["bb%d" % s])
        proj = np.stack([FOCAL[0] * jr[..., 0] / jr[..., 2] + c[:, None, 0], FOCAL[1] * jr[..., 1] / jr[..., 2] + c[:, None, 1]], -1)
        M = max(np.abs(proj).max(), np.abs(j2).max())
        worst["projection"] = max(worst.get("projection", 0), np.abs(proj - j2).max() / (8 * ULP * M))
        centre = (bb[:, None, :2] + 1.0) * c[:, None]
        crop = bb[:, None, 2:3] * (j2 - centre)
        M = (bb[:, 2].max()) * max(np.abs(j2).max(), np.abs(centre).max())
        worst["crop"] = max(worst.get("crop", 0), np.abs(crop - jc).max() / (20 * ULP * M))
        E = _np(new["extr%d" % s])[:, 0]
        for i in range(N):
            R, t = E[i, :3, :3], E[i, :3, 3]
            for key, src in (("smpl_vertices_rel", rec["smpl_vertices_wrt_origin"][i, 0]), ("smpl_joints_rel", rec["smpl_joints_wrt_origin"][i, 0]),
                             ("smpltrans_rel", rec["smpltrans"][i][None])):
                x = src.astype(np.float64)
                got = _np(new["%s%d" % (key, s)])[i].reshape(-1, 3)
                M = (np.abs(x) @ np.abs(R).T + np.abs(t)).max()
                worst["extrinsics"] = max(worst.get("extrinsics", 0), np.abs(x @ R.T + t - got).max() / (8 * ULP * M))
            o = rec["smplorient_rotmat_wrt_origin"][i, 0].astype(np.float64)
            got = _np(new["smplorient_rel%d" % s])[i, 0]
            M = (np.abs(R) @ np.abs(o)).max()
            worst["extrinsics"] = max(worst["extrinsics"], np.abs(R @ o - got).max() / (8 * ULP * M))
            worst["orthonormal"] = max(worst.get("orthonormal", 0), np.abs(got.T @ got - np.eye(3)).max() / (24 * ULP))
            assert abs(np.linalg.det(got) - 1) < 1e-5        # a rotation, not a reflection
            assert np.array_equal(E[i, 2:], _np(batch["extr%d" % s])[i, 0, 2:])            # rows 2 and 3 copied
    return worst


# ------------------------------------------------------------------------------------------------ no GPU
def test_methods_refuse_their_arguments_by_name():
    """types and shapes first, the devices last: all reachable with CPU tensors"""
    from airpose_amd import CameraRoll
    a = CameraRoll(device="cuda:0")
    n = 3
    index = torch.arange(n, dtype=torch.int32)
    f32, i32 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    batch = {"bb0": f32(n, 3), "bb1": f32(n, 3), "intr0": f32(n, 3, 3), "intr1": f32(n, 3, 3), "crops0": i32(n, 4), "crops1": i32(n, 4),
             "smpl_joints_rel0": f32(n, 1, 5, 3), "smpl_joints_rel1": f32(n, 1, 5, 3), "smpl_joints_2d0": f32(n, 1, 5, 2),
             "smpl_joints_2d1": f32(n, 1, 5, 2)}
    frames, rot = torch.zeros(2, n, 8, 9, 3, dtype=torch.uint8), f32(2, n, 2)
    with pytest.raises(RuntimeError, match="index must be a tensor, got list"):
        a.draw([1, 2, 3])
    with pytest.raises(RuntimeError, match="index must be int32 .* got torch.int64"):
        a.draw(index.long())
    with pytest.raises(RuntimeError, match=r"index must be \(n,\), got \(3, 1\)"):
        a.draw(index[:, None])
    with pytest.raises(RuntimeError, match="epoch must be an integer, got float"):
        a.draw(index, epoch=0.5)
    with pytest.raises(RuntimeError, match="cam must be None, 0, 1 or an"):
        a.draw(index, cam=2)
    with pytest.raises(RuntimeError, match=r"cam must be \(n,\) with n = 3, got \(2,\)"):
        a.draw(index, cam=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="index lives on cpu; it must be a CUDA .* there is no CPU path"):
        a.draw(index)
    with pytest.raises(RuntimeError, match="batch must be the dict"):
        a.apply([batch], frames, rot)
    with pytest.raises(RuntimeError, match="batch has no 'crops1'"):
        a.apply({k: v for k, v in batch.items() if k != "crops1"}, frames, rot)
    with pytest.raises(RuntimeError, match=r"batch\['bb1'\] must be float32 .* got torch.float64"):
        a.apply(dict(batch, bb1=batch["bb1"].double()), frames, rot)
    with pytest.raises(RuntimeError, match=r"batch\['intr0'\] must be .* with n = 3, got \(3, 4, 4\)"):
        a.apply(dict(batch, intr0=f32(n, 4, 4)), frames, rot)
    with pytest.raises(RuntimeError, match="batch has 'smpl_joints_rel0' without 'smpl_joints_rel1'"):
        a.apply({k: v for k, v in batch.items() if k != "smpl_joints_rel1"}, frames, rot)
    with pytest.raises(RuntimeError, match=r"batch\['smpl_joints_rel0'\] and batch\['smpl_joints_rel1'\] must have one shape"):
        a.apply(dict(batch, smpl_joints_rel1=f32(n, 1, 6, 3)), frames, rot)
    with pytest.raises(RuntimeError, match=r"batch\['smpl_joints_2d0'\] must end in 2 .* or 3"):
        a.apply(dict(batch, smpl_joints_2d0=f32(n, 1, 5, 4), smpl_joints_2d1=f32(n, 1, 5, 4)), frames, rot)
    with pytest.raises(RuntimeError, match=r"batch\['extr0'\] must be \(n, ...\) \+ \(4, 4\)"):
        a.apply(dict(batch, extr0=f32(n, 1, 3, 4), extr1=f32(n, 1, 3, 4)), frames, rot)
    with pytest.raises(RuntimeError, match="must hold the same points"):
        a.apply(dict(batch, smpl_joints_2d_crop0=f32(n, 6, 2), smpl_joints_2d_crop1=f32(n, 6, 2)), frames, rot)
    with pytest.raises(RuntimeError, match="frames must be uint8, got torch.float32"):
        a.apply(batch, frames.float(), rot)
    with pytest.raises(RuntimeError, match=r"frames must be \(2, n, Hc, Wc, 3\) with n = 3, got \(2, 2, 8, 9, 3\)"):
        a.apply(batch, frames[:, :2], rot)
    with pytest.raises(RuntimeError, match=r"frames\[1\] must be \(n, H, W, 3\) with n = 3"):
        a.apply(batch, (frames[0], frames[1, :2]), rot)
    with pytest.raises(RuntimeError, match="frames must be a .* tensor or the pair"):
        a.apply(batch, None, rot)
    with pytest.raises(RuntimeError, match=r"rot must be \(2, n, 2\) with n = 3, got \(2, 3\)"):
        a.apply(batch, frames, rot[..., 0])
    with pytest.raises(RuntimeError, match="rot must be float32"):
        a.apply(batch, frames, rot.double())
    with pytest.raises(RuntimeError, match="cam must be None, 0, 1 or an"):
        a.apply(dict(batch, cam=3), frames, rot)
    with pytest.raises(RuntimeError, match=r"batch\['bb0'\] lives on cpu; it must be a CUDA .* there is no CPU path"):
        a.apply(batch, frames, rot)
    with pytest.raises(RuntimeError, match="batch must be the dict"):
        a(None, frames, index)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_rolled_labels_are_one_camera_s_geometry(dev, synth):
    from airpose_amd import CameraRoll
    rec, frames, index, batch = synth
    base = _check_geometry(rec, batch, batch)                # the un-rolled dict meets the identities (their own bars are tighter)
    print("un-rolled, error / bar:", {k: round(v, 3) for k, v in base.items()})
    a = CameraRoll(device=dev)
    new = a.apply(batch, frames, _rot(25.0, -140.0, dev))
    assert not bool((a.status & U.CENTRE_OUT).any()), a.status
    worst = _check_geometry(rec, batch, new)
    print("rolled, error / bar:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1 for v in worst.values()), worst
    # the labels did move, by the planted angles
    for s, deg in ((0, 25.0), (1, -140.0)):
        r = _np(new["roll%d" % s])
        assert np.abs(r - (np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)))).max() < 1e-7
        assert not torch.equal(new["smpl_joints_rel%d" % s], batch["smpl_joints_rel%d" % s])
    # the new dict: rolled keys are new tensors of the old shapes, every other key is the same object
    rolled = {k + s for k in ("im", "bb", "smpl_vertices_rel", "smpl_joints_rel", "smplorient_rel", "smpltrans_rel", "extr", "smpl_joints_2d",
                              "smpl_joints_2d_crop") for s in "01"}
    assert set(new) == set(batch) | {"roll0", "roll1"} and new is not batch
    for k in batch:
        if k in rolled:
            assert new[k] is not batch[k] and new[k].shape == batch[k].shape and new[k].dtype == batch[k].dtype, k
            assert new[k].data_ptr() != batch[k].data_ptr(), k
        else:
            assert new[k] is batch[k], k
    assert tuple(a.status.shape) == (2, N) and a.status.dtype == torch.int32 and tuple(new["roll0"].shape) == (N, 2)


@pytest.mark.gpu
def test_a_blob_at_a_joint_stays_at_the_joint(dev, synth):
    from airpose_amd import CameraRoll
    rec, frames, index, batch = synth
    base = _centroid_error(batch)
    a = CameraRoll(device=dev)
    for deg0, deg1 in ((25.0, -140.0), (-140.0, 25.0)):
        new = a.apply(batch, frames, _rot(deg0, deg1, dev))
        assert not bool((a.status & U.CENTRE_OUT).any())
        err = _centroid_error(new)
        print("centroid error, un-rolled:", np.round(base, 3).tolist(), "rolled by (%g, %g):" % (deg0, deg1), np.round(err, 3).tolist())
        assert (err <= base + 0.5).all(), (deg0, deg1, err - base)
        assert not torch.equal(new["im0"], batch["im0"])
    # planted (1, 0): the batch's own images and labels, bit for bit
    same = a.apply(batch, frames, _rot(0.0, 0.0, dev))
    for k in ("im0", "im1", "bb0", "bb1", "smpl_vertices_rel0", "smpl_joints_2d1", "smpl_joints_2d_crop0", "extr1", "smplorient_rel0", "smpltrans_rel1"):
        assert torch.equal(same[k].contiguous().view(torch.int32), batch[k].contiguous().view(torch.int32)), k
    assert not bool(a.status.any())


@pytest.mark.gpu
def test_call_draws_with_the_dict_s_cameras_and_feeds_the_chain(dev, synth, copenet_sd):
    from airpose_amd import CameraRoll, CropAugment, copenet_model
    rec, frames, index, batch = synth
    a = CameraRoll(seed=U.SEED, p=1.0, max_deg=30.0, device=dev)
    new = a(batch, frames, index, epoch=2)
    rot = a.draw(index, 2, batch["cam0"])
    want = a.apply(batch, frames, rot)
    for k in ("im0", "im1", "bb1", "smpl_vertices_rel0", "roll0", "roll1"):
        assert torch.equal(new[k], want[k]), k
    gate, ang, cs = U.draw(U.SEED, 2, np.asarray(INDEX), batch["cam0"].cpu().numpy(), 1.0, np.float32(a.max_rad))
    assert gate.all() and np.abs(rot.cpu().numpy().astype(np.float64) - cs).max() <= 2.0 ** -23
    assert np.abs(ang).max() <= np.float32(np.pi / 6) and not torch.equal(new["im0"], batch["im0"])
    none = CameraRoll(seed=U.SEED, p=0.0, device=dev)(batch, frames, index, epoch=2)
    assert torch.equal(none["im0"], batch["im0"]) and torch.equal(none["smpl_joints_rel1"], batch["smpl_joints_rel1"])
    # batch -> CameraRoll -> CropAugment -> network
    aug = CropAugment(seed=U.SEED, p=1.0, device=dev)(new, index, epoch=2)
    assert aug["bb0"] is new["bb0"] and not torch.equal(aug["im0"], new["im0"])
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    with torch.no_grad():
        res = net.forward(aug["im0"], aug["im1"], aug["bb0"], aug["bb1"], aug["smpltrans_rel0"], aug["smpltrans_rel1"])
    assert len(res) == 4 and tuple(res[0].shape)[0] == N and all(bool(torch.isfinite(t).all()) for t in res)


@pytest.mark.gpu
@pytest.mark.parametrize("first_cam", [0, 1])
def test_real_data_dict(dev, first_cam):
    from airpose_amd import CameraRoll, RealSequenceBatches
    n = 2
    K = torch.zeros(2, 3, 3)
    for v, (cx, cy) in enumerate(RU.PRINCIPAL):
        K[v] = torch.tensor([[300.0 + 10 * v, 0.0, cx], [0.0, 310.0 + 10 * v, cy], [0.0, 0.0, 1.0]])
    g = torch.Generator().manual_seed(77)
    frames = [torch.randint(0, 256, (n, Hh, Ww, 3), generator=g, dtype=torch.uint8).to(dev) for Hh, Ww in RU.SIZES]
    rb = RealSequenceBatches(RU.case(50).to(dev), K, device=dev, border=50, first_cam=first_cam)
    batch = rb.batch(frames[0], frames[1], 1)
    a = CameraRoll(device=dev)
    ang = np.deg2rad(np.asarray([[12.0, 0.0], [-20.0, 8.0]]))
    rot = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32))
    rot[0, 1] = torch.tensor([1.0, 0.0])
    new = a.apply(batch, (frames[0], frames[1]), rot.to(dev))
    assert set(new) == set(batch) | {"roll0", "roll1"}      # no 3-D key appears
    status = a.status.cpu().numpy()
    for s in (0, 1):
        cam = first_cam ^ s
        Kc = K[cam].numpy()
        for i in range(n):
            c, sn, nbb, st = U.decide(rot[s, i].numpy(), Kc, batch["bb%d" % s][i].cpu().numpy())
            st |= U.off_canvas(c, sn, Kc, batch["crops%d" % s][i].cpu().numpy(), *RU.SIZES[cam])
            assert status[s, i] == st and new["roll%d" % s][i].cpu().tolist() == [float(c), float(sn)]
            assert np.array_equal(new["bb%d" % s][i].cpu().numpy().view(np.uint32), nbb.view(np.uint32))
            lab = {"j2d": batch["smpl_joints_2d%d" % s][i].cpu().numpy(), "j2d_crop": batch["smpl_joints_2d_crop%d" % s][i].cpu().numpy()}
            want = U.roll_labels(c, sn, Kc, lab)
            for k, key in (("j2d", "smpl_joints_2d"), ("j2d_crop", "smpl_joints_2d_crop")):
                got = new["%s%d" % (key, s)][i].cpu().numpy()
                assert got.shape == (2, 24, 3) and np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), (s, i, k)
                assert np.array_equal(got[..., 2].view(np.uint32), lab[k][..., 2].view(np.uint32))          # the confidences' bits
            if (s, i) == (0, 1):
                assert torch.equal(new["im0"][1], batch["im0"][1]) and torch.equal(new["smpl_joints_2d0"][1], batch["smpl_joints_2d0"][1])
            elif st & U.CENTRE_OUT == 0:
                assert not torch.equal(new["im%d" % s][i], batch["im%d" % s][i])
                img = U.roll_image(frames[cam][i].cpu().numpy(), batch["crops%d" % s][i].cpu().numpy(), c, sn, Kc, 1)
                assert np.array_equal(new["im%d" % s][i].cpu().numpy().view(np.uint32), img.view(np.uint32)), (s, i)
    for k in batch:
        if k[:-1] not in ("im", "bb", "smpl_joints_2d", "smpl_joints_2d_crop"):
            assert new[k] is batch[k], k
