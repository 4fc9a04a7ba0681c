"""apg_roll_labels, apg_roll_crops and apg_roll_draw (airpose_amd/csrc/roll.hip) on the GPU against the contract of
include/airpose_grad.h as tests/roll_util.py restates it, through the C ABI.  n = 3 and both views, the two-pointer form with one
canvas size per camera (96 x 128 and 61 x 47), boxes that give a wide, a tall, a full-canvas, a one-row, a three-column and a square
crop, V = 5, J = 3, a 2-D table of 4 points with stride 3, fx != fy in camera 1, every tensor placed 4 bytes off a 16-byte boundary.
The planted angles are 80 degrees on a view whose principal point makes that trip CENTRE_OUT, +7, 90 (the full canvas: OFF_CANVAS),
-7, 179 degrees and exactly (1, 0).
  1. a (1, 0) row -- planted, or left by the refusal -- gives the bits of apg_synth_crops on the same box and of the input labels;
  2. every label and every pixel is BIT-IDENTICAL to the numpy float32 restatement (roll.hip is compiled without contraction);
  3. every element lies within the fp64 oracle's per-element bar (roll_util's docstring derives it); no element is left out;
  4. the draws against the numpy Philox: the draw writes nothing but (cos, sin), so the gate word is read off as "exactly (1, 0) or
     not" and the angle word is held THROUGH cos and sin of the restated fp32 angle, within 1 ulp of fp32 -- not bit for bit: an
     angle off by an ulp near 0 would pass --; p = 0 and max_deg = 0 give all (1, 0);
  5. a sample alone and as row 2 of a batch of 3: identical bits;
  6. the status bits are exactly where the restatement puts them.
Measured on an MI355X (gfx950), worst error / bar: labels and bb 0.773; pixels 0.307 on each of the four rolled images, the padding's
two roundings of (0 - mean) / std.  The bits are the restatement's, so tests/test_roll_abi.py reports the same figures without a GPU."""
import numpy as np
import pytest
import torch

import roll_util as U
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)

EPOCH = 3


def off4(a, dev):
    """a numpy array on the device, 4 bytes off a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    skip = 4 // a.itemsize
    flat = torch.empty(a.size + skip, device=dev, dtype=t.dtype)
    out = flat[skip:].view(a.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def filled(shape, dtype, dev, misalign=True):
    """an output buffer that shows what was not written: NaN / -1"""
    n = int(np.prod(shape))
    flat = torch.full((n + 1,), float("nan") if dtype == torch.float32 else -1, device=dev, dtype=dtype)
    return (flat[1:] if misalign else flat[:-1]).view(shape)


def run_labels(dev, case, keys=U.LABEL_KEYS, cam_all=None, misalign=True):
    from airpose_amd import _native_grad as G
    put = (lambda a: off4(a, dev)) if misalign else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    n = case["rot"].shape[1]
    lab = {k: put(case["labels"][k]) for k in keys}
    out = {k: filled(case["labels"][k].shape, torch.float32, dev, misalign) for k in keys}
    rot, intr, bb, crops = put(case["rot"]), put(case["intr"]), put(case["bb"]), put(case["crops"])
    cam = None if cam_all is not None else put(case["cam"])
    rot_used, bb_out, status = filled((2, n, 2), torch.float32, dev, misalign), filled((2, n, 3), torch.float32, dev, misalign), \
        filled((2, n), torch.int32, dev, misalign)
    V = case["labels"]["verts"].shape[2] if "verts" in keys else 0
    J = case["labels"]["joints"].shape[2] if "joints" in keys else 0
    two = [k for k in ("j2d", "j2d_crop") if k in keys]
    P, ps = (case["labels"][two[0]].shape[2:] if two else (0, 0))
    (H0, W0), (H1, W1) = case["sizes"]
    vp = G.vp
    with torch.cuda.device(dev):
        G.check(G.lib().apg_roll_labels(n, V, J, P, ps, H0, W0, H1, W1, vp(cam), cam_all or 0, vp(rot), vp(intr), vp(bb), vp(crops),
                                        *[vp(lab.get(k)) for k in U.LABEL_KEYS], vp(rot_used), vp(bb_out), vp(status),
                                        *[vp(out.get(k)) for k in U.LABEL_KEYS], G.stream(dev)), "apg_roll_labels")
    torch.cuda.synchronize(dev)
    return dict(rot_used=rot_used.cpu().numpy(), bb_out=bb_out.cpu().numpy(), status=status.cpu().numpy(),
                labels={k: v.cpu().numpy() for k, v in out.items()})


def run_crops(dev, case, rot_used, bgr=1, cam_all=None, misalign=True):
    from airpose_amd import _native_grad as G
    put = (lambda a: off4(a, dev)) if misalign else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    n = rot_used.shape[1]
    fr = [put(f) for f in case["frames"]]
    crops, intr, ru = put(case["crops"]), put(case["intr"]), put(rot_used)
    cam = None if cam_all is not None else put(case["cam"])
    im = filled((2, n, 3, 224, 224), torch.float32, dev, misalign)
    (H0, W0), (H1, W1) = case["sizes"]
    vp = G.vp
    with torch.cuda.device(dev):
        G.check(G.lib().apg_roll_crops(n, H0, W0, H1, W1, bgr, vp(fr[0]), vp(fr[1]), vp(cam), cam_all or 0, vp(crops), vp(intr), vp(ru),
                                       vp(im), G.stream(dev)), "apg_roll_crops")
    torch.cuda.synchronize(dev)
    return im.cpu().numpy()


def run_synth_crops(dev, frame, box, bgr=1):
    """the batch's own image of one box: apg_synth_crops with the canvas under both cameras"""
    from airpose_amd import _native_grad as G
    Hc, Wc = frame.shape[:2]
    fr = torch.from_numpy(np.ascontiguousarray(np.stack([frame, frame])[:, None])).to(dev)
    crops = torch.from_numpy(np.ascontiguousarray(np.stack([box, box])[:, None]).astype(np.int32)).to(dev)
    flip = torch.zeros(1, device=dev, dtype=torch.int32)
    im, scale, pad = torch.empty(2, 1, 3, 224, 224, device=dev), torch.empty(2, 1, device=dev), torch.empty(2, 1, 2, device=dev, dtype=torch.int32)
    vp = G.vp
    with torch.cuda.device(dev):
        G.check(G.lib().apg_synth_crops(1, Hc, Wc, bgr, vp(fr), vp(crops), vp(flip), vp(im), vp(scale), vp(pad), G.stream(dev)), "apg_synth_crops")
    torch.cuda.synchronize(dev)
    return im[0, 0].cpu().numpy()


def run_draw(dev, index, p, max_rad, cam=None, cam_all=0, seed=U.SEED, epoch=EPOCH):
    from airpose_amd import _native_grad as G
    n = len(index)
    idx = off4(np.asarray(index, np.int32), dev)
    camt = None if cam is None else off4(np.asarray(cam, np.int32), dev)
    rot = filled((2, n, 2), torch.float32, dev)
    with torch.cuda.device(dev):
        G.check(G.lib().apg_roll_draw(n, seed, epoch, G.vp(idx), G.vp(camt), cam_all, p, max_rad, G.vp(rot), G.stream(dev)), "apg_roll_draw")
    torch.cuda.synchronize(dev)
    return rot.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def planted(dev):
    """the case, the restatement and the GPU's answer, once for the tests below"""
    c = U.case()
    want = U.restate(c)
    got = run_labels(dev, c)
    got["im"] = run_crops(dev, c, got["rot_used"])
    return c, want, got


@pytest.mark.gpu
def test_labels_status_and_decisions_are_the_restatement_s_bits(dev, planted):
    c, want, got = planted
    assert np.array_equal(got["status"], want["status"])     # (6)
    assert got["status"].tolist() == [[U.CENTRE_OUT, 0, U.OFF_CANVAS], [0, 0, 0]]
    assert np.array_equal(bits(got["rot_used"]), bits(want["rot_used"])) and np.array_equal(bits(got["bb_out"]), bits(want["bb_out"]))
    for k in U.LABEL_KEYS:                                   # (2): NaN-filled buffers, so every element was written
        assert np.array_equal(bits(got["labels"][k]), bits(want["labels"][k])), k
    for s, i in ((0, 0), (1, 2)):                            # (1): the refused and the planted (1, 0)
        assert got["rot_used"][s, i].tolist() == [1, 0]
        assert np.array_equal(bits(got["bb_out"][s, i]), bits(c["bb"][s, i]))
        for k in U.LABEL_KEYS:
            assert np.array_equal(bits(got["labels"][k][s, i]), bits(c["labels"][k][s, i])), (s, i, k)
    assert bits(got["labels"]["verts"][1, 2, 0, 0]) == 0x80000000                          # the negative zero came through
    for k in ("j2d", "j2d_crop"):                            # the third column is copied everywhere
        assert np.array_equal(bits(got["labels"][k][..., 2]), bits(c["labels"][k][..., 2]))
    assert np.array_equal(bits(got["bb_out"][..., 2]), bits(c["bb"][..., 2]))
    # (3) the oracle's bar, every element of every rolled row
    worst = 0.0
    for s in (0, 1):
        for i in range(U.N):
            cu, su = got["rot_used"][s, i]
            if cu == 1 and su == 0:
                continue
            K = c["intr"][s, i]
            o = U.roll_labels(cu, su, K, {k: v[s, i] for k, v in c["labels"].items()}, oracle=True)
            for k in o:
                worst = max(worst, U.worst(np.abs(got["labels"][k][s, i].astype(np.float64) - o[k].v), o[k].e))
            t = U.Turn(U.E(cu), U.E(su), U.E(K))
            u, v = U.fwd(t, U.E(c["bb"][s, i, 0]) * t.cx, U.E(c["bb"][s, i, 1]) * t.cy)
            for g, w in ((got["bb_out"][s, i, 0], u / t.cx), (got["bb_out"][s, i, 1], v / t.cy)):
                worst = max(worst, U.worst(abs(float(g) - w.v), w.e))
    print("labels and bb: worst error / bar %.3f" % worst)
    assert worst <= 1
    # the same bits from 16-byte aligned tensors
    again = run_labels(dev, c, misalign=False)
    for k in U.LABEL_KEYS:
        assert np.array_equal(bits(again["labels"][k]), bits(got["labels"][k])), k
    assert np.array_equal(again["status"], got["status"])


@pytest.mark.gpu
def test_pixels_are_the_restatement_s_bits_and_inside_the_oracle_s_bar(dev, planted):
    c, want, got = planted
    im = got["im"]
    assert np.isfinite(im).all()                             # NaN-filled: every pixel was written
    worst = 0.0
    for s in (0, 1):
        for i in range(U.N):
            cu, su = got["rot_used"][s, i]
            cam = U.camera_of(s, i)
            frame, box, K = c["frames"][cam][i], c["crops"][s, i], c["intr"][s, i]
            if cu == 1 and su == 0:                          # (1)
                assert np.array_equal(bits(im[s, i]), bits(run_synth_crops(dev, frame, box))), (s, i)
                continue
            a = U.roll_image(frame, box, cu, su, K, 1)
            assert np.array_equal(bits(im[s, i]), bits(a)), (s, i, int((bits(im[s, i]) != bits(a)).sum()))      # (2)
            v, bar = U.roll_image(frame, box, cu, su, K, 1, oracle=True)
            w = U.worst(np.abs(im[s, i].astype(np.float64) - v), bar)                      # (3)
            print("image (%d, %d): worst error / bar %.3f" % (s, i, w))
            worst = max(worst, w)
            assert w <= 1, (s, i, w)
    print("pixels: worst error / bar %.3f" % worst)
    # the content did turn: the quarter turn of the full canvas shows the canvas's centre column along the crop's centre row
    assert not np.array_equal(bits(im[0, 2]), bits(run_synth_crops(dev, c["frames"][0][2], c["crops"][0, 2])))
    # rgb order, 16-byte aligned tensors: the restatement's bits again
    rgb = run_crops(dev, c, got["rot_used"], bgr=0, misalign=False)
    assert np.array_equal(bits(rgb[0, 1]), bits(U.roll_image(c["frames"][1][1], c["crops"][0, 1], *got["rot_used"][0, 1], c["intr"][0, 1], 0)))


@pytest.mark.gpu
def test_absent_labels_and_a_table_of_stride_2(dev):
    c = U.case()
    c["labels"] = {"j2d": np.ascontiguousarray(c["labels"]["j2d"][..., :2]), "trans": c["labels"]["trans"]}
    want = U.restate(c)
    got = run_labels(dev, c, keys=("trans", "j2d"))
    for k in ("trans", "j2d"):
        assert np.array_equal(bits(got["labels"][k]), bits(want["labels"][k])), k
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(bits(got["bb_out"]), bits(want["bb_out"]))
    # a planted (1, 0) row with a zero focal length: tx and ty are exactly 0 there, so its corners are the box's and nothing is NaN
    c["intr"][1, 2, 0, 0] = 0.0
    flat = run_labels(dev, c, keys=("trans", "j2d"))
    assert np.array_equal(flat["status"], want["status"]) and flat["status"][1, 2] == 0 and flat["rot_used"][1, 2].tolist() == [1, 0]
    assert np.array_equal(bits(flat["labels"]["j2d"][1, 2]), bits(c["labels"]["j2d"][1, 2]))
    none = run_labels(dev, c, keys=())
    assert np.array_equal(none["status"], want["status"]) and np.array_equal(bits(none["rot_used"]), bits(want["rot_used"]))


@pytest.mark.gpu
def test_a_sample_alone_and_as_row_2_of_a_batch(dev, planted):
    c, _, got = planted
    one = dict(frames=[f[2:3] for f in c["frames"]], rot=c["rot"][:, 2:3], intr=c["intr"][:, 2:3], bb=c["bb"][:, 2:3], crops=c["crops"][:, 2:3],
               cam=c["cam"][2:3], sizes=c["sizes"], labels={k: v[:, 2:3] for k, v in c["labels"].items()})
    a = run_labels(dev, one)
    for k in U.LABEL_KEYS:
        assert np.array_equal(bits(a["labels"][k][:, 0]), bits(got["labels"][k][:, 2])), k
    assert np.array_equal(a["status"][:, 0], got["status"][:, 2]) and np.array_equal(bits(a["bb_out"][:, 0]), bits(got["bb_out"][:, 2]))
    im = run_crops(dev, one, a["rot_used"])
    assert np.array_equal(bits(im[:, 0]), bits(got["im"][:, 2]))
    # the camera as a number: sample 2's suffix 0 is camera 0
    b = run_crops(dev, one, a["rot_used"], cam_all=0)
    assert np.array_equal(bits(b), bits(im))


@pytest.mark.gpu
def test_draws_are_the_restatement_s(dev):
    n = 37                                                   # not a multiple of the draw kernel's 64 threads; 2 n = 74 > 64
    index = np.concatenate([[7, 123456, 2 ** 31 - 1], np.arange(5000, 5000 + n - 3)]).astype(np.int32)
    cam = (np.arange(n) % 3 == 0).astype(np.int32)
    for p, max_deg in ((0.5, 30.0), (1.0, 180.0), (0.8, 1.0)):
        max_rad = np.float32(max_deg * (np.pi / 180))
        got = run_draw(dev, index, p, max_rad, cam=cam)
        gate, ang, cs = U.draw(U.SEED, EPOCH, index, cam, p, max_rad)
        off = (got == np.asarray([1, 0], np.float32)).all(-1)
        assert np.array_equal(off, ~gate | (ang == 0)), (p, max_deg)                       # the gate words, exact
        err = np.abs(got.astype(np.float64) - cs)
        assert (err <= U.ulp32(cs)).all(), (p, max_deg, float((err / U.ulp32(cs)).max()))   # the angle words, through cos and sin
        assert np.abs((got.astype(np.float64) ** 2).sum(-1) - 1).max() < 4 * 2.0 ** -24
        if p == 1.0:
            assert gate.all() and np.abs(np.arctan2(got[..., 1], got[..., 0])).max() > 2.5
    for p, max_rad in ((0.0, np.float32(0.5)), (1.0, np.float32(0.0))):
        assert (run_draw(dev, index, p, max_rad, cam=cam) == np.asarray([1, 0], np.float32)).all(), (p, max_rad)
    one, two = run_draw(dev, index[:1], 1.0, np.float32(0.5), cam_all=1), run_draw(dev, index[:1], 1.0, np.float32(0.5), cam=np.ones(1, np.int32))
    assert np.array_equal(bits(one), bits(two))
    big = run_draw(dev, index, 1.0, np.float32(0.5), cam=cam)
    alone = run_draw(dev, index[2:3], 1.0, np.float32(0.5), cam=cam[2:3])
    assert np.array_equal(bits(alone[:, 0]), bits(big[:, 2]))
    for kw in (dict(seed=U.SEED + 1), dict(epoch=EPOCH + 1)):
        assert not np.array_equal(bits(run_draw(dev, index, 1.0, np.float32(0.5), cam=cam, **kw)), bits(big))
