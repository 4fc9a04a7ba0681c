"""apg_augment_crops and apg_augment_draw (airpose_amd/csrc/augment.hip) on the GPU against the contract of include/airpose_grad.h as
tests/augment_util.py restates it, through the C ABI.  n = 3 and both views: six images whose crop boxes give a wide, a tall, a
full, a one-row, an empty and a three-column letter-box, and six planted parameter sets (augment_util.planted_params) that are moved
round the images, so that every box meets every set.  Per image, by augment_util.check_image:
  (a) padding pixels, empty-content images and all-neutral images are BIT-IDENTICAL to the input;
  (b) with gamma = 1 and no noise the output is BIT-IDENTICAL to the numpy float32 restatement (blur, colour, clamp, occluders,
      re-normalisation: the point of -ffp-contract=off -fno-slp-vectorize);
  (c) and within the fp64 oracle's per-element bar: every rounding of the element's chain, 2^-24 |its result|, carried to the output;
  (d) gamma: against fp64 pow of the restatement's fp32 input, 2 ulp of powf (the ulp table of the device library is not installed
      here), times 2, plus the floor of the re-normalisation's own two roundings (augment_util's docstring says why); no element
      is left out;
  (e) noise: against the fp64 Box-Muller of the same Philox words, sigma 2^-20 (1 + sqrt(-2 ln u1)) plus 2 ulp.
  (f) the draws against augment_util.draw: integers and the fp32 ranges exact, color and blur_taps within 1 ulp of fp32;
  (g) a sample alone and as row 2 of a batch of 3: bit-identical parameters and pixels.
Measured on an MI355X (gfx950), the worst error / bar over all six rotations: (c) 0.31; (d) 0.76 where powf reaches, 0.92 on the
channels with gamma = 1 of those images, whose bar is the bare two-rounding floor; (e) 0.38; gamma and noise together 0.22."""
import ctypes

import numpy as np
import pytest
import torch

import augment_util as U
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)

EPOCH = 3


def run_crops(dev, x, boxes, P, index, cam=None, cam_all=0, seed=U.SEED, epoch=EPOCH, misalign=False):
    """apg_augment_crops on numpy inputs -> (out (2, n, 3, 224, 224) fp32 numpy, status (2, n))"""
    from airpose_amd import _native_grad as G
    n = x.shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if misalign:                                             # 4 bytes off a 16-byte boundary: the 4-byte loads and stores
        flat = torch.empty(x.size + 1, device=dev, dtype=torch.float32)
        im = flat[1:].view(x.shape)
        im.copy_(t(x))
        out = torch.empty(x.size + 1, device=dev, dtype=torch.float32)[1:].view(x.shape)
        assert im.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    else:
        im, out = t(x), torch.empty(x.shape, device=dev, dtype=torch.float32)
    d = {k: t(P[k]) for k in U.KEYS}
    crops, idx, status = t(boxes), t(index), torch.full((2, n), -1, device=dev, dtype=torch.int32)
    camt = None if cam is None else t(cam)
    vp = G.vp
    with torch.cuda.device(dev):
        G.check(G.lib().apg_augment_crops(n, seed, epoch, vp(idx), vp(camt), cam_all, vp(im), vp(crops), *[vp(d[k]) for k in U.KEYS],
                                          vp(out), vp(status), G.stream(dev)), "apg_augment_crops")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), status.cpu().numpy()


def run_draw(dev, index, cfg, cam=None, cam_all=0, seed=U.SEED, epoch=EPOCH):
    from airpose_amd import _native_grad as G
    n = len(index)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o = {k: torch.empty(v.shape, device=dev, dtype=torch.from_numpy(v).dtype) for k, v in U.neutral(n).items()}
    o["status"] = torch.full((2, n), -1, device=dev, dtype=torch.int32)
    idx, camt = t(np.asarray(index, np.int32)), None if cam is None else t(np.asarray(cam, np.int32))
    c = (ctypes.c_float * G.AUG_CFG)(*cfg)
    with torch.cuda.device(dev):
        G.check(G.lib().apg_augment_draw(n, seed, epoch, G.vp(idx), G.vp(camt), cam_all, c, *[G.vp(o[k]) for k in U.KEYS], G.vp(o["status"]),
                                         G.stream(dev)), "apg_augment_draw")
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in o.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("roll", range(6))
def test_planted_images_meet_the_contract(dev, roll):
    x, boxes = U.planted_images(), U.BOXES
    P = U.rolled(U.planted_params(), roll)
    out, status = run_crops(dev, x, boxes, P, U.INDEX, cam=U.CAM0)
    kinds = {}
    for s in (0, 1):
        for i in range(3):
            p = U.image_params(P, s, i)
            cam = (int(U.CAM0[i]) & 1) ^ s
            detail = {}
            kind, w = U.check_image(out[s, i], x[s, i], boxes[s, i], p, U.SEED, EPOCH, U.INDEX[i], cam, detail)
            print("roll %d, image (%d, %d): %-11s worst error / bar %.3f" % (roll, s, i, kind, w) +
                  (" (where a libm call reaches: %.3f)" % detail["libm"] if detail else ""))
            if detail:
                WORST[kind + " libm"] = max(WORST.get(kind + " libm", 0.0), detail["libm"])
            kinds[s, i] = kind
            WORST[kind] = max(WORST.get(kind, 0.0), w)
            assert w <= 1, (s, i, kind, w)
            assert status[s, i] == U.expected_status(boxes[s, i], p), (s, i, status[s, i])
    print("worst so far:", {k: round(v, 3) for k, v in WORST.items()})
    assert kinds[1, 1] == "copy"                             # the empty letter-box, whatever its parameters
    if roll == 0:
        assert kinds == {(0, 0): "exact", (0, 1): "gamma", (0, 2): "noise", (1, 0): "exact", (1, 1): "copy", (1, 2): "gamma+noise"}
        assert status[0, 0] == U.RECT_CLIPPED and status[0, 2] == U.RECT_CLIPPED and status[1, 1] == 0
        # the planted values did reach both clamps, the occluders and the noise
        inner = out[0, 0][:, 75:149].astype(np.float64) * U.STD[:, None, None] + U.MEAN[:, None, None]
        assert (np.abs(inner) < 1e-6).mean() > 0.05 and (np.abs(inner - 1) < 1e-6).mean() > 0.05
        assert np.allclose(inner[:, 30, 60], (0.1, 0.9, 0.6), atol=1e-6) and np.allclose(inner[:, 20, 35], (0.25, 0.5, 0.75), atol=1e-6)   # the later rect covers
        assert np.allclose(inner[:, 0, 160], (1.0, 0.0, 0.3), atol=1e-6)                   # row 75 of the rect that starts in the padding
        assert (out[0, 2] != x[0, 2]).mean() > 0.9


@pytest.mark.gpu
def test_neutral_parameters_and_unaligned_images(dev):
    x, boxes = U.planted_images(), U.BOXES
    out, status = run_crops(dev, x, boxes, U.neutral(3), U.INDEX)
    assert np.array_equal(bits(out), bits(x)) and not status.any()
    P = U.planted_params()
    a, sa = run_crops(dev, x, boxes, P, U.INDEX, cam=U.CAM0)
    b, sb = run_crops(dev, x, boxes, P, U.INDEX, cam=U.CAM0, misalign=True)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa, sb)
    # the same camera for the whole batch, given as a number: cam_all
    c, _ = run_crops(dev, x, boxes, P, U.INDEX, cam=np.ones(3, np.int32))
    d, _ = run_crops(dev, x, boxes, P, U.INDEX, cam_all=1)
    assert np.array_equal(bits(c), bits(d)) and not np.array_equal(bits(c[0, 2]), bits(run_crops(dev, x, boxes, P, U.INDEX)[0][0, 2]))
    # seed, epoch and index move the noise and nothing else
    for kw in (dict(seed=U.SEED + 1), dict(epoch=EPOCH + 1)):
        e, _ = run_crops(dev, x, boxes, P, U.INDEX, cam=U.CAM0, **kw)
        assert np.array_equal(bits(e[0, :2]), bits(a[0, :2])) and not np.array_equal(bits(e[0, 2]), bits(a[0, 2]))


@pytest.mark.gpu
def test_values_checked_on_the_device(dev):
    x, boxes = U.planted_images(), U.BOXES.copy()
    P = {k: v.copy() for k, v in U.planted_params().items()}
    P["blur_taps"][0, 0, 3] = np.nan                         # -> no blur
    P["color"][0, 2, 1, 1] = np.inf                          # -> [I | 0]
    P["gamma"][0, 1] = (np.nan, -2.0, 0.5)                   # -> 1, 1, 0.5
    P["noise_sigma"][1, 2] = -np.inf                         # -> 0
    P["rect_rgb"][0, 0, 2, 1] = np.nan                       # -> that rect is empty
    P["rect_rgb"][0, 1, 0] = (1.5, -0.5, 0.25)               # clamped to 1, 0, 0.25
    boxes[1, 0] = (50, 40, 0, 300)                           # inverted: the image is a copy
    out, status = run_crops(dev, x, boxes, P, U.INDEX, cam=U.CAM0)
    for s in (0, 1):
        for i in range(3):
            p = U.image_params(P, s, i)
            kind, w = U.check_image(out[s, i], x[s, i], boxes[s, i], p, U.SEED, EPOCH, U.INDEX[i], (int(U.CAM0[i]) & 1) ^ s)
            assert w <= 1 and status[s, i] == U.expected_status(boxes[s, i], p), (s, i, kind, w, status[s, i])
    assert status[0, 0] == status[0, 1] == status[0, 2] == U.NONFINITE | U.RECT_CLIPPED
    assert status[1, 0] == U.BAD_BOX and status[1, 1] == 0 and status[1, 2] == U.NONFINITE
    assert np.isfinite(out[0, :, :, 111, 100:124]).all()     # content pixels of the three images with a planted NaN or Inf
    assert np.array_equal(bits(out[1, 0]), bits(x[1, 0]))
    px = out[0, 1][:, 30, 80].astype(np.float64) * U.STD + U.MEAN
    assert np.allclose(px, (1.0, 0.0, 0.25), atol=1e-6)


@pytest.mark.gpu
def test_draws_are_the_oracle_s(dev):
    from airpose_amd import CropAugment
    n = 37                                                   # not a multiple of the draw kernel's 64 threads; 2 n = 74 > 64
    index = np.concatenate([U.INDEX, np.arange(5000, 5000 + n - 3)]).astype(np.int32)
    cam = (np.arange(n) % 3 == 0).astype(np.int32)
    for kw in (dict(), dict(p=1.0, occluders=4, blur_sigma=(1.5, 3.0)), dict(p=0.8, hue_deg=None, gamma=None, blur_sigma=0, occluders=1)):
        cfg = list(CropAugment(device=dev, seed=U.SEED, **kw)._cfg)
        got, want = run_draw(dev, index, cfg, cam=cam), U.draw(U.SEED, EPOCH, index, cam, cfg)
        for k in ("rects", "status"):
            assert np.array_equal(got[k], want[k]), (kw, k)
        for k in ("gamma", "noise_sigma", "rect_rgb"):       # fp32 chains of single roundings: exact
            assert np.array_equal(bits(got[k]), bits(want[k])), (kw, k)
        for k in ("color", "blur_taps"):                     # composed in fp64, rounded once: 1 ulp of fp32
            err = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64))
            assert (err <= U.ulp32(want[k])).all(), (kw, k, float((err / U.ulp32(want[k])).max()))
            assert ((got[k] == 0) == (want[k] == 0)).all() and ((got[k] == 1) == (want[k] == 1)).all(), (kw, k)
        if kw.get("p") == 1.0:
            assert (got["status"] != 0).any() and (got["status"] == 0).any() and (got["rects"][..., 1] > got["rects"][..., 0]).all()
    one = run_draw(dev, index[:1], cfg, cam_all=1)
    two = run_draw(dev, index[:1], cfg, cam=np.ones(1, np.int32))
    for k in U.KEYS:
        assert np.array_equal(one[k], two[k]), k


@pytest.mark.gpu
def test_a_sample_does_not_depend_on_its_batch(dev):
    """(index 7, epoch 3) alone, and the same sample as row 2 of a batch of 3: bit-identical parameters and pixels"""
    from airpose_amd import CropAugment
    cfg = list(CropAugment(device=dev, seed=U.SEED, p=1.0, blur_sigma=(0.5, 2.0), noise_sigma=(0.01, 0.03))._cfg)
    x, boxes = U.planted_images(), U.BOXES
    three = np.asarray([99, 12345, 7], np.int32)
    xa = np.stack([x[:, 2]] * 3, 1)                          # the square and the narrow box's images in every row
    ba = np.stack([boxes[:, 2]] * 3, 1)
    Pa, P1 = run_draw(dev, three, cfg, cam=np.asarray([0, 1, 1], np.int32)), run_draw(dev, three[2:], cfg, cam_all=1)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint32)  # (every parameter is 4 bytes wide)
    for k in U.KEYS:
        assert np.array_equal(raw(Pa[k][:, 2]), raw(P1[k][:, 0])), k
        assert not np.array_equal(Pa[k][:, 1], Pa[k][:, 2]), k
    oa, _ = run_crops(dev, xa, ba, {k: Pa[k] for k in U.KEYS}, three, cam=np.asarray([0, 1, 1], np.int32))
    o1, _ = run_crops(dev, xa[:, 2:], ba[:, 2:], {k: P1[k] for k in U.KEYS}, three[2:], cam_all=1)
    assert np.array_equal(bits(oa[:, 2]), bits(o1[:, 0])) and not np.array_equal(bits(oa[:, 1]), bits(oa[:, 2]))
    assert (P1["noise_sigma"] > 0).all() and (P1["blur_taps"][..., 1] > 0).all()           # every stage did run
