"""apg_real_batch (airpose_amd/csrc/seq_batch.hip) through the C ABI against the fp64 restatement of copenet_real.py in
real_batch_util.py: frames of 120 x 160 and 90 x 200, L = 7, border 10 and 50, the spans (a, n) of real_batch_util.SPANS, coordinates
that are multiples of 1/8 (so x +- border and the sums are exact in fp32 and fp64 alike) and the planted cases of
real_batch_util.case.

Exact: crops, crop_info, status, the confidences; j2d is the input bit for bit except the zeroed confidences; bb[..., 2] is bit for
bit the scale ap_preprocess_crops writes for the same boxes.
bb[..., :2]: half an ulp at bb + 1 (the divide) and half an ulp at bb (the subtract): real_batch_util.bb_bar, which says why this is
the `2 ulp at the value's magnitude` of one rounding in each and is never wider.
j2d_crop: real_batch_util.crop_bar, the rounding budget of the fp32 chain at these frame sizes --
  (224 / smallest box side) * (2 * 2^-22 * 97.25 + 2^-17 + 2^-17) = 1.38e-3 px at border 10 (side 10), 2.76e-4 px at border 50 (side 50)
  over the whole sequence (a span that leaves the fallback frames out has a larger smallest side and a smaller bar)
-- beside the error of the same expression evaluated in fp32 on the host against the same fp64 (numpy, one rounding per operation,
which is what torch's fp32 does element-wise): measured on the CPU 1.46e-4 and 3.17e-5, so the derivation allows the kernel 9.4 and
8.7 times that floor.  The kernel is expected to BE that evaluation bit for bit; both figures are printed.

The hostile test runs the box kernel ONLY: it copies `crops` to the host and asserts the invariant for every row; nothing that reads
a frame is launched from those boxes."""
import ctypes

import numpy as np
import pytest
import torch

import real_batch_util as U
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)


def run(dev, det, a, n, border, agreement_px=U.AGREEMENT_PX):
    """one apg_real_batch launch -> dict of device tensors"""
    from airpose_amd import _native_grad as G
    d = det.to(dev).contiguous()
    f32 = lambda *s: torch.full(s, float("nan"), device=dev, dtype=torch.float32)          # (nothing may be left as it was)
    i32 = lambda *s: torch.full(s, -77, device=dev, dtype=torch.int32)
    o = dict(j2d=f32(2, n, 2, 24, 3), crops=i32(2, n, 4), crop_info=i32(2, n, 2, 2), bb=f32(2, n, 3), j2d_crop=f32(2, n, 2, 24, 3),
             status=i32(2, n))
    pr = (ctypes.c_float * 4)(*[c for p in U.PRINCIPAL for c in p])
    sz = G.ints([s for hw in U.SIZES for s in hw])
    with torch.cuda.device(dev):
        G.check(G.lib().apg_real_batch(det.shape[1], a, n, G.vp(d), pr, sz, float(agreement_px), int(border),
                                       *[G.vp(o[k]) for k in ("j2d", "crops", "crop_info", "bb", "j2d_crop", "status")], G.stream(dev)),
                "apg_real_batch")
    return o


@pytest.fixture(scope="module")
def outputs(dev):
    """every (border, span) once, copied to the host; the tests share them and leave them unchanged"""
    got = {}
    for border in U.BORDERS:
        for a, n in U.SPANS:
            got[border, a, n] = {k: v.cpu().numpy() for k, v in run(dev, U.case(border), a, n, border).items()}
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("border", U.BORDERS)
@pytest.mark.parametrize("a,n", U.SPANS)
def test_against_the_restatement(outputs, border, a, n):
    det, got = U.case(border), outputs[border, a, n]
    ref = U.ref_batch(det, a, n, border)
    r32 = U.ref_batch(det, a, n, border, dtype=np.float32)
    for k in ("crops", "crop_info", "status"):
        assert np.array_equal(got[k], ref[k]), k
    src = det[:, a:a + n].numpy()
    assert np.array_equal(got["j2d"][..., :2].view(np.int32), src[..., :2].view(np.int32))
    assert np.array_equal(got["j2d"][..., 2].view(np.int32), ref["j2d"][..., 2].astype(np.float32).view(np.int32))
    kept = got["j2d"][..., 2] != 0
    assert np.array_equal(got["j2d"][..., 2][kept].view(np.int32), src[..., 2][kept].view(np.int32))
    assert np.array_equal(got["j2d_crop"][..., 2].view(np.int32), got["j2d"][..., 2].view(np.int32))
    # bb
    err = np.abs(got["bb"][..., :2].astype(np.float64) - ref["bb"][..., :2])
    bar = U.bb_bar(ref["bb"][..., :2])
    same = np.array_equal(got["bb"].view(np.int32), r32["bb"].view(np.int32))
    print("border %d span (%d, %d): bb worst err / bar %.3f, bit-equal to the fp32 evaluation: %s" % (border, a, n, float((err / bar).max()), same))
    assert (err <= bar).all()
    assert np.array_equal(got["bb"][..., 2].view(np.int32), ref["scale"].astype(np.float32).view(np.int32))
    # j2d_crop
    side = min(int((ref["crops"][..., 1] - ref["crops"][..., 0]).min()), int((ref["crops"][..., 3] - ref["crops"][..., 2]).min()))
    cbar = U.crop_bar(side)                                  # (the span's own smallest side: never wider than the sequence's)
    e = float(np.abs(got["j2d_crop"][..., :2].astype(np.float64) - ref["j2d_crop"][..., :2]).max())
    floor = float(np.abs(r32["j2d_crop"][..., :2].astype(np.float64) - ref["j2d_crop"][..., :2]).max())
    same = np.array_equal(got["j2d_crop"].view(np.int32), r32["j2d_crop"].view(np.int32))
    print("border %d span (%d, %d): j2d_crop err %.3e px, the fp32 evaluation's %.3e px, bar %.3e px (smallest side %d), bit-equal: %s" %
          (border, a, n, e, floor, cbar, side, same))
    assert side >= border and e <= cbar


@pytest.mark.gpu
@pytest.mark.parametrize("border", U.BORDERS)
def test_the_inputs_tell_the_mutants_apart(outputs, border):
    det, got = U.case(border), outputs[border, 0, U.L]
    assert U.differs(got, U.ref_batch(det, 0, U.L, border)) == []
    for m in U.MUTATIONS:
        bad = U.differs(got, U.ref_batch(det, 0, U.L, border, mut=m))
        print("%s: %s" % (m, ", ".join(bad)))
        assert bad, m
    for m in U.EQUIVALENT:                                   # (real_batch_util's docstring: why this one cannot differ)
        assert U.differs(got, U.ref_batch(det, 0, U.L, border, mut=m)) == [], m


@pytest.mark.gpu
def test_scale_is_the_image_kernel_s(dev, outputs):
    """bb[..., 2] against the scale ap_preprocess_crops writes for the same (valid, checked above) boxes, bit for bit"""
    from airpose_amd import utils
    for border in U.BORDERS:
        got = outputs[border, 0, U.L]
        for v, (H, W) in enumerate(U.SIZES):
            frames = torch.zeros(U.L, H, W, 3, device=dev, dtype=torch.uint8)
            _, scale, _ = utils.preprocess_crops(frames, torch.from_numpy(got["crops"][v]))
            assert np.array_equal(scale.cpu().numpy().view(np.int32), got["bb"][v, :, 2].view(np.int32)), (border, v)


@pytest.mark.gpu
@pytest.mark.parametrize("border", [50, 0])
def test_hostile_input_keeps_the_box_invariant(dev, border):
    """NaN, +-inf, +-1e30 and negative coordinates under non-zero confidence: the box kernel alone, `crops` on the host, the
    invariant for every row, then the status bits and the boxes against the restatement.  border = 0 adds the empty axis: the lone
    keypoint on the corner (W, H) and the fallback box become one pixel"""
    det, want = U.hostile()
    got = {k: v.cpu().numpy() for k, v in run(dev, det, 0, U.L, border).items()}
    for v, (H, W) in enumerate(U.SIZES):
        y0, y1, x0, x1 = got["crops"][v].T.astype(np.int64)
        assert (0 <= x0).all() and (x0 < x1).all() and (x1 <= W).all(), (v, got["crops"][v])
        assert (0 <= y0).all() and (y0 < y1).all() and (y1 <= H).all(), (v, got["crops"][v])
    ref = U.ref_batch(det, 0, U.L, border)
    assert np.array_equal(got["crops"], ref["crops"]) and np.array_equal(got["crop_info"], ref["crop_info"])
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["status"] & (U.FALLBACK | U.CLAMPED), want.numpy())
    widened = (got["status"] & U.WIDENED) != 0
    if border:
        assert not widened.any()
    else:
        assert widened[:, 2].all() and widened[:, 5].all() and not widened[:, [0, 1, 3, 4, 6]].any()
        for v, (H, W) in enumerate(U.SIZES):
            assert got["crops"][v, 5].tolist() == [H - 1, H, W - 1, W] and got["crops"][v, 2].tolist() == [0, 1, 0, 1]
    assert np.isfinite(got["bb"]).all()
