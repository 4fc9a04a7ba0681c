"""Augmentation of the training crops on the GPU: blur, colour, gamma, noise and occluders -- CropAugment.

The reference's dataset lists its augmentations, commented out, at copenet/src/copenet/dsets/aerialpeople.py:72-76 (imgaug: brightness,
hue and saturation, colour temperature, per-channel gamma, grayscale).  The crops of SyntheticBatches and RealSequenceBatches are born
on the device, so this runs there too:
  apg_augment_draw (csrc/augment.hip, include/airpose_grad.h): one small launch writes the parameter set of both views -- the blur's
    taps, the colour matrix [M | b], the per-channel gamma, the noise's sigma, the occluders and their colours -- from stateless draws
    (Philox4x32-10 keyed by seed, counted by dataset index, epoch, camera and a block number >= 1, so that nothing collides with
    SyntheticBatches' jitter and flip under the same seed);
  apg_augment_crops: one launch applies a parameter set to all 2 n images, each read once and written once.
No host copy and no synchronisation.  A sample's augmentation depends on (seed, index, epoch, camera) alone: not on the batch it
arrives in and not on the camera shuffle.  The defaults are this class's own; imgaug is not a dependency and parity with it is
UNPINNED, as cv2's is for the crops and pyrender's for the renderer: the contract in include/airpose_grad.h is what is pinned and
tested.  There is no CPU path and no fallback: a missing library is an error.
"""
import ctypes
import math

import torch

from . import _args as A
from . import _native_grad as G

NAME = "CropAugment"
IMG = 224
MAX_N = 65535                                                # include/airpose_grad.h
# the parameter set: name -> (trailing shape, dtype)
PARAMS = {"blur_taps": ((G.AUG_MAX_RADIUS + 1,), torch.float32), "color": ((3, 4), torch.float32), "gamma": ((3,), torch.float32),
          "noise_sigma": ((), torch.float32), "rects": ((G.AUG_MAX_RECTS, 4), torch.int32),
          "rect_rgb": ((G.AUG_MAX_RECTS, 3), torch.float32)}


def _number(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError("%s: %s must be a finite number, got %r" % (NAME, name, v))
    return float(v)


def _pair(v, name, neutral, lo=None, hi=None):
    """a range (a, b) with a <= b inside [lo, hi]; None or 0 -> the neutral range (the stage is off)"""
    if v is None or (not isinstance(v, bool) and isinstance(v, (int, float)) and v == 0):
        return (neutral, neutral)
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a range (lo, hi), None or 0, got %r" % (NAME, name, v)) from None
    a, b = _number(a, name + "[0]"), _number(b, name + "[1]")
    if a > b or (lo is not None and a < lo) or (hi is not None and b > hi):
        raise ValueError("%s: %s must be lo <= hi within %s .. %s, got %r" % (NAME, name, "-inf" if lo is None else lo,
                                                                               "inf" if hi is None else hi, v))
    return (a, b)


def _amplitude(v, name):
    """a symmetric range -v .. v; None or 0 -> off"""
    if v is None:
        return 0.0
    v = _number(v, name)
    if v < 0:
        raise ValueError("%s: %s must be >= 0, got %r" % (NAME, name, v))
    return v


class CropAugment:
    """CropAugment(seed=0, p=0.5, blur_sigma=(0.0, 2.0), brightness=30/255, hue_deg=35.0, saturation=(0.6, 1.4),
                   channel_gain=(0.8, 1.2), gamma=(0.5, 2.0), grayscale=(0.0, 1.0), noise_sigma=(0.0, 0.03), occluders=2,
                   occluder_side=(0.1, 0.4), device=None)

    Each stage is applied with probability p, drawn separately per stage, image and epoch, with its strength uniform in its range:
    a Gaussian blur of sigma pixels (radius ceil(3 sigma), at most 6), brightness +-B on [0, 1] RGB, a hue rotation of +-hue_deg
    degrees in YIQ, saturation, a per-channel gain (colour temperature), a per-channel gamma, a blend towards grayscale, Gaussian
    noise, and `occluders` (0 .. 4) filled rectangles whose sides are fractions `occluder_side` of the 224-pixel crop.  A range of
    None, 0, or (x, x) at the stage's neutral value switches that stage off.  The letter-box padding of a crop is never touched.
    Parity with imgaug is UNPINNED (the module docstring); the arithmetic is include/airpose_grad.h's.

    draw(index, epoch=0, cam=None) -> params: blur_taps (2, n, 7), color (2, n, 3, 4), gamma (2, n, 3), noise_sigma (2, n), rects
      (2, n, 4, 4) int32, rect_rgb (2, n, 4, 3) and status (2, n) int32 (_native_grad.AUG_*), device tensors indexed by suffix.
      index (n,) int32 on the device: the samples' dataset indices (real data: start + arange(n)).  cam: the camera under suffix 0 --
      a (n,) int32 device tensor (SyntheticBatches' cam0), 0 / 1 for the whole batch (RealSequenceBatches' cam), None = 0.
    apply(im, crops, params, index, epoch=0, cam=None, out=None) -> (2, n, 3, 224, 224): im (2, n, 3, 224, 224) float32 and crops
      (2, n, 4) int32 = y0, y1, x0, x1 as the batch classes write them (the letter-box is recomputed from them); params as draw()
      returns them, or planted.  out must not overlap im.  self.status holds the call's (2, n) int32 status.
    __call__(batch, index, epoch=0) -> dict: a SyntheticBatches / RealSequenceBatches dict in; a new dict out with im0 / im1
      replaced and every other key the SAME object.  The camera of suffix s is batch["cam0"] ^ s (synthetic), batch["cam"] ^ s
      (real), s when neither key exists.
    """

    def __init__(self, seed=0, p=0.5, blur_sigma=(0.0, 2.0), brightness=30 / 255, hue_deg=35.0, saturation=(0.6, 1.4),
                 channel_gain=(0.8, 1.2), gamma=(0.5, 2.0), grayscale=(0.0, 1.0), noise_sigma=(0.0, 0.03), occluders=2,
                 occluder_side=(0.1, 0.4), device=None):
        self.device = A.cuda_device(NAME, device)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError("%s: seed must be a whole number in 0 .. 2^64 - 1, got %r" % (NAME, seed))
        self.seed = seed
        self.p = _number(p, "p")
        if not 0.0 <= self.p <= 1.0:
            raise ValueError("%s: p must be in 0 .. 1, got %r" % (NAME, p))
        if occluders is None:
            occluders = 0
        if isinstance(occluders, bool) or not isinstance(occluders, int) or not 0 <= occluders <= G.AUG_MAX_RECTS:
            raise ValueError("%s: occluders must be a whole number in 0 .. %d, got %r" % (NAME, G.AUG_MAX_RECTS, occluders))
        self.blur_sigma = _pair(blur_sigma, "blur_sigma", 0.0, lo=0.0)
        self.brightness = _amplitude(brightness, "brightness")
        self.hue_deg = _amplitude(hue_deg, "hue_deg")
        self.saturation = _pair(saturation, "saturation", 1.0, lo=0.0)
        self.channel_gain = _pair(channel_gain, "channel_gain", 1.0, lo=0.0)
        self.gamma = _pair(gamma, "gamma", 1.0, lo=0.0)
        self.grayscale = _pair(grayscale, "grayscale", 0.0, lo=0.0, hi=1.0)
        self.noise_sigma = _pair(noise_sigma, "noise_sigma", 0.0, lo=0.0)
        self.occluder_side = _pair(occluder_side, "occluder_side", 0.0, lo=0.0, hi=1.0)
        self.occluders = occluders if self.occluder_side != (0.0, 0.0) else 0
        cfg = [self.p, *self.blur_sigma, self.brightness, self.hue_deg, *self.saturation, *self.channel_gain, *self.gamma,
               *self.grayscale, *self.noise_sigma, float(self.occluders), *self.occluder_side]
        assert len(cfg) == G.AUG_CFG
        self._cfg = (ctypes.c_float * G.AUG_CFG)(*cfg)
        self.status = None

    # ---------------------------------------------------------------------------------------- the arguments
    def _index_cam(self, index, cam, n=None):
        """-> n, the device tensors to check, cam as (tensor or None, whole-batch camera)"""
        A.exact_tensor(NAME, index, torch.int32, "index")
        if index.dim() != 1 or index.shape[0] < 1 or (n is not None and index.shape[0] != n):
            raise RuntimeError("%s: index must be (n,)%s, got %s" % (NAME, "" if n is None else " with n = %d" % n, tuple(index.shape)))
        n = int(index.shape[0])
        if n > MAX_N:
            raise RuntimeError("%s: a batch holds at most %d samples, got %d" % (NAME, MAX_N, n))
        ten = {"index": index}
        if cam is None:
            return n, ten, (None, 0)
        if torch.is_tensor(cam):
            A.exact_tensor(NAME, cam, torch.int32, "cam")
            if tuple(cam.shape) != (n,):
                raise RuntimeError("%s: cam must be (n,) with n = %d, got %s" % (NAME, n, tuple(cam.shape)))
            ten["cam"] = cam
            return n, ten, (cam, 0)
        if isinstance(cam, bool) or not isinstance(cam, int) or cam not in (0, 1):
            raise RuntimeError("%s: cam must be None, 0, 1 or an (n,) int32 tensor, got %r" % (NAME, cam))
        return n, ten, (None, cam)

    def _devices(self, ten):
        for name, t in ten.items():
            A.lives_on(NAME, t, self.device, name, "the augmentation")

    # ---------------------------------------------------------------------------------------- the draws
    def draw(self, index, epoch=0, cam=None):
        n, ten, (cam_t, cam_all) = self._index_cam(index, cam)
        epoch = A.epoch_index(NAME, epoch)
        self._devices(ten)
        dev = self.device
        index = index.contiguous()
        cam_t = None if cam_t is None else cam_t.contiguous()
        o = {k: torch.empty((2, n) + tail, device=dev, dtype=dt) for k, (tail, dt) in PARAMS.items()}
        o["status"] = torch.empty(2, n, device=dev, dtype=torch.int32)
        vp = G.vp
        with torch.cuda.device(dev):
            G.check(G.lib().apg_augment_draw(n, self.seed, epoch, vp(index), vp(cam_t), cam_all, self._cfg,
                                             *[vp(o[k]) for k in PARAMS], vp(o["status"]), G.stream(dev)), "apg_augment_draw")
        return o

    # ---------------------------------------------------------------------------------------- the images
    def apply(self, im, crops, params, index, epoch=0, cam=None, out=None):
        A.exact_tensor(NAME, im, torch.float32, "im")
        if im.dim() != 5 or im.shape[0] != 2 or im.shape[1] < 1 or tuple(im.shape[2:]) != (3, IMG, IMG):
            raise RuntimeError("%s: im must be (2, n, 3, %d, %d), got %s" % (NAME, IMG, IMG, tuple(im.shape)))
        n = int(im.shape[1])
        n, ten, (cam_t, cam_all) = self._index_cam(index, cam, n)
        ten["im"] = im
        A.exact_tensor(NAME, crops, torch.int32, "crops")
        if tuple(crops.shape) != (2, n, 4):
            raise RuntimeError("%s: crops must be (2, n, 4) with n = %d, got %s" % (NAME, n, tuple(crops.shape)))
        ten["crops"] = crops
        if not isinstance(params, dict):
            raise RuntimeError("%s: params must be the dict draw() returns, got %s" % (NAME, type(params).__name__))
        for k, (tail, dt) in PARAMS.items():
            if k not in params:
                raise RuntimeError("%s: params has no %r" % (NAME, k))
            t = params[k]
            A.exact_tensor(NAME, t, dt, "params[%r]" % k)
            if tuple(t.shape) != (2, n) + tail:
                want = "(" + ", ".join(("2", "n") + tuple(map(str, tail))) + ")"
                raise RuntimeError("%s: params[%r] must be %s with n = %d, got %s" % (NAME, k, want, n, tuple(t.shape)))
            ten["params[%r]" % k] = t
        if out is not None:
            if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != tuple(im.shape) or not out.is_contiguous():
                raise RuntimeError("%s: out must be a contiguous float32 tensor of im's shape %s" % (NAME, tuple(im.shape)))
            ten["out"] = out
        epoch = A.epoch_index(NAME, epoch)
        self._devices(ten)
        dev = self.device
        im, crops, index = im.detach().contiguous(), crops.contiguous(), index.contiguous()
        cam_t = None if cam_t is None else cam_t.contiguous()
        if out is None:
            out = torch.empty_like(im)
        else:
            lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
            if im.data_ptr() < hi and lo < im.data_ptr() + im.numel() * 4:
                raise RuntimeError("%s: out must not overlap im (a blur in place would race across tile seams)" % NAME)
        status = torch.empty(2, n, device=dev, dtype=torch.int32)
        vp = G.vp
        with torch.cuda.device(dev):
            G.check(G.lib().apg_augment_crops(n, self.seed, epoch, vp(index), vp(cam_t), cam_all, vp(im), vp(crops),
                                              *[vp(params[k].contiguous()) for k in PARAMS], vp(out), vp(status), G.stream(dev)),
                    "apg_augment_crops")
        self.status = status
        return out

    # ---------------------------------------------------------------------------------------- the batch dict
    _pair_view = staticmethod(A.pair_view)                  # (shared with CameraRoll: _args.py)

    def __call__(self, batch, index, epoch=0):
        if not isinstance(batch, dict):
            raise RuntimeError("%s: batch must be the dict of SyntheticBatches / RealSequenceBatches, got %s" % (NAME, type(batch).__name__))
        for k in ("im0", "im1", "crops0", "crops1"):
            if k not in batch:
                raise RuntimeError("%s: batch has no %r" % (NAME, k))
            A.is_tensor(NAME, batch[k], "batch[%r]" % k)
        for v in (0, 1):
            t = batch["im%d" % v]
            if t.dim() != 4 or tuple(t.shape[1:]) != (3, IMG, IMG) or t.shape != batch["im0"].shape:
                raise RuntimeError("%s: batch['im%d'] must be (n, 3, %d, %d), got %s" % (NAME, v, IMG, IMG, tuple(t.shape)))
        cam = batch["cam0"] if "cam0" in batch else batch.get("cam")
        # suffix 1 stored in front of suffix 0 (RealSequenceBatches with first_cam = 1): the same pair, rows swapped
        swap = False
        im = self._pair_view(batch["im0"], batch["im1"])
        if im is None and not torch.is_tensor(cam) and cam in (None, 0, 1):
            im = self._pair_view(batch["im1"], batch["im0"])
            swap = im is not None
        names = ("1", "0") if swap else ("0", "1")
        if im is None:
            im = torch.stack([batch["im0"], batch["im1"]])
        crops = self._pair_view(batch["crops" + names[0]], batch["crops" + names[1]])
        if crops is None:
            crops = torch.stack([batch["crops" + names[0]], batch["crops" + names[1]]])
        if swap:
            cam = 1 - (cam or 0)
        out = self.apply(im, crops, self.draw(index, epoch, cam), index, epoch, cam)
        if swap:
            self.status = self.status.flip(0)                # (indexed by suffix again)
        new = dict(batch)
        new["im" + names[0]], new["im" + names[1]] = out[0], out[1]
        return new
