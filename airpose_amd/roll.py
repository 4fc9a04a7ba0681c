"""Camera-roll augmentation on the GPU: the crops rolled about the optical axis WITH their labels -- CameraRoll.

The geometric half of the training chain's augmentation (CropAugment is the photometric half).  AirPose looks at people from drones;
the in-image orientation of the person is set by the drone's yaw and roll, and the AerialPeople records cover only the orientations
that were rendered.  The exact form is a roll of the camera about its optical axis by theta, a rigid motion of the camera: every 3-D
label in the camera's frame is multiplied by Rz(theta), extr with it, every pixel coordinate turns about the principal point, the
crop box's centre (hence bb) turns with it and the crop's content turns about its own centre.  No label becomes approximate and the
two views stay consistent through extr.  The reference has no image-plane augmentation: its rottrans_tfm (not called) moves the
WORLD frame -- extr and the *_wrt_origin labels -- and no pixel.  Flips (a mirrored body is not a rigid motion) and zoom (it changes
the depth the network must predict at a fixed focal length) are NOT built.
  apg_roll_draw (csrc/roll.hip, include/airpose_grad.h): (cos, sin) of both views from stateless draws (Philox4x32-10 keyed by seed,
    counted by dataset index, epoch, camera and block 15, which no other stream of the data path uses);
  apg_roll_labels: one launch decides each (sample, view) -- a roll that would carry the crop centre out of a frame centred on the
    principal point is refused ON THE DEVICE and reported in status -- and rolls bb and every label the dict has, each byte read once
    and written once;
  apg_roll_crops: one launch rebuilds im0 / im1 from the frames: the batch's own pixel arithmetic where a view is not rolled
    (bit-identical), a bilinear sample of the zero-continued canvas where it is.
Three launches on the current stream, no host copy and no synchronisation.  A sample's roll depends on (seed, index, epoch, camera)
alone.  The defaults (p = 0.5, 30 degrees) are this class's own: NOBODY HAS MEASURED what they do to accuracy.  Use it between the
batch class and CropAugment, in training only: batch -> CameraRoll -> CropAugment -> network; never in validation or test.
There is no CPU path and no fallback: a missing library is an error.
"""
import math

import torch

from . import _args as A
from . import _native_grad as G

NAME = "CameraRoll"
IMG = 224
MAX_N, MAX_SIDE = 65535, 1 << 20                             # include/airpose_grad.h
# the labels that roll: key -> (the entry's argument, trailing shapes it may have with None = free)
LABELS = {"smpl_vertices_rel": "verts", "smpl_joints_rel": "joints", "smplorient_rel": "orient", "smpltrans_rel": "trans",
          "extr": "extr", "smpl_joints_2d": "j2d", "smpl_joints_2d_crop": "j2d_crop"}
ORDER = ("verts", "joints", "orient", "trans", "extr", "j2d", "j2d_crop")
NEEDED = ("bb", "intr", "crops")


def _number(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError("%s: %s must be a finite number, got %r" % (NAME, name, v))
    return float(v)


class CameraRoll:
    """CameraRoll(seed=0, p=0.5, max_deg=30.0, device=None)

    With probability p, drawn per (sample, view, epoch), the view's camera is rolled by an angle uniform in -max_deg .. max_deg
    degrees (0 .. 180).  The defaults are this class's own and their effect on accuracy is unmeasured.

    draw(index, epoch=0, cam=None) -> rot (2, n, 2) float32 = (cos, sin) per suffix; exactly (1, 0) where the gate is off.  index
      (n,) int32 on the device: the samples' dataset indices.  cam: the camera under suffix 0 -- a (n,) int32 device tensor
      (SyntheticBatches' cam0), 0 / 1 for the whole batch (RealSequenceBatches' cam), None = 0.
    apply(batch, frames, rot, bgr=True) -> dict: batch a SyntheticBatches / RealSequenceBatches dict; frames what the batch class
      took -- the (2, n, Hc, Wc, 3) uint8 tensor of SyntheticBatches.batch or the pair (frames0, frames1) of
      RealSequenceBatches.batch, indexed by camera; rot as draw() returns it, or planted.  The returned dict is new: im0/1, bb0/1,
      and, where the dict has them, smpl_vertices_rel, smpl_joints_rel, smpltrans_rel, smplorient_rel, extr, smpl_joints_2d and
      smpl_joints_2d_crop (both suffixes) are NEW tensors; every other key is the SAME object -- crops, crop_info, scale, pad and intr
      among them: crops keeps describing the un-rolled box, whose height and width are what CropAugment reads.  roll0 / roll1 (n, 2)
      hold the (cos, sin) actually used.  self.status holds the call's (2, n) int32 (_native_grad.ROLL_CENTRE_OUT: the roll was
      refused, the view is un-rolled; ROLL_OFF_CANVAS: a corner of the rolled box left the canvas, a black wedge shows).
    __call__(batch, frames, index, epoch=0, bgr=True) -> dict: draw, then apply; the camera is batch["cam0"] (synthetic), batch["cam"]
      (real), 0 when neither key exists.
    """

    def __init__(self, seed=0, p=0.5, max_deg=30.0, device=None):
        self.device = A.cuda_device(NAME, device)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError("%s: seed must be a whole number in 0 .. 2^64 - 1, got %r" % (NAME, seed))
        self.seed = seed
        self.p = _number(p, "p")
        if not 0.0 <= self.p <= 1.0:
            raise ValueError("%s: p must be in 0 .. 1, got %r" % (NAME, p))
        self.max_deg = _number(max_deg, "max_deg")
        if not 0.0 <= self.max_deg <= 180.0:
            raise ValueError("%s: max_deg must be in 0 .. 180, got %r" % (NAME, max_deg))
        self.max_rad = self.max_deg * (math.pi / 180.0)
        self.status = None

    # ---------------------------------------------------------------------------------------- the arguments
    @staticmethod
    def _cam(cam, n):
        """-> (tensor or None, whole-batch camera)"""
        if cam is None:
            return None, 0
        if torch.is_tensor(cam):
            A.exact_tensor(NAME, cam, torch.int32, "cam")
            if tuple(cam.shape) != (n,):
                raise RuntimeError("%s: cam must be (n,) with n = %d, got %s" % (NAME, n, tuple(cam.shape)))
            return cam, 0
        if isinstance(cam, bool) or not isinstance(cam, int) or cam not in (0, 1):
            raise RuntimeError("%s: cam must be None, 0, 1 or an (n,) int32 tensor, got %r" % (NAME, cam))
        return None, cam

    @staticmethod
    def _both(batch, key):
        """the two suffixes of a key as ONE contiguous (2, ...) tensor: a view where the batch class left them in one allocation"""
        a, b = batch[key + "0"], batch[key + "1"]
        t = A.pair_view(a, b)
        return torch.stack([a, b]) if t is None else t

    # ---------------------------------------------------------------------------------------- the draws
    def draw(self, index, epoch=0, cam=None):
        A.exact_tensor(NAME, index, torch.int32, "index")
        if index.dim() != 1 or index.shape[0] < 1:
            raise RuntimeError("%s: index must be (n,), got %s" % (NAME, tuple(index.shape)))
        n = int(index.shape[0])
        if n > MAX_N:
            raise RuntimeError("%s: a batch holds at most %d samples, got %d" % (NAME, MAX_N, n))
        cam_t, cam_all = self._cam(cam, n)
        epoch = A.epoch_index(NAME, epoch)
        A.lives_on(NAME, index, self.device, "index", "the roll")
        if cam_t is not None:
            A.lives_on(NAME, cam_t, self.device, "cam", "the roll")
            cam_t = cam_t.contiguous()
        dev = self.device
        index = index.contiguous()
        rot = torch.empty(2, n, 2, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            G.check(G.lib().apg_roll_draw(n, self.seed, epoch, G.vp(index), G.vp(cam_t), cam_all, self.p, self.max_rad, G.vp(rot),
                                          G.stream(dev)), "apg_roll_draw")
        return rot

    # ---------------------------------------------------------------------------------------- the batch dict
    def apply(self, batch, frames, rot, bgr=True):
        if not isinstance(batch, dict):
            raise RuntimeError("%s: batch must be the dict of SyntheticBatches / RealSequenceBatches, got %s" % (NAME, type(batch).__name__))
        for k in NEEDED:
            for s in "01":
                if k + s not in batch:
                    raise RuntimeError("%s: batch has no %r" % (NAME, k + s))
        ten = {}
        for k, dt in (("bb", torch.float32), ("intr", torch.float32), ("crops", torch.int32)):
            for s in "01":
                A.exact_tensor(NAME, batch[k + s], dt, "batch[%r]" % (k + s))
                ten["batch[%r]" % (k + s)] = batch[k + s]
        bb0 = batch["bb0"]
        if bb0.dim() != 2 or bb0.shape[1] != 3 or bb0.shape[0] < 1:
            raise RuntimeError("%s: batch['bb0'] must be (n, 3), got %s" % (NAME, tuple(bb0.shape)))
        n = int(bb0.shape[0])
        if n > MAX_N:
            raise RuntimeError("%s: a batch holds at most %d samples, got %d" % (NAME, MAX_N, n))
        for k, tail in (("bb", (3,)), ("intr", (3, 3)), ("crops", (4,))):
            for s in "01":
                if tuple(batch[k + s].shape) != (n,) + tail:
                    raise RuntimeError("%s: batch[%r] must be %s with n = %d, got %s" % (NAME, k + s, ("n",) + tail, n,
                                                                                         tuple(batch[k + s].shape)))
        # the labels the dict has
        have = {}
        for key, arg in LABELS.items():
            k0, k1 = key + "0", key + "1"
            if k0 not in batch and k1 not in batch:
                continue
            if k0 not in batch or k1 not in batch:
                raise RuntimeError("%s: batch has %r without %r" % (NAME, k1 if k0 not in batch else k0, k0 if k0 not in batch else k1))
            for k in (k0, k1):
                A.exact_tensor(NAME, batch[k], torch.float32, "batch[%r]" % k)
                ten["batch[%r]" % k] = batch[k]
            a, b = batch[k0], batch[k1]
            if a.shape != b.shape or a.dim() < 2 or a.shape[0] != n or a.numel() == 0:
                raise RuntimeError("%s: batch[%r] and batch[%r] must have one shape (n, ...) with n = %d, got %s and %s" %
                                   (NAME, k0, k1, n, tuple(a.shape), tuple(b.shape)))
            tail = {"orient": (3, 3), "trans": (3,), "extr": (4, 4)}.get(arg)
            last = tuple(a.shape[-len(tail):]) if tail else None
            if arg in ("verts", "joints") and a.shape[-1] != 3:
                raise RuntimeError("%s: batch[%r] must be (n, ..., 3), got %s" % (NAME, k0, tuple(a.shape)))
            if tail and (last != tail or a.numel() != n * math.prod(tail)):
                raise RuntimeError("%s: batch[%r] must be (n, ...) + %s, got %s" % (NAME, k0, tail, tuple(a.shape)))
            if arg in ("j2d", "j2d_crop") and a.shape[-1] not in (2, 3):
                raise RuntimeError("%s: batch[%r] must end in 2 (x, y) or 3 (x, y, confidence), got %s" % (NAME, k0, tuple(a.shape)))
            have[arg] = key
        V = batch["smpl_vertices_rel0"].numel() // (3 * n) if "verts" in have else 0
        J = batch["smpl_joints_rel0"].numel() // (3 * n) if "joints" in have else 0
        P = ps = 0
        for arg in ("j2d", "j2d_crop"):
            if arg in have:
                t = batch[have[arg] + "0"]
                p_here, ps_here = t.numel() // (int(t.shape[-1]) * n), int(t.shape[-1])
                if P and (p_here, ps_here) != (P, ps):
                    raise RuntimeError("%s: batch['smpl_joints_2d0'] and batch['smpl_joints_2d_crop0'] must hold the same points, got "
                                       "%s and %s" % (NAME, tuple(batch["smpl_joints_2d0"].shape), tuple(t.shape)))
                P, ps = p_here, ps_here
        # the canvases, by camera
        if torch.is_tensor(frames):
            if frames.dtype != torch.uint8:
                raise RuntimeError("%s: frames must be uint8, got %s" % (NAME, frames.dtype))
            if frames.dim() != 5 or frames.shape[0] != 2 or frames.shape[1] != n or frames.shape[4] != 3 or min(frames.shape[2:4]) < 1:
                raise RuntimeError("%s: frames must be (2, n, Hc, Wc, 3) with n = %d, got %s" % (NAME, n, tuple(frames.shape)))
            fr = [frames[0], frames[1]]
            ten["frames"] = frames
        elif isinstance(frames, (tuple, list)) and len(frames) == 2:
            fr = list(frames)
            for v, t in enumerate(fr):
                A.is_tensor(NAME, t, "frames[%d]" % v)
                if t.dtype != torch.uint8:
                    raise RuntimeError("%s: frames[%d] must be uint8, got %s" % (NAME, v, t.dtype))
                if t.dim() != 4 or t.shape[0] != n or t.shape[3] != 3 or min(t.shape[1:3]) < 1:
                    raise RuntimeError("%s: frames[%d] must be (n, H, W, 3) with n = %d, got %s" % (NAME, v, n, tuple(t.shape)))
                ten["frames[%d]" % v] = t
        else:
            raise RuntimeError("%s: frames must be a (2, n, Hc, Wc, 3) uint8 tensor or the pair (frames0, frames1), got %s" %
                               (NAME, type(frames).__name__))
        for v, t in enumerate(fr):
            if max(t.shape[1:3]) > MAX_SIDE:
                raise RuntimeError("%s: frames must be at most %d pixels a side, got %s" % (NAME, MAX_SIDE, tuple(t.shape)))
        A.exact_tensor(NAME, rot, torch.float32, "rot")
        if tuple(rot.shape) != (2, n, 2):
            raise RuntimeError("%s: rot must be (2, n, 2) with n = %d, got %s" % (NAME, n, tuple(rot.shape)))
        ten["rot"] = rot
        cam = batch["cam0"] if "cam0" in batch else batch.get("cam")
        cam_t, cam_all = self._cam(cam, n)
        if cam_t is not None:
            ten["batch['cam0']"] = cam_t
        for name, t in ten.items():
            A.lives_on(NAME, t, self.device, name, "the roll")

        dev = self.device
        fr = [t.contiguous() for t in fr]
        rot = rot.detach().contiguous()
        cam_t = None if cam_t is None else cam_t.contiguous()
        bb, intr, crops = (self._both(batch, k) for k in NEEDED)
        src = {arg: self._both(batch, key).detach() for arg, key in have.items()}
        out = {arg: torch.empty_like(t) for arg, t in src.items()}
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        rot_used, bb_out, im = f32(2, n, 2), f32(2, n, 3), f32(2, n, 3, IMG, IMG)
        status = torch.empty(2, n, device=dev, dtype=torch.int32)
        sizes = [int(fr[0].shape[1]), int(fr[0].shape[2]), int(fr[1].shape[1]), int(fr[1].shape[2])]
        vp = G.vp
        with torch.cuda.device(dev):
            st = G.stream(dev)
            G.check(G.lib().apg_roll_labels(n, V, J, P, ps, *sizes, vp(cam_t), cam_all, vp(rot), vp(intr), vp(bb.detach()), vp(crops),
                                            *[vp(src.get(a)) for a in ORDER], vp(rot_used), vp(bb_out), vp(status),
                                            *[vp(out.get(a)) for a in ORDER], st), "apg_roll_labels")
            G.check(G.lib().apg_roll_crops(n, *sizes, int(bool(bgr)), vp(fr[0]), vp(fr[1]), vp(cam_t), cam_all, vp(crops), vp(intr),
                                           vp(rot_used), vp(im), st), "apg_roll_crops")
        self.status = status
        new = dict(batch)
        for s in (0, 1):
            new["im%d" % s], new["bb%d" % s], new["roll%d" % s] = im[s], bb_out[s], rot_used[s]
            for arg, key in have.items():
                new["%s%d" % (key, s)] = out[arg][s]
        return new

    def __call__(self, batch, frames, index, epoch=0, bgr=True):
        if not isinstance(batch, dict):
            raise RuntimeError("%s: batch must be the dict of SyntheticBatches / RealSequenceBatches, got %s" % (NAME, type(batch).__name__))
        cam = batch["cam0"] if "cam0" in batch else batch.get("cam")
        return self.apply(batch, frames, self.draw(index, epoch, cam), bgr)
