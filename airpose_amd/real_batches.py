"""Real-data batches on the GPU: the two cameras' frames and the raw detections in, the network's inputs out -- RealSequenceBatches.

copenet_real/dsets/copenet_real.py: __getitem__ (:162-258) and the agreement filter of __init__ (:105-106), for a batch of consecutive
frames and both cameras:
  apg_real_batch (csrc/seq_batch.hip, include/airpose_grad.h): the two detectors filtered by agreement, the box round the surviving
    OpenPose keypoints with its border, bb = (box centre / principal point - 1, scale), the keypoints in crop coordinates;
  ap_preprocess_crops (libairpose_hip.so), once per camera, READING THE BOXES ON THE DEVICE: crop, letter-box, normalise.
Three launches on the current stream, no host copy and no synchronisation: the kernel itself guarantees that every box is non-empty and
inside its frame (the header's box invariant), which utils.preprocess_crops has to check on the host.  File I/O stays with the caller:
cv2.imread, the pickles, and the detector-format index maps op_map2smpl / al_map2smpl (index once; the tables are the reference's).
Two deviations from the reference, both the identity wherever the reference itself works: a keypoint outside the frame is clamped to
it before the box is taken, and a non-finite keypoint is treated as absent (`status` says where).  Parity of the images with cv2's
resize is UNPINNED, as for ap_preprocess_crops.  Per-sample camera shuffling is not built: shuffle per batch with first_cam.
There is no CPU path and no fallback: a missing library is an error.
"""
import ctypes
import operator

import torch

from . import _args as A
from . import _native as N
from . import _native_grad as G

NAME = "RealSequenceBatches"
AGREEMENT_PX, BORDER = 100.0, 50                             # copenet_real.py:22 (kp_agrmnt_threshold), :170 (border_buffer)
PRED_KEYS = {"pred_angles": (22, 3), "pred_smpltrans": (3,)}  # per view, what AirPosePlusSequence.prepare reads
IMG = 224


class RealSequenceBatches:
    """RealSequenceBatches(detections, intr, device=None, first_cam=0, agreement_px=100.0, border=50)

    detections (2 cameras, L, 2 detectors, 24, 3) = x, y, confidence, fp32 CUDA, detector 0 OpenPose and detector 1 AlphaPose in
    SMPL order with the unmapped joints 0: what AirPosePlusSequence.prepare takes.  intr (2, 3, 3): the cameras' matrices, on any
    device (the principal points are read on the host, once, here).  Shapes, types and devices are refused by name.

    batch(frames0, frames1, start, bgr=True) -> dict
      frames0 (n, H0, W0, 3), frames1 (n, H1, W1, 3): uint8 CUDA, the frames of cameras 0 and 1 at sequence positions
      [start, start + n) as cv2.imread returns them (bgr=True).  The reference's keys, camera `first_cam` under suffix 0 and the
      other camera under suffix 1: im (n, 3, 224, 224), bb (n, 3), intr (n, 3, 3) (an expanded view), crop_info (n, 2, 2) int32 =
      [[y0, x0], [y1, x1]], smpl_joints_2d and smpl_joints_2d_crop (n, 2, 24, 3) (row 0 OpenPose), plus crops (n, 4) int32 = y0, y1,
      x0, x1, scale (n,), pad (n, 2) int32 = left, top, status (n,) int32 (_native_grad.BATCH_*), and cam = first_cam.
      TwoViewInference.__call__ / submit and RealDataLoss.forward take the dict as it is.
    predict(pipe, frame_source, batch_size=64, **pipe_args) -> dict
      frame_source(start, stop) -> (frames0, frames1) is the caller's loader; pipe is a TwoViewInference.  Walks [0, L) and returns
      pred_angles0/1 (L, 22, 3), pred_smpltrans0/1 (L, 3) and status (2, L), all indexed by CAMERA (whatever first_cam is), so that
      the dict and `detections` go straight into AirPosePlusSequence.prepare.
    intr_fit: (2, 4) = fx, fy, cx, cy, what AirPosePlusSequence.fit takes.
    """

    def __init__(self, detections, intr, device=None, first_cam=0, agreement_px=AGREEMENT_PX, border=BORDER):
        self.device = A.cuda_device(NAME, device)
        if first_cam not in (0, 1):
            raise ValueError("%s: first_cam must be 0 or 1, got %r" % (NAME, first_cam))
        if not isinstance(agreement_px, (int, float)) or not 0 <= agreement_px < float("inf"):
            raise ValueError("%s: agreement_px must be a finite number that is not negative, got %r" % (NAME, agreement_px))
        if not isinstance(border, int) or isinstance(border, bool) or border < 0:
            raise ValueError("%s: border must be a whole number of pixels that is not negative, got %r" % (NAME, border))
        for t, nd, tail, name, what in ((detections, 5, (2, 24, 3), "detections", "(2, L, 2, 24, 3)"), (intr, 3, (3, 3), "intr", "(2, 3, 3)")):
            A.is_tensor(NAME, t, name)
            if not t.is_floating_point():
                raise RuntimeError("%s: %s must be a floating-point tensor, got %s" % (NAME, name, t.dtype))
            if t.dim() != nd or t.shape[0] != 2 or tuple(t.shape[-len(tail):]) != tail or t.shape[1] < 1:
                raise RuntimeError("%s: %s must be %s, got %s" % (NAME, name, what, tuple(t.shape)))
        A.exact_tensor(NAME, detections, torch.float32, "detections")
        A.lives_on(NAME, detections, self.device, "detections", "the batches")
        self.first_cam, self.agreement_px, self.border = int(first_cam), float(agreement_px), border
        self.detections = detections.detach().contiguous()
        self.L = int(detections.shape[1])
        K = intr.detach().to(device="cpu", dtype=torch.float32)                           # the one host copy, at construction
        self._principal = (ctypes.c_float * 4)(float(K[0, 0, 2]), float(K[0, 1, 2]), float(K[1, 0, 2]), float(K[1, 1, 2]))
        if not all(0 < c < float("inf") for c in self._principal):
            raise ValueError("%s: the principal points intr[:, :2, 2] must be finite and positive, got %s" % (NAME, list(self._principal)))
        self.intr = K.to(self.device)
        self.intr_fit = torch.stack([self.intr[:, 0, 0], self.intr[:, 1, 1], self.intr[:, 0, 2], self.intr[:, 1, 2]], 1).contiguous()

    def _frames(self, frames0, frames1, start):
        fs = (frames0, frames1)
        for v, t in enumerate(fs):
            A.is_tensor(NAME, t, "frames%d" % v)
            if t.dtype != torch.uint8:
                raise RuntimeError("%s: frames%d must be uint8, got %s" % (NAME, v, t.dtype))
            if t.dim() != 4 or t.shape[3] != 3 or min(t.shape[:3]) < 1:
                raise RuntimeError("%s: frames%d must be (n, H, W, 3), got %s" % (NAME, v, tuple(t.shape)))
        if frames0.shape[0] != frames1.shape[0]:
            raise RuntimeError("%s: frames0 and frames1 must hold the same number of frames, got %d and %d" %
                               (NAME, frames0.shape[0], frames1.shape[0]))
        n = int(frames0.shape[0])
        try:
            start = operator.index(start)
        except TypeError:
            raise RuntimeError("%s: start must be an integer, got %s" % (NAME, type(start).__name__)) from None
        if start < 0 or start + n > self.L:
            raise RuntimeError("%s: frames [start, start + n) must lie in the sequence's %d frames, got start = %r, n = %d" %
                               (NAME, self.L, start, n))
        for v, t in enumerate(fs):
            A.lives_on(NAME, t, self.device, "frames%d" % v, "the batches")
        return [t.contiguous() for t in fs], n, start

    def batch(self, frames0, frames1, start, bgr=True):
        frames, n, start = self._frames(frames0, frames1, start)
        dev = self.device
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        j2d, j2d_crop, bb = f32(2, n, 2, 24, 3), f32(2, n, 2, 24, 3), f32(2, n, 3)
        crops, crop_info, status = i32(2, n, 4), i32(2, n, 2, 2), i32(2, n)
        im, scale, pad = f32(2, n, 3, IMG, IMG), f32(2, n), i32(2, n, 2)
        size = G.ints([int(frames[0].shape[1]), int(frames[0].shape[2]), int(frames[1].shape[1]), int(frames[1].shape[2])])
        with torch.cuda.device(dev):
            st = G.stream(dev)
            G.check(G.lib().apg_real_batch(self.L, start, n, G.vp(self.detections), self._principal, size, self.agreement_px,
                                           self.border, G.vp(j2d), G.vp(crops), G.vp(crop_info), G.vp(bb), G.vp(j2d_crop),
                                           G.vp(status), st), "apg_real_batch")
            for v in (0, 1):                                 # the image kernel reads the boxes where the box kernel left them
                H, W = int(frames[v].shape[1]), int(frames[v].shape[2])
                N.check(N.lib().ap_preprocess_crops(G.vp(frames[v]), H * W * 3, n, H, W, int(bool(bgr)), G.vp(crops[v]), G.vp(im[v]),
                                                    G.vp(scale[v]), G.vp(pad[v]), st), "ap_preprocess_crops")
        out = {"cam": self.first_cam}
        for s in (0, 1):                                     # suffix s is camera first_cam ^ s: swapping is naming
            c = self.first_cam ^ s
            for key, t in (("im", im), ("bb", bb), ("crop_info", crop_info), ("smpl_joints_2d", j2d), ("smpl_joints_2d_crop", j2d_crop),
                           ("crops", crops), ("scale", scale), ("pad", pad), ("status", status)):
                out["%s%d" % (key, s)] = t[c]
            out["intr%d" % s] = self.intr[c].expand(n, 3, 3)
        return out

    def predict(self, pipe, frame_source, batch_size=64, **pipe_args):
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError("%s: batch_size must be a positive integer, got %r" % (NAME, batch_size))
        if not callable(frame_source):
            raise TypeError("%s: frame_source must be callable: frame_source(start, stop) -> (frames0, frames1)" % NAME)
        if "want_angles" in pipe_args:
            raise TypeError("%s.predict: want_angles is always on (AirPosePlusSequence.prepare reads the angles)" % NAME)
        L, dev = self.L, self.device
        out = {"%s%d" % (k, c): torch.empty((L,) + shape, device=dev, dtype=torch.float32) for k, shape in PRED_KEYS.items() for c in (0, 1)}
        out["status"] = torch.empty(2, L, device=dev, dtype=torch.int32)
        for a in range(0, L, batch_size):
            b = min(a + batch_size, L)
            frames0, frames1 = frame_source(a, b)
            batch = self.batch(frames0, frames1, a)
            if batch["im0"].shape[0] != b - a:
                raise RuntimeError("%s: frame_source(%d, %d) must return %d frames per camera, got %d" %
                                   (NAME, a, b, b - a, batch["im0"].shape[0]))
            res = pipe(batch, want_angles=True, **pipe_args)
            for s in (0, 1):                                 # the pipeline's outputs live in workspaces the next call reuses: copy
                c = self.first_cam ^ s
                for k in PRED_KEYS:
                    out["%s%d" % (k, c)][a:b].copy_(res["%s%d" % (k, s)])
                out["status"][c, a:b].copy_(batch["status%d" % s])
        return out
