"""Synthetic-data batches on the GPU: AerialPeople records and images in, the trainers' batch dict out -- SyntheticBatches.

copenet/src/copenet/dsets/aerialpeople.py, aerialpeople_crop.__getitem__ (:81-226), for n samples and both cameras:
  apg_synth_batch (csrc/synth_batch.hip, include/airpose_grad.h): the jittered crop boxes, bb, crop_info, the ground truth in each
    camera's frame (vertices, joints, orientation, translation, the joints in pixels and in crop pixels), smplpose_rotmat and the
    per-sample camera shuffle, every per-view output written to its suffix's row by the kernels;
  apg_synth_crops: both suffixes' images in one launch, READING THE BOXES AND FLIPS ON THE DEVICE (the arithmetic of
    ap_preprocess_crops, one source);
  SMPLX.forward once per gender present, on the rows of that gender (grouped on the host from the gender strings), for the
    canonical body smpl_vertices / smpl_joints.
No host copy and no synchronisation: the kernel itself guarantees that every box is non-empty and inside its canvas (the header's box
invariant), and `status` says where a rule had to act.  File I/O stays with the caller: the pickles and cv2.imread.  The draws are
stateless (Philox4x32-10 keyed by seed, counted by dataset index, epoch and camera), so a sample's jitter and shuffle do not depend
on the batch it arrives in, and they are not numpy's: the reference's np.random stream is not reproduced.  Parity of the images with
cv2's resize is UNPINNED, as for ap_preprocess_crops.  There is no CPU path and no fallback: a missing library is an error.
"""
import torch

from . import _args as A
from . import _native_grad as G
from .pipeline import FOCAL_LENGTH
from .smplx import SMPLX

NAME = "SyntheticBatches"
GENDERS = ("male", "female", "neutral")
IMG = 224
MAX_SIDE, MAX_N = 1 << 20, 65535                             # include/airpose_grad.h
# records: field -> (what it must be, trailing shape with None = free, dtype)
FIELDS = {"bb": ("(n, 2, 2, 2)", (2, 2, 2), torch.int32), "intr": ("(n, 2, 3, 3)", (2, 3, 3), torch.float32),
          "extr": ("(n, 2, 4, 4)", (2, 4, 4), torch.float32), "smplpose": ("(n, 63)", (63,), torch.float32),
          "smplshape": ("(n, 10)", (10,), torch.float32), "smpl_vertices_wrt_origin": ("(n, 1, V, 3)", (1, None, 3), torch.float32),
          "smpl_joints_wrt_origin": ("(n, 1, J, 3)", (1, None, 3), torch.float32),
          "smplorient_rotmat_wrt_origin": ("(n, 1, 3, 3)", (1, 3, 3), torch.float32), "smpltrans": ("(n, 3)", (3,), torch.float32)}
VIEW_KEYS = ("im", "intr", "extr", "bb", "crop_info", "smpltrans_rel", "smplorient_rel", "smpl_vertices_rel", "smpl_joints_rel",
             "smpl_joints_2d", "smpl_joints_2d_crop", "crops", "scale", "pad", "status")


def _whole(v, lo, hi, name):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError("%s: %s must be a whole number in %d .. %d, got %r" % (NAME, name, lo, hi, v))
    return v


class SyntheticBatches:
    """SyntheticBatches(smplx_models, device=None, frame_size=(1080, 1920), margin=200, focal_length=(1475.0, 1475.0), seed=0,
                        jitter=True, shuffle=True)

    smplx_models: {"male" | "female" | "neutral": airpose_amd.SMPLX}, any non-empty subset; a gender met in a batch without its
    model is refused by name (as in the reference, a gender string that is neither "male" nor "female" in any case is neutral).
    frame_size = (H, W) of the frames the records' boxes refer to; margin: the reference's 200 pixels round the box.

    batch(records, frames, index, epoch=0, bgr=True, origin="region") -> dict
      records: the pickle's fields of n samples, stacked, on the device: bb (n, 2 cameras, 2, 2) int32 = [[x0, y0], [x1, y1]], intr
        (n, 2, 3, 3), extr (n, 2, 4, 4), smplpose (n, 63), smplshape (n, 10), smpl_vertices_wrt_origin (n, 1, V, 3),
        smpl_joints_wrt_origin (n, 1, J, 3), smplorient_rotmat_wrt_origin (n, 1, 3, 3), smpltrans (n, 3), all float32 (nothing is
        cast), and smplgender, a HOST list of n strings.
      frames (2 cameras, n, Hc, Wc, 3) uint8: one canvas size for both cameras.  origin="region" (the reference's pre-cropped
        dataset): the image of the region crop_info = [[ymin, xmin], [ymax, xmax]] sits at the canvas's top-left; origin="frame":
        the canvas is the whole frame.  bgr=True for cv2.imread images.
      index (n,) int32 on the device: the samples' dataset indices; with seed and epoch they key the draws.
      The reference's keys: im0/1 (n, 3, 224, 224), intr0/1 (n, 3, 3), extr0/1 (n, 1, 4, 4), bb0/1 (n, 3), crop_info0/1 (n, 2, 2)
      int32, smplbetas (n, 10), smpltrans_rel0/1 (n, 3), smplpose_rotmat (n, 21, 3, 3), focal_length (n, 2), img_size (n, 2) = W, H,
      smplorient_rel0/1 (n, 1, 3, 3), smpl_vertices_rel0/1 (n, 1, V, 3), smpl_joints_rel0/1 (n, 1, J, 3), smpl_joints_2d0/1
      (n, 1, J, 2), smpl_joints_2d_crop0/1 (n, J, 2), smpl_vertices (n, 1, Vm, 3), smpl_joints (n, 1, Jm, 3) (the model's own
      counts), smpl_gender; plus crops0/1 (n, 4) int32 = y0, y1, x0, x1 on the canvas, scale0/1 (n,), pad0/1 (n, 2) int32 = left,
      top, status0/1 (n,) int32 (_native_grad.SYNTH_*) and cam0 (n,) int32: the camera under suffix 0.  Suffix s of sample i is
      camera cam0[i] ^ s.  TwoViewInference.__call__ / submit, copenet.forward, TrainingLoss.forward, EvalMetrics.update and
      MeshMetrics.update take the dict as it is.
    """

    def __init__(self, smplx_models, device=None, frame_size=(1080, 1920), margin=200, focal_length=FOCAL_LENGTH, seed=0,
                 jitter=True, shuffle=True):
        self.device = A.cuda_device(NAME, device)
        if not isinstance(smplx_models, dict) or not smplx_models:
            raise TypeError("%s: smplx_models must be a non-empty dict of %s -> airpose_amd.SMPLX" % (NAME, " / ".join(GENDERS)))
        for g, m in smplx_models.items():
            if g not in GENDERS:
                raise ValueError("%s: smplx_models has the key %r; the genders are %s" % (NAME, g, ", ".join(GENDERS)))
            if not isinstance(m, SMPLX):
                raise TypeError("%s: smplx_models[%r] must be an airpose_amd.SMPLX, got %s" % (NAME, g, type(m).__name__))
        self.models = dict(smplx_models)
        try:
            H, W = frame_size
        except (TypeError, ValueError):
            raise ValueError("%s: frame_size must be (H, W), got %r" % (NAME, frame_size)) from None
        self.frame_size = (_whole(H, 1, MAX_SIDE, "frame_size[0]"), _whole(W, 1, MAX_SIDE, "frame_size[1]"))
        self.margin = _whole(margin, 0, MAX_SIDE, "margin")
        self.seed = _whole(seed, 0, 2 ** 64 - 1, "seed")
        f = (focal_length, focal_length) if isinstance(focal_length, (int, float)) else tuple(focal_length)
        if len(f) != 2 or not all(isinstance(v, (int, float)) and abs(v) < float("inf") for v in f):
            raise ValueError("%s: focal_length must be a finite number or a pair of them, got %r" % (NAME, focal_length))
        self.focal_length = (float(f[0]), float(f[1]))
        self.jitter, self.shuffle = bool(jitter), bool(shuffle)
        self._const = None                                   # focal_length, img_size, I and 0 on the device, made at the first batch

    # ---------------------------------------------------------------------------------------- the arguments
    def _check(self, records, frames, index, epoch, origin):
        """types and shapes first, devices last (so that a wrong argument is named as such on any machine)"""
        if not isinstance(records, dict):
            raise RuntimeError("%s: records must be a dict of the record's fields, got %s" % (NAME, type(records).__name__))
        for k in tuple(FIELDS) + ("smplgender",):
            if k not in records:
                raise RuntimeError("%s: records has no %r" % (NAME, k))
        ten = {"records[%r]" % k: (records[k], "(n,) + " + str(tail), dt, what) for k, (what, tail, dt) in FIELDS.items()}
        ten["frames"] = (frames, None, torch.uint8, "(2, n, Hc, Wc, 3)")
        ten["index"] = (index, None, torch.int32, "(n,)")
        for name, (t, _, dt, what) in ten.items():
            A.exact_tensor(NAME, t, dt, name)
        bb = records["bb"]
        n = int(bb.shape[0]) if bb.dim() else 0
        for k, (what, tail, _) in FIELDS.items():
            t = records[k]
            ok = t.dim() == 1 + len(tail) and t.shape[0] == n and all(w is None or w == s for w, s in zip(tail, t.shape[1:]))
            if not ok or n < 1 or t.numel() == 0:
                raise RuntimeError("%s: records[%r] must be %s with n = %d, got %s" % (NAME, k, what, n, tuple(t.shape)))
        if n > MAX_N:
            raise RuntimeError("%s: a batch holds at most %d samples, got %d" % (NAME, MAX_N, n))
        if frames.dim() != 5 or frames.shape[0] != 2 or frames.shape[1] != n or frames.shape[4] != 3 or min(frames.shape[2:4]) < 1:
            raise RuntimeError("%s: frames must be (2, n, Hc, Wc, 3) with n = %d, got %s" % (NAME, n, tuple(frames.shape)))
        if max(frames.shape[2:4]) > MAX_SIDE:
            raise RuntimeError("%s: frames must be at most %d pixels a side, got %s" % (NAME, MAX_SIDE, tuple(frames.shape)))
        if tuple(index.shape) != (n,):
            raise RuntimeError("%s: index must be (n,) with n = %d, got %s" % (NAME, n, tuple(index.shape)))
        genders = records["smplgender"]
        if not isinstance(genders, (list, tuple)) or len(genders) != n or not all(isinstance(g, str) for g in genders):
            raise RuntimeError("%s: records['smplgender'] must be a host list of n = %d strings" % (NAME, n))
        epoch = A.epoch_index(NAME, epoch)
        if origin not in G.SYNTH_ORIGINS:
            raise RuntimeError("%s: origin must be 'region' or 'frame', got %r" % (NAME, origin))
        rows = {}
        for i, g in enumerate(genders):                      # the reference's rule: FEMALE, MALE, anything else is neutral
            g = g.lower() if g.lower() in ("male", "female") else "neutral"
            rows.setdefault(g, []).append(i)
        for g in rows:
            if g not in self.models:
                raise RuntimeError("%s: sample %d is %s and smplx_models has no %r model" % (NAME, rows[g][0], g, g))
        for name, (t, _, _, _) in ten.items():
            A.lives_on(NAME, t, self.device, name, "the batches")
        return n, epoch, rows

    def _constants(self):
        if self._const is None:
            dev = self.device
            self._const = (torch.tensor(self.focal_length, device=dev, dtype=torch.float32),
                           torch.tensor([self.frame_size[1], self.frame_size[0]], device=dev, dtype=torch.float32),
                           torch.eye(3, device=dev, dtype=torch.float32).reshape(1, 1, 3, 3), torch.zeros(1, 3, device=dev))
        return self._const

    # ---------------------------------------------------------------------------------------- the batch
    def batch(self, records, frames, index, epoch=0, bgr=True, origin="region"):
        n, epoch, rows = self._check(records, frames, index, epoch, origin)
        dev = self.device
        r = {k: records[k].detach().contiguous() for k in FIELDS}
        frames, index = frames.contiguous(), index.contiguous()
        V, J = int(r["smpl_vertices_wrt_origin"].shape[2]), int(r["smpl_joints_wrt_origin"].shape[2])
        Hc, Wc = int(frames.shape[2]), int(frames.shape[3])
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
        o = dict(crops=i32(2, n, 4), crop_info=i32(2, n, 2, 2), status=i32(2, n), flip=i32(n), bb=f32(2, n, 3), intr=f32(2, n, 3, 3),
                 extr=f32(2, n, 1, 4, 4), smpl_vertices_rel=f32(2, n, 1, V, 3), smpl_joints_rel=f32(2, n, 1, J, 3),
                 smplorient_rel=f32(2, n, 1, 3, 3), smpltrans_rel=f32(2, n, 3), smpl_joints_2d=f32(2, n, 1, J, 2),
                 smpl_joints_2d_crop=f32(2, n, J, 2), smplpose_rotmat=f32(n, 21, 3, 3))
        o.update(im=f32(2, n, 3, IMG, IMG), scale=f32(2, n), pad=i32(2, n, 2))
        focal, img_size, eye, zero = self._constants()
        vp = G.vp
        with torch.cuda.device(dev):
            st = G.stream(dev)
            G.check(G.lib().apg_synth_batch(
                n, V, J, self.frame_size[0], self.frame_size[1], Hc, Wc, self.margin, G.SYNTH_ORIGINS[origin], int(self.jitter),
                int(self.shuffle), self.focal_length[0], self.focal_length[1], self.seed, epoch, vp(index), vp(r["bb"]), vp(r["intr"]),
                vp(r["extr"]), vp(r["smplpose"]), vp(r["smpl_vertices_wrt_origin"]), vp(r["smpl_joints_wrt_origin"]),
                vp(r["smplorient_rotmat_wrt_origin"]), vp(r["smpltrans"]),
                *[vp(o[k]) for k in ("crops", "crop_info", "status", "flip", "bb", "intr", "extr", "smpl_vertices_rel", "smpl_joints_rel",
                                     "smplorient_rel", "smpltrans_rel", "smpl_joints_2d", "smpl_joints_2d_crop", "smplpose_rotmat")],
                st), "apg_synth_batch")
            # the image kernel reads the boxes and the flips where the box kernel left them
            G.check(G.lib().apg_synth_crops(n, Hc, Wc, int(bool(bgr)), vp(frames), vp(o["crops"]), vp(o["flip"]), vp(o["im"]),
                                            vp(o["scale"]), vp(o["pad"]), st), "apg_synth_crops")
            verts = joints = None
            for g, idx in rows.items():                      # the canonical body: one forward per gender present
                whole = len(idx) == n
                at = None if whole else torch.tensor(idx, device=dev, dtype=torch.int64)       # (host -> device, no synchronisation)
                pick = (lambda t: t) if whole else (lambda t: t.index_select(0, at))
                k = len(idx)
                with torch.no_grad():
                    body = self.models[g].forward(betas=pick(r["smplshape"]), body_pose=pick(o["smplpose_rotmat"]),
                                                  global_orient=eye.expand(k, 1, 3, 3), transl=zero.expand(k, 3), pose2rot=False)
                if whole:
                    verts, joints = body.vertices, body.joints
                    break
                if verts is None:
                    verts, joints = f32(n, *body.vertices.shape[1:]), f32(n, *body.joints.shape[1:])
                elif verts.shape[1:] != body.vertices.shape[1:] or joints.shape[1:] != body.joints.shape[1:]:
                    raise RuntimeError("%s: the %s model has %d vertices and %d joints, another of the batch's models %d and %d" % (
                        NAME, g, body.vertices.shape[1], body.joints.shape[1], verts.shape[1], joints.shape[1]))
                verts.index_copy_(0, at, body.vertices)
                joints.index_copy_(0, at, body.joints)
        out = {"smplbetas": r["smplshape"], "smplpose_rotmat": o["smplpose_rotmat"], "focal_length": focal.expand(n, 2),
               "img_size": img_size.expand(n, 2), "smpl_vertices": verts.unsqueeze(1), "smpl_joints": joints.unsqueeze(1),
               "smpl_gender": list(records["smplgender"]), "cam0": o["flip"]}
        for s in (0, 1):
            for key in VIEW_KEYS:
                out["%s%d" % (key, s)] = o[key][s]
        return out
