"""The reference trainers' get_loss as one hand-written gfx950 pass: TrainingLoss.

get_loss of copenet_twoview.py:83-161, copenet_singleview.py:76-117, hmr.py:75-116 and muhmr.py:76-131 is a weighted sum of mean
squared differences, so the gradient of the total with respect to every prediction is known the moment a difference is formed.
apg_loss_fwd_bwd (csrc/loss_grad.hip, include/airpose_grad.h) evaluates the terms and writes those gradient seeds in the same sweep:
two launches (and one copy of the loss into storage of its own) instead of about sixty, reductions in a fixed order
(bit-reproducible, which torch's mean() does not promise), and the autograd backward is a scaling of the saved seeds by grad_output.  There is no fallback: a missing library is an error.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from . import _native_grad as G

KINDS = ("twoview", "singleview", "hmr", "muhmr")
# include/airpose_grad.h: APG_LOSS_CROSS_*
CROSS_JOINTS, CROSS_VERTS, CROSS_POSE, CROSS_BETAS = 1, 2, 4, 8
_CROSS = {"twoview": CROSS_JOINTS | CROSS_VERTS | CROSS_POSE | CROSS_BETAS, "singleview": 0, "hmr": 0, "muhmr": CROSS_POSE}
_HAS_TRANS = {"twoview": True, "singleview": True, "hmr": False, "muhmr": False}

# the order of the kernel's terms output, under the reference's names (loss_cam is hmr's / muhmr's unnamed last summand)
TERM_NAMES = ("loss", "loss_regr_trans", "loss_keypoints", "loss_keypoints_3d", "loss_regr_shape", "loss_rootrot", "loss_regr_pose",
              "loss_regul_betas", "loss_cam")
# the order of the kernel's weights input (APG_LOSS_W_*); the last two entries are not hparams
WEIGHT_NAMES = ("trans_loss_weight", "keypoint2d_loss_weight", "keypoint3d_loss_weight", "shape_loss_weight", "rootrot_loss_weight",
                "pose_loss_weight", "beta_loss_weight", None, "limbs3d_loss_weight", "limbstheta_loss_weight", None)
CAM_COEFFICIENT = 1.0    # the reference adds mean(exp(-10 s)^2) unweighted (its cams_loss_weight hparam is never read)
LOSS_SCALE = 60.0        # `loss *= 60`

# add_model_specific_args of each trainer
DEFAULTS = {
    "twoview": dict(shape_loss_weight=50.0, keypoint2d_loss_weight=0.002, keypoint3d_loss_weight=1.0, limbs3d_loss_weight=3.0,
                    limbstheta_loss_weight=1.0, trans_loss_weight=10.0, rootrot_loss_weight=1.0, pose_loss_weight=50.0,
                    beta_loss_weight=1.0),
    "singleview": dict(shape_loss_weight=1.0, keypoint2d_loss_weight=0.001, keypoint3d_loss_weight=1.0, limbs3d_loss_weight=3.0,
                       limbstheta_loss_weight=3.0, trans_loss_weight=1.0, rootrot_loss_weight=1.0, pose_loss_weight=1.0,
                       beta_loss_weight=1.0),
    "hmr": dict(shape_loss_weight=1.0, keypoint2d_loss_weight=0.001, keypoint3d_loss_weight=1.0, limbs3d_loss_weight=3.0,
                limbstheta_loss_weight=3.0, trans_loss_weight=1.0, rootrot_loss_weight=1.0, pose_loss_weight=1.0,
                beta_loss_weight=1.0),
    "muhmr": dict(shape_loss_weight=100.0, keypoint2d_loss_weight=0.05, keypoint3d_loss_weight=1.0, limbs3d_loss_weight=3.0,
                  limbstheta_loss_weight=1.0, trans_loss_weight=1.0, rootrot_loss_weight=1.0, pose_loss_weight=100.0,
                  beta_loss_weight=1.0),
}

# per view, in the order of the kernel's pred / grads tables (APG_LOSS_PER_VIEW entries)
PRED_NAMES = ("trans", "rotmat", "betas", "joints", "verts", "j2d", "cam")


def _pred(t, dev, shape, name):
    """fp32, contiguous, on dev, of `shape` (None = any extent); anything else is refused by name"""
    if not torch.is_tensor(t):
        raise RuntimeError("TrainingLoss: %s must be a tensor, got %s" % (name, type(t).__name__))
    if t.device != dev:
        raise RuntimeError("TrainingLoss: %s lives on %s, the predictions on %s" % (name, t.device, dev))
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise RuntimeError("TrainingLoss: %s must be %s, got %s" % (name, tuple("*" if s is None else s for s in shape), tuple(t.shape)))
    if t.dtype != torch.float32:
        if not t.is_floating_point():
            raise RuntimeError("TrainingLoss: %s must be a floating-point tensor, got %s" % (name, t.dtype))
        t = t.float()
    return t.contiguous()


def _joints_vertices(out, name):
    """the reference passes the SMPL-X output object; a (joints, vertices) pair is taken as well"""
    if hasattr(out, "joints") and hasattr(out, "vertices"):
        return out.joints, out.vertices
    if isinstance(out, (tuple, list)) and len(out) == 2:
        return out[0], out[1]
    raise RuntimeError("TrainingLoss: %s must have .joints and .vertices, or be a (joints, vertices) pair" % name)


class _Loss(torch.autograd.Function):
    """(cfg, gt table, 7 predictions per view) -> (the 0-d loss in storage of its own, the (9,) terms: not differentiable)"""

    @staticmethod
    def forward(ctx, cfg, gts, *preds):
        nviews, cross, B, J, Jg, V, weights, dev = cfg["nviews"], cfg["cross"], cfg["B"], cfg["J"], cfg["Jg"], cfg["V"], cfg["weights"], cfg["dev"]
        # (needs_input_grad follows requires_grad alone; under no_grad nothing will call backward, so nothing is asked for)
        need = ctx.needs_input_grad[2:] if cfg["grad"] else (False,) * len(preds)
        # every seed is a slice of ONE flat buffer (each slice starts on a 16-byte boundary), so that backward scales them in one launch
        offs, total = [], 0
        for k, p in enumerate(preds):
            offs.append(total if (p is not None and need[k]) else None)
            if offs[-1] is not None:
                total += (p.numel() + 3) // 4 * 4
        flat = torch.empty(total, device=dev, dtype=torch.float32) if total else None
        grads = [None if o is None else flat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, preds)]
        terms = torch.empty(len(TERM_NAMES), device=dev, dtype=torch.float32)
        L = G.lib()
        nbytes = L.apg_loss_workspace_bytes(B, V)
        if nbytes < 0:
            raise RuntimeError("TrainingLoss: no workspace for B = %d, V = %d" % (B, V))
        ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
        w = (ctypes.c_float * len(weights))(*weights)
        with torch.cuda.device(dev):
            G.check(L.apg_loss_fwd_bwd(nviews, cross, B, J, Jg, V, w, G.ptrs(preds), G.ptrs(gts), N.dptr(terms),
                                       G.ptrs(grads) if total else None,      # all NULL: forward only
                                       N.dptr(ws), nbytes, N.stream_ptr(dev)), "apg_loss_fwd_bwd")
        ctx.flat, ctx.offs, ctx.shapes = flat, offs, [None if p is None else p.shape for p in preds]     # this call's own buffer
        loss = terms[0].clone()                                  # its own element: in-place work on terms cannot reach the loss
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms):
        if ctx.flat is None:
            return (None, None) + (None,) * len(ctx.offs)
        scaled = ctx.flat * g                                    # the padding between slices is never read
        return (None, None) + tuple(None if o is None else scaled[o:o + s.numel()].view(s) for o, s in zip(ctx.offs, ctx.shapes))


class TrainingLoss(torch.nn.Module):
    """get_loss of one of the four reference trainers on libairpose_grad.so.  No parameters.

    kind: "twoview", "singleview", "hmr" or "muhmr"; **weights: the reference's hparams names (WEIGHT_NAMES), defaulting to that
    trainer's own argparse defaults (DEFAULTS[kind]).  forward takes what that trainer's get_loss takes, in its order:
      twoview     (input_batch, pred_smpltrans0, pred_smpltrans1, pred_rotmat0, pred_rotmat1, pred_betas0, pred_betas1,
                   pred_output_cam0, pred_output_cam1, pred_joints_2d_cam0, pred_joints_2d_cam1)
      singleview  (input_batch, pred_smpltrans, pred_rotmat, pred_betas, pred_output_cam, pred_joints_2d_cam)
      hmr         (input_batch, pred_camera, pred_rotmat, pred_betas, pred_output_cam, pred_joints_2d_cam)
      muhmr       (input_batch, pred_rotmat0, pred_betas0, pred_output_cam0, pred_joints_2d_cam0, pred_camera0,
                   pred_rotmat1, pred_betas1, pred_output_cam1, pred_joints_2d_cam1, pred_camera1)
    pred_output_cam: an object with .joints (B, J >= 22, 3) and .vertices (B, V, 3), or the (joints, vertices) pair.
    input_batch: the reference's keys, the ground-truth meshes, joints and 2-D joints with their singleton dimension 1.
    -> (loss, terms): loss is 0-d and attached to the graph; terms is the detached (9,) device tensor in TERM_NAMES order
    (absent terms 0); self.losses(terms) makes the reference's `losses` dict with one host copy.
    """

    def __init__(self, kind, **weights):
        super().__init__()
        if kind not in KINDS:
            raise ValueError("TrainingLoss: kind must be one of %s, got %r" % (", ".join(KINDS), kind))
        unknown = sorted(set(weights) - set(DEFAULTS[kind]))
        if unknown:
            raise ValueError("TrainingLoss: unknown weight(s) %s; the names are %s" % (unknown, sorted(DEFAULTS[kind])))
        self.kind = kind
        self.weights = dict(DEFAULTS[kind])
        self.weights.update({k: float(v) for k, v in weights.items()})

    def extra_repr(self):
        return "kind=%r, %s" % (self.kind, ", ".join("%s=%g" % kv for kv in sorted(self.weights.items())))

    def weight_vector(self):
        """the 11 floats of apg_loss_fwd_bwd's weights"""
        w = [CAM_COEFFICIENT if k == 7 else LOSS_SCALE if k == 10 else self.weights[n] for k, n in enumerate(WEIGHT_NAMES)]
        return w

    def losses(self, terms):
        """the reference's `losses` dict of this kind from forward's terms: ONE device-to-host copy (the reference does eight)"""
        host = terms.detach().cpu().tolist()
        skip = ("loss_cam",) if _HAS_TRANS[self.kind] else ("loss_cam", "loss_regr_trans")
        return {n: v for n, v in zip(TERM_NAMES, host) if n not in skip}

    def _views(self, args):
        """-> per view a dict of PRED_NAMES (absent entries None), from the kind's positional arguments"""
        k = self.kind
        want = {"twoview": 10, "singleview": 5, "hmr": 5, "muhmr": 10}[k]
        if len(args) != want:
            raise RuntimeError("TrainingLoss(%s).forward takes input_batch and %d predictions, got %d" % (k, want, len(args)))
        if k == "twoview":
            t0, t1, r0, r1, b0, b1, o0, o1, p0, p1 = args
            return [dict(trans=t0, rotmat=r0, betas=b0, out=o0, j2d=p0, cam=None), dict(trans=t1, rotmat=r1, betas=b1, out=o1, j2d=p1, cam=None)]
        if k == "singleview":
            t, r, b, o, p = args
            return [dict(trans=t, rotmat=r, betas=b, out=o, j2d=p, cam=None)]
        if k == "hmr":
            c, r, b, o, p = args
            return [dict(trans=None, rotmat=r, betas=b, out=o, j2d=p, cam=c)]
        r0, b0, o0, p0, c0, r1, b1, o1, p1, c1 = args
        return [dict(trans=None, rotmat=r0, betas=b0, out=o0, j2d=p0, cam=c0), dict(trans=None, rotmat=r1, betas=b1, out=o1, j2d=p1, cam=c1)]

    def forward(self, input_batch, *args):
        views = self._views(args)
        nviews = len(views)
        crop = "" if _HAS_TRANS[self.kind] else "_crop"              # hmr / muhmr compare in the crop's pixels
        first = views[0]["rotmat"]
        if not torch.is_tensor(first) or not first.is_cuda:
            raise RuntimeError("TrainingLoss: predictions must be CUDA (ROCm) tensors; there is no CPU path")
        dev = first.device
        B = first.shape[0]
        preds = []
        J = V = None
        for v, d in enumerate(views):
            joints, verts = _joints_vertices(d["out"], "pred_output_cam%d" % v)
            if J is None:
                if joints.dim() != 3 or verts.dim() != 3:
                    raise RuntimeError("TrainingLoss: joints and vertices must be (B, J, 3) and (B, V, 3)")
                J, V = joints.shape[1], verts.shape[1]
            tensors = dict(trans=(d["trans"], (B, 3)), rotmat=(d["rotmat"], (B, 22, 3, 3)), betas=(d["betas"], (B, 10)),
                           joints=(joints, (B, J, 3)), verts=(verts, (B, V, 3)), j2d=(d["j2d"], (B, J, 2)), cam=(d["cam"], (B, 3)))
            for n in PRED_NAMES:
                t, shape = tensors[n]
                preds.append(None if t is None else _pred(t, dev, shape, "%s of view %d" % (n, v)))
        if B < 1 or J < 22 or V < 1:
            raise RuntimeError("TrainingLoss: needs B >= 1, J >= 22 and V >= 1, got B = %d, J = %d, V = %d" % (B, J, V))

        def gt(key, shape, squeeze=False):
            if key not in input_batch:
                raise RuntimeError("TrainingLoss(%s): input_batch has no %r" % (self.kind, key))
            t = input_batch[key]
            if squeeze and torch.is_tensor(t):
                t = t.squeeze(1)
            return _pred(t.detach() if torch.is_tensor(t) else t, dev, shape, "input_batch[%r]" % key)

        gt_joints = gt("smpl_joints", (B, None, 3), True)
        Jg = gt_joints.shape[1]
        gts = [gt("smplpose_rotmat", (B, 21, 3, 3)), gt_joints, gt("smpl_vertices", (B, V, 3), True)]
        for v in range(nviews):
            gts += [gt("smplorient_rel%d" % v, (B, 1, 3, 3)), gt("smpl_joints_2d%s%d" % (crop, v), (B, Jg, 2), True),
                    gt("smpltrans_rel%d" % v, (B, 3)) if _HAS_TRANS[self.kind] else None]
        if Jg < 22:
            raise RuntimeError("TrainingLoss: input_batch['smpl_joints'] must have at least 22 joints, got %d" % Jg)
        cfg = dict(nviews=nviews, cross=_CROSS[self.kind], B=B, J=J, Jg=Jg, V=V, weights=self.weight_vector(), dev=dev,
                   grad=torch.is_grad_enabled())
        return _Loss.apply(cfg, gts, *preds)
