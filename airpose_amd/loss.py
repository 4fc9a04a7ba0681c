"""The reference trainers' get_loss as one hand-written gfx950 pass: TrainingLoss.

get_loss of copenet_twoview.py:83-161, copenet_singleview.py:76-117, hmr.py:75-116 and muhmr.py:76-131 is a weighted sum of mean
squared differences, so the gradient of the total with respect to every prediction is known the moment a difference is formed.
apg_loss_fwd_bwd (csrc/loss_grad.hip, include/airpose_grad.h) evaluates the terms and writes those gradient seeds in the same sweep:
two launches (and one copy of the loss into storage of its own) instead of about sixty, reductions in a fixed order
(bit-reproducible, which torch's mean() does not promise), and the autograd backward is a scaling of the saved seeds by grad_output.  There is no fallback: a missing library is an error.
"""
import ctypes

import torch

from . import _native as N
from . import _native_grad as G
from . import _seeded_loss as S

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
    """fp32 (another floating-point type is cast), contiguous, on dev, of `shape`; anything else is refused by name"""
    return S.check_tensor("TrainingLoss", t, dev, shape, name, cast=True)


def _joints_vertices(out, name):
    """the reference passes the SMPL-X output object; a (joints, vertices) pair is taken as well"""
    if hasattr(out, "joints") and hasattr(out, "vertices"):
        return out.joints, out.vertices
    if isinstance(out, (tuple, list)) and len(out) == 2:
        return out[0], out[1]
    raise RuntimeError("TrainingLoss: %s must have .joints and .vertices, or be a (joints, vertices) pair" % name)


class TrainingLoss(S.SeededLossModule):
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

    _owner, _kinds, _defaults, _term_names = "TrainingLoss", KINDS, DEFAULTS, TERM_NAMES
    # what losses() leaves out (its one device-to-host copy stands for the reference's eight)
    _skip = {k: ("loss_cam",) if _HAS_TRANS[k] else ("loss_cam", "loss_regr_trans") for k in KINDS}

    def __init__(self, kind, **weights):
        super().__init__(kind, weights, "TrainingLoss")

    def weight_vector(self):
        """the 11 floats of apg_loss_fwd_bwd's weights"""
        w = [CAM_COEFFICIENT if k == 7 else LOSS_SCALE if k == 10 else self.weights[n] for k, n in enumerate(WEIGHT_NAMES)]
        return w

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
        dev = self._device_of(first)
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
        cross, weights = _CROSS[self.kind], self.weight_vector()

        def launch(terms, grads):
            L = G.lib()
            nbytes = L.apg_loss_workspace_bytes(B, V)
            if nbytes < 0:
                raise RuntimeError("TrainingLoss: no workspace for B = %d, V = %d" % (B, V))
            ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
            w = (ctypes.c_float * len(weights))(*weights)
            G.check(L.apg_loss_fwd_bwd(nviews, cross, B, J, Jg, V, w, G.ptrs(preds), G.ptrs(gts), N.dptr(terms),
                                       G.ptrs(grads) if grads else None,      # all NULL: forward only
                                       N.dptr(ws), nbytes, N.stream_ptr(dev)), "apg_loss_fwd_bwd")

        return S.SeededLoss.apply(dev, len(TERM_NAMES), torch.is_grad_enabled(), launch, *preds)
