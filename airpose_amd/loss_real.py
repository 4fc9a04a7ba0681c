"""The copenet_real trainers' get_loss -- the fine-tune on real two-view footage -- as one hand-written gfx950 pass: RealDataLoss.

get_loss of copenet_real's copenet_twoview.py:100-160, copenet_twoview_sep.py:93-150, hmr.py:82-118, hmr_camswap_difffl.py:92-128 and
spin.py:86-122 has no 3-D ground truth: a confidence- and limb-weighted 2-D reprojection term, a VPoser prior on the body pose
(rotations -> tgm axis-angle -> vp_model.encode -> rsample -> mean(z^2)), cross-view pose and betas terms and an exp(-depth)^2
barrier.  apg_real_loss_fwd_bwd (csrc/loss_real_grad.hip, include/airpose_grad.h) evaluates the terms and writes the gradient
seeds in the same sweep -- the prior's gradient goes back through softplus, the encoder and the axis-angle conversion inside the
kernel -- in two launches instead of about a hundred, every sum in a fixed order.  The autograd backward is one scaling of the
saved seeds by grad_output.  There is no fallback: a missing library is an error.

The encoder is VPoser V02_05's encoder_net as published in human_body_prior/models/vposer_model.py (the commit oracle/fitting_ref.py
cites for the decoder), restated from the published source: the package is not a dependency, so parity with it is UNPINNED, like
the fitter's decoder.  Its load_model puts it in eval mode and the trainers hold it in a module global that Lightning's .train()
never reaches, so BatchNorm uses its running statistics and Dropout is the identity: the encoder is two affine maps around one
LeakyReLU, folded here once in fp64 (fold_encoder) and packed once on the device.
"""
import ctypes

import torch

from . import _native as N
from . import _native_grad as G
from . import _seeded_loss as S

KINDS = ("twoview", "twoview_sep", "hmr", "hmr_camswap", "spin")
CROSS_POSE, CROSS_BETAS = 4, 8                                # include/airpose_grad.h: APG_LOSS_CROSS_*
_TWO = {"twoview": True, "twoview_sep": True, "hmr": False, "hmr_camswap": False, "spin": False}
# (column, gain) of the barrier exp(-gain d[:, column])^2: the two-view trainers and hmr_camswap / spin on a translation's z,
# hmr on its weak-perspective scale
_DEPTH = {"twoview": (2, 1.0), "twoview_sep": (2, 1.0), "hmr": (0, 10.0), "hmr_camswap": (2, 1.0), "spin": (2, 1.0)}

# the order of the kernel's terms output, under the reference's names (loss_depth is the trainers' unnamed last summand)
TERM_NAMES = ("loss", "loss_regul_vposer", "loss_regr_pose", "loss_keypoints", "loss_regul_betas", "loss_depth")
# the order of the kernel's weights input (APG_REAL_LOSS_W_*); the last entry is not an hparam
WEIGHT_NAMES = ("keypoint2d_loss_weight", "beta_loss_weight", "vposer_loss_weight", "pose_loss_weight", "limbs2d_loss_weight", None)
LOSS_SCALE = 60.0        # `loss *= 60`

# add_model_specific_args of each trainer, restricted to what its get_loss reads.  copenet_twoview_sep has no limb weights
# (limbs2d = 1 reproduces it and is not an argument there).  hmr.py, hmr_camswap_difffl.py and spin.py READ hparams.limbs2d_loss_weight
# and hparams.vposer_loss_weight but declare neither in their argparse: the reference has no default for them, so there is none
# here and the caller must pass both (REQUIRED).
DEFAULTS = {
    "twoview": dict(keypoint2d_loss_weight=0.001, limbs2d_loss_weight=1.5, pose_loss_weight=1.0, beta_loss_weight=1.0,
                    vposer_loss_weight=1.0),
    "twoview_sep": dict(keypoint2d_loss_weight=0.001, pose_loss_weight=1.0, beta_loss_weight=1.0, vposer_loss_weight=1.0),
    "hmr": dict(keypoint2d_loss_weight=0.001, beta_loss_weight=1.0),
    "hmr_camswap": dict(keypoint2d_loss_weight=0.001, beta_loss_weight=1.0),
    "spin": dict(keypoint2d_loss_weight=0.001, beta_loss_weight=1.0),
}
REQUIRED = {"twoview": (), "twoview_sep": (), "hmr": ("limbs2d_loss_weight", "vposer_loss_weight"),
            "hmr_camswap": ("limbs2d_loss_weight", "vposer_loss_weight"), "spin": ("limbs2d_loss_weight", "vposer_loss_weight")}

# per view, in the order of the kernel's pred / grads tables (APG_REAL_LOSS_PER_VIEW entries)
PRED_NAMES = ("rotmat", "betas", "j2d", "depth")
NZ = 32                  # the latent's width
BN_EPS = 1e-5            # nn.BatchNorm1d's default, which VPoser keeps
LEAKY_SLOPE = 0.01       # nn.LeakyReLU's default, likewise

# the published state-dict keys of the encoder: name -> shape
ENCODER_KEYS = {
    "encoder_net.1.weight": (63,), "encoder_net.1.bias": (63,), "encoder_net.1.running_mean": (63,), "encoder_net.1.running_var": (63,),
    "encoder_net.2.weight": (512, 63), "encoder_net.2.bias": (512,),
    "encoder_net.4.weight": (512,), "encoder_net.4.bias": (512,), "encoder_net.4.running_mean": (512,), "encoder_net.4.running_var": (512,),
    "encoder_net.6.weight": (512, 512), "encoder_net.6.bias": (512,),
    "encoder_net.7.weight": (512, 512), "encoder_net.7.bias": (512,),
    "encoder_net.8.mu.weight": (32, 512), "encoder_net.8.mu.bias": (32,),
    "encoder_net.8.logvar.weight": (32, 512), "encoder_net.8.logvar.bias": (32,),
}


def fold_encoder(state_dict):
    """VPoser's encoder_net in eval mode as two affine maps around the LeakyReLU -> (W1 (512, 63), b1 (512), W2 (64, 512), b2 (64)),
    fp64 on the CPU.  [mu | s] = W2 leaky(W1 aa + b1) + b2, the scale of the posterior being softplus(s).

    state_dict: the published keys (ENCODER_KEYS), optionally behind a `vp_model.` prefix; other entries (the decoder, BatchNorm's
    num_batches_tracked) are ignored.  A missing key or a wrong shape is refused by name."""
    sd = {}
    for k, v in state_dict.items():
        k = k[len("vp_model."):] if k.startswith("vp_model.") else k
        if k in ENCODER_KEYS:
            sd[k] = v
    p = {}
    for k, shape in ENCODER_KEYS.items():
        if k not in sd:
            raise KeyError("RealDataLoss: the vposer state dict has no %r" % k)
        t = torch.as_tensor(sd[k]).detach().to(device="cpu", dtype=torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError("RealDataLoss: vposer[%r] must be %s, got %s" % (k, shape, tuple(t.shape)))
        p[k[len("encoder_net."):]] = t
    s1 = p["1.weight"] / torch.sqrt(p["1.running_var"] + BN_EPS)           # BatchNorm1d(63): x s1 + t1
    t1 = p["1.bias"] - p["1.running_mean"] * s1
    W1 = p["2.weight"] * s1[None, :]
    b1 = p["2.weight"] @ t1 + p["2.bias"]
    s2 = p["4.weight"] / torch.sqrt(p["4.running_var"] + BN_EPS)           # BatchNorm1d(512) after the LeakyReLU
    t2 = p["4.bias"] - p["4.running_mean"] * s2
    Wd = torch.cat([p["8.mu.weight"], p["8.logvar.weight"]], 0)            # (64, 512)
    bd = torch.cat([p["8.mu.bias"], p["8.logvar.bias"]], 0)
    M = Wd @ p["7.weight"] @ p["6.weight"]
    W2 = M * s2[None, :]
    b2 = Wd @ (p["7.weight"] @ (p["6.weight"] @ t2 + p["6.bias"]) + p["7.bias"]) + bd
    return W1, b1, W2, b2


def _pred(t, dev, shape, name):
    """fp32 (nothing is cast), contiguous, on dev, of `shape` (None = any extent); anything else is refused by name"""
    return S.check_tensor("RealDataLoss", t, dev, shape, name, cast=False)


class RealDataLoss(S.SeededLossModule):
    """get_loss of one of the five copenet_real trainers on libairpose_grad.so.  No parameters (the encoder is a frozen buffer).

    kind: "twoview", "twoview_sep", "hmr", "hmr_camswap" or "spin".
    vposer: a state dict with VPoser V02_05's published encoder keys (ENCODER_KEYS; an optional `vp_model.` prefix is stripped), folded
    in fp64 and packed once, on the first forward's device.
    **weights: the reference's hparams names, defaulting to that trainer's own argparse defaults (DEFAULTS[kind]); hmr, hmr_camswap
    and spin need limbs2d_loss_weight and vposer_loss_weight given, as their trainers declare no default for either.
    forward takes what that trainer's get_loss takes, in its order (pred_output_cam is accepted and, as there, not read):
      twoview, twoview_sep   (input_batch, pred_smpltrans0, pred_smpltrans1, pred_rotmat0, pred_rotmat1, pred_betas0, pred_betas1,
                              pred_output_cam0, pred_output_cam1, pred_joints_2d_cam0, pred_joints_2d_cam1)
      hmr, spin              (input_batch, pred_camera, pred_rotmat, pred_betas, pred_output_cam, pred_joints_2d_cam)
      hmr_camswap            (input_batch, pred_cam_t, pred_rotmat, pred_betas, pred_output_cam, pred_joints_2d_cam)
    and the keywords eps (per view a (B, 32) tensor: the standard-normal draw of rsample(); a list of two for the two-view kinds)
    or generator.  With neither, eps is torch.randn((B, 32)) on the device, view 0 then view 1: the order of the reference's two
    rsample() calls.
    input_batch: 'smpl_joints_2d0' / 'smpl_joints_2d1' (two views) or 'smpl_joints_2d_crop0', each (B, 1, Jg, 3) = x, y, confidence.
    -> (loss, terms): loss is 0-d and attached to the graph; terms is the detached (6,) device tensor in TERM_NAMES order;
    self.losses(terms) makes the reference's `losses` dict with one host copy.
    """

    _owner, _kinds, _defaults, _required, _term_names = "RealDataLoss", KINDS, DEFAULTS, REQUIRED, TERM_NAMES
    _skip = {k: ("loss_depth",) if _TWO[k] else ("loss_depth", "loss_regr_pose") for k in KINDS}

    def __init__(self, kind, vposer, **weights):
        super().__init__(kind, weights, "RealDataLoss(%s)" % kind)
        W1, b1, W2, b2 = fold_encoder(vposer)                    # fp64, once
        self._folded = [t.float().contiguous() for t in (W1, b1, W2, b2)]
        self._packed = None

    def weight_vector(self):
        """the 6 floats of apg_real_loss_fwd_bwd's weights"""
        d = dict(pose_loss_weight=0.0, limbs2d_loss_weight=1.0)  # what a kind without the term / the limb weights amounts to
        d.update(self.weights)
        return [LOSS_SCALE if n is None else d[n] for n in WEIGHT_NAMES]

    def encoder(self, dev):
        """the packed encoder table on dev (packed on first use, again if the device changes)"""
        if self._packed is None or self._packed.device != dev:
            L = G.lib()
            nbytes = L.apg_real_loss_encoder_bytes()
            packed = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
            src = [t.to(dev) for t in self._folded]
            with torch.cuda.device(dev):
                G.check(L.apg_real_loss_pack_encoder(*[N.dptr(t) for t in src], N.dptr(packed), nbytes, N.stream_ptr(dev)),
                        "apg_real_loss_pack_encoder")
                torch.cuda.current_stream(dev).synchronize()     # src may be freed once this returns
            self._packed = packed
        return self._packed

    def _views(self, args):
        """-> per view a dict of PRED_NAMES, from the kind's positional arguments"""
        k = self.kind
        want = 10 if _TWO[k] else 5
        if len(args) != want:
            raise RuntimeError("RealDataLoss(%s).forward takes input_batch and %d predictions, got %d" % (k, want, len(args)))
        if _TWO[k]:
            t0, t1, r0, r1, b0, b1, _o0, _o1, p0, p1 = args
            return [dict(depth=t0, rotmat=r0, betas=b0, j2d=p0), dict(depth=t1, rotmat=r1, betas=b1, j2d=p1)]
        c, r, b, _o, p = args
        return [dict(depth=c, rotmat=r, betas=b, j2d=p)]

    def forward(self, input_batch, *args, eps=None, generator=None):
        views = self._views(args)
        nviews = len(views)
        first = views[0]["rotmat"]
        dev = self._device_of(first)
        B = first.shape[0]
        j2d0 = views[0]["j2d"]
        if not torch.is_tensor(j2d0) or j2d0.dim() != 3:
            raise RuntimeError("RealDataLoss: pred_joints_2d_cam must be (B, J, 2)")
        J = j2d0.shape[1]
        if B < 1 or J < 22:
            raise RuntimeError("RealDataLoss: needs B >= 1 and J >= 22, got B = %d, J = %d" % (B, J))
        shapes = dict(rotmat=(B, 22, 3, 3), betas=(B, 10), j2d=(B, J, 2), depth=(B, 3))
        preds = [_pred(d[n], dev, shapes[n], "%s of view %d" % (n, v)) for v, d in enumerate(views) for n in PRED_NAMES]

        if eps is not None and generator is not None:
            raise RuntimeError("RealDataLoss: give eps or generator, not both")
        if eps is None:
            eps = [torch.randn((B, NZ), device=dev, dtype=torch.float32, generator=generator) for _ in range(nviews)]
        elif torch.is_tensor(eps):
            eps = [eps]
        if len(eps) != nviews:
            raise RuntimeError("RealDataLoss(%s): eps must hold %d tensor(s), got %d" % (self.kind, nviews, len(eps)))
        gts, Jg = [], None
        for v in range(nviews):
            key = "smpl_joints_2d%d" % v if _TWO[self.kind] else "smpl_joints_2d_crop0"
            if key not in input_batch:
                raise RuntimeError("RealDataLoss(%s): input_batch has no %r" % (self.kind, key))
            t = input_batch[key]
            if not torch.is_tensor(t) or t.dim() != 4:
                raise RuntimeError("RealDataLoss: input_batch[%r] must be a (B, 1, Jg, 3) tensor" % key)
            t = t[:, 0]
            Jg = t.shape[1] if Jg is None else Jg
            gts.append(_pred(t.detach(), dev, (B, Jg, 3), "input_batch[%r][:, 0]" % key))
            gts.append(_pred(eps[v].detach() if torch.is_tensor(eps[v]) else eps[v], dev, (B, NZ), "eps of view %d" % v))
        if Jg < 22:
            raise RuntimeError("RealDataLoss: the 2-D ground truth must have at least 22 joints, got %d" % Jg)
        col, gain = _DEPTH[self.kind]
        cross, weights, encoder = (CROSS_POSE | CROSS_BETAS) if _TWO[self.kind] else 0, self.weight_vector(), self.encoder(dev)

        def launch(terms, grads):
            L = G.lib()
            nbytes = L.apg_real_loss_workspace_bytes(B)
            if nbytes < 0:
                raise RuntimeError("RealDataLoss: no workspace for B = %d" % B)
            ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
            w = (ctypes.c_float * len(weights))(*weights)
            G.check(L.apg_real_loss_fwd_bwd(nviews, cross, B, J, Jg, col, gain, w, N.dptr(encoder), G.ptrs(preds), G.ptrs(gts),
                                            N.dptr(terms), G.ptrs(grads) if grads else None,      # all NULL: forward only
                                            N.dptr(ws), nbytes, N.stream_ptr(dev)), "apg_real_loss_fwd_bwd")

        return S.SeededLoss.apply(dev, len(TERM_NAMES), torch.is_grad_enabled(), launch, *preds)
