"""airpose_amd: MI355X-native (gfx950 HIP) implementation of AirPose's two-view inference hot path.

Public mirrors of the reference interfaces:
  copenet_model.copenet / getcopenet   <- copenet/src/copenet/models/model_copenet.py
  smplx.SMPLX                          <- the smplx submodule as called by copenet_twoview.py
  geometry.rot6d_to_rotmat / perspective_projection, utils.transform_smpl
  pipeline.TwoViewInference            <- inference branch of copenet_twoview.fwd_pass_and_loss
  TrainingLoss (loss.py)               <- get_loss of copenet_twoview / copenet_singleview / hmr / muhmr
  RealDataLoss (loss_real.py)          <- get_loss of the copenet_real fine-tune trainers (2-D keypoints + VPoser prior)
  FusedAdam (optim.py)                 <- torch.optim.Adam(..., amsgrad=True) of the trainers' configure_optimizers
  clip_grad_norm_ (optim.py)           <- torch.nn.utils.clip_grad_norm_, Lightning's --gradient_clip_val; FusedAdam(max_grad_norm=,
                                          skip_nonfinite=) is the fused form, with --terminate_on_nan's guard on the device
  EvalMetrics (eval_metrics.py)        <- test_epoch_end of the four trainers: MPJPE, MPE, angle error
  Renderer (renderer.py)               <- utils/renderer.py Renderer: visualize_tb of the trainers' summaries(), without pyrender
  MeshMetrics (mesh_metrics.py)        <- no counterpart in the reference: MPJPE / PVE, absolute, root- and Procrustes-aligned
  CrossViewMetrics (cross_view_metrics.py) <- copenet_real/scripts/*_res_compile.py and utils/geometry.py lstsq_triangulation: real
                                          two-view data scored without ground truth (cross-view gaps, reprojection, triangulation)
  AirPosePlusSequence (sequence.py)    <- copenet_real_data/scripts/bundle_adj.py around its loop: network outputs in, fitted bodies out
  RealSequenceBatches (real_batches.py) <- copenet_real/dsets/copenet_real.py __getitem__ and its agreement filter: frames and raw
                                          detections in, the batch dict of TwoViewInference / RealDataLoss out, boxes kept on the device
  SyntheticBatches (synth_batches.py)  <- copenet/src/copenet/dsets/aerialpeople.py __getitem__: AerialPeople records and images in,
                                          the batch dict of the trainers, TrainingLoss, EvalMetrics and MeshMetrics out
  CropAugment (augment.py)             <- the imgaug list commented out at copenet/src/copenet/dsets/aerialpeople.py:72-76: blur, colour,
                                          gamma, noise and occluders on the crops of the two batch classes (imgaug parity UNPINNED)
  CameraRoll (roll.py)                 <- no counterpart in the reference (its unused rottrans_tfm moves the world frame, no pixel): a
                                          roll of the camera about its optical axis, the crops and every label together
The compute lives in libairpose_hip.so (include/airpose_hip.h); nothing here falls back to CPU.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # airpose_amd.TrainingLoss, resolved on first use: importing the package loads neither loss.py nor the gradient library
    if name == "TrainingLoss":
        from .loss import TrainingLoss
        return TrainingLoss
    if name == "RealDataLoss":                                            # likewise (loss_real.py)
        from .loss_real import RealDataLoss
        return RealDataLoss
    if name == "FusedAdam":                                               # likewise (optim.py)
        from .optim import FusedAdam
        return FusedAdam
    if name == "clip_grad_norm_":                                         # likewise (optim.py)
        from .optim import clip_grad_norm_
        return clip_grad_norm_
    if name == "EvalMetrics":                                             # likewise (eval_metrics.py)
        from .eval_metrics import EvalMetrics
        return EvalMetrics
    if name == "Renderer":                                                # likewise (renderer.py)
        from .renderer import Renderer
        return Renderer
    if name == "MeshMetrics":                                             # likewise (mesh_metrics.py)
        from .mesh_metrics import MeshMetrics
        return MeshMetrics
    if name == "CrossViewMetrics":                                        # likewise (cross_view_metrics.py)
        from .cross_view_metrics import CrossViewMetrics
        return CrossViewMetrics
    if name == "AirPosePlusSequence":                                     # likewise (sequence.py)
        from .sequence import AirPosePlusSequence
        return AirPosePlusSequence
    if name == "RealSequenceBatches":                                     # likewise (real_batches.py)
        from .real_batches import RealSequenceBatches
        return RealSequenceBatches
    if name == "SyntheticBatches":                                        # likewise (synth_batches.py)
        from .synth_batches import SyntheticBatches
        return SyntheticBatches
    if name == "CropAugment":                                             # likewise (augment.py)
        from .augment import CropAugment
        return CropAugment
    if name == "CameraRoll":                                              # likewise (roll.py)
        from .roll import CameraRoll
        return CameraRoll
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
