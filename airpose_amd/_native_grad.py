"""ctypes binding of libairpose_grad.so (the C ABI in include/airpose_grad.h): the gradient entry points.

Same pattern as _native.py: PyTorch is used for device memory and streams only, the library is loaded lazily and checked
against the header's ABI number, and there is NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import threading

import torch  # noqa: F401  (must be imported first so that libamdhip64 is the one torch loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AIRPOSE_GRAD_LIB", os.path.join(_HERE, "libairpose_grad.so"))

_c = ctypes
_vp, _i, _f, _i64, _u64 = _c.c_void_p, _c.c_int, _c.c_float, _c.c_int64, _c.c_uint64
_vpp, _ip = _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_int)

# name -> (restype, argtypes); mirrors include/airpose_grad.h one to one
SIGNATURES = {
    "apg_version": (_c.c_char_p, []),
    "apg_abi_version": (_i, []),
    "apg_last_error": (_c.c_char_p, []),
    "apg_dropout_mask": (_i, [_u64, _i, _i, _i, _f, _vp, _vp]),
    "apg_head_fwd": (_i, [_i, _vp, _vp, _vpp, _ip] + [_vp] * 8 + [_u64, _f, _f] + [_vp] * 3 + [_vpp, _vpp, _vp]),
    "apg_head_bwd_workspace_bytes": (_i64, [_i, _i]),
    "apg_head_bwd": (_i, [_i] + [_vp] * 7 + [_u64, _f, _f, _vpp, _vpp, _vpp, _vp, _i64, _vp]),
    # the generic view-local head (head_local_grad.hip)
    "apg_head_local_fwd": (_i, [_i, _vp, _i, _vpp, _ip, _ip] + [_vp] * 4 + [_i, _vpp, _vpp, _ip, _ip, _u64, _f, _f] + [_vp] * 4 +
                           [_vpp, _vp]),
    "apg_head_local_bwd_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "apg_head_local_bwd": (_i, [_i, _i, _ip, _ip, _i, _ip, _ip] + [_vp] * 6 + [_u64, _f, _f, _vpp, _vpp, _vp, _vpp, _vp, _i64, _vp]),
    "apg_rot6d_to_rotmat_bwd": (_i, [_vp, _i, _vp, _vp, _vp]),
    "apg_perspective_projection_bwd": (_i, [_vp, _i, _i, _vp, _vp, _f, _f] + [_vp] * 5 + [_vp]),
    "apg_transform_points_bwd": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "apg_conv_fwd": (_i, [_vp] + [_i] * 4 + [_vp] + [_i] * 5 + [_vp, _vp]),
    "apg_conv_bwd_workspace_bytes": (_i64, [_i] * 9),
    "apg_conv_bwd": (_i, [_vp] + [_i] * 4 + [_vp] + [_i] * 5 + [_vp] * 4 + [_i64, _vp]),
    "apg_bn_workspace_bytes": (_i64, [_i, _i]),
    "apg_bn_fwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "apg_bn_bwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "apg_maxpool_fwd": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "apg_maxpool_bwd": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "apg_avgpool_fwd": (_i, [_vp, _i, _i, _vp, _vp]),
    "apg_avgpool_bwd": (_i, [_vp, _i, _i, _vp, _vp]),
    "apg_trunk_workspace_bytes": (_i64, [_i, _i]),
    "apg_trunk_fwd": (_i, [_i, _vp, _vpp, _i, _f, _f, _vp, _i, _vp, _i64, _vp]),
    "apg_trunk_bwd": (_i, [_i, _vpp, _i, _vp, _vpp, _vp, _vp, _i64, _vp]),
    # the bf16 training mode (trunk_grad_bf16.hip)
    "apg_trunk_precisions": (_i, []),
    "apg_pack_weights_bf16": (_i, [_vp] + [_i] * 5 + [_vp, _vp, _vp]),
    "apg_conv_fwd_bf16": (_i, [_vp] + [_i] * 4 + [_vp] + [_i] * 5 + [_vp, _vp]),
    "apg_conv_bwd_bf16_workspace_bytes": (_i64, [_i] * 9),
    "apg_conv_bwd_bf16": (_i, [_vp] + [_i] * 4 + [_vp] + [_i] * 5 + [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i64, _vp]),
    "apg_bn_bf16_workspace_bytes": (_i64, [_i, _i]),
    "apg_bn_fwd_bf16": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "apg_bn_bwd_bf16": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "apg_maxpool_fwd_bf16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "apg_maxpool_bwd_bf16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "apg_avgpool_fwd_bf16": (_i, [_vp, _i, _i, _vp, _vp]),
    "apg_avgpool_bwd_bf16": (_i, [_vp, _i, _i, _vp, _vp]),
    "apg_trunk_workspace_bytes_p": (_i64, [_i, _i, _i]),
    "apg_trunk_fwd_p": (_i, [_i, _i, _vp, _vpp, _i, _f, _f, _vp, _i, _vp, _i64, _vp]),
    "apg_trunk_bwd_p": (_i, [_i, _i, _vpp, _i, _vp, _vpp, _vp, _vp, _i64, _vp]),
    # the training loss and its gradient seeds (loss_grad.hip)
    "apg_loss_workspace_bytes": (_i64, [_i, _i]),
    "apg_loss_fwd_bwd": (_i, [_i] * 6 + [_c.POINTER(_f), _vpp, _vpp, _vp, _vpp, _vp, _i64, _vp]),
    # the real-data fine-tuning loss with the VPoser prior (loss_real_grad.hip)
    "apg_real_loss_workspace_bytes": (_i64, [_i]),
    "apg_real_loss_encoder_bytes": (_i64, []),
    "apg_real_loss_pack_encoder": (_i, [_vp] * 5 + [_i64, _vp]),
    "apg_real_loss_fwd_bwd": (_i, [_i] * 6 + [_f, _c.POINTER(_f), _vp, _vpp, _vpp, _vp, _vpp, _vp, _i64, _vp]),
    # the optimizer step (optim.hip)
    "apg_adam_step": (_i, [_i] + [_vpp] * 5 + [_c.POINTER(_i64)] * 2 + [_c.c_double] * 5 + [_vp]),
    # gradient clipping and the non-finite guard (guard/grad_guard.hip)
    "apg_grad_norm_workspace_bytes": (_i64, [_i, _c.POINTER(_i64)]),
    "apg_grad_norm": (_i, [_i, _vpp, _c.POINTER(_i64), _c.c_double, _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    "apg_grad_scale": (_i, [_i, _vpp, _c.POINTER(_i64), _vp, _vp]),
    "apg_adam_step_guarded": (_i, [_i] + [_vpp] * 5 + [_c.POINTER(_i64)] * 2 + [_c.c_double] * 5 + [_vp, _vp]),
    # the evaluation metrics (eval_metrics.hip)
    "apg_eval_workspace_bytes": (_i64, [_i, _i]),
    "apg_eval_acc_doubles": (_i64, []),
    "apg_eval_update": (_i, [_i, _i, _i, _vp, _ip, _vpp] + [_vp] * 6 + [_i64, _vp]),
    # the mesh overlay renderer (render.hip)
    "apg_render_workspace_bytes": (_i64, [_i] * 5),
    "apg_render_overlay": (_i, [_i] * 5 + [_vp] * 4 + [_i, _vp, _vp] + [_f] * 6 + [_vp] + [_f] * 5 + [_vp] * 4 + [_i64, _vp]),
    # the mesh metrics (eval_align.hip)
    "apg_align_workspace_bytes": (_i64, [_i, _i, _i]),
    "apg_align_acc_doubles": (_i64, []),
    "apg_align_update": (_i, [_i, _i, _i] + [_i64] * 4 + [_vpp] + [_vp] * 4 + [_i64, _vp]),
    # the cross-view metrics (xview_metrics.hip); strides is a HOST array
    "apg_xview_workspace_bytes": (_i64, [_i, _i, _i]),
    "apg_xview_acc_doubles": (_i64, []),
    "apg_xview_update": (_i, [_i] * 5 + [_c.POINTER(_i64), _vpp, _c.c_double] + [_vp] * 4 + [_i64, _vp]),
    "apg_xview_triangulate": (_i, [_i, _i] + [_vp] * 6 + [_c.c_double, _vp, _vp]),
    # AirPose+ on a whole sequence (seq_fit.hip)
    "apg_seq_init": (_i, [_i] + [_vp] * 9 + [_f, _f] + [_vp] * 5 + [_vp]),
    "apg_seq_export": (_i, [_i] + [_vp] * 13 + [_vp]),
    # real-data batches (seq_batch.hip); principal and size are HOST arrays
    "apg_real_batch": (_i, [_i, _i, _i, _vp, _c.POINTER(_f), _ip, _f, _i] + [_vp] * 6 + [_vp]),
    # synthetic-data batches (synth_batch.hip): 9 inputs and 14 outputs, all device pointers
    "apg_synth_batch": (_i, [_i] * 11 + [_f, _f, _u64, _i] + [_vp] * 9 + [_vp] * 14 + [_vp]),
    "apg_synth_crops": (_i, [_i] * 4 + [_vp] * 6 + [_vp]),
    # crop augmentation (augment.hip); cfg is a HOST array of AUG_CFG floats
    "apg_augment_draw": (_i, [_i, _u64, _i, _vp, _vp, _i, _c.POINTER(_f)] + [_vp] * 7 + [_vp]),
    "apg_augment_crops": (_i, [_i, _u64, _i, _vp, _vp, _i] + [_vp] * 10 + [_vp]),
    # camera roll (roll.hip): 11 inputs and 10 outputs of apg_roll_labels, all device pointers (a label may be NULL)
    "apg_roll_draw": (_i, [_i, _u64, _i, _vp, _vp, _i, _f, _f, _vp, _vp]),
    "apg_roll_labels": (_i, [_i] * 9 + [_vp, _i] + [_vp] * 11 + [_vp] * 10 + [_vp]),
    "apg_roll_crops": (_i, [_i] * 6 + [_vp, _vp, _vp, _i] + [_vp] * 4 + [_vp]),
}
# include/airpose_grad.h: APG_AUG_*; the last four are the bits of status
AUG_TILE, AUG_THREADS, AUG_MAX_RADIUS, AUG_MAX_RECTS, AUG_CFG = 32, 256, 6, 4, 18
AUG_BLUR_CLAMPED, AUG_NONFINITE, AUG_RECT_CLIPPED, AUG_BAD_BOX = 1, 2, 4, 8
GUARD_BYTES, GRAD_NORM_BATCH = 16, 192    # include/airpose_grad.h: APG_GUARD_BYTES, APG_GRAD_NORM_BATCH
ROLL_THREADS = 256      # include/airpose_grad.h: APG_ROLL_THREADS
ROLL_CENTRE_OUT, ROLL_OFF_CANVAS = 1, 2                      # include/airpose_grad.h: APG_ROLL_*, the bits of status
SYNTH_ORIGINS = {"region": 0, "frame": 1}                    # include/airpose_grad.h: APG_SYNTH_ORIGIN_*
SYNTH_CLAMPED, SYNTH_WIDENED, SYNTH_OUTSIDE = 1, 2, 4        # include/airpose_grad.h: APG_SYNTH_*, the bits of status
SYNTH_THREADS = 128      # include/airpose_grad.h: APG_SYNTH_THREADS
SEQ_ROWS = 4             # include/airpose_grad.h: APG_SEQ_ROWS
BATCH_WAVES = 4          # include/airpose_grad.h: APG_BATCH_WAVES
BATCH_FALLBACK, BATCH_CLAMPED, BATCH_WIDENED = 1, 2, 4       # include/airpose_grad.h: APG_BATCH_*, the bits of status
PRECISIONS = {"fp32": 0, "bf16": 1}          # include/airpose_grad.h: APG_PREC_*

ABI_VERSION = 2          # include/airpose_grad.h: APG_ABI_VERSION
_lib = None
_lib_lock = threading.Lock()


def lib():
    """Load (once) and return the gradient library; raises if it has not been built."""
    global _lib
    if _lib is None:
        with _lib_lock:
            if _lib is None:
                if not os.path.isfile(LIB_PATH):
                    raise RuntimeError(
                        "airpose_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
                L = ctypes.CDLL(LIB_PATH)
                abi = getattr(L, "apg_abi_version", None)
                if abi is None or abi() != ABI_VERSION:
                    raise RuntimeError("airpose_amd: %s exports ABI %s, this binding is written against ABI %d (include/airpose_grad.h: "
                                       "APG_ABI_VERSION) -- rebuild the library" % (LIB_PATH, "?" if abi is None else abi(), ABI_VERSION))
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(L, name)
                    fn.restype, fn.argtypes = res, args
                _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().apg_last_error().decode("utf-8", "replace")
        raise RuntimeError("airpose_grad %s failed (status %d): %s" % (what, rc, msg))


def ptrs(tensors):
    """HOST array of device pointers (None -> NULL) for the entry points that take one."""
    arr = (_c.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
    return arr


def ints(values):
    return (_c.c_int * len(values))(*values)


def vp(t):
    """a tensor's device pointer (None -> NULL)"""
    return _c.c_void_p(None if t is None else t.data_ptr())


def stream(device):
    """the current stream of `device`, as the entry points take it"""
    return _c.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dropout_mask(seed, layer, rows, cols, p, device):
    """(rows, cols) uint8 on `device`: exactly the keep mask of (seed, layer) the head kernels apply (1 = kept)."""
    out = torch.empty(rows, cols, device=device, dtype=torch.uint8)
    with torch.cuda.device(device):
        check(lib().apg_dropout_mask(int(seed), int(layer), int(rows), int(cols), float(p), vp(out), stream(device)),
              "apg_dropout_mask")
    return out
