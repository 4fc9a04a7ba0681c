"""The one function the reference takes from the body-model package's `lbs` module (`from smplx import lbs`,
copenet/src/copenet/dsets/aerialpeople.py:177: `lbs.batch_rodrigues(smplpose.reshape(-1, 3))`), as one HIP launch through the
C ABI.  smplx 0.1.28 `lbs.batch_rodrigues` (the package is absent here: restated from the published source, held by
known-answer tests and the CPU oracle): angle = |r + 1e-8|, K = skew(r / angle), R = I + sin K + (1 - cos) K K."""
import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from .geometry import _rodrigues


class _BatchRodrigues(torch.autograd.Function):
    """(N,3) fp32 contiguous CUDA axis-angle -> (N,3,3); backward: ap_batch_rodrigues_bwd (the kernel's own adjoint)."""

    @staticmethod
    def forward(ctx, aa):
        ctx.save_for_backward(aa)
        return _rodrigues(aa, 0, "lbs.batch_rodrigues")

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        aa, = ctx.saved_tensors
        dev = aa.device
        g = N.f32c(g, dev)
        out = torch.empty_like(aa)
        if aa.shape[0]:
            with torch.cuda.device(dev):
                N.check(N.lib().ap_batch_rodrigues_bwd(N.dptr(aa), aa.shape[0], N.dptr(g), N.dptr(out), N.stream_ptr(dev)),
                        "ap_batch_rodrigues_bwd")
        return out


def batch_rodrigues(rot_vecs, epsilon=1e-8, dtype=None):
    """(N,3) axis-angle -> (N,3,3).  `epsilon` is the published default and is what the kernel uses; `dtype` is ignored
    (float32 on the GPU).  Differentiable when rot_vecs requires grad."""
    if epsilon != 1e-8:
        raise ValueError("airpose_amd.lbs.batch_rodrigues: only the published epsilon = 1e-8 is implemented")
    if torch.is_grad_enabled() and isinstance(rot_vecs, torch.Tensor) and rot_vecs.requires_grad and rot_vecs.is_cuda:
        return _BatchRodrigues.apply(N.f32c(rot_vecs).reshape(-1, 3))      # (conversions: autograd-transparent)
    return _rodrigues(rot_vecs, 0, "lbs.batch_rodrigues")
