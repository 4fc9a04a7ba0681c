"""GPU versions of the reference's geometry helpers on the hot path
(copenet/src/copenet/utils/geometry.py:47-61 rot6d_to_rotmat, :63-91 perspective_projection).
Each is one launch of a hand-written HIP kernel through the C ABI; no CPU path.  rot6d_to_rotmat and perspective_projection are
differentiable when an input requires grad: the forward is the same kernel, the backward a kernel of libairpose_grad.so."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from . import _native_grad as G


def _cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError("airpose_amd.geometry.%s: CUDA (ROCm) tensors only; there is no CPU path" % name)
    return t.device


def _grad_wanted(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _rot6d_fwd(x):
    dev = x.device
    out = torch.empty(x.shape[0], 3, 3, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        N.check(N.lib().ap_rot6d_to_rotmat(N.dptr(x), x.shape[0], N.dptr(out), N.stream_ptr(dev)), "ap_rot6d_to_rotmat")
    return out


class _Rot6d(torch.autograd.Function):
    """Forward: ap_rot6d_to_rotmat (the no-grad kernel, same bits); backward: apg_rot6d_to_rotmat_bwd."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _rot6d_fwd(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        dev = x.device
        g = N.f32c(g)
        gx = torch.empty_like(x)
        with torch.cuda.device(dev):
            G.check(G.lib().apg_rot6d_to_rotmat_bwd(N.dptr(x), x.shape[0], N.dptr(g), N.dptr(gx), N.stream_ptr(dev)),
                    "apg_rot6d_to_rotmat_bwd")
        return gx


def rot6d_to_rotmat(x):
    """(B,6k) 6-D rotations -> (B*k,3,3)   [geometry.py:47-61]; differentiable when x requires grad."""
    _cuda(x, "rot6d_to_rotmat")
    if _grad_wanted(x):
        return _Rot6d.apply(N.f32c(x).reshape(-1, 6))
    return _rot6d_fwd(N.f32c(x).reshape(-1, 6))


def _rodrigues(theta, variant, name):
    dev = _cuda(theta, name)
    t = N.f32c(theta).reshape(-1, 3)
    out = torch.empty(t.shape[0], 3, 3, device=dev, dtype=torch.float32)
    if t.shape[0]:
        with torch.cuda.device(dev):
            N.check(N.lib().ap_batch_rodrigues(N.dptr(t), t.shape[0], variant, N.dptr(out), N.stream_ptr(dev)),
                    "ap_batch_rodrigues")
    return out


def batch_rodrigues(theta):
    """(N,3) axis-angle -> (N,3,3) through a unit quaternion   [geometry.py:9-45]"""
    return _rodrigues(theta, 1, "batch_rodrigues")


def rotation_matrix_to_angle_axis(rotation_matrix):
    """tgm.rotation_matrix_to_angle_axis (torchgeometry 0.1.2): (N,3,4) -- or (N,3,3) -- -> (N,3), the conversion the
    caller applies to pred_rotmat for pred_angles [copenet_twoview.py:323-324]."""
    dev = _cuda(rotation_matrix, "rotation_matrix_to_angle_axis")
    r = N.f32c(rotation_matrix)
    if r.dim() != 3 or r.shape[1] != 3 or r.shape[2] not in (3, 4):
        raise ValueError("rotation_matrix_to_angle_axis: expected (N,3,4) or (N,3,3), got %s" % (tuple(r.shape),))
    out = torch.empty(r.shape[0], 3, device=dev, dtype=torch.float32)
    if r.shape[0]:
        with torch.cuda.device(dev):
            N.check(N.lib().ap_rotmat_to_angle_axis(N.dptr(r), r.shape[0], r.shape[2], N.dptr(out), N.stream_ptr(dev)),
                    "ap_rotmat_to_angle_axis")
    return out


def _projection_fwd(points, rotation, translation, fx, fy, cc):
    dev = points.device
    B, P = points.shape[0], points.shape[1]
    out = torch.empty(B, P, 2, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        N.check(N.lib().ap_perspective_projection(N.dptr(points), B, P, N.dptr(rotation), N.dptr(translation), fx, fy,
                                                  N.dptr(cc), N.dptr(out), N.stream_ptr(dev)), "ap_perspective_projection")
    return out


class _Projection(torch.autograd.Function):
    """Forward: ap_perspective_projection (the no-grad kernel, same bits); backward: apg_perspective_projection_bwd."""

    @staticmethod
    def forward(ctx, points, rotation, translation, cc, fx, fy):
        ctx.fxy = (fx, fy)
        ctx.save_for_backward(points, rotation, translation)
        return _projection_fwd(points, rotation, translation, fx, fy, cc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        points, rotation, translation = ctx.saved_tensors
        need = ctx.needs_input_grad
        dev = points.device
        B = points.shape[0]
        g = N.f32c(g)
        mk = lambda flag, *shape: torch.empty(*shape, device=dev, dtype=torch.float32) if flag else None
        gp, gr, gt, gc = mk(need[0], *points.shape), mk(need[1], B, 3, 3), mk(need[2], B, 3), mk(need[3], B, 2)
        with torch.cuda.device(dev):
            G.check(G.lib().apg_perspective_projection_bwd(N.dptr(points), B, points.shape[1], N.dptr(rotation),
                                                           N.dptr(translation), ctx.fxy[0], ctx.fxy[1], N.dptr(g), N.dptr(gp),
                                                           N.dptr(gr), N.dptr(gt), N.dptr(gc), N.stream_ptr(dev)),
                    "apg_perspective_projection_bwd")
        return gp, gr, gt, gc, None, None


def perspective_projection(points, rotation, translation, focal_length, camera_center):
    """(bs,N,3) -> (bs,N,2)   [geometry.py:63-91]; camera_center (bs,2) or the caller's (1,bs,2).  Differentiable in points,
    rotation, translation and camera_center when one of them requires grad; focal_length is not differentiable."""
    dev = _cuda(points, "perspective_projection")
    B = points.shape[0]
    if isinstance(focal_length, torch.Tensor) and focal_length.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("perspective_projection: focal_length is not differentiable (pass it detached)")
    points = N.f32c(points)
    rotation = N.f32c(rotation, dev)
    translation = N.f32c(translation, dev)
    cc = N.f32c(camera_center, dev).reshape(-1, 2)
    if cc.shape[0] != B:
        cc = cc.expand(B, 2).contiguous()
    fx, fy = float(focal_length[0]), float(focal_length[1])
    if _grad_wanted(points, rotation, translation, cc):
        return _Projection.apply(points, rotation, translation, cc, fx, fy)
    return _projection_fwd(points, rotation, translation, fx, fy, cc)


def lstsq_triangulation(intrinsic, extrinsic, points_2d, min_ray_angle_deg=0.0):
    """The batched two-camera mirror of the reference's lstsq_triangulation (copenet_real utils/geometry.py:160-192), one launch of
    apg_xview_triangulate (libairpose_grad.so), solved per joint in fp64 on the device.
    intrinsic (B, 2, 3, 3) (fx, fy, cx, cy are read: the reference's K^-1 agrees where the skew is 0); extrinsic (B, 2, 4, 4) or
    (B, 2, 3, 4), world -> camera; points_2d (B, 2, J, 2) or (B, 2, J, 3) with a confidence (absent: 1).
    -> (points (B, J, 3) in the world frame, valid (B, J) bool).  A joint is valid where both confidences are > 0, both points are
    finite, the extrinsics are finite and orthonormal to 1e-3 and the two rays meet at min_ray_angle_deg or more; points is 0
    elsewhere."""
    dev = _cuda(points_2d, "lstsq_triangulation")
    if points_2d.dim() != 4 or points_2d.shape[1] != 2 or points_2d.shape[3] not in (2, 3) or points_2d.shape[2] < 1:
        raise RuntimeError("lstsq_triangulation: points_2d must be (B, 2, J, 2 or 3), got %s" % (tuple(points_2d.shape),))
    B, J = points_2d.shape[0], points_2d.shape[2]
    if tuple(intrinsic.shape) != (B, 2, 3, 3):
        raise RuntimeError("lstsq_triangulation: intrinsic must be (%d, 2, 3, 3), got %s" % (B, tuple(intrinsic.shape)))
    if tuple(extrinsic.shape) not in ((B, 2, 4, 4), (B, 2, 3, 4)):
        raise RuntimeError("lstsq_triangulation: extrinsic must be (%d, 2, 4, 4) or (%d, 2, 3, 4), got %s" % (B, B, tuple(extrinsic.shape)))
    if not 0.0 <= float(min_ray_angle_deg) <= 90.0:
        raise RuntimeError("lstsq_triangulation: min_ray_angle_deg must be in 0 .. 90, got %r" % (min_ray_angle_deg,))
    if B < 1:
        raise RuntimeError("lstsq_triangulation: points_2d holds no sample")
    pts = N.f32c(points_2d.detach(), dev)
    if pts.shape[3] == 2:
        pts = torch.cat([pts, torch.ones(B, 2, J, 1, device=dev, dtype=torch.float32)], 3)
    K, E = N.f32c(intrinsic.detach(), dev), N.f32c(extrinsic.detach(), dev)
    if E.shape[2] == 3:                                      # the entry point strides over 4 x 4 matrices; row 3 is never read
        E = torch.cat([E, torch.zeros(B, 2, 1, 4, device=dev, dtype=torch.float32)], 2)
    kp, Kv, Ev = [pts[:, v].contiguous() for v in range(2)], [K[:, v].contiguous() for v in range(2)], [E[:, v].contiguous() for v in range(2)]
    out = torch.empty(B, J, 4, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        G.check(G.lib().apg_xview_triangulate(B, J, G.vp(kp[0]), G.vp(kp[1]), G.vp(Kv[0]), G.vp(Kv[1]), G.vp(Ev[0]), G.vp(Ev[1]),
                                              math.sin(math.radians(float(min_ray_angle_deg))) ** 2, G.vp(out), G.stream(dev)),
                "apg_xview_triangulate")
    return out[..., :3], out[..., 3] > 0
