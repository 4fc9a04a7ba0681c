"""Trainable IEF regressor head: copenet.forward_reg (model_copenet.py:178-204) as an autograd Function on libairpose_grad.so.

Forward and backward are hand-written gfx950 kernels (apg_head_fwd / apg_head_bwd) on the LIVE fp32 parameters of fc1, fc2,
decpose and decshape: nothing is packed, so an optimizer step takes effect on the next call.  Both views run as one pass of
R = 2B rows.  The backward keeps what apg_head_fwd wrote (the fc1 input with its snapshot of the state columns, and the two
dropped-out hidden layers) and none of the caller's state tensors, so the caller may change them in place after the forward
(the reference divides pred_pose[:, :3] and the translation by trans_scale in place, copenet_twoview.py:214-220).
"""
import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from . import _head_util as U
from . import _native_grad as G
from ._head_util import new_seed  # noqa: F401  (the models and tests import it from here)

STATE_W = (3, 3, 6, 126, 10)              # bb, pos, orient, art, shape
PARAMS = ("fc1", "fc2", "decpose", "decshape")


class _HeadReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, xf0, xf1, bb0, pos0, or0, art0, sh0, bb1, pos1, or1, art1, sh1, W1, b1, W2, b2, Wp, bp, Ws, bs):
        B, seed, p1, p2, dev = cfg
        R = 2 * B
        xc = torch.empty(R, 2332, device=dev, dtype=torch.float32)
        h1d = torch.empty(R, 1024, device=dev, dtype=torch.float32)
        h2d = torch.empty(R, 1024, device=dev, dtype=torch.float32)
        pose = [torch.empty(B, 135, device=dev, dtype=torch.float32) for _ in range(2)]
        betas = [torch.empty(B, 10, device=dev, dtype=torch.float32) for _ in range(2)]
        state = (bb0, pos0, or0, art0, sh0, bb1, pos1, or1, art1, sh1)
        with torch.cuda.device(dev):
            G.check(G.lib().apg_head_fwd(B, N.dptr(xf0, "xf0"), N.dptr(xf1, "xf1"), G.ptrs(state), G.ints([t.stride(0) for t in state]),
                                         *(N.dptr(w, "head parameter") for w in (W1, b1, W2, b2, Wp, bp, Ws, bs)),
                                         seed, p1, p2, N.dptr(xc), N.dptr(h1d), N.dptr(h2d), G.ptrs(pose), G.ptrs(betas),
                                         N.stream_ptr(dev)), "apg_head_fwd")
        ctx.cfg = cfg
        ctx.xc, ctx.h1d, ctx.h2d = xc, h1d, h2d                  # the library's own buffers: nobody else writes them
        ctx.save_for_backward(W1, W2, Wp, Ws)
        return pose[0], betas[0], pose[1], betas[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, gp0, gs0, gp1, gs1):
        B, seed, p1, p2, dev = ctx.cfg
        W1, W2, Wp, Ws = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_out = [None if g is None else N.f32c(g, dev) for g in (gp0, gs0, gp1, gs1)]
        # inputs: 1 xf0, 2 xf1, 3..7 state of view 0, 8..12 state of view 1; parameters 13..20
        pshapes = [W1.shape, (1024,), W2.shape, (1024,), Wp.shape, (135,), Ws.shape, (10,)]
        g_param = [torch.empty(s, device=dev, dtype=torch.float32) if need[13 + k] else None for k, s in enumerate(pshapes)]
        g_in = []
        for v in range(2):
            g_in.append(torch.empty(B, 2048, device=dev, dtype=torch.float32) if need[1 + v] else None)
            for k, w in enumerate(STATE_W):
                g_in.append(torch.empty(B, w, device=dev, dtype=torch.float32) if need[3 + 5 * v + k] else None)
        need_gxf = int(g_in[0] is not None or g_in[6] is not None)
        L = G.lib()
        nbytes = L.apg_head_bwd_workspace_bytes(B, need_gxf)
        ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            G.check(L.apg_head_bwd(B, N.dptr(ctx.xc), N.dptr(ctx.h1d), N.dptr(ctx.h2d), N.dptr(W1), N.dptr(W2), N.dptr(Wp),
                                   N.dptr(Ws), seed, p1, p2, G.ptrs(g_out), G.ptrs(g_param), G.ptrs(g_in), N.dptr(ws), nbytes,
                                   N.stream_ptr(dev)), "apg_head_bwd")
        gxf = (g_in[0], g_in[6])
        gst = g_in[1:6] + g_in[7:12]
        return (None,) + gxf + tuple(gst) + tuple(g_param)


def forward_reg(net, xf0, xf1, bb0, bb1, pos0, pos1, orient0, orient1, art0, art1, shape0, shape1, seed=None):
    """One differentiable evaluation of the two-view head -> (pred_pose0, pred_shape0, pred_pose1, pred_shape1)."""
    if not xf0.is_cuda:
        raise RuntimeError("airpose_amd.copenet: inputs must be CUDA (ROCm) tensors; there is no CPU path")
    dev = xf0.device
    B = xf0.shape[0]
    if B < 1 or xf0.dim() != 2 or xf0.shape[1] != 2048 or tuple(xf1.shape) != tuple(xf0.shape):
        raise RuntimeError("forward_reg expects two (B, 2048) feature tensors with B >= 1")
    params = U.params(net, PARAMS, dev)
    xf0 = U.rows(xf0, dev, B, 2048, "xf0", True).contiguous()
    xf1 = U.rows(xf1, dev, B, 2048, "xf1", True).contiguous()
    names = ("bb", "pred_position", "pred_orient", "pred_art_pose", "pred_shape")
    st = []
    for v, ts in enumerate(((bb0, pos0, orient0, art0, shape0), (bb1, pos1, orient1, art1, shape1))):
        st += [U.rows(t, dev, B, w, "%s%d" % (n, v), True) for t, w, n in zip(ts, STATE_W, names)]
    p1, p2, seed = U.dropout(net, seed)
    return _HeadReg.apply((B, seed, p1, p2, dev), xf0, xf1, *st, *params)


def forward_ief(net, xf0, xf1, bb0, bb1, init_position0, init_position1, init_theta0=None, init_theta1=None,
                init_shape0=None, init_shape1=None, iters=3):
    """The IEF loop (model_copenet.py:121-157) from trunk features, forward_reg once per iteration with fresh masks."""
    if int(iters) < 1:
        raise RuntimeError("iters must be >= 1 (forward always evaluates the regressor once)")
    B = xf0.shape[0]

    def _theta(t, name):
        t = net.init_pose if t is None else t
        if t.dim() != 2 or t.shape[1] < 132 or t.shape[0] not in (1, B):
            raise RuntimeError("%s must be (1|B, >=132)" % name)
        return t[:, :6], t[:, 6:132]

    def _shape(t, name):
        t = net.init_shape if t is None else t
        if t.dim() != 2 or t.shape[1] < 10 or t.shape[0] not in (1, B):
            raise RuntimeError("%s must be (1|B, >=10)" % name)
        return t[:, :10]

    o0, a0 = _theta(init_theta0, "init_theta0")
    o1, a1 = _theta(init_theta1, "init_theta1")
    s0, s1 = _shape(init_shape0, "init_shape0"), _shape(init_shape1, "init_shape1")
    p0, b0, p1, b1 = forward_reg(net, xf0, xf1, bb0, bb1, init_position0, init_position1, o0, o1, a0, a1, s0, s1)
    for _ in range(int(iters) - 1):
        p0, b0, p1, b1 = forward_reg(net, xf0, xf1, bb0, bb1, p0[:, :3], p1[:, :3], p0[:, 3:9], p1[:, 3:9],
                                     p0[:, 9:], p1[:, 9:], b0, b1)
    return p0, b0, p1, b1
