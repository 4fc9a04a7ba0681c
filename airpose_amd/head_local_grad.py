"""Trainable view-local and baseline heads: one autograd Function on the generic head of libairpose_grad.so
(apg_head_local_fwd / apg_head_local_bwd, csrc/head_local_grad.hip).

One weight set over R rows, the fc1 column layout given by LAYOUTS: xc = [xf (2048) | segments], fc1 -> drop1 -> fc2 -> drop2 ->
two or three decoders, each added onto a column range of the segments.  It serves
  * copenet.regressor_step (model_copenet.py:185-204 for ONE view, the partner's (art_pose | shape) supplied by the caller), and
    through it copenet_sep (model_copenet_sep.py:189-214);
  * model_hmr.forward_reg (:160-172), model_muhmr.forward_reg (:177-203, both views as 2B rows) and
    model_copenet_singleview.forward_reg (:159-170).
Forward and backward read the LIVE fp32 parameters; the backward keeps only what the forward kernel wrote (xc, h1d, h2d and the
packed decoder weights), so the caller may change its state tensors in place afterwards.  Dropout rows are [0, R).  A (1, width)
segment is broadcast to the R rows and its gradient, (1, width), is summed by the kernels in row order.  Behind
net.set_trainable(True); there is no eager fallback.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from . import _head_util as U
from . import _native_grad as G

# model -> (segments (name, width) in fc1 column order behind the 2048 features, decoders (module, n, residual column))
LAYOUTS = {
    "step": ((("bb", 3), ("pose", 135), ("betas", 10), ("partner", 136)), (("decpose", 135, 3), ("decshape", 10, 138))),
    "hmr": ((("pred_pose", 132), ("pred_shape", 10), ("pred_cam", 3)),
            (("decpose", 132, 0), ("decshape", 10, 132), ("deccam", 3, 142))),
    "muhmr": ((("pred_cam", 3), ("pred_pose", 132), ("pred_shape", 10), ("partner", 136)),
              (("decpose", 132, 3), ("decshape", 10, 135), ("deccam", 3, 0))),
    "singleview": ((("bb", 3), ("pred_pose", 135), ("pred_shape", 10)), (("decpose", 135, 3), ("decshape", 10, 138))),
}


class _HeadLocal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, xf, *rest):
        R, seed, p1, p2, dev, seg_w, dec_n, dec_res = cfg
        nseg, ndec = len(seg_w), len(dec_n)
        segs, (W1, b1, W2, b2), dec = rest[:nseg], rest[nseg:nseg + 4], rest[nseg + 4:]
        K1, Nd = 2048 + sum(seg_w), sum(dec_n)
        xc = torch.empty(R, K1, device=dev, dtype=torch.float32)
        h1d = torch.empty(R, 1024, device=dev, dtype=torch.float32)
        h2d = torch.empty(R, 1024, device=dev, dtype=torch.float32)
        wdec = torch.empty(Nd * 1025, device=dev, dtype=torch.float32)
        outs = [torch.empty(R, n, device=dev, dtype=torch.float32) for n in dec_n]
        ld = [0 if (t.shape[0] == 1 and R != 1) else t.stride(0) for t in segs]
        with torch.cuda.device(dev):
            G.check(G.lib().apg_head_local_fwd(
                R, N.dptr(xf, "xf"), nseg, G.ptrs(segs), G.ints(ld), G.ints(seg_w),
                *(N.dptr(w, "head parameter") for w in (W1, b1, W2, b2)), ndec, G.ptrs(dec[0::2]), G.ptrs(dec[1::2]),
                G.ints(dec_n), G.ints(dec_res), seed, p1, p2, N.dptr(xc), N.dptr(h1d), N.dptr(h2d), N.dptr(wdec), G.ptrs(outs),
                N.stream_ptr(dev)), "apg_head_local_fwd")
        ctx.cfg = cfg
        ctx.bcast = [int(t.shape[0] == 1 and R != 1) for t in segs]
        ctx.xc, ctx.h1d, ctx.h2d, ctx.wdec = xc, h1d, h2d, wdec  # the library's own buffers: nobody else writes them
        ctx.save_for_backward(W1, W2)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        R, seed, p1, p2, dev, seg_w, dec_n, dec_res = ctx.cfg
        nseg, ndec = len(seg_w), len(dec_n)
        W1, W2 = ctx.saved_tensors
        need = ctx.needs_input_grad                            # 0 cfg, 1 xf, 2.. segments, then fc1 / fc2, then the decoders
        K1, Nd = 2048 + sum(seg_w), sum(dec_n)
        new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        g_out = [None if g is None else N.f32c(g, dev) for g in gouts]
        g_xf = new(R, 2048) if need[1] else None
        g_seg = [new(1 if b else R, w) if need[2 + k] else None for k, (w, b) in enumerate(zip(seg_w, ctx.bcast))]
        pshapes = [(1024, K1), (1024,), (1024, 1024), (1024,)]
        for n in dec_n:
            pshapes += [(n, 1024), (n,)]
        g_param = [new(*s) if need[2 + nseg + k] else None for k, s in enumerate(pshapes)]
        L = G.lib()
        nbytes = L.apg_head_local_bwd_workspace_bytes(R, K1, Nd, int(g_xf is not None))
        ws = new((nbytes + 3) // 4)
        with torch.cuda.device(dev):
            G.check(L.apg_head_local_bwd(
                R, nseg, G.ints(seg_w), G.ints(ctx.bcast), ndec, G.ints(dec_n), G.ints(dec_res), N.dptr(ctx.xc), N.dptr(ctx.h1d),
                N.dptr(ctx.h2d), N.dptr(ctx.wdec), N.dptr(W1), N.dptr(W2), seed, p1, p2, G.ptrs(g_out), G.ptrs(g_param),
                N.dptr(g_xf), G.ptrs(g_seg), N.dptr(ws), nbytes, N.stream_ptr(dev)), "apg_head_local_bwd")
        return (None, g_xf) + tuple(g_seg) + tuple(g_param)


def head(net, model, xf, segments, seed=None):
    """One differentiable evaluation of `net`'s head in the layout LAYOUTS[model] on R = xf.shape[0] rows -> one (R, n_d) tensor
    per decoder.  segments: one (1|R, width) tensor per segment.  The seed is recorded in net.last_dropout_seed."""
    if not isinstance(xf, torch.Tensor) or not xf.is_cuda:
        raise RuntimeError("airpose_amd.copenet: inputs must be CUDA (ROCm) tensors; there is no CPU path")
    seg_l, dec_l = LAYOUTS[model]
    dev, R = xf.device, xf.shape[0]
    if R < 1 or xf.dim() != 2 or xf.shape[1] != 2048:
        raise RuntimeError("the head expects (R, 2048) features with R >= 1")
    K1 = 2048 + sum(w for _, w in seg_l)
    params = U.params(net, ("fc1", "fc2") + tuple(d[0] for d in dec_l), dev)
    if tuple(net.fc1.weight.shape) != (1024, K1) or any(tuple(getattr(net, n).weight.shape) != (k, 1024) for n, k, _ in dec_l):
        raise RuntimeError("airpose_amd.copenet: the module's fc1 / decoders do not have the %s layout" % model)
    xf = U.rows(xf, dev, R, 2048, "xf", False).contiguous()
    segs = [U.rows(t, dev, R, w, n, False) for t, (n, w) in zip(segments, seg_l)]
    p1, p2, seed = U.dropout(net, seed)
    cfg = (R, int(seed), p1, p2, dev, tuple(w for _, w in seg_l), tuple(n for _, n, _ in dec_l), tuple(r for _, _, r in dec_l))
    return _HeadLocal.apply(cfg, xf, *segs, *params)


def regressor_step(net, xf, bb, pose, betas, partner, seed=None):
    """copenet.regressor_step, differentiable -> (pose (B,135), betas (B,10)); gradients reach xf, bb, pose, betas and partner."""
    return head(net, "step", xf, (bb, pose, betas, partner), seed)


def hmr_forward_reg(net, xf, pred_pose, pred_shape, pred_cam, iters=1, seed=None):
    """model_hmr.forward_reg (:160-172), `iters` evaluations with fresh masks -> (pose (B,132), shape, cam)."""
    for it in range(max(int(iters), 1)):
        pred_pose, pred_shape, pred_cam = head(net, "hmr", xf, (pred_pose, pred_shape, pred_cam), seed if it == 0 else None)
    return pred_pose, pred_shape, pred_cam


def singleview_forward_reg(net, xf, bb, pred_pose, pred_shape, iters=1, seed=None):
    """model_copenet_singleview.forward_reg (:159-170), `iters` evaluations with fresh masks -> (pose (B,135), shape)."""
    for it in range(max(int(iters), 1)):
        pred_pose, pred_shape = head(net, "singleview", xf, (bb, pred_pose, pred_shape), seed if it == 0 else None)
    return pred_pose, pred_shape


def muhmr_forward_reg(net, xf0, xf1, orient0, orient1, art0, art1, shape0, shape1, cam0, cam1, seed=None):
    """model_muhmr.forward_reg (:177-203): both views as ONE call of 2B rows (view 0, then view 1); each view's partner columns
    are the other view's OLD (art_pose | shape), put there with torch.cat, so autograd routes their gradient."""
    B = xf0.shape[0]
    ex = lambda t: t.expand(B, -1) if t.shape[0] == 1 and B != 1 else t
    orient0, orient1, art0, art1, shape0, shape1, cam0, cam1 = (ex(t) for t in (orient0, orient1, art0, art1, shape0, shape1,
                                                                              cam0, cam1))
    xf = torch.cat([xf0, xf1], 0)
    cam = torch.cat([cam0, cam1], 0)
    pose = torch.cat([torch.cat([orient0, art0], 1), torch.cat([orient1, art1], 1)], 0)
    shape = torch.cat([shape0, shape1], 0)
    partner = torch.cat([torch.cat([art1, shape1], 1), torch.cat([art0, shape0], 1)], 0)
    p, s, c = head(net, "muhmr", xf, (cam, pose, shape, partner), seed)
    return p[:B], s[:B], c[:B], p[B:], s[B:], c[B:]
