"""Trainable ResNet-50 trunk: copenet.forward_feat_ext (model_copenet.py:161-176) as an autograd Function on libairpose_grad.so.

Forward and backward are hand-written gfx950 kernels (trunk_grad.hip) driven by one C++ walker per call (apg_trunk_fwd /
apg_trunk_bwd): the ~400 launches of a step stay off ctypes.  The 53 conv weights and BatchNorm affines are read live from the
module on every call (nothing is packed), so an optimizer step takes effect on the next call.

BatchNorm follows the module's mode, as nn.BatchNorm2d does:
  - train mode: batch statistics, and running_mean / running_var updated in place by the kernels (momentum, unbiased variance);
    num_batches_tracked += 1 here.  The kernels write through raw pointers, so the version counters of the running buffers are
    bumped explicitly: copenet._signature then repacks the inference handle on the next eval-mode call;
  - eval mode: the running statistics (the "frozen BN" fine-tune), left unchanged.
The activations backward needs live in one workspace the forward fills (apg_trunk_workspace_bytes(n, 1), kept by the autograd
graph until backward); without grad the forward runs on a smaller one and records nothing.

precision="bf16" (copenet.set_trunk_trainable(True, precision="bf16")) runs the same graph through trunk_grad_bf16.hip: bf16 NHWC
activations and activation gradients inside the workspace, bf16 x bf16 products accumulated in fp32, fp32 BatchNorm statistics.
The parameters, their .grad, the running buffers, xf and the crop gradient stay fp32 tensors; the bf16 copy of the conv weights is
packed into the call's workspace on every forward call, so nothing is cached across calls either.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from . import _native_grad as G

NLAYERS = 53


def conv_bn_pairs(net):
    """The 53 (Conv2d, BatchNorm2d) pairs of the trunk in state_dict order: conv1 / bn1, then per bottleneck conv1 / bn1,
    conv2 / bn2, conv3 / bn3 and downsample.0 / downsample.1."""
    pairs = [(net.conv1, net.bn1)]
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            pairs += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                pairs.append((blk.downsample[0], blk.downsample[1]))
    assert len(pairs) == NLAYERS
    return pairs


def bn_config(pairs):
    """(momentum, eps) shared by every BatchNorm2d of the trunk; the walker takes one value of each."""
    moms = {bn.momentum for _, bn in pairs}
    epss = {bn.eps for _, bn in pairs}
    if None in moms:
        raise RuntimeError("airpose_amd.copenet: BatchNorm2d(momentum=None) (a cumulative moving average) is not supported by the "
                           "trainable trunk; give every BatchNorm2d a float momentum")
    if len(moms) != 1 or len(epss) != 1:
        raise RuntimeError("airpose_amd.copenet: the trainable trunk needs one momentum and one eps for all 53 BatchNorm2d modules, "
                           "got momentum %s, eps %s" % (sorted(moms), sorted(epss)))
    if any(not bn.track_running_stats or not bn.affine for _, bn in pairs):
        raise RuntimeError("airpose_amd.copenet: the trainable trunk needs affine BatchNorm2d modules that track running stats")
    return float(moms.pop()), float(epss.pop())


def _live(t, dev, what):
    if t.device != dev:
        raise RuntimeError("airpose_amd.copenet: the trunk's %s live on %s, the inputs on %s -- call net.to(dev) first"
                           % (what, t.device, dev))
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("airpose_amd.copenet: the trunk's %s must be contiguous fp32" % what)
    return t


def _tables(pairs, dev):
    """params: 53 x (W, gamma, beta) (the autograd inputs); bufs: 53 x (running_mean, running_var)."""
    params, bufs = [], []
    for conv, bn in pairs:
        params += [_live(conv.weight, dev, "parameters"), _live(bn.weight, dev, "parameters"), _live(bn.bias, dev, "parameters")]
        bufs += [_live(bn.running_mean, dev, "buffers"), _live(bn.running_var, dev, "buffers")]
    return params, bufs


def _table_ptrs(params, bufs):
    t = []
    for k in range(NLAYERS):
        t += list(params[3 * k:3 * k + 3]) + list(bufs[2 * k:2 * k + 2])
    return G.ptrs(t)


def _prec(precision):
    if precision not in G.PRECISIONS:
        raise RuntimeError("airpose_amd.copenet: the trainable trunk's precision is one of %s, got %r" % (sorted(G.PRECISIONS), precision))
    return G.PRECISIONS[precision]


def _run_fwd(n, x, params, bufs, train, momentum, eps, save, dev, precision="fp32"):
    L = G.lib()
    if precision != "fp32":
        return _run_fwd_p(L, _prec(precision), n, x, params, bufs, train, momentum, eps, save, dev)
    nbytes = L.apg_trunk_workspace_bytes(n, int(save))
    if nbytes <= 0:
        raise RuntimeError("airpose_amd.copenet: the trainable trunk takes 1 <= n <= 2048 crops per call, got %d" % n)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    xf = torch.empty(n, 2048, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        G.check(L.apg_trunk_fwd(n, N.dptr(x, "x"), _table_ptrs(params, bufs), int(train), momentum, eps, N.dptr(xf), int(save),
                                ws.data_ptr(), nbytes, N.stream_ptr(dev)), "apg_trunk_fwd")
    return xf, ws


def _run_fwd_p(L, prec, n, x, params, bufs, train, momentum, eps, save, dev):
    nbytes = L.apg_trunk_workspace_bytes_p(n, int(save), prec)
    if nbytes <= 0:
        raise RuntimeError("airpose_amd.copenet: the trainable trunk takes 1 <= n <= 2048 crops per call, got %d" % n)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)     # the caching allocator hands out 512-byte aligned blocks
    xf = torch.empty(n, 2048, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        G.check(L.apg_trunk_fwd_p(prec, n, N.dptr(x, "x"), _table_ptrs(params, bufs), int(train), momentum, eps, N.dptr(xf), int(save),
                                  ws.data_ptr(), nbytes, N.stream_ptr(dev)), "apg_trunk_fwd_p")
    return xf, ws


class _Trunk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, x, *params):
        n, train, momentum, eps, bufs, dev, precision = cfg
        xf, ws = _run_fwd(n, x, params, bufs, train, momentum, eps, True, dev, precision)
        ctx.cfg = cfg
        ctx.ws = ws                                              # saved activations: the library's own buffer
        ctx.save_for_backward(*params)                           # version check: the parameters must not change before backward
        return xf

    @staticmethod
    @once_differentiable
    def backward(ctx, g_xf):
        n, train, momentum, eps, bufs, dev, precision = ctx.cfg
        params = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_xf = N.f32c(g_xf, dev)
        g_params = [torch.empty_like(p) if need[2 + k] else None for k, p in enumerate(params)]
        g_x = torch.empty(n, 3, 224, 224, device=dev, dtype=torch.float32) if need[1] else None
        ws, ctx.ws = ctx.ws, None
        with torch.cuda.device(dev):
            if precision == "fp32":
                G.check(G.lib().apg_trunk_bwd(n, _table_ptrs(list(params), bufs), int(train), N.dptr(g_xf), G.ptrs(g_params),
                                              N.dptr(g_x), ws.data_ptr(), ws.numel(), N.stream_ptr(dev)), "apg_trunk_bwd")
            else:
                G.check(G.lib().apg_trunk_bwd_p(_prec(precision), n, _table_ptrs(list(params), bufs), int(train), N.dptr(g_xf),
                                                G.ptrs(g_params), N.dptr(g_x), ws.data_ptr(), ws.numel(), N.stream_ptr(dev)),
                        "apg_trunk_bwd_p")
        return (None, g_x) + tuple(g_params)


def forward_feat_ext(net, x, precision="fp32"):
    """(n, 3, 224, 224) NCHW crops -> (n, 2048) features on the trainable path; BatchNorm in the module's mode (see the module
    docstring).  Records the autograd graph when grad is enabled and x or a trunk parameter requires grad.  precision: "fp32"
    or "bf16" (see the module docstring)."""
    _prec(precision)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("airpose_amd.copenet: inputs must be CUDA (ROCm) tensors; there is no CPU path")
    dev = x.device
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224) or x.shape[0] < 1:
        raise RuntimeError("forward_feat_ext expects (n, 3, 224, 224) NCHW crops (AvgPool2d(7) fixes the size)")
    pairs = conv_bn_pairs(net)
    momentum, eps = bn_config(pairs)
    params, bufs = _tables(pairs, dev)
    train = bool(net.training)
    x = N.f32c(x)
    n = x.shape[0]
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        xf = _Trunk.apply((n, train, momentum, eps, bufs, dev, precision), x, *params)
    else:
        xf, _ = _run_fwd(n, x, params, bufs, train, momentum, eps, False, dev, precision)
    if train:
        with torch.no_grad():
            torch._foreach_add_([bn.num_batches_tracked for _, bn in pairs], 1)
        torch.autograd.graph.increment_version(bufs)            # the kernels wrote running_mean / running_var
    return xf
