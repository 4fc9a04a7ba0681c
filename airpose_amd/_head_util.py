"""What the bindings of the two trainable heads (head_grad.py, head_local_grad.py) share: input and parameter checks and the
dropout configuration of one evaluation."""
import torch


def new_seed():
    """A fresh dropout seed from torch's default CPU generator (torch.manual_seed reproduces a run)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def rows(t, dev, R, width, name, expand):
    """fp32 on dev, (1|R, width) with contiguous columns (any row stride >= width, or 0).  expand: a (1, width) input comes back as
    R rows of stride 0; otherwise it stays one row."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != width or t.shape[0] not in (1, R):
        raise RuntimeError("%s must be (%d, %d), got %s" % (name, R, width, tuple(getattr(t, "shape", ()))))
    if t.device != dev:
        t = t.to(dev)
    if t.dtype != torch.float32:
        t = t.float()
    if expand and t.shape[0] != R:
        t = t.expand(R, width)
    if t.stride(1) != 1 or (t.stride(0) != 0 and t.stride(0) < width):
        t = t.contiguous()
    return t


def params(net, names, dev):
    """[weight, bias] of each named module of net, checked: on dev, contiguous fp32 (the kernels read them in place)."""
    out = []
    for name in names:
        m = getattr(net, name)
        for p in (m.weight, m.bias):
            if p.device != dev:
                raise RuntimeError("airpose_amd.copenet: the head's parameters live on %s, the inputs on %s -- call net.to(dev) "
                                   "first" % (p.device, dev))
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("airpose_amd.copenet: the head's parameters must be contiguous fp32")
            out.append(p)
    return out


def dropout(net, seed):
    """(p1, p2, seed) of one evaluation: the rates of net.drop1 / drop2 (0 in eval mode) and the seed, a fresh one when None; it is
    recorded in net.last_dropout_seed."""
    p1 = float(net.drop1.p) if net.drop1.training else 0.0
    p2 = float(net.drop2.p) if net.drop2.training else 0.0
    if seed is None:
        seed = new_seed()
    net.last_dropout_seed = seed
    return p1, p2, seed
