"""What TrainingLoss (loss.py) and RealDataLoss (loss_real.py) share: a fused loss whose C entry point writes the terms and the gradient
seeds in one pass.  The autograd Function that owns the seed buffer, the tensor check, and the modules' base class.
"""
import torch
from torch.autograd.function import once_differentiable


def check_tensor(owner, t, dev, shape, name, cast):
    """fp32, contiguous, on dev, of `shape` (None = any extent); anything else is refused by name, in owner's name.
    cast: another floating-point type is converted (True) or refused (False)"""
    if not torch.is_tensor(t):
        raise RuntimeError("%s: %s must be a tensor, got %s" % (owner, name, type(t).__name__))
    if t.device != dev:
        raise RuntimeError("%s: %s lives on %s, the predictions on %s" % (owner, name, t.device, dev))
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise RuntimeError("%s: %s must be %s, got %s" % (owner, name, tuple("*" if s is None else s for s in shape), tuple(t.shape)))
    if t.dtype != torch.float32:
        if not cast:
            raise RuntimeError("%s: %s must be float32, got %s" % (owner, name, t.dtype))
        if not t.is_floating_point():
            raise RuntimeError("%s: %s must be a floating-point tensor, got %s" % (owner, name, t.dtype))
        t = t.float()
    return t.contiguous()


class SeededLoss(torch.autograd.Function):
    """(dev, number of terms, grad flag, launch, the predictions: None = absent) -> (the 0-d loss in storage of its own, the
    (nterms,) terms: not differentiable).  launch(terms, grads) makes the workspace query and the C call, looking the library up
    through _native_grad.lib() as it runs; grads holds per prediction its seed tensor or None, and is None itself when no
    gradient is wanted (forward only)."""

    @staticmethod
    def forward(ctx, dev, nterms, grad, launch, *preds):
        # (needs_input_grad follows requires_grad alone; under no_grad nothing will call backward, so nothing is asked for)
        need = ctx.needs_input_grad[4:] if grad else (False,) * len(preds)
        # every seed is a slice of ONE flat buffer (each slice starts on a 16-byte boundary), so that backward scales them in one launch
        offs, total = [], 0
        for k, p in enumerate(preds):
            offs.append(total if (p is not None and need[k]) else None)
            if offs[-1] is not None:
                total += (p.numel() + 3) // 4 * 4
        flat = torch.empty(total, device=dev, dtype=torch.float32) if total else None
        grads = [None if o is None else flat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, preds)]
        terms = torch.empty(nterms, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            launch(terms, grads if total else None)
        ctx.flat, ctx.offs, ctx.shapes = flat, offs, [None if p is None else p.shape for p in preds]     # this call's own buffer
        loss = terms[0].clone()                                  # its own element: in-place work on terms cannot reach the loss
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms):
        if ctx.flat is None:
            return (None,) * (4 + len(ctx.offs))
        scaled = ctx.flat * g                                    # the padding between slices is never read
        return (None,) * 4 + tuple(None if o is None else scaled[o:o + s.numel()].view(s) for o, s in zip(ctx.offs, ctx.shapes))


class SeededLossModule(torch.nn.Module):
    """A loss of several kinds, each with its reference trainer's default weights.  A subclass sets
      _owner       its name in messages
      _kinds       the kinds
      _defaults    kind -> {weight name: default}
      _required    kind -> weight names without a default, which the caller must give
      _term_names  the order of the kernel's terms output
      _skip        kind -> the terms its `losses` dict leaves out
    """
    _required = {}

    def __init__(self, kind, weights, who):
        """who: what the weight-name refusals call the module"""
        super().__init__()
        if kind not in self._kinds:
            raise ValueError("%s: kind must be one of %s, got %r" % (self._owner, ", ".join(self._kinds), kind))
        required = self._required.get(kind, ())
        names = set(self._defaults[kind]) | set(required)
        unknown = sorted(set(weights) - names)
        if unknown:
            raise ValueError("%s: unknown weight(s) %s; the names are %s" % (who, unknown, sorted(names)))
        missing = [n for n in required if n not in weights]
        if missing:
            raise ValueError("%s: %s must be given: the reference trainer reads them and declares no default" % (who, ", ".join(missing)))
        self.kind = kind
        self.weights = dict(self._defaults[kind])
        self.weights.update({k: float(v) for k, v in weights.items()})

    def extra_repr(self):
        return "kind=%r, %s" % (self.kind, ", ".join("%s=%g" % kv for kv in sorted(self.weights.items())))

    def losses(self, terms):
        """the reference's `losses` dict of this kind from forward's terms: ONE device-to-host copy"""
        host = terms.detach().cpu().tolist()
        return {n: v for n, v in zip(self._term_names, host) if n not in self._skip[self.kind]}

    def _device_of(self, first):
        """the device of the first prediction, which the others must share"""
        if not torch.is_tensor(first) or not first.is_cuda:
            raise RuntimeError("%s: predictions must be CUDA (ROCm) tensors; there is no CPU path" % self._owner)
        return first.device
