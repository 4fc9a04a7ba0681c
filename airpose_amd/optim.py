"""torch.optim.Adam's update as one hand-written gfx950 pass over a whole parameter list: FusedAdam.

All four reference trainers configure `torch.optim.Adam(self.model.parameters(), lr=..., weight_decay=0, amsgrad=True)`
(copenet_twoview.py, copenet_singleview.py, hmr.py, muhmr.py: configure_optimizers); swapping the class name is the whole change.
apg_adam_step (csrc/optim.hip, include/airpose_grad.h) reads p, g, m, v, vmax and writes p, m, v, vmax once, 64 tensors per launch,
where torch's foreach path makes one pass per arithmetic operation.  The per-element algorithm is _single_tensor_adam's with
maximize = False and L2 weight decay; the state (`step` as a CPU tensor, `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq`) and the
param-group layout are torch's, so a state_dict of either class loads into the other.  There is no fallback: a parameter the kernel
cannot take (CPU, not fp32, not contiguous, a sparse gradient) is refused by name, and a missing library is an error.
"""
import ctypes
import operator

import torch

from . import _native_grad as G

# the options of torch.optim.Adam this class does not implement, with the only value each may hold in a param group (they are part of
# every group so that state_dict() has exactly torch's layout and loads into torch.optim.Adam)
_INERT = dict(maximize=False, foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
# of those, the ones that only choose between torch's implementations of the same update: a checkpoint's values are kept (they
# travel back to torch.optim.Adam with the next state_dict) and ignored
_IMPLEMENTATION = ("foreach", "fused")


def _check_options(group):
    lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
    for name, x in (("lr", lr), ("eps", eps), ("weight_decay", wd), ("betas[0]", b1), ("betas[1]", b2)):
        if torch.is_tensor(x):
            raise TypeError("FusedAdam: %s must be a Python number, not a tensor (that is torch's capturable mode)" % name)
    if not 0.0 <= lr:
        raise ValueError("FusedAdam: invalid learning rate: %r" % (lr,))
    if not 0.0 <= eps:
        raise ValueError("FusedAdam: invalid epsilon value: %r" % (eps,))
    if not 0.0 <= b1 < 1.0:
        raise ValueError("FusedAdam: invalid beta parameter at index 0: %r" % (b1,))
    if not 0.0 <= b2 < 1.0:
        raise ValueError("FusedAdam: invalid beta parameter at index 1: %r" % (b2,))
    if not 0.0 <= wd:
        raise ValueError("FusedAdam: invalid weight_decay value: %r" % (wd,))
    for name, inert in _INERT.items():
        if name not in _IMPLEMENTATION and group.get(name, inert):
            raise ValueError("FusedAdam: a param group with %s=%r is not supported" % (name, group[name]))


def _check_param(p):
    if not torch.is_tensor(p):
        raise TypeError("FusedAdam: parameters must be tensors, got %s" % type(p).__name__)
    if not p.is_cuda:
        raise ValueError("FusedAdam: a parameter of shape %s lives on %s; the step is a GPU kernel and there is no CPU fallback"
                         % (tuple(p.shape), p.device))
    if p.dtype != torch.float32:
        raise TypeError("FusedAdam: a parameter of shape %s is %s; only float32 parameters are supported" % (tuple(p.shape), p.dtype))
    if not p.is_contiguous():
        raise ValueError("FusedAdam: a parameter of shape %s and strides %s is not contiguous" % (tuple(p.shape), tuple(p.stride())))


def _check_grad(p, g):
    if g.is_sparse:
        raise ValueError("FusedAdam: the gradient of a parameter of shape %s is sparse; sparse gradients are not supported" % (tuple(p.shape),))
    if g.device != p.device or g.dtype != torch.float32 or g.shape != p.shape:
        raise TypeError("FusedAdam: the gradient of a parameter of shape %s on %s is %s %s on %s" %
                        (tuple(p.shape), p.device, g.dtype, tuple(g.shape), g.device))
    if not g.is_contiguous():
        raise ValueError("FusedAdam: the gradient of a parameter of shape %s has strides %s: not contiguous" %
                         (tuple(p.shape), tuple(g.stride())))


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad) with the whole update of a param group in one apg_adam_step call.

    maximize, capturable, differentiable, foreach and fused are not accepted.  Parameters must be contiguous float32 CUDA tensors with
    dense contiguous gradients.  step() runs under no_grad on the current stream of the parameters' device and never synchronises the
    host; a parameter whose .grad is None is left out: its state stays untouched and its step count does not advance."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), **_INERT)
        _check_options(defaults)
        super().__init__(params, defaults)
        G.lib()                                                           # a missing library is an error here, not at the first step

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _check_options(group)
            for p in group["params"]:
                _check_param(p)
        except (TypeError, ValueError):
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for name, inert in _INERT.items():
                group.setdefault(name, inert)
            group.setdefault("amsgrad", False)
            _check_options(group)
            for p in group["params"]:
                st = self.state.get(p, None)
                if st and "step" in st:                                   # a fused / capturable checkpoint keeps it on the device
                    s = st["step"]
                    st["step"] = torch.tensor(float(s), dtype=torch.float32) if not torch.is_tensor(s) else s.detach().to("cpu", torch.float32)
        self.__dict__.pop("_fused_tables", None)

    def _tables(self, group, plist, ptrs, amsgrad):
        """Validate the parameters of one group that have a gradient and their state (created here on first use, as torch does), and
        build what a step needs of them: the HOST pointer tables of apg_adam_step and a numpy view of every step count.  Kept between
        steps while the same parameters, storages and state tensors come back (step() checks that), because this is most of a step's
        host cost: with it a step costs a few attribute reads per tensor."""
        f32 = torch.float32
        dev = plist[0].device
        names = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if amsgrad else ("exp_avg", "exp_avg_sq")
        states = []
        for p in plist:
            _check_param(p)
            if p.device != dev:
                raise ValueError("FusedAdam: one param group holds parameters on %s and on %s; give each device a group of its own" % (dev, p.device))
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=f32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if amsgrad:
                    st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if amsgrad and "max_exp_avg_sq" not in st:                        # amsgrad switched on after the first step: torch raises KeyError
                raise ValueError("FusedAdam: amsgrad=True, but the state of a parameter of shape %s has no max_exp_avg_sq" % (tuple(p.shape),))
            for name in names:
                s = st[name]
                if not (torch.is_tensor(s) and s.dtype is f32 and s.device == dev and s.shape == p.shape and s.is_contiguous()):
                    raise ValueError("FusedAdam: state %s of a parameter of shape %s must be a contiguous float32 tensor of that shape "
                                     "on %s" % (name, tuple(p.shape), dev))
            t = st["step"]
            if not (torch.is_tensor(t) and t.device.type == "cpu" and t.dtype is f32 and t.dim() == 0):
                t = st["step"] = torch.tensor(float(t), dtype=f32)
            states.append(st)
        n = len(plist)
        # the step counts move into ONE CPU buffer, each state["step"] a 0-d view of its element (still a CPU float32 tensor of its own
        # to every reader, torch.optim.Adam included): a step then advances all of them with one addition
        counts = torch.stack([st["step"] for st in states])
        for i, st in enumerate(states):
            st["step"] = counts[i]
        held = [tuple(st[name] for name in ("step",) + names) for st in states]
        vp = ctypes.c_void_p * n
        tab = lambda k: vp(*[h[k].data_ptr() or None for h in held])          # (a tensor without elements may have no storage: NULL)
        return dict(ids=[id(p) for p in plist], ptrs=ptrs, amsgrad=amsgrad, dev=dev, states=states, held=held, shapes=[p.shape for p in plist],
                    getter=operator.itemgetter(*(("step",) + names)), held_ids=[tuple(map(id, h)) for h in held],
                    counts=counts.numpy(), n=n, P=vp(*[x or None for x in ptrs]), G=vp(), M=tab(1), V=tab(2), X=tab(3) if amsgrad else None,
                    numel=(ctypes.c_int64 * n)(*[p.numel() for p in plist]), step=(ctypes.c_int64 * n)())

    def _current(self, e, plist, ptrs, amsgrad):
        """the tables of the last step still describe this one: the same parameters at the same addresses with the same state tensors"""
        if e is None or e["amsgrad"] != amsgrad or e["ptrs"] != ptrs or e["ids"] != [id(p) for p in plist]:
            return False
        getter, state = e["getter"], self.state
        try:
            for p, st, ids in zip(plist, e["states"], e["held_ids"]):
                if state.get(p) is not st or tuple(map(id, getter(st))) != ids:
                    return False
        except KeyError:
            return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = G.lib()
        f32, strided = torch.float32, torch.strided
        cache = self.__dict__.setdefault("_fused_tables", {})
        for gi, group in enumerate(self.param_groups):
            _check_options(group)
            amsgrad = bool(group["amsgrad"])
            plist, glist = [], []
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    plist.append(p)
                    glist.append(g)
            if not plist:
                continue
            # everything is checked before any step count moves, so a refused step changes nothing
            ptrs = [p.data_ptr() for p in plist]
            e = cache.get(gi)
            if not self._current(e, plist, ptrs, amsgrad):
                cache.pop(gi, None)
                e = cache[gi] = self._tables(group, plist, ptrs, amsgrad)
            dev, gp = e["dev"], []
            for p, g, shape in zip(plist, glist, e["shapes"]):
                # (the fast predicate only decides whether to call the check that words the refusal)
                if not (g.dtype is f32 and g.layout is strided and g.shape == shape and g.device == dev and g.is_contiguous()):
                    _check_grad(p, g)
                gp.append(g.data_ptr() or None)
            n = e["n"]
            e["G"] = (ctypes.c_void_p * n)(*gp)
            counts = e["counts"]                                              # numpy view of the buffer behind every state["step"]
            counts += 1
            e["step"][:] = counts.astype("int64").tolist()
            beta1, beta2 = group["betas"]
            with torch.cuda.device(dev):
                rc = L.apg_adam_step(n, e["P"], e["G"], e["M"], e["V"], e["X"], e["numel"], e["step"], float(group["lr"]), float(beta1),
                                     float(beta2), float(group["eps"]), float(group["weight_decay"]), G.stream(dev))
            G.check(rc, "apg_adam_step")
        return loss
