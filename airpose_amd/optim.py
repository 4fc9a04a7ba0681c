"""torch.optim.Adam's update as one hand-written gfx950 pass over a whole parameter list: FusedAdam.

All four reference trainers configure `torch.optim.Adam(self.model.parameters(), lr=..., weight_decay=0, amsgrad=True)`
(copenet_twoview.py, copenet_singleview.py, hmr.py, muhmr.py: configure_optimizers); swapping the class name is the whole change.
apg_adam_step (csrc/optim.hip, include/airpose_grad.h) reads p, g, m, v, vmax and writes p, m, v, vmax once, 64 tensors per launch,
where torch's foreach path makes one pass per arithmetic operation.  The per-element algorithm is _single_tensor_adam's with
maximize = False and L2 weight decay; the state (`step` as a CPU tensor, `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq`) and the
param-group layout are torch's, so a state_dict of either class loads into the other.  There is no fallback: a parameter the kernel
cannot take (CPU, not fp32, not contiguous, a sparse gradient) is refused by name, and a missing library is an error.

Gradient clipping and the non-finite guard.  clip_grad_norm_ below is torch.nn.utils.clip_grad_norm_ on apg_grad_norm + apg_grad_scale (csrc/guard/grad_guard.hip);
FusedAdam(max_grad_norm=, skip_nonfinite=) takes the same norm (one read of the gradients, fp64 accumulation) and hands the clip
coefficient and the skip flag to apg_adam_step_guarded on the device: no second pass over the gradients and no host synchronisation.
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


def _grad_tables(grads, what):
    """HOST tables of apg_grad_norm / apg_grad_scale for a list of gradients, each refused by name unless it is a dense contiguous
    float32 CUDA tensor on the one device -> (device, n, pointer table, numel table)"""
    dev = None
    for g in grads:
        if not torch.is_tensor(g):
            raise TypeError("%s: gradients must be tensors, got %s" % (what, type(g).__name__))
        if g.is_sparse or g.layout is not torch.strided:
            raise ValueError("%s: a gradient of shape %s is sparse; sparse gradients are not supported" % (what, tuple(g.shape)))
        if not g.is_cuda:
            raise ValueError("%s: a gradient of shape %s lives on %s; the norm is a GPU kernel and there is no CPU fallback" %
                             (what, tuple(g.shape), g.device))
        if g.dtype != torch.float32:
            raise TypeError("%s: a gradient of shape %s is %s; only float32 gradients are supported" % (what, tuple(g.shape), g.dtype))
        if not g.is_contiguous():
            raise ValueError("%s: a gradient of shape %s and strides %s is not contiguous" % (what, tuple(g.shape), tuple(g.stride())))
        if dev is None:
            dev = g.device
        elif g.device != dev:
            raise ValueError("%s: gradients on %s and on %s; gradients on more than one device are not supported" % (what, dev, g.device))
    n = len(grads)
    return dev, n, (ctypes.c_void_p * n)(*[g.data_ptr() or None for g in grads]), (ctypes.c_int64 * n)(*[g.numel() for g in grads])


def _check_max_norm(what, max_norm):
    if torch.is_tensor(max_norm) or isinstance(max_norm, bool):
        raise TypeError("%s: max_norm must be a Python number, not %s" % (what, type(max_norm).__name__))
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError("%s: max_norm must be >= 0, got %r" % (what, max_norm))
    return max_norm


class _Guard(object):
    """the device tensors a norm needs: the workspace (grown on demand), the 16-byte guard record and, for an optimizer that keeps
    them between steps, the two counters.  Only the counters are initialised: apg_grad_norm writes the rest before anything reads it"""

    def __init__(self, dev, counters):
        self.dev = dev
        self.record = torch.empty(G.GUARD_BYTES // 4, dtype=torch.float32, device=dev)       # coef, norm, skip (int32), reserved
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev) if counters else None  # steps seen, steps skipped
        self.workspace = torch.empty(0, dtype=torch.float64, device=dev)

    def norm(self, L, n, gtab, numel, max_norm, skip_nonfinite):
        need = L.apg_grad_norm_workspace_bytes(n, numel)
        if need < 0:
            raise RuntimeError("airpose_grad apg_grad_norm_workspace_bytes refused the list")
        if self.workspace.numel() * 8 < need:
            self.workspace = torch.empty(need // 8, dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = L.apg_grad_norm(n, gtab, numel, max_norm, int(bool(skip_nonfinite)), self.workspace.data_ptr() or None,
                                 self.workspace.numel() * 8, self.record.data_ptr(), None, None if self.counters is None else self.counters.data_ptr(),
                                 G.stream(self.dev))
        G.check(rc, "apg_grad_norm")


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ for dense contiguous float32 CUDA gradients on one device: one apg_grad_norm and one
    apg_grad_scale on the current stream, nothing else.  Returns the total norm as a 0-d float32 tensor on the gradients' device; the
    gradients are multiplied in place by min(1, max_norm / (norm + 1e-6)), and not stored at all where that is 1.  The sum of squares is
    accumulated in fp64, so the norm neither overflows nor flushes where torch's fp32 one does.  Parameters without .grad are left
    out; an empty list returns a zero.  norm_type other than 2 is refused.  error_if_nonfinite=True raises torch's RuntimeError for a
    NaN or Inf norm (before the gradients are touched) and is the only path that synchronises the host.  Every call takes its 16-byte
    record and its workspace (8 bytes per 4096-element chunk and per tensor) from torch's caching allocator, two allocations per call and
    no kernel; the returned norm is a view of that record, so it stays valid.  FusedAdam(max_grad_norm=) keeps both between steps.  With a non-finite norm and
    error_if_nonfinite=False every gradient becomes NaN (include/airpose_grad.h: coef)."""
    what = "clip_grad_norm_"
    if torch.is_tensor(parameters):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise ValueError("%s: norm_type=%r is not supported; only the L2 norm (norm_type=2) is" % (what, norm_type))
    max_norm = _check_max_norm(what, max_norm)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev, n, gtab, numel = _grad_tables(grads, what)
    L = G.lib()
    guard = _Guard(dev, counters=False)                                   # fresh per call: the returned norm is a view of its record
    guard.norm(L, n, gtab, numel, max_norm, False)
    total = guard.record[1]
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError("The total norm of order %s for gradients from `parameters` is non-finite, so it cannot be clipped. To disable "
                           "this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`" % (float(norm_type),))
    with torch.cuda.device(dev):
        rc = L.apg_grad_scale(n, gtab, numel, guard.record.data_ptr(), G.stream(dev))
    G.check(rc, "apg_grad_scale")
    return total


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad) with the whole update of a param group in one apg_adam_step call.

    maximize, capturable, differentiable, foreach and fused are not accepted.  Parameters must be contiguous float32 CUDA tensors with
    dense contiguous gradients.  step() runs under no_grad on the current stream of the parameters' device and never synchronises the
    host; a parameter whose .grad is None is left out: its state stays untouched and its step count does not advance.

    max_grad_norm (None, or a number >= 0) and skip_nonfinite are attributes of the optimizer, not param-group keys: state_dict() has
    torch.optim.Adam's layout with or without them, and a loaded state_dict leaves them as they are.  With both at their defaults step()
    is the plain path.  Otherwise one apg_grad_norm takes the global L2 norm over the gradients of ALL groups (fp64 accumulation, one
    read), and each group's apg_adam_step_guarded multiplies its gradients by min(1, max_grad_norm / (norm + 1e-6)) on the way in: what
    torch.nn.utils.clip_grad_norm_ followed by step() computes, except that .grad is never rewritten.  All groups must then live on one
    device.  grad_norm is the 0-d device tensor of the last step's norm (a view the next step overwrites; reading it is the reader's
    synchronisation, step() never synchronises).  With skip_nonfinite=True a step whose gradients hold a NaN or an Inf changes no
    parameter and no moment; skipped_steps() copies the device's count out (one synchronisation: call it when you log).  With
    skip_nonfinite=False such a step turns every parameter it updates into NaN, as torch's does to the run.

    Step counts across a skip: the decision to skip is taken on the device and the host never learns of it, so state["step"] -- a host
    count -- advances on a skipped step too.  Each skip therefore puts the bias correction one step ahead of the moments: the
    correction factors 1 / (1 - beta^t) are taken at t + k after k skips.  They tend to 1, so the effect is a slightly smaller update
    during the first steps (at step 10 and one skip: 3 % in the first moment's factor, 5 % in the second's root) and nothing measurable
    after a few hundred; it is reported, not hidden: skipped_steps() is the k."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None,
                 skip_nonfinite=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), **_INERT)
        _check_options(defaults)
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm("FusedAdam", max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        super().__init__(params, defaults)
        G.lib()                                                           # a missing library is an error here, not at the first step

    @property
    def grad_norm(self):
        """the global gradient norm of the last guarded step: a 0-d float32 device tensor, None before the first such step"""
        guard = self.__dict__.get("_guard")
        return None if guard is None else guard.record[1]

    def skipped_steps(self):
        """how many steps the device skipped for a non-finite gradient; copies one int64 to the host (a synchronisation)"""
        guard = self.__dict__.get("_guard")
        return 0 if guard is None else int(guard.counters[1])

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

    def __getstate__(self):
        state = super().__getstate__()                                    # torch keeps defaults, state and param_groups only
        state.update(max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("skip_nonfinite", False)
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

    def _prepare(self, cache, gi, group):
        """one group's tables for this step (None when no parameter of it has a gradient): everything is checked here, before any step
        count moves and before any launch, so a refused step changes nothing"""
        f32, strided = torch.float32, torch.strided
        _check_options(group)
        amsgrad = bool(group["amsgrad"])
        plist, glist = [], []
        for p in group["params"]:
            g = p.grad
            if g is not None:
                plist.append(p)
                glist.append(g)
        if not plist:
            return None
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
        e["G"] = (ctypes.c_void_p * e["n"])(*gp)
        return e

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = G.lib()
        cache = self.__dict__.setdefault("_fused_tables", {})
        guarded = self.max_grad_norm is not None or self.skip_nonfinite
        record = None
        if guarded:
            # the global norm over every group's gradients, then one guarded step per group: all groups are checked first
            ready = [(group, self._prepare(cache, gi, group)) for gi, group in enumerate(self.param_groups)]
            ready = [(group, e) for group, e in ready if e is not None]
            if not ready:
                return loss
            dev = ready[0][1]["dev"]
            for _, e in ready:
                if e["dev"] != dev:
                    raise ValueError("FusedAdam: max_grad_norm / skip_nonfinite take one norm over all param groups, but the groups live on "
                                     "%s and on %s" % (dev, e["dev"]))
            guard = self.__dict__.get("_guard")
            if guard is None or guard.dev != dev:
                guard = self.__dict__["_guard"] = _Guard(dev, counters=True)
            n = sum(e["n"] for _, e in ready)
            gtab = (ctypes.c_void_p * n)(*[x for _, e in ready for x in e["G"]])
            numel = (ctypes.c_int64 * n)(*[x for _, e in ready for x in e["numel"]])
            max_norm = float("inf") if self.max_grad_norm is None else _check_max_norm("FusedAdam", self.max_grad_norm)
            guard.norm(L, n, gtab, numel, max_norm, self.skip_nonfinite)
            record = ctypes.c_void_p(guard.record.data_ptr())
        else:
            ready = ((group, self._prepare(cache, gi, group)) for gi, group in enumerate(self.param_groups))
        for group, e in ready:
            if e is None:
                continue
            n, dev = e["n"], e["dev"]
            counts = e["counts"]                                              # numpy view of the buffer behind every state["step"]
            counts += 1
            e["step"][:] = counts.astype("int64").tolist()
            beta1, beta2 = group["betas"]
            args = (n, e["P"], e["G"], e["M"], e["V"], e["X"], e["numel"], e["step"], float(group["lr"]), float(beta1), float(beta2),
                    float(group["eps"]), float(group["weight_decay"]))
            with torch.cuda.device(dev):
                if record is None:
                    rc = L.apg_adam_step(*args, G.stream(dev))
                else:
                    rc = L.apg_adam_step_guarded(*args, record, G.stream(dev))
            G.check(rc, "apg_adam_step" if record is None else "apg_adam_step_guarded")
        return loss
