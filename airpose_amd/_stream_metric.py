"""What EvalMetrics (eval_metrics.py) and MeshMetrics (mesh_metrics.py) share: a metric that adds fp64 sums on the device over a stream
of (output, batch) dicts and moves nothing to the host until compute().  The kinds, the tensor rule (Renderer uses it too), the
classes' base and the evaluate loop.
"""
import torch

from . import _args as A

KINDS = ("twoview", "singleview", "hmr", "muhmr")
VIEWS = {"twoview": 2, "singleview": 1, "hmr": 1, "muhmr": 2}


def check_what(owner, t, shape, name):
    """what a tensor must be, wherever it lives: a tensor, of `shape`, floating point; anything else is refused by name, in owner's
    name.  shape: a tuple, or the owner's own rule: a function of the tensor's shape -> what it should have been, None where it fits"""
    A.is_tensor(owner, t, name)
    want = shape(tuple(t.shape)) if callable(shape) else (None if tuple(t.shape) == tuple(shape) else tuple(shape))
    if want is not None:
        raise RuntimeError("%s: %s must be %s, got %s" % (owner, name, want, tuple(t.shape)))
    if not t.is_floating_point():
        raise RuntimeError("%s: %s must be a floating-point tensor, got %s" % (owner, name, t.dtype))


def check_where(owner, t, dev, name, anchor):
    """where a tensor must live: on the GPU, on dev (None: any CUDA device), which is where `anchor` ("the metrics") lives
    -> fp32, detached, contiguous"""
    A.lives_on(owner, t, dev, name, anchor)
    if t.dtype != torch.float32:
        t = t.float()
    return t.detach().contiguous()


def place(owner, entries, dev, anchor="the metrics"):
    """entries: (tensor, shape, name) or None each -> the tensors as check_where leaves them (None stays None).  What EVERY tensor
    must be is checked first, then where each must live"""
    for e in entries:
        if e is not None:
            check_what(owner, *e)
    return [None if e is None else check_where(owner, e[0], dev, e[2], anchor) for e in entries]


class StreamMetric(object):
    """The base of a metric class.  A subclass gives NAME (for the messages), ACC_SHAPE (of its fp64 sums, (2, ...): the C
    accumulator's layout), STATE (the entries of its state beside kind and acc: attribute name -> the words of the refusal, for
    (the state's value, this object's)), summarise(acc, views) and _configure(...) for the constructor arguments of its own; its update
    takes the device buffers from _buffers()."""
    NAME, ACC_SHAPE, STATE = None, None, {}

    def __init__(self, kind, device, per_sample, *own):
        if kind not in KINDS:
            raise ValueError("%s: kind must be one of %s, got %r" % (self.NAME, ", ".join(KINDS), kind))
        self.kind, self.views, self.per_sample = kind, VIEWS[kind], bool(per_sample)
        self._configure(*own)                                    # (between the two: a call with two mistakes hears of the same one)
        self.device = A.cuda_device(self.NAME, device)
        self._acc = self._ws = None
        self.reset()

    # ---------------------------------------------------------------------------------------- the dict
    def _lookup(self, output, batch):
        """-> find(keys): the first (key, value) of `keys` in output, then in batch, whose value is not None, or None;
        need(keys, what): the same, a miss refused by name"""
        def find(keys):
            for src in (output, batch):
                for k in keys:
                    if src is not None and k in src and src[k] is not None:
                        return k, src[k]
            return None

        def need(keys, what):
            hit = find(keys)
            if hit is None:
                raise RuntimeError("%s(%s): neither output nor batch has %s (%s)" % (self.NAME, self.kind, " / ".join(keys), what))
            return hit
        return find, need

    def _batch_size(self, hit):
        """B of the (key, tensor) that leads an update"""
        if not torch.is_tensor(hit[1]) or hit[1].dim() < 1:
            raise RuntimeError("%s: %s must be a tensor with a batch dimension" % (self.NAME, hit[0]))
        return hit[1].shape[0]

    # ---------------------------------------------------------------------------------------- the sums
    def _buffers(self, nbytes):
        """(the sums, a workspace of at least nbytes) on the device; call under torch.cuda.device(self.device).  The sums move
        there at first use; the workspace grows and never shrinks"""
        if self._acc is None:
            self._acc = self._host.to(self.device)
        if self._ws is None or self._ws.numel() * 8 < nbytes:
            self._ws = torch.empty((nbytes + 7) // 8, device=self.device, dtype=torch.float64)
        return self._acc, self._ws

    def reset(self):
        self._host = torch.zeros(self.ACC_SHAPE, dtype=torch.float64)     # the sums while they are not on the device
        if self._acc is not None:
            self._acc.zero_()

    def state(self):
        """{"kind", the STATE entries, "acc": ACC_SHAPE float64 host tensor: the raw sums and counts}; one host synchronisation"""
        acc = self._acc.cpu() if self._acc is not None else self._host.clone()
        return dict([("kind", self.kind)] + [(k, getattr(self, k)) for k in self.STATE] + [("acc", acc)])

    def load_state(self, state):
        acc = torch.as_tensor(state["acc"])
        if state.get("kind", self.kind) != self.kind:
            raise RuntimeError("%s: the state is of kind %r, this object of kind %r" % (self.NAME, state.get("kind"), self.kind))
        for k, words in self.STATE.items():
            if state.get(k, getattr(self, k)) != getattr(self, k):
                raise RuntimeError("%s: %s" % (self.NAME, words % (state.get(k), getattr(self, k))))
        if tuple(acc.shape) != self.ACC_SHAPE or acc.dtype != torch.float64:
            raise RuntimeError("%s: state['acc'] must be %s float64, got %s %s" % (self.NAME, self.ACC_SHAPE, tuple(acc.shape), acc.dtype))
        self._host = acc.detach().cpu().clone()
        if self._acc is not None:
            self._acc.copy_(self._host)

    def compute(self):
        return self.summarise(self.state()["acc"], self.views)


def evaluate(pipe, batches, metrics_list):
    """Score a stream of batches behind TwoViewInference.submit with several metric objects over ONE submit stream, so that
    EvalMetrics and MeshMetrics score the same pass: for each batch, submit(batch, want_angles=True), make the current stream wait
    for the Pending and update every object with (its outputs, the batch); the host synchronises in the compute() calls after the
    last batch (and where submit itself does when more than its DEPTH batches are in flight).  `batches` yields dicts with submit's
    inputs and the ground truth on the GPU.  -> the list of the objects' compute() dicts"""
    metrics_list = list(metrics_list)
    for batch in batches:
        pend = pipe.submit(batch, want_angles=True)
        out = pend.wait(torch.cuda.current_stream(metrics_list[0].device))
        for m in metrics_list:
            m.update(out, batch)
    return [m.compute() for m in metrics_list]
