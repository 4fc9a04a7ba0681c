"""The numbers mesh-recovery papers tabulate, as two hand-written gfx950 passes per batch: MeshMetrics.

EvalMetrics reproduces the reference's test_epoch_end (MPJPE on a betas = 0 skeleton, MPE, angle error); the reference computes
neither a vertex error nor a Procrustes-aligned one.  MeshMetrics compares what TwoViewInference emits (pred_j3d_cam*,
pred_vertices_cam*, the real predicted mesh with the predicted betas) with what the batch carries (smpl_joints_rel*,
smpl_vertices_rel*), in metres:
    mpjpe_abs / pve_abs     mean over samples of mean_i |p_i - q_i|
    mpjpe_root / pve_root   the same after moving joint 0 of each joint set to the origin (the vertices use the joints' roots)
    pa_mpjpe / pa_pve       the same after the least-squares similarity (s, R, t) of the prediction onto the ground truth, det R = +1
apg_align_update (csrc/eval_align.hip, include/airpose_grad.h) takes the moments and solves the 3 x 3 problem in fp64 on the
device and reduces in a fixed order: two calls of two launches per batch (joints, vertices), no torch.linalg.svd, nothing moved to
the host until compute().  There is no fallback: a missing library is an error.
"""
import ctypes

import torch

from . import _native_grad as G
from .eval_metrics import KINDS, _VIEWS

ACC = 5                                  # include/airpose_grad.h: APG_ALIGN_ACC_PER_VIEW
A_COUNT, A_ABS, A_ROOT, A_PA, A_NROOT = range(5)
SETS = ("joints", "vertices")
_LABELS = (("mpjpe_abs", "mpjpe_root", "pa_mpjpe"), ("pve_abs", "pve_root", "pa_pve"))


def _points(t, dev, B, n_min, n_exact, name):
    """(B, n, 3) or (B, 1, n, 3) floating tensor with n >= n_min (n == n_exact if given) -> fp32 contiguous (B, n, 3) on dev;
    anything else is refused by name (EvalMetrics' rules).  dev = None: shape and dtype only"""
    if not torch.is_tensor(t):
        raise RuntimeError("MeshMetrics: %s must be a tensor, got %s" % (name, type(t).__name__))
    shape = tuple(t.shape)
    if len(shape) == 4 and shape[1] == 1:
        shape = (shape[0],) + shape[2:]
    want = "(%d, %s, 3)" % (B, ("%d" % n_exact) if n_exact is not None else ("at least %d" % n_min))
    if len(shape) != 3 or shape[0] != B or shape[2] != 3 or shape[1] < n_min or (n_exact is not None and shape[1] != n_exact):
        raise RuntimeError("MeshMetrics: %s must be %s, got %s" % (name, want, tuple(t.shape)))
    if not t.is_floating_point():
        raise RuntimeError("MeshMetrics: %s must be a floating-point tensor, got %s" % (name, t.dtype))
    if dev is None:
        return t
    if not t.is_cuda:
        raise RuntimeError("MeshMetrics: %s lives on %s; it must be a CUDA (ROCm) tensor, there is no CPU path" % (name, t.device))
    if t.device != dev:
        raise RuntimeError("MeshMetrics: %s lives on %s, the metrics on %s" % (name, t.device, dev))
    if t.dtype != torch.float32:
        t = t.float()
    return t.detach().reshape(shape).contiguous()


class MeshMetrics(object):
    """MPJPE and PVE, absolute, root-aligned and Procrustes-aligned, of a stream of inference outputs, on libairpose_grad.so.

    MeshMetrics(kind="twoview" | "singleview" | "hmr" | "muhmr", n_joints=22, device=None, per_sample=False)

    update(output, batch=None): each key is looked up in `output` first and then in `batch`.  Per view v (two-view kinds: the
    names with 0 / 1; one-view kinds: the names without the index or with 0):
      pred_j3d_cam{v} (B, J >= n_joints, 3) with smpl_joints_rel{v} (B, J' >= n_joints, 3) or (B, 1, J', 3)     required: the
                                                                                      first n_joints are compared, joint 0 is the root
      pred_vertices_cam{v} (B, V, 3) with smpl_vertices_rel{v} (B, V, 3) or (B, 1, V, 3)      optional, as a pair, for every view or none
    A missing key, a CPU tensor, a tensor on another device, a wrong shape and a non-floating dtype are refused by name.  update
    runs on the current stream and never synchronises the host; with per_sample=True it returns (joint_err (views, B, 3) = abs,
    root, pa per sample, vertex_err the same or None, transform (views, B, 13) = s, R row-major, t of the joint sets).

    compute() synchronises once and returns Python floats: count and, per view, mpjpe_abs{v}, mpjpe_root{v}, pa_mpjpe{v} and, where
    vertices were fed, pve_abs{v}, pve_root{v}, pa_pve{v}, in metres (single-view kinds carry index 0 only).  reset() clears the sums.
    state() / load_state() expose the raw fp64 sums and counts ((2, 2, 5): point set, view, the accumulator layout of
    include/airpose_grad.h) so that ranks or shards can add them; no collective is part of this class.
    """

    def __init__(self, kind="twoview", n_joints=22, device=None, per_sample=False):
        if kind not in KINDS:
            raise ValueError("MeshMetrics: kind must be one of %s, got %r" % (", ".join(KINDS), kind))
        if int(n_joints) != n_joints or n_joints < 1:
            raise ValueError("MeshMetrics: n_joints must be a positive integer, got %r" % (n_joints,))
        self.kind, self.views, self.n_joints, self.per_sample = kind, _VIEWS[kind], int(n_joints), bool(per_sample)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()
                                                                                   if torch.cuda.is_available() else 0)
        if self.device.type != "cuda":
            raise RuntimeError("MeshMetrics: device must be a CUDA (ROCm) device, got %s; there is no CPU path" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._host = torch.zeros(2, 2, ACC, dtype=torch.float64)  # the sums while they are not on the device
        self._acc = self._ws = None

    # ---------------------------------------------------------------------------------------- the dict
    def _names(self, v):
        sfx = [str(v)] if self.views == 2 else ["", "0"]
        return {"pred_joints": ["pred_j3d_cam" + s for s in sfx], "gt_joints": ["smpl_joints_rel" + s for s in sfx],
                "pred_vertices": ["pred_vertices_cam" + s for s in sfx], "gt_vertices": ["smpl_vertices_rel" + s for s in sfx]}

    def gather(self, output, batch=None):
        """-> per view a dict pred_joints / gt_joints / pred_vertices / gt_vertices of (key, tensor) or None: which entries of
        output / batch an update would read.  Refuses a missing joint key and a vertex pair given by half (within a view or
        across the views), by name; looks at no tensor."""
        def find(keys):
            for src in (output, batch):
                if src is None:
                    continue
                for k in keys:
                    if k in src and src[k] is not None:
                        return k, src[k]
            return None
        views = []
        for v in range(self.views):
            n = self._names(v)
            d = {k: find(n[k]) for k in n}
            for k, what in (("pred_joints", "the predicted joints"), ("gt_joints", "the ground-truth joints")):
                if d[k] is None:
                    raise RuntimeError("MeshMetrics(%s): neither output nor batch has %s (%s)" % (self.kind, " / ".join(n[k]), what))
            for k, o in (("pred_vertices", "gt_vertices"), ("gt_vertices", "pred_vertices")):
                if d[k] is not None and d[o] is None:
                    raise RuntimeError("MeshMetrics(%s): %s is given without %s" % (self.kind, d[k][0], " / ".join(n[o])))
            if views and (d["pred_vertices"] is None) != (views[0]["pred_vertices"] is None):
                have, miss = (d, 0) if d["pred_vertices"] is not None else (views[0], v)
                raise RuntimeError("MeshMetrics(%s): %s is given for one view only (%s is missing)" % (
                    self.kind, have["pred_vertices"][0], " / ".join(self._names(miss)["pred_vertices"])))
            views.append(d)
        return views

    # ---------------------------------------------------------------------------------------- the sums
    def update(self, output, batch=None):
        views = self.gather(output, batch)
        dev, nj = self.device, self.n_joints
        first = views[0]["pred_joints"][1]
        if not torch.is_tensor(first) or first.dim() < 1:
            raise RuntimeError("MeshMetrics: %s must be a tensor with a batch dimension" % views[0]["pred_joints"][0])
        B = first.shape[0]
        if B < 1:
            raise RuntimeError("MeshMetrics: %s holds no sample" % views[0]["pred_joints"][0])
        has_verts = views[0]["pred_vertices"] is not None
        V = None
        if has_verts:
            pv = views[0]["pred_vertices"][1]
            V = pv.shape[1] if torch.is_tensor(pv) and pv.dim() == 3 else None
        entries = []                                             # (tensor, n_min, n_exact, name)
        for d in views:
            entries += [(d["pred_joints"][1], nj, None, d["pred_joints"][0]), (d["gt_joints"][1], nj, None, d["gt_joints"][0])]
            if has_verts:
                entries += [(d["pred_vertices"][1], 1, V, d["pred_vertices"][0]), (d["gt_vertices"][1], 1, V, d["gt_vertices"][0])]
        for t, lo, ex, name in entries:                          # what every tensor must be first, then where it must live
            _points(t, None, B, lo, ex, name)
        ten = [_points(t, dev, B, lo, ex, name) for t, lo, ex, name in entries]
        step = 4 if has_verts else 2
        pj, gj = ten[0::step], ten[1::step]
        L = G.lib()
        with torch.cuda.device(dev):
            if self._acc is None:
                self._acc = self._host.to(dev)
            nbytes = L.apg_align_workspace_bytes(B, self.views, max(nj, V or 1))
            if nbytes < 0:
                raise RuntimeError("MeshMetrics: B = %d with %d points is outside apg_align_update's limits" % (B, max(nj, V or 1)))
            if self._ws is None or self._ws.numel() * 8 < nbytes:
                self._ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
            je = ve = tr = None
            if self.per_sample:
                je = torch.empty(self.views, B, 3, device=dev, dtype=torch.float32)
                tr = torch.empty(self.views, B, 13, device=dev, dtype=torch.float32)
                ve = torch.empty(self.views, B, 3, device=dev, dtype=torch.float32) if has_verts else None
            vp = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            sj, sg = pj[0].shape[1] * 3, gj[0].shape[1] * 3
            for v in range(1, self.views):                       # one stride serves both views
                if pj[v].shape[1] * 3 != sj or gj[v].shape[1] * 3 != sg:
                    raise RuntimeError("MeshMetrics: %s / %s hold another number of joints than view 0's" % (
                        views[v]["pred_joints"][0], views[v]["gt_joints"][0]))
            table = [t for v in range(self.views) for t in (pj[v], gj[v], pj[v], gj[v])]
            G.check(L.apg_align_update(B, self.views, nj, sj, sg, sj, sg, G.ptrs(table), vp(je), vp(tr), vp(self._acc[0]),
                                       vp(self._ws), self._ws.numel() * 8, stream), "apg_align_update (joints)")
            if has_verts:
                pvx, gvx = ten[2::step], ten[3::step]
                table = [t for v in range(self.views) for t in (pvx[v], gvx[v], pj[v], gj[v])]
                G.check(L.apg_align_update(B, self.views, V, 3 * V, 3 * V, sj, sg, G.ptrs(table), vp(ve), None, vp(self._acc[1]),
                                           vp(self._ws), self._ws.numel() * 8, stream), "apg_align_update (vertices)")
        return (je, ve, tr) if self.per_sample else None

    def reset(self):
        self._host = torch.zeros(2, 2, ACC, dtype=torch.float64)
        if self._acc is not None:
            self._acc.zero_()

    def state(self):
        """{"kind", "n_joints", "acc": (2, 2, 5) float64 host tensor: per point set and view the raw sums and counts}; one host
        synchronisation"""
        acc = self._acc.cpu() if self._acc is not None else self._host.clone()
        return {"kind": self.kind, "n_joints": self.n_joints, "acc": acc}

    def load_state(self, state):
        acc = torch.as_tensor(state["acc"])
        if state.get("kind", self.kind) != self.kind:
            raise RuntimeError("MeshMetrics: the state is of kind %r, this object of kind %r" % (state.get("kind"), self.kind))
        if state.get("n_joints", self.n_joints) != self.n_joints:
            raise RuntimeError("MeshMetrics: the state compares %r joints, this object %d" % (state.get("n_joints"), self.n_joints))
        if tuple(acc.shape) != (2, 2, ACC) or acc.dtype != torch.float64:
            raise RuntimeError("MeshMetrics: state['acc'] must be (2, 2, %d) float64, got %s %s" % (ACC, tuple(acc.shape), acc.dtype))
        self._host = acc.detach().cpu().clone()
        if self._acc is not None:
            self._acc.copy_(self._host)

    def compute(self):
        return summarise(self.state()["acc"], self.views)


def summarise(acc, views):
    """the metrics dict from the raw sums ((2, 2, 5) float64, host)"""
    acc = acc.tolist()
    out = {"count": int(acc[0][0][A_COUNT])}
    for k, labels in enumerate(_LABELS):
        for v in range(views):
            a = acc[k][v]
            n = a[A_COUNT]
            if k == 1 and not n:                                  # no vertices were fed
                continue
            out["%s%d" % (labels[0], v)] = a[A_ABS] / n if n else float("nan")
            out["%s%d" % (labels[1], v)] = a[A_ROOT] / a[A_NROOT] if a[A_NROOT] else float("nan")
            out["%s%d" % (labels[2], v)] = a[A_PA] / n if n else float("nan")
    return out


def evaluate(pipe, batches, metrics_list):
    """eval_metrics.evaluate's loop for several metric objects over ONE submit stream, so that EvalMetrics and MeshMetrics score the
    same pass: for each batch, submit(batch, want_angles=True), make the current stream wait for the Pending and update every
    object with (its outputs, the batch); the host synchronises in the compute() calls after the last batch (and where submit
    itself does when more than its DEPTH batches are in flight).  -> the list of the objects' compute() dicts"""
    metrics_list = list(metrics_list)
    for batch in batches:
        pend = pipe.submit(batch, want_angles=True)
        out = pend.wait(torch.cuda.current_stream(metrics_list[0].device))
        for m in metrics_list:
            m.update(out, batch)
    return [m.compute() for m in metrics_list]
