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
import torch

from . import _native_grad as G
from . import _stream_metric as S
from ._stream_metric import evaluate  # noqa: F401  (the loop over several metric objects: importable from here as before)

ACC = 5                                  # include/airpose_grad.h: APG_ALIGN_ACC_PER_VIEW
A_COUNT, A_ABS, A_ROOT, A_PA, A_NROOT = range(5)
SETS = ("joints", "vertices")
_LABELS = (("mpjpe_abs", "mpjpe_root", "pa_mpjpe"), ("pve_abs", "pve_root", "pa_pve"))


def _points(B, n_min, n_exact):
    """the shape rule of a point set (S.check_what): (B, n, 3) or (B, 1, n, 3) with n >= n_min (n == n_exact if given)"""
    def rule(shape):
        if len(shape) == 4 and shape[1] == 1:
            shape = (shape[0],) + shape[2:]
        if len(shape) != 3 or shape[0] != B or shape[2] != 3 or shape[1] < n_min or (n_exact is not None and shape[1] != n_exact):
            return "(%d, %s, 3)" % (B, ("%d" % n_exact) if n_exact is not None else ("at least %d" % n_min))
    return rule


class MeshMetrics(S.StreamMetric):
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

    NAME, ACC_SHAPE = "MeshMetrics", (2, 2, ACC)
    STATE = {"n_joints": "the state compares %r joints, this object %d"}

    def __init__(self, kind="twoview", n_joints=22, device=None, per_sample=False):
        S.StreamMetric.__init__(self, kind, device, per_sample, n_joints)

    def _configure(self, n_joints):
        if int(n_joints) != n_joints or n_joints < 1:
            raise ValueError("MeshMetrics: n_joints must be a positive integer, got %r" % (n_joints,))
        self.n_joints = int(n_joints)

    # ---------------------------------------------------------------------------------------- the dict
    def _names(self, v):
        sfx = [str(v)] if self.views == 2 else ["", "0"]
        return {"pred_joints": ["pred_j3d_cam" + s for s in sfx], "gt_joints": ["smpl_joints_rel" + s for s in sfx],
                "pred_vertices": ["pred_vertices_cam" + s for s in sfx], "gt_vertices": ["smpl_vertices_rel" + s for s in sfx]}

    def gather(self, output, batch=None):
        """-> per view a dict pred_joints / gt_joints / pred_vertices / gt_vertices of (key, tensor) or None: which entries of
        output / batch an update would read.  Refuses a missing joint key and a vertex pair given by half (within a view or
        across the views), by name; looks at no tensor."""
        find, need = self._lookup(output, batch)
        views = []
        for v in range(self.views):
            n = self._names(v)
            d = {"pred_joints": need(n["pred_joints"], "the predicted joints"), "gt_joints": need(n["gt_joints"], "the ground-truth joints"),
                 "pred_vertices": find(n["pred_vertices"]), "gt_vertices": find(n["gt_vertices"])}
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
        B = self._batch_size(views[0]["pred_joints"])
        if B < 1:
            raise RuntimeError("MeshMetrics: %s holds no sample" % views[0]["pred_joints"][0])
        has_verts = views[0]["pred_vertices"] is not None
        V = None
        if has_verts:
            pv = views[0]["pred_vertices"][1]
            V = pv.shape[1] if torch.is_tensor(pv) and pv.dim() == 3 else None
        joints, verts = _points(B, nj, None), _points(B, 1, V)
        entries = []                                             # (tensor, shape rule, name)
        for d in views:
            entries += [(d["pred_joints"][1], joints, d["pred_joints"][0]), (d["gt_joints"][1], joints, d["gt_joints"][0])]
            if has_verts:
                entries += [(d["pred_vertices"][1], verts, d["pred_vertices"][0]), (d["gt_vertices"][1], verts, d["gt_vertices"][0])]
        ten = [t.reshape(B, -1, 3) for t in S.place(self.NAME, entries, dev)]                # (B, 1, n, 3) -> (B, n, 3)
        step = 4 if has_verts else 2
        pj, gj = ten[0::step], ten[1::step]
        L = G.lib()
        with torch.cuda.device(dev):
            nbytes = L.apg_align_workspace_bytes(B, self.views, max(nj, V or 1))
            if nbytes < 0:
                raise RuntimeError("MeshMetrics: B = %d with %d points is outside apg_align_update's limits" % (B, max(nj, V or 1)))
            acc, ws = self._buffers(nbytes)
            je = ve = tr = None
            if self.per_sample:
                je = torch.empty(self.views, B, 3, device=dev, dtype=torch.float32)
                tr = torch.empty(self.views, B, 13, device=dev, dtype=torch.float32)
                ve = torch.empty(self.views, B, 3, device=dev, dtype=torch.float32) if has_verts else None
            vp, stream = G.vp, G.stream(dev)
            sj, sg = pj[0].shape[1] * 3, gj[0].shape[1] * 3
            for v in range(1, self.views):                       # one stride serves both views
                if pj[v].shape[1] * 3 != sj or gj[v].shape[1] * 3 != sg:
                    raise RuntimeError("MeshMetrics: %s / %s hold another number of joints than view 0's" % (
                        views[v]["pred_joints"][0], views[v]["gt_joints"][0]))
            table = [t for v in range(self.views) for t in (pj[v], gj[v], pj[v], gj[v])]
            G.check(L.apg_align_update(B, self.views, nj, sj, sg, sj, sg, G.ptrs(table), vp(je), vp(tr), vp(acc[0]),
                                       vp(ws), ws.numel() * 8, stream), "apg_align_update (joints)")
            if has_verts:
                pvx, gvx = ten[2::step], ten[3::step]
                table = [t for v in range(self.views) for t in (pvx[v], gvx[v], pj[v], gj[v])]
                G.check(L.apg_align_update(B, self.views, V, 3 * V, 3 * V, sj, sg, G.ptrs(table), vp(ve), None, vp(acc[1]),
                                           vp(ws), ws.numel() * 8, stream), "apg_align_update (vertices)")
        return (je, ve, tr) if self.per_sample else None

    summarise = staticmethod(lambda acc, views: summarise(acc, views))


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
