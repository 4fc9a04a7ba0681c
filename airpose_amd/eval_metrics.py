"""The reference trainers' test_epoch_end as one hand-written gfx950 pass per batch: EvalMetrics.

test_epoch_end of copenet_twoview.py:539-601, copenet_singleview.py:394-432, muhmr.py:463-517 and hmr.py:365-386 (repeated by
copenet_real/scripts/*_res_compile.py) is the only thing in the reference that yields the paper's accuracy numbers.  It collects
every test_step output dict, moves it to the host, turns pred_angles into matrices with tgm.angle_axis_to_rotation_matrix, calls
SMPLX.forward four times per batch (ground truth and prediction, two views; betas = 0), reads 22 joints of each and averages in
numpy:
    mpjpe = mean over samples x 22 joints of |joints_pred - joints_gt|_2          (metres)
    mpe   = mean over samples of |pred_smpltrans - gt_smpltrans|_2
    hmr:    mean over samples x 22 of |pred_angles - gt_angles|_2
With betas = 0 those joints depend on the 22 rotations and the rest joints J_regressor v_template alone, so apg_eval_update
(csrc/eval_metrics.hip, include/airpose_grad.h) does the conversion, the four 22-joint chains, the distances and a fixed-order fp64
reduction on the device: two launches per batch, no vertex, nothing moved to the host until compute().  There is no fallback: a
missing library is an error.

torchgeometry is absent here, so the parity of the angle-axis conversion with tgm 0.1.2 is UNPINNED; the
formula is restated from its published source.

The reference's print labels mix its two loaders: copenet_twoview.py:596 prints the TRAIN loader's view-0 translation error as
"test_mpe1", and the view-1 errors it computed are never printed.  That is not reproduced: here index 0 / 1 is always the view, and
one EvalMetrics scores one stream of batches (use two objects for two loaders).
"""
import torch

from . import _native_grad as G
from . import _stream_metric as S
from ._stream_metric import KINDS  # noqa: F401  (importable from here as before)

NJ = 22
ANGLE_AXIS, ROTMAT = 0, 1                # include/airpose_grad.h: APG_EVAL_ANGLE_AXIS, APG_EVAL_ROTMAT
PER_VIEW = 5                             # APG_EVAL_PER_VIEW: gt_orient, pred_rot, gt_trans, pred_trans, gt_angles
ACC = 28                                 # APG_EVAL_ACC_PER_VIEW
# one view's accumulator (include/airpose_grad.h)
A_COUNT, A_JOINT, A_PER_JOINT, A_TRANS, A_ANGLE, A_NTRANS, A_NANGLE = 0, 1, 2, 24, 25, 26, 27


def rest_joints(model):
    """(j_rest (22, 3) float32, parents: 22 ints) of an airpose_amd.SMPLX or of a model dict (airpose_amd.smplx_model)"""
    md = getattr(model, "_md", model)
    try:
        J, v, par = md["J_regressor"], md["v_template"], md["parents"]
    except (KeyError, TypeError, IndexError):
        raise RuntimeError("EvalMetrics: needs an airpose_amd.SMPLX or a model dict with J_regressor, v_template and parents")
    j = (torch.as_tensor(J).double() @ torch.as_tensor(v).double())[:NJ]
    if j.shape != (NJ, 3):
        raise RuntimeError("EvalMetrics: J_regressor @ v_template must have at least 22 rows of 3, got %s" % (tuple(j.shape),))
    parents = [int(x) for x in list(par)[:NJ]]
    parents[0] = -1                      # (some model files store the root's parent as 2^32 - 1)
    if len(parents) != NJ or any(not 0 <= p < k for k, p in enumerate(parents) if k):
        raise RuntimeError("EvalMetrics: parents[j] must lie in 0 .. j - 1 for the 22 body joints, got %s" % (parents,))
    return j.float().contiguous(), parents


class EvalMetrics(S.StreamMetric):
    """MPJPE, MPE and the angle-axis error of a stream of test_step output dicts, on libairpose_grad.so.

    EvalMetrics(smplx_or_model_dict, kind="twoview" | "singleview" | "hmr" | "muhmr", device=None, per_sample=False)

    update(output, batch=None) takes the reference's test_step output dict key for key.  Each key is looked up in `output` first and
    then in `batch` (our TwoViewInference does not echo the ground truth):
      two views (twoview, muhmr)   pred_angles0/1 (B, 22, 3)  or  pred_rotmat0/1 (B, 22, 3, 3)      required
                                   smplorient_rel0/1 (B, 1, 3, 3), smplpose_rotmat (B, 21, 3, 3)   required
                                   pred_smpltrans0/1 with gt_smpltrans0/1 (B, 3)                   optional, as a pair -> mpe
                                   gt_angles0/1 (B, 22, 3), with pred_angles only                  optional -> angle_err
      one view (singleview, hmr)   the same names without the index (smplorient_rel or smplorient_rel0: the single-view trainer
                                   writes the second and reads the first)
    gt_smpltrans* falls back to the batch's smpltrans_rel* (what the trainers copy it from).  A prediction whose ground truth is
    missing, a CPU tensor, a tensor on another device, a wrong shape and a non-floating dtype are refused by name.
    update runs on the current stream and never synchronises the host; with per_sample=True it returns (joint_err (views, B, 22),
    trans_err (views, B) or None, angle_err (views, B, 22) or None).

    compute() synchronises once and returns Python floats and lists: count, mpjpe0 / mpjpe1 (metres, mean over samples x 22),
    per_joint0 / per_joint1 (22 entries), mpe0 / mpe1 and angle_err0 / angle_err1 where they were fed (single-view kinds carry index
    0 only).  reset() clears the sums.  state() / load_state() expose the raw fp64 sums and counts ((2, 28), the accumulator layout
    of include/airpose_grad.h) so that ranks or shards can add them; no collective is part of this class.
    """

    NAME, ACC_SHAPE = "EvalMetrics", (2, ACC)

    def __init__(self, model, kind="twoview", device=None, per_sample=False):
        S.StreamMetric.__init__(self, kind, device, per_sample, model)

    def _configure(self, model):
        self._j_host, self.parents = rest_joints(model)
        self._j = None
        self._cparents = G.ints(self.parents)

    # ---------------------------------------------------------------------------------------- the dict
    def _names(self, v):
        """the key candidates of view v, in lookup order"""
        sfx = [str(v)] if self.views == 2 else ["", "0"]
        return {"pred_angles": ["pred_angles" + s for s in sfx], "pred_rotmat": ["pred_rotmat" + s for s in sfx],
                "gt_orient": ["smplorient_rel" + s for s in sfx], "pred_trans": ["pred_smpltrans" + s for s in sfx],
                "gt_trans": ["gt_smpltrans" + s for s in sfx] + ["smpltrans_rel" + (s or "0") for s in sfx],
                "gt_angles": ["gt_angles" + s for s in sfx]}

    def gather(self, output, batch=None):
        """-> (mode, gt_body, per view a dict gt_orient / pred_rot / gt_trans / pred_trans / gt_angles of (key, tensor) or None):
        which entries of output / batch an update would read.  Refuses a missing required key and a translation without its
        ground truth, by name; looks at no tensor."""
        find, need = self._lookup(output, batch)
        body = need(["smplpose_rotmat"], "the ground-truth body pose")
        views, mode = [], None
        for v in range(self.views):
            n = self._names(v)
            pred = find(n["pred_angles"])
            m = ANGLE_AXIS
            if pred is None:
                pred, m = find(n["pred_rotmat"]), ROTMAT
                if pred is None:
                    raise RuntimeError("EvalMetrics(%s): neither output nor batch has %s or %s" % (
                        self.kind, " / ".join(n["pred_angles"]), " / ".join(n["pred_rotmat"])))
            if mode is not None and m != mode:
                raise RuntimeError("EvalMetrics(%s): %s is given where view 0 gave the other of pred_angles / pred_rotmat" % (self.kind, pred[0]))
            mode = m
            d = {"gt_orient": need(n["gt_orient"], "the ground-truth global orientation"), "pred_rot": pred,
                 "pred_trans": find(n["pred_trans"]), "gt_trans": None, "gt_angles": None}
            if d["pred_trans"] is not None:
                d["gt_trans"] = find(n["gt_trans"])
                if d["gt_trans"] is None:
                    raise RuntimeError("EvalMetrics(%s): %s is given without %s" % (self.kind, d["pred_trans"][0], " / ".join(n["gt_trans"])))
            if mode == ANGLE_AXIS:
                d["gt_angles"] = find(n["gt_angles"])
            views.append(d)
        return mode, body, views

    # ---------------------------------------------------------------------------------------- the sums
    def update(self, output, batch=None):
        mode, body, views = self.gather(output, batch)
        dev = self.device
        B = self._batch_size(views[0]["pred_rot"])
        shapes = {"gt_orient": (B, 1, 3, 3), "pred_rot": (B, NJ, 3) if mode == ANGLE_AXIS else (B, NJ, 3, 3), "gt_trans": (B, 3),
                  "pred_trans": (B, 3), "gt_angles": (B, NJ, 3)}
        order = ("gt_orient", "pred_rot", "gt_trans", "pred_trans", "gt_angles")
        entries = [None if d[n] is None else (d[n][1], shapes[n], d[n][0]) for d in views for n in order] + [(body[1], (B, 21, 3, 3), body[0])]
        table = S.place(self.NAME, entries, dev)
        gt_body = table.pop()
        has_trans = all(d["pred_trans"] is not None for d in views)
        has_angles = all(d["gt_angles"] is not None for d in views)
        L = G.lib()
        with torch.cuda.device(dev):
            if self._j is None:
                self._j = self._j_host.to(dev)
            acc, ws = self._buffers(L.apg_eval_workspace_bytes(B, self.views))
            je = te = ae = None
            if self.per_sample:
                je = torch.empty(self.views, B, NJ, device=dev, dtype=torch.float32)
                te = torch.empty(self.views, B, device=dev, dtype=torch.float32) if has_trans else None
                ae = torch.empty(self.views, B, NJ, device=dev, dtype=torch.float32) if has_angles else None
            vp = G.vp
            G.check(L.apg_eval_update(B, self.views, mode, vp(self._j), self._cparents, G.ptrs(table), vp(gt_body), vp(je), vp(te),
                                      vp(ae), vp(acc), vp(ws), ws.numel() * 8, G.stream(dev)), "apg_eval_update")
        return (je, te, ae) if self.per_sample else None

    summarise = staticmethod(lambda acc, views: summarise(acc, views))


def summarise(acc, views):
    """the metrics dict from the raw sums ((2, 28) float64, host)"""
    acc = acc.tolist()
    out = {"count": int(acc[0][A_COUNT])}
    for v in range(views):
        a = acc[v]
        n = a[A_COUNT]
        out["mpjpe%d" % v] = a[A_JOINT] / (n * NJ) if n else float("nan")
        out["per_joint%d" % v] = [x / n if n else float("nan") for x in a[A_PER_JOINT:A_PER_JOINT + NJ]]
        if a[A_NTRANS]:
            out["mpe%d" % v] = a[A_TRANS] / a[A_NTRANS]
        if a[A_NANGLE]:
            out["angle_err%d" % v] = a[A_ANGLE] / (a[A_NANGLE] * NJ)
    return out


def evaluate(pipe, batches, metrics):
    """Score a stream of batches behind TwoViewInference.submit with ONE metric object (_stream_metric.evaluate's loop) -> its
    compute() dict.  `batches` yields dicts with submit's inputs and the ground truth (smplorient_rel0/1, smplpose_rotmat, optionally
    smpltrans_rel0/1) on the GPU."""
    return S.evaluate(pipe, batches, [metrics])[0]
