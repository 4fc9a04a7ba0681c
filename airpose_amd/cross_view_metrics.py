"""How well the two views of a calibrated pair agree on one body, as two hand-written gfx950 launches per batch: CrossViewMetrics.

EvalMetrics and MeshMetrics need 3-D ground truth; real footage has none.  What it has is two calibrated cameras (extr0/1, intr0/1)
and 2-D detections with confidences, and the reference scores it from those in its result scripts
(copenet_real/scripts/copenet_real_res_compile.py:132-143, final_res_compile.py:149-152, utils/geometry.py lstsq_triangulation, the
reprojection term of copenet_twoview.py:112-123): each view's prediction is carried into the world frame and the two are compared,
the detections are triangulated and each view's joints compared with the result.  apg_xview_update (csrc/xview_metrics.hip,
include/airpose_grad.h) does all of it on the device, in fp64 where it matters, in a fixed order: no torch.inverse, no bmm over the
vertices, no lstsq loop, nothing moved to the host until compute().  There is no fallback: a missing library is an error.
"""
import math

import torch

from . import _native_grad as G
from . import _stream_metric as S

ACC = 26                                 # include/airpose_grad.h: APG_XVIEW_ACC
PER_VIEW = 9                             # APG_XVIEW_PER_VIEW: joints, extr, vertices, root, trans, rot, j2d, keypoints, intr
NJ = 22                                  # the body joints of rotations, reprojection and triangulation
ROOTS = ("trans", "joint0")
# the columns of the per-sample output (APG_XVIEW_PER_SAMPLE = 16)
PER_SAMPLE = ("skipped", "joint_gap_world", "joint_gap_root", "vertex_gap_world", "vertex_gap_root", "trans_gap", "orient_gap_deg",
              "pose_gap_deg", "reproj_px0", "reproj_px1", "reproj_n0", "reproj_n1", "tri_mpjpe0", "tri_mpjpe1", "tri_n", "reserved")
# accumulator slots
(A_SEEN, A_SKIPPED, A_JW, A_JR, A_NROOT, A_VW, A_VR, A_NVERT, A_NVROOT, A_TRANS, A_NTRANS, A_ORIENT, A_POSE, A_NROT, A_RP0, A_RP1,
 A_RS0, A_RS1, A_RN0, A_RN1, A_NRP, A_TRI0, A_TRI1, A_TRIN, A_NTRI, A_RESERVED) = range(ACC)


def _rule(B, tail, at_least=None):
    """a shape rule (S.check_what): (B,) + tail, where the entry tail[0] may be larger when at_least is set"""
    def rule(shape):
        ok = len(shape) == 1 + len(tail) and shape[0] == B and tuple(shape[2:]) == tuple(tail[1:]) and \
            (shape[1] >= tail[0] if at_least else shape[1] == tail[0])
        if not ok:
            return "(%d, %s%s)" % (B, "at least " if at_least else "", ", ".join(str(t) for t in tail))
    return rule


def _extr_rule(B):
    def rule(shape):
        if len(shape) != 3 or shape[0] != B or shape[1] not in (3, 4) or shape[2] != 4:
            return "(%d, 4, 4) or (%d, 3, 4)" % (B, B)
    return rule


def _keypoint_rule(B):
    def rule(shape):
        flat = len(shape) == 3 and shape[0] == B and shape[1] >= NJ and shape[2] == 3
        rows = len(shape) == 4 and shape[0] == B and shape[1] >= 1 and shape[2] >= NJ and shape[3] == 3
        if not (flat or rows):
            return "(%d, 2, 24, 3) (row 0 = OpenPose) or (%d, at least %d, 3)" % (B, B, NJ)
    return rule


class CrossViewMetrics(S.StreamMetric):
    """Score two-view results without ground truth, on libairpose_grad.so: a TwoViewInference stream or an AirPosePlusSequence.export
    dict, before and after fitting, before and after fine-tuning.

    CrossViewMetrics(n_joints=22, root="trans" | "joint0", min_ray_angle_deg=1.0, device=None, per_sample=False); two views only.

    With E_v = extr{v} = [R_v | t_v] (world -> camera) and W_v(p) = R_v^T (p - t_v), per sample and averaged over the stream:
      joint_gap_world / vertex_gap_world   mean_i |W_0(p0_i) - W_1(p1_i)| over the first n_joints joints / all vertices, metres
      joint_gap_root / vertex_gap_root     the same after subtracting each view's root (root="trans": pred_smpltrans{v}, the
                                           reference's choice; "joint0": joint 0 of pred_j3d_cam{v})
      trans_gap                            |W_0(s0) - W_1(s1)| of pred_smpltrans0/1
      orient_gap_deg, pose_gap_deg         the angle between the root rotations carried into the world; the mean angle between the
                                           views' 21 body-joint rotations (degrees)
      reproj_px{v}, reproj_n{v}            sum_i c_i |pred_j2d_cam{v}_i - k_i| / sum_i c_i over the first 22 joints against the
                                           OpenPose row of smpl_joints_2d{v} (the pair RealDataLoss compares); the keypoints with c > 0
      tri_mpjpe{v}, tri_n                  the mean distance of W_v(p_v,i) from the point T_i the two detections triangulate to
                                           (lstsq_triangulation, solved in fp64 on the device) over the valid joints; their number
    A sample whose extrinsics are not finite or not orthonormal to 1e-3 is skipped and counted under `skipped`.  A triangulated
    joint is valid where both confidences are > 0, both keypoints are finite and the two rays meet at min_ray_angle_deg or more.
    The 1 degree default is a design choice: at 10 m range and f = 1500 px one pixel of detector noise already moves the
    triangulated depth by about 0.4 m at that angle, and below it the depth is noise.

    update(output, batch=None): each key is looked up in `output` first and then in `batch`.
      pred_j3d_cam0/1 (B, J >= n_joints, 3) and extr0/1 (B, 4, 4) or (B, 3, 4)                     required
      pred_vertices_cam0/1 (B, V, 3)                                                             optional
      pred_smpltrans0/1 (B, 3)                                                                   optional; required with root="trans"
      pred_rotmat0/1 (B, 22, 3, 3), else pred_angles0/1 (B, 22, 3)                               optional
      pred_j2d_cam0/1 (B, J >= 22, 2) with smpl_joints_2d0/1 (B, 2, 24, 3) or (B, J >= 22, 3)      optional
      intr0/1 (B, 3, 3)                                switches the triangulation on when the keypoints are there (J >= 22 joints)
    Every optional entry is given for both views or for neither.  A missing key, a half-given pair, a CPU tensor, a wrong shape and
    a non-floating dtype are refused by name.  update runs on the current stream and never synchronises the host; with
    per_sample=True it returns (values (B, 16) in the columns PER_SAMPLE, tri (B, 22, 4) = x, y, z, valid in the world frame, or
    None without triangulation).

    compute() synchronises once and returns Python floats: count, skipped and the keys above where they were fed.  reset() clears
    the sums; state() / load_state() expose the raw fp64 sums ((2, 13): the 26 slots of include/airpose_grad.h) so that ranks or
    shards can add them.  _stream_metric.evaluate takes the object next to EvalMetrics and MeshMetrics.

    An AirPosePlusSequence.export dict is scored with one camera as the world: export's cam1_wrt_cam0 = smpl_wrt_cam0
    smpl_wrt_cam1^-1 carries camera 1's coordinates into camera 0's, so it is extr0 with world = camera 1 and extr1 = the identity
    (its inverse would be extr1 with world = camera 0).  The dict's pred_j3d_cam0/1 and pred_vertices_cam0/1 are read as they
    are; pass trans0 / trans1 as pred_smpltrans0/1 (the roots), for the frames of export's slice.
    """

    NAME, ACC_SHAPE = "CrossViewMetrics", (2, ACC // 2)
    STATE = {"n_joints": "the state compares %r joints, this object %d",
             "root": "the state's root is %r, this object's %r",
             "min_ray_angle_deg": "the state's min_ray_angle_deg is %r, this object's %r"}

    def __init__(self, n_joints=22, root="trans", min_ray_angle_deg=1.0, device=None, per_sample=False):
        S.StreamMetric.__init__(self, "twoview", device, per_sample, n_joints, root, min_ray_angle_deg)

    def _configure(self, n_joints, root, min_ray_angle_deg):
        if int(n_joints) != n_joints or n_joints < 1:
            raise ValueError("CrossViewMetrics: n_joints must be a positive integer, got %r" % (n_joints,))
        if root not in ROOTS:
            raise ValueError("CrossViewMetrics: root must be one of %s, got %r" % (", ".join(ROOTS), root))
        a = float(min_ray_angle_deg)
        if not 0.0 <= a <= 90.0:
            raise ValueError("CrossViewMetrics: min_ray_angle_deg must be in 0 .. 90, got %r" % (min_ray_angle_deg,))
        self.n_joints, self.root, self.min_ray_angle_deg = int(n_joints), root, a
        self.min_sin2 = math.sin(math.radians(a)) ** 2

    # ---------------------------------------------------------------------------------------- the dict
    def gather(self, output, batch=None):
        """-> dict name -> [(key, tensor) of view 0, of view 1] or None: which entries of output / batch an update would read
        (joints, extr, vertices, trans, rot, j2d, keypoints, intr, and "rot_kind").  Refuses a missing required key and an entry
        given for one view only, by name; looks at no tensor."""
        find, need = self._lookup(output, batch)
        got = {"joints": [need(["pred_j3d_cam%d" % v], "the predicted joints") for v in range(2)],
               "extr": [need(["extr%d" % v], "the extrinsics, world -> camera") for v in range(2)]}

        def pair(fmt):
            hit = [find([fmt % v]) for v in range(2)]
            if (hit[0] is None) != (hit[1] is None):
                v = 0 if hit[0] is not None else 1
                raise RuntimeError("%s(%s): %s is given for one view only (%s is missing)" % (self.NAME, self.kind, hit[v][0], fmt % (1 - v)))
            return hit if hit[0] is not None else None
        got["vertices"] = pair("pred_vertices_cam%d")
        got["trans"] = pair("pred_smpltrans%d")
        if self.root == "trans" and got["trans"] is None:
            need(["pred_smpltrans0"], 'the roots of root="trans"')
        rot, angles = pair("pred_rotmat%d"), pair("pred_angles%d")
        got["rot"], got["rot_kind"] = (rot, "rotmat") if rot is not None else (angles, "angles" if angles is not None else None)
        got["j2d"], got["keypoints"], got["intr"] = pair("pred_j2d_cam%d"), pair("smpl_joints_2d%d"), pair("intr%d")
        if got["j2d"] is not None and got["keypoints"] is None:
            raise RuntimeError("%s(%s): %s is given without smpl_joints_2d0" % (self.NAME, self.kind, got["j2d"][0][0]))
        return got

    # ---------------------------------------------------------------------------------------- the sums
    def update(self, output, batch=None):
        got = self.gather(output, batch)
        dev, nj = self.device, self.n_joints
        B = self._batch_size(got["joints"][0])
        if B < 1:
            raise RuntimeError("CrossViewMetrics: %s holds no sample" % got["joints"][0][0])
        use_kp = got["keypoints"] is not None and (got["j2d"] is not None or got["intr"] is not None)
        use_tri = got["keypoints"] is not None and got["intr"] is not None
        need_j = max(nj, NJ if use_tri else 1)
        rules = {"joints": _rule(B, (need_j, 3), at_least=True), "extr": _extr_rule(B), "vertices": _rule(B, (1, 3), at_least=True),
                 "trans": _rule(B, (3,)), "rot": _rule(B, (NJ, 3, 3) if got["rot_kind"] == "rotmat" else (NJ, 3)),
                 "j2d": _rule(B, (NJ, 2), at_least=True), "keypoints": _keypoint_rule(B), "intr": _rule(B, (3, 3))}
        order = ["joints", "extr", "vertices", "trans", "rot", "j2d", "keypoints", "intr"]
        used = [k for k in order if got[k] is not None and (k != "keypoints" or use_kp) and (k != "intr" or use_tri)]
        entries = [(got[k][v][1], rules[k], got[k][v][0]) for k in used for v in range(2)]
        ten = S.place(self.NAME, entries, dev)
        t = {k: (ten[2 * i], ten[2 * i + 1]) for i, k in enumerate(used)}
        for k in used:                                           # the two views share one stride
            if t[k][0].shape != t[k][1].shape:
                raise RuntimeError("CrossViewMetrics: %s must have the shape of %s, %s, got %s" % (
                    got[k][1][0], got[k][0][0], tuple(t[k][0].shape), tuple(t[k][1].shape)))

        def stride(k):
            return t[k][0][0].numel() if k in t else 0
        root = t["trans"] if self.root == "trans" else t["joints"]
        V = t["vertices"][0].shape[1] if "vertices" in t else 0
        opt = lambda k, v: t[k][v] if k in t else None
        table = [x for v in range(2) for x in (t["joints"][v], t["extr"][v], opt("vertices", v), root[v], opt("trans", v), opt("rot", v),
                                               opt("j2d", v), opt("keypoints", v), opt("intr", v))]
        strides = [stride("joints"), stride("extr"), stride("vertices"), stride("trans" if self.root == "trans" else "joints"),
                   stride("trans"), stride("rot"), stride("j2d"), stride("keypoints"), stride("intr")]
        L = G.lib()
        with torch.cuda.device(dev):
            nbytes = L.apg_xview_workspace_bytes(B, 2, V)
            if nbytes < 0:
                raise RuntimeError("CrossViewMetrics: B = %d with %d vertices is outside apg_xview_update's limits" % (B, V))
            acc, ws = self._buffers(nbytes)
            ps = tri = None
            if self.per_sample:
                ps = torch.empty(B, len(PER_SAMPLE), device=dev, dtype=torch.float32)
                tri = torch.empty(B, NJ, 4, device=dev, dtype=torch.float32) if use_tri else None
            G.check(L.apg_xview_update(B, 2, nj, V, 1 if got["rot_kind"] == "rotmat" else 0, (G._i64 * PER_VIEW)(*strides),
                                       G.ptrs(table), self.min_sin2, G.vp(ps), G.vp(tri), G.vp(acc), G.vp(ws), ws.numel() * 8,
                                       G.stream(dev)), "apg_xview_update")
        return (ps, tri) if self.per_sample else None

    summarise = staticmethod(lambda acc, views: summarise(acc, views))


def summarise(acc, views=2):
    """the metrics dict from the raw sums ((2, 13) float64, host: the 26 slots of include/airpose_grad.h)"""
    a = torch.as_tensor(acc).reshape(-1).tolist()
    count = a[A_SEEN] - a[A_SKIPPED]
    out = {"count": int(count), "skipped": int(a[A_SKIPPED])}

    def mean(name, s, n, fed=None):
        if a[n if fed is None else fed]:
            out[name] = a[s] / a[n] if a[n] else float("nan")
    if count:
        out["joint_gap_world"] = a[A_JW] / count
    mean("joint_gap_root", A_JR, A_NROOT)
    mean("vertex_gap_world", A_VW, A_NVERT)
    mean("vertex_gap_root", A_VR, A_NVROOT)
    mean("trans_gap", A_TRANS, A_NTRANS)
    mean("orient_gap_deg", A_ORIENT, A_NROT)
    mean("pose_gap_deg", A_POSE, A_NROT)
    for v in range(2):
        mean("reproj_px%d" % v, A_RP0 + v, A_RS0 + v, fed=A_NRP)
        if a[A_NRP]:
            out["reproj_n%d" % v] = int(a[A_RN0 + v])
    for v in range(2):
        mean("tri_mpjpe%d" % v, A_TRI0 + v, A_TRIN, fed=A_NTRI)
    if a[A_NTRI]:
        out["tri_n"] = int(a[A_TRIN])
    return out
