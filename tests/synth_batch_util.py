"""Shared by tests/test_synth_batch_abi.py, test_synth_batch_fp64.py and test_synth_batch_module.py: the numpy restatement of what
apg_synth_batch (airpose_amd/csrc/synth_batch.hip) computes, a numpy Philox4x32-10, the planted records, and the bars.  CPU only.

The restatement is written from reading copenet/src/copenet/dsets/aerialpeople.py, aerialpeople_crop.__getitem__: the region
ymin = y0 - m if y0 - m > 0 else 0, ymax = y1 + m if y1 + m < H else H, x likewise with W (:98-101); four offsets drawn in the order
ymin side, ymax side, xmin side, xmax side, each 0 when its range is 0 and otherwise uniform in [0, range) (:104-122); crop_info =
[[ymin, xmin], [ymax, xmax]], the REGION (:132); bb = (crop centre / principal point - 1) (:134-135) with s = 224 / max(h, w) of the
crop appended (:200); transform_smpl of vertices, joints, orientation and translation (:160-164); perspective_projection with R = I,
t = 0 (:166-170); the joints in crop pixels s * (j2d - (bb + 1) * c), no pad offset (:172); lbs.batch_rodrigues of the body pose
(:177); cam1 = randint(2) per sample (:208-211) -- plus the three rules of include/airpose_grad.h that hold where the reference itself
breaks (a corner outside the frame is clamped to it, an empty crop becomes one pixel, a crop that leaves the canvas is clamped to it)
and the header's draws (Philox4x32-10 keyed by the seed, counted by dataset index, epoch and camera) in place of np.random.
`mut=` replaces one line.  `dtype=np.float32` evaluates the same chains with every operation rounded to fp32: the host floor.

clamp_le_not_lt is an EQUIVALENT mutant, and the tests say so instead of asking it to differ: `y0 - m if y0 - m > 0 else 0` and
`y0 - m if y0 - m >= 0 else 0` differ only at y0 - m == 0, where both give 0, and `y1 + m if y1 + m < H else H` against `<=` only at
y1 + m == H, where both give H.  What the planted boxes (one with y0 - m == 0 and y1 + m == H exactly) do tell apart is a clamp
against the other axis's size (clamp_sizes_swapped) and a clamp that is off by one (clamp_off_by_one); those must differ."""
import functools

import numpy as np
import torch

from oracle import geometry_ref, smplx_ref

H, W, MARGIN, HC, WC = 120, 160, 20, 96, 128                 # frame, margin, canvas (origin "region"); origin "frame": canvas = frame
FOCAL = (1475.0, 1475.0)
SEED = 0x9E3779B97F4A7C15                                   # both key words in use
NS, VS, JS = (1, 5), (1, 67, 10475), (22, 127)               # 10475 = 40 * 256 + 235: no multiple of any block
INDEX = (7, 123456, 3, 2 ** 31 - 1, 0)                       # the samples' dataset indices
CLAMPED, WIDENED, OUTSIDE = 1, 2, 4                          # include/airpose_grad.h: APG_SYNTH_*
ORIGINS = {"region": 0, "frame": 1}
MUTATIONS = ("draw_order_swapped", "crop_info_is_crop", "clamp_sizes_swapped", "clamp_off_by_one", "offset_is_word_mod_range",
             "bb_from_region", "crop_adds_pad", "flip_is_camera_0_s_draw")
EQUIVALENT = ("clamp_le_not_lt",)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
U32 = 2.0 ** -24                                             # half an ulp, relative: one fp32 rounding of v is at most U32 |v|
G2 = 1.0 + 2.0 ** -20                                        # the second-order terms of a first-order budget
PER_VIEW = ("crops", "crop_info", "status", "bb", "intr", "extr", "verts_rel", "joints_rel", "orient_rel", "trans_rel", "j2d", "j2d_crop")
INT_KEYS = ("crops", "crop_info", "status", "flip")

# the planted boxes [[x0, y0], [x1, y1]] of sample i, camera c (the rest are drawn): every region fits the 96 x 128 canvas except
# FULL's, whose crop the canvas clamps (OUTSIDE) under origin "region"
B_GENERIC, B_TOP_LEFT, B_BOTTOM_RIGHT, B_RANGE1_LOW, B_RANGE1_HIGH, B_DEGENERATE, B_FULL, B_EXACT, B_ONE_OFF = (
    (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (4, 0))
PLANTED = {B_GENERIC: ((50, 30), (90, 80)),
           B_TOP_LEFT: ((0, 0), (40, 30)),                   # ranges 0 on the ymin and xmin sides -> offsets 0
           B_BOTTOM_RIGHT: ((W - 40, H - 30), (W, H)),       # ranges 0 on the ymax and xmax sides
           B_RANGE1_LOW: ((1, 1), (41, 31)),                 # range 1: the only value is 0
           B_RANGE1_HIGH: ((W - 41, H - 31), (W - 1, H - 1)),
           B_DEGENERATE: ((70, 50), (70, 50)),               # no pixel inside; the margin keeps the crop non-empty
           B_FULL: ((0, 0), (W, H)),
           B_EXACT: ((80, MARGIN), (W - MARGIN, 60)),        # y0 - m == 0 and x1 + m == W exactly
           B_ONE_OFF: ((80, MARGIN + 1), (W - MARGIN - 1, 61))}       # y0 - m == 1 and x1 + m == W - 1


# ------------------------------------------------------------------------------------------------ Philox4x32-10
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox(ctr, key):
    """Random123's Philox4x32-10: ctr = 4 and key = 2 arrays (or numbers) of 32-bit words -> (..., 4) uint32"""
    c = [np.asarray(x, np.uint64) & np.uint64(_MASK) for x in ctr]
    k0, k1 = (np.asarray(x, np.uint64) & np.uint64(_MASK) for x in key)
    m = np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(_W0)) & m, (k1 + np.uint64(_W1)) & m
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def draws(seed, epoch, index, cam):
    """the four words of (seed, epoch, dataset index, camera; camera 2 = the flip's counter)"""
    return philox((np.asarray(index, np.int64) & _MASK, epoch & _MASK, cam, 0), (seed & _MASK, (seed >> 32) & _MASK))


def offset(word, r, mut=None):
    """word k of the draw -> offset k over the range r: 0 if r == 0 else mulhi32(word, r), in [0, r)"""
    if r == 0:
        return 0
    return int(word) % r if mut == "offset_is_word_mod_range" else (int(word) * r) >> 32


# ------------------------------------------------------------------------------------------------ inputs
def _rotation(g):
    q, r = np.linalg.qr(g.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def case(n, V, J):
    """the stacked record fields of n samples as float32 / int32 numpy arrays, and their dataset indices"""
    g = np.random.default_rng(8100 + 1000 * n + 10 * V + J)
    bb = np.zeros((n, 2, 2, 2), np.int32)
    for i in range(n):
        for c in (0, 1):
            if (i, c) in PLANTED:
                bb[i, c] = PLANTED[i, c]
            else:                                            # h <= 56 and w <= 88: the region fits the canvas
                h, w = int(g.integers(8, 57)), int(g.integers(8, 89))
                y0, x0 = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
                bb[i, c] = ((x0, y0), (x0 + w, y0 + h))
    intr = np.zeros((n, 2, 3, 3), np.float32)
    extr = np.zeros((n, 2, 4, 4), np.float32)
    for i in range(n):
        for c in (0, 1):                                     # the sample's own principal point, never a half-integer
            intr[i, c] = [[1400.0 + 10 * i, 0, 83.25 + 3 * i + c], [0, 1410.0 + 10 * c, 57.25 + 2 * i - c], [0, 0, 1]]
            extr[i, c, :3, :3] = _rotation(g)
            extr[i, c, :3, 3] = [g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(4, 6)]     # joints within 0.87 of the origin: z >= 2
            extr[i, c, 3] = [0, 0, 0, 1]
    pose = (0.4 * g.standard_normal((n, 63))).astype(np.float32)
    pose[0, 0:3] = 0.0                                       # the identity (the angle is |1e-8|)
    pose[0, 3:6] = [1e-4, -2e-4, 5e-5]                       # a small angle
    pose[0, 6:9] = [2.2, -1.9, 0.6]                          # an angle near pi
    rec = dict(bb=bb, intr=intr, extr=extr, smplpose=pose, smplshape=g.standard_normal((n, 10)).astype(np.float32),
               smpl_vertices_wrt_origin=g.uniform(-1, 1, (n, 1, V, 3)).astype(np.float32),
               smpl_joints_wrt_origin=g.uniform(-0.5, 0.5, (n, 1, J, 3)).astype(np.float32),
               smplorient_rotmat_wrt_origin=np.stack([_rotation(g) for _ in range(n)])[:, None].astype(np.float32),
               smpltrans=g.uniform(-3, 3, (n, 3)).astype(np.float32))
    return rec, np.asarray(INDEX[:n], np.int32)


@functools.lru_cache(maxsize=None)
def hostile():
    """records of 5 samples whose boxes no dataset holds, for the box kernel alone: outside the frame on every side, inverted,
    negative, INT_MIN / INT_MAX in every position"""
    rec, index = case(5, 1, 22)
    rec = dict(rec)
    lo, hi = INT_MIN, INT_MAX
    rec["bb"] = np.asarray([
        [[[200, 150], [260, 190]], [[-90, -70], [-10, -5]]],          # beyond the bottom-right corner; beyond the top-left
        [[[100, 100], [10, 10]], [[60, 50], [50, 40]]],               # inverted far apart (always empty); inverted by 10 (empty or not, by the draw)
        [[[lo, lo], [hi, hi]], [[hi, hi], [lo, lo]]],
        [[[lo, lo], [lo, lo]], [[hi, hi], [hi, hi]]],
        [[[lo, 40], [30, hi]], [[W, H], [W, H]]]], np.int32)          # mixed; the degenerate box on the far corner
    return rec, index


# ------------------------------------------------------------------------------------------------ the chains, in `dtype`
def rigid(M, p, dtype, translate=True):
    """((R0 x + R1 y) + R2 z) + t per row of M (..., 3 or 4, 4) for points p (..., P, 3), one rounding per operation"""
    M, p = np.asarray(M, dtype), np.asarray(p, dtype)
    x, y, z = (p[..., None, :, k] for k in range(3))         # (..., 1, P)
    out = (M[..., :3, 0, None] * x + M[..., :3, 1, None] * y) + M[..., :3, 2, None] * z
    if translate:
        out = out + M[..., :3, 3, None]
    return np.swapaxes(out, -1, -2)                          # (..., P, 3)


def project(X, focal, centre, dtype):
    """f (x / z, y / z) + c"""
    X, c = np.asarray(X, dtype), np.asarray(centre, dtype)
    f = np.asarray(focal, dtype)
    return f * (X[..., :2] / X[..., 2:3]) + c[..., None, :]


def to_crop(j2d, bb, centre, dtype):
    """s * (j2d - (bb_xy + 1) * c)"""
    j, b, c = np.asarray(j2d, dtype), np.asarray(bb, dtype), np.asarray(centre, dtype)
    return b[..., None, 2:3] * (j - ((b[..., :2] + dtype(1)) * c)[..., None, :])


def rodrigues(r, dtype):
    """lbs.batch_rodrigues (epsilon 1e-8): (.., 3) -> (.., 3, 3), K K summed in bmm's order"""
    r = np.asarray(r, dtype)
    e = r + dtype(1e-8)
    angle = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    x, y, z = (r[..., k] / angle for k in range(3))
    s, c1 = np.sin(angle), dtype(1) - np.cos(angle)
    o = np.zeros_like(x)
    K = np.stack([o, -z, y, z, o, -x, -y, x, o], -1)
    KK = np.stack([-(z * z) - y * y, y * x, z * x, x * y, -(z * z) - x * x, z * y, x * z, y * z, -(y * y) - x * x], -1)
    eye = np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype)
    return ((eye + s[..., None] * K) + c1[..., None] * KK).reshape(r.shape[:-1] + (3, 3)).astype(dtype)


# ------------------------------------------------------------------------------------------------ the restatement
def _axis(a0, a1, S, Sc, m, region, w0, w1, jitter, mut):
    st = 0
    c0, c1 = min(max(a0, 0), S), min(max(a1, 0), S)          # rule 1
    if (c0, c1) != (a0, a1):
        st |= CLAMPED
    if mut == "clamp_le_not_lt":
        lo, hi = (c0 - m if c0 - m >= 0 else 0), (c1 + m if c1 + m <= S else S)
    elif mut == "clamp_off_by_one":
        lo, hi = (c0 - m if c0 - m > 1 else 0), (c1 + m if c1 + m < S - 1 else S)
    else:
        lo, hi = (c0 - m if c0 - m > 0 else 0), (c1 + m if c1 + m < S else S)
    o0 = offset(w0, c0 - lo, mut) if jitter else 0
    o1 = offset(w1, hi - c1, mut) if jitter else 0
    p0, p1 = lo + o0, hi - o1
    if p1 <= p0:                                             # rule 2
        p0 = min(p0, S - 1)
        p1 = p0 + 1
        st |= WIDENED
    base = lo if region else 0
    q0, q1 = p0 - base, p1 - base
    if q0 < 0 or q1 > Sc:                                    # rule 3
        q0 = min(max(q0, 0), Sc - 1)
        q1 = min(max(q1, q0 + 1), Sc)
        st |= OUTSIDE
    return lo, hi, q0 + base, q1 + base, q0, q1, st


def ref_batch(rec, index, seed=SEED, epoch=0, origin="region", jitter=True, shuffle=True, margin=MARGIN, frame=(H, W), canvas=None,
              focal=FOCAL, mut=None, dtype=np.float64, boxes_only=False):
    """what apg_synth_batch writes, indexed by SUFFIX like the kernel's outputs: crops (2, n, 4), crop_info (2, n, 2, 2), status
    (2, n), flip (n) int32; in `dtype` bb (2, n, 3), intr, extr (copies), verts_rel (2, n, V, 3), joints_rel (2, n, J, 3), orient_rel
    (2, n, 3, 3), trans_rel (2, n, 3), j2d and j2d_crop (2, n, J, 2), pose_rotmat (n, 21, 3, 3); scale (2, n) float64 unrounded"""
    assert mut is None or mut in MUTATIONS + EQUIVALENT, mut
    Hf, Wf = frame
    Hc, Wc = canvas if canvas is not None else ((HC, WC) if origin == "region" else frame)
    bb_in = rec["bb"].astype(np.int64)
    n = bb_in.shape[0]
    V, J = rec["smpl_vertices_wrt_origin"].shape[2], rec["smpl_joints_wrt_origin"].shape[2]
    o = dict(crops=np.zeros((2, n, 4), np.int32), crop_info=np.zeros((2, n, 2, 2), np.int32), status=np.zeros((2, n), np.int32),
             flip=np.zeros(n, np.int32), bb=np.zeros((2, n, 3), dtype), scale=np.zeros((2, n)), intr=np.zeros((2, n, 3, 3), dtype),
             extr=np.zeros((2, n, 4, 4), dtype), verts_rel=np.zeros((2, n, V, 3), dtype), joints_rel=np.zeros((2, n, J, 3), dtype),
             orient_rel=np.zeros((2, n, 3, 3), dtype), trans_rel=np.zeros((2, n, 3), dtype), j2d=np.zeros((2, n, J, 2), dtype),
             j2d_crop=np.zeros((2, n, J, 2), dtype))
    for i in range(n):
        flip = int(draws(seed, epoch, index[i], 0 if mut == "flip_is_camera_0_s_draw" else 2)[0] >> 31) if shuffle else 0
        o["flip"][i] = flip
        for c in (0, 1):
            s = c ^ flip
            w = draws(seed, epoch, index[i], c)
            (x0, y0), (x1, y1) = (int(v) for v in bb_in[i, c, 0]), (int(v) for v in bb_in[i, c, 1])
            wy, wx = ((w[2], w[3]), (w[0], w[1])) if mut == "draw_order_swapped" else ((w[0], w[1]), (w[2], w[3]))
            Sy, Sx = (Wf, Hf) if mut == "clamp_sizes_swapped" else (Hf, Wf)
            ylo, yhi, py0, py1, qy0, qy1, sty = _axis(y0, y1, Sy, Hc, margin, origin == "region", wy[0], wy[1], jitter, mut)
            xlo, xhi, px0, px1, qx0, qx1, stx = _axis(x0, x1, Sx, Wc, margin, origin == "region", wx[0], wx[1], jitter, mut)
            o["crops"][s, i] = (qy0, qy1, qx0, qx1)
            o["crop_info"][s, i] = ((py0, px0), (py1, px1)) if mut == "crop_info_is_crop" else ((ylo, xlo), (yhi, xhi))
            o["status"][s, i] = sty | stx
            if boxes_only:
                continue
            K, E = rec["intr"][i, c].astype(dtype), rec["extr"][i, c].astype(dtype)
            centre = np.asarray([K[0, 2], K[1, 2]], dtype)
            mid = np.asarray([xlo + xhi, ylo + yhi] if mut == "bb_from_region" else [px0 + px1, py0 + py1], dtype)
            s64 = 224.0 / max(qy1 - qy0, qx1 - qx0)
            o["scale"][s, i] = s64
            with np.errstate(divide="ignore", invalid="ignore"):
                o["bb"][s, i, :2] = mid / dtype(2) / centre - dtype(1)
            o["bb"][s, i, 2] = dtype(s64)
            o["intr"][s, i], o["extr"][s, i] = K, E
            o["verts_rel"][s, i] = rigid(E, rec["smpl_vertices_wrt_origin"][i, 0], dtype)
            o["joints_rel"][s, i] = rigid(E, rec["smpl_joints_wrt_origin"][i, 0], dtype)
            o["orient_rel"][s, i] = rigid(E, rec["smplorient_rotmat_wrt_origin"][i, 0].T, dtype, translate=False).T
            o["trans_rel"][s, i] = rigid(E, rec["smpltrans"][i][None], dtype)[0]
            o["j2d"][s, i] = project(o["joints_rel"][s, i], focal, centre, dtype)
            o["j2d_crop"][s, i] = to_crop(o["j2d"][s, i], o["bb"][s, i], centre, dtype)
            if mut == "crop_adds_pad":
                o["j2d_crop"][s, i] += ((224 - int(s64 * (qx1 - qx0))) // 2, (224 - int(s64 * (qy1 - qy0))) // 2)
    if not boxes_only:
        o["pose_rotmat"] = rodrigues(rec["smplpose"].reshape(n, 21, 3), dtype)
    return o


def oracle_pieces(rec):
    """the pieces that oracle/ already states, from the same records in fp64, per CAMERA: verts_rel and joints_rel
    (geometry_ref.transform_smpl), j2d (geometry_ref.perspective_projection with R = I, t = 0), pose_rotmat (smplx_ref.batch_rodrigues)"""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    n = rec["bb"].shape[0]
    out = dict(verts_rel=[], joints_rel=[], j2d=[])
    for c in (0, 1):
        v, j = geometry_ref.transform_smpl(t(rec["extr"][:, c]), t(rec["smpl_vertices_wrt_origin"][:, 0]), t(rec["smpl_joints_wrt_origin"][:, 0]))
        p = geometry_ref.perspective_projection(j, torch.eye(3, dtype=torch.float64).expand(n, 3, 3), torch.zeros(n, 3, dtype=torch.float64),
                                                t(FOCAL), t(rec["intr"][:, c, :2, 2]))
        out["verts_rel"].append(v.numpy()), out["joints_rel"].append(j.numpy()), out["j2d"].append(p.numpy())
    out = {k: np.stack(v) for k, v in out.items()}
    out["pose_rotmat"] = smplx_ref.batch_rodrigues(t(rec["smplpose"]).reshape(-1, 3)).reshape(n, 21, 3, 3).numpy()
    return out


def by_camera(per_suffix, flip):
    """(2 suffixes, n, ...) -> (2 cameras, n, ...): camera c of sample i sits under suffix c ^ flip[i]"""
    a = np.asarray(per_suffix)
    idx = np.arange(a.shape[1])
    return np.stack([a[flip, idx], a[1 - flip, idx]])


def differs(got, ref, keys=None):
    """the outputs of `got` (tensors or arrays) that are not what `ref` says: integers exactly, floats by more than 1e-3 (far above
    any rounding at these sizes, far below what a mutation moves)"""
    bad = []
    for k in keys or [k for k in ref if k in got and k != "scale"]:
        g = np.asarray(got[k].cpu() if torch.is_tensor(got[k]) else got[k])
        if k in INT_KEYS:
            if not np.array_equal(g, ref[k]):
                bad.append(k)
        else:
            with np.errstate(invalid="ignore"):
                if not (np.abs(g.astype(np.float64) - np.asarray(ref[k], np.float64)) <= 1e-3).all():
                    bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ the bars
def ulp32(x):
    """the spacing of fp32 at |x| (normal range)"""
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.where(x > 0, x, 1.0))) - 23), 2.0 ** -149)


def rigid_bar(M, p, translate=True):
    """X = fl(fl(fl(a + b) + c) + t), a = fl(R0 x), b = fl(R1 y), c = fl(R2 z), from EXACT fp32 M and p: one rounding of at most
    U32 |v| at each of a, b, c, a + b, (a + b) + c and X (five without t), to first order; G2 carries the second order"""
    M, p = np.asarray(M, np.float64), np.asarray(p, np.float64)
    x, y, z = (p[..., None, :, k] for k in range(3))
    a, b, c = M[..., :3, 0, None] * x, M[..., :3, 1, None] * y, M[..., :3, 2, None] * z
    bar = np.abs(a) + np.abs(b) + np.abs(c) + np.abs(a + b) + np.abs(a + b + c)
    if translate:
        bar = bar + np.abs(a + b + c + M[..., :3, 3, None])
    return np.swapaxes(U32 * G2 * bar, -1, -2)


def project_bar(X, focal, centre):
    """j = fl(fl(f fl(x / z)) + c) from EXACT fp32 x, z, f, c: the divide's rounding U32 |q| carried through f, the product's
    U32 |f q|, the sum's U32 |j|"""
    X = np.asarray(X, np.float64)
    fq = np.asarray(focal, np.float64) * (X[..., :2] / X[..., 2:3])
    return U32 * G2 * (2 * np.abs(fq) + np.abs(fq + np.asarray(centre, np.float64)[..., None, :]))


def crop_bar(j2d, bb, centre):
    """r = fl(s fl(j - fl(fl(b + 1) c))) from EXACT fp32 j, b, s, c: U32 |b + 1| carried through c and s, U32 |p| of the product p =
    (b + 1) c and U32 |d| of the difference d = j - p carried through s, U32 |r| of the last product"""
    j, b, c = np.asarray(j2d, np.float64), np.asarray(bb, np.float64), np.asarray(centre, np.float64)
    t1 = b[..., :2] + 1.0
    p = (t1 * c)[..., None, :]
    d = j - p
    s = np.abs(b[..., None, 2:3])
    return U32 * G2 * (s * (np.abs(t1 * c)[..., None, :] + np.abs(p) + np.abs(d)) + np.abs(s * d))


def rodrigues_bar(r):
    """R = fl(fl(I + fl(s k)) + fl(c1 kk)) per ELEMENT, from EXACT fp32 r, with u = U32 and the device's sinf / cosf taken as 4 ulp
    (the allowance of tests/test_smplx_fwd_fp64.py):
      e = fl(r + 1e-8) u; e^2 3 u; the sum of the three 5 u; a = sqrt of it 3.5 u;  d = fl(r / a) 4.5 u, all relative
      s = sinf(a): 3.5 u a |cos a| + 4 ulp(sin a) =: ds;   c1 = fl(1 - cosf(a)): 3.5 u a |sin a| + 4 ulp(cos a) + u c1 =: dc
      k = 0 or +-d_m:  fl(s k) carries |k| ds + |s k| (4.5 u + u)
      kk = d_i d_j off the diagonal (9 u, + u) or -(d_i^2) - d_j^2 on it (10 u each square, + u): 11 u |kk| at most;
                       fl(c1 kk) carries |kk| dc + c1 |kk| (11 u + u)
      the two sums: u (|I + s k| + |R|)
    bar = |k| ds + 5.5 u |s k| + |kk| dc + 12 u c1 |kk| + u (|I + s k| + |R|), each element with its own k and kk."""
    r = np.asarray(r, np.float64)
    a = np.sqrt(((r + 1e-8) ** 2).sum(-1))
    x, y, z = (r[..., k] / a for k in range(3))
    o = np.zeros_like(x)
    K = np.stack([o, -z, y, z, o, -x, -y, x, o], -1)
    KK = np.stack([-(z * z) - y * y, y * x, z * x, x * y, -(z * z) - x * x, z * y, x * z, y * z, -(y * y) - x * x], -1)
    eye = np.asarray([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    s, c, c1 = np.sin(a)[..., None], np.cos(a)[..., None], (1.0 - np.cos(a))[..., None]
    ds = 3.5 * U32 * a[..., None] * np.abs(c) + 4 * ulp32(s)
    dc = 3.5 * U32 * a[..., None] * np.abs(s) + 4 * ulp32(c) + U32 * c1
    first = eye + s * K
    bar = np.abs(K) * ds + 5.5 * U32 * np.abs(s * K) + np.abs(KK) * dc + 12 * U32 * c1 * np.abs(KK) + U32 * (np.abs(first) + np.abs(first + c1 * KK))
    return (G2 * bar).reshape(r.shape[:-1] + (3, 3))


def chain_checks(rec, got, ref):
    """-> [(chain, |got - fp64|, bar)] for one batch: the transforms and the rotations against the restatement `ref` (their inputs are
    the records' exact fp32 values), the projection and the crop pixels each against fp64 on `got`'s OWN upstream outputs (exact
    fp32 values again), so that every chain is held to its own rounding budget and to nothing else"""
    f64 = lambda a: np.asarray(a, np.float64)
    flip = np.asarray(got["flip"])
    cam = lambda k, src: by_camera(f64(src[k]), flip)
    E = rec["extr"].transpose(1, 0, 2, 3)                    # (camera, n, 4, 4)
    n = rec["bb"].shape[0]
    centre = f64(got["intr"])[..., :2, 2]
    out = [("verts_rel", np.abs(cam("verts_rel", got) - cam("verts_rel", ref)), rigid_bar(E, rec["smpl_vertices_wrt_origin"][:, 0][None])),
           ("joints_rel", np.abs(cam("joints_rel", got) - cam("joints_rel", ref)), rigid_bar(E, rec["smpl_joints_wrt_origin"][:, 0][None])),
           ("orient_rel", np.abs(cam("orient_rel", got) - cam("orient_rel", ref)).transpose(0, 1, 3, 2),
            rigid_bar(E, rec["smplorient_rotmat_wrt_origin"][:, 0].transpose(0, 2, 1)[None], translate=False)),
           ("trans_rel", np.abs(cam("trans_rel", got) - cam("trans_rel", ref))[:, :, None], rigid_bar(E, rec["smpltrans"][:, None][None])),
           ("pose_rotmat", np.abs(f64(got["pose_rotmat"]) - ref["pose_rotmat"]), rodrigues_bar(rec["smplpose"].reshape(n, 21, 3))),
           ("j2d", np.abs(f64(got["j2d"]) - project(f64(got["joints_rel"]), FOCAL, centre, np.float64)),
            project_bar(f64(got["joints_rel"]), FOCAL, centre)),
           ("j2d_crop", np.abs(f64(got["j2d_crop"]) - to_crop(f64(got["j2d"]), f64(got["bb"]), centre, np.float64)),
            crop_bar(f64(got["j2d"]), f64(got["bb"]), centre))]
    return out


def worst(err, bar):
    """max err / bar; where the bar is 0 (an exact zero, such as an identity's off-diagonal) the error must be 0"""
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    assert (err[bar == 0] == 0).all()
    return float(np.divide(err, bar, out=np.zeros_like(err), where=bar > 0).max())
