"""Shared by tests/test_real_batch_abi.py, test_real_batch_fp64.py and test_real_batch_module.py: the fp64 restatement of what
apg_real_batch (airpose_amd/csrc/seq_batch.hip) computes, the planted inputs, and the bars.  CPU only.

The restatement is written from reading copenet_real/dsets/copenet_real.py: the agreement filter of __init__ (:105-106) and
__getitem__ (:162-258) -- x = opose[..., 0] where opose[..., 2] != 0, np.array([0]) when empty; xmin = int(min - 50) if that is > 0
else 0; xmax = int(max + 50) if that is below the frame's width else the width; bb = (box centre / principal point - 1); s =
224 / max(h, w) (resize_with_pad); crop = s * (xy - (bb + 1) * c) for both detectors, no pad offset -- plus the three rules of
include/airpose_grad.h that hold where the reference itself breaks (a non-finite keypoint is absent, a keypoint outside the frame is
clamped to it, an empty axis becomes one pixel).  For in-frame input all three are the identity.  `mut=` replaces one line.

floor_not_trunc is an EQUIVALENT mutant, and the tests say so instead of asking it to differ: every operand of int() that survives the
clamps at 0 and at the frame's size is >= 0 (min - border < 0 gives 0 through the clamp, whichever way it is rounded), and int() and
floor agree there.  What the planted cases of test_real_batch_fp64.py (min - border in (0, 1), min - border < 0, fractional max +
border) do tell apart from int() is rounding to NEAREST: the mutant round_not_trunc, which must differ."""
import functools
import math

import numpy as np
import torch

SIZES = ((120, 160), (90, 200))                              # (H, W) per view: small, non-square, unequal
PRINCIPAL = ((83.25, 57.25), (97.25, 49.75))                 # (cx, cy) per view: not the frame's centre, never a half-integer
L = 7
BORDERS = (10, 50)
SPANS = ((0, 1), (0, 3), (2, 5), (0, 7))                     # (a, n): 2 n below, at and across APG_BATCH_WAVES, and a > 0
AGREEMENT_PX = 100.0
F_GENERIC, F_TRUNC, F_NEGATIVE, F_EDGES, F_ZERO_CONF, F_ALPHA_ONLY, F_SPREAD = range(7)  # the frames of case()
J_EXACT, J_BEYOND = 5, 6                                     # frame F_GENERIC: the pair exactly 100 px apart, the pair one step beyond
MUTATIONS = ("agreement_ge", "filter_one_detector", "box_from_both_detectors", "round_not_trunc", "border_one_side",
             "centre_over_size", "crop_adds_pad", "fallback_empty_is_whole_frame")
EQUIVALENT = ("floor_not_trunc",)
FALLBACK, CLAMPED, WIDENED = 1, 2, 4                         # include/airpose_grad.h: APG_BATCH_*
SEED = 5200


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def case(border):
    """det (2, L, 2, 24, 3) fp32, every coordinate a multiple of 1/8 and inside its frame, for the box border `border`"""
    g = torch.Generator().manual_seed(SEED + border)
    eighth = lambda lo, hi, *s: torch.randint(int(lo * 8), int(hi * 8) + 1, s, generator=g).double() / 8
    det = torch.zeros(2, L, 2, 24, 3, dtype=torch.float64)
    for v, (H, W) in enumerate(SIZES):
        for f in range(L):
            op = torch.stack([eighth(30, W - 30, 24), eighth(20, H - 20, 24)], 1)
            al = op + eighth(-6, 6, 24, 2)
            conf = 0.1 + 0.9 * torch.rand(2, 24, generator=g, dtype=torch.float64)
            conf[0, [3, 6, 9, 13, 14, 15, 22, 23]] = 0.0     # op_map2smpl == -1
            conf[1, [0, 3, 6, 9, 10, 11, 13, 14, 15, 22, 23]] = 0.0
            if f == F_GENERIC:
                op[J_EXACT], al[J_EXACT] = torch.tensor([20.0, 5.0]), torch.tensor([80.0, 85.0])          # (60, 80): 100 px exactly
                op[J_BEYOND], al[J_BEYOND] = torch.tensor([20.0, 5.0]), torch.tensor([80.125, 85.0])      # 100.075 px
                conf[:, [J_EXACT, J_BEYOND]] = 0.75
                conf[0, 6], conf[1, 6] = 0.75, 0.5
            elif f == F_TRUNC:                               # min - border = 0.625, max + border fractional and inside
                op = torch.stack([eighth(border + 0.625, border + 8.625, 24), eighth(border + 0.625, border + 8.625, 24)], 1)
                op[1] = torch.tensor([border + 0.625, border + 0.625])
                op[2] = torch.tensor([border + 8.625, border + 8.625])
                al = op + eighth(-2, 2, 24, 2)
            elif f == F_NEGATIVE:                            # min - border = -3.5
                op[1] = torch.tensor([border - 3.5, border - 3.5])
                al[1] = op[1] + 1.0
            elif f == F_EDGES:                               # the box touches all four edges
                op[1], op[2] = torch.tensor([2.0, 3.0]), torch.tensor([W - 2.0, H - 1.0])
                al[1], al[2] = op[1] + 0.5, op[2] - 0.5
            elif f == F_ZERO_CONF:
                conf[:] = 0.0
            elif f == F_ALPHA_ONLY:                          # only AlphaPose's survive: the box must ignore them
                conf[0] = 0.0
            elif f == F_SPREAD:                              # AlphaPose reaches beyond OpenPose's extent; some pairs far apart
                op = torch.stack([eighth(70, 90, 24), eighth(40, 50, 24)], 1)
                al = op + eighth(-6, 6, 24, 2)
                al[4], al[5] = op[4] + torch.tensor([-40.0, 30.0]), op[5] + torch.tensor([60.0, -35.0])
                op[7], al[7] = torch.tensor([70.0, 40.0]), torch.tensor([W - 5.0, H - 5.0])               # > 100 px away
            if f in (F_GENERIC, F_SPREAD):
                conf[:, 1:3] = 0.5
                conf[:, 4:6] = 0.5
                conf[:, 7] = 0.5
            det[v, f, 0, :, :2], det[v, f, 1, :, :2], det[v, f, :, :, 2] = op, al, conf
    det = det.float()
    assert torch.equal(det[..., :2] * 8, (det[..., :2] * 8).round())
    for v, (H, W) in enumerate(SIZES):
        xy = det[v, ..., :2]
        assert bool((xy >= 0).all()) and bool((xy[..., 0] <= W).all()) and bool((xy[..., 1] <= H).all()), v
    return det


@functools.lru_cache(maxsize=None)
def hostile():
    """det (2, L, 2, 24, 3) fp32 with NaN, +-inf, +-1e30 and negative coordinates under non-zero confidence, and what each frame's
    status must say.  Frame 0: everything in the frame (status 0); 1: one NaN x; 2: every used keypoint non-finite (fallback);
    3: -1e30 and +1e30; 4: small negative and beyond the size; 5: one point exactly on the corner (W, H) and nothing else; 6: NaN
    confidence on a finite keypoint (used, as NaN != 0) and an inf y"""
    det = case(50).clone()
    nan, inf = float("nan"), float("inf")
    want = torch.zeros(2, L, dtype=torch.int32)
    for v, (H, W) in enumerate(SIZES):
        det[v, 0] = case(50)[v, F_SPREAD]
        det[v, 1] = case(50)[v, F_SPREAD]
        det[v, 1, :, 4, 0] = nan
        det[v, 2, 0, :, 0] = torch.tensor([nan, inf, -inf] * 8)
        det[v, 2, 1, :, 0] = torch.tensor([nan, inf, -inf] * 8)
        det[v, 2, :, :, 2] = 0.5
        det[v, 3] = case(50)[v, F_SPREAD]
        det[v, 3, :, 1, :2] = -1e30
        det[v, 3, :, 2, :2] = 1e30
        det[v, 4] = case(50)[v, F_SPREAD]
        det[v, 4, :, 1, :2] = torch.tensor([-7.5, -0.125])
        det[v, 4, :, 2, :2] = torch.tensor([W + 0.125, H + 300.0])
        det[v, 5, :, :, 2] = 0.0
        det[v, 5, :, 1] = torch.tensor([float(W), float(H), 0.5])
        det[v, 6] = case(50)[v, F_SPREAD]
        det[v, 6, :, 4, 2] = nan
        det[v, 6, :, 5, 1] = inf
        want[v] = torch.tensor([0, CLAMPED, CLAMPED | FALLBACK, CLAMPED, CLAMPED, 0, CLAMPED], dtype=torch.int32)
    return det, want


# ------------------------------------------------------------------------------------------------ the restatement
def _axis(vals, border, size, mut, rnd, upper_border=True):
    lo, hi = float(np.min(vals)) - border, float(np.max(vals)) + (border if upper_border else 0)
    p0 = rnd(lo) if rnd(lo) > 0 else 0
    p1 = rnd(hi) if rnd(hi) < size else size
    widened = p1 <= p0
    if widened:
        p0 = min(p0, size - 1)
        p1 = p0 + 1
    return p0, p1, widened


def ref_batch(det, a, n, border, agreement_px=AGREEMENT_PX, sizes=SIZES, principal=PRINCIPAL, mut=None, dtype=np.float64):
    """what apg_real_batch returns for frames [a, a + n): j2d, j2d_crop (2, n, 2, 24, 3), bb (2, n, 3) in `dtype` (np.float64: the
    reference; np.float32: the same expressions with every operation rounded to fp32), crops (2, n, 4), crop_info (2, n, 2, 2),
    status (2, n) int32, scale (2, n) float64 = 224 / max(h, w) unrounded"""
    assert mut is None or mut in MUTATIONS + EQUIVALENT, mut
    d = det.double().numpy()
    rnd = {"floor_not_trunc": math.floor, "round_not_trunc": lambda t: int(math.floor(t + 0.5))}.get(mut, int)
    out = dict(j2d=np.zeros((2, n, 2, 24, 3), dtype), j2d_crop=np.zeros((2, n, 2, 24, 3), dtype), bb=np.zeros((2, n, 3), dtype),
               crops=np.zeros((2, n, 4), np.int32), crop_info=np.zeros((2, n, 2, 2), np.int32), status=np.zeros((2, n), np.int32),
               scale=np.zeros((2, n), np.float64))
    for v in (0, 1):
        (H, W), c = sizes[v], np.asarray(principal[v], dtype)
        for i in range(n):
            op, al = d[v, a + i, 0].copy(), d[v, a + i, 1].copy()
            with np.errstate(invalid="ignore", over="ignore"):
                dist = np.sqrt((op[:, 0] - al[:, 0]) ** 2 + (op[:, 1] - al[:, 1]) ** 2)
                apart = dist >= agreement_px if mut == "agreement_ge" else dist > agreement_px
            op[apart, 2] = 0
            if mut != "filter_one_detector":
                al[apart, 2] = 0
            pts = op[op[:, 2] != 0, :2]
            if mut == "box_from_both_detectors":
                pts = np.concatenate([pts, al[al[:, 2] != 0, :2]])
            status = 0
            fin = np.isfinite(pts).all(1)                    # rule 1: a non-finite keypoint is absent
            inside = np.clip(pts[fin], [0, 0], [W, H])       # rule 2: clamped to the frame
            if not fin.all() or (inside != pts[fin]).any():
                status |= CLAMPED
            if len(inside) == 0:
                status |= FALLBACK
            if len(inside) == 0 and mut == "fallback_empty_is_whole_frame":
                x0, x1, y0, y1, wx, wy = 0, W, 0, H, False, False
            else:
                xs, ys = (inside[:, 0], inside[:, 1]) if len(inside) else (np.array([0.0]), np.array([0.0]))
                x0, x1, wx = _axis(xs, border, W, mut, rnd, upper_border=mut != "border_one_side")
                y0, y1, wy = _axis(ys, border, H, mut, rnd, upper_border=mut != "border_one_side")
            if wx or wy:                                     # rule 3
                status |= WIDENED
            centre = np.asarray([(x0 + x1) / 2, (y0 + y1) / 2], dtype)
            bb = centre / (np.asarray([W / 2, H / 2], dtype) if mut == "centre_over_size" else c) - dtype(1)
            h, w = y1 - y0, x1 - x0
            s64 = 224.0 / max(h, w)
            s = dtype(s64)
            off = (bb + dtype(1)) * c
            for k, p in enumerate((op, al)):
                out["j2d"][v, i, k] = p
                with np.errstate(invalid="ignore", over="ignore"):
                    out["j2d_crop"][v, i, k, :, :2] = s * (p[:, :2].astype(dtype) - off)
                out["j2d_crop"][v, i, k, :, 2] = p[:, 2]
            if mut == "crop_adds_pad":
                out["j2d_crop"][v, i, :, :, 0] += (224 - int(s64 * w)) // 2
                out["j2d_crop"][v, i, :, :, 1] += (224 - int(s64 * h)) // 2
            out["bb"][v, i] = (bb[0], bb[1], s)
            out["crops"][v, i] = (y0, y1, x0, x1)
            out["crop_info"][v, i] = ((y0, x0), (y1, x1))
            out["status"][v, i] = status
            out["scale"][v, i] = s64
    return out


def differs(got, ref):
    """the outputs of `got` (tensors or arrays) that are not what `ref` says: integers and confidences exactly, bb and j2d_crop by
    more than 1e-3 (far above any rounding, far below what a mutation moves)"""
    bad = []
    g = {k: np.asarray(v.cpu() if torch.is_tensor(v) else v) for k, v in got.items()}
    for k in ("crops", "crop_info", "status"):
        if not np.array_equal(g[k], ref[k]):
            bad.append(k)
    if not np.array_equal(g["j2d"][..., 2], ref["j2d"][..., 2].astype(np.float32)):
        bad.append("confidence")
    for k in ("bb", "j2d_crop"):
        with np.errstate(invalid="ignore"):
            if not (np.abs(g[k].astype(np.float64) - ref[k].astype(np.float64)) <= 1e-3).all():
                bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ the bars
def ulp32(x):
    """the spacing of fp32 at |x| (normal range)"""
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.where(x > 0, x, 1.0))) - 23), 2.0 ** -149)


def bb_bar(ref_bb):
    """bb = fl(fl(m / c) - 1) with m exact: half an ulp at q = bb + 1 from the divide and half an ulp at bb from the subtract.  This is
    what `2 ulp at the value's magnitude, one rounding in the divide and one in the subtract` comes to wherever |bb| >= |bb + 1| / 3;
    nearer 0 the divide's rounding, made at q's magnitude, is many ulps OF bb for every fp32 evaluation, the reference's own included,
    so there the bar keeps the two roundings where they are made.  Never wider than 2 ulp of max(|bb|, |bb + 1|)."""
    return 0.5 * ulp32(ref_bb + 1.0) + 0.5 * ulp32(ref_bb)


def crop_bar(smallest_side):
    """the fp32 chain r = s * (xy - (bb + 1) * c) at the sizes of this file: 2 ulp on u = bb + 1 < 4 (2 * 2^-22), carried through the
    product with c <= max principal coordinate; half an ulp of the product p = u c <= max frame side < 256 (2^-17); half an ulp of the
    difference |xy - p| < 256 (2^-17); all of it times the largest scale 224 / (smallest box side of the test)"""
    cmax = max(max(p) for p in PRINCIPAL)
    assert max(max(s) for s in SIZES) < 256 and all(W / cx < 4 and H / cy < 4 for (H, W), (cx, cy) in zip(SIZES, PRINCIPAL))
    return (224.0 / smallest_side) * (2 * 2.0 ** -22 * cmax + 2.0 ** -17 + 2.0 ** -17)
