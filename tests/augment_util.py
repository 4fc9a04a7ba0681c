"""Shared by tests/test_augment_abi.py, test_augment_fp64.py and test_augment_module.py: the contract of the crop augmentation
(include/airpose_grad.h, "Crop augmentation (augment.hip)") restated in numpy, three ways, plus the planted inputs.  CPU only.

  chain(..., dtype=np.float64)   the ORACLE: every stage in fp64 from the exact fp32 inputs, and with it a running error bar: each
                                 rounding the fp32 chain performs on an element adds 2^-24 |its result| (half an ulp, relative), and
                                 is carried to the output through the later stages' |coefficients| and the final 1 / std; the
                                 clamps are 1-Lipschitz and carry it unchanged, a filled occluder resets it to 0.
  chain(..., dtype=np.float32)   the RESTATEMENT: the same stages in numpy float32, one rounding per operation in the written order.
                                 Up to the first libm stage (gamma, noise) this is what the kernel must give BIT FOR BIT; `pre` is
                                 the fp32 value entering that stage.
  finish(pre, ...)               the libm stages, the occluders and the re-normalisation in fp64 from that fp32 `pre`, with the bar
                                 of the libm stages (see LIBM BARS below).
  draw(...)                      apg_augment_draw restated: the numpy Philox of synth_batch_util.py (imported, not copied), fp32
                                 ranges, the colour matrix and the taps composed in fp64 and rounded once.

LIBM BARS, in units of the output (every error of a de-normalised value v reaches the output through 1 / std):
  gamma: the ROCm device-library documentation with its ulp table is not installed beside the compiler this suite runs against, so
    powf counts as ULP_POWF = 2 ulp; times the margin 2 for the re-normalisation: 2 * ULP_POWF * ulp32(p) / std, p = pow(pre, gamma)
    in fp64.  That margin covers the two roundings of (p - mean) / std only while p is not small against mean: at p -> 0 the term
    vanishes while fl(fl(p - mean) / std) still rounds a number near -2.1 twice.  No arithmetic can beat that floor -- a CORRECTLY
    ROUNDED powf followed by the two fp32 operations misses the bare 2 * ULP_POWF * ulp32(p) / std on 7.9 % of the planted gamma
    image's elements, by up to 1.7e4 times -- so it is added in the oracle's own form: 2^-24 (|p - mean| / std + |out|).
  noise: sigma 2^-20 (1 + sqrt(-2 ln u1)) for the fp32 rounding of 2 pi u2 and the libm bounds, plus 2 ulp; the ulp is fp32's at
    1.0, the top of v's range (2^-23), since the chain's roundings (the product, the sum, the difference, the quotient) act on
    values of that range.  Both over std.
None of these is fitted to the kernel: they were written before it ran."""
import functools
import math

import numpy as np

from synth_batch_util import philox

IMG = 224
MEAN = np.asarray([0.485, 0.456, 0.406], np.float32)
STD = np.asarray([0.229, 0.224, 0.225], np.float32)
LUMA = np.asarray([0.299, 0.587, 0.114])
HUE_K = np.asarray([[0.168, 0.330, -0.497], [-0.328, 0.035, 0.292], [1.25, -1.05, -0.203]])
RMAX, NRECT, NCFG = 6, 4, 18                                 # include/airpose_grad.h: APG_AUG_*
BLUR_CLAMPED, NONFINITE, RECT_CLIPPED, BAD_BOX = 1, 2, 4, 8
U32 = 2.0 ** -24                                             # one fp32 rounding of v is at most U32 |v|
G2 = 1.0 + 2.0 ** -20                                        # the second-order terms of a first-order budget
ULP_POWF = 2.0
SEED = 0x9E3779B97F4A7C15                                   # both key words in use
KEYS = ("blur_taps", "color", "gamma", "noise_sigma", "rects", "rect_rgb")


def ulp32(x):
    """the spacing of fp32 at |x| (normal range)"""
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.where(x > 0, x, 1.0))) - 23), 2.0 ** -149)


def content_rect(crop):
    """preprocess_px.inc's letter-box of a crop box y0, y1, x0, x1 -> rows cy0 .. cy1 - 1, columns cx0 .. cx1 - 1 (empty: all 0)"""
    y0, y1, x0, x1 = (int(v) for v in crop)
    if y1 <= y0 or x1 <= x0:
        return 0, 0, 0, 0
    h, w = y1 - y0, x1 - x0
    scale = 224.0 / float(max(h, w))
    dw, dh = int(scale * w), int(scale * h)
    if dw == 0 or dh == 0:
        return 0, 0, 0, 0
    top, left = (224 - dh) // 2, (224 - dw) // 2
    return top, top + dh, left, left + dw


# ------------------------------------------------------------------------------------------------ the parameter set
def neutral(n):
    taps = np.zeros((2, n, RMAX + 1), np.float32)
    taps[..., 0] = 1
    color = np.zeros((2, n, 3, 4), np.float32)
    color[..., :3] = np.eye(3, dtype=np.float32)
    return dict(blur_taps=taps, color=color, gamma=np.ones((2, n, 3), np.float32), noise_sigma=np.zeros((2, n), np.float32),
                rects=np.zeros((2, n, NRECT, 4), np.int32), rect_rgb=np.zeros((2, n, NRECT, 3), np.float32))


def gauss_taps(sigma):
    """(taps fp32 (7,), clamped): fp64, r = min(ceil(3 sigma), 6), normalised, rounded once; sigma an fp32 value"""
    w = np.zeros(RMAX + 1, np.float32)
    w[0] = 1
    sd = float(np.float32(sigma))
    if not sd > 0:
        return w, False
    r = int(math.ceil(3.0 * sd))
    clamped = r > RMAX
    r = min(r, RMAX)
    e = [0.0] + [math.exp(-float(k * k) / (2.0 * sd * sd)) if k <= r else 0.0 for k in range(1, RMAX + 1)]
    total = 1.0
    for k in range(1, RMAX + 1):
        total += 2.0 * e[k]
    w[0] = np.float32(1.0 / total)
    for k in range(1, RMAX + 1):
        w[k] = np.float32(e[k] / total)
    return w, clamped


def luma_mix(t, u):
    """t L + u I in fp64, L's rows the luma weights"""
    return t * np.tile(LUMA, (3, 1)) + u * np.eye(3)


def hue_matrix(theta):
    cs, sn = math.cos(theta), math.sin(theta)
    return luma_mix(1.0 - cs, cs) + sn * HUE_K


def left_mul(a, m):
    """a m, row by column, summed left to right (the kernel's order)"""
    return np.asarray([[(a[r, 0] * m[0, c] + a[r, 1] * m[1, c]) + a[r, 2] * m[2, c] for c in range(3)] for r in range(3)])


def compose(gain=None, theta=None, sat=None, gray=None):
    """M in fp64: diag(gain), then the hue rotation, saturation and grayscale from the left, each only where given"""
    m = np.eye(3)
    if gain is not None:
        m = np.diag(np.asarray(gain, np.float64))
    if theta is not None:
        m = left_mul(hue_matrix(theta), m)
    if sat is not None:
        m = left_mul(luma_mix(1.0 - sat, sat), m)
    if gray is not None:
        m = left_mul(luma_mix(gray, 1.0 - gray), m)
    return m


def _uni(w):
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _range(w, lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    return np.float32(lo + _uni(w) * np.float32(hi - lo))


def words(seed, epoch, index, cam, k):
    """the four words of block k of (seed, epoch, dataset index, camera)"""
    return philox((int(index) & 0xFFFFFFFF, epoch & 0xFFFFFFFF, int(cam), k), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def draw(seed, epoch, index, cam0, cfg):
    """apg_augment_draw: index (n,) dataset indices, cam0 (n,) the camera under suffix 0, cfg the 18 floats -> the parameter set and
    status, (2, n, ...) indexed by suffix"""
    cfg = np.asarray(cfg, np.float32)
    assert cfg.shape == (NCFG,)
    n = len(index)
    o = neutral(n)
    o["status"] = np.zeros((2, n), np.int32)
    p = cfg[0]
    for s in (0, 1):
        for i in range(n):
            cam = (int(cam0[i]) & 1) ^ s
            d = {k: words(seed, epoch, index[i], cam, k) for k in range(1, 7)}
            on = lambda w: bool(_uni(w) < p)
            if (cfg[1] != 0 or cfg[2] != 0) and on(d[1][0]):
                o["blur_taps"][s, i], clamped = gauss_taps(_range(d[1][1], cfg[1], cfg[2]))
                o["status"][s, i] |= BLUR_CLAMPED if clamped else 0
            beta = _range(d[1][3], -cfg[3], cfg[3]) if cfg[3] != 0 and on(d[1][2]) else np.float32(0)
            gain = [float(_range(d[3][1 + c], cfg[7], cfg[8])) for c in range(3)] if (cfg[7] != 1 or cfg[8] != 1) and on(d[3][0]) else None
            theta = float(_range(d[2][1], -cfg[4], cfg[4])) * (3.141592653589793 / 180.0) if cfg[4] != 0 and on(d[2][0]) else None
            sat = float(_range(d[2][3], cfg[5], cfg[6])) if (cfg[5] != 1 or cfg[6] != 1) and on(d[2][2]) else None
            gray = float(_range(d[5][1], cfg[11], cfg[12])) if (cfg[11] != 0 or cfg[12] != 0) and on(d[5][0]) else None
            o["color"][s, i, :, :3] = compose(gain, theta, sat, gray).astype(np.float32)
            o["color"][s, i, :, 3] = beta
            if (cfg[13] != 0 or cfg[14] != 0) and on(d[5][2]):
                o["noise_sigma"][s, i] = _range(d[5][3], cfg[13], cfg[14])
            if (cfg[9] != 1 or cfg[10] != 1) and on(d[4][0]):
                o["gamma"][s, i] = [_range(d[4][1 + c], cfg[9], cfg[10]) for c in range(3)]
            count = int(cfg[15])
            if count > 0 and on(d[6][0]):
                for j in range(count):
                    b, c = words(seed, epoch, index[i], cam, 7 + j), words(seed, epoch, index[i], cam, 11 + j)
                    hy = int(np.float32(_range(b[0], cfg[16], cfg[17]) * np.float32(224)))
                    hx = int(np.float32(_range(b[1], cfg[16], cfg[17]) * np.float32(224)))
                    cy, cx = int(np.float32(_uni(b[2]) * np.float32(224))), int(np.float32(_uni(b[3]) * np.float32(224)))
                    y0, x0 = cy - hy // 2, cx - hx // 2
                    o["rects"][s, i, j] = (y0, y0 + hy, x0, x0 + hx)
                    o["rect_rgb"][s, i, j] = _uni(c[:3])
    return o


# ------------------------------------------------------------------------------------------------ the stages
def radius(taps):
    nz = np.nonzero(np.asarray(taps)[1:])[0]
    return int(nz[-1]) + 1 if len(nz) else 0


def skipped(p):
    """every stage of one image's parameters p (a dict of that image's slices) is skipped"""
    ident = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)], 1)
    rects = any(r[1] > r[0] and r[3] > r[2] and np.isfinite(c).all() for r, c in zip(p["rects"], p["rect_rgb"]))
    return radius(p["blur_taps"]) == 0 and np.array_equal(p["color"], ident) and (p["gamma"] == 1).all() and p["noise_sigma"] == 0 and not rects


def expected_status(crop, p):
    """the bits apg_augment_crops reports for one image"""
    st = 0
    if crop[1] <= crop[0] or crop[3] <= crop[2]:
        st |= BAD_BOX
    cy0, cy1, cx0, cx1 = content_rect(crop)
    if not (np.isfinite(p["blur_taps"]).all() and np.isfinite(p["color"]).all() and np.isfinite(p["noise_sigma"])):
        st |= NONFINITE
    if not ((np.asarray(p["gamma"]) >= 0) & np.isfinite(p["gamma"])).all():
        st |= NONFINITE
    for q, col in zip(p["rects"], p["rect_rgb"]):
        if q[1] > q[0] and q[3] > q[2]:
            if not np.isfinite(col).all():
                st |= NONFINITE
            elif cy1 > cy0 and (q[0] < cy0 or q[1] > cy1 or q[2] < cx0 or q[3] > cx1):
                st |= RECT_CLIPPED
    return st


def safe(p):
    """one image's parameters with every value the kernel treats as neutral (APG_AUG_NONFINITE) made neutral"""
    q = {k: np.array(v, copy=True) for k, v in p.items()}
    if not np.isfinite(q["blur_taps"]).all():
        q["blur_taps"] = np.asarray([1, 0, 0, 0, 0, 0, 0], np.float32)
    if not np.isfinite(q["color"]).all():
        q["color"] = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)], 1)
    q["gamma"] = np.where((q["gamma"] >= 0) & np.isfinite(q["gamma"]), q["gamma"], np.float32(1)).astype(np.float32)
    if not np.isfinite(q["noise_sigma"]):
        q["noise_sigma"] = np.float32(0)
    for k in range(NRECT):
        if not np.isfinite(q["rect_rgb"][k]).all():
            q["rects"][k], q["rect_rgb"][k] = 0, 0
    return q


def image_params(P, s, i):
    return {k: np.asarray(P[k])[s, i] for k in KEYS}


def _blur_pass(v, e, w, r, axis, T):
    """t = w_r p(-r), then t + w_|k| p(k) for k = -r + 1 .. r, coordinates clamped; e the error bar of v (fp64 only)"""
    size = v.shape[axis]
    t = te = None
    for k in range(-r, r + 1):
        at = np.clip(np.arange(size) + k, 0, size - 1)
        wk = T(w[abs(k)])
        prod = wk * np.take(v, at, axis)
        if e is not None:
            pe = abs(float(wk)) * np.take(e, at, axis) + U32 * np.abs(prod)
        if t is None:
            t, te = prod, (pe if e is not None else None)
        else:
            t = t + prod
            if e is not None:
                te = te + pe + U32 * np.abs(t)
    return t, te


def _noise_words(seed, epoch, index, cam, rect):
    cy0, cy1, cx0, cx1 = rect
    yy, xx = np.meshgrid(np.arange(cy0, cy1), np.arange(cx0, cx1), indexing="ij")
    pix = (yy * IMG + xx).astype(np.int64) | 0x80000000
    return philox((int(index) & 0xFFFFFFFF, epoch & 0xFFFFFFFF, int(cam), pix), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))   # (dh, dw, 4)


def box_muller(wd, T):
    """words (dh, dw, 4) -> z (3, dh, dw) and rho (3, dh, dw) in T: R, G from words (0, 1), B the cosine of words (2, 3)"""
    u1 = lambda w: ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = lambda w: (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    if T is np.float32:
        ra, rb = (np.sqrt(T(-2) * np.log(u1(wd[..., k]).astype(T))) for k in (0, 2))
        pa, pb = (T(6.2831855) * u2(wd[..., k]).astype(T) for k in (1, 3))
    else:
        ra, rb = (np.sqrt(-2.0 * np.log(u1(wd[..., k]))) for k in (0, 2))
        pa, pb = (2.0 * math.pi * u2(wd[..., k]) for k in (1, 3))
    return np.stack([ra * np.cos(pa), ra * np.sin(pa), rb * np.cos(pb)]), np.stack([ra, ra, rb])


def _rect_masks(p, rect):
    """[(mask over the content rectangle, colour clamped)] of the filled occluders, in order"""
    cy0, cy1, cx0, cx1 = rect
    yy, xx = np.meshgrid(np.arange(cy0, cy1), np.arange(cx0, cx1), indexing="ij")
    out = []
    for q, col in zip(p["rects"], p["rect_rgb"]):
        if q[1] > q[0] and q[3] > q[2] and np.isfinite(col).all():
            out.append(((yy >= q[0]) & (yy < q[1]) & (xx >= q[2]) & (xx < q[3]), np.clip(col, 0, 1)))
    return out


def finish(pre, p, rect, wd, T=np.float64):
    """from `pre` (3, dh, dw), the value entering the gamma stage: gamma, noise, occluders, re-normalisation in T.
    -> (out (3, dh, dw), the libm bar in units of the output -- fp64 only)"""
    v = np.asarray(pre, T)
    std, mean = STD.astype(T)[:, None, None], MEAN.astype(T)[:, None, None]
    bar = np.zeros(v.shape)
    gam, sig = np.asarray(p["gamma"], np.float32), np.float32(p["noise_sigma"])
    v = v.copy()
    for c in range(3):
        if gam[c] != 1:
            v[c] = np.power(np.clip(v[c], 0, 1), T(gam[c]))
            bar[c] += 2 * ULP_POWF * ulp32(v[c])
    if sig != 0:
        z, rho = box_muller(wd, T)
        v = np.clip(v + T(sig) * z, 0, 1)
        bar += abs(float(sig)) * 2.0 ** -20 * (1 + rho) + 2 * 2.0 ** -23
    filled = np.zeros(v.shape[1:], bool)
    for mask, col in _rect_masks(p, rect):
        for c in range(3):
            v[c][mask] = T(col[c])
        filled |= mask
    out = (v - mean) / std
    bar = bar / std.astype(np.float64)
    if sig == 0:                                             # the floor of the two last roundings (the module docstring)
        bar = bar + U32 * (np.abs(v - mean) / std + np.abs(out))
    bar[:, filled] = (U32 * (np.abs(v - mean) / std + np.abs(out)))[:, filled]
    return out, G2 * bar


def chain(x, crop, p, seed=SEED, epoch=0, index=0, cam=0, dtype=np.float64):
    """one image x (3, 224, 224) fp32 through the contract in `dtype`.  -> dict(out (3, 224, 224) float32 for the restatement,
    float64 for the oracle; copied: the image is a bit copy; rect: the content rectangle; pre (3, dh, dw): the value entering the
    gamma stage; libm: a gamma or noise stage runs; bar (3, 224, 224): the oracle's error bar, 0 on copied pixels; words)"""
    T = dtype
    x = np.asarray(x, np.float32)
    p = safe(p)
    rect = content_rect(crop)
    cy0, cy1, cx0, cx1 = rect
    res = dict(out=x.copy(), copied=True, rect=rect, pre=None, libm=False, bar=np.zeros(x.shape), words=None)
    if cy1 <= cy0 or skipped(p):
        return res                                           # (a copy is fp32 bits in either dtype)
    with np.errstate(invalid="ignore", over="ignore"):       # (the padding's bit patterns; only the content is compared in fp64)
        res["out"] = x.astype(T)
    res["copied"] = False
    track = T is np.float64
    std, mean = STD.astype(T)[:, None, None], MEAN.astype(T)[:, None, None]
    xs = x[:, cy0:cy1, cx0:cx1].astype(T)
    prod = xs * std
    v = prod + mean
    e = U32 * (np.abs(prod) + np.abs(v)) if track else None
    r = radius(p["blur_taps"])
    if r and np.isfinite(p["blur_taps"]).all():
        v, e = _blur_pass(v, e, p["blur_taps"], r, 2, T)
        v, e = _blur_pass(v, e, p["blur_taps"], r, 1, T)
    M = np.asarray(p["color"], np.float32)
    ident = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)], 1)
    if not np.array_equal(M, ident) and np.isfinite(M).all():
        Mt = M.astype(T)
        rows, errs = [], []
        for c in range(3):
            a, b, d = Mt[c, 0] * v[0], Mt[c, 1] * v[1], Mt[c, 2] * v[2]
            s1 = a + b
            s2 = s1 + d
            q = s2 + Mt[c, 3]
            rows.append(np.clip(q, 0, 1))
            if track:
                A = np.abs(M[c].astype(np.float64))
                errs.append(A[0] * e[0] + A[1] * e[1] + A[2] * e[2] + U32 * (np.abs(a) + np.abs(b) + np.abs(d) + np.abs(s1) + np.abs(s2) + np.abs(q)))
        v = np.stack(rows)
        e = np.stack(errs) if track else None
    res["pre"] = v
    res["libm"] = bool((np.asarray(p["gamma"]) != 1).any() or p["noise_sigma"] != 0)
    wd = _noise_words(seed, epoch, index, cam, rect) if p["noise_sigma"] != 0 else None
    res["words"] = wd
    out, _ = finish(v, p, rect, wd, T)
    res["out"][:, cy0:cy1, cx0:cx1] = out
    if track and not res["libm"]:
        filled = np.zeros(v.shape[1:], bool)
        for mask, col in _rect_masks(p, rect):
            filled |= mask
            v = v.copy()
            for c in range(3):
                v[c][mask] = col[c]
        e[:, filled] = 0
        bar = (e + U32 * np.abs(v - mean)) / std + U32 * np.abs(out)
        res["bar"][:, cy0:cy1, cx0:cx1] = G2 * bar
    return res


# ------------------------------------------------------------------------------------------------ the planted inputs
# crop boxes y0, y1, x0, x1 -> the letter-box inside the 224 x 224 image
BOX_WIDE = (10, 110, 20, 320)          # 100 x 300: rows 75 .. 148, every column: padding above and below, content over every tile seam
BOX_TALL = (0, 300, 5, 95)             # 300 x 90: columns 78 .. 144, every row: padding left and right
BOX_SQUARE = (7, 231, 3, 227)          # 224 x 224: no padding
BOX_ONE_ROW = (40, 42, 0, 300)         # 2 x 300: one content row (row 111), narrower than any blur radius
BOX_EMPTY = (40, 41, 0, 300)           # 1 x 300: dh = 0, no content
BOX_NARROW = (0, 300, 50, 55)          # 300 x 5: three content columns (110 .. 112), narrower than r = 6
BOXES = np.asarray([[BOX_WIDE, BOX_TALL, BOX_SQUARE], [BOX_ONE_ROW, BOX_EMPTY, BOX_NARROW]], np.int32)     # (suffix, sample)
INDEX = np.asarray([7, 123456, 2 ** 31 - 1], np.int32)
CAM0 = np.asarray([1, 0, 1], np.int32)


@functools.lru_cache(maxsize=None)
def planted_images():
    """(2, 3, 3, 224, 224) fp32: the content de-normalises to uniform [0, 1] with exact 0s and 1s among it (the clamp in front of
    powf), the padding holds arbitrary bit patterns (a NaN with a payload, -0, an infinity, denormals) that only a bit copy keeps"""
    g = np.random.default_rng(20240)
    v = g.uniform(0, 1, (2, 3, 3, IMG, IMG)).astype(np.float32)
    v[g.uniform(size=v.shape) < 0.01] = 0
    v[g.uniform(size=v.shape) < 0.01] = 1
    x = ((v - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32)
    odd = np.asarray([0x7FC01234, 0x80000000, 0x7F800000, 0x00000001, 0xFF800000, 0x3F800000], np.uint32).view(np.float32)
    for s in (0, 1):
        for i in range(3):
            cy0, cy1, cx0, cx1 = content_rect(BOXES[s, i])
            pad = np.ones((IMG, IMG), bool)
            pad[cy0:cy1, cx0:cx1] = False
            noise = g.integers(0, 2 ** 32, (3, IMG, IMG), dtype=np.uint64).astype(np.uint32).view(np.float32)
            noise[:, ::7, ::5] = odd[g.integers(0, len(odd), noise[:, ::7, ::5].shape)]
            x[s, i][:, pad] = noise[:, pad]
    return x


@functools.lru_cache(maxsize=None)
def planted_params():
    """(2, 3, ...) parameter sets, one image each (flattened order suffix-major):
      0 WIDE      r = 6, a matrix that drives values past both clamps, rects: inside, over the padding, overlapping, empty   libm-free
      1 TALL      r = 1, [I | 0], gamma (0.5, 2, 1), one rect                                                                gamma
      2 SQUARE    r = 0, a mild matrix, noise 0.03, one rect                                                                 noise
      3 ONE_ROW   r = 6 on one content row, a mild matrix with an offset                                                     libm-free
      4 EMPTY     everything on: the image must still be a copy
      5 NARROW    r = 6 on three content columns, gamma (2, 0.5, 0.5) and noise 0.03                                         gamma + noise"""
    P = neutral(3)
    t6, _ = gauss_taps(2.0)
    t1, _ = gauss_taps(0.3)
    assert radius(t6) == 6 and radius(t1) == 1
    strong = np.asarray([[12, -2, 2, -5.5], [-3, 16, -3, -4.5], [1, 1, 10, -5.5]], np.float32)          # 0.5 +- 0.5 round the blurred 0.5 +- 0.04
    mild = np.concatenate([compose([1.1, 0.9, 1.05], 0.4, 0.8, 0.25).astype(np.float32), np.full((3, 1), 0.03125, np.float32)], 1)
    P["blur_taps"][0, 0], P["color"][0, 0] = t6, strong
    P["rects"][0, 0] = [(90, 120, 30, 70), (60, 100, 150, 200), (100, 130, 50, 100), (140, 140, 10, 50)]
    P["rect_rgb"][0, 0] = [(0.25, 0.5, 0.75), (1.0, 0.0, 0.3), (0.1, 0.9, 0.6), (0.5, 0.5, 0.5)]
    P["blur_taps"][0, 1], P["gamma"][0, 1] = t1, (0.5, 2.0, 1.0)
    P["rects"][0, 1, 0], P["rect_rgb"][0, 1, 0] = (20, 60, 70, 100), (0.2, 0.4, 0.6)
    P["color"][0, 2], P["noise_sigma"][0, 2] = mild, 0.03
    P["rects"][0, 2, 1], P["rect_rgb"][0, 2, 1] = (200, 260, -20, 40), (0.7, 0.1, 0.2)
    P["blur_taps"][1, 0], P["color"][1, 0] = t6, mild
    P["blur_taps"][1, 1], P["color"][1, 1], P["gamma"][1, 1], P["noise_sigma"][1, 1] = t6, strong, (0.5, 0.5, 2.0), 0.03
    P["rects"][1, 1, 0], P["rect_rgb"][1, 1, 0] = (0, 224, 0, 224), (0.5, 0.5, 0.5)
    P["blur_taps"][1, 2], P["gamma"][1, 2], P["noise_sigma"][1, 2] = t6, (2.0, 0.5, 0.5), 0.03
    return P


def rolled(P, k):
    """the same six parameter sets, moved on by k images: every box meets every set over k = 0 .. 5"""
    return {key: np.roll(np.asarray(v).reshape((6,) + v.shape[2:]), k, 0).reshape(v.shape) for key, v in P.items()}


def worst(err, bar):
    """max err / bar; where the bar is 0 (a copied pixel) the error must be 0"""
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    assert (err[bar == 0] == 0).all()
    return float(np.divide(err, bar, out=np.zeros_like(err), where=bar > 0).max()) if err.size else 0.0


def check_image(got, x, crop, p, seed, epoch, index, cam, detail=None):
    """one image of the kernel's output against the contract.  -> (kind, worst error / bar): kind is "copy" (bit-identical to the
    input), "exact" (bit-identical to the restatement AND within the oracle's bar), "gamma", "noise" or "gamma+noise" (within the libm
    bar of fp64 from the restatement's fp32 `pre`).  Padding pixels are compared bit for bit in every kind."""
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    p = safe(p)
    r32 = chain(x, crop, p, seed, epoch, index, cam, np.float32)
    cy0, cy1, cx0, cx1 = r32["rect"]
    pad = np.ones((IMG, IMG), bool)
    pad[cy0:cy1, cx0:cx1] = False
    assert np.array_equal(bits(got)[:, pad], bits(x)[:, pad]), "padding pixels are not a bit copy"
    if r32["copied"]:
        assert np.array_equal(bits(got), bits(x)), "the image is not a bit copy"
        return "copy", 0.0
    inner = got[:, cy0:cy1, cx0:cx1].astype(np.float64)
    if not r32["libm"]:
        assert np.array_equal(bits(got), bits(r32["out"])), "differs from the fp32 restatement in %d elements" % (bits(got) != bits(r32["out"])).sum()
        r64 = chain(x, crop, p, seed, epoch, index, cam, np.float64)
        return "exact", worst(np.abs(inner - r64["out"][:, cy0:cy1, cx0:cx1]), r64["bar"][:, cy0:cy1, cx0:cx1])
    want, bar = finish(r32["pre"], p, r32["rect"], r32["words"], np.float64)
    kind = "+".join(k for k, on in (("gamma", (np.asarray(p["gamma"]) != 1).any()), ("noise", p["noise_sigma"] != 0)) if on)
    if detail is not None:                                   # the same ratio over the elements a libm call reaches: off the occluders and
        free = np.ones(inner.shape, bool)                    # the channels with gamma = 1, whose bar is the bare two-rounding floor
        for mask, _ in _rect_masks(p, r32["rect"]):
            free[:, mask] = False
        if p["noise_sigma"] == 0:
            free[np.asarray(p["gamma"]) == 1] = False
        detail["libm"] = worst(np.abs(inner - want)[free], bar[free])
    return kind, worst(np.abs(inner - want), bar)
