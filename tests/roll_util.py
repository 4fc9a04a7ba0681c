"""Shared by tests/test_roll_abi.py, test_roll_fp64.py and test_roll_module.py: the contract of the camera roll
(include/airpose_grad.h, "Camera roll (roll.hip)") restated in numpy, twice from ONE text, plus the planted inputs.  CPU only.

The chain is written once, with + - * / on its operands; what the operands are decides what it computes:
  np.float32 arrays   the RESTATEMENT: one rounding per operation in the written order.  roll.hip is compiled without contraction, so
                      this is what the kernels must give BIT FOR BIT, labels and pixels alike.
  E(value, bound)     the ORACLE: the value in fp64 from the exact fp32 inputs, and beside it a running bound on what the fp32 chain
                      may have drifted from it.  Every operation propagates its operands' bounds to first order with the cross term
                      (|a| e_b + |b| e_a + e_a e_b for a product, e_a + e_b for a sum, (e_a + |a / b| e_b) / (|b| - e_b) for a
                      quotient) and then adds its own rounding, 2^-24 (|result| + bound): half an ulp of the largest value the fp32
                      result can have.  Nothing is fitted to the kernel: the bars were written before it ran.
For a pixel the chain gives the sampling position q with its bound e_q; the value's bar is then
  e_qx Lx + e_qy Ly     the position error times the local slope of the zero-continued bilinear surface: Lx (Ly) is the largest
                        |difference of horizontally (vertically) adjacent taps| over the 3 x 3 cells round q's cell (e_q < 1 pixel is
                        asserted), which bounds the surface's slope wherever q32 may lie, cell seams and the canvas edge included;
  + 7 * 2^-24 M         the interpolation's own roundings -- byte / 255, 1 - a_x, the product, the sum, 1 - a_y, the product, the sum
                        -- on a convex combination of taps that are at most M, the largest tap of the 4 x 4 neighbourhood;
  then through (v - mean) / std: (e_v + 2^-24 |v - mean|) / std + 2^-24 |out|.
The discrete decisions (the refusal, the status bits) are the float32 restatement's: the oracle is given the (c, sn) in force."""
import numpy as np

from synth_batch_util import philox

IMG = 224
MEAN = np.asarray([0.485, 0.456, 0.406], np.float32)
STD = np.asarray([0.229, 0.224, 0.225], np.float32)
CENTRE_OUT, OFF_CANVAS = 1, 2                                # include/airpose_grad.h: APG_ROLL_*
BLOCK = 15                                                   # the draw's counter block
U32 = 2.0 ** -24
G2 = 1.0 + 2.0 ** -20                                        # the second-order terms of the pixel's first-order budget
TINY = 2.0 ** -149
SEED = 0x9E3779B97F4A7C15
F = np.float32
LABEL_KEYS = ("verts", "joints", "orient", "trans", "extr", "j2d", "j2d_crop")


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.where(x > 0, x, 1.0))) - 23), 2.0 ** -149)


def worst(err, bar):
    """the largest error / bar; an error on a zero bar counts as infinite"""
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.max(r))


# ------------------------------------------------------------------------------------------------ the oracle's operand
class E(object):
    """a value in fp64 and a bound on |the fp32 chain's value - it|"""
    __array_ufunc__ = None                                   # numpy scalars defer to __rmul__ and its kin

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def _round(v, e):
        return E(v, e + U32 * (np.abs(v) + e) + TINY)

    def __mul__(self, o):
        o = E.lift(o)
        return E._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __add__(self, o):
        o = E.lift(o)
        return E._round(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o)
        return E._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o) - self

    def __truediv__(self, o):
        o = E.lift(o)
        v = self.v / o.v
        den = np.abs(o.v) - o.e
        assert (den > 0).all(), "a divisor whose bound reaches zero"
        return E._round(v, (self.e + np.abs(v) * o.e) / den)

    def __getitem__(self, k):
        return E(self.v[k], self.e[k])


def stack(parts, axis=-1):
    if isinstance(parts[0], E):
        return E(np.stack([p.v for p in parts], axis), np.stack([p.e for p in parts], axis))
    return np.stack(parts, axis)


def ncol(a):
    return (a.v if isinstance(a, E) else a).shape[-1]


# ------------------------------------------------------------------------------------------------ the chain, written once
class Turn(object):
    def __init__(self, c, sn, K):
        self.c, self.sn, self.cx, self.cy = c, sn, K[0, 2], K[1, 2]
        if not isinstance(c, E) and c == 1 and sn == 0:      # an un-rolled row: exactly 0, whatever intr holds
            self.tx = self.ty = F(0)
            return
        with np.errstate(all="ignore"):
            kx, ky = K[0, 0] / K[1, 1], K[1, 1] / K[0, 0]
            self.tx, self.ty = sn * kx, sn * ky


def fwd(t, x, y):
    return (t.c * x) - (t.tx * y), (t.ty * x) + (t.c * y)


def back(t, x, y):
    return (t.c * x) + (t.tx * y), (t.c * y) - (t.ty * x)


def rz(t, x, y):
    return (t.c * x) - (t.sn * y), (t.sn * x) + (t.c * y)


def decide(rot, K, bb):
    """float32: -> (c, sn) in force, bb', the status's CENTRE_OUT"""
    c, sn = F(rot[0]), F(rot[1])
    if c == 1 and sn == 0:
        return F(1), F(0), bb.copy(), 0
    K, bb = K.astype(F), bb.astype(F)
    t = Turn(c, sn, K)
    with np.errstate(all="ignore"):
        u, v = fwd(t, bb[0] * t.cx, bb[1] * t.cy)
        nx, ny = u / t.cx, v / t.cy
    if not (abs(nx) <= 1 and abs(ny) <= 1):
        return F(1), F(0), bb.copy(), CENTRE_OUT
    return c, sn, np.asarray([nx, ny, bb[2]], F), 0


def off_canvas(c, sn, K, box, Hc, Wc):
    """float32: the status's OFF_CANVAS of the (c, sn) in force"""
    t = Turn(F(c), F(sn), K.astype(F))
    y0, y1, x0, x1 = (int(v) for v in box)
    hh, hw = F(y1 - y0) * F(0.5), F(x1 - x0) * F(0.5)
    my, mx = F(y0) + hh, F(x0) + hw
    off = False
    for k in range(4):
        ux, uy = (hw if k & 1 else -hw), (hh if k & 2 else -hh)
        rx, ry = back(t, ux, uy)
        qx, qy = mx + rx, my + ry
        off = off or not (qx >= 0 and qx <= F(Wc) and qy >= 0 and qy <= F(Hc))
    return OFF_CANVAS if off else 0


def roll_labels(c, sn, K, labels, oracle=False):
    """one (sample, view): labels {name: fp32 array} -> the rolled ones, float32 arrays (the restatement) or E (the oracle); (c, sn)
    is the pair IN FORCE (after the refusal)"""
    ident = c == 1 and sn == 0
    W = (lambda a: E(np.asarray(a, F))) if oracle else (lambda a: np.asarray(a, F))
    out = {}
    if ident:
        return {k: W(v) for k, v in labels.items()}
    t = Turn(W(c), W(sn), W(K))
    for name, a in labels.items():
        a = W(a)
        if name in ("verts", "joints", "trans"):
            x, y = rz(t, a[..., 0], a[..., 1])
            out[name] = stack([x, y, a[..., 2]])
        elif name == "orient":                               # per column: rows 0 and 1 mixed
            x, y = rz(t, a[0, :], a[1, :])
            out[name] = stack([x, y, a[2, :]], 0)
        elif name == "extr":
            x, y = rz(t, a[0, :], a[1, :])
            out[name] = stack([x, y, a[2, :], a[3, :]], 0)
        elif name == "j2d":
            u, v = fwd(t, a[..., 0] - t.cx, a[..., 1] - t.cy)
            out[name] = stack([t.cx + u, t.cy + v] + ([a[..., 2]] if ncol(a) == 3 else []))
        elif name == "j2d_crop":
            u, v = fwd(t, a[..., 0], a[..., 1])
            out[name] = stack([u, v] + ([a[..., 2]] if ncol(a) == 3 else []))
    return out


def letter_box(box):
    y0, y1, x0, x1 = (int(v) for v in box)
    h, w = y1 - y0, x1 - x0
    scale = 224.0 / float(max(h, w))
    dw, dh = int(scale * w), int(scale * h)
    return h, w, dw, dh, (224 - dh) // 2, (224 - dw) // 2


def _positions(box):
    """preprocess_px.inc's source position before the floor, in fp64 (each operation rounded once), and the content mask"""
    h, w, dw, dh, top, left = letter_box(box)
    oy, ox = np.mgrid[0:IMG, 0:IMG]
    dy, dx = oy - top, ox - left
    content = (dy >= 0) & (dy < dh) & (dx >= 0) & (dx < dw)
    if not content.any():
        return content, None, None
    sxd, syd = 1.0 / (float(dw) / float(w)), 1.0 / (float(dh) / float(h))
    return content, (dx + 0.5) * sxd - 0.5, (dy + 0.5) * syd - 0.5


def _window_max(a, rows, cols):
    """out[r, k] = max of a[r + dr, k + dk] over dr in rows, dk in cols (zero beyond the array)"""
    H, Wd = a.shape[:2]
    lo_r, hi_r, lo_c, hi_c = -min(rows), max(rows), -min(cols), max(cols)
    p = np.pad(a, ((lo_r, hi_r), (lo_c, hi_c)) + ((0, 0),) * (a.ndim - 2))
    out = np.zeros_like(a)
    for dr in rows:
        for dk in cols:
            out = np.maximum(out, p[lo_r + dr:lo_r + dr + H, lo_c + dk:lo_c + dk + Wd])
    return out


def roll_image(frame, box, c, sn, K, bgr, oracle=False):
    """one ROLLED (sample, view): frame (Hc, Wc, 3) uint8 -> (3, 224, 224): float32 (the restatement), or (value fp64, bar)"""
    Hc, Wc = frame.shape[:2]
    y0, y1, x0, x1 = (int(v) for v in box)
    h, w = y1 - y0, x1 - x0
    content, fx64, fy64 = _positions(box)
    src = frame[:, :, ::-1] if bgr else frame
    mean, std = (MEAN, STD) if not oracle else (MEAN.astype(np.float64), STD.astype(np.float64))
    if fx64 is None:
        v = np.zeros((IMG, IMG, 3), np.float64 if oracle else F)
        if oracle:
            val = (v - mean) / std
            return val.transpose(2, 0, 1), (U32 * np.abs(val) * G2).transpose(2, 0, 1)
        return ((v - mean) / std).transpose(2, 0, 1)
    hw, hh = F(w) * F(0.5), F(h) * F(0.5)
    if not oracle:
        t = Turn(F(c), F(sn), K.astype(F))
        with np.errstate(all="ignore"):
            rx, ry = back(t, fx64.astype(F) - hw, fy64.astype(F) - hh)
            qx, qy = (F(x0) + hw) + rx, (F(y0) + hh) + ry
            inside = (qx > -1) & (qx < F(Wc)) & (qy > -1) & (qy < F(Hc)) & content
            flx, fly = np.floor(qx), np.floor(qy)
            ix, iy = np.where(inside, flx, 0).astype(np.int64), np.where(inside, fly, 0).astype(np.int64)
            ax, ay = qx - flx, qy - fly
            T = np.zeros((Hc + 2, Wc + 2, 3), F)
            T[1:-1, 1:-1] = src.astype(F) / F(255)
            one = F(1)
            t00, t01, t10, t11 = T[iy + 1, ix + 1], T[iy + 1, ix + 2], T[iy + 2, ix + 1], T[iy + 2, ix + 2]
            wx0, wx1, wy0, wy1 = (one - ax)[..., None], ax[..., None], (one - ay)[..., None], ay[..., None]
            topv, botv = (t00 * wx0) + (t01 * wx1), (t10 * wx0) + (t11 * wx1)
            v = np.where(inside[..., None], (topv * wy0) + (botv * wy1), F(0)).astype(F)
        return ((v - mean) / std).astype(F).transpose(2, 0, 1)
    # the oracle
    t = Turn(E(F(c)), E(F(sn)), E(K.astype(F)))
    fx, fy = E(fx64, U32 * np.abs(fx64) + 2.0 ** -50 * (1 + np.abs(fx64))), E(fy64, U32 * np.abs(fy64) + 2.0 ** -50 * (1 + np.abs(fy64)))
    rx, ry = back(t, fx - E(hw), fy - E(hh))
    qx, qy = (E(F(x0)) + E(hw)) + rx, (E(F(y0)) + E(hh)) + ry
    # a = q - floor(q) rounds once more where q lies in (-1, 0): a position error like the others
    eqx, eqy = qx.e + U32 * 1.0, qy.e + U32 * 1.0
    assert eqx[content].max() < 1 and eqy[content].max() < 1
    PAD = 4
    T = np.zeros((Hc + 2 * PAD, Wc + 2 * PAD, 3))
    T[PAD:-PAD, PAD:-PAD] = src.astype(np.float64) / 255.0
    flx, fly = np.clip(np.floor(qx.v), -2, Wc), np.clip(np.floor(qy.v), -2, Hc)
    ax, ay = np.clip(qx.v - flx, 0, 1)[..., None], np.clip(qy.v - fly, 0, 1)[..., None]
    ix, iy = flx.astype(np.int64) + PAD, fly.astype(np.int64) + PAD
    top_ = T[iy, ix] * (1 - ax) + T[iy, ix + 1] * ax
    bot_ = T[iy + 1, ix] * (1 - ax) + T[iy + 1, ix + 1] * ax
    v = top_ * (1 - ay) + bot_ * ay
    DX = np.zeros_like(T)
    DX[:, :-1] = np.abs(T[:, 1:] - T[:, :-1])                # DX[r, k] = |T[r, k + 1] - T[r, k]|
    DY = np.zeros_like(T)
    DY[:-1] = np.abs(T[1:] - T[:-1])
    Lx = _window_max(DX, (-1, 0, 1, 2), (-1, 0, 1))[iy, ix]
    Ly = _window_max(DY, (-1, 0, 1), (-1, 0, 1, 2))[iy, ix]
    M = _window_max(T, (-1, 0, 1, 2), (-1, 0, 1, 2))[iy, ix]
    ev = eqx[..., None] * Lx + eqy[..., None] * Ly + 7 * U32 * M
    v = np.where(content[..., None], v, 0.0)
    ev = np.where(content[..., None], ev, 0.0)
    val = (v - mean) / std
    bar = ((ev + U32 * np.abs(v - mean)) / std * (1 + 2 * U32) + U32 * np.abs(val) + TINY) * G2
    return val.transpose(2, 0, 1), bar.transpose(2, 0, 1)


# ------------------------------------------------------------------------------------------------ the draw
def draw(seed, epoch, index, cam0, p, max_rad):
    """apg_roll_draw: -> gate (2, n) bool, the fp32 angle (2, n), and (cos, sin) (2, n, 2) in fp64 of that fp32 angle"""
    index = np.asarray(index, np.int64)
    cam = np.stack([(np.asarray(cam0) & 1) ^ s for s in (0, 1)])
    w = philox((index[None, :] & 0xFFFFFFFF, epoch & 0xFFFFFFFF, cam, BLOCK), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = (w >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    gate = u[..., 0] < F(p)
    ang = ((F(2) * u[..., 1]) - F(1)) * F(max_rad)
    ang = np.where(gate, ang, F(0)).astype(F)
    a64 = ang.astype(np.float64)
    return gate, ang, np.stack([np.cos(a64), np.sin(a64)], -1)


# ------------------------------------------------------------------------------------------------ the planted case
N, V, J, P, PS = 3, 5, 3, 4, 3
SIZES = ((96, 128), (61, 47))                                # (Hc, Wc) of camera 0 and camera 1
CAM0 = np.asarray([0, 1, 0], np.int32)                       # the camera under suffix 0
# y0, y1, x0, x1 per (suffix, sample), each on its camera's canvas: wide, tall, the full canvas / one row, three columns, a square
BOXES = np.asarray([[(30, 50, 10, 110), (5, 55, 20, 35), (0, 96, 0, 128)],
                    [(30, 31, 3, 44), (10, 90, 60, 63), (8, 48, 4, 44)]], np.int32)
DEG = np.pi / 180
# (0, 0) trips CENTRE_OUT (its principal point is planted for it), (0, 2) rolls the full canvas (OFF_CANVAS), (1, 2) is (1, 0)
ANGLES = np.asarray([[80 * DEG, 7 * DEG, 90 * DEG], [-7 * DEG, 179 * DEG, 0.0]])


def camera_of(s, i):
    return (int(CAM0[i]) & 1) ^ s


def case():
    """the planted inputs of tests/test_roll_fp64.py, all float32 / int32 / uint8 numpy"""
    g = np.random.default_rng(20241021)
    frames = [g.integers(0, 256, (N,) + SIZES[c] + (3,), dtype=np.uint8) for c in (0, 1)]
    rot = np.stack([np.cos(ANGLES), np.sin(ANGLES)], -1).astype(F)
    rot[1, 2] = (1, 0)
    intr = np.zeros((2, N, 3, 3), F)
    bb = np.zeros((2, N, 3), F)
    for s in (0, 1):
        for i in range(N):
            cam = camera_of(s, i)
            Hc, Wc = SIZES[cam]
            fx, fy = (1475.0, 1475.0) if cam == 0 else (410.0, 395.5)          # fx != fy in camera 1
            cx, cy = (Wc / 2 + 1.25, Hc / 2 - 0.75)
            if (s, i) == (0, 0):
                cx, cy = 100.0, 30.0                         # the box centre (60, 40) turned by 80 degrees leaves +-cy
            intr[s, i] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
            y0, y1, x0, x1 = BOXES[s, i]
            K = intr[s, i]
            bb[s, i] = [F(F(F(x0 + x1) / F(2)) / K[0, 2]) - F(1), F(F(F(y0 + y1) / F(2)) / K[1, 2]) - F(1), F(224.0 / max(y1 - y0, x1 - x0))]
    lab = dict(verts=g.normal(0, 1, (2, N, V, 3)) + (0, 0, 6), joints=g.normal(0, 1, (2, N, J, 3)) + (0, 0, 6),
               orient=g.normal(0, 1, (2, N, 3, 3)), trans=g.normal(0, 2, (2, N, 3)), extr=g.normal(0, 3, (2, N, 4, 4)),
               j2d=g.uniform(-20, 140, (2, N, P, PS)), j2d_crop=g.uniform(-150, 150, (2, N, P, PS)))
    lab = {k: v.astype(F) for k, v in lab.items()}
    lab["verts"][0, 1, 0] = (-0.0, -3.0, 2.0)                # a negative zero: only a copy keeps it under (1, 0)
    lab["verts"][1, 2, 0] = (-0.0, -3.0, 2.0)
    return dict(frames=frames, rot=rot, intr=intr, bb=bb, crops=BOXES.copy(), cam=CAM0.copy(), sizes=SIZES, labels=lab)


def restate(case_, rows=None):
    """the float32 restatement of apg_roll_labels for the whole case: rot_used, bb_out, status, the labels"""
    n = case_["rot"].shape[1]
    out = dict(rot_used=np.zeros((2, n, 2), F), bb_out=np.zeros((2, n, 3), F), status=np.zeros((2, n), np.int32),
               labels={k: np.zeros_like(v) for k, v in case_["labels"].items()})
    for s in (0, 1):
        for i in range(n):
            K = case_["intr"][s, i]
            c, sn, nbb, st = decide(case_["rot"][s, i], K, case_["bb"][s, i])
            cam = (int(case_["cam"][i]) & 1) ^ s
            st |= off_canvas(c, sn, K, case_["crops"][s, i], *case_["sizes"][cam])
            out["rot_used"][s, i], out["bb_out"][s, i], out["status"][s, i] = (c, sn), nbb, st
            r = roll_labels(c, sn, K, {k: v[s, i] for k, v in case_["labels"].items()})
            for k, v in r.items():
                out["labels"][k][s, i] = v
    return out
