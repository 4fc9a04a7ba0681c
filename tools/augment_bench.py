"""Time airpose_amd.CropAugment at the trainers' size: n = 64 samples, both views, 2 n crops of 3 x 224 x 224 whose boxes are a
person's (about 250 x 500 px: a tall letter-box with padding left and right), every stage on with the class's default ranges.

  call        CropAugment.__call__ on a SyntheticBatches-style dict: apg_augment_draw + apg_augment_crops (two launches)
  apply       CropAugment.apply alone, on parameters drawn before
  eager       the arithmetic of apg_augment_crops (include/airpose_grad.h) in eager torch on the device, from the SAME drawn parameters:
              the letter-box from the boxes, de-normalise, the separable blur as 13 + 13 clamped gathers, the colour matrix, gamma, the
              per-pixel Philox and Box-Muller in int64 / fp32 tensors, the occluders, re-normalise, the padding kept by torch.where.
              It draws nothing: the draw would add to it.
  copy        out.copy_(im): the bytes the augmentation must read and write, 2 * (2 n * 3 * 224^2 * 4), moved by a plain device copy
  *_ops       an OPERATOR count per call as in tools/loss_bench.py: every aten operator outside LaunchCount.VIEWS counts one, every
              call of a C entry point of the library counts one

The four take turns in one process (HIP events around --reps calls, the median of --windows windows and their max - min).  Before
anything is timed the kernel's output is compared with the eager path's (1e-4: eager torch may fuse a product into a sum, and its
powf / logf / cosf are other code than the kernel's).  One JSON line; --out also writes it to a file.

    python tools/augment_bench.py [--n 64] [--out profiles/augment_bench.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd.augment import CropAugment  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402

IMG = 224
MASK = 0xFFFFFFFF
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def synthetic(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    x0, y0 = (r(2, n) * 1600).int(), (r(2, n) * 500).int()
    w, h = (200 + r(2, n) * 100).int(), (400 + r(2, n) * 150).int()
    crops = torch.stack([y0, y0 + h, x0, x0 + w], -1).int()                               # (2, n, 4)
    mean, std = torch.tensor(MEAN).reshape(3, 1, 1), torch.tensor(STD).reshape(3, 1, 1)
    v = r(2, n, 3, IMG, IMG)
    side = torch.maximum(h, w).double()
    scale = torch.full_like(side, 224.0) / side              # (224.0 / tensor is reciprocal * 224 in torch: two roundings, not the kernels' one)
    dw, dh = (scale * w).long(), (scale * h).long()
    ar = torch.arange(IMG)
    cols = (ar >= ((IMG - dw) // 2)[..., None]) & (ar < ((IMG - dw) // 2 + dw)[..., None])
    rows = (ar >= ((IMG - dh) // 2)[..., None]) & (ar < ((IMG - dh) // 2 + dh)[..., None])
    v = v * (rows[..., :, None] & cols[..., None, :])[:, :, None]                         # zero padding, as the crop kernels leave it
    im = (v - mean) / std
    batch = {"im0": None, "im1": None, "cam0": (r(n) < 0.5).int().to(dev)}
    im, crops = im.to(dev), crops.to(dev)
    for s in (0, 1):
        batch["im%d" % s], batch["crops%d" % s] = im[s], crops[s]
    return batch, im, crops, torch.arange(1000, 1000 + n, dtype=torch.int32).to(dev)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on int64 tensors holding 32-bit words"""
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57            # (wraps mod 2^64: the low 64 bits are the product's)
        c0, c1, c2, c3 = ((p1 >> 32) & MASK) ^ c1 ^ k0, p1 & MASK, ((p0 >> 32) & MASK) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def eager_apply(im, crops, P, index, cam0, seed, epoch):
    dev = im.device
    n = im.shape[1]
    B = 2 * n
    x = im.reshape(B, 3, IMG, IMG)
    mean, std = torch.tensor(MEAN, device=dev).reshape(1, 3, 1, 1), torch.tensor(STD, device=dev).reshape(1, 3, 1, 1)
    c = crops.reshape(B, 4).double()
    h, w = c[:, 1] - c[:, 0], c[:, 3] - c[:, 2]
    side = torch.maximum(h, w)
    scale = torch.full_like(side, 224.0) / side              # one rounding, as preprocess_px.inc's 224.0 / (double)max(h, w)
    dw, dh = (scale * w).long(), (scale * h).long()
    cy0, cx0 = (IMG - dh) // 2, (IMG - dw) // 2
    cy1, cx1 = cy0 + dh, cx0 + dw
    ar = torch.arange(IMG, device=dev)
    rows, cols = (ar >= cy0[:, None]) & (ar < cy1[:, None]), (ar >= cx0[:, None]) & (ar < cx1[:, None])
    content = (rows[:, :, None] & cols[:, None, :])[:, None]                               # (B, 1, 224, 224)
    taps, M = P["blur_taps"].reshape(B, 7), P["color"].reshape(B, 3, 4)
    gam, sig = P["gamma"].reshape(B, 3, 1, 1), P["noise_sigma"].reshape(B, 1, 1, 1)
    rects, rgb = P["rects"].reshape(B, 4, 4), P["rect_rgb"].reshape(B, 4, 3).clamp(0, 1)
    v = x * std + mean
    for axis, lo, hi in ((3, cx0, cx1), (2, cy0, cy1)):      # the separable blur, coordinates clamped to the letter-box
        acc = None
        for k in range(-6, 7):
            at = torch.minimum(torch.maximum(ar[None] + k, lo[:, None]), hi[:, None] - 1).clamp(0, IMG - 1)
            at = at[:, None, None, :].expand(B, 3, IMG, IMG) if axis == 3 else at[:, None, :, None].expand(B, 3, IMG, IMG)
            term = taps[:, abs(k)].reshape(B, 1, 1, 1) * torch.gather(v, axis, at)
            acc = term if acc is None else acc + term
        v = acc
    ident = torch.eye(3, 4, device=dev)
    q = ((M[:, :, 0, None, None] * v[:, 0:1] + M[:, :, 1, None, None] * v[:, 1:2]) + M[:, :, 2, None, None] * v[:, 2:3]) + M[:, :, 3, None, None]
    v = torch.where((M != ident).any(-1).any(-1).reshape(B, 1, 1, 1), q.clamp(0, 1), v)
    v = torch.where(gam != 1, torch.pow(v.clamp(0, 1), gam), v)
    idx = (index.long() & MASK).repeat(2).reshape(B, 1, 1)
    cam = torch.cat([cam0 & 1, (cam0 & 1) ^ 1]).long().reshape(B, 1, 1)
    pix = (ar[:, None] * IMG + ar[None, :]).long()[None] | 0x80000000
    w0, w1, w2, w3 = philox(idx + 0 * pix, epoch + 0 * pix, cam + 0 * pix, pix + 0 * idx, seed & MASK, (seed >> 32) & MASK)
    u1 = lambda t: ((t >> 8) + 1).float() * 2.0 ** -24
    u2 = lambda t: (t >> 8).float() * 2.0 ** -24
    ra, rb = torch.sqrt(-2 * torch.log(u1(w0))), torch.sqrt(-2 * torch.log(u1(w2)))
    pa, pb = 6.2831855 * u2(w1), 6.2831855 * u2(w3)
    z = torch.stack([ra * torch.cos(pa), ra * torch.sin(pa), rb * torch.cos(pb)], 1)
    v = torch.where(sig != 0, (v + sig * z).clamp(0, 1), v)
    filled = torch.zeros(B, 1, 1, 1, dtype=torch.bool, device=dev)
    for k in range(4):
        y0, y1, x0, x1 = (rects[:, k, e].reshape(B, 1, 1, 1) for e in range(4))
        inside = (ar.reshape(1, 1, IMG, 1) >= y0) & (ar.reshape(1, 1, IMG, 1) < y1) & (ar.reshape(1, 1, 1, IMG) >= x0) & (ar.reshape(1, 1, 1, IMG) < x1)
        v = torch.where(inside, rgb[:, k].reshape(B, 3, 1, 1), v)
        filled = filled | ((y1 > y0) & (x1 > x0))
    work = (taps[:, 1:] != 0).any(-1).reshape(B, 1, 1, 1) | (M != ident).any(-1).any(-1).reshape(B, 1, 1, 1) | (gam != 1).any(1, keepdim=True) | (sig != 0) | filled
    return torch.where(content & work, (v - mean) / std, x).reshape(im.shape)


def count(fn):
    """operators of one call of fn: aten operators outside VIEWS + one per call into the library"""
    calls = {"n": 0}

    class Spy(object):
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if not callable(f) or name.endswith("_last_error"):
                return f

            def counted(*a):
                calls["n"] += 1
                return f(*a)
            return counted
    real = G.lib
    spy = Spy(G.lib())
    G.lib = lambda: spy
    try:
        with LaunchCount() as m:
            fn()
    finally:
        G.lib = real
    torch.cuda.synchronize()
    return m.n + calls["n"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seed", type=int, default=79)
    ap.add_argument("--only", choices=("blur", "colour", "gamma", "noise", "occluders"), default=None,
                    help="switch every other stage off (default: every stage on)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    n = args.n
    batch, im, crops, index = synthetic(n, args.seed, dev)
    on = dict(blur_sigma=(0.5, 2.0), noise_sigma=(0.005, 0.03))                           # every stage on every image ...
    if args.only:                                                                         # ... or one group of stages alone
        off = dict(blur_sigma=None, brightness=None, hue_deg=None, saturation=None, channel_gain=None, gamma=None, grayscale=None,
                   noise_sigma=None, occluders=0)
        keep = {"blur": ("blur_sigma",), "colour": ("brightness", "hue_deg", "saturation", "channel_gain", "grayscale"), "gamma": ("gamma",),
                "noise": ("noise_sigma",), "occluders": ("occluders",)}[args.only]
        on = dict({k: v for k, v in off.items() if k not in keep}, **{k: v for k, v in on.items() if k in keep})
    aug = CropAugment(seed=args.seed, p=1.0, device=dev, **on)
    P = aug.draw(index, 0, batch["cam0"])
    out = torch.empty_like(im)

    def call():
        return aug(batch, index, epoch=0)

    def apply():
        return aug.apply(im, crops, P, index, 0, batch["cam0"], out=out)

    def eager():
        return eager_apply(im, crops, P, index, batch["cam0"], args.seed, 0)

    def copy():
        return out.copy_(im)

    got = call()
    got = torch.stack([got["im0"], got["im1"]])
    want = eager()
    torch.cuda.synchronize()
    worst = float((got - want).abs().max())
    changed = float((got != im).float().mean())
    if not worst <= 1e-4 or not torch.equal(got, apply()):
        raise SystemExit("the kernel against the eager path: max |difference| %.3e" % worst)
    ops = [count(fn) for fn in (call, apply, eager, copy)]
    med, spread = timed_interleaved([call, apply, eager, copy], args.warmup, args.reps, args.windows)
    moved = 2 * (2 * n * 3 * IMG * IMG * 4)
    rec = {"tool": "augment_bench", "n": n, "stages": args.only or "all", "call_us": round(med[0], 1), "apply_us": round(med[1], 1), "eager_us": round(med[2], 1),
           "copy_us": round(med[3], 1), "spread_us": [round(x, 1) for x in spread], "eager_over_call": round(med[2] / med[0], 2),
           "apply_over_copy": round(med[1] / med[3], 2), "moved_mb": round(moved / 1e6, 1),
           "apply_gb_per_s": round(moved / med[1] / 1e3, 1), "copy_gb_per_s": round(moved / med[3] / 1e3, 1),
           "call_ops": ops[0], "apply_ops": ops[1], "eager_ops": ops[2], "copy_ops": ops[3], "max_abs_against_eager": worst,
           "pixels_changed": round(changed, 3), "status_nonzero": int((aug.status != 0).sum()), "windows": args.windows, "reps": args.reps,
           "grad_lib": os.path.basename(G.LIB_PATH)}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
