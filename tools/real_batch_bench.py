"""Time airpose_amd.RealSequenceBatches.batch at the reference's frame size: n = 64 consecutive frames of 1080 x 1920 from both cameras,
seeded synthetic frames and detections (a person of about 250 x 500 px somewhere in the frame, AlphaPose scattered around OpenPose,
one pair in eight further than 100 px apart).

  batch       RealSequenceBatches.batch: apg_real_batch, then ap_preprocess_crops once per camera reading the boxes on the device
  host        what a user does without it: detections[:, a:a + n].cpu(), the filter, boxes, bb and crop coordinates in numpy one
              sample at a time (copenet_real.__getitem__'s arithmetic), utils.preprocess_crops per camera (which copies the boxes back
              to validate them), and bb and the keypoints copied to the device
  *_ops       an OPERATOR count per call as in tools/loss_bench.py: every aten operator outside LaunchCount.VIEWS counts one, every
              apg_real_batch / ap_preprocess_crops call counts one (its one launch)
  *_host_copies   calls of Tensor.cpu / item / tolist / numpy on a CUDA tensor during one call: each blocks the host on the stream
  *_enqueue_us    host clock around the call WITHOUT a synchronise: what the host spends before it can go on.  For `host` this
              contains the waits of its copies

The two take turns in one process (HIP events around --reps calls, the median of --windows windows and their max - min).  Before
anything is timed the two paths' boxes, bb, crop coordinates and images are compared (boxes and images: equal; bb and coordinates:
the host works in fp64).  One JSON line; --out also writes it to a file.

    python tools/real_batch_bench.py [--n 64] [--height 1080] [--width 1920] [--out profiles/real_batch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native as N  # noqa: E402
from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd import utils  # noqa: E402
from airpose_amd.real_batches import RealSequenceBatches  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402

COPIES = ("cpu", "item", "tolist", "numpy")


def synthetic(L, H, W, seed):
    """detections (2, L, 2, 24, 3) fp32 inside the frame, frames per camera (L, H, W, 3) uint8"""
    g = torch.Generator().manual_seed(seed)
    centre = torch.stack([300 + (W - 600) * torch.rand(2, L, generator=g), 300 + (H - 600) * torch.rand(2, L, generator=g)], -1)
    op = centre.unsqueeze(2) + torch.tensor([125.0, 250.0]) * (2 * torch.rand(2, L, 24, 2, generator=g) - 1)
    al = op + 6.0 * torch.randn(2, L, 24, 2, generator=g)
    far = torch.rand(2, L, 24, generator=g) < 0.125
    al[..., 0] = torch.where(far, al[..., 0] + 150.0, al[..., 0])
    det = torch.zeros(2, L, 2, 24, 3)
    det[:, :, 0, :, :2], det[:, :, 1, :, :2] = op, al
    det[..., :2] = torch.minimum(det[..., :2].clamp_min(0.0), torch.tensor([float(W), float(H)]))
    det[..., 2] = 0.2 + 0.8 * torch.rand(2, L, 2, 24, generator=g)
    det[:, :, 0, [3, 6, 9, 13, 14, 15, 22, 23], 2] = 0.0
    det[:, :, 1, [0, 3, 6, 9, 10, 11, 13, 14, 15, 22, 23], 2] = 0.0
    frames = [torch.randint(0, 256, (L, H, W, 3), generator=g, dtype=torch.uint8) for _ in (0, 1)]
    return det, frames


def host_batch(det_dev, frames, K, a, n, agreement_px=100.0, border=50):
    """copenet_real.py:105-106 and __getitem__'s arithmetic on the host, sample by sample, then the package's image kernel"""
    dev = det_dev.device
    d = det_dev[:, a:a + n].cpu().numpy().astype(np.float64)
    out = {}
    for v in (0, 1):
        H, W = frames[v].shape[1:3]
        c = K[v, :2, 2]
        crops, bbs, j2d, j2dc = np.zeros((n, 4), np.int32), np.zeros((n, 3), np.float32), np.zeros((n, 2, 24, 3), np.float32), np.zeros((n, 2, 24, 3), np.float32)
        for i in range(n):
            op, al = d[v, i, 0].copy(), d[v, i, 1].copy()
            apart = np.sqrt((op[:, 0] - al[:, 0]) ** 2 + (op[:, 1] - al[:, 1]) ** 2) > agreement_px
            op[apart, 2] = 0
            al[apart, 2] = 0
            x, y = op[op[:, 2] != 0, 0], op[op[:, 2] != 0, 1]
            x, y = (x, y) if x.size else (np.array([0]), np.array([0]))
            x0 = int(x.min() - border) if int(x.min() - border) > 0 else 0
            y0 = int(y.min() - border) if int(y.min() - border) > 0 else 0
            x1 = int(x.max() + border) if int(x.max() + border) < W else W
            y1 = int(y.max() + border) if int(y.max() + border) < H else H
            bb = np.array([(x0 + x1) / 2, (y0 + y1) / 2]) / c - 1
            s = 224.0 / max(y1 - y0, x1 - x0)
            crops[i], bbs[i] = (y0, y1, x0, x1), (bb[0], bb[1], s)
            for k, p in enumerate((op, al)):
                j2d[i, k] = p
                j2dc[i, k, :, :2], j2dc[i, k, :, 2] = s * (p[:, :2] - (bb + 1) * c), p[:, 2]
        im, scale, pad = utils.preprocess_crops(frames[v], torch.from_numpy(crops).to(dev))
        out.update({"im%d" % v: im, "bb%d" % v: torch.from_numpy(bbs).to(dev), "smpl_joints_2d%d" % v: torch.from_numpy(j2d).to(dev),
                    "smpl_joints_2d_crop%d" % v: torch.from_numpy(j2dc).to(dev), "crops%d" % v: crops})
    return out


def count(fn):
    """(operators, host copies) of one call of fn"""
    calls = {"n": 0, "copies": 0}

    class Spy(object):
        def __init__(self, lib, names):
            self._lib, self._names = lib, names

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if name not in self._names:
                return f

            def counted(*a):
                calls["n"] += 1
                return f(*a)
            return counted
    real_g, real_n = G.lib, N.lib
    spy_g, spy_n = Spy(G.lib(), ("apg_real_batch",)), Spy(N.lib(), ("ap_preprocess_crops",))
    G.lib, N.lib = (lambda: spy_g), (lambda: spy_n)
    saved = {k: getattr(torch.Tensor, k) for k in COPIES}

    def patch(orig):
        def counted(self, *a, **k):
            if self.is_cuda:
                calls["copies"] += 1
            return orig(self, *a, **k)
        return counted
    for k, orig in saved.items():
        setattr(torch.Tensor, k, patch(orig))
    try:
        with LaunchCount() as m:
            fn()
    finally:
        G.lib, N.lib = real_g, real_n
        for k, orig in saved.items():
            setattr(torch.Tensor, k, orig)
    torch.cuda.synchronize()
    return m.n + calls["n"], calls["copies"]


def enqueue_us(fn, reps):
    """median host time of one call that is not followed by a synchronise (the queue is drained before each)"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("real_batch_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    n, H, W = args.n, args.height, args.width
    det, frames = synthetic(n, H, W, args.seed)
    det, frames = det.to(dev), [f.to(dev) for f in frames]
    K = np.array([[[1475.0, 0, 960.0], [0, 1475.0, 540.0], [0, 0, 1]], [[1470.0, 0, 955.5], [0, 1470.0, 541.25], [0, 0, 1]]])
    rb = RealSequenceBatches(det, torch.from_numpy(K).float(), device=dev)

    def batch():
        return rb.batch(frames[0], frames[1], 0)

    def host():
        return host_batch(det, frames, K, 0, n)

    b, h = batch(), host()
    torch.cuda.synchronize()
    same = {}
    for v in (0, 1):
        same["crops%d" % v] = bool(np.array_equal(b["crops%d" % v].cpu().numpy(), h["crops%d" % v]))
        same["im%d" % v] = bool(torch.equal(b["im%d" % v], h["im%d" % v]))
        same["conf%d" % v] = bool(torch.equal(b["smpl_joints_2d%d" % v], h["smpl_joints_2d%d" % v]))
        same["bb%d_max_abs" % v] = float((b["bb%d" % v] - h["bb%d" % v]).abs().max())
        same["crop_xy%d_max_abs" % v] = float((b["smpl_joints_2d_crop%d" % v] - h["smpl_joints_2d_crop%d" % v]).abs().max())
        if not (same["crops%d" % v] and same["im%d" % v] and same["conf%d" % v]) or same["bb%d_max_abs" % v] > 1e-6 or same["crop_xy%d_max_abs" % v] > 1e-2:
            raise SystemExit("batch against the host path: %r" % same)
    status = torch.stack([b["status0"], b["status1"]]).cpu()
    del b, h
    ops = [count(fn) for fn in (batch, host)]
    med, spread = timed_interleaved([batch, host], args.warmup, args.reps, args.windows)
    enq = [enqueue_us(fn, args.reps) for fn in (batch, host)]
    rec = {"tool": "real_batch_bench", "n": n, "height": H, "width": W,
           "batch_us": round(med[0], 1), "host_us": round(med[1], 1), "host_over_batch": round(med[1] / med[0], 2),
           "spread_us": [round(x, 1) for x in spread],
           "batch_enqueue_us": round(enq[0], 1), "host_enqueue_us": round(enq[1], 1),
           "batch_ops": ops[0][0], "host_ops": ops[1][0], "batch_host_copies": ops[0][1], "host_host_copies": ops[1][1],
           "batch_blocks_host": ops[0][1] > 0, "host_blocks_host": ops[1][1] > 0,
           "status_nonzero": int((status != 0).sum()), "batch_vs_host": same, "windows": args.windows, "reps": args.reps,
           "grad_lib": os.path.basename(G.LIB_PATH)}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
