"""Time the fused training loss (airpose_amd.TrainingLoss, apg_loss_fwd_bwd) against the same two-view get_loss written in eager
torch, on the GPU, at B in {32, 64} with V = 10475 vertices and J = 127 joints:

  fused_fwd_us / eager_fwd_us         the loss under no_grad
  fused_fwdbwd_us / eager_fwdbwd_us   the loss and loss.backward() down to the fourteen prediction tensors
  *_ops                               an OPERATOR count per call, this tool's stand-in for launches: every aten operator dispatched
                                      during the call counts one unless its name is in VIEWS (views and allocations, which launch
                                      nothing), every apg_loss_fwd_bwd call counts two (loss_main_kernel and loss_combine_kernel:
                                      the entry point's two hipLaunchKernelGGL).  It is not a launch count: an operator that
                                      launches several kernels counts one, and so does a copy autograd makes when it accumulates

The four candidates' windows take turns in one process (HIP events around --reps calls, the median of --windows windows), as
tools/head_grad_bench.py does.  One JSON line per batch size; --out also writes them to a file.

    python tools/loss_bench.py [--sizes 32,64] [--reps 20] [--windows 7] [--out profiles/r10_loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch
from torch.utils._python_dispatch import TorchDispatchMode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd.loss import DEFAULTS, TrainingLoss  # noqa: E402

LIMB1, LIMB2 = [4, 5, 18, 19], [7, 8, 20, 21]


def eager_loss(h, batch, t0, t1, R0, R1, b0, b1, o0, o1, p0, p1):
    """the two-view get_loss in eager torch, term by term as the trainer writes it"""
    mse = lambda a, b: (a - b) ** 2
    gv, gj = batch["smpl_vertices"].squeeze(1), batch["smpl_joints"].squeeze(1)
    g2 = [batch["smpl_joints_2d0"].squeeze(1), batch["smpl_joints_2d1"].squeeze(1)]
    kp = mse(p0[:, :22], g2[0][:, :22]).mean() + mse(p1[:, :22], g2[1][:, :22]).mean()
    l = mse(o0.joints[:, :22], gj[:, :22]) + mse(o1.joints[:, :22], gj[:, :22]) + mse(o0.joints[:, :22], o1.joints[:, :22])
    l[:, LIMB1] *= h["limbs3d_loss_weight"]
    l[:, LIMB2] *= h["limbs3d_loss_weight"] ** 2
    kp3d = l.mean()
    shape = mse(o0.vertices, gv).mean() + mse(o1.vertices, gv).mean() + mse(o0.vertices, o1.vertices).mean()
    trans = mse(t0, batch["smpltrans_rel0"]).mean() + mse(t1, batch["smpltrans_rel1"]).mean()
    root = mse(R0[:, :1], batch["smplorient_rel0"]).mean() + mse(R1[:, :1], batch["smplorient_rel1"]).mean()
    l = mse(R0[:, 1:], batch["smplpose_rotmat"]) + mse(R1[:, 1:], batch["smplpose_rotmat"]) + mse(R0[:, 1:], R1[:, 1:])
    l[:, [j - 1 for j in LIMB1]] *= h["limbstheta_loss_weight"]
    l[:, [j - 1 for j in LIMB2]] *= h["limbstheta_loss_weight"] ** 2
    pose = l.mean()
    betas = (b0 * b0).mean() + (b1 * b1).mean() + mse(b0, b1).mean()
    loss = h["trans_loss_weight"] * trans + h["keypoint2d_loss_weight"] * kp + h["keypoint3d_loss_weight"] * kp3d + \
        h["shape_loss_weight"] * shape + h["rootrot_loss_weight"] * root + h["pose_loss_weight"] * pose + h["beta_loss_weight"] * betas
    return loss * 60


class LaunchCount(TorchDispatchMode):
    # overload packets (func.overloadpacket.__name__) that launch nothing
    VIEWS = frozenset(("view", "slice", "select", "squeeze", "unsqueeze", "expand", "detach", "alias", "t", "transpose", "_unsafe_view",
                       "reshape", "_reshape_alias", "as_strided", "permute", "narrow", "empty", "empty_like", "empty_strided",
                       "new_empty", "new_empty_strided"))

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func.overloadpacket.__name__ not in self.VIEWS:
            self.n += 1
        return out


def count_ops(fn):
    """aten operators outside VIEWS + 2 per apg_loss_fwd_bwd call, over one call of fn"""
    calls = {"n": 0}
    lib = G.lib()

    class Spy(object):
        def __getattr__(self, name):
            f = getattr(lib, name)
            if name != "apg_loss_fwd_bwd":
                return f

            def counted(*a):
                calls["n"] += 1
                return f(*a)
            return counted
    real = G.lib
    G.lib = lambda: Spy()
    try:
        with LaunchCount() as m:
            fn()
    finally:
        G.lib = real
    torch.cuda.synchronize()
    return m.n + 2 * calls["n"]


def timed_interleaved(fns, warmup, reps, windows):
    """medians of `windows` windows of `reps` calls per function, the functions' windows taking turns (A/B in one process)"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) * 1e3 / reps)
    return [statistics.median(o) for o in out], [max(o) - min(o) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--verts", type=int, default=10475)
    ap.add_argument("--joints", type=int, default=127)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    V, J = args.verts, args.joints
    h = DEFAULTS["twoview"]
    fused = TrainingLoss("twoview")
    lines = []
    for B in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(B)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)
        batch = {"smplpose_rotmat": r(B, 21, 3, 3), "smpltrans_rel0": r(B, 3), "smpltrans_rel1": r(B, 3), "smplorient_rel0": r(B, 1, 3, 3),
                 "smplorient_rel1": r(B, 1, 3, 3), "smpl_vertices": r(B, 1, V, 3), "smpl_joints": r(B, 1, J, 3),
                 "smpl_joints_2d0": r(B, 1, J, 2) * 100 + 500, "smpl_joints_2d1": r(B, 1, J, 2) * 100 + 500}
        leaf = lambda *s: r(*s).requires_grad_(True)
        t0, t1, R0, R1, b0, b1 = leaf(B, 3), leaf(B, 3), leaf(B, 22, 3, 3), leaf(B, 22, 3, 3), leaf(B, 10), leaf(B, 10)
        o0 = types.SimpleNamespace(joints=leaf(B, J, 3), vertices=leaf(B, V, 3))
        o1 = types.SimpleNamespace(joints=leaf(B, J, 3), vertices=leaf(B, V, 3))
        p0, p1 = (r(B, J, 2) * 100 + 500).requires_grad_(True), (r(B, J, 2) * 100 + 500).requires_grad_(True)
        preds = (t0, t1, R0, R1, b0, b1, o0, o1, p0, p1)
        leaves = [t0, t1, R0, R1, b0, b1, o0.joints, o0.vertices, o1.joints, o1.vertices, p0, p1]

        def clear():
            for t in leaves:
                t.grad = None

        def fused_fwd():
            with torch.no_grad():
                fused(batch, *preds)

        def eager_fwd():
            with torch.no_grad():
                eager_loss(h, batch, *preds)

        def fused_fwdbwd():
            clear()
            fused(batch, *preds)[0].backward()

        def eager_fwdbwd():
            clear()
            eager_loss(h, batch, *preds).backward()
        a, b = float(fused(batch, *preds)[0]), float(eager_loss(h, batch, *preds))
        if abs(a - b) > 1e-4 * abs(b):
            raise SystemExit("fused loss %r against eager %r" % (a, b))
        fns = [fused_fwd, eager_fwd, fused_fwdbwd, eager_fwdbwd]
        launches = [count_ops(fn) for fn in fns]
        med, spread = timed_interleaved(fns, args.warmup, args.reps, args.windows)
        rec = {"tool": "loss_bench", "kind": "twoview", "B": B, "V": V, "J": J,
               "fused_fwd_us": round(med[0], 1), "eager_fwd_us": round(med[1], 1), "fused_fwdbwd_us": round(med[2], 1),
               "eager_fwdbwd_us": round(med[3], 1), "fwd_speedup": round(med[1] / med[0], 2), "fwdbwd_speedup": round(med[3] / med[2], 2),
               "fused_fwd_ops": launches[0], "eager_fwd_ops": launches[1], "fused_fwdbwd_ops": launches[2],
               "eager_fwdbwd_ops": launches[3], "spread_us": [round(x, 1) for x in spread], "windows": args.windows, "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
