"""Time the fused mesh metrics (airpose_amd.MeshMetrics.update, apg_align_update) against the eager formulation a user would write
with torch today, on the GPU, two views, V vertices and 22 of 25 joints, at B in {30 (the reference's eval batch), 256}:

  eager          torch ops per view and point set: the differences, norms and means for abs and root, the centred moments,
                 a batched torch.linalg.svd of the (B, 3, 3) covariances, the reflection fix, the scale and the aligned error;
                 the twelve batch means stay on the device (no .cpu() is counted against it)
  eager_cpu      the same with ONE .cpu() of the stacked means at the end of the batch, as an evaluation loop would have it
  fused          MeshMetrics.update on the same dicts: two apg_align_update calls of two launches each, sums left on the device
                 (compute() reads them once, after the last batch; it is not part of a batch and not timed)
  copy           a plain device copy (Tensor.copy_) of as many bytes as the kernels read, 2 * views * B * (V + J) * 12: the floor
  *_ops          an OPERATOR count per call, as in tools/eval_bench.py: every aten operator dispatched during the call counts one
                 unless its name is in LaunchCount.VIEWS, every apg_align_update call counts two (its two launches)

The windows of every candidate of every size take turns in one process (HIP events around --reps calls, the median of --windows
windows and their max - min).  One JSON line per batch size; --out also writes them to a file.

    python tools/align_bench.py [--sizes 30,256] [--verts 10475] [--reps 20] [--windows 7] [--out profiles/align_bench.json]
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
from airpose_amd.mesh_metrics import MeshMetrics  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402

NJ, J_PRED = 22, 25


def eager_set(P, Q, rp, rq):
    """abs, root, pa batch means of (B, N, 3) sets with (B, 3) roots, in torch ops"""
    e_abs = (P - Q).norm(dim=2).mean(1)
    e_root = ((P - rp[:, None]) - (Q - rq[:, None])).norm(dim=2).mean(1)
    a, b = P - P.mean(1, keepdim=True), Q - Q.mean(1, keepdim=True)
    K = b.transpose(1, 2) @ a
    U, S, Vh = torch.linalg.svd(K)
    D = torch.ones_like(S)
    D[:, 2] = torch.sign(torch.det(U) * torch.det(Vh))
    R = (U * D[:, None, :]) @ Vh
    s = (S * D).sum(1) / a.pow(2).sum((1, 2))
    e_pa = (s[:, None, None] * (a @ R.transpose(1, 2)) - b).norm(dim=2).mean(1)
    return torch.stack([e_abs.mean(), e_root.mean(), e_pa.mean()])


def eager(out, batch):
    res = []
    for v in (0, 1):
        pj, gj = out["pred_j3d_cam%d" % v][:, :NJ], batch["smpl_joints_rel%d" % v][:, 0, :NJ]
        res.append(eager_set(pj, gj, pj[:, 0], gj[:, 0]))
        res.append(eager_set(out["pred_vertices_cam%d" % v], batch["smpl_vertices_rel%d" % v][:, 0], pj[:, 0], gj[:, 0]))
    return torch.stack(res)                                      # (view x set, 3)


def count_ops(fn):
    """aten operators outside VIEWS + 2 per apg_align_update call, over one call of fn"""
    calls = {"n": 0}
    lib = G.lib()

    class Spy(object):
        def __getattr__(self, name):
            f = getattr(lib, name)
            if name != "apg_align_update":
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30,256")
    ap.add_argument("--verts", type=int, default=10475)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    V = args.verts
    sizes = [int(s) for s in args.sizes.split(",")]
    feeds = {}
    for B in sizes:
        g = torch.Generator().manual_seed(B)
        out, batch = {}, {}
        for v in (0, 1):
            for n, pk, gk, keep in ((V, "pred_vertices_cam%d", "smpl_vertices_rel%d", V), (J_PRED, "pred_j3d_cam%d", "smpl_joints_rel%d", NJ)):
                q = (torch.rand(B, n, 3, generator=g) - 0.5) * torch.tensor([0.6, 1.0, 0.4]) + torch.tensor([0.3, -0.2, 10.0])
                p = q + 0.03 * torch.randn(B, n, 3, generator=g) + torch.tensor([0.05, -0.02, 0.4])
                out[pk % v], batch[gk % v] = p.to(dev), q[:, :keep].unsqueeze(1).contiguous().to(dev)
        feeds[B] = (out, batch)

    def candidates(B):
        out, batch = feeds[B]
        metrics = MeshMetrics(kind="twoview", device=dev)
        nbytes = 2 * 2 * B * (V + NJ) * 12
        src = torch.empty(nbytes // 4, device=dev, dtype=torch.float32).normal_()
        dst = torch.empty_like(src)

        def fused():
            metrics.update(out, batch)

        def eager_dev():
            with torch.no_grad():
                return eager(out, batch)

        def eager_cpu():
            with torch.no_grad():
                return eager(out, batch).cpu()

        def copy():
            dst.copy_(src)
        metrics.reset()
        fused()
        a = metrics.compute()
        b = eager_cpu().double().tolist()
        labels = (("mpjpe_abs", "mpjpe_root", "pa_mpjpe"), ("pve_abs", "pve_root", "pa_pve"))
        worst = max(abs(a["%s%d" % (labels[k][i], v)] - b[2 * v + k][i]) for v in (0, 1) for k in (0, 1) for i in range(3))
        if not worst <= 1e-4:
            raise SystemExit("fused metrics %r against the eager formulation %r" % (a, b))
        return [fused, eager_dev, eager_cpu, copy], nbytes, worst
    cands = [candidates(B) for B in sizes]
    fns = [fn for c in cands for fn in c[0]]
    ops = [count_ops(fn) for fn in fns]
    med, spread = timed_interleaved(fns, args.warmup, args.reps, args.windows)      # every size's candidates take turns
    lines = []
    for i, B in enumerate(sizes):
        m, o, sp = med[4 * i:4 * i + 4], ops[4 * i:4 * i + 4], spread[4 * i:4 * i + 4]
        rec = {"tool": "align_bench", "kind": "twoview", "B": B, "V": V, "J": NJ, "bytes_read": cands[i][1],
               "fused_us": round(m[0], 1), "eager_us": round(m[1], 1), "eager_cpu_us": round(m[2], 1), "copy_us": round(m[3], 1),
               "speedup_vs_eager": round(m[1] / m[0], 2), "speedup_vs_eager_cpu": round(m[2] / m[0], 2),
               "fused_over_copy": round(m[0] / m[3], 2), "fused_ops": o[0], "eager_ops": o[1], "eager_cpu_ops": o[2],
               "copy_ops": o[3], "spread_us": [round(x, 1) for x in sp], "max_abs_diff_m": cands[i][2], "windows": args.windows,
               "reps": args.reps, "grad_lib": os.path.basename(G.LIB_PATH)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
