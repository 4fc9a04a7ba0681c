"""Time the fused cross-view metrics (airpose_amd.CrossViewMetrics.update, apg_xview_update) against the eager formulation a user
would write with torch today, on the GPU, V vertices and 22 of 25 joints, at B in {30 (the reference's eval batch), 256}:

  eager          torch ops: torch.inverse of the two (B, 4, 4) extrinsics, four bmm that carry joints and vertices of both views into
                 the world, the norms and means of the world and root gaps, the translation gap, the two angle gaps (bmm, atan2), the
                 confidence-weighted reprojection error, and a per-joint torch.linalg.lstsq of the (B, 4, 3) triangulation systems
                 with the two tri errors; the batch means stay on the device (no .cpu() is counted against it)
  eager_cpu      the same with ONE .cpu() of the stacked means at the end of the batch, as an evaluation loop would have it
  fused          CrossViewMetrics.update on the same dicts: one apg_xview_update call of two launches, sums left on the device
                 (compute() reads them once, after the last batch; it is not part of a batch and not timed)
  copy           a plain device copy (Tensor.copy_) of as many bytes as the kernels read, 2 * B * (V + J) * 12: the floor
  *_ops          an OPERATOR count per call, as in tools/eval_bench.py: every aten operator dispatched during the call counts one
                 unless its name is in LaunchCount.VIEWS, every apg_xview_update call counts two (its two launches)

The windows of every candidate of every size take turns in one process (HIP events around --reps calls, the median of --windows
windows and their max - min).  torch's batched lstsq on the device walks the batch a matrix at a time, so one eager call at B = 256
is 22 x 256 factorisations: the defaults below take minutes, and the first call's wall time goes to stderr so that a run can be sized
(--reps, --windows); --eager-solver normal_equations gives the eager path torch.linalg.solve of the 3 x 3 normal equations instead,
which is batched, and is also what the eager path falls back to where this torch build has no torch.linalg.lstsq on the device.  The
record names the solver under "eager_solver".  One JSON line per batch size; --out also writes them to a file.

    python tools/xview_bench.py [--sizes 30,256] [--verts 10475] [--reps 20] [--windows 7] [--eager-solver lstsq] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd.cross_view_metrics import CrossViewMetrics  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402

NJ, J_PRED = 22, 25
KEYS = ("joint_gap_world", "joint_gap_root", "vertex_gap_world", "vertex_gap_root", "trans_gap", "orient_gap_deg", "pose_gap_deg",
        "reproj_px0", "reproj_px1", "tri_mpjpe0", "tri_mpjpe1")


def angle_deg(A, B):
    D = A.transpose(-1, -2) @ B
    ax = torch.stack([D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]], -1)
    return torch.rad2deg(torch.atan2(ax.norm(dim=-1), D.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0))


def eager(out, batch, solver):
    """the eleven batch means of KEYS, in torch ops"""
    inv = [torch.inverse(batch["extr%d" % v]) for v in (0, 1)]
    Ri = [m[:, :3, :3] for m in inv]
    world = lambda v, P: torch.bmm(P, Ri[v].transpose(1, 2)) + inv[v][:, None, :3, 3]
    rel = lambda v, P: torch.bmm(P - out["pred_smpltrans%d" % v][:, None], Ri[v].transpose(1, 2))
    res = []
    Jw = None
    for key, n in (("pred_j3d_cam%d", NJ), ("pred_vertices_cam%d", None)):
        P = [out[key % v][:, :n] for v in (0, 1)]
        W = [world(v, P[v]) for v in (0, 1)]
        Jw = W if Jw is None else Jw
        res.append((W[0] - W[1]).norm(dim=2).mean())
        res.append((rel(0, P[0]) - rel(1, P[1])).norm(dim=2).mean())
    s = [world(v, out["pred_smpltrans%d" % v][:, None]) for v in (0, 1)]
    res.append((s[0] - s[1]).norm(dim=2).mean())
    Q = [out["pred_rotmat%d" % v] for v in (0, 1)]
    res.append(angle_deg(Ri[0] @ Q[0][:, 0], Ri[1] @ Q[1][:, 0]).mean())
    res.append(angle_deg(Q[0][:, 1:], Q[1][:, 1:]).mean())
    kp = [batch["smpl_joints_2d%d" % v][:, 0, :NJ] for v in (0, 1)]
    for v in (0, 1):
        c = kp[v][..., 2]
        d = (out["pred_j2d_cam%d" % v][:, :NJ] - kp[v][..., :2]).norm(dim=2)
        res.append(((c * d).sum(1) / c.sum(1)).mean())
    # lstsq_triangulation, a joint at a time as the reference has it, batched over the samples
    rows, rhs = [], []
    for v in (0, 1):
        K, E = batch["intr%d" % v], batch["extr%d" % v]
        n = torch.stack([(kp[v][..., 0] - K[:, None, 0, 2]) / K[:, None, 0, 0], (kp[v][..., 1] - K[:, None, 1, 2]) / K[:, None, 1, 1]], -1)
        rows.append(n[..., None] * E[:, None, None, 2, :3] - E[:, None, :2, :3])           # (B, 22, 2, 3)
        rhs.append(E[:, None, :2, 3] - E[:, None, 2, 3, None] * n)                          # (B, 22, 2)
    A, y = torch.cat(rows, 2), torch.cat(rhs, 2)
    T = []
    for j in range(NJ):
        if solver == "lstsq":
            T.append(torch.linalg.lstsq(A[:, j], y[:, j, :, None]).solution[..., 0])
        else:
            At = A[:, j].transpose(1, 2)
            T.append(torch.linalg.solve(At @ A[:, j], (At @ y[:, j, :, None])[..., 0]))
    T = torch.stack(T, 1)
    for v in (0, 1):
        res.append((Jw[v] - T).norm(dim=2).mean())
    return torch.stack(res)


def make_feed(B, V, dev, seed):
    """a body both views agree on up to 2 cm of noise, two cameras 6 to 10 m away and 20 to 120 degrees apart, f = 1500 px"""
    rng = np.random.default_rng(seed)
    out, batch = {}, {}
    Xw = rng.uniform(-0.25, 0.25, (B, J_PRED, 3))
    Yw = rng.uniform(-0.25, 0.25, (B, V, 3))
    sw = rng.uniform(-0.05, 0.05, (B, 3))
    aa = rng.standard_normal((B, NJ, 3))
    d0 = rng.standard_normal((B, 3))
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    perp = np.cross(d0, rng.standard_normal((B, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    sep = np.radians(rng.uniform(20, 120, (B, 1)))
    dirs = [d0, np.cos(sep) * d0 + np.sin(sep) * perp]

    def rodrigues(r):
        th = np.linalg.norm(r, axis=-1)[..., None, None]
        k = r / th[..., 0]
        Kx = np.zeros(r.shape[:-1] + (3, 3))
        Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0], Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    Qw = rodrigues(aa)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    for v in (0, 1):
        C = rng.uniform(6, 10, (B, 1)) * dirs[v]
        z = -C / np.linalg.norm(C, axis=1, keepdims=True)
        x = np.cross(rng.standard_normal((B, 3)), z)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        R = np.stack([x, np.cross(z, x), z], 1)
        t = -np.einsum("bij,bj->bi", R, C)
        E = np.tile(np.eye(4), (B, 1, 1))
        E[:, :3, :3], E[:, :3, 3] = R, t
        cam = lambda P: np.einsum("bij,bnj->bni", R, P) + t[:, None]
        K = np.tile(np.array([[1500.0, 0, 960], [0, 1500.0, 540], [0, 0, 1]]), (B, 1, 1))
        proj = lambda P: np.stack([1500.0 * P[..., 0] / P[..., 2] + 960, 1500.0 * P[..., 1] / P[..., 2] + 540], -1)
        J = cam(Xw) + rng.normal(0, 0.02, (B, J_PRED, 3))
        out["pred_j3d_cam%d" % v], out["pred_vertices_cam%d" % v] = f(J), f(cam(Yw) + rng.normal(0, 0.02, (B, V, 3)))
        out["pred_smpltrans%d" % v] = f(cam(sw[:, None])[:, 0])
        Qv = Qw @ rodrigues(rng.normal(0, 0.05, (B, NJ, 3)))
        Qv[:, 0] = R @ Qv[:, 0]
        out["pred_rotmat%d" % v] = f(Qv)
        out["pred_j2d_cam%d" % v] = f(proj(J))
        kp = np.concatenate([proj(cam(Xw))[:, :24] + rng.uniform(-3, 3, (B, 24, 2)), rng.uniform(0.3, 1.0, (B, 24, 1))], 2)
        batch["smpl_joints_2d%d" % v] = f(np.stack([kp, kp[:, ::-1]], 1))
        batch["extr%d" % v], batch["intr%d" % v] = f(E), f(K)
    return out, batch


def count_ops(fn):
    """aten operators outside VIEWS + 2 per apg_xview_update call, over one call of fn"""
    calls = {"n": 0}
    lib = G.lib()

    class Spy(object):
        def __getattr__(self, name):
            f = getattr(lib, name)
            if name != "apg_xview_update":
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
    ap.add_argument("--eager-solver", default="lstsq", choices=("lstsq", "normal_equations"),
                    help="how the eager path solves the 22 triangulation systems: torch.linalg.lstsq as the reference has it, or "
                         "torch.linalg.solve of their normal equations")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    V = args.verts
    sizes = [int(s) for s in args.sizes.split(",")]
    feeds = {B: make_feed(B, V, dev, B) for B in sizes}
    solver = args.eager_solver
    try:
        torch.linalg.lstsq(torch.eye(4, 3, device=dev).expand(2, 4, 3), torch.ones(2, 4, 1, device=dev))
        torch.cuda.synchronize()
    except RuntimeError:
        solver = "normal_equations"

    def candidates(B):
        out, batch = feeds[B]
        metrics = CrossViewMetrics(device=dev)
        nbytes = 2 * B * (V + J_PRED) * 12
        src = torch.empty(nbytes // 4, device=dev, dtype=torch.float32).normal_()
        dst = torch.empty_like(src)

        def fused():
            metrics.update(out, batch)

        def eager_dev():
            with torch.no_grad():
                return eager(out, batch, solver)

        def eager_cpu():
            with torch.no_grad():
                return eager(out, batch, solver).cpu()

        def copy():
            dst.copy_(src)
        metrics.reset()
        t0 = time.time()
        fused()
        a = metrics.compute()
        t1 = time.time()
        b = eager_cpu().double().tolist()
        print("B = %d: first fused call and compute %.3f s, first eager call %.3f s (%s)" % (B, t1 - t0, time.time() - t1, solver),
              file=sys.stderr, flush=True)
        if a["skipped"] or a["tri_n"] != B * NJ:
            raise SystemExit("the feed has skipped samples or invalid triangulations: %r" % (a,))
        # the eager numbers are fp32 throughout: metres to 1e-4, degrees and pixels to 1e-2
        worst = max(abs(a[k] - x) / (1.0 if k.endswith("deg") or k.startswith("reproj") else 0.01) for k, x in zip(KEYS, b))
        if not worst <= 1e-2:
            raise SystemExit("fused metrics %r against the eager formulation %r" % (a, dict(zip(KEYS, b))))
        return [fused, eager_dev, eager_cpu, copy], nbytes, worst
    cands = [candidates(B) for B in sizes]
    fns = [fn for c in cands for fn in c[0]]
    ops = [count_ops(fn) for fn in fns]
    med, spread = timed_interleaved(fns, args.warmup, args.reps, args.windows)      # every size's candidates take turns
    lines = []
    for i, B in enumerate(sizes):
        m, o, sp = med[4 * i:4 * i + 4], ops[4 * i:4 * i + 4], spread[4 * i:4 * i + 4]
        rec = {"tool": "xview_bench", "B": B, "V": V, "J": NJ, "bytes_read": cands[i][1], "eager_solver": solver,
               "fused_us": round(m[0], 1), "eager_us": round(m[1], 1), "eager_cpu_us": round(m[2], 1), "copy_us": round(m[3], 1),
               "speedup_vs_eager": round(m[1] / m[0], 2), "speedup_vs_eager_cpu": round(m[2] / m[0], 2),
               "fused_over_copy": round(m[0] / m[3], 2), "fused_ops": o[0], "eager_ops": o[1], "eager_cpu_ops": o[2],
               "copy_ops": o[3], "spread_us": [round(x, 1) for x in sp], "worst_scaled_diff": round(cands[i][2], 6),
               "min_ray_angle_deg": 1.0, "windows": args.windows, "reps": args.reps, "grad_lib": os.path.basename(G.LIB_PATH)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
