"""Time the fused evaluation metrics (airpose_amd.EvalMetrics.update, apg_eval_update) against the restatement of the reference's
test_epoch_end a user would write with this project today, on the GPU, two views, at B in {30 (the reference's eval batch), 256}:

  restatement    torch ops for tgm.angle_axis_to_rotation_matrix on pred_angles0/1, FOUR airpose_amd.SMPLX.forward calls (ground truth
                 and prediction, both views, betas = 0), torch ops for the 22-joint distances, the translation errors and the means,
                 and .cpu() on the results at the end of the batch, as the reference does
  fused          EvalMetrics.update on the same dicts: two launches, sums left on the device (compute() reads them once, after the
                 last batch; it is not part of a batch and not timed)
  *_ops          an OPERATOR count per call, as in tools/loss_bench.py: every aten operator dispatched during the call counts one
                 unless its name is in VIEWS, every apg_eval_update call counts two (its two launches), every ap_smplx_fwd call is
                 counted as the launches of its body-only path (--smplx-launches, default 3: smplx_run's prep kernel, the fused blend +
                 skinning kernel and the joints kernel)

The two candidates' windows take turns in one process (HIP events around --reps calls, the median of --windows windows and their
max - min).  One JSON line per batch size; --out also writes them to a file.

    python tools/eval_bench.py [--sizes 30,256] [--reps 20] [--windows 7] [--out profiles/eval_bench.json]
"""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd import smplx, smplx_model  # noqa: E402
from airpose_amd.eval_metrics import EvalMetrics  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402


def tgm_angle_axis_to_rotation_matrix(aa, eps=1e-6):
    """torchgeometry 0.1.2's conversion on (N, 3) -> (N, 3, 3), in torch ops as tgm writes it (both branches, blended by masks)"""
    t2 = (aa * aa).sum(1)
    th = torch.sqrt(t2)
    w = aa / (th + eps)[:, None]
    wx, wy, wz = w.unbind(1)
    c, s = torch.cos(th), torch.sin(th)
    k = 1.0 - c
    normal = torch.stack([c + wx * wx * k, wx * wy * k - wz * s, wy * s + wx * wz * k,
                          wz * s + wx * wy * k, c + wy * wy * k, -wx * s + wy * wz * k,
                          -wy * s + wx * wz * k, wx * s + wy * wz * k, c + wz * wz * k], 1)
    rx, ry, rz = aa.unbind(1)
    one = torch.ones_like(rx)
    taylor = torch.stack([one, -rz, ry, rz, one, -rx, -ry, rx, one], 1)
    mask = (t2 > eps).to(aa.dtype)[:, None]
    return (mask * normal + (1 - mask) * taylor).view(-1, 3, 3)


def restatement(body, zeros, out):
    """the reference's per-batch recipe on this project's SMPLX.forward -> host floats"""
    B = out["pred_angles0"].shape[0]
    res = {}
    for v in (0, 1):
        R = tgm_angle_axis_to_rotation_matrix(out["pred_angles%d" % v].reshape(-1, 3)).view(B, 22, 3, 3)
        gt = body.forward(betas=zeros, body_pose=out["smplpose_rotmat"], global_orient=out["smplorient_rel%d" % v], pose2rot=False)
        pr = body.forward(betas=zeros, body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False)
        err = (pr.joints[:, :22] - gt.joints[:, :22]).pow(2).sum(2).sqrt()
        res["mpjpe%d" % v] = err.mean()
        res["per_joint%d" % v] = err.mean(0)
        res["mpe%d" % v] = (out["pred_smpltrans%d" % v] - out["gt_smpltrans%d" % v]).pow(2).sum(1).sqrt().mean()
    return {k: t.cpu() for k, t in res.items()}


def count_ops(fn, smplx_launches):
    """aten operators outside VIEWS + 2 per apg_eval_update + smplx_launches per ap_smplx_fwd, over one call of fn"""
    from airpose_amd import _native as N
    calls = {"eval": 0, "smplx": 0}

    def spy(lib, name, key):
        class Spy(object):
            def __getattr__(self, n):
                f = getattr(lib, n)
                if n != name:
                    return f

                def counted(*a):
                    calls[key] += 1
                    return f(*a)
                return counted
        return Spy()
    glib, nlib = G.lib(), N.lib()
    real_g, real_n = G.lib, N.lib
    G.lib, N.lib = (lambda: spy(glib, "apg_eval_update", "eval")), (lambda: spy(nlib, "ap_smplx_fwd", "smplx"))
    try:
        with LaunchCount() as m:
            fn()
    finally:
        G.lib, N.lib = real_g, real_n
    torch.cuda.synchronize()
    return m.n + 2 * calls["eval"] + smplx_launches * calls["smplx"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--smplx-launches", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    md = smplx_model.make_synthetic_model(4321)
    body = smplx.SMPLX(model_data=md)
    lines = []
    for B in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(B)

        def rot(n):                                              # orthonormal rotations at angles over (0, pi)
            a = torch.randn(n, 3, generator=g, dtype=torch.float64)
            a = a / a.norm(dim=1, keepdim=True) * (math.pi * torch.rand(n, 1, generator=g, dtype=torch.float64))
            return tgm_angle_axis_to_rotation_matrix(a, eps=0.0).float()
        out = {"smplpose_rotmat": rot(B * 21).view(B, 21, 3, 3).to(dev)}
        for v in (0, 1):
            out["smplorient_rel%d" % v] = rot(B).view(B, 1, 3, 3).to(dev)
            out["pred_angles%d" % v] = (torch.randn(B, 22, 3, generator=g) * 0.8).to(dev)
            out["gt_smpltrans%d" % v] = (torch.randn(B, 3, generator=g) + torch.tensor([0.0, 0.0, 10.0])).to(dev)
            out["pred_smpltrans%d" % v] = out["gt_smpltrans%d" % v] + 0.3 * torch.randn(B, 3, generator=g).to(dev)
        zeros = torch.zeros(B, 10, device=dev)
        metrics = EvalMetrics(body, kind="twoview", device=dev)

        def fused():
            metrics.update(out)

        def eager():
            with torch.no_grad():
                restatement(body, zeros, out)
        metrics.reset()
        fused()
        a, b = metrics.compute(), {k: t.tolist() for k, t in restatement(body, zeros, out).items()}
        worst = max(abs(a[k] - b[k]) for k in ("mpjpe0", "mpjpe1", "mpe0", "mpe1"))
        worst = max([worst] + [abs(x - y) for v in (0, 1) for x, y in zip(a["per_joint%d" % v], b["per_joint%d" % v])])
        if not worst <= 1e-4:
            raise SystemExit("fused metrics %r against the restatement %r" % (a, b))
        fns = [fused, eager]
        ops = [count_ops(fn, args.smplx_launches) for fn in fns]
        med, spread = timed_interleaved(fns, args.warmup, args.reps, args.windows)
        rec = {"tool": "eval_bench", "kind": "twoview", "B": B, "fused_us": round(med[0], 1), "restatement_us": round(med[1], 1),
               "speedup": round(med[1] / med[0], 2), "fused_ops": ops[0], "restatement_ops": ops[1],
               "spread_us": [round(x, 1) for x in spread], "max_abs_diff_m": worst, "windows": args.windows, "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
