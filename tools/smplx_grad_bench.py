"""Time the differentiable SMPL-X layer on the GPU: the no-grad forward (ap_smplx_fwd), the forward under grad (the
autograd Function around the same call) and the backward alone (ap_smplx_bwd with every input gradient wanted), on the
synthetic model at n in {64, 256, 512} bodies, body-only (K = 224) and with hand / face poses (K = 512).

HIP events around windows of --reps calls after --warmup calls; the median of --windows windows is reported per call.  The
backward's bytes come from an analytic model of what its kernels move (each buffer once; see bwd_bytes) and are printed
against 8 TB/s.  One JSON line per configuration; --out also writes them to a file.

    python tools/smplx_grad_bench.py [--sizes 64,256,512] [--reps 20] [--windows 5] [--out profiles/x.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from airpose_amd import _native as N          # noqa: E402
from airpose_amd import lbs, smplx, smplx_model  # noqa: E402

HBM_PEAK = 8e12
RV, RC = 1024, 1024                           # SMPLX_BWD_RV / SMPLX_BWD_RC (airpose_amd/csrc/kernels.h)


def bwd_bytes(n, V, J, K, nj=127):
    """Bytes ap_smplx_bwd moves, each buffer counted once: recompute (coefficients, v_posed written), the LBS adjoint
    (grad_vertices, v_posed and g_vposed), the contraction (g_vposed, the fp32 directions, split partials) and the chain."""
    f, rows = 4, 3 * V
    nr, ns = (V + RV - 1) // RV, ((rows + 15) // 16 * 16 + RC - 1) // RC
    recompute = n * 512 * f + rows * K * f + n * rows * f                 # coefficient rows, directions (GEMM operand), v_posed
    skin = n * rows * f * 3 + n * nj * 3 * f + n * nr * J * 12 * f          # grad_vertices + v_posed in, g_vposed out; joints; g_A
    contraction = n * rows * f * ((K + 255) // 256) + rows * K * f + ns * n * K * f
    chain = ns * n * K * f + n * nr * J * 12 * f + n * 200 * f
    return recompute + skin + contraction + chain


def timed(fn, warmup, reps, windows):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)                      # us per call
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,512")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "smplx_grad_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    md = smplx_model.make_synthetic_model(4321)
    body = smplx.SMPLX(model_data=md)
    V, J = md["v_template"].shape[0], md["J_regressor"].shape[0]
    gen = torch.Generator().manual_seed(5)
    rows = []
    for n in [int(s) for s in args.sizes.split(",")]:
        for extra in (False, True):
            rot = lambda k: lbs.batch_rodrigues((torch.randn(k, 3, generator=gen) * 0.4).to(dev))  # noqa: E731
            inp = dict(betas=torch.randn(n, 10, generator=gen), expression=torch.randn(n, 10, generator=gen) * 0.5,
                       global_orient=rot(n).view(n, 1, 3, 3), body_pose=rot(n * 21).view(n, 21, 3, 3),
                       transl=torch.randn(n, 3, generator=gen))
            if extra:
                inp.update(jaw_pose=rot(n).view(n, 1, 3, 3), left_hand_pose=rot(n * 15).view(n, 15, 3, 3),
                           right_hand_pose=rot(n * 15).view(n, 15, 3, 3))
            inp = {k: v.to(dev).contiguous() for k, v in inp.items()}
            leaves = {k: v.clone().requires_grad_(True) for k, v in inp.items()}

            def fwd_nograd():
                with torch.no_grad():
                    body.forward(**inp, pose2rot=False)

            def fwd_grad():
                body.forward(**leaves, pose2rot=False)

            # backward alone: ap_smplx_bwd on the converted inputs with every gradient wanted (what _SmplxFunction.backward calls)
            ext = None
            if extra:
                eye = torch.eye(3, device=dev).expand(n, 1, 3, 3)
                ext = torch.cat([inp["jaw_pose"], eye, eye, inp["left_hand_pose"], inp["right_hand_pose"]], 1).contiguous()
            gv = torch.randn(n, V, 3, device=dev)
            gj = torch.randn(n, 127, 3, device=dev)
            outs = [torch.empty(n, k, device=dev) for k in (10, 10, 9, 21 * 9, (J - 22) * 9, 3)]
            if not extra:
                outs[4] = None
            with torch.cuda.device(dev):
                h = body._native(dev)
            L, sp = N.lib(), N.stream_ptr(dev)
            cargs = [h, n] + [N.dptr(t) for t in (inp["betas"], inp["expression"], inp["global_orient"], inp["body_pose"], ext,
                                                   inp["transl"], gv, gj)] + [N.dptr(t) for t in outs] + [sp]

            def bwd():
                N.check(L.ap_smplx_bwd(*cargs), "ap_smplx_bwd")

            t_f = timed(fwd_nograd, args.warmup, args.reps, args.windows)
            t_fg = timed(fwd_grad, args.warmup, args.reps, args.windows)
            t_b = timed(bwd, args.warmup, args.reps, args.windows)
            K = 512 if extra else 224
            nb = bwd_bytes(n, V, J, K)
            row = {"n": n, "poses": "hands+face" if extra else "body", "K": K,
                   "fwd_nograd_us": round(t_f[0], 1), "fwd_grad_us": round(t_fg[0], 1), "bwd_us": round(t_b[0], 1),
                   "bwd_us_min_max": [round(t_b[1], 1), round(t_b[2], 1)], "bwd_over_fwd": round(t_b[0] / t_f[0], 2),
                   "bwd_model_MB": round(nb / 1e6, 1), "bwd_model_TBps": round(nb / (t_b[0] * 1e-6) / 1e12, 2),
                   "frac_of_8TBps": round(nb / (t_b[0] * 1e-6) / HBM_PEAK, 3),
                   "bwd_mfma_GFLOP": round(2.0 * n * 3 * V * K / 1e9, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
