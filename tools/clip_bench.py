"""Time gradient clipping in front of the optimizer step over the two-view model's parameters (tools/optim_bench.py's set: 338 tensors,
54.2 M floats, random values and gradients) on the GPU:

  adam                 (a) airpose_amd.FusedAdam(amsgrad=True) alone: apg_adam_step
  torch_clip_adam      (b) torch.nn.utils.clip_grad_norm_(max_norm=1) + the same FusedAdam: what Lightning's --gradient_clip_val runs
  fused_clip_adam      (c) airpose_amd.clip_grad_norm_(max_norm=1) + the same FusedAdam: apg_grad_norm, apg_grad_scale, apg_adam_step
  guarded_adam         (d) FusedAdam(max_grad_norm=1.0, skip_nonfinite=True): apg_grad_norm, apg_adam_step_guarded

The candidates' windows take turns in one process (HIP events around --reps steps, the median of --windows windows and the spread
max - min), as tools/optim_bench.py does.  Every candidate steps its own copy of the parameters and owns its gradients, which start
with a norm of about 7.4.  (b) and (c) rewrite theirs: after their first step the norm sits at max_norm, and the coefficient
max_norm / (norm + 1e-6) stays just below 1, so every later step still takes the full clipping path (the multiply is not skipped);
(d) never writes a gradient and clips by 1 / 7.4 every step.
norm_pass_us = (d) - (a) and norm_pass_tbs = 4 B per parameter over it: what the one extra read of the gradients costs.  holds: the
median of (d) is shorter than that of (b) by more than the larger of the two spreads.  One JSON line per candidate and one summary
line, written to --out as well.

    python tools/clip_bench.py [--reps 10] [--windows 9] [--out profiles/clip_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import FusedAdam, clip_grad_norm_  # noqa: E402
from optim_bench import model_shapes, timed_interleaved  # noqa: E402

GRAD_NORM_BATCH, ADAM_BATCH = 192, 64      # include/airpose_grad.h: APG_GRAD_NORM_BATCH; csrc/adam_seq.inc: ADAM_BATCH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = model_shapes()
    n = len(shapes)
    nparam = sum(math.prod(s) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    start = [0.05 * torch.randn(s, generator=gen, device=dev) for s in shapes]
    grads = [1e-3 * torch.randn(s, generator=gen, device=dev) for s in shapes]
    kw = dict(lr=args.lr, weight_decay=0, amsgrad=True)

    def candidate(clip=None, **opts):
        ps = [torch.nn.Parameter(t.clone()) for t in start]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt = FusedAdam(ps, **dict(kw, **opts))
        if clip is None:
            return opt, opt.step

        def step():
            clip(ps, args.max_norm)
            opt.step()
        return opt, step
    adam_launches = -(-n // ADAM_BATCH)
    norm_launches = 2 * -(-n // GRAD_NORM_BATCH) + 1
    cands = [("adam", candidate(), adam_launches),
             ("torch_clip_adam", candidate(torch.nn.utils.clip_grad_norm_), None),
             ("fused_clip_adam", candidate(clip_grad_norm_), norm_launches + -(-n // GRAD_NORM_BATCH) + adam_launches),
             ("guarded_adam", candidate(max_grad_norm=args.max_norm, skip_nonfinite=True), norm_launches + adam_launches)]
    times = timed_interleaved([c[1][1] for c in cands], args.warmup, args.reps, args.windows)
    med = {name: statistics.median(t) for (name, _, _), t in zip(cands, times)}
    spread = {name: max(t) - min(t) for (name, _, _), t in zip(cands, times)}
    lines = []
    for (name, _, launches), t in zip(cands, times):
        rec = {"tool": "clip_bench", "candidate": name, "tensors": n, "parameters": nparam, "step_us": round(med[name], 1),
               "spread_us": round(spread[name], 1), "min_us": round(min(t), 1), "windows": args.windows, "reps": args.reps,
               "max_norm": args.max_norm, "torch": torch.__version__}
        if launches is not None:
            rec["launches_per_step"] = launches
        lines.append(rec)
    skipped = cands[3][1][0].skipped_steps()
    norm_us = med["guarded_adam"] - med["adam"]
    margin = med["torch_clip_adam"] - med["guarded_adam"]
    holds = margin > max(spread["torch_clip_adam"], spread["guarded_adam"])
    lines.append({"tool": "clip_bench", "summary": True, "norm_pass_us": round(norm_us, 1), "norm_pass_bytes": 4 * nparam,
                  "norm_pass_tbs": round(4 * nparam / (norm_us * 1e-6) / 1e12, 2) if norm_us > 0 else None,
                  "torch_clip_minus_guarded_us": round(margin, 1),
                  "larger_spread_us": round(max(spread["torch_clip_adam"], spread["guarded_adam"]), 1), "holds": bool(holds),
                  "fused_clip_minus_guarded_us": round(med["fused_clip_adam"] - med["guarded_adam"], 1), "guarded_skipped_steps": skipped})
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    if not holds:
        raise SystemExit("the guarded step's median (%.1f us) is not shorter than torch's clip + step (%.1f us) by more than the larger "
                         "spread (%.1f us)" % (med["guarded_adam"], med["torch_clip_adam"], max(spread["torch_clip_adam"], spread["guarded_adam"])))


if __name__ == "__main__":
    main()
