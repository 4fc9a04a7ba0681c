"""Time one optimizer step over the two-view model's parameters (copenet_sep: two ResNet-50 trunks and two IEF heads, 338 tensors,
54.2 M floats; the shapes come from airpose_amd's own model classes, values and gradients are random) on the GPU:

  fused_adam      airpose_amd.FusedAdam(amsgrad=True): apg_adam_step, ceil(tensors / 64) launches (ADAM_BATCH of csrc/optim.hip; the
                  count is read from the code, not measured)
  torch_foreach   torch.optim.Adam(amsgrad=True) at its defaults (the foreach path)
  torch_single    the same with foreach=False
  torch_fused     the same with fused=True, when the installed torch accepts it on this device; a refusal is recorded, not a failure

The candidates' windows take turns in one process (HIP events around --reps steps, the median of --windows windows and the spread
max - min), as tools/loss_bench.py does.  Every candidate steps its own copy of the parameters with the same fixed gradients.
bytes_per_step is the AMSGrad floor 36 B per parameter (p, g, m, v, vmax read, p, m, v, vmax written), floor_us that over --hbm-tbs
(DESIGN.md section 5 uses 8 TB/s), floor_frac = floor_us / step_us.  One JSON line per candidate; --out also writes them to a file.

    python tools/optim_bench.py [--reps 10] [--windows 9] [--out profiles/optim_bench.json]
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

from airpose_amd import FusedAdam, copenet_sep_model  # noqa: E402

MEAN = os.path.join(REPO, "airpose_amd", "data", "smpl_mean_params.npz")
ADAM_BATCH = 64          # csrc/optim.hip


def model_shapes():
    return [tuple(p.shape) for p in copenet_sep_model.getcopenet_sep(MEAN, precision="fp32").parameters()]


def timed_interleaved(fns, warmup, reps, windows):
    """per function the window times (us per call) of `windows` windows of `reps` calls, the functions' windows taking turns"""
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = model_shapes()
    nparam = sum(math.prod(s) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    start = [0.05 * torch.randn(s, generator=gen, device=dev) for s in shapes]
    grads = [1e-3 * torch.randn(s, generator=gen, device=dev) for s in shapes]

    def candidate(make):
        ps = [torch.nn.Parameter(t.clone()) for t in start]
        for p, g in zip(ps, grads):
            p.grad = g
        return make(ps)
    kw = dict(lr=args.lr, weight_decay=0, amsgrad=True)
    cands = [("fused_adam", candidate(lambda ps: FusedAdam(ps, **kw)), {"launches_per_step": -(-len(shapes) // ADAM_BATCH)}),
             ("torch_foreach", candidate(lambda ps: torch.optim.Adam(ps, **kw)), {}),
             ("torch_single", candidate(lambda ps: torch.optim.Adam(ps, foreach=False, **kw)), {})]
    refused = None
    try:
        opt = candidate(lambda ps: torch.optim.Adam(ps, fused=True, **kw))
        opt.step()
        torch.cuda.synchronize()
        cands.append(("torch_fused", opt, {}))
    except Exception as e:  # noqa: BLE001  (whatever this torch raises for an unsupported fused path is the record)
        refused = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
    times = timed_interleaved([c[1].step for c in cands], args.warmup, args.reps, args.windows)
    floor_us = 36.0 * nparam / (args.hbm_tbs * 1e12) * 1e6
    med = {name: statistics.median(t) for (name, _, _), t in zip(cands, times)}
    lines = []
    for (name, _, extra), t in zip(cands, times):
        rec = {"tool": "optim_bench", "candidate": name, "tensors": len(shapes), "parameters": nparam, "bytes_per_step": 36 * nparam,
               "step_us": round(med[name], 1), "spread_us": round(max(t) - min(t), 1), "min_us": round(min(t), 1),
               "floor_us": round(floor_us, 1), "floor_frac": round(floor_us / med[name], 3),
               "fused_adam_speedup": round(med[name] / med["fused_adam"], 2), "windows": args.windows, "reps": args.reps,
               "torch": torch.__version__}
        rec.update(extra)
        lines.append(rec)
    if refused is not None:
        lines.append({"tool": "optim_bench", "candidate": "torch_fused", "tensors": len(shapes), "parameters": nparam,
                      "bytes_per_step": 36 * nparam, "refused": refused, "torch": torch.__version__})
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    if med["fused_adam"] > med["torch_foreach"]:
        raise SystemExit("FusedAdam's median step (%.1f us) is longer than torch's default foreach step (%.1f us)"
                         % (med["fused_adam"], med["torch_foreach"]))


if __name__ == "__main__":
    main()
