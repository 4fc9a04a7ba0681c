"""Time the trainable IEF head (copenet.forward_reg / forward_ief on libairpose_grad.so) on the GPU, in train mode with both
dropouts active, at B in {8, 64, 256, 1024} view pairs:

  fwd_us       one forward_reg forward on the grad path (apg_head_fwd)
  fwdbwd_us    one forward_reg forward + backward (weights, state and feature gradients)
  step_us      one 3-iteration head training step: forward_ief(iters=3) + backward
  eager_us     the same 3-iteration step in torch eager fp32 autograd (torch.cat + F.linear + F.dropout) on the same GPU
  step_tflops  the step's matrix FLOPs / step_us, and its fraction of the 157.3 TF fp32 matrix peak

HIP events around windows of --reps calls after --warmup calls; the median of --windows windows is reported per call.  One JSON
line per batch size; --out also writes them to a file.

    python tools/head_grad_bench.py [--sizes 8,64,256,1024] [--reps 10] [--windows 5] [--out profiles/x.json]

--model {step,sep,hmr,muhmr,singleview} times the view-local / baseline heads behind set_trainable(True) (head_local_grad.py,
apg_head_local_fwd / _bwd) instead: per batch size B one forward_reg evaluation (step: copenet.regressor_step on B rows; sep: the
two regressor_step calls of copenet_sep.forward_reg; muhmr: 2B rows), forward and forward + backward, next to
  merged_*     the merged two-view head (apg_head_fwd / apg_head_bwd) at the SAME row count, windows interleaved in one process
  eager_*      the same evaluation in torch eager fp32 autograd (torch.cat + F.linear + F.dropout)
--model copenet (the default) is the two-view output described above, unchanged.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from airpose_amd import copenet_model  # noqa: E402
from airpose_amd import weights as W   # noqa: E402

PEAK = 157.3e12
MEAN = os.path.join(REPO, "airpose_amd", "data", "smpl_mean_params.npz")


def reg_flops(B, gxf):
    """Matrix FLOPs of one forward_reg at R = 2B rows: forward fc1 / fc2 / decoders; backward the three weight gradients, the
    two hidden-layer gradients and g_xc (state columns, + the 2048 feature columns when gxf)."""
    R = 2 * B
    fwd = 2 * R * (2332 * 1024 + 1024 * 1024 + 1024 * 145)
    bwd = 2 * R * (145 * 1024 + 1024 * 1024 + 1024 * 2332 + 145 * 1024 + 1024 * 1024 + 1024 * (2332 if gxf else 284))
    return fwd, bwd


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
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out)


def eager_step(sd, xf0, xf1, bb0, bb1, pos0, pos1, init_pose, init_shape, iters, p=0.5):
    lin = lambda x, n: F.linear(x, sd[n + ".weight"], sd[n + ".bias"])
    B = xf0.shape[0]
    o0 = o1 = init_pose[:, :6].expand(B, -1)
    a0 = a1 = init_pose[:, 6:132].expand(B, -1)
    s0 = s1 = init_shape.expand(B, -1)
    q0, q1 = pos0, pos1
    for _ in range(iters):
        outs = []
        for xf, bb, q, o, a, s, pa, ps in ((xf0, bb0, q0, o0, a0, s0, a1, s1), (xf1, bb1, q1, o1, a1, s1, a0, s0)):
            h = F.dropout(lin(F.dropout(lin(torch.cat([xf, bb, q, o, a, s, pa, ps], 1), "fc1"), p), "fc2"), p)
            outs += [torch.cat([q, o, a], 1) + lin(h, "decpose"), s + lin(h, "decshape")]
        P0, b0, P1, b1 = outs
        q0, q1, o0, o1, a0, a1, s0, s1 = P0[:, :3], P1[:, :3], P0[:, 3:9], P1[:, 3:9], P0[:, 9:], P1[:, 9:], b0, b1
    return P0, b0, P1, b1


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


def eager_local(net, model, xf, segs, p=0.5):
    """one evaluation of head_local_grad.LAYOUTS[model] in torch eager"""
    from airpose_amd.head_local_grad import LAYOUTS
    xc = torch.cat([xf] + list(segs), 1)
    h = F.dropout(net.fc2(F.dropout(net.fc1(xc), p)), p)
    return [xc[:, 2048 + r:2048 + r + n] + getattr(net, d)(h) for d, n, r in LAYOUTS[model][1]]


def main_local(args):
    from airpose_amd import copenet_sep_model, copenet_singleview_model, head_local_grad, hmr_model, muhmr_model
    dev = torch.device("cuda", 0)
    model = args.model

    def make(mod, variant, seed):
        net = mod.getcopenet(MEAN, precision="fp32")
        net.load_state_dict(W.to_torch(W.copenet_state_dict(seed, MEAN, variant=variant)))
        return net.to(dev).set_trainable(True).train()
    merged = make(copenet_model, "copenet", 20240901)
    if model in ("step", "sep"):
        nets = [make(copenet_model, "copenet", 20240901 + i) for i in range(2 if model == "sep" else 1)]
        layout = "step"
    else:
        mod = {"hmr": hmr_model, "muhmr": muhmr_model, "singleview": copenet_singleview_model}[model]
        nets, layout = [make(mod, model, 20240901)], model
    seg_w = [w for _, w in head_local_grad.LAYOUTS[layout][0]]
    lines = []
    for B in [int(s) for s in args.sizes.split(",")]:
        R = 2 * B if model == "muhmr" else B                 # rows of one generic-head call
        calls = 2 if model == "sep" else 1
        rows = R * calls
        if rows % 2:
            raise SystemExit("--model %s at B = %d is %d rows: the two-view yardstick needs an even count" % (model, B, rows))
        g = torch.Generator().manual_seed(B)
        data = []
        for _ in range(calls):
            xf = torch.relu(torch.randn(R, 2048, generator=g)).to(dev).requires_grad_(True)
            data.append((xf, [torch.randn(R, w, generator=g).to(dev).requires_grad_(True) for w in seg_w]))
        Bm = rows // 2                                        # the merged head at the same row count
        mxf = [torch.relu(torch.randn(Bm, 2048, generator=g)).to(dev).requires_grad_(True) for _ in range(2)]
        mst = [torch.randn(Bm, w, generator=g).to(dev).requires_grad_(True) for w in (3, 3, 3, 3, 6, 6, 126, 126, 10, 10)]

        def new():
            outs = []
            for net, (xf, segs) in zip(nets, data):
                outs += head_local_grad.head(net, layout, xf, segs)
            return outs

        def old():
            return merged.forward_reg(*mxf, *mst)

        def eager():
            outs = []
            for net, (xf, segs) in zip(nets, data):
                outs += eager_local(net, layout, xf, segs)
            return outs

        def nograd(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        def withbwd(fn):
            return lambda: sum(o.sum() for o in fn()).backward()
        fns = [nograd(new), nograd(old), nograd(eager), withbwd(new), withbwd(old), withbwd(eager)]
        med, spread = timed_interleaved(fns, args.warmup, args.reps, args.windows)
        rec = {"tool": "head_grad_bench", "model": model, "B": B, "rows": rows, "calls": calls,
               "fwd_us": round(med[0], 1), "merged_fwd_us": round(med[1], 1), "eager_fwd_us": round(med[2], 1),
               "fwdbwd_us": round(med[3], 1), "merged_fwdbwd_us": round(med[4], 1), "eager_fwdbwd_us": round(med[5], 1),
               "spread_us": [round(x, 1) for x in spread], "windows": args.windows, "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        for net in nets + [merged]:
            net.zero_grad(set_to_none=True)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="copenet", choices=("copenet", "step", "sep", "hmr", "muhmr", "singleview"))
    ap.add_argument("--sizes", default="8,64,256,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.model != "copenet":
        return main_local(args)
    dev = torch.device("cuda", 0)
    net = copenet_model.getcopenet(MEAN, precision="fp32")
    net.load_state_dict(W.to_torch(W.copenet_state_dict(20240901, MEAN)))
    net = net.to(dev).train()
    sd = {n: p for n, p in net.named_parameters() if n.split(".")[0] in ("fc1", "fc2", "decpose", "decshape")}
    lines = []
    for B in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(B)
        xf0 = torch.relu(torch.randn(B, 2048, generator=g)).to(dev).requires_grad_(True)
        xf1 = torch.relu(torch.randn(B, 2048, generator=g)).to(dev).requires_grad_(True)
        bb0, bb1 = (torch.rand(B, 3, generator=g).to(dev) + 0.2 for _ in range(2))
        pos0, pos1 = (torch.tensor([[0., 0., 10.]]).expand(B, 3).contiguous().to(dev) for _ in range(2))
        st = [torch.randn(B, w, generator=g).to(dev) for w in (6, 6, 126, 126, 10, 10)]
        reg_in = (xf0, xf1, bb0, bb1, pos0, pos1) + tuple(st)

        def fwd():
            with torch.no_grad():
                net.forward_reg(*reg_in)

        def fwdbwd():
            sum(o.sum() for o in net.forward_reg(*reg_in)).backward()

        def step():
            sum(o.sum() for o in net.forward_ief(xf0, xf1, bb0, bb1, pos0, pos1, iters=3)).backward()

        def eager():
            sum(o.sum() for o in eager_step(sd, xf0, xf1, bb0, bb1, pos0, pos1, net.init_pose, net.init_shape, 3)).backward()

        t_f = timed(fwd, args.warmup, args.reps, args.windows)
        t_fb = timed(fwdbwd, args.warmup, args.reps, args.windows)
        t_s = timed(step, args.warmup, args.reps, args.windows)
        t_e = timed(eager, args.warmup, args.reps, args.windows)
        f, b = reg_flops(B, True)
        step_flops = 3 * (f + b)
        rec = {"tool": "head_grad_bench", "pairs": B, "rows": 2 * B, "fwd_us": round(t_f, 1), "fwdbwd_us": round(t_fb, 1),
               "step_us": round(t_s, 1), "eager_us": round(t_e, 1), "step_vs_eager": round(t_e / t_s, 2),
               "step_gflop": round(step_flops / 1e9, 2), "step_tflops": round(step_flops / t_s / 1e6, 2),
               "step_peak_frac": round(step_flops / t_s / 1e6 / (PEAK / 1e12), 4), "peak_tflops": PEAK / 1e12}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        net.zero_grad(set_to_none=True)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
