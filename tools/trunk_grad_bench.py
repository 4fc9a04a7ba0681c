"""Time the trainable ResNet-50 trunk (copenet.forward_feat_ext after set_trunk_trainable(True), libairpose_grad.so) on the GPU,
in train mode (batch-statistics BatchNorm), at B in {8, 32, 64} view pairs -- both views, as two trunk calls of B crops each, the
way the reference's training_step runs them:

  fwd_ms        the two views' train-mode trunk forwards (no graph)
  fwdbwd_ms     the two views' trunk forwards + backward (every conv weight, gamma and beta)
  eager_fwd_ms / eager_fwdbwd_ms   the same in torch eager fp32 (F.conv2d / F.batch_norm / F.max_pool2d / F.avg_pool2d, i.e.
                MIOpen) on the same GPU: the yardstick
  step_ms       the full reference step: both trunks, the 3-iteration head, rot6d, SMPL-X, transform_smpl, the projection, a
                get_loss-style loss, backward
  fwdbwd_tflops the trunk's convolution FLOPs (forward, data and weight gradients) / fwdbwd_ms, and the fraction of the 157.3 TF
                fp32 matrix peak

HIP events around windows of --reps calls after --warmup calls; the median of --windows windows is reported per call.  One JSON line
per batch size; --out also writes them to a file.

--precision {fp32,bf16} times the trunk in that mode (set_trunk_trainable(True, precision=...)) and, in the same process with the
windows of all candidates interleaved round-robin (so clocks and neighbours drift over all alike), the fp32 path of the same build
(fp32_fwd_ms / fp32_fwdbwd_ms), torch eager fp32 and torch eager under autocast(bfloat16) (autocast_fwd_ms / autocast_fwdbwd_ms);
the peak fraction is then against the 2.5 PF bf16 matrix peak for bf16.  Without the flag the output is what it always was.

    python tools/trunk_grad_bench.py [--sizes 8,32,64] [--reps 3] [--windows 3] [--precision bf16] [--out profiles/x.json]
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

from airpose_amd import copenet_model, geometry, smplx, smplx_model, utils  # noqa: E402
from airpose_amd import weights as W   # noqa: E402

PEAK = 157.3e12
MEAN = os.path.join(REPO, "airpose_amd", "data", "smpl_mean_params.npz")


def conv_flops(n):
    """(forward, backward) multiply-add FLOPs x 2 of the 53 convolutions at n crops; backward = data + weight gradients (no data
    gradient for the stem: the crops need none)."""
    geo = [(112, 3, 64, 7)]                                  # (output size, C_in, C_out, kernel)
    H, C = 56, 64
    for li, (nb, p) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512))):
        for b in range(nb):
            Ho = H // 2 if (b == 0 and li > 0) else H
            geo += [(H, C, p, 1), (Ho, p, p, 3), (Ho, p, 4 * p, 1)]
            if b == 0:
                geo.append((Ho, C, 4 * p, 1))
            H, C = Ho, 4 * p
    fwd = sum(2 * n * o * o * k * ci * r * r for o, ci, k, r in geo)
    return fwd, 2 * fwd - 2 * n * 112 * 112 * 64 * 3 * 49


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
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def timed_interleaved(fns, warmup, reps, windows, between):
    """{name: median ms per call}: one window of every candidate per round, `windows` rounds"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
        between()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
            between()
    return {k: round(statistics.median(v), 3) for k, v in out.items()}


def eager_trunk(net, x):
    """forward_feat_ext in torch eager fp32 with train-mode BatchNorm (the module's own running buffers updated)."""
    def cbr(x, conv, bn, relu=True, res=None):
        y = F.batch_norm(F.conv2d(x, conv.weight, stride=conv.stride, padding=conv.padding), bn.running_mean, bn.running_var,
                         bn.weight, bn.bias, True, bn.momentum, bn.eps)
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y
    x = F.max_pool2d(cbr(x, net.conv1, net.bn1), 3, 2, 1)
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            out = cbr(cbr(x, blk.conv1, blk.bn1), blk.conv2, blk.bn2)
            res = x if blk.downsample is None else cbr(x, blk.downsample[0], blk.downsample[1], relu=False)
            x = cbr(out, blk.conv3, blk.bn3, res=res)
    return F.avg_pool2d(x, 7, stride=1).flatten(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,32,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    net = copenet_model.getcopenet(MEAN, precision="fp32")
    net.load_state_dict(W.to_torch(W.copenet_state_dict(20240901, MEAN)))
    net = net.to(dev).train().set_trunk_trainable(True)
    body = smplx.SMPLX(model_data=smplx_model.make_synthetic_model(4321))
    lines = []
    for B in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(B)
        x0, x1 = (torch.randn(B, 3, 224, 224, generator=g).to(dev) for _ in range(2))
        bb0, bb1 = (torch.rand(B, 3, generator=g).to(dev) + 0.2 for _ in range(2))
        pos = torch.tensor([[0., 0., 10.]]).expand(B, 3).contiguous().to(dev)
        j2d = (torch.randn(B, 22, 2, generator=g) * 100 + 500).to(dev)
        j3d = torch.randn(B, 22, 3, generator=g).to(dev)
        eye = torch.eye(3, device=dev).expand(B, 1, 3, 3)
        cc = torch.full((B, 2), 500., device=dev)

        def fwd():
            with torch.no_grad():
                net.forward_feat_ext(x0)
                net.forward_feat_ext(x1)

        def fwdbwd():
            (net.forward_feat_ext(x0).sum() + net.forward_feat_ext(x1).sum()).backward()

        def eager_fwd():
            with torch.no_grad():
                eager_trunk(net, x0)
                eager_trunk(net, x1)

        def eager_fwdbwd():
            (eager_trunk(net, x0).sum() + eager_trunk(net, x1).sum()).backward()

        def step():
            p0, b0, p1, b1 = net(x0, x1, bb0, bb1, pos, pos)
            loss = 0.
            for pose, betas in ((p0, b0), (p1, b1)):
                rotmat = geometry.rot6d_to_rotmat(pose[:, 3:]).view(B, 22, 3, 3)
                o = body.forward(betas=betas, body_pose=rotmat[:, 1:], global_orient=eye, transl=torch.zeros(B, 3, device=dev),
                                 pose2rot=False)
                M = torch.cat([rotmat[:, 0], pose[:, :3].unsqueeze(2)], dim=2)
                _, jc = utils.transform_smpl(M, o.vertices, o.joints)[:2]
                pj = geometry.perspective_projection(jc, None, None, (5000., 5000.), cc)
                loss = loss + ((pj[:, :22] - j2d) ** 2).mean() * 1e-4 + ((jc[:, :22] - j3d) ** 2).mean() + (betas ** 2).mean()
            loss.backward()

        if args.precision is not None:
            def mode(precision, fn):
                def run():
                    net.set_trunk_trainable(True, precision=precision)
                    fn()
                return run

            def autocast(fn):
                def run():
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        fn()
                return run
            res = timed_interleaved({"fwd_ms": mode(args.precision, fwd), "fwdbwd_ms": mode(args.precision, fwdbwd),
                                     "fp32_fwd_ms": mode("fp32", fwd), "fp32_fwdbwd_ms": mode("fp32", fwdbwd),
                                     "eager_fwd_ms": eager_fwd, "eager_fwdbwd_ms": eager_fwdbwd,
                                     "autocast_fwd_ms": autocast(eager_fwd), "autocast_fwdbwd_ms": autocast(eager_fwdbwd),
                                     "step_ms": mode(args.precision, step)}, args.warmup, args.reps, args.windows,
                                    lambda: net.zero_grad(set_to_none=True))
            f, b = conv_flops(2 * B)
            peak = 2.5e15 if args.precision == "bf16" else PEAK
            L = __import__("airpose_amd._native_grad", fromlist=["lib"]).lib()
            rec = {"tool": "trunk_grad_bench", "precision": args.precision, "pairs": B, "images": 2 * B, **res,
                   "fwdbwd_vs_fp32_path": round(res["fp32_fwdbwd_ms"] / res["fwdbwd_ms"], 2),
                   "fwdbwd_vs_eager": round(res["eager_fwdbwd_ms"] / res["fwdbwd_ms"], 2),
                   "fwdbwd_vs_autocast": round(res["autocast_fwdbwd_ms"] / res["fwdbwd_ms"], 2),
                   "fwd_vs_eager": round(res["eager_fwd_ms"] / res["fwd_ms"], 2),
                   "fwdbwd_tflop": round((f + b) / 1e12, 3), "fwdbwd_tflops": round((f + b) / res["fwdbwd_ms"] / 1e9, 2),
                   "fwdbwd_peak_frac": round((f + b) / res["fwdbwd_ms"] / 1e9 / (peak / 1e12), 4), "peak_tflops": peak / 1e12,
                   "save_workspace_bytes_per_call": int(L.apg_trunk_workspace_bytes_p(B, 1, 1 if args.precision == "bf16" else 0)),
                   "save_workspace_bytes_n64": {"bf16": int(L.apg_trunk_workspace_bytes_p(64, 1, 1)),
                                                "fp32": int(L.apg_trunk_workspace_bytes_p(64, 1, 0))}}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            continue
        res = {}
        for name, fn in (("fwd_ms", fwd), ("fwdbwd_ms", fwdbwd), ("eager_fwd_ms", eager_fwd), ("eager_fwdbwd_ms", eager_fwdbwd),
                         ("step_ms", step)):
            res[name] = round(timed(fn, args.warmup, args.reps, args.windows), 3)
            net.zero_grad(set_to_none=True)
        f, b = conv_flops(2 * B)
        rec = {"tool": "trunk_grad_bench", "pairs": B, "images": 2 * B, **res,
               "fwdbwd_vs_eager": round(res["eager_fwdbwd_ms"] / res["fwdbwd_ms"], 2),
               "fwd_vs_eager": round(res["eager_fwd_ms"] / res["fwd_ms"], 2),
               "fwdbwd_tflop": round((f + b) / 1e12, 3), "fwdbwd_tflops": round((f + b) / res["fwdbwd_ms"] / 1e9, 2),
               "fwdbwd_peak_frac": round((f + b) / res["fwdbwd_ms"] / 1e9 / (PEAK / 1e12), 4), "peak_tflops": PEAK / 1e12}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
