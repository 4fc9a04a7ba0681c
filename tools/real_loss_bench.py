"""Time the fused real-data loss (airpose_amd.RealDataLoss, apg_real_loss_fwd_bwd) against the same two-view get_loss of the
copenet_real trainer written in eager torch (the VPoser encoder as its literal layer chain, tgm's rotation -> axis-angle conversion
as oracle/geometry_ref.py restates it in differentiable torch ops), on the GPU, at B in {32, 64} with J = 127 joints:

  fused_fwd_us / eager_fwd_us         the loss under no_grad
  fused_fwdbwd_us / eager_fwdbwd_us   the loss and loss.backward() down to the eight prediction tensors
  *_ops                               an OPERATOR count per call, this tool's stand-in for launches, as in tools/loss_bench.py: every
                                      aten operator dispatched during the call counts one unless its name is in VIEWS, every
                                      apg_real_loss_fwd_bwd call counts two (its two hipLaunchKernelGGL)

Both sides are given the same eps (the draw of rsample() is not timed).  The four candidates' windows take turns in one process (HIP
events around --reps calls, the median of --windows windows).  One JSON line per batch size; --out also writes them to a file.

    python tools/real_loss_bench.py [--sizes 32,64] [--reps 20] [--windows 7] [--out profiles/real_loss_bench.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loss_bench  # noqa: E402  (LaunchCount, timed_interleaved)
from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd.loss_real import DEFAULTS, ENCODER_KEYS, RealDataLoss  # noqa: E402
from oracle import geometry_ref  # noqa: E402  (tgm 0.1.2's rotation_matrix_to_angle_axis, restated in differentiable torch ops)

LIMB1, LIMB2 = [4, 5, 18, 19], [7, 8, 20, 21]
F = torch.nn.functional


def make_encoder(seed, dev):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in ENCODER_KEYS.items():
        if k.endswith("running_var"):
            t = torch.rand(*shape, generator=g) + 0.5
        elif len(shape) == 2:
            t = torch.randn(*shape, generator=g) / shape[1] ** 0.5
        elif k.endswith(".weight"):
            t = 1 + 0.2 * torch.randn(*shape, generator=g)
        else:
            t = 0.1 * torch.randn(*shape, generator=g)
        sd[k] = t.to(dev)
    return sd


def encode(sd, aa):
    """encoder_net in eval mode, layer by layer -> (mu, scale)"""
    p = lambda k: sd["encoder_net." + k]
    x = F.batch_norm(aa, p("1.running_mean"), p("1.running_var"), p("1.weight"), p("1.bias"), False, 0.1, 1e-5)
    x = F.leaky_relu(F.linear(x, p("2.weight"), p("2.bias")), 0.01)
    x = F.batch_norm(x, p("4.running_mean"), p("4.running_var"), p("4.weight"), p("4.bias"), False, 0.1, 1e-5)
    x = F.linear(F.linear(x, p("6.weight"), p("6.bias")), p("7.weight"), p("7.bias"))
    return F.linear(x, p("8.mu.weight"), p("8.mu.bias")), F.softplus(F.linear(x, p("8.logvar.weight"), p("8.logvar.bias")))


def eager_loss(h, sd, eps, batch, t0, t1, R0, R1, b0, b1, o0, o1, p0, p1):
    """the two-view get_loss of copenet_real in eager torch, term by term as the trainer writes it"""
    mse = lambda a, b: (a - b) ** 2
    g0, g1 = batch["smpl_joints_2d0"][:, 0], batch["smpl_joints_2d1"][:, 0]
    B = g0.shape[0]
    kp = mse(p0[:, :22], g0[:, :22, :2]) * g0[:, :22, 2:] + mse(p1[:, :22], g1[:, :22, :2]) * g1[:, :22, 2:]
    kp[:, LIMB1] *= h["limbs2d_loss_weight"]
    kp[:, LIMB2] *= h["limbs2d_loss_weight"] ** 2
    kp = kp.mean()
    vp = 0
    for R, e in ((R0, eps[0]), (R1, eps[1])):
        aa = torch.cat([R[:, 1:], torch.zeros(B, 21, 3, 1).type_as(R)], dim=3).view([-1, 3, 4])
        mu, scale = encode(sd, geometry_ref.rotation_matrix_to_angle_axis(aa).reshape([B, 63]))
        z = mu + scale * e
        vp = vp + torch.mul(z, z).mean()
    pose = mse(R0[:, 1:], R1[:, 1:]).mean()
    betas = torch.mul(b0, b0).mean() + torch.mul(b1, b1).mean() + mse(b0, b1).mean()
    loss = h["keypoint2d_loss_weight"] * kp + h["beta_loss_weight"] * betas + h["vposer_loss_weight"] * vp + \
        h["pose_loss_weight"] * pose + (torch.exp(-t0[:, 2]) ** 2).mean() + (torch.exp(-t1[:, 2]) ** 2).mean()
    return loss * 60


def count_ops(fn):
    """aten operators outside VIEWS + 2 per apg_real_loss_fwd_bwd call, over one call of fn"""
    calls = {"n": 0}
    lib = G.lib()

    class Spy(object):
        def __getattr__(self, name):
            f = getattr(lib, name)
            if name != "apg_real_loss_fwd_bwd":
                return f

            def counted(*a):
                calls["n"] += 1
                return f(*a)
            return counted
    real = G.lib
    G.lib = lambda: Spy()
    try:
        with loss_bench.LaunchCount() as m:
            fn()
    finally:
        G.lib = real
    torch.cuda.synchronize()
    return m.n + 2 * calls["n"]


def rotations(n, g):
    """n random rotations (Gram-Schmidt of normal 6-vectors)"""
    x = torch.randn(n, 3, 2, generator=g)
    b1 = F.normalize(x[:, :, 0], dim=1)
    b2 = F.normalize(x[:, :, 1] - (b1 * x[:, :, 1]).sum(1, keepdim=True) * b1, dim=1)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2, dim=1)), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--joints", type=int, default=127)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    J = args.joints
    h = DEFAULTS["twoview"]
    sd = make_encoder(1, dev)
    fused = RealDataLoss("twoview", sd)
    lines = []
    for B in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(B)
        r = lambda *s: torch.randn(*s, generator=g)
        gt = lambda: torch.cat([r(B, 1, J, 2) * 100 + 500, torch.rand(B, 1, J, 1, generator=g)], 3).to(dev)
        batch = {"smpl_joints_2d0": gt(), "smpl_joints_2d1": gt()}
        leaf = lambda t: t.to(dev).requires_grad_(True)
        trans = lambda: torch.cat([r(B, 2), torch.rand(B, 1, generator=g) * 6 + 0.5], 1)
        t0, t1 = leaf(trans()), leaf(trans())
        R0, R1 = leaf(rotations(B * 22, g).view(B, 22, 3, 3)), leaf(rotations(B * 22, g).view(B, 22, 3, 3))
        b0, b1 = leaf(r(B, 10)), leaf(r(B, 10))
        p0, p1 = leaf(r(B, J, 2) * 100 + 500), leaf(r(B, J, 2) * 100 + 500)
        eps = [r(B, 32).to(dev), r(B, 32).to(dev)]
        preds = (t0, t1, R0, R1, b0, b1, None, None, p0, p1)
        leaves = [t0, t1, R0, R1, b0, b1, p0, p1]

        def clear():
            for t in leaves:
                t.grad = None

        def fused_fwd():
            with torch.no_grad():
                fused(batch, *preds, eps=eps)

        def eager_fwd():
            with torch.no_grad():
                eager_loss(h, sd, eps, batch, *preds)

        def fused_fwdbwd():
            clear()
            fused(batch, *preds, eps=eps)[0].backward()

        def eager_fwdbwd():
            clear()
            eager_loss(h, sd, eps, batch, *preds).backward()
        a, b = float(fused(batch, *preds, eps=eps)[0].detach()), float(eager_loss(h, sd, eps, batch, *preds).detach())
        if abs(a - b) > 1e-4 * abs(b):
            raise SystemExit("fused loss %r against eager %r" % (a, b))
        fns = [fused_fwd, eager_fwd, fused_fwdbwd, eager_fwdbwd]
        launches = [count_ops(fn) for fn in fns]
        med, spread = loss_bench.timed_interleaved(fns, args.warmup, args.reps, args.windows)
        rec = {"tool": "real_loss_bench", "kind": "twoview", "B": B, "J": J,
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
