"""Time airpose_amd.SyntheticBatches.batch at the reference's sizes: n = 64 AerialPeople samples, canvases of 1080 x 1920 for both
cameras (origin "frame"), 10475 vertices and the body models' own joint count, seeded synthetic records (a person's box of about
250 x 500 px somewhere in the frame, three genders).

  batch       SyntheticBatches.batch: apg_synth_batch (two launches), apg_synth_crops (one), one SMPLX.forward per gender present
  eager       the same arithmetic with what the package offered before, in eager torch on the device: the draws (Philox in int64
              tensors) and the box arithmetic as tensor operators, utils.preprocess_crops per camera (which copies the boxes back to
              validate them), utils.transform_smpl and geometry.perspective_projection per camera, lbs.batch_rodrigues, the
              per-sample shuffle as torch.where over every per-view output, three masked SMPLX.forward
  *_ops       an OPERATOR count per call as in tools/loss_bench.py: every aten operator outside LaunchCount.VIEWS counts one, every
              call of a C entry point of the two libraries counts one (whatever it launches)
  *_host_copies   calls of Tensor.cpu / item / tolist / numpy on a CUDA tensor during one call: each blocks the host on the stream
  *_enqueue_us    host clock around the call WITHOUT a synchronise: what the host spends before it can go on
  moved_mb    the bytes the non-image part must move per batch (vertices and joints in, both cameras' out), from the shapes

The two take turns in one process (HIP events around --reps calls, the median of --windows windows and their max - min).  Before
anything is timed the two paths' outputs are compared (integers and images: equal; the fp32 chains: to 1e-3, eager torch may fuse
where the kernel rounds once).  One JSON line; --out also writes it to a file.

    python tools/synth_batch_bench.py [--n 64] [--height 1080] [--width 1920] [--out profiles/synth_batch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native as N  # noqa: E402
from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd import geometry, lbs, smplx, smplx_model, utils  # noqa: E402
from airpose_amd.synth_batches import SyntheticBatches  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402

COPIES = ("cpu", "item", "tolist", "numpy")
GENDERS = ("male", "female", "neutral")
MASK = 0xFFFFFFFF


def synthetic(n, H, W, V, J, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    x0, y0 = (r(n, 2) * (W - 300)).int(), (r(n, 2) * (H - 550)).int()
    w, h = (200 + r(n, 2) * 100).int(), (400 + r(n, 2) * 150).int()
    bb = torch.stack([torch.stack([x0, y0], -1), torch.stack([x0 + w, y0 + h], -1)], 2)      # (n, 2, 2, 2)
    intr = torch.tensor([[1475.0, 0, W / 2], [0, 1475.0, H / 2], [0, 0, 1]]).expand(n, 2, 3, 3).clone()
    q = torch.linalg.qr(torch.randn(n, 2, 3, 3, generator=g))[0]
    extr = torch.eye(4).expand(n, 2, 4, 4).clone()
    extr[..., :3, :3] = q
    extr[..., :3, 3] = torch.stack([2 * r(n, 2) - 1, 2 * r(n, 2) - 1, 8 + 4 * r(n, 2)], -1)
    rec = dict(bb=bb.int(), intr=intr, extr=extr, smplpose=0.3 * torch.randn(n, 63, generator=g), smplshape=torch.randn(n, 10, generator=g),
               smpl_vertices_wrt_origin=2 * r(n, 1, V, 3) - 1, smpl_joints_wrt_origin=r(n, 1, J, 3) - 0.5,
               smplorient_rotmat_wrt_origin=torch.linalg.qr(torch.randn(n, 1, 3, 3, generator=g))[0], smpltrans=4 * r(n, 3) - 2)
    genders = [GENDERS[i % 3] for i in range(n)]
    frames = torch.randint(0, 256, (2, n, H, W, 3), generator=g, dtype=torch.uint8)
    return rec, genders, frames, torch.arange(1000, 1000 + n, dtype=torch.int32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on int64 tensors holding 32-bit words"""
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57            # (wraps mod 2^64: the low 64 bits are the product's)
        c0, c1, c2, c3 = ((p1 >> 32) & MASK) ^ c1 ^ k0, p1 & MASK, ((p0 >> 32) & MASK) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def eager_batch(sb, models, rec, genders, frames, index, epoch=0, bgr=True):
    """the arithmetic of SyntheticBatches.batch (origin "frame") from the package's older pieces, in eager torch"""
    dev = frames.device
    n = frames.shape[1]
    H, W = sb.frame_size
    m = sb.margin
    idx = index.long() & MASK
    zero = torch.zeros_like(idx)
    k0, k1 = sb.seed & MASK, (sb.seed >> 32) & MASK
    flip = (philox(idx, zero + epoch, zero + 2, zero, k0, k1)[0] >> 31).bool()
    bb = rec["bb"].long()
    per_cam = []
    for c in (0, 1):
        w = philox(idx, zero + epoch, zero + c, zero, k0, k1)
        box = {}
        for a0, a1, S, w0, w1, ax in ((bb[:, c, 0, 1], bb[:, c, 1, 1], H, w[0], w[1], "y"), (bb[:, c, 0, 0], bb[:, c, 1, 0], W, w[2], w[3], "x")):
            c0, c1 = a0.clamp(0, S), a1.clamp(0, S)
            lo, hi = torch.where(c0 - m > 0, c0 - m, torch.zeros_like(c0)), torch.where(c1 + m < S, c1 + m, torch.full_like(c1, S))
            p0, p1 = lo + ((w0 * (c0 - lo)) >> 32), hi - ((w1 * (hi - c1)) >> 32)
            box[ax] = (lo, hi, p0, p1)
        (ylo, yhi, y0, y1), (xlo, xhi, x0, x1) = box["y"], box["x"]
        crops = torch.stack([y0, y1, x0, x1], 1).int()
        im, scale, pad = utils.preprocess_crops(frames[c], crops, bgr=bgr)
        K, E = rec["intr"][:, c], rec["extr"][:, c]
        centre = K[:, :2, 2]
        bbxy = torch.stack([(x0 + x1).float(), (y0 + y1).float()], 1) / 2 / centre - 1
        verts, joints, orient, trans = utils.transform_smpl(E, rec["smpl_vertices_wrt_origin"][:, 0], rec["smpl_joints_wrt_origin"][:, 0],
                                                            rec["smplorient_rotmat_wrt_origin"][:, 0], rec["smpltrans"])
        j2d = geometry.perspective_projection(joints, torch.eye(3, device=dev).expand(n, 3, 3), torch.zeros(n, 3, device=dev),
                                              sb.focal_length, centre)
        j2d_crop = scale[:, None, None] * (j2d - ((bbxy + 1) * centre)[:, None])
        per_cam.append(dict(im=im, intr=K, extr=E.unsqueeze(1), bb=torch.cat([bbxy, scale[:, None]], 1), crops=crops,
                            crop_info=torch.stack([ylo, xlo, yhi, xhi], 1).int().reshape(n, 2, 2), smpltrans_rel=trans,
                            smplorient_rel=orient.unsqueeze(1), smpl_vertices_rel=verts.unsqueeze(1), smpl_joints_rel=joints.unsqueeze(1),
                            smpl_joints_2d=j2d.unsqueeze(1), smpl_joints_2d_crop=j2d_crop, scale=scale, pad=pad))
    out = {"cam0": flip.int()}
    for k in per_cam[0]:                                     # the per-sample shuffle: suffix s is camera flip ^ s
        a, b = per_cam[0][k], per_cam[1][k]
        f = flip.reshape((n,) + (1,) * (a.dim() - 1))
        out[k + "0"], out[k + "1"] = torch.where(f, b, a), torch.where(f, a, b)
    rot = lbs.batch_rodrigues(rec["smplpose"].reshape(-1, 3)).reshape(n, 21, 3, 3)
    out["smplpose_rotmat"] = rot
    verts = joints = None
    for g in GENDERS:                                        # three masked forwards
        at = torch.tensor([i for i, x in enumerate(genders) if x == g], device=dev, dtype=torch.int64)
        k = at.numel()
        if not k:
            continue
        with torch.no_grad():
            body = models[g].forward(betas=rec["smplshape"][at], body_pose=rot[at], global_orient=torch.eye(3, device=dev).expand(k, 1, 3, 3),
                                     transl=torch.zeros(k, 3, device=dev), pose2rot=False)
        if verts is None:
            verts, joints = torch.empty(n, *body.vertices.shape[1:], device=dev), torch.empty(n, *body.joints.shape[1:], device=dev)
        verts[at], joints[at] = body.vertices, body.joints
    out["smpl_vertices"], out["smpl_joints"] = verts.unsqueeze(1), joints.unsqueeze(1)
    return out


def count(fn):
    """(operators, host copies) of one call of fn: aten operators outside VIEWS + one per call into either library"""
    calls = {"n": 0, "copies": 0}

    class Spy(object):
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if not callable(f) or name.endswith(("_last_error", "_bytes", "_num_joints_out")):
                return f

            def counted(*a):
                calls["n"] += 1
                return f(*a)
            return counted
    real_g, real_n = G.lib, N.lib
    spy_g, spy_n = Spy(G.lib()), Spy(N.lib())
    G.lib, N.lib = (lambda: spy_g), (lambda: spy_n)
    saved = {k: getattr(torch.Tensor, k) for k in COPIES}

    def patch(orig):
        def counted(self, *a, **k):
            if self.is_cuda:
                calls["copies"] += 1
            return orig(self, *a, **k)
        return counted
    for k, orig in saved.items():
        setattr(torch.Tensor, k, patch(orig))
    try:
        with LaunchCount() as m:
            fn()
    finally:
        G.lib, N.lib = real_g, real_n
        for k, orig in saved.items():
            setattr(torch.Tensor, k, orig)
    torch.cuda.synchronize()
    return m.n + calls["n"], calls["copies"]


def enqueue_us(fn, reps):
    """median host time of one call that is not followed by a synchronise (the queue is drained before each)"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seed", type=int, default=78)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("synth_batch_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    n, H, W = args.n, args.height, args.width
    models = {g: smplx.SMPLX(model_data=smplx_model.make_synthetic_model(4321 + k)) for k, g in enumerate(GENDERS)}
    probe = models["neutral"].forward(betas=torch.zeros(1, 10, device=dev), body_pose=torch.eye(3, device=dev).expand(1, 21, 3, 3).contiguous(),
                                      global_orient=torch.eye(3, device=dev).reshape(1, 1, 3, 3), transl=torch.zeros(1, 3, device=dev),
                                      pose2rot=False)
    V, J = int(probe.vertices.shape[1]), int(probe.joints.shape[1])
    rec, genders, frames, index = synthetic(n, H, W, V, J, args.seed)
    rec = {k: v.to(dev).contiguous() for k, v in rec.items()}
    frames, index = frames.to(dev), index.to(dev)
    rec["smplgender"] = genders
    sb = SyntheticBatches(models, device=dev, frame_size=(H, W), seed=args.seed)

    def batch():
        return sb.batch(rec, frames, index, origin="frame")

    def eager():
        return eager_batch(sb, models, rec, genders, frames, index)

    b, e = batch(), eager()
    torch.cuda.synchronize()
    same = {}
    for k in sorted(e):
        if b[k].dtype == torch.int32 or k.startswith("im"):
            same[k] = bool(torch.equal(b[k], e[k]))
        else:
            same[k] = float((b[k] - e[k]).abs().max())
    wrong = [k for k, v in same.items() if v is False or (v is not True and v > 1e-3)]
    if wrong:
        raise SystemExit("batch against the eager path: %r" % {k: same[k] for k in wrong})
    status = torch.stack([b["status0"], b["status1"]]).cpu()
    del b, e
    ops = [count(fn) for fn in (batch, eager)]
    med, spread = timed_interleaved([batch, eager], args.warmup, args.reps, args.windows)
    enq = [enqueue_us(fn, args.reps) for fn in (batch, eager)]
    moved = n * (V + J) * 3 * 4 * 3 + n * J * 2 * 4 * 4       # points in once and out twice; j2d and j2d_crop for two cameras
    rec_out = {"tool": "synth_batch_bench", "n": n, "height": H, "width": W, "verts": V, "joints": J,
               "batch_us": round(med[0], 1), "eager_us": round(med[1], 1), "eager_over_batch": round(med[1] / med[0], 2),
               "spread_us": [round(x, 1) for x in spread],
               "batch_enqueue_us": round(enq[0], 1), "eager_enqueue_us": round(enq[1], 1),
               "batch_ops": ops[0][0], "eager_ops": ops[1][0], "batch_host_copies": ops[0][1], "eager_host_copies": ops[1][1],
               "moved_mb": round(moved / 1e6, 1), "status_nonzero": int((status != 0).sum()),
               "max_abs_against_eager": {k: v for k, v in same.items() if v is not True}, "windows": args.windows, "reps": args.reps,
               "grad_lib": os.path.basename(G.LIB_PATH)}
    print(json.dumps(rec_out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec_out) + "\n")


if __name__ == "__main__":
    main()
