"""Time airpose_amd.CameraRoll at the trainers' size: a SyntheticBatches dict of n = 64 samples and both views, 1080 x 1920 canvases,
person-sized boxes (about 250 x 500 px), V = 10475 vertices and J = 127 joints per view, every (sample, view) rolled (p = 1, 30 degrees).

  call        CameraRoll.__call__: apg_roll_draw + apg_roll_labels + apg_roll_crops (three launches)
  apply       CameraRoll.apply alone, on angles drawn before
  eager       the same arithmetic in eager torch on the device, from the SAME angles: the labels as batched bmm / elementwise
              operators (Rz on vertices, joints, trans, orient and extr; A(theta) on the 2-D tables and on bb; the refusal as a
              torch.where on the angles), the images per (sample, view) as affine_grid + grid_sample (bilinear, zeros) ON THE CROPPED
              REGION, letter-boxed and normalised.  Its boxes are read to the host once, before anything is timed -- a step the
              kernels do not need and the timing does not charge.  Outside the box it sees zeros where the kernel sees the canvas,
              so the images are compared where all four taps lie inside the box.
  copy        ONE device copy that moves the bytes the roll must read and write: every label read and written, im written, the
              boxes' canvas bytes read
  *_ops       an OPERATOR count per call as in tools/augment_bench.py

The four take turns in one process (HIP events around --reps calls, the median of --windows windows and their max - min).  Before
anything is timed the kernels' labels are compared with the eager path's (1e-3 of a pixel / 1e-5 of a metre) and the images where
the two are defined alike (5e-3 in normalised units: affine_grid's fp32 grid places a tap to 1e-4 of a pixel on noise).  One JSON line; --out also writes it to a file.

    python tools/roll_bench.py [--n 64] [--out profiles/roll_bench.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd import smplx, smplx_model  # noqa: E402
from airpose_amd.roll import CameraRoll  # noqa: E402
from airpose_amd.synth_batches import SyntheticBatches  # noqa: E402
from augment_bench import count  # noqa: E402
from loss_bench import timed_interleaved  # noqa: E402
from synth_batch_bench import synthetic  # noqa: E402

IMG = 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROLLED = ("smpl_vertices_rel", "smpl_joints_rel", "smplorient_rel", "smpltrans_rel", "extr", "smpl_joints_2d", "smpl_joints_2d_crop", "bb")


def eager_labels(batch, rot):
    """-> the rolled labels as (2, n, ...) tensors, and the (c, sn) in force"""
    both = lambda k: torch.stack([batch[k + "0"], batch[k + "1"]])
    K, bb = both("intr"), both("bb")
    n = bb.shape[1]
    c, sn = rot[..., 0], rot[..., 1]
    cx, cy = K[..., 0, 2], K[..., 1, 2]
    kx, ky = K[..., 0, 0] / K[..., 1, 1], K[..., 1, 1] / K[..., 0, 0]
    u, v = bb[..., 0] * cx, bb[..., 1] * cy
    nbx, nby = (c * u - sn * kx * v) / cx, (sn * ky * u + c * v) / cy
    refused = ~((nbx.abs() <= 1) & (nby.abs() <= 1))
    c, sn = torch.where(refused, torch.ones_like(c), c), torch.where(refused, torch.zeros_like(sn), sn)
    tx, ty = sn * kx, sn * ky
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    Rz = torch.stack([c, -sn, zero, sn, c, zero, zero, zero, one], -1).reshape(2 * n, 3, 3)
    A = torch.stack([c, -tx, ty, c], -1).reshape(2 * n, 2, 2)
    R4 = torch.eye(4, device=c.device).repeat(2 * n, 1, 1)
    R4[:, :3, :3] = Rz
    out = {}
    for k in ("smpl_vertices_rel", "smpl_joints_rel", "smpltrans_rel"):
        t = both(k)
        out[k] = torch.bmm(t.reshape(2 * n, -1, 3), Rz.transpose(1, 2)).reshape(t.shape)
    t = both("smplorient_rel")
    out["smplorient_rel"] = torch.bmm(Rz, t.reshape(2 * n, 3, 3)).reshape(t.shape)
    t = both("extr")
    out["extr"] = torch.bmm(R4, t.reshape(2 * n, 4, 4)).reshape(t.shape)
    centre = torch.stack([cx, cy], -1).reshape(2 * n, 1, 2)
    t = both("smpl_joints_2d")
    out["smpl_joints_2d"] = (centre + torch.bmm(t.reshape(2 * n, -1, 2) - centre, A.transpose(1, 2))).reshape(t.shape)
    t = both("smpl_joints_2d_crop")
    out["smpl_joints_2d_crop"] = torch.bmm(t.reshape(2 * n, -1, 2), A.transpose(1, 2)).reshape(t.shape)
    u, v = bb[..., 0] * cx, bb[..., 1] * cy
    out["bb"] = torch.stack([(c * u - tx * v) / cx, (ty * u + c * v) / cy, bb[..., 2]], -1)
    return out, torch.stack([c, sn, tx, ty], -1)


def eager_images(frames, boxes, cams, turn, bgr=True, coverage=False):
    """(2, n, 3, 224, 224): per (suffix, sample) affine_grid + grid_sample on the cropped region; boxes and cams are HOST lists"""
    dev = frames.device
    n = frames.shape[1]
    mean, std = torch.tensor(MEAN, device=dev).reshape(3, 1, 1), torch.tensor(STD, device=dev).reshape(3, 1, 1)
    out = ((torch.zeros(3, 1, 1, device=dev) - mean) / std).expand(2, n, 3, IMG, IMG).clone()
    if coverage:
        out.zero_()
    for s in (0, 1):
        for i in range(n):
            y0, y1, x0, x1 = boxes[s][i]
            h, w = y1 - y0, x1 - x0
            scale = 224.0 / max(h, w)
            dw, dh = int(scale * w), int(scale * h)
            top, left = (IMG - dh) // 2, (IMG - dw) // 2
            c, sn, tx, ty = turn[s, i]
            theta = torch.stack([c, tx * (h / w), (1 - c - tx) / w, -ty * (w / h), c, (1 - c + ty) / h]).reshape(1, 2, 3)
            grid = F.affine_grid(theta, (1, 3, dh, dw), align_corners=False)
            if coverage:
                out[s, i, :, top:top + dh, left:left + dw] = F.grid_sample(torch.ones(1, 1, h, w, device=dev), grid, mode="bilinear",
                                                                           padding_mode="zeros", align_corners=False)[0]
                continue
            region = frames[cams[i] ^ s, i, y0:y1, x0:x1]
            region = (region.flip(-1) if bgr else region).permute(2, 0, 1).float() / 255
            v = F.grid_sample(region[None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]
            out[s, i, :, top:top + dh, left:left + dw] = (v - mean) / std
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--verts", type=int, default=10475)
    ap.add_argument("--joints", type=int, default=127)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seed", type=int, default=80)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roll_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    n, H, W = args.n, args.height, args.width
    models = {"neutral": smplx.SMPLX(model_data=smplx_model.make_synthetic_model(4321))}
    rec, _, frames, index = synthetic(n, H, W, args.verts, args.joints, args.seed)
    rec = {k: v.to(dev).contiguous() for k, v in rec.items()}
    frames, index = frames.to(dev), index.to(dev)
    rec["smplgender"] = ["neutral"] * n
    batch = SyntheticBatches(models, device=dev, frame_size=(H, W), seed=args.seed).batch(rec, frames, index, origin="frame")
    roll = CameraRoll(seed=args.seed, p=1.0, max_deg=30.0, device=dev)
    rot = roll.draw(index, 0, batch["cam0"])
    boxes = [batch["crops%d" % s].cpu().tolist() for s in (0, 1)]           # the eager path's host step, not timed
    cams = batch["cam0"].cpu().tolist()

    def call():
        return roll(batch, frames, index, epoch=0)

    def apply():
        return roll.apply(batch, frames, rot)

    def eager():
        lab, turn = eager_labels(batch, rot)
        return lab, eager_images(frames, boxes, cams, turn)

    got = call()
    status = roll.status.clone()
    want, want_im = eager()
    cover = eager_images(frames, boxes, cams, eager_labels(batch, rot)[1], coverage=True)
    torch.cuda.synchronize()
    worst = {k: float((torch.stack([got[k + "0"], got[k + "1"]]) - want[k]).abs().max()) for k in ROLLED}
    im = torch.stack([got["im0"], got["im1"]])
    alike = cover >= 1 - 1e-6
    worst_im = float(((im - want_im).abs() * alike).max())
    if not (max(worst[k] for k in ("smpl_joints_2d", "smpl_joints_2d_crop")) <= 1e-3 and worst_im <= 5e-3 and
            max(worst[k] for k in ROLLED if not k.startswith("smpl_joints_2d")) <= 1e-5):
        raise SystemExit("the kernels against the eager path: labels %r, images %.3e" % (worst, worst_im))
    labels = sum(batch[k + s].numel() * 4 for k in ROLLED for s in "01")
    canvas = sum((b[1] - b[0]) * (b[3] - b[2]) * 3 for s in (0, 1) for b in boxes[s])
    moved = 2 * labels + im.numel() * 4 + canvas
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def copy():
        return dst.copy_(src)

    ops = [count(fn) for fn in (call, apply, eager, copy)]
    med, spread = timed_interleaved([call, apply, eager, copy], args.warmup, args.reps, args.windows)
    rec = {"tool": "roll_bench", "n": n, "canvas": [H, W], "V": args.verts, "J": args.joints, "call_us": round(med[0], 1),
           "apply_us": round(med[1], 1), "eager_us": round(med[2], 1), "copy_us": round(med[3], 1), "spread_us": [round(x, 1) for x in spread],
           "eager_over_call": round(med[2] / med[0], 2), "apply_over_copy": round(med[1] / med[3], 2), "moved_mb": round(moved / 1e6, 1),
           "label_mb": round(2 * labels / 1e6, 1), "apply_gb_per_s": round(moved / med[1] / 1e3, 1), "copy_gb_per_s": round(moved / med[3] / 1e3, 1),
           "call_ops": ops[0], "apply_ops": ops[1], "eager_ops": ops[2], "copy_ops": ops[3], "max_abs_labels_against_eager": max(worst.values()),
           "max_abs_images_against_eager": worst_im, "pixels_compared": round(float(alike.float().mean()), 3),
           "centre_out": int((status & G.ROLL_CENTRE_OUT != 0).sum()), "off_canvas": int((status & G.ROLL_OFF_CANVAS != 0).sum()),
           "windows": args.windows, "reps": args.reps, "grad_lib": os.path.basename(G.LIB_PATH)}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
