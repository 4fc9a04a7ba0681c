"""Time the mesh overlay (airpose_amd.Renderer.render, apg_render_overlay) on the two workloads of the reference's summaries():

  summaries   n = 8 (4 samples x 2 views) at 1080 x 1920, focal length 1475, a closed mesh of 10 406 vertices / 20 808 faces
              (bench_mesh() below, body-sized) 6 - 10 m from the camera: copenet_twoview's visualize_tb call
  crops       n = 64 at 224 x 224, the same mesh filling the crop: the single-view trainers' call
  close       the first workload with the mesh 2 - 3 m away: its faces exceed the 16-pixel cap of the one-thread-per-face pass, so
              all of them go through the tile pass, whose cost is tiles x large faces

The yardstick is NOT an earlier run of the renderer: it is a plain device copy of the background into the output (out.copy_(images))
on the same tensors, the bytes any overlay must move.  The two take turns in one process (HIP events around --reps calls, the median
of --windows windows and their max - min).  The renderer is timed as visualize_tb uses it (rgb only) and with depth and face as well.
One JSON line per workload; --out also writes them to a file.

    python tools/render_bench.py [--reps 20] [--windows 7] [--out profiles/render_bench.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

WORKLOADS = {
    # name: n, H, W, focal length, distance range (m)
    "summaries": (8, 1080, 1920, 1475.0, (6.0, 10.0)),
    "crops": (64, 224, 224, 500.0, (3.5, 4.5)),
    "close": (8, 1080, 1920, 1475.0, (2.0, 3.0)),
}
BENCH_MESH = dict(rings=103, segments=102, radii=(0.3, 0.9, 0.25))      # body-sized: 10 406 vertices, 20 808 faces


def ellipsoid_mesh(rings, segments, radii=(1.0, 1.0, 1.0), centre=(0.0, 0.0, 0.0)):
    """A closed latitude / longitude ellipsoid with outward counter-clockwise faces: (vertices (2 + (rings - 1) segments, 3) float32,
    faces (2 segments (rings - 1), 3) int32).  The benchmark's and the tests' stand-in for a body mesh."""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segments))], -1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    at = lambda r, s: 1 + r * segments + (s % segments)
    faces = []
    for s in range(segments):
        faces.append((0, at(0, s), at(0, s + 1)))
        for r in range(rings - 2):
            faces.append((at(r, s), at(r + 1, s), at(r + 1, s + 1)))
            faces.append((at(r, s), at(r + 1, s + 1), at(r, s + 1)))
        faces.append((v.shape[0] - 1, at(rings - 2, s + 1), at(rings - 2, s)))
    v = v * np.asarray(radii, np.float64) + np.asarray(centre, np.float64)
    return v.astype(np.float32), np.asarray(faces, np.int32)


def bench_mesh():
    return ellipsoid_mesh(**BENCH_MESH)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="summaries,crops,close")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from airpose_amd.renderer import Renderer
    from loss_bench import timed_interleaved
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    v, f = bench_mesh()
    lines = []
    for name in args.workloads.split(","):
        n, H, W, focal, (near, far) = WORKLOADS[name]
        rs = np.random.RandomState(n)
        verts = torch.from_numpy(np.repeat(v[None], n, 0)).to(dev)
        R = torch.from_numpy(np.stack([rotation(rs.randn(3), rs.uniform(0, math.pi)) for _ in range(n)]).astype(np.float32)).to(dev)
        z = rs.uniform(near, far, n)
        t = torch.from_numpy(np.stack([rs.uniform(-0.2, 0.2, n) * z * W / focal, rs.uniform(-0.1, 0.1, n) * z * H / focal, z], 1)
                             .astype(np.float32)).to(dev)
        images = torch.rand(n, 3, H, W, device=dev)
        out = torch.empty_like(images)
        r = Renderer(focal_length=[focal, focal], img_res=[W, H], faces=f)

        def overlay():
            r.render(verts, t, R, images, want_depth=False, want_face=False)

        def overlay_all():
            r.render(verts, t, R, images)

        def copy():
            out.copy_(images)
        rgb, depth, face = r.render(verts, t, R, images)
        shown = float((face >= 0).float().mean())
        if not 0.002 < shown < 0.95 or not torch.equal(rgb[face[:, None].expand(-1, 3, -1, -1) < 0], images[face[:, None].expand(-1, 3, -1, -1) < 0]):
            raise SystemExit("%s: the overlay shows the mesh on %.4f of the pixels or does not keep the background" % (name, shown))
        med, spread = timed_interleaved([overlay, copy, overlay_all], args.warmup, args.reps, args.windows)
        rec = {"tool": "render_bench", "workload": name, "n": n, "H": H, "W": W, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
               "pixels_shown": round(shown, 4), "overlay_us": round(med[0], 1), "copy_us": round(med[1], 1),
               "overlay_over_copy": round(med[0] / med[1], 2), "overlay_depth_face_us": round(med[2], 1),
               "spread_us": [round(x, 1) for x in spread], "copy_bytes": 2 * images.numel() * 4, "windows": args.windows, "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
