"""Time airpose_amd.AirPosePlusSequence on a sequence of the reference's length: L = 6990 frames in windows of 2000, seeded synthetic
inputs in the style of fitting.synthetic_fit_problem (a random-initialised VPoser encoder and decoder, detections scattered around a
fixed layout; the loop runs a fixed number of iterations whatever the data, so these are LATENCY figures).

  prepare        AirPosePlusSequence.prepare: one apg_seq_init launch and the one host copy of `robust`
  prepare_eager  the same maths in eager torch on the GPU (folded encoder as two matmuls, pytorch3d's axis_angle_to_matrix, the
                 agreement filter, the mask and its host copy)
  export         AirPosePlusSequence.export(want_vertices=False): one apg_seq_export launch, parameters for all L frames
  export_eager   the same in eager torch (decoder, Gram-Schmidt, tgm's matrot2aa with torch.where, rotation_6d_to_matrix, the 4 x 4s,
                 torch.linalg.inv for cam1_wrt_cam0)
  export_meshes  export(frames=slice(0, --mesh-frames)): parameters for all frames and the meshes of 256 (SMPLX.forward and
                 transform_smpl: existing kernels; no eager yardstick)
  fit            AirPosePlusSequence.fit, --iters iterations per window, timed whole with a host clock around a device synchronise
                 (one call is tenths of a second); per window, per iteration and per frame-iteration derived from it; fit_64 is ONE
                 window of 64 frames with the same iterations, the only size ap_fit_run had been run at before
  *_ops          an OPERATOR count per call as in tools/loss_bench.py: every aten operator outside LaunchCount.VIEWS counts one,
                 every apg_seq_* call counts one (its one launch)

prepare / export and their yardsticks take turns in one process (HIP events around --reps calls, the median of --windows windows
and their max - min).  The fit is run --fit-runs times; its results must be finite and two runs bit-equal, which the record states
(finite, deterministic) beside the first and last 2-D loss of every window.  One JSON line; --out also writes it to a file.

    python tools/seq_fit_bench.py [--frames 6990] [--chunk 2000] [--iters 300] [--out profiles/seq_fit_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from airpose_amd import _native_grad as G  # noqa: E402
from airpose_amd import smplx, smplx_model  # noqa: E402
from airpose_amd.fitting import synthetic_fit_problem  # noqa: E402
from airpose_amd.loss_real import ENCODER_KEYS  # noqa: E402
from airpose_amd.sequence import AirPosePlusSequence  # noqa: E402
from loss_bench import LaunchCount, timed_interleaved  # noqa: E402


def synthetic_vposer(decoder, seed):
    """one state dict: a seeded encoder (nn.Linear init, BatchNorm statistics away from (0, 1)) and the given decoder"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in ENCODER_KEYS.items():
        if k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith("running_mean") or (len(shape) == 1 and k.endswith("bias")):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            sd[k] = 1.0 + 0.2 * torch.randn(shape, generator=g)
        else:
            sd[k] = (torch.rand(shape, generator=g) * 2 - 1) / shape[1] ** 0.5
    for i, n in zip((0, 3, 5), (1, 2, 3)):
        sd["decoder_net.%d.weight" % i], sd["decoder_net.%d.bias" % i] = decoder["w%d" % n], decoder["b%d" % n]
    return sd


# ------------------------------------------------------------------------------------------------ the eager yardsticks
def aa_to_matrix(a):
    t = a.norm(dim=-1, keepdim=True)
    small = t < 1e-6
    k = torch.where(small, 0.5 - t * t / 48, torch.sin(0.5 * t) / torch.where(small, torch.ones_like(t), t))
    q = torch.cat([torch.cos(0.5 * t), a * k], -1)
    r, i, j, k = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    return torch.stack((1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r), s * (i * j + k * r), 1 - s * (i * i + k * k),
                        s * (j * k - i * r), s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)), -1).reshape(-1, 3, 3)


def eager_prepare(enc, pred, det, px, conf):
    W1, b1, Wmu, bmu = enc
    L = det.shape[1]
    z = F.leaky_relu(pred["pred_angles0"][:, 1:22].reshape(L, 63) @ W1.t() + b1, 0.01) @ Wmu.t() + bmu
    phi = torch.stack([aa_to_matrix(pred["pred_angles%d" % v][:, 0])[:, :2].reshape(L, 6) for v in (0, 1)])
    tau = torch.stack([pred["pred_smpltrans0"], pred["pred_smpltrans1"]])
    d = det[:, :, 0, :, :2] - det[:, :, 1, :, :2]
    keep = ~(torch.sqrt((d * d).sum(-1)) > px)
    j2d = det.clone()
    j2d[..., 2] = det[..., 2] * keep.unsqueeze(2)
    robust = (j2d[:, :, 1, :, 2].sum((0, 2)) > conf).to(torch.int32).cpu()
    return z, phi, tau, j2d, robust


def matrot2aa(R):
    """tgm 0.1.2 rotation_matrix_to_angle_axis on (n, 3, 3), its four branches through torch.where"""
    t = R.transpose(1, 2)
    t00, t11, t22 = t[:, 0, 0], t[:, 1, 1], t[:, 2, 2]
    q0 = torch.stack([t[:, 1, 2] - t[:, 2, 1], 1 + t00 - t11 - t22, t[:, 0, 1] + t[:, 1, 0], t[:, 2, 0] + t[:, 0, 2]], -1)
    q1 = torch.stack([t[:, 2, 0] - t[:, 0, 2], t[:, 0, 1] + t[:, 1, 0], 1 - t00 + t11 - t22, t[:, 1, 2] + t[:, 2, 1]], -1)
    q2 = torch.stack([t[:, 0, 1] - t[:, 1, 0], t[:, 2, 0] + t[:, 0, 2], t[:, 1, 2] + t[:, 2, 1], 1 - t00 - t11 + t22], -1)
    q3 = torch.stack([1 + t00 + t11 + t22, t[:, 1, 2] - t[:, 2, 1], t[:, 2, 0] - t[:, 0, 2], t[:, 0, 1] - t[:, 1, 0]], -1)
    low, c01, c23 = (t22 < 1e-6).unsqueeze(1), (t00 > t11).unsqueeze(1), (t00 < -t11).unsqueeze(1)
    q = torch.where(low, torch.where(c01, q0, q1), torch.where(c23, q2, q3))
    tt = torch.where(low, torch.where(c01, q0[:, 1:2], q1[:, 2:3]), torch.where(c23, q2[:, 3:4], q3[:, 0:1]))
    q = q * (0.5 / torch.sqrt(tt))
    ss = (q[:, 1:] * q[:, 1:]).sum(1)
    sn = torch.sqrt(ss)
    two = 2.0 * torch.where(q[:, 0] < 0, torch.atan2(-sn, -q[:, 0]), torch.atan2(sn, q[:, 0]))
    k = torch.where(ss > 0, two / torch.where(ss > 0, sn, torch.ones_like(sn)), torch.full_like(sn, 2.0))
    return q[:, 1:] * k.unsqueeze(1)


def sixd_rows(d6):
    b1 = F.normalize(d6[..., :3], dim=-1)
    b2 = F.normalize(d6[..., 3:] - (b1 * d6[..., 3:]).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def eager_export(dec, res):
    w1, b1, w2, b2, w3, b3 = dec
    L = res["z"].shape[0]
    h = F.leaky_relu(F.linear(res["z"], w1, b1), 0.01)
    o = F.linear(F.leaky_relu(F.linear(h, w2, b2), 0.01), w3, b3).view(-1, 3, 2)
    c1 = F.normalize(o[:, :, 0], dim=1)
    c2 = F.normalize(o[:, :, 1] - (c1 * o[:, :, 1]).sum(1, keepdim=True) * c1, dim=-1)
    thetas = matrot2aa(torch.stack([c1, c2, torch.cross(c1, c2, dim=1)], dim=-1)).view(L, 63)
    Rv = torch.stack([sixd_rows(res["phi%d" % v]) for v in (0, 1)])
    T = torch.zeros(2, L, 4, 4, device=Rv.device)
    T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = Rv, torch.stack([res["tau0"], res["tau1"]]), 1.0
    return thetas, Rv, T, T[0] @ torch.linalg.inv(T[1])


def count_ops(fn):
    """aten operators outside VIEWS + 1 per apg_seq_* call, over one call of fn"""
    calls = {"n": 0}
    lib = G.lib()

    class Spy(object):
        def __getattr__(self, name):
            f = getattr(lib, name)
            if not name.startswith("apg_seq_"):
                return f

            def counted(*a):
                calls["n"] += 1
                return f(*a)
            return counted
    real = G.lib
    G.lib = lambda: Spy()
    try:
        with LaunchCount() as m:
            fn()
    finally:
        G.lib = real
    torch.cuda.synchronize()
    return m.n + calls["n"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6990)
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--mesh-frames", type=int, default=256)
    ap.add_argument("--fit-runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq_fit_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    L = args.frames
    decoder, state, data = synthetic_fit_problem(L, args.seed, dev)
    body = smplx.SMPLX(model_data=smplx_model.make_synthetic_model(4321))
    seq = AirPosePlusSequence(synthetic_vposer(decoder, args.seed + 1), body, device=dev, chunk=args.chunk)
    g = torch.Generator().manual_seed(args.seed + 2)
    pred = {}
    for v in (0, 1):
        a = 0.3 * torch.randn(L, 22, 3, generator=g)
        a[:, 0] = torch.tensor([3.0, 0.0, 0.0]) + 0.1 * torch.randn(L, 3, generator=g)     # near the upright pose seen by a camera
        pred["pred_angles%d" % v], pred["pred_smpltrans%d" % v] = a.to(dev), state["tau%d" % v].contiguous()
    det = data["j2d"]
    enc, dec = seq._weights()

    st, dd = seq.prepare(pred, det)
    ez, ephi, etau, ej2d, erob = eager_prepare(enc, pred, det, 100.0, 14.0)
    diff = {"z": float((st["z"] - ez).abs().max()), "phi": float((st["phi0"] - ephi[0]).abs().max()),
            "conf": float((dd["j2d"] - ej2d).abs().max()), "robust": int((dd["robust"] != erob).sum())}
    if diff["z"] > 1e-4 or diff["phi"] > 1e-5 or diff["conf"] != 0:
        raise SystemExit("prepare against its eager form: %r" % diff)

    # ---- the fit: whole sequence, then one window of 64
    def fit_once(s, d, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = seq.fit(s, d, data["intr"], data["extr"], n_iters=n, want_loss=True)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    fit_once(st, dd, 2)                                          # warm-up: code objects, the handle's buffers
    runs = [fit_once(st, dd, args.iters) for _ in range(args.fit_runs)]
    res = runs[0][0]
    keys = ("z", "phi0", "phi1", "tau0", "tau1", "beta")
    finite = all(bool(torch.isfinite(res[k]).all()) for k in keys) and all(bool(torch.isfinite(h).all()) for h in res["loss"])
    same = all(torch.equal(res[k].view(torch.int32), r[k].view(torch.int32)) for r, _ in runs[1:] for k in keys)
    fit_s = statistics.median(t for _, t in runs)
    s64 = {k: v[:64] for k, v in st.items()}
    d64 = {"j2d": dd["j2d"][:, :64], "robust": dd["robust"][:64]}
    fit_once(s64, d64, 2)
    fit64_s = statistics.median(fit_once(s64, d64, args.iters)[1] for _ in range(args.fit_runs))
    n_win = len(res["chunks"])

    # ---- prepare / export and their yardsticks
    def prepare():
        return seq.prepare(pred, det)

    def prepare_eager():
        with torch.no_grad():
            return eager_prepare(enc, pred, det, 100.0, 14.0)

    def export():
        return seq.export(res, want_vertices=False)

    def export_eager():
        with torch.no_grad():
            return eager_export(dec, res)

    def export_meshes():
        return seq.export(res, frames=slice(0, args.mesh_frames))
    out = export()
    eth, eR, eT, eC = export_eager()
    ediff = {"thetas": float((out["thetas"] - eth).abs().max()), "root_rot": float((out["root_rot0"] - eR[0]).abs().max()),
             "cam1_wrt_cam0": float((out["cam1_wrt_cam0"] - eC).abs().max())}
    fns = [prepare, prepare_eager, export, export_eager, export_meshes]
    ops = [count_ops(fn) for fn in fns]
    med, spread = timed_interleaved(fns, args.warmup, args.reps, args.windows)
    rec = {"tool": "seq_fit_bench", "L": L, "chunk": args.chunk, "n_windows": n_win, "iters": args.iters, "mesh_frames": args.mesh_frames,
           "prepare_us": round(med[0], 1), "prepare_eager_us": round(med[1], 1), "export_us": round(med[2], 1),
           "export_eager_us": round(med[3], 1), "export_meshes_us": round(med[4], 1),
           "prepare_speedup": round(med[1] / med[0], 2), "export_speedup": round(med[3] / med[2], 2),
           "prepare_ops": ops[0], "prepare_eager_ops": ops[1], "export_ops": ops[2], "export_eager_ops": ops[3], "export_meshes_ops": ops[4],
           "spread_us": [round(x, 1) for x in spread],
           "fit_s": round(fit_s, 4), "fit_runs_s": [round(t, 4) for _, t in runs], "fit_us_per_iteration": round(fit_s * 1e6 / (n_win * args.iters), 1),
           "fit_ns_per_frame_iteration": round(fit_s * 1e9 / (L * args.iters), 1),
           "fit_64_s": round(fit64_s, 4), "fit_64_us_per_iteration": round(fit64_s * 1e6 / args.iters, 1),
           "fit_finite": finite, "fit_deterministic": same, "robust_frames": int(dd["robust"].sum()),
           "loss2d_first_last": [[round(float(h[0, 0]), 5), round(float(h[-1, 0]), 5)] for h in res["loss"]],
           "prepare_vs_eager_max_abs": diff, "export_vs_eager_max_abs": ediff, "windows": args.windows, "reps": args.reps,
           "grad_lib": os.path.basename(G.LIB_PATH)}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
