#!/usr/bin/env python
"""Headline benchmark: two-view frames (pairs) per second of the AirPose inference hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W     (N > 1 without WORLD_SIZE in the environment: re-launches itself through
                                                     torch.distributed.run, one rank per GPU; the driver's own torchrun command
                                                     works unchanged)

One step = one pass of the whole hot path over one batch of synthetic input resident in HBM:
copenet_twoview forward (ResNet-50 trunk on both views, 3 IEF iterations with cross-view fusion)
-> in-place translation un-scale -> rot6d -> SMPL-X LBS (10475 verts) -> root transform -> 2-D
projection, at 256 pairs per GPU (BASELINE.json metric: "two-view frames/sec at batch 256"), in the 16-bit throughput mode named
by --precision (default f16: fp16 storage; `dtype` of the line).  Pairs are independent units: every rank owns its own 256 pairs,
no data-path collective (weak scaling).

A plain run sets up, warms up (W steps), times the K steps and prints ONE JSON line on rank 0: metric, value (pairs/s over the K
timed steps, all GPUs), unit, higher_is_better, dtype, ms_per_step (wall time of one timed step) and the configuration.  The timed
steps carry no instrumentation.

  --dump-outputs DIR   after the timed steps, what the last of them returned (the output dict of the timed path) as
                       DIR/<name>.npy in float32; an output above 4 MiB keeps a fixed, seeded sample of its rows.  Weights and
                       inputs are seeded: the same arguments give the same inputs in every run, so two builds compare output for output.
  --full               everything below as well, after the headline's steps (the timed steps then carry the conv-stack HIP events
                       the roofline needs).  The options of the "secondary measurements" group act only here.

With --full the line holds these extra objects:
  roofline      SURVEY 8(d): pairs/s x 16.3916 GFLOP per pair against the dense bf16 / fp16 MFMA peak (whole step time); the conv
                stack alone (its launch count read back from the library, HIP events on the streams that run it) beside it;
                `traffic` = HBM bytes per STEP from the latest committed PMC pass
  cpu_baseline  the CPU oracle (a torch restatement pinned to the reference) timed on this box's host
                cores on a bounded sample -- a reported baseline, not the target
  repeat_blocks the K-step block repeated (same fences) after the contract's block: median / min / max pairs/s
  parity_mode   throughput of the modes that meet the 1e-4 bar + the measured per-slice error of every mode against
                the CPU oracle on the first pairs of the batch
  parity_sweep  every mode x 5 checkpoints (3 weight seeds, a wide BatchNorm range, SURVEY 8(d)'s exact recipe) against the CPU
                oracle, next to what the GPU parity probe (ap_net_parity_probe) says about the same checkpoint and what
                precision="auto" picks for it
  view_split    (N >= 2 ranks) BASELINE config 4: one view per rank, the 136-float partner state exchanged over
                RCCL pair groups before IEF iterations 2 and 3, hidden behind the partner-independent half of the step
  and stage_ms_per_step, smplx_tail_roofline, smplx_blend_roofline, parity_of_timed_mode, f16_range_check, b64, airpose_plus and
  stream_ordered (or overlap_tail): see the code that fills them.
Every `frac` recomputes from `stage_ms_per_step` and the byte / FLOP constants stated next to it.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
MEAN = os.path.join(REPO, "airpose_amd", "data", "smpl_mean_params.npz")

PEAK_BF16_DENSE_TFLOPS = 2500.0      # MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA
PEAK_FP32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0
DUMP_ARRAY_BYTES = 4 << 20           # --dump-outputs: larger outputs keep a seeded sample of their rows (<= 14 outputs: < 64 MB in all)


def conv_stack_flops_per_image():
    """2*MAC of the 52 implicit-GEMM convolutions (everything in the trunk but the 7x7 stem)."""
    layers, planes = (3, 4, 6, 3), (64, 128, 256, 512)
    macs, inpl, H = 0, 64, 56
    for li, (pl, nb) in enumerate(zip(planes, layers)):
        for bi in range(nb):
            stride = 2 if (bi == 0 and li > 0) else 1
            Ho = H // stride
            macs += H * H * inpl * pl                      # conv1 1x1
            macs += Ho * Ho * pl * pl * 9                  # conv2 3x3 (stride here)
            macs += Ho * Ho * pl * pl * 4                  # conv3 1x1
            if bi == 0:
                macs += Ho * Ho * inpl * pl * 4            # downsample 1x1
            inpl, H = pl * 4, Ho
    return 2 * macs


TAIL_BYTES_PER_BODY = 129084         # beta 40 + 22 rotmats 792 + t 12 + vertices 125700 + joints 1524 + j2d 1016
TAIL_CONST_BYTES = 25.5e6            # v_template + shapedirs[:, :, :10] + posedirs[:189] + sparse regressors, once per launch
BLEND_K_ALGORITHMIC = 10 + 21 * 9    # = 199
STEM_FLOPS_PER_IMAGE = 2 * 112 * 112 * 64 * 147
REG_FLOPS_PER_PAIR = 2 * 3 * 2 * (2332 * 1024 + 1024 * 1024 + 1024 * 145)


def pmc_traffic():
    """HBM bytes per STEP of 256 pairs from the latest committed rocprofv3 PMC passes (FETCH_SIZE x2-corrected + WRITE_SIZE,
    profiles/r*_pmc_hbm_traffic.csv via tools/collect_profiles.sh): counters cannot be collected inside the timed run."""
    try:
        import glob
        with open(sorted(glob.glob(os.path.join(REPO, "profiles", "r*_pmc_traffic.json")))[-1]) as f:
            d = json.load(f)
        return d["fetch_bytes_per_step_x2"] + d["write_bytes_per_step"]
    except Exception:
        return None


def cpu_baseline(sd, md, sample_pairs):
    """Time the oracle (pure torch CPU restatement of the reference path) on a bounded sample.  torch's intra-op pool
    at one thread per core is NOT the fastest setting on a many-core host for operators this small (128 threads were
    8x slower than 8 on the MI355X box), so a short sweep over thread counts is timed and the best one is the baseline;
    `cores` is the thread count of that best run and the whole sweep is reported."""
    import torch
    from airpose_amd import weights as W
    from oracle import pipeline_ref
    inp = {k: torch.from_numpy(v) for k, v in W.synthetic_inputs(4321, sample_pairs).items()}
    n_all = torch.get_num_threads()
    sweep = {}
    want = None
    try:
        for n in sorted({t for t in (8, 16, 32, 64, n_all) if t <= n_all}):
            torch.set_num_threads(n)
            best = None
            with torch.no_grad():
                for i in range(3):                         # 1 warm-up + best of 2
                    t0 = time.perf_counter()
                    want = pipeline_ref.infer(sd, md, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], inp["intr0"], inp["intr1"])
                    dt = time.perf_counter() - t0
                    if i and (best is None or dt < best):
                        best = dt
            sweep[n] = sample_pairs / best
    finally:
        torch.set_num_threads(n_all)
    n_best = max(sweep, key=sweep.get)
    res = {"value": sweep[n_best], "unit": "pairs/s", "cores": n_best, "kind": "port",
           "sample": "%d pairs (224x224, 3 IEF iterations, SMPL-X tail), fp32 torch CPU oracle, best of 2 after 1 warm-up, "
                     "best of the thread-count sweep" % sample_pairs,
           "host_cores": n_all, "threads_sweep_pairs_per_s": {str(k): v for k, v in sorted(sweep.items())}}
    return res, inp, want                                  # the sample and the oracle's outputs on it: parity_block's checker


def slice_errs(got, want, elementwise_atol=None):
    """max |a-b| / max |b| per semantic slice of the output dict (a pose vector = translation | 6-D rotations); with
    elementwise_atol: max |a-b| / (atol + |b|) instead (tests/conftest.py: elem_err -- the like-for-like form of a relative bar)."""
    import numpy as np
    out = {}
    for k in ("pred_pose0", "pred_pose1", "pred_betas0", "pred_betas1", "pred_j3d_cam0", "pred_j3d_cam1",
              "pred_j2d_cam0", "pred_j2d_cam1", "pred_vertices_cam0", "pred_vertices_cam1"):
        a, b = got[k].double().numpy(), want[k].double().numpy()
        parts = {"theta.trans": (a[:, :3], b[:, :3]), "theta.rot6d": (a[:, 3:], b[:, 3:])} if "pose" in k else \
                {k[5:-1].replace("_cam", ""): (a, b)}
        for nm, (x, y) in parts.items():
            if elementwise_atol is None:
                e = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30))
            else:
                e = float((np.abs(x - y) / (elementwise_atol + np.abs(y))).max())
            out[nm] = max(out.get(nm, 0.0), e)
    return out


def timed_mode_parity(sd, md, pipe, dev, n_threads, seeds=(4321, 777), pairs_per_seed=64, submit=False):
    """The TIMED mode against the fp32 CPU oracle on len(seeds) x pairs_per_seed pairs of fresh synthetic inputs (the
    headline's parity on >= 128 pairs and two input seeds).  The oracle runs at the thread count the cpu_baseline sweep found
    fastest; it is the checker here, outside every timed region."""
    import torch
    from airpose_amd import weights as W
    from oracle import pipeline_ref
    n_all = torch.get_num_threads()
    worst, worst_el, per_seed = {}, {}, {}
    t0 = time.perf_counter()
    try:
        torch.set_num_threads(n_threads)
        for seed in seeds:
            inp = {k: torch.from_numpy(v) for k, v in W.synthetic_inputs(seed, pairs_per_seed).items()}
            with torch.no_grad():
                want = pipeline_ref.infer(sd, md, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], inp["intr0"], inp["intr1"])
            dbatch = {k: v.to(dev) for k, v in inp.items()}
            # the form the timed region issued its steps in
            gout = pipe.submit(dbatch, want_rotmat=True).synchronize() if submit else pipe(dbatch, want_rotmat=True)
            got = {k: v.float().cpu() for k, v in gout.items()}
            e, el = slice_errs(got, want), slice_errs(got, want, elementwise_atol=1e-2)
            per_seed[str(seed)] = max(e.values())
            for k in e:
                worst[k] = max(worst.get(k, 0.0), e[k])
                worst_el[k] = max(worst_el.get(k, 0.0), el[k])
    finally:
        torch.set_num_threads(n_all)
    return {"checked_pairs": len(seeds) * pairs_per_seed, "input_seeds": list(seeds), "max_rel_err": max(worst.values()),
            "rel_err_by_slice": worst, "max_rel_err_by_seed": per_seed,
            "elementwise_err_by_slice": worst_el, "elementwise_measure": "max |a-b| / (1e-2 + |b|) over the slice's entries",
            "error_measure": "max|a-b| / max|b| per semantic slice (translation, 6-D rotations, betas, 3-D joints, vertices, 2-D projection)",
            "checker": "fp32 CPU oracle (oracle/pipeline_ref.py) on fresh synthetic inputs, %d threads" % n_threads,
            "issued_through": "TwoViewInference.submit" if submit else "TwoViewInference.__call__",
            "oracle_seconds": time.perf_counter() - t0}


def parity_sweep(args, md, body, dev, n_threads, pairs_per_cell=16):
    """The parity claim as a property of the CHECKPOINT.  EVERY mode against the fp32 CPU oracle over
    5 checkpoints x 2 input seeds: three weight seeds of the benchmark's family, a second BatchNorm-statistics range (gamma,
    running_var ~ U(.25, 2)) and SURVEY 8(d)'s recipe to the letter (gamma ~ U(.5, 1.5) on EVERY BatchNorm; the benchmark family
    halves it on the last BatchNorm of a block).  Per (mode, checkpoint): worst slice-max and element-wise error against the oracle
    AND what the GPU parity probe (ap_net_parity_probe: the mode's trunk against the exact-fp32 trunk of the same weights, no CPU
    involved) measured, so the probe's verdict can be held against the oracle's; per checkpoint: what precision="auto" picks."""
    import torch
    from airpose_amd import _native as Nn
    from airpose_amd import copenet_model, pipeline
    from airpose_amd import weights as W
    from oracle import pipeline_ref
    ckpts = [("seed20240901", 20240901, "default"), ("seed7", 7, "default"), ("seed99", 99, "default"),
             ("seed20240901_widebn", 20240901, "wide"), ("seed20240901_survey8d", 20240901, "survey")]
    in_seeds = (4321, 777)
    modes = ("f16", "bf16", "bf16x2", "fp32")
    n_all = torch.get_num_threads()
    res = {m: {"max_rel_err": 0.0, "max_elementwise_err": 0.0, "by_checkpoint": {}, "worst_slice": None} for m in modes}
    auto = {}
    t0 = time.perf_counter()
    nets = {}
    try:
        for name, wseed, bn in ckpts:
            sdw = W.to_torch(W.copenet_state_dict(wseed, MEAN, bn=bn))
            cells = []
            torch.set_num_threads(n_threads)
            for s in in_seeds:
                inp = {k: torch.from_numpy(v) for k, v in W.synthetic_inputs(s, pairs_per_cell).items()}
                with torch.no_grad():
                    want = pipeline_ref.infer(sdw, md, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], inp["intr0"], inp["intr1"])
                cells.append((inp, want))
            torch.set_num_threads(n_all)
            for m in modes:
                if m not in nets:
                    nets[m] = copenet_model.getcopenet(MEAN, precision=m).eval()
                net = nets[m]
                net.load_state_dict(sdw)
                pipe = pipeline.TwoViewInference(net, body, iters=3)
                worst, worst_el, wslice, err_txt, probe = 0.0, 0.0, None, None, None
                try:
                    pr = net.parity_probe(8)
                    probe = {"max_rel_err": pr["max_rel_err"], "worst_slice": max(pr["rel_err_by_slice"], key=pr["rel_err_by_slice"].get),
                             "ms": pr["ms"], "holds": pr["max_rel_err"] < 1e-4}
                    for inp, want in cells:
                        got = {k: v.float().cpu() for k, v in pipe({k: v.to(dev) for k, v in inp.items()}, want_rotmat=True).items()}
                        e, el = slice_errs(got, want), slice_errs(got, want, elementwise_atol=1e-2)
                        ks = max(e, key=e.get)
                        if e[ks] > worst:
                            worst, wslice = e[ks], ks
                        worst_el = max(worst_el, max(el.values()))
                    if m == "f16":
                        net.range_status()
                except Nn.RangeError as ex:                   # fp16 storage cannot hold this checkpoint: reported, and the flag cleared
                    err_txt = "fp16 range: " + str(ex)[:120]
                    worst = worst_el = float("inf")
                    try:
                        net.range_status(reset=True)
                    except Nn.RangeError:
                        pass
                except RuntimeError as ex:
                    if "fp16 range" not in str(ex):
                        raise
                    err_txt = "fp16 range (weights): " + str(ex)[:120]
                    worst = worst_el = float("inf")
                cell = {"max_rel_err": None if err_txt else worst, "max_elementwise_err": None if err_txt else worst_el,
                        "meets_bar": (not err_txt) and worst < 1e-4, "probe": probe}
                if err_txt:
                    cell["error"] = err_txt
                    if probe is None:
                        cell["probe"] = {"holds": False, "error": "fp16 range"}
                res[m]["by_checkpoint"][name] = cell
                if worst > res[m]["max_rel_err"]:
                    res[m]["max_rel_err"], res[m]["worst_slice"] = worst, "%s @ %s" % (wslice or "range", name)
                res[m]["max_elementwise_err"] = max(res[m]["max_elementwise_err"], worst_el)
                del pipe
            # what the run-time guard does with this checkpoint
            na = copenet_model.getcopenet(MEAN, precision="auto").eval()
            na.load_state_dict(sdw)
            na.forward_feat_ext(torch.zeros(1, 3, 224, 224, device=dev))
            chosen = na.auto_report["chosen"]
            auto[name] = {"chosen": chosen, "chosen_meets_bar_vs_oracle": res[chosen]["by_checkpoint"][name]["meets_bar"],
                          "fastest_mode_that_meets_bar_vs_oracle": next((m for m in na.AUTO_ORDER if res[m]["by_checkpoint"][name]["meets_bar"]), None)}
            del na
    finally:
        torch.set_num_threads(n_all)
    del nets
    torch.cuda.empty_cache()
    agree = tot = 0
    for m in modes:
        r = res[m]
        r["meets_bar"] = r["max_rel_err"] < 1e-4
        for c in r["by_checkpoint"].values():
            if c.get("probe"):
                tot += 1
                agree += int(bool(c["probe"]["holds"]) == bool(c["meets_bar"]))
        if r["max_rel_err"] == float("inf"):
            r["max_rel_err"] = r["max_elementwise_err"] = None
    return {"modes": res, "auto": auto, "probe_agrees_with_oracle": "%d of %d (mode, checkpoint) cells" % (agree, tot),
            "bar": 1e-4, "checkpoints": [c[0] for c in ckpts], "input_seeds": list(in_seeds),
            "pairs_per_checkpoint": len(in_seeds) * pairs_per_cell, "checked_pairs_per_mode": len(ckpts) * len(in_seeds) * pairs_per_cell,
            "error_measure": "max|a-b| / max|b| per semantic slice; elementwise: max |a-b| / (1e-2 + |b|)",
            "checkpoints_note": "copenet_state_dict(seed, bn=...) of airpose_amd/weights.py; widebn: BatchNorm gamma / running_var ~ U(.25, 2) "
                                "(last BN of a block: gamma ~ U(.125, 1)); survey8d: gamma ~ U(.5, 1.5) on every BatchNorm, the last one of a "
                                "block included (SURVEY 8(d) to the letter: trunk features of order 5e3, stored activations near the fp16 range)",
            "seconds": time.perf_counter() - t0}


def airpose_plus_block(body_md, dev, frames=64, iters=300):
    """BASELINE config 4 (AirPose+: copenet_twoview + SMPLify-X-style fitting loop, batch 64, end-to-end latency): the fitting loop
    of bundle_adj.py:262-401 (300 Adam steps over a sequence of 64 frames, 2 views x 2 detectors x 24 joints) through ap_fit_run
    on a seeded synthetic problem; the network forward of the same 64 pairs is the b64 block of this line."""
    import torch
    from airpose_amd import smplx as smplx_mod
    from airpose_amd.fitting import AirPosePlusFitter, synthetic_fit_problem
    body = smplx_mod.SMPLX(model_data=body_md, batch_size=frames, create_transl=False).to(dev)
    vp, st, dd = synthetic_fit_problem(frames, 77, dev)
    fitter = AirPosePlusFitter(vp, body, dev)
    run = lambda n: fitter.run(st, dd["j2d"], dd["robust"], dd["intr"], dd["extr"], n_iters=n, want_loss=True)
    run(5)
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        _, hist = run(iters)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None or ms < best else best
    return {"frames": frames, "iters": iters, "ms": best, "ms_per_iteration": best / iters, "unit": "ms", "higher_is_better": False,
            "what": "ap_fit_run: %d Adam steps (VPoser latent, per-view root 6D + translation, shared betas), inputs resident on the "
                    "device, best of 3; loss %.4g -> %.4g" % (iters, float(hist[0, :3].sum()), float(hist[-1, :3].sum())),
            "reference": "copenet_real_data/scripts/bundle_adj.py:262-401"}


def b64_block(args, sd, body, dev):
    """BASELINE config 1 (copenet_twoview forward, batch 64 two-view, 3 IEF iterations, network only) in both 16-bit storage
    types: pairs/s and the conv-stack fraction of the MFMA peak from HIP events inside its own timed steps."""
    import torch
    from airpose_amd import copenet_model, pipeline
    from airpose_amd import weights as W
    B, steps = 64, 20
    batch = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(99, B).items()}
    res = {"workload": "copenet_twoview forward (ResNet-50 x2 views, 3 IEF iterations), 64 pairs, network only", "steps": steps}
    for prec in ("bf16", "f16"):
        net = copenet_model.getcopenet(MEAN, precision=prec).eval()
        net.load_state_dict(sd)
        pipe = pipeline.TwoViewInference(net, body, iters=3)
        for _ in range(3):
            pipe.forward_net(batch["im0"], batch["im1"], batch["bb0"], batch["bb1"])
        torch.cuda.synchronize()
        net.enable_timing(2)
        net.timing(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.forward_net(batch["im0"], batch["im1"], batch["bb0"], batch["bb1"])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tm = net.timing(reset=True)
        net.enable_timing(0)
        n_launch = net.last_conv_launches()
        # the same steps issued as a serving loop (TwoViewInference.submit_net: passes of step i+1 behind those of step i, IEF loop
        # on a second stream)
        for _ in range(3):
            pend = pipe.submit_net(batch["im0"], batch["im1"], batch["bb0"], batch["bb1"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pend = pipe.submit_net(batch["im0"], batch["im1"], batch["bb0"], batch["bb1"])
        torch.cuda.synchronize()
        dts = time.perf_counter() - t0
        del pend
        conv_ms = tm["conv_ms"] / max(tm["passes"], 1)
        tf = conv_stack_flops_per_image() * 2 * B / (conv_ms * 1e-3) / 1e12
        res[prec] = {"pairs_per_s": B * steps / dt, "ms_per_step": 1e3 * dt / steps,
                     "submit_pairs_per_s": B * steps / dts, "submit_ms_per_step": 1e3 * dts / steps, "conv_stack_ms": conv_ms,
                     "conv_stack_tflops": tf, "conv_stack_frac": tf / PEAK_BF16_DENSE_TFLOPS, "conv_launches_per_step": n_launch}
        del pipe, net
        torch.cuda.empty_cache()
    return res


def parity_block(args, sd, body, batch, net_bf, sample, want, dev):
    """The modes that meet north_star's 1e-4 bar, timed on the same batch after the bf16 loop -- bf16x2 (split-bf16
    pairs on the bf16 matrix pipe: the fast parity mode) and fp32 (exact fp32 MFMA chain) -- and the measured per-slice
    error of all three modes on the CPU-baseline sample (the oracle outputs the cpu_baseline leg produced anyway are
    the checker; the oracle is not run again here)."""
    import torch
    from airpose_amd import copenet_model, pipeline
    if args.parity_steps <= 0 or args.precision not in ("bf16", "f16"):
        return None
    gin = {k: v.to(dev) for k, v in sample.items()} if want is not None else None
    modes = {}
    other16 = "bf16" if args.precision == "f16" else "f16"    # the throughput kernels with the other 16-bit storage type
    for prec, steps in (("bf16x2", 2 * args.parity_steps), ("fp32", args.parity_steps), (other16, 4 * args.parity_steps)):
        net = copenet_model.getcopenet(MEAN, precision=prec).eval()
        net.load_state_dict(sd)
        if args.chunk:
            net.set_chunk(args.chunk)
        pipe = pipeline.TwoViewInference(net, body, iters=3)
        out = pipe(batch, want_rotmat=True)                    # warm-up (packs the weights)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = pipe(batch, want_rotmat=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del out
        m = {"pairs_per_s": args.batch * steps / dt, "ms_per_step": 1e3 * dt / steps, "steps": steps}
        if gin is not None:
            e = slice_errs({k: v.float().cpu() for k, v in pipe(gin, want_rotmat=True).items()}, want)
            m.update({"max_rel_err": max(e.values()), "rel_err_by_slice": e})
        modes[prec] = m
        del pipe, net
        torch.cuda.empty_cache()
    res = dict(modes["bf16x2"])
    res.update({"dtype": "bf16x2", "bar": 1e-4,
                "arithmetic": "split-bf16 storage (hi + lo bf16 per value, planar groups of 8 channels, fp32 bytes); each product as "
                              "hi*hi + hi*lo + lo*hi in three v_mfma_f32_16x16x32_bf16 per 8 K elements, fp32 accumulate",
                "fp32_mode": dict(modes["fp32"], arithmetic="fp32 storage, v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain)"),
                other16 + "_mode": dict(modes[other16], arithmetic="the timed mode's kernels with %s storage and "
                                        "v_mfma_f32_16x16x32_%s" % (("bf16", "bf16") if other16 == "bf16" else ("fp16", "f16")))})
    if gin is not None:
        ebf = slice_errs({k: v.float().cpu() for k, v in
                          pipeline.TwoViewInference(net_bf, body, iters=3)(gin, want_rotmat=True).items()}, want)
        res.update({"throughput_mode_rel_err_by_slice": ebf, "throughput_mode_max_rel_err": max(ebf.values()),
                    "checked_pairs": int(sample["im0"].shape[0]),
                    "error_measure": "max|a-b| / max|b| per semantic slice (translation, 6-D rotations, betas, 3-D "
                                     "joints, vertices, 2-D projection) vs the fp32 CPU oracle on the cpu_baseline sample"})
    return res


def view_split_block(args, net, batch, dev, rank, world):
    """BASELINE config 4 on RCCL: ranks (2k, 2k+1) hold view 0 / view 1 of the same B pairs.  One step = the trunk on
    this rank's view + the IEF loop with the partner's [art_pose | shape] (136 floats per sample) all-gathered on the
    pair group before iterations 2 and 3 (model_copenet.py:185,192).  Odd world sizes cannot pair up: skipped."""
    import torch
    import torch.distributed as dist
    from airpose_amd import dist as D
    if world % 2:
        return None
    groups = D.make_pair_groups(world, timeout_s=120)
    split = (net.regressor_feat_part, net.regressor_step_local, net.regressor_step_finish) if net.fold_status()[0] == 1 else None
    ief = D.ViewSplitIEF(net.regressor_step, groups[rank // 2], (2 * (rank // 2), 2 * (rank // 2) + 1), split_step=split)
    v = rank % 2
    im, bb = batch["im%d" % v], batch["bb%d" % v]
    B = im.shape[0]
    pos = torch.tensor([0.0, 0.0, 10.0], device=dev).expand(B, -1).contiguous() * 0.05
    th, sh = net.init_pose.to(dev), net.init_shape.to(dev)

    def fence():
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, n):
        for _ in range(2):
            fn()
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        fence()
        t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) / n

    n0 = ief.n_exchanges
    t_ov = timed(lambda: ief.run(net.forward_feat_ext(im), bb, pos, th, sh, iters=3, shared_init=True), args.steps)
    n_ex = (ief.n_exchanges - n0) // (args.steps + 2)
    # the IEF loop alone from resident features: with the exchange hidden behind the local half of the step, waited for in line, and
    # not issued at all (the partner's rows taken from a buffer: what the loop costs without a wire)
    xf = net.forward_feat_ext(im)
    pose, betas = ief.run(xf, bb, pos, th, sh, iters=3, shared_init=True)
    t_ief_ov = timed(lambda: ief.run(xf, bb, pos, th, sh, iters=3, shared_init=True), 50) if split else None
    t_ief_sync = timed(lambda: ief.run(xf, bb, pos, th, sh, iters=3, shared_init=True, overlap=False), 50)
    partner = torch.cat([pose[:, 9:], betas], 1).contiguous()

    def no_wire():
        p, b = pose, betas
        for _ in range(3):
            p, b = net.regressor_step(xf, bb, p, b, partner)

    t_ief_nowire = timed(no_wire, 50)
    tx = timed(lambda: ief.exchange(pose, betas), 50)
    return {"pairs_per_s": (world // 2) * B / t_ov, "ms_per_step": 1e3 * t_ov,
            "exchange_us": 1e6 * tx, "n_exchanges": n_ex, "bytes_per_exchange": B * 136 * 4,
            "ief_loop_us": {"exchange_hidden_behind_local_half": None if t_ief_ov is None else 1e6 * t_ief_ov,
                            "exchange_waited_in_line": 1e6 * t_ief_sync, "no_exchange": 1e6 * t_ief_nowire},
            "exchange_exposed_us_per_forward": {"overlapped": None if t_ief_ov is None else 1e6 * (t_ief_ov - t_ief_nowire),
                                                "in_line": 1e6 * (t_ief_sync - t_ief_nowire)},
            "overlap": "exchange_start before the 2196 partner-independent columns (ap_regressor_step_local), exchange_wait before the 136 "
                       "partner columns (ap_regressor_step_finish)" if split else "off: the handle runs the literal chain",
            "topology": "%d pair groups of 2 ranks, one view per rank, %d pairs per group" % (world // 2, B),
            "collective": "2-rank all_gather on the pair group, torch.distributed backend %s%s" % (
                dist.get_backend(), " (= RCCL over xGMI)" if dist.get_backend() == "nccl" else " (host-staged: test aid)")}


def step_outputs(out):
    """What a caller of the timed path receives from one step, as name -> tensor: the output dict of TwoViewInference.__call__ /
    submit (a Pending is waited for first, with the range check it carries), or the four tensors of the network-only forms."""
    from airpose_amd import pipeline
    if isinstance(out, pipeline.Pending):
        out = out.synchronize()
    if isinstance(out, dict):
        return dict(out.items())
    return dict(zip(("pred_pose0", "pred_betas0", "pred_pose1", "pred_betas1"), out))


def dump_outputs(outs, d, seed=0):
    """outs -> d/<name>.npy in float32 (float64 stays float64).  An output above DUMP_ARRAY_BYTES keeps a fixed, seeded sample of its
    rows (axis 0, sorted; the same rows for every output of that length): pred_vertices_cam* (256 x 10475 x 3) -> 33 bodies."""
    import numpy as np
    import torch
    os.makedirs(d, exist_ok=True)
    for name, t in sorted(outs.items()):
        a = (t.double() if t.dtype == torch.float64 else t.float()).cpu().numpy()
        if a.nbytes > DUMP_ARRAY_BYTES and a.ndim:
            k = max(1, DUMP_ARRAY_BYTES // (a.nbytes // a.shape[0]))
            a = a[np.sort(np.random.default_rng(seed).choice(a.shape[0], k, replace=False))]
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a))


def self_launch(argv, n):
    """`python bench.py --gpus N` without a launcher's environment: become `python -m torch.distributed.run --standalone`-style
    (explicit 127.0.0.1 rendezvous on a free port: the container hostname may not resolve) with N ranks of this script."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.stdout.flush()
    os.execvp(cmd[0], cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="pairs per GPU")
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "bf16x2", "fp32"],
                    help="f16 (default) / bf16: the throughput kernels with fp16 / bf16 storage; bf16x2, fp32: the parity-grade modes")
    ap.add_argument("--chunk", type=int, default=0, help="images per depth-first trunk chunk (0 = default)")
    ap.add_argument("--no-tail", action="store_true", help="time the network only (BASELINE config 2 shape)")
    ap.add_argument("--force-dist", action="store_true", help="initialise the RCCL process group even with one rank (test aid)")
    ap.add_argument("--dual-stream", type=int, default=1, help="two-view trunk as two concurrent passes (default) or one pass (0)")
    ap.add_argument("--overlap-tail", type=int, default=1,
                    help="1 (default): steps issued through TwoViewInference.submit (serving form: the passes of step i+1 queue behind "
                         "those of step i, IEF loop + SMPL-X stage of step i on a second stream under them); 0: the stream-ordered "
                         "forward.  With --full the other form is timed for one more block and reported beside the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them returned as DIR/<name>.npy (float32 / float64; a fixed "
                         "seeded sample of the rows of every output above %d MiB)" % (DUMP_ARRAY_BYTES >> 20))
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement and check after the headline's steps: conv-stack HIP events in the "
                         "timed steps, roofline and per-stage figures, repeat blocks, the other step-issue form, the fp16 range check, "
                         "CPU baseline, parity against the CPU oracle, the other precisions, batch 64, AirPose+ fitting, view split")
    fl = ap.add_argument_group("secondary measurements (with --full only)")
    fl.add_argument("--cpu-sample", type=int, default=16, help="pairs in the CPU baseline sample (0 = skip)")
    fl.add_argument("--stage-steps", type=int, default=5, help="extra untimed steps with per-stage HIP events")
    fl.add_argument("--repeat-blocks", type=int, default=6, help="extra blocks after the contract's K-step one (spread; GPU busy >= 3 s)")
    fl.add_argument("--repeat-steps", type=int, default=100, help="steps of each extra block")
    fl.add_argument("--parity-sweep", type=int, default=1, help="every mode vs the CPU oracle over 3 weight seeds x 2 input seeds + a second BN range (0 = skip)")
    fl.add_argument("--airpose-plus", type=int, default=1, help="BASELINE config 4: 300-iteration fit of 64 frames (0 = skip)")
    fl.add_argument("--parity-steps", type=int, default=3, help="steps of the parity-grade mode after the main loop (0 = skip)")
    fl.add_argument("--parity-pairs", type=int, default=128, help="pairs (two input seeds) on which the TIMED mode is checked against the CPU oracle (0 = skip)")
    fl.add_argument("--other-form", type=int, default=1, help="0: skip the extra block that times the other step-issue form (profiling runs)")
    fl.add_argument("--b64", type=int, default=1, help="also time BASELINE config 1 (batch 64, network only, bf16 and f16): 0 = skip")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:     # the plain command: launch the N ranks ourselves (never returns)
        self_launch(sys.argv[1:], args.gpus)

    import torch
    import torch.distributed as dist
    from airpose_amd import copenet_model, pipeline, smplx, smplx_model
    from airpose_amd import weights as W

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:                                           # N ranks generate their weights / inputs side by side: share the host cores
        torch.set_num_threads(max(1, (os.cpu_count() or 8) // world))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (a launcher started another number of ranks than --gpus names)" % (args.gpus, world))
    if os.environ.get("AIRPOSE_BENCH_LAUNCH_ONLY") == "1":
        # test aid (tests/test_abi.py, no GPU): everything up to the point the GPU is needed -- the launcher, the rendezvous, one
        # collective over all ranks -- then one JSON line from rank 0
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world > 1:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.ones(1)
        if world > 1:
            dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"launcher": "ok", "n_gpus": world, "n_ranks_seen": int(t.item()), "local_rank": local_rank}))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py needs the MI355X; there is no CPU fallback"
    # test aid (a 1-GPU box cannot host two RCCL ranks): AIRPOSE_BENCH_SHARE_GPU=1 puts every rank on cuda:0 with the gloo
    # backend, so the N > 1 code paths (max-over-ranks timing, view_split block) can be exercised on one GPU
    share = os.environ.get("AIRPOSE_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    n_ranks_seen = 1
    if use_dist:
        t = torch.ones(1, device=dev)
        dist.all_reduce(t)
        n_ranks_seen = int(t.item())
    B = args.batch
    sd = W.to_torch(W.copenet_state_dict(20240901, MEAN))
    md = smplx_model.make_synthetic_model(4321)
    net = copenet_model.getcopenet(MEAN, precision=args.precision).eval()
    net.load_state_dict(sd)
    body = smplx.SMPLX(model_data=md)
    pipe = pipeline.TwoViewInference(net, body, iters=3)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(1234 + rank, B).items()}
    if args.chunk:
        torch.zeros(1, device=dev)
        net.set_chunk(args.chunk)
    if args.dual_stream != 1:                               # 0 = one pass; 1 + k = the second pass starts k stages late (tuning)
        torch.zeros(1, device=dev)
        net.set_dual_stream(args.dual_stream)
    if os.environ.get("AIRPOSE_SMPLX_FUSED"):               # A/B aid: fused contraction + skinning on (default) / off
        body.set_fused(int(os.environ["AIRPOSE_SMPLX_FUSED"]))
    if os.environ.get("AIRPOSE_FUSE_PAIR"):                 # A/B aid: fused conv3 -> conv1 pairs on (default) / off
        net.set_fuse_pair(int(os.environ["AIRPOSE_FUSE_PAIR"]))
    if os.environ.get("AIRPOSE_TILED"):                     # A/B aid: fragment-tiled pair-kernel intermediates (default) / NHWC
        net.set_tiled(int(os.environ["AIRPOSE_TILED"]))
    if os.environ.get("AIRPOSE_FUSE_STEM"):                 # A/B aid: 1 persistent stem + pool kernel (default), 2 its first cut, 0 two kernels
        net.set_fuse_stem(int(os.environ["AIRPOSE_FUSE_STEM"]))
    if os.environ.get("AIRPOSE_FUSE_POOL"):                 # A/B aid: AvgPool2d(7) in the last convolution's epilogue (default) / own kernel
        net.set_fuse_pool(int(os.environ["AIRPOSE_FUSE_POOL"]))
    if os.environ.get("AIRPOSE_FUSE_TAIL"):                 # A/B aid: conv1 of layer2.0 inside layer1's last kernel (default) / own convolution
        net.set_fuse_tail(int(os.environ["AIRPOSE_FUSE_TAIL"]))
    if os.environ.get("AIRPOSE_PW_CONV"):                   # A/B aid: layer4's pointwise layers on conv_pw.hip (1: by size, default; 2 always) / generic kernels (0)
        net.set_pw_conv(int(os.environ["AIRPOSE_PW_CONV"]))
    if os.environ.get("AIRPOSE_IMG3"):                      # A/B aid: layer2's 3x3 with half an image resident in LDS (default) / slab kernel
        net.set_img3(int(os.environ["AIRPOSE_IMG3"]))
    if os.environ.get("AIRPOSE_S2P"):                       # A/B aid: layer2.0's stride-2 3x3 on the polyphase kernel (1) / the ring kernel (0, default)
        net.set_s2p(int(os.environ["AIRPOSE_S2P"]))
    if os.environ.get("AIRPOSE_STEM"):                      # A/B aid: stem + pool as persistent workgroups (1, default) / a workgroup per strip (2)
        net.set_fuse_stem(int(os.environ["AIRPOSE_STEM"]))
    if os.environ.get("AIRPOSE_IMG_BLOCK"):                 # A/B aid: layer3 identity blocks as image-resident kernels (default) / conv2 + pairs
        net.set_img_block(int(os.environ["AIRPOSE_IMG_BLOCK"]))
    if os.environ.get("AIRPOSE_EVEN_OUT"):                  # A/B aid: block outputs only a stride-2 downsample reads: even pixels (default) / in full
        net.set_even_out(int(os.environ["AIRPOSE_EVEN_OUT"]))
    if os.environ.get("AIRPOSE_FUSE_BLOCK"):                # A/B aid: layer1 blocks: 1 fused kernel each (default), 0 separate convs
        net.set_fuse_block(int(os.environ["AIRPOSE_FUSE_BLOCK"]))
    if os.environ.get("AIRPOSE_CONV_CONFIG"):                # A/B aid: tile configuration of the conv kernels (ap_set_conv_config)
        from airpose_amd import _native as Nn
        Nn.check(Nn.lib().ap_set_conv_config(int(os.environ["AIRPOSE_CONV_CONFIG"])), "ap_set_conv_config")

    def step():
        if args.no_tail:
            if args.overlap_tail and not instrumented[0]:
                return pipe.submit_net(batch["im0"], batch["im1"], batch["bb0"], batch["bb1"])
            return pipe.forward_net(batch["im0"], batch["im1"], batch["bb0"], batch["bb1"])
        if args.overlap_tail and not instrumented[0]:
            return pipe.submit(batch, want_rotmat=True)
        return pipe(batch, want_rotmat=True)

    instrumented = [False]                                   # the per-stage steps after the timed region run serially

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(max(args.warmup, 1)):
        out = step()
    torch.cuda.synchronize()
    # Timed region.  --full: the conv stack carries HIP events (the roofline line needs that pair; every event record costs
    # a ~5 us bubble on the stream), the per-stage breakdown comes from extra, untimed steps below.  A plain run: no events.
    if args.full:
        net.enable_timing(2)
        net.timing(reset=True)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    fence()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:                      # before anything else reuses the buffers the last step wrote
        dump_outputs(step_outputs(out), args.dump_outputs)
    if args.full:
        tm = net.timing(reset=True)
        launches_timed = net.last_conv_launches()            # conv-stack launches of the last timed step, all passes (ap_net_last_conv_launches)
        # the same block again, a few times: spread of the headline inside one process (the contract's `value` stays the
        # first block; the timed region of 20 steps is only ~0.14 s)
        blocks = [world * B * args.steps / elapsed]
        rsteps = max(args.repeat_steps, 1)
        for _ in range(max(args.repeat_blocks, 0)):
            fence()
            t1 = time.perf_counter()
            for _ in range(rsteps):
                out = step()
            fence()
            dt = time.perf_counter() - t1
            if use_dist:
                t = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            blocks.append(world * B * rsteps / dt)
        # the other form of the same forward, one more block of K steps: stream-ordered __call__ when the headline is the serving form
        # (TwoViewInference.submit) and the other way round -- same kernels, bit-identical outputs
        other = None
        if not args.no_tail and args.other_form:
            other_step = (lambda: pipe(batch, want_rotmat=True)) if args.overlap_tail else (lambda: pipe.submit(batch, want_rotmat=True))
            for _ in range(2):
                pend = other_step()
            fence()
            net.timing(reset=True)
            t1 = time.perf_counter()
            for _ in range(args.steps):
                pend = other_step()
            fence()
            dt = time.perf_counter() - t1
            tm_other = net.timing(reset=True)
            del pend
            if use_dist:
                t = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            other = {"pairs_per_s": world * B * args.steps / dt, "ms_per_step": 1e3 * dt / args.steps,
                     "conv_stack_ms": tm_other["conv_ms"] / max(tm_other["passes"], 1),
                     "what": ("TwoViewInference.__call__: every step complete in the order of the caller's stream before the next one "
                              "starts (the reference boundary's semantics)") if args.overlap_tail else
                             ("TwoViewInference.submit: the passes of step i+1 queue behind those of step i, IEF loop + SMPL-X stage "
                              "of step i on a second stream under them; outputs ready at Pending.wait")}
        net.timing(reset=True)
        # stage breakdown: a few more steps, fully instrumented, outside the timed region
        net.enable_timing(1)
        instrumented[0] = True
        if not args.no_tail:
            body.enable_timing(True)
            body.timing(reset=True)
        for _ in range(args.stage_steps):
            out = step()
        torch.cuda.synchronize()
        ts = net.timing(reset=True)
        tb = body.timing(reset=True) if not args.no_tail else None
        # the tail once more as ONE span (an event in front of its first kernel and one behind its last): every event record between two
        # kernels costs a bubble of several microseconds on the stream, three of them sit inside the per-stage sum above
        tail_span_ms = None
        if not args.no_tail and args.stage_steps > 0:
            body.enable_timing(2)
            body.timing(reset=True)
            for _ in range(args.stage_steps):
                out = step()
            torch.cuda.synchronize()
            t2 = body.timing(reset=True)
            tail_span_ms = t2["prep_ms"] / max(t2["passes"], 1)
            body.enable_timing(False)
        net.enable_timing(0)
        del out
        # fp16 storage: the range sentinel (deferred mode: nothing on the hot path) must be silent after everything timed above
        range_ok = None
        if args.precision == "f16":
            net.range_status()                                   # raises airpose_amd._native.RangeError if any pass left the fp16 range
            range_ok = True
        cpu, sample, want = (None, None, None)
        if rank == 0 and world == 1 and args.cpu_sample > 0:
            cpu, sample, want = cpu_baseline(sd, md, args.cpu_sample)
        parity = parity_block(args, sd, body, batch, net, sample, want, dev) if (rank == 0 and world == 1 and not args.no_tail) else None
        timed_parity = None
        if rank == 0 and world == 1 and not args.no_tail and cpu is not None and args.parity_pairs > 0:
            timed_parity = timed_mode_parity(sd, md, pipe, dev, cpu["cores"], pairs_per_seed=max(1, args.parity_pairs // 2),
                                             submit=bool(args.overlap_tail))
        b64 = None
        if rank == 0 and world == 1 and args.b64 and args.precision in ("bf16", "f16") and B != 64:
            b64 = b64_block(args, sd, body, dev)
        sweep = None
        if rank == 0 and world == 1 and not args.no_tail and cpu is not None and args.parity_sweep:
            sweep = parity_sweep(args, md, body, dev, cpu["cores"])
        fitres = None
        if rank == 0 and world == 1 and args.airpose_plus and not args.no_tail:
            try:
                fitres = airpose_plus_block(md, dev)
            except Exception as e:                               # noqa: BLE001 (reported, not swallowed)
                fitres = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        # the secondary measurement must never cost the primary one: an exception in the view-split block (it needs the pair
        # communicators of a multi-GPU node, which no box of this round offered) is reported in the line instead of ending the run
        vs = None
        if world >= 2:
            try:
                vs = view_split_block(args, net, batch, dev, rank, world)
            except Exception as e:                               # noqa: BLE001 (reported, not swallowed)
                vs = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}

    if rank == 0:
        value = world * B * args.steps / elapsed
        chunk = args.chunk or 512
        # two-view forwards of >= 64 pairs run the two views as two concurrent trunk passes (two internal streams)
        dual = bool(args.dual_stream) and B >= 64 and chunk >= 128    # (views above chunk / 2 images: slices of chunk / 2 per pass stream)
        res = {
            "metric": "two-view frames/sec at batch %d (224x224)" % B,
            "value": value,
            "unit": "pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic",
            "arithmetic": {"f16": "fp16 storage, v_mfma_f32_16x16x32_f16, fp32 accumulate and epilogues",
                           "bf16": "bf16 storage, v_mfma_f32_16x16x32_bf16, fp32 accumulate and epilogues",
                           "bf16x2": "split-bf16 pairs, three bf16 MFMA products per product, fp32 accumulate",
                           "fp32": "fp32 storage, v_mfma_f32_16x16x4_f32"}[args.precision],
            "config": {"workload": "copenet_twoview forward (ResNet-50 x2 views, 3 IEF iterations) + SMPL-X LBS tail "
                                   "(10475 verts, 127 joints, projection)" if not args.no_tail else
                                   "copenet_twoview forward only (ResNet-50 x2 views, 3 IEF iterations)",
                       "pairs_per_gpu": B, "global_pairs": world * B, "image": "224x224", "ief_iters": 3,
                       "trunk_chunk_images": chunk,
                       "trunk_passes": "2 concurrent passes (one per view) on 2 HIP streams" if dual else "1 pass per chunk",
                       "step_issue": ("TwoViewInference.submit (serving form): the trunk passes of step i+1 queue behind those of step i, IEF loop + "
                                      "SMPL-X stage of step i on a second stream under them (at most 3 steps in flight); all K steps "
                                      "complete inside the timed region; outputs bit-identical to forward().  The figure with the "
                                      "REFERENCE's forward() semantics (every step complete in stream order before the next starts) is "
                                      "`stream_ordered.pairs_per_s` of the --full line -- use that one to compare across rounds") if args.overlap_tail else
                                     "stream-ordered: every step complete on the caller's stream before the next starts (the reference's forward() semantics)",
                       "sharding": "whole pairs per GPU, no data-path collective"},
        }
    if rank == 0 and args.full:
        n_img = 2 * B
        conv_flops_step = conv_stack_flops_per_image() * n_img
        conv_ms_step = tm["conv_ms"] / max(tm["passes"], 1)
        # 52 convs: 4 downsample convs folded into conv3, layer1's 3 bottlenecks are one fused kernel each (bf16)
        # two concurrent trunk passes: twice the launches at half the images each; conv_ms is then the span over both passes
        launches = launches_timed                                # read back from the library behind the timed region: what it chose for this batch
        # bf16x2 runs on the bf16 matrix pipe (3 MFMA products per algorithmic product): priced against the same peak
        peak = PEAK_FP32_TFLOPS if args.precision == "fp32" else PEAK_BF16_DENSE_TFLOPS
        achieved = conv_flops_step / (conv_ms_step * 1e-3) / 1e12
        # roofline.achieved of the trunk + regressor line = pairs/s x 16.3916 GFLOP (trunk 2 x 8.174 incl. the stem +
        # regressor 0.043) against the dense bf16 / fp16 MFMA peak -- the WHOLE step time in the denominator
        path_flops_pair = (conv_stack_flops_per_image() + STEM_FLOPS_PER_IMAGE) * 2 + REG_FLOPS_PER_PAIR
        path_tf = value / world * path_flops_pair / 1e12
        # the conv stack alone, as a span: the stream-ordered block (the two passes of a step run in lock step and the HIP events
        # bracket both) when it was timed; in the serving form the passes of consecutive steps drift apart and only each pass's own
        # duration exists (reported as conv_stack_own_ms: it shares the chip with the other pass's stem / pooling part of the time)
        span_ms = other.get("conv_stack_ms") if (other is not None and args.overlap_tail) else (conv_ms_step if not args.overlap_tail else None)
        res.update({
            "roofline": {"bound": "mfma",
                         "kernel": "the 52 fused conv+BN(+residual)+ReLU layers of the trunk in %d launches per step; in the 16-bit modes, by share of "
                                   "the stack's time: blk_img_kernel (layer3's five identity bottlenecks, one image-resident kernel each), "
                                   "conv_pair_kernel (conv3 of the layer2 blocks / layer3.0 together with the next block's conv1), bneck2_kernel (layer1's "
                                   "three bottlenecks, the last one with conv1 of layer2.0), conv_slab_kernel (stride-1 3x3 of layer2 / layer4), "
                                   "conv_pw_kernel (conv1 and conv3+downsample of layer4; alone on the chip also the 3x3/2 of layer3.0 / 4.0), "
                                   "conv_pipe_kernel<T,128,128,2,4,2> (the remaining stride-2 3x3 layers), conv_lean_kernel (conv3 of the layer4 "
                                   "identity blocks); time = HIP events around the conv stack on the streams that run "
                                   "it: stream-ordered steps: the span over both concurrent passes; steps issued through submit (the "
                                   "passes of consecutive steps run free of each other and drift apart): the mean of the two passes' "
                                   "own durations, each of which shares the chip with the other stream throughout (equal to the "
                                   "span in lock step); frac_of_step_time = the same flops over the whole step time" % launches,
                         "achieved": path_tf, "peak": peak, "unit": "TFLOP/s", "frac": path_tf / peak,
                         "formula": "SURVEY 8(d): pairs/s per GPU x %.4f GFLOP per pair (trunk incl. stem x 2 views + 3 IEF iterations) / peak; "
                                    "whole step time in the denominator" % (path_flops_pair / 1e9),
                         "conv_stack_span_ms": span_ms,
                         "conv_stack_achieved": None if span_ms is None else conv_flops_step / (span_ms * 1e-3) / 1e12,
                         "conv_stack_frac": None if span_ms is None else conv_flops_step / (span_ms * 1e-3) / 1e12 / peak,
                         "conv_stack_span_of": "the stream-ordered block of this run (HIP events bracket both lock-step passes of a step)",
                         "conv_stack_own_ms": conv_ms_step, "conv_stack_own_frac": achieved / peak,
                         "frac_of_step_time": conv_flops_step / (elapsed / args.steps) / 1e12 / peak,
                         "traffic": pmc_traffic(), "traffic_unit": "HBM bytes per step of %d pairs (FETCH_SIZE x 2 + WRITE_SIZE over the conv-stack kernels)" % 256,
                         "traffic_source": "latest committed rocprofv3 PMC pass (profiles/r*_pmc_traffic.json): counters cannot be collected inside the timed run",
                         "flops_per_launch": conv_flops_step / launches, "launches_per_step": launches,
                         "avg_launch_ms": (span_ms if span_ms is not None else conv_ms_step) / launches,
                         "peak_note": "peak is the guide's dense 16-bit figure; a loop of nothing but v_mfma_f32_16x16x32 in this library's "
                                      "shape sustains 1.7-1.8 PFLOP/s on all 256 CUs (clock 2.35 -> 1.64-1.79 GHz under that load; "
                                      "tools/probes/mfma_rate_probe.hip, profiles/r06_mfma_rate_probe.txt): frac %.3f of peak = %.2f-%.2f of that"
                                      % (path_tf / peak, path_tf / 1800.0, path_tf / 1700.0)},
            "stage_ms_per_step": {"stem_maxpool": ts["stem_ms"] / max(ts["passes"], 1), "conv_stack": conv_ms_step,
                                  "avgpool": ts["avgpool_ms"] / max(ts["passes"], 1),
                                  "regressor": ts["regressor_ms"] / max(ts["passes"], 1),
                                  "source": "conv_stack: HIP events inside the timed region; other stages: %d extra "
                                            "instrumented steps after it" % args.stage_steps},
            "path_tflops": path_tf,
        })
        srt = sorted(blocks)
        res["repeat_blocks"] = {"n": len(blocks), "steps_each": rsteps, "median": srt[len(srt) // 2], "min": srt[0],
                                "max": srt[-1], "unit": "pairs/s", "note": "block 0 is `value` (K = %d steps); the others run %d steps each" % (args.steps, rsteps)}
        if tb is not None and tb["passes"] > 0:              # (--stage-steps 0: no instrumented tail passes)
            p = max(tb["passes"], 1)
            # default: blend-shape contraction + skinning are ONE kernel (smplx_lbs_fused_kernel), timed in the blend slot; the
            # skin slot is then empty (two-kernel path: AIRPOSE_SMPLX_FUSED=0)
            fused_tail = os.environ.get("AIRPOSE_SMPLX_FUSED", "1") != "0"
            st = {"smplx_prep": tb["prep_ms"] / p, ("smplx_lbs_fused" if fused_tail else "smplx_blend_gemm"): tb["blend_gemm_ms"] / p,
                  "smplx_skin": tb["skin_ms"] / p, "smplx_joints": tb["joints_ms"] / p}
            res["stage_ms_per_step"].update(st)
            # the WHOLE tail (prep + blend-shape contraction + skinning + joints/projection: every kernel that
            # touches the bytes below) against 129 084 B per body + 25.5 MB of model constants per launch
            stage_sum_ms = sum(st.values())
            tail_ms = tail_span_ms if tail_span_ms else stage_sum_ms
            tail_bytes = n_img * TAIL_BYTES_PER_BODY + TAIL_CONST_BYTES
            res["smplx_tail_roofline"] = {"bound": "hbm", "achieved": tail_bytes / (tail_ms * 1e-3) / 1e9,
                                          "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                          "frac": tail_bytes / (tail_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                          "bytes": tail_bytes, "ms": tail_ms,
                                          "ms_is": "the span from the first kernel of the tail to its last, two HIP events, behind the trunk (stream-ordered "
                                                   "steps)" if tail_span_ms else "sum of the per-stage times",
                                          "sum_of_stage_ms": stage_sum_ms,
                                          "frac_from_sum_of_stage_ms": tail_bytes / (stage_sum_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                          "note": "the per-stage times carry one event record each between the kernels (a bubble of several microseconds "
                                                  "on the stream): their sum overstates the tail; rounds 1-5 reported that sum",
                                          "kernels": ("smplx_prep + smplx_lbs_fused (blend-shape contraction + skinning in one kernel) + smplx_joints "
                                                      if fused_tail else "smplx_prep + smplx_blend_gemm + smplx_skin + smplx_joints ") +
                                                     "(their launches back to back on one stream)",
                                          "formula": "n_bodies * 129084 B + 25.5e6 B, n_bodies = 2 * pairs"}
            # algorithmic contraction length: 10 shape + 21 body joints x 9 pose-feature entries, not the
            # zero-padded operand width the kernel runs
            gemm_flops = 2.0 * BLEND_K_ALGORITHMIC * 31425 * n_img
            # the contraction runs in split-bf16 form on the bf16 matrix pipe: three MFMA products per algorithmic product,
            # so the pipe's ceiling for ALGORITHMIC flops is a third of the dense bf16 peak
            blend_peak = PEAK_BF16_DENSE_TFLOPS / 3
            blend_ms = st["smplx_lbs_fused"] if fused_tail else st["smplx_blend_gemm"]
            res["smplx_blend_roofline"] = {"bound": "mfma-bf16 (split-bf16 operands, 3 MFMA products per product)",
                                           "achieved": gemm_flops / (blend_ms * 1e-3) / 1e12,
                                           "peak": blend_peak, "unit": "TFLOP/s",
                                           "frac": gemm_flops / (blend_ms * 1e-3) / 1e12 / blend_peak,
                                           "flops": gemm_flops, "formula": "2 * 199 * 31425 * n_bodies",
                                           "note": ("the contraction is one phase of the fused contraction + skinning kernel: its time includes "
                                                    "the skinning and the vertex stores" if fused_tail else
                                                    "output-bound: the launch writes n_bodies * 125.7 KB of fp32 v_posed")}
        if parity is not None:
            res["parity_mode"] = parity
        if timed_parity is not None:                         # the timed mode itself against north_star's bar
            res["parity_of_timed_mode"] = dict(timed_parity, dtype=args.precision, bar=1e-4,
                                               meets_bar=timed_parity["max_rel_err"] < 1e-4)
        elif parity is not None and "throughput_mode_max_rel_err" in parity:
            res["parity_of_timed_mode"] = {"dtype": args.precision, "max_rel_err": parity["throughput_mode_max_rel_err"],
                                           "bar": 1e-4, "meets_bar": parity["throughput_mode_max_rel_err"] < 1e-4,
                                           "rel_err_by_slice": parity["throughput_mode_rel_err_by_slice"],
                                           "checked_pairs": parity.get("checked_pairs"),
                                           "checker": "fp32 CPU oracle on the cpu_baseline sample"}
        if range_ok is not None:
            res["f16_range_check"] = {"ok": range_ok, "mode": "deferred (host-mapped flag set by the pooling stage of every trunk pass; "
                                                             "read after the timed and instrumented steps)"}
        if b64 is not None:
            res["b64"] = b64
        if sweep is not None:
            res["parity_sweep"] = sweep
            if "parity_of_timed_mode" in res and args.precision in sweep["modes"]:
                sm = sweep["modes"][args.precision]
                res["parity_of_timed_mode"].update({
                    "holds_on_every_checkpoint_of_the_sweep": sm["meets_bar"], "sweep_max_rel_err": sm["max_rel_err"],
                    "sweep_worst": sm["worst_slice"],
                    "modes_that_hold_the_bar_on_every_checkpoint": [m for m, v in sweep["modes"].items() if v["meets_bar"]],
                    "note": "meets_bar refers to the benchmark checkpoint (128 pairs, 2 input seeds); parity_sweep repeats the check for every "
                            "mode over 3 weight seeds and a second BatchNorm-statistics range"})
        if fitres is not None:
            res["airpose_plus"] = fitres
        if other is not None:
            res["stream_ordered" if args.overlap_tail else "overlap_tail"] = other
        if vs is not None:
            res["view_split"] = vs
        if cpu is not None:
            res["cpu_baseline"] = cpu
            # BASELINE.md publishes no throughput for this metric: vs_baseline stays null (the contract); the ratio to the CPU path
            # measured on this box is reported under its own name
            res["gpu_over_cpu_baseline"] = res["value"] / cpu["value"]
    if rank == 0:
        res["n_ranks_seen"] = n_ranks_seen
        print(json.dumps(res))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
