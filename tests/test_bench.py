"""bench.py's contract: a plain run prints the headline line only, --steps sets the timed steps, --dump-outputs writes what the
last timed step returned (float32, a seeded row sample of large outputs, at most 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MEAN_PARAMS, REPO, pose_rel_errs, rel_err


def test_dump_outputs_is_float32_and_samples_large_outputs(tmp_path):
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    verts = torch.randn(256, 10475, 3, generator=g)
    outs = {"pred_pose0": torch.randn(256, 135, generator=g), "pred_vertices_cam0": verts, "pred_vertices_cam1": verts + 1,
            "half": torch.randn(4, 3, generator=g).to(torch.bfloat16), "wide": torch.randn(5, dtype=torch.float64, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert sorted(got) == sorted(outs)
    assert got["pred_pose0"].dtype == np.float32 and np.array_equal(got["pred_pose0"], outs["pred_pose0"].numpy())
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], outs["half"].float().numpy())
    assert got["wide"].dtype == np.float64 and np.array_equal(got["wide"], outs["wide"].numpy())
    v0, v1 = got["pred_vertices_cam0"], got["pred_vertices_cam1"]
    assert v0.dtype == np.float32 and v0.shape == (bench.DUMP_ARRAY_BYTES // (10475 * 3 * 4), 10475, 3)
    assert v0.nbytes <= bench.DUMP_ARRAY_BYTES
    np.testing.assert_array_equal(v1, v0 + 1)                   # the same rows of every output of that length
    rows = [int(np.flatnonzero((verts.numpy() == r).all(axis=(1, 2)))[0]) for r in v0]
    assert rows == sorted(set(rows))                            # distinct rows of the original, in order
    for f in os.listdir(str(tmp_path / "a")):                   # the same sample in every run
        assert np.array_equal(np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))), f
    assert sum(a.nbytes for a in got.values()) <= 64 << 20


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run: the headline keys and nothing measured after the steps; value and ms_per_step describe exactly --steps steps; the
    dumped outputs are those of the stream-ordered forward of the same seeded weights and inputs."""
    import torch
    from airpose_amd import copenet_model, pipeline, smplx, smplx_model
    from airpose_amd import weights as W
    B, steps, d = 8, 3, str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", d], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["dtype"] == "f16" and line["unit"] == "pairs/s" and line["higher_is_better"] is True
    assert abs(line["value"] * line["ms_per_step"] / (1e3 * B) - 1) < 1e-9
    for k in ("roofline", "repeat_blocks", "cpu_baseline", "parity_sweep", "b64", "airpose_plus", "stream_ordered"):
        assert k not in line, k
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert got["pred_vertices_cam0"].shape == (B, 10475, 3) and got["pred_pose1"].shape == (B, 135)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())

    dev = torch.device("cuda", 0)
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    net.load_state_dict(W.to_torch(W.copenet_state_dict(20240901, MEAN_PARAMS)))
    pipe = pipeline.TwoViewInference(net, smplx.SMPLX(model_data=smplx_model.make_synthetic_model(4321)), iters=3)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(1234, B).items()}
    want = {k: v.float().cpu().numpy() for k, v in pipe(batch, want_rotmat=True).items()}
    assert sorted(got) == sorted(want)
    for k in want:
        errs = pose_rel_errs(got[k], want[k]).values() if k.startswith("pred_pose") else [rel_err(got[k], want[k])]
        assert max(errs) < 1e-5, k
