"""The launch-side caches are per DEVICE (csrc/ap_device.h): what ran on cuda:0 first runs on cuda:1 afterwards, in ONE process.

That order is the one in which a process-wide "already opted in" flag is wrong: the second device launches a kernel that asks for
more than 64 KiB of dynamic LDS without its hipFuncSetAttribute.  (fitting.hip kept such a flag until its launchers moved onto
ap_lds_optin.)  Every kernel here is deterministic and its grid depends on the problem and the CU count alone, so two equal devices
give equal bits: the results of cuda:1 are compared bit for bit with those of cuda:0, and no call may raise.

Skipped on a machine with fewer than two GPUs.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
MEAN_PARAMS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "airpose_amd", "data", "smpl_mean_params.npz")


@pytest.fixture(scope="module")
def devices():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs in one process")
    return torch.device("cuda", 0), torch.device("cuda", 1)            # cuda:0 FIRST


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_fitter_on_the_second_device(devices, smplx_model):
    """4 frames = one workgroup of the decoder's DR = 4 rows; n_iters = 2 with switch_iter = 1 launches all four fit kernels in one
    call (decode, frame, adam before the switch; decode, backprop-adam after it); the two that opt in to 84 480 bytes of LDS are among them"""
    from airpose_amd import smplx
    from airpose_amd.fitting import AirPosePlusFitter, synthetic_fit_problem
    vp, st, dd = synthetic_fit_problem(frames=4, seed=77, device="cpu")
    fitted = []
    for dev in devices:
        body = smplx.SMPLX(model_data=smplx_model)
        fitter = AirPosePlusFitter(vp, body, dev)
        out, hist = fitter.run(st, dd["j2d"], dd["robust"], dd["intr"], dd["extr"], n_iters=2, switch_iter=1, want_loss=True)
        torch.cuda.synchronize(dev)
        assert all(v.device == dev and torch.isfinite(v).all() for v in out.values()), dev
        assert any(not torch.equal(out[k].cpu(), st[k]) for k in ("z", "phi0", "tau0")), "the fit moved nothing"
        fitted.append(dict(out, loss=hist))
    for k in fitted[0]:
        assert torch.equal(bits(fitted[0][k]), bits(fitted[1][k])), (k, "cuda:1 differs from cuda:0")


def test_trunk_and_smplx_on_the_second_device(devices, golden, copenet_sd, copenet_inputs, smplx_model):
    """the copenet_b2 case (batch 2, fp16 storage) through copenet.forward and SMPLX.forward_fused: the default path's dynamic-LDS
    kernels (stem, bottleneck, pair, image kernels, pooled tail, fused LBS) on a device that did not make the first call"""
    from airpose_amd import copenet_model, smplx
    pos = torch.from_numpy(golden["copenet_b2"]["init_position"])
    got = []
    for dev in devices:
        net = copenet_model.getcopenet(MEAN_PARAMS, precision="f16")
        net.load_state_dict(copenet_sd)
        net = net.to(dev).eval()
        body = smplx.SMPLX(model_data=smplx_model)
        gin = {k: v.to(dev) for k, v in copenet_inputs.items()}
        p = pos.to(dev)
        with torch.no_grad():
            p0, b0, p1, b1 = [t.clone() for t in net(gin["im0"], gin["im1"], gin["bb0"], gin["bb1"], p, p, iters=3)]
            cc = torch.tensor([960.0, 540.0], device=dev).expand(p0.shape[0], 2).contiguous()
            o = body.forward_fused(p0, b0, cc)
        torch.cuda.synchronize(dev)
        res = dict(pose0=p0, betas0=b0, pose1=p1, betas1=b1, **{k: v for k, v in o.items() if torch.is_tensor(v)})
        assert all(v.device == dev and torch.isfinite(v).all() for v in res.values()), dev
        got.append(res)
    assert {"vertices_cam", "j3d_cam", "j2d_cam"} <= set(got[0])
    for k in got[0]:
        assert torch.equal(bits(got[0][k]), bits(got[1][k])), (k, "cuda:1 differs from cuda:0")
