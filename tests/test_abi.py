"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol
include/airpose_hip.h declares (no compute calls: there is no GPU here), the host mirrors keep the
reference's contracts, and the product refuses to run without the GPU instead of falling back."""
import os
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import MEAN_PARAMS, REPO


def _declared():
    src = open(os.path.join(REPO, "include", "airpose_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ap_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from airpose_amd import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _native.lib()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), n
        assert n in _native.SIGNATURES, "ctypes signature missing for " + n
    assert sorted(_native.SIGNATURES) == names
    assert b"gfx950" in L.ap_version()


def test_abi_version_matches_header_and_binding():
    """An out-of-tree caller built against another header must be able to tell: the library exports the ABI number of the header
    it was built from, and the ctypes binding refuses any other."""
    import re
    from airpose_amd import _native
    hdr = open(os.path.join(REPO, "include", "airpose_hip.h")).read()
    want = int(re.search(r"#define\s+AP_ABI_VERSION\s+(\d+)", hdr).group(1))
    L = ctypes.CDLL(_native.LIB_PATH)
    L.ap_abi_version.restype = ctypes.c_int
    assert L.ap_abi_version() == want == _native.ABI_VERSION
    L.ap_version.restype = ctypes.c_char_p
    assert ("abi %d" % want).encode() in L.ap_version()


def test_state_dict_contract_matches_reference(golden, copenet_sd):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS)
    ref_keys = [str(k) for k in golden["copenet_b2"]["state_dict_keys"]]
    assert list(net.state_dict().keys()) == ref_keys            # same names, same order, 331 entries
    res = net.load_state_dict(copenet_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert net.init_pose.shape == (1, 144) and net.init_shape.shape == (1, 10) and net.init_cam.shape == (1, 3)
    for attr in ("fc1", "fc2", "decpose", "decshape", "deccam", "conv1", "bn1", "layer1", "layer4"):
        assert hasattr(net, attr)
    assert net.fc1.in_features == 2332 and net.decpose.out_features == 135


def test_lightning_style_checkpoint_loads(copenet_sd, tmp_path):
    """Lightning checkpoints prefix the network with 'model.' (copenet_twoview.py:60)."""
    from airpose_amd import copenet_model

    class Wrapper(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.model = copenet_model.getcopenet(MEAN_PARAMS)

    ck = {"state_dict": {"model." + k: v for k, v in copenet_sd.items()}}
    p = str(tmp_path / "last.ckpt")
    torch.save(ck, p)
    w = Wrapper()
    w.load_state_dict(torch.load(p)["state_dict"], strict=True)
    assert torch.equal(w.model.fc1.weight, copenet_sd["fc1.weight"])


def test_no_cpu_fallback(copenet_sd):
    from airpose_amd import copenet_model, geometry, smplx, smplx_model
    net = copenet_model.getcopenet(MEAN_PARAMS).eval()
    with pytest.raises(RuntimeError, match="no CPU"):
        net(torch.zeros(1, 3, 224, 224), torch.zeros(1, 3, 224, 224), torch.zeros(1, 3), torch.zeros(1, 3),
            torch.zeros(1, 3), torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="no CPU"):
        geometry.rot6d_to_rotmat(torch.zeros(2, 6))
    small = smplx_model.make_synthetic_model(1, num_verts=300, num_faces=100)
    body = smplx.SMPLX(model_data=small)
    with pytest.raises(RuntimeError, match="no CPU"):
        body.forward(betas=torch.zeros(1, 10), body_pose=torch.eye(3).expand(1, 21, 3, 3), pose2rot=False)
    with pytest.raises(FileNotFoundError):
        smplx.SMPLX("/nonexistent/models/smplx")


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under airpose_amd/ may import or call it."""
    pkg = os.path.join(REPO, "airpose_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "/root/reference" not in txt, f


def test_synthetic_inputs_contract():
    from airpose_amd import weights as W
    d = W.synthetic_inputs(1234, 3)
    assert d["im0"].shape == (3, 3, 224, 224) and d["im0"].dtype == np.float32
    assert d["bb0"].shape == (3, 3) and (d["bb0"][:, 2] >= 0.2).all()
    assert d["intr0"][0, 0, 0] == 1475 and d["intr0"][0, 0, 2] == 960 and d["intr0"][0, 1, 2] == 540


def test_conv_config_knob_validates_on_the_host():
    """ap_set_conv_config is host-only state: every documented value is accepted, anything else is refused with AP_EINVAL
    and leaves the automatic choice in place (no GPU needed)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    ok = [-1, -4, -5, 100, 17] + list(range(0, 15))
    try:
        for c in ok:
            assert L.ap_set_conv_config(c) == 0, c
        for c in (-2, -3, -6, 15, 16, 18, 19, 20, 24, 28, 99, 101):
            assert L.ap_set_conv_config(c) != 0, c
    finally:
        assert L.ap_set_conv_config(-1) == 0


def test_range_hook_entries_validate_on_the_host():
    """ap_debug_set_range_hook / ap_debug_range_status (ABI 12): declared, bound and exported; off is the default and needs no GPU;
    with the hook off the status is AP_OK for every precision without touching a stream, and a bad precision is AP_EINVAL."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    assert Nn.ABI_VERSION >= 12 and L.ap_abi_version() >= 12
    for name in ("ap_debug_set_range_hook", "ap_debug_range_status"):
        assert name in _declared() and name in Nn.SIGNATURES and hasattr(L, name)
    assert Nn.SIGNATURES["ap_debug_set_range_hook"][1] == [ctypes.c_int]
    assert Nn.SIGNATURES["ap_debug_range_status"][1] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    assert L.ap_debug_set_range_hook(0) == 0
    for prec in sorted(Nn.PRECISIONS.values()):
        for reset in (0, 1):
            assert L.ap_debug_range_status(prec, None, reset) == 0, prec
    for prec in (-1, 4, 7):
        assert L.ap_debug_range_status(prec, None, 0) == -1, prec
    hdr = open(os.path.join(REPO, "include", "airpose_hip.h")).read()
    assert "sentinel is not connected" not in hdr


def test_trunk_form_entries_check_their_arguments():
    """ABI 13: ap_conv2d_tiled_nhwc / _fold_nhwc / _pool_nhwc and ap_conv_pair_layout_nhwc refuse NULL pointers, a bad precision and
    every shape or layout combination the header lists, before any launch (host only: no GPU needed)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    assert Nn.ABI_VERSION == 13 and L.ap_abi_version() == 13
    one = ctypes.c_void_p(256)
    BF, F16, F32, X2 = Nn.AP_PREC_BF16, Nn.AP_PREC_F16, Nn.AP_PREC_FP32, Nn.AP_PREC_BF16X2
    EINVAL, ESHAPE = -1, -2

    def tiled(prec=BF, x=one, w=one, s=one, h=one, y=one, N=1, H=5, W=5, Cin=64, Cout=8, k=3, st=1, pad=1):
        return L.ap_conv2d_tiled_nhwc(prec, x, w, s, h, None, y, N, H, W, Cin, Cout, k, st, pad, 1, None)
    for kw in (dict(prec=7), dict(prec=-1), dict(x=None), dict(w=None), dict(s=None), dict(h=None), dict(y=None), dict(N=0), dict(H=0), dict(k=0),
               dict(st=0), dict(pad=-1)):
        assert tiled(**kw) == EINVAL, kw
    for kw in (dict(Cin=32), dict(Cin=0), dict(Cout=12), dict(prec=F32, Cin=48), dict(prec=F32, Cout=6), dict(H=1, k=5, pad=0)):
        assert tiled(**kw) == ESHAPE, kw

    def fold(prec=BF, t=one, x2=one, w=one, s=one, h=one, y=one, N=1, Ho=7, H2=14, Cin=64, Cin2=64, Cout=8, s2=2):
        return L.ap_conv2d_fold_nhwc(prec, t, x2, w, s, h, None, y, N, Ho, H2, Cin, Cin2, Cout, s2, 1, None)
    for kw in (dict(prec=4), dict(t=None), dict(x2=None), dict(w=None), dict(s=None), dict(h=None), dict(y=None), dict(N=0), dict(Ho=0), dict(H2=0),
               dict(s2=0), dict(s2=3)):
        assert fold(**kw) == EINVAL, kw
    for kw in (dict(Cin=32), dict(Cin2=96), dict(Cin2=0), dict(Cout=4), dict(prec=F32, Cin2=16), dict(H2=12), dict(H2=15), dict(s2=1),
               dict(Ho=7, H2=8, s2=1)):
        assert fold(**kw) == ESHAPE, kw                      # (H2 = 13 and 14 are the two sizes stride 2 maps to Ho = 7; stride 1: H2 = Ho)

    # what the configuration cannot run is found before any launch as well: the explicit ones, and the two the AUTOMATIC choice makes
    big = dict(N=16, H=56, W=56, Cin=64, Cout=256, k=1, st=1, pad=0)     # 1 x 1 on 784 tiles of 128 x 128: conv_lean (17) under -1
    fbig = dict(N=11, Ho=56, H2=56, s2=1, Cout=64)                        # Cout <= 64 on 270 rows of tiles: the 64-wide tile 12 under -1
    try:
        assert tiled(**big) == ESHAPE and b"fragment-tiled" in L.ap_last_error()
        assert tiled(prec=F32) == ESHAPE and tiled(prec=X2, Cin=32) == ESHAPE
        assert fold(**fbig) == ESHAPE and b"64-wide" in L.ap_last_error()
        assert fold(N=512, Ho=64, H2=128, Cin2=256, Cout=136) == ESHAPE and b"4 GiB" in L.ap_last_error()
        for cfg in (4, 5, 6, 7, 17):
            assert L.ap_set_conv_config(cfg) == 0 and tiled() == ESHAPE, cfg
        for cfg in (2, 3, 6, 7, 9, 12, 13):
            assert L.ap_set_conv_config(cfg) == 0 and fold() == ESHAPE and fold(prec=F32, Cin=32, Cin2=32, Cout=4) == ESHAPE, cfg
        for cfg in (0, 1, 5, 8, 10, 13):
            assert L.ap_set_conv_config(cfg) == 0 and fold(prec=X2) == ESHAPE and b"split-bf16" in L.ap_last_error(), cfg
    finally:
        assert L.ap_set_conv_config(-1) == 0

    def pool(prec=BF, x=one, w=one, s=one, h=one, res=one, out=one, N=1, Cin=64, Cout=256):
        return L.ap_conv2d_pool_nhwc(prec, x, w, s, h, res, out, N, Cin, Cout, None)
    for kw in (dict(prec=5), dict(x=None), dict(w=None), dict(s=None), dict(h=None), dict(res=None), dict(out=None), dict(N=0)):
        assert pool(**kw) == EINVAL, kw
    for kw in (dict(prec=F32), dict(prec=X2), dict(Cin=48), dict(Cin=0), dict(Cout=12), dict(Cout=0), dict(prec=F16, Cin=16), dict(Cin=32),
               dict(Cin=96)):
        assert pool(**kw) == ESHAPE, kw                      # never a silent y: what the pooling kernel does not take is refused

    def pair(prec=BF, t2=one, inp=one, ws=one, s3=one, h3=one, s1=one, h1=one, out=one, t1n=one, N=1, Ho=7, P=128, P2=0, st=2, N1=128,
             lay=(0, 0, 0, 0)):
        return L.ap_conv_pair_layout_nhwc(prec, t2, inp, ws, s3, h3, s1, h1, out, t1n, N, Ho, P, P2, st, N1, lay[0], lay[1], lay[2], lay[3], None)
    for kw in (dict(prec=F32), dict(prec=X2), dict(prec=9), dict(t2=None), dict(inp=None), dict(ws=None), dict(s3=None), dict(h3=None), dict(out=None),
               dict(s1=None), dict(h1=None), dict(t1n=None), dict(N=0), dict(Ho=0)):
        assert pair(**kw) == EINVAL, kw
    for kw in (dict(P=64), dict(N1=64), dict(P2=256, N1=256), dict(P2=256, st=3), dict(P2=256, st=0), dict(P=256, P2=512, N1=128),
               dict(P2=256, lay=(0, 1, 0, 0)), dict(lay=(0, 0, 1, 1)), dict(lay=(1, 1, 1, 1)), dict(P=256, P2=512, N1=0, lay=(0, 0, 0, 1))):
        assert pair(**kw) == ESHAPE, kw
    assert b"ap_conv_pair_layout_nhwc" in L.ap_last_error()


def test_one_library_carries_both_16bit_storage_types():
    """AP_PREC_F16 is a precision of the ONE library (no second .so, no flavour switch): the enum values are distinct, the
    f16 kernel set (namespace k_f16) is linked in, and the host-only entry points validate the precision argument."""
    import subprocess
    from airpose_amd import _native as Nn
    assert sorted(Nn.PRECISIONS.values()) == [0, 1, 2, 3] and Nn.PRECISIONS["f16"] == 3 and Nn.PRECISIONS["bf16"] == 1
    assert not os.path.exists(os.path.join(REPO, "airpose_amd", "libairpose_hip_f16.so"))
    syms = subprocess.run(["nm", "-D", "--defined-only", Nn.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for ns in ("k_bf16", "k_f16"):
        for fn in ("ap_launch_conv_pipe", "ap_launch_conv_pair", "ap_launch_bneck2", "ap_launch_stem_pool", "ap_launch_conv_slab"):
            assert re.search(r"_ZN%d%s\d+%s" % (len(ns), ns, fn), syms), (ns, fn)
    L = Nn.lib()
    # pair-stream size: a host-only query; unsupported shapes are refused
    assert L.ap_conv_pair_stream_bytes(128, 0, 128) > 0 and L.ap_conv_pair_stream_bytes(256, 512, 0) > 0
    assert L.ap_conv_pair_stream_bytes(64, 0, 64) < 0
    # the stand-alone 16-bit operators take AP_PREC_BF16 / AP_PREC_F16 only (argument check comes before any launch)
    assert L.ap_conv_pair_pack(Nn.AP_PREC_FP32, None, None, 128, 0, 128, None, None) == -1
    assert L.ap_net_range_status(None, None, 0) == -1 and L.ap_net_set_range_check(None, 1) == -1


def test_host_layer_exports_the_header_and_nothing_internal():
    """The host layer is several translation units (csrc/api_*.hip) that share helpers through namespace ap_internal (hidden
    visibility, csrc/api_internal.h): none of those may reach the dynamic symbol table, and the C names the library defines are
    exactly the functions include/airpose_hip.h declares."""
    import subprocess
    from airpose_amd import _native as Nn
    out = subprocess.run(["nm", "-D", "--defined-only", Nn.LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert len(syms) >= 99
    assert [s for s in syms if "ap_internal" in s] == []
    assert sorted(s for s in syms if s.startswith("ap_")) == _declared()


def test_bench_launches_itself_for_n_gpus():
    """`python bench.py --gpus 2` with no launcher environment (the shape of the driver's plain command) must start its own ranks
    (it used to die with SystemExit before touching a GPU).  AIRPOSE_BENCH_LAUNCH_ONLY=1 stops each rank where the GPU
    would be needed: self-launch through torch.distributed.run, gloo rendezvous on 127.0.0.1, one all_reduce, ONE JSON line."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["AIRPOSE_BENCH_LAUNCH_ONLY"] = "1"
    env["OMP_NUM_THREADS"] = "1"
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["launcher"] == "ok" and rec["n_gpus"] == 2 and rec["n_ranks_seen"] == 2
    # and a launcher that started another number of ranks than --gpus names is refused loudly
    env2 = dict(env, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    bad = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"], env=env2, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "WORLD_SIZE=3" in (bad.stderr + bad.stdout)
