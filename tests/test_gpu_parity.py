"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle and the committed
golden vectors.  Need a real MI355X:  python -m pytest tests -m gpu

Tolerances (written here, as the scope demands):
  fp32 parity mode   1e-4 relative (max |a-b| / max |b|) on regressed theta/beta, 3-D joints/vertices, 2-D
                     projection -- the bar of BASELINE.json north_star
  bf16 throughput    reported; asserted < 5e-2 (bf16 storage has 8 mantissa bits through 53 convs)
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS, elem_err, key_errs, pose_rel_errs, rel_err

pytestmark = pytest.mark.gpu

TOL32 = 1e-4
TOLBF = 5e-2


def pose_err(a, b):
    """worst per-slice error of a pose vector (translation and 6-D rotation normalised separately)"""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else b
    return max(pose_rel_errs(a, b).values())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def net32(copenet_sd, dev):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    return net


@pytest.fixture(scope="module")
def netbf(copenet_sd, dev):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="bf16").eval()
    net.load_state_dict(copenet_sd)
    return net


@pytest.fixture(scope="module")
def netf16(copenet_sd, dev):
    """The throughput kernels with fp16 storage (AP_PREC_F16; the library's default precision)."""
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    net.load_state_dict(copenet_sd)
    return net


@pytest.fixture(scope="module", params=["bf16", "f16"])
def net16(request, netbf, netf16):
    """Both 16-bit storage types of the throughput kernels (same sources, two kernel sets of the one library)."""
    return netbf if request.param == "bf16" else netf16


H16 = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def netx2(copenet_sd, dev):
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="bf16x2").eval()
    net.load_state_dict(copenet_sd)
    return net


@pytest.fixture(scope="module")
def body(smplx_model, dev):
    from airpose_amd import smplx
    return smplx.SMPLX(model_data=smplx_model)


def test_native_library_is_loaded():
    from airpose_amd import _native
    L = _native.lib()
    assert b"gfx950" in L.ap_version()
    with open("/proc/self/maps") as f:
        assert "libairpose_hip.so" in f.read()


# ------------------------------------------------------------------------------------------------ conv primitive
def _split_parts(t):
    """fp32 tensor -> (bf16 hi, bf16 lo, the fp32 values hi + lo they stand for): the bf16x2 representation"""
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi, lo, hi.float() + lo.float()


def _split_pack(t):
    """fp32 tensor (channels last, C % 8 == 0) -> (int32 tensor of the same shape in the bf16x2 storage layout: every
    group of 8 channels = 32 bytes = 8 bf16 hi parts | 8 bf16 lo parts;  the fp32 values it stands for)"""
    hi, lo, val = _split_parts(t)
    C = t.shape[-1]
    assert C % 8 == 0
    g = torch.stack([hi.reshape(*t.shape[:-1], C // 8, 8), lo.reshape(*t.shape[:-1], C // 8, 8)], dim=-2)  # (.., C/8, 2, 8) bf16
    return g.contiguous().view(torch.int32).reshape(*t.shape[:-1], C), val


def _split_unpack(word):
    """inverse of _split_pack: int32 (.., C) in the bf16x2 layout -> fp32 (.., C)"""
    C = word.shape[-1]
    g = word.contiguous().view(torch.bfloat16).reshape(*word.shape[:-1], C // 8, 2, 8).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*word.shape[:-1], C)


def _conv_case(dev, prec, N, H, Cin, Cout, k, stride, pad, relu, use_res, seed):
    if prec == "bf16x2":
        return _conv_case_split(dev, N, H, Cin, Cout, k, stride, pad, relu, use_res, seed)
    from airpose_amd import _native as Nn
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (k * k * Cin)) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    Ho = (H + 2 * pad - k) // stride + 1
    res = torch.randn(N, Cout, Ho, Ho, generator=g) if use_res else None
    tdt = H16.get(prec, torch.float32)
    xq, wq = x.to(tdt), w.to(tdt)
    resq = res.to(tdt) if use_res else None
    # oracle on the SAME (rounded) operands, fp64 accumulate
    ref = F.conv2d(xq.double(), wq.double(), stride=stride, padding=pad)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if use_res:
        ref = ref + resq.double()
    if relu:
        ref = ref.clamp_min(0)
    cpad = (Cout + 127) // 128 * 128
    wp = torch.zeros(cpad, k, k, Cin, dtype=tdt)
    wp[:Cout] = wq.permute(0, 2, 3, 1)
    sp, hp = torch.ones(cpad), torch.zeros(cpad)
    sp[:Cout], hp[:Cout] = scale, shift
    xd = xq.permute(0, 2, 3, 1).contiguous().to(dev)
    rd = resq.permute(0, 2, 3, 1).contiguous().to(dev) if use_res else None
    wd, sd_, hd = wp.to(dev), sp.to(dev), hp.to(dev)
    y = torch.full((N, Ho, Ho, Cout), float("nan"), dtype=tdt, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = Nn.lib().ap_conv2d_nhwc(Nn.PRECISIONS[prec], p(xd), p(wd), p(sd_), p(hd), p(rd), p(y), N, H, H, Cin, Cout, k,
                                 stride, pad, int(relu), Nn.stream_ptr(dev))
    Nn.check(rc, "ap_conv2d_nhwc")
    torch.cuda.synchronize()
    got = y.float().cpu().permute(0, 3, 1, 2).double()
    return got, ref


def _conv_case_split(dev, N, H, Cin, Cout, k, stride, pad, relu, use_res, seed):
    """ap_conv2d_nhwc in split-bf16 storage: operands and residual are (hi, lo) bf16 parts in planar groups of 8 channels;
    the fp64 oracle runs on the values they stand for, so what is tested is the three-term product on the bf16 matrix
    pipe + fp32 accumulate (the dropped lo*lo term is 2^-18 relative) and the 2^-17 rounding of the stored result."""
    from airpose_amd import _native as Nn
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (k * k * Cin)) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    Ho = (H + 2 * pad - k) // stride + 1
    xw, xq = _split_pack(x.permute(0, 2, 3, 1).contiguous())            # NHWC
    ww, wq = _split_pack(w.permute(0, 2, 3, 1).contiguous())            # [Cout][kh][kw][Cin]
    ref = F.conv2d(xq.permute(0, 3, 1, 2).double(), wq.permute(0, 3, 1, 2).double(), stride=stride, padding=pad)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    rd = None
    if use_res:
        rw, rq = _split_pack(torch.randn(N, Ho, Ho, Cout, generator=g))
        ref = ref + rq.permute(0, 3, 1, 2).double()
        rd = rw.to(dev)
    if relu:
        ref = ref.clamp_min(0)
    cpad = (Cout + 127) // 128 * 128
    wp = torch.zeros(cpad, k, k, Cin, dtype=torch.int32)
    wp[:Cout] = ww
    sp, hp = torch.ones(cpad), torch.zeros(cpad)
    sp[:Cout], hp[:Cout] = scale, shift
    xd = xw.to(dev)
    wd, sd_, hd = wp.to(dev), sp.to(dev), hp.to(dev)
    y = torch.full((N, Ho, Ho, Cout), 0x7fc07fc0, dtype=torch.int32, device=dev)      # NaN | NaN
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = Nn.lib().ap_conv2d_nhwc(Nn.PRECISIONS["bf16x2"], p(xd), p(wd), p(sd_), p(hd), p(rd), p(y), N, H, H, Cin, Cout, k,
                                 stride, pad, int(relu), Nn.stream_ptr(dev))
    Nn.check(rc, "ap_conv2d_nhwc")
    torch.cuda.synchronize()
    got = _split_unpack(y.cpu()).permute(0, 3, 1, 2).double()
    return got, ref


CONV_CASES = [
    # N, H, Cin, Cout, k, stride, pad, relu, res
    (2, 56, 64, 64, 1, 1, 0, True, False),      # layer1 conv1: single K step, BN=64 tile
    (2, 56, 64, 64, 3, 1, 1, True, False),      # layer1 conv2: 3x3 halo
    (2, 56, 64, 256, 1, 1, 0, True, True),      # conv3 + residual + relu
    (1, 56, 256, 128, 1, 1, 0, True, False),
    (2, 56, 128, 128, 3, 2, 1, True, False),    # stride-2 3x3 (layer2.0 conv2)
    (2, 56, 256, 512, 1, 2, 0, False, False),   # stride-2 1x1 downsample, no relu
    (3, 14, 256, 256, 3, 1, 1, True, False),    # ragged M (3*196 = 588)
    (1, 7, 512, 2048, 1, 1, 0, True, True),     # tiny M = 49, wide N
    (5, 7, 512, 512, 3, 1, 1, True, False),     # K = 4608
    (64, 28, 128, 512, 1, 1, 0, True, True),    # large M -> 128x128 tiles
]


# -1 = automatic choice; 0..3 = LDS-DMA pipelined kernel (256x128, 128x128, 128x64, 256x64 tiles), 4..7 = the same
# with the register epilogue; 8..13 = 2-stage rings with 4 or 8 waves; 100 = register-staged kernel
ALL_CFGS = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 17, 100]
F16_CFGS = [-1, 1, 11, 12, 14, 17, 100]       # fp16 storage: the automatic choice, the kernels it picks (11 ring, 12, 14 slab, 17 lean,
                                              # 100 register-staged) and a 4-wave 4-stage ring; the bf16 set runs the whole sweep


@pytest.mark.parametrize("prec,cfg", [(pr, c) for pr in ("fp32", "bf16") for c in ALL_CFGS] + [("f16", c) for c in F16_CFGS])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_primitive(dev, prec, case, cfg):
    from airpose_amd import _native as Nn
    N, H, Cin, Cout, k, stride, pad, relu, use_res = case
    Nn.check(Nn.lib().ap_set_conv_config(cfg), "ap_set_conv_config")
    try:
        got, ref = _conv_case(dev, prec, N, H, Cin, Cout, k, stride, pad, relu, use_res, seed=hash(case) % 10000)
    finally:
        Nn.lib().ap_set_conv_config(-1)
    assert torch.isfinite(got).all()
    # operands identical: fp32 differs only by accumulation order, bf16 additionally by the output rounding
    tol = {"fp32": 2e-5, "bf16": 6e-3, "f16": 8e-4}[prec]
    assert rel_err(got.numpy(), ref.numpy()) < tol


PAIR_CASES = [
    # images, H, P (planes), N1 (next block's conv1 width)
    (2, 28, 128, 128),      # layer2 identity block -> next layer2 block; M = 1568 (ragged: 24.5 tiles of 64 pixels)
    (3, 28, 128, 256),      # layer2.3 -> layer3.0 (conv1 of the stage-first block runs before the stride)
    (5, 14, 256, 256),      # layer3 identity pair; M = 980 (ragged)
    (1, 7, 128, 128),       # M = 49: a single, partly empty tile
]


def _pair_stream(dev, prec, w3, w1, P, P2, N1):
    """The caller-owned weight stream of the fused pair kernel (ap_conv_pair_pack) for w3 [4P][P + P2], w1 [N1][4P]."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    nb = L.ap_conv_pair_stream_bytes(P, P2, N1)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    Nn.check(L.ap_conv_pair_pack(Nn.PRECISIONS[prec], p(w3), p(w1) if N1 else None, P, P2, N1, p(ws), Nn.stream_ptr(dev)),
             "ap_conv_pair_pack")
    return ws


def _pair_case(dev, n, H, P, N1, seed, prec="bf16"):
    """Operands of one fused pair: t2, identity x, conv3 / conv1 weights and BatchNorm constants (16-bit tensors on `dev`)."""
    g = torch.Generator().manual_seed(seed)
    M, C3 = n * H * H, 4 * P
    bf = H16[prec]
    t2 = torch.randn(M, P, generator=g).clamp_min(0).to(bf)
    x = torch.randn(M, C3, generator=g).clamp_min(0).to(bf)
    w3 = (torch.randn(C3, P, generator=g) * (2.0 / P) ** 0.5).to(bf)
    w1 = (torch.randn(N1, C3, generator=g) * (2.0 / C3) ** 0.5).to(bf)
    s3, h3 = torch.rand(C3, generator=g) + 0.5, torch.randn(C3, generator=g) * 0.1
    s1, h1 = torch.rand(N1, generator=g) + 0.5, torch.randn(N1, generator=g) * 0.1
    return [t.to(dev) for t in (t2, x, w3, w1, s3, h3, s1, h1)]


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("case", PAIR_CASES)
def test_conv_pair_equals_two_convs_and_fp64(dev, case, prec):
    """conv_pair.hip: conv3 (+ identity, ReLU) of a block and conv1 of the next block in one kernel.  Bit-identical to the two
    stand-alone launches (same K order, same k-slot assignment, same epilogue expression), the block output against an fp64
    evaluation on identical operands, and rows beyond M untouched (ragged last tile)."""
    from airpose_amd import _native as Nn
    n, H, P, N1 = case
    L = Nn.lib()
    M, C3 = n * H * H, 4 * P
    t2, x, w3, w1, s3, h3, s1, h1 = _pair_case(dev, n, H, P, N1, seed=100 + P + N1 + H, prec=prec)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    PR, bf = Nn.PRECISIONS[prec], H16[prec]
    ws = _pair_stream(dev, prec, w3, w1, P, 0, N1)
    guard = 8                                                # rows behind M must stay as they were
    out = torch.full((M + guard, C3), float("nan"), dtype=bf, device=dev)
    t1n = torch.full((M + guard, N1), float("nan"), dtype=bf, device=dev)
    Nn.check(L.ap_conv_pair_nhwc(PR, p(t2), p(ws), p(s3), p(h3), p(x), p(s1), p(h1), p(out), p(t1n), M, P, N1,
                                 Nn.stream_ptr(dev)), "ap_conv_pair_nhwc")
    torch.cuda.synchronize()
    assert torch.isnan(out[M:].float()).all() and torch.isnan(t1n[M:].float()).all()
    # the two stand-alone launches (ring kernel, configuration 11)
    ref_out = torch.empty(M, C3, dtype=bf, device=dev)
    ref_t1 = torch.empty(M, N1, dtype=bf, device=dev)
    L.ap_set_conv_config(11)
    try:
        Nn.check(L.ap_conv2d_nhwc(PR, p(t2), p(w3), p(s3), p(h3), p(x), p(ref_out), n, H, H, P, C3, 1, 1, 0, 1,
                                  Nn.stream_ptr(dev)), "conv3")
        Nn.check(L.ap_conv2d_nhwc(PR, p(ref_out), p(w1), p(s1), p(h1), None, p(ref_t1), n, H, H, C3, N1, 1, 1, 0, 1,
                                  Nn.stream_ptr(dev)), "conv1")
        torch.cuda.synchronize()
    finally:
        L.ap_set_conv_config(-1)
    assert torch.equal(out[:M], ref_out)
    assert torch.equal(t1n[:M], ref_t1)
    # fp64 on identical operands
    want = (t2.double() @ w3.double().T) * s3.double() + h3.double() + x.double()
    want = want.clamp_min(0)
    tol = 6e-3 if prec == "bf16" else 8e-4
    assert rel_err(out[:M].double().cpu().numpy(), want.cpu().numpy()) < tol
    want1 = ((out[:M].double() @ w1.double().T) * s1.double() + h1.double()).clamp_min(0)
    assert rel_err(t1n[:M].double().cpu().numpy(), want1.cpu().numpy()) < tol


def test_conv_pair_stream_is_caller_owned(dev):
    """The library keeps no copy of a pair's weights keyed by their ADDRESS (an allocator reuses addresses): new
    contents at the same addresses, re-packed into the same stream buffer, give the new result."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    n, H, P, N1 = 2, 14, 256, 256
    M, C3 = n * H * H, 4 * P
    t2, x, w3, w1, s3, h3, s1, h1 = _pair_case(dev, n, H, P, N1, seed=3)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    PR = Nn.PRECISIONS["bf16"]
    outs = []
    ws = None
    for rnd in range(2):
        if rnd:                                              # same tensors, same addresses, new contents
            w3.copy_(w3.flip(0))
            w1.mul_(-1.0)
        if ws is None:
            ws = _pair_stream(dev, "bf16", w3, w1, P, 0, N1)
        else:
            Nn.check(L.ap_conv_pair_pack(PR, p(w3), p(w1), P, 0, N1, p(ws), Nn.stream_ptr(dev)), "ap_conv_pair_pack")
        out = torch.empty(M, C3, dtype=torch.bfloat16, device=dev)
        t1n = torch.empty(M, N1, dtype=torch.bfloat16, device=dev)
        Nn.check(L.ap_conv_pair_nhwc(PR, p(t2), p(ws), p(s3), p(h3), p(x), p(s1), p(h1), p(out), p(t1n), M, P, N1,
                                     Nn.stream_ptr(dev)), "ap_conv_pair_nhwc")
        ref = torch.empty(M, C3, dtype=torch.bfloat16, device=dev)
        Nn.check(L.ap_conv2d_nhwc(PR, p(t2), p(w3), p(s3), p(h3), p(x), p(ref), n, H, H, P, C3, 1, 1, 0, 1, Nn.stream_ptr(dev)), "conv3")
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("case", [(3, 28, 128, 256, 128), (5, 14, 256, 512, 0), (1, 28, 128, 256, 128)])
def test_conv_pair_stage_first_block_matches_fp64(dev, case, prec):
    """conv_pair.hip on a stage's first block: conv3 with the downsample branch as a second K segment (the block input read at
    the stride-2 pixel), ReLU, and -- layer2.0 -- the next block's conv1 from the registers; against fp64 on identical operands."""
    from airpose_amd import _native as Nn
    n, Ho, P, P2, N1 = case
    L = Nn.lib()
    g = torch.Generator().manual_seed(7 + P + n)
    H2, C3, M = 2 * Ho, 4 * P, n * Ho * Ho
    bf = H16[prec]
    t2 = torch.randn(M, P, generator=g).clamp_min(0).to(bf)
    x = torch.randn(n, H2, H2, P2, generator=g).clamp_min(0).to(bf)
    w3d = (torch.randn(C3, P + P2, generator=g) * (1.0 / (P + P2)) ** 0.5).to(bf)
    h3 = torch.randn(C3, generator=g) * 0.1
    w1 = (torch.randn(max(N1, 128), C3, generator=g) * (2.0 / C3) ** 0.5).to(bf)
    s1, h1 = torch.rand(max(N1, 128), generator=g) + 0.5, torch.randn(max(N1, 128), generator=g) * 0.1
    ones = torch.ones(C3)                                    # the BatchNorm scales are folded into w3d (pack_c3_ds)
    d = lambda t: t.to(dev)
    t2, x, w3d, h3, w1, s1, h1, ones = map(d, (t2, x, w3d, h3, w1, s1, h1, ones))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = _pair_stream(dev, prec, w3d, w1[:N1].contiguous() if N1 else None, P, P2, N1)
    out = torch.full((M + 8, C3), float("nan"), dtype=bf, device=dev)
    t1n = torch.full((M + 8, max(N1, 1)), float("nan"), dtype=bf, device=dev)
    Nn.check(L.ap_conv_pair_ds_nhwc(Nn.PRECISIONS[prec], p(t2), p(x), p(ws), p(ones), p(h3), p(s1) if N1 else None, p(h1) if N1 else None,
                                    p(out), p(t1n) if N1 else None, n, Ho, P, P2, 2, N1, Nn.stream_ptr(dev)), "ap_conv_pair_ds_nhwc")
    torch.cuda.synchronize()
    assert torch.isnan(out[M:].float()).all()
    xs = x[:, ::2, ::2, :].reshape(M, P2)                       # the strided pixels of the block input
    want = (torch.cat([t2, xs], 1).double() @ w3d.double().T + h3.double()).clamp_min(0)
    tol = 6e-3 if prec == "bf16" else 8e-4
    assert rel_err(out[:M].double().cpu().numpy(), want.cpu().numpy()) < tol
    if N1:
        assert torch.isnan(t1n[M:].float()).all()
        want1 = ((out[:M].double() @ w1[:N1].double().T) * s1[:N1].double() + h1[:N1].double()).clamp_min(0)
        assert rel_err(t1n[:M].double().cpu().numpy(), want1.cpu().numpy()) < tol


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_pair_full_size_is_deterministic(dev, prec):
    """BASELINE-size layer3 pair (256 images: 50 176 pixels, 784 workgroups on 512 slots, hand-counted waits under full
    memory load): repeated runs identical, equal to the two stand-alone kernels."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    n, H, P, N1 = 256, 14, 256, 256
    M, C3 = n * H * H, 4 * P
    t2, x, w3, w1, s3, h3, s1, h1 = _pair_case(dev, n, H, P, N1, seed=5, prec=prec)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    PR, bf = Nn.PRECISIONS[prec], H16[prec]
    ws = _pair_stream(dev, prec, w3, w1, P, 0, N1)
    outs = []
    for _ in range(3):
        out = torch.full((M, C3), float("nan"), dtype=bf, device=dev)
        t1n = torch.full((M, N1), float("nan"), dtype=bf, device=dev)
        Nn.check(L.ap_conv_pair_nhwc(PR, p(t2), p(ws), p(s3), p(h3), p(x), p(s1), p(h1), p(out), p(t1n), M, P, N1,
                                     Nn.stream_ptr(dev)), "ap_conv_pair_nhwc")
        torch.cuda.synchronize()
        outs.append((out, t1n))
    ref_out = torch.empty(M, C3, dtype=bf, device=dev)
    ref_t1 = torch.empty(M, N1, dtype=bf, device=dev)
    Nn.check(L.ap_conv2d_nhwc(PR, p(t2), p(w3), p(s3), p(h3), p(x), p(ref_out), n, H, H, P, C3, 1, 1, 0, 1,
                              Nn.stream_ptr(dev)), "conv3")
    Nn.check(L.ap_conv2d_nhwc(PR, p(ref_out), p(w1), p(s1), p(h1), None, p(ref_t1), n, H, H, C3, N1, 1, 1, 0, 1,
                              Nn.stream_ptr(dev)), "conv1")
    torch.cuda.synchronize()
    for o, t in outs:
        assert torch.equal(o, ref_out) and torch.equal(t, ref_t1)


def test_trunk_with_and_without_fused_pairs_bitwise(net16, dev):
    netbf = net16
    """The trunk with the fused conv3 -> conv1 pairs (layer2 / layer3 identity blocks, layer2 -> layer3) against the same
    trunk with one convolution per launch: identical features, bit for bit; 6 images make every pair's pixel count ragged."""
    gen = torch.Generator(device="cpu").manual_seed(23)
    x = torch.randn(6, 3, 224, 224, generator=gen).to(dev)
    feats = []
    try:
        for on in (0, 1, 1):
            netbf.set_fuse_pair(on)
            feats.append(netbf.forward_feat_ext(x).clone())
    finally:
        netbf.set_fuse_pair(1)
    assert torch.isfinite(feats[0]).all()
    assert torch.equal(feats[0], feats[1]) and torch.equal(feats[1], feats[2])


@pytest.mark.parametrize("cfg", [-1, 11, 12, 100])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_primitive_split_bf16(dev, case, cfg):
    """bf16x2 storage (the fast parity mode): every product = hi*hi + hi*lo + lo*hi on the bf16 matrix pipe.
    Against the fp64 oracle on the values the pairs stand for; the bar is that of the fp32 kernel plus the 2^-17
    rounding of the stored result."""
    from airpose_amd import _native as Nn
    N, H, Cin, Cout, k, stride, pad, relu, use_res = case
    Nn.check(Nn.lib().ap_set_conv_config(cfg), "ap_set_conv_config")
    try:
        got, ref = _conv_case(dev, "bf16x2", N, H, Cin, Cout, k, stride, pad, relu, use_res, seed=hash(case) % 10000)
    finally:
        Nn.lib().ap_set_conv_config(-1)
    assert torch.isfinite(got).all()
    e = rel_err(got.numpy(), ref.numpy())
    print("split-bf16 conv rel err %.3e" % e)
    assert e < 3e-5


def test_split_bf16_configs_agree_bitwise(dev):
    from airpose_amd import _native as Nn
    outs = []
    for cfg in (11, 12, 100):
        Nn.lib().ap_set_conv_config(cfg)
        try:
            got, _ = _conv_case(dev, "bf16x2", 3, 28, 128, 192, 3, 1, 1, True, True, seed=5)
        finally:
            Nn.lib().ap_set_conv_config(-1)
        outs.append(got)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


@pytest.mark.parametrize("B", [63, 64, 65, 128])
def test_two_stream_trunk_is_bit_identical_to_single_pass(netbf, net32, dev, B):
    """Two-view forwards of >= 64 pairs run the two views as two concurrent trunk passes on two internal streams
    (fork / join on the caller's stream).  Same kernels on the same rows: bit-identical to the single pass over the
    concatenated views, in both storage types, and repeatable (no race on the per-pass workspaces).  B = 63 / 64 / 65
    straddle the switch (trunk_fwd: n0 >= 64 && n1 >= 64; 64 pairs = BASELINE config 2's batch): below it the knob
    must change nothing, at and above it the two routes must agree bit for bit."""
    gen = torch.Generator(device="cpu").manual_seed(31)
    x0, x1 = torch.randn(B, 3, 224, 224, generator=gen).to(dev), torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    bb0, bb1 = torch.rand(B, 3, generator=gen).to(dev), torch.rand(B, 3, generator=gen).to(dev)
    pos = torch.tensor([0.0, 0.0, 0.5], device=dev).expand(B, 3).contiguous()
    nets = (netbf, net32) if B == 128 else (netbf,)
    for net in nets:
        try:
            net.set_dual_stream(0)
            one = [t.clone() for t in net(x0, x1, bb0, bb1, pos, pos, iters=3)]
            net.set_dual_stream(1)
            for _ in range(3):
                two = net(x0, x1, bb0, bb1, pos, pos, iters=3)
                torch.cuda.synchronize()
                for a, b in zip(one, two):
                    assert torch.equal(a, b)
        finally:
            net.set_dual_stream(1)
    # work submitted to the caller's stream after the forward sees its results (the join is on that stream)
    netbf.set_dual_stream(0)
    ref = netbf(x0, x1, bb0, bb1, pos, pos, iters=3)[0].clone()
    netbf.set_dual_stream(1)
    torch.cuda.synchronize()                                 # one in-flight call per handle: the side stream does not wait for this one
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p0 = netbf(x0, x1, bb0, bb1, pos, pos, iters=3)[0]
        chk = p0.sum()
    side.synchronize()
    assert torch.isfinite(chk) and torch.equal(p0, ref)


def test_conv_configs_agree_bitwise(dev):
    """Every tile configuration accumulates each output element in the same K order."""
    from airpose_amd import _native as Nn
    outs = []
    for cfg in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 100):
        Nn.lib().ap_set_conv_config(cfg)
        try:
            got, _ = _conv_case(dev, "bf16", 3, 28, 128, 192, 3, 1, 1, True, True, seed=5)
        finally:
            Nn.lib().ap_set_conv_config(-1)
        outs.append(got)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


# ------------------------------------------------------------------------------------------------ fused bottleneck
def _bneck_case(dev, N, H, ds, seed, W=None, prec="bf16"):
    """Bottleneck.forward (model_copenet.py:27-47) for planes = 64 on bf16 operands: fp64 oracle that rounds the two
    64-channel intermediates to bf16 exactly where the kernel (and the three-convolution path) does."""
    from airpose_amd import _native as Nn
    g = torch.Generator().manual_seed(seed)
    cin = 64 if ds else 256
    bf = H16[prec]
    W = H if W is None else W
    x = torch.randn(N, cin, H, W, generator=g).to(bf)
    w1 = (torch.randn(64, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5).to(bf)
    w2 = (torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5).to(bf)
    w3 = (torch.randn(256, 64, 1, 1, generator=g) * (2.0 / 64) ** 0.5).to(bf)
    wd = (torch.randn(256, 64, 1, 1, generator=g) * (2.0 / 64) ** 0.5).to(bf)       # folded downsample columns
    sc = [torch.rand(c, generator=g) + 0.5 for c in (64, 64, 256)]
    sh = [torch.randn(c, generator=g) * 0.1 for c in (64, 64, 256)]
    if ds:
        sc[2] = torch.ones(256)                 # pack_c3_ds folds the BN scales into the weights
    bn = lambda t, i: t * sc[i].double().view(1, -1, 1, 1) + sh[i].double().view(1, -1, 1, 1)
    m1 = bn(F.conv2d(x.double(), w1.double()), 0).clamp_min(0).to(bf)
    m2 = bn(F.conv2d(m1.double(), w2.double(), padding=1), 1).clamp_min(0).to(bf)
    t = F.conv2d(m2.double(), w3.double())
    ref = (bn(t + F.conv2d(x.double(), wd.double()), 2) if ds else bn(t, 2) + x.double()).clamp_min(0)

    def rows(w, rows_pad):                      # OIHW -> [O..][kh][kw][I] bf16, rows zero-padded
        o = torch.zeros(rows_pad, w.shape[2], w.shape[3], w.shape[1], dtype=bf)
        o[:w.shape[0]] = w.permute(0, 2, 3, 1)
        return o.contiguous().to(dev)
    w3p = torch.cat([w3, wd], 1) if ds else w3
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    y = torch.full((N, H, W, 256), float("nan"), dtype=bf, device=dev)
    dv = [rows(w1, 128), rows(w2, 128), rows(w3p, 256)] + [t.to(dev) for t in sc + sh]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = Nn.lib().ap_bottleneck64_nhwc(Nn.PRECISIONS[prec], p(xd), p(dv[0]), p(dv[3]), p(dv[6]), p(dv[1]), p(dv[4]), p(dv[7]), p(dv[2]),
                                       p(dv[5]), p(dv[8]), p(y), N, H, W, cin, int(ds), Nn.stream_ptr(dev))
    Nn.check(rc, "ap_bottleneck64_nhwc")
    torch.cuda.synchronize()
    return y.float().cpu().permute(0, 3, 1, 2).double(), ref


@pytest.mark.parametrize("ds", [0, 1])
@pytest.mark.parametrize("N,H", [(2, 56), (3, 14), (1, 28), (5, 56), (21, 56)])   # 21*16 = 336 tiles > 256 CUs: persistent loop
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_fused_bottleneck_primitive(dev, N, H, ds, prec):
    got, ref = _bneck_case(dev, N, H, ds, seed=100 * N + H + ds, prec=prec)
    assert torch.isfinite(got).all()
    # same operands and the same 16-bit rounding points: what differs is the fp32 accumulation order (an intermediate
    # may round to the neighbouring 16-bit value) and the rounding of the output
    assert rel_err(got.numpy(), ref.numpy()) < (8e-3 if prec == "bf16" else 1e-3)


@pytest.mark.parametrize("ds", [0, 1])
def test_fused_bottleneck_rectangular_image(dev, ds):
    """H != W (2 x 3 tiles): tile rows / columns and the image border masks are not interchangeable."""
    got, ref = _bneck_case(dev, 3, 28, ds, seed=31 + ds, W=42)
    assert torch.isfinite(got).all()
    assert rel_err(got.numpy(), ref.numpy()) < 8e-3


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_fused_bottleneck_persistent_loop_equals_three_convs(dev, prec):
    """More tiles than CUs (and not a multiple): every workgroup of the persistent kernel walks several tiles, the
    last round is partial.  The fused block must equal conv1 -> conv2 -> conv3(+identity) bit for bit (same operands,
    same bf16 rounding points, same K order per output element)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    bf = H16[prec]
    g = torch.Generator().manual_seed(77)
    N, H = 37, 56                                           # 592 tiles on 256 CUs
    x = torch.randn(N, H, H, 256, generator=g).to(bf).to(dev)
    w1 = (torch.randn(128, 256, generator=g) * (2.0 / 256) ** 0.5).to(bf).to(dev)
    w2 = (torch.randn(128, 576, generator=g) * (2.0 / 576) ** 0.5).to(bf).to(dev)
    w3 = (torch.randn(256, 64, generator=g) * (2.0 / 64) ** 0.5).to(bf).to(dev)
    sc = [(torch.rand(c, generator=g) + 0.5).to(dev) for c in (128, 128, 256)]
    sh = [(torch.randn(c, generator=g) * 0.1).to(dev) for c in (128, 128, 256)]
    y = torch.full((N, H, H, 256), float("nan"), dtype=bf, device=dev)
    y2 = torch.empty_like(y)
    t1 = torch.empty(N, H, H, 64, dtype=bf, device=dev)
    t2 = torch.empty_like(t1)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS[prec]
    Nn.check(L.ap_bottleneck64_nhwc(B, p(x), p(w1), p(sc[0]), p(sh[0]), p(w2), p(sc[1]), p(sh[1]), p(w3), p(sc[2]), p(sh[2]),
                                    p(y), N, H, H, 256, 0, st), "ap_bottleneck64_nhwc")
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w1), p(sc[0]), p(sh[0]), None, p(t1), N, H, H, 256, 64, 1, 1, 0, 1, st), "c1")
    Nn.check(L.ap_conv2d_nhwc(B, p(t1), p(w2), p(sc[1]), p(sh[1]), None, p(t2), N, H, H, 64, 64, 3, 1, 1, 1, st), "c2")
    Nn.check(L.ap_conv2d_nhwc(B, p(t2), p(w3), p(sc[2]), p(sh[2]), p(x), p(y2), N, H, H, 64, 256, 1, 1, 0, 1, st), "c3")
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


def test_fused_bottleneck_is_deterministic(dev):
    a, _ = _bneck_case(dev, 4, 56, 0, seed=9)
    b, _ = _bneck_case(dev, 4, 56, 0, seed=9)
    assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_fused_bottleneck_full_size_is_deterministic(dev, prec):
    """512 images (32 tiles per workgroup: the steady state of the persistent loop, every hand-counted wait met many times
    over): the same bits run to run, in both storage types."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    bf = H16[prec]
    g = torch.Generator().manual_seed(5)
    N, H = 512, 56
    x = torch.randn(N, H, H, 256, generator=g, dtype=torch.float32).to(bf).to(dev)
    w1 = (torch.randn(128, 256, generator=g) * (2.0 / 256) ** 0.5).to(bf).to(dev)
    w2 = (torch.randn(128, 576, generator=g) * (2.0 / 576) ** 0.5).to(bf).to(dev)
    w3 = (torch.randn(256, 64, generator=g) * (2.0 / 64) ** 0.5).to(bf).to(dev)
    sc = [(torch.rand(c, generator=g) + 0.5).to(dev) for c in (128, 128, 256)]
    sh = [(torch.randn(c, generator=g) * 0.1).to(dev) for c in (128, 128, 256)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = Nn.stream_ptr(dev)
    outs = []
    for _ in range(3):
        y = torch.full((N, H, H, 256), float("nan"), dtype=bf, device=dev)
        Nn.check(L.ap_bottleneck64_nhwc(Nn.PRECISIONS[prec], p(x), p(w1), p(sc[0]), p(sh[0]), p(w2), p(sc[1]), p(sh[1]), p(w3), p(sc[2]),
                                        p(sh[2]), p(y), N, H, H, 256, 0, st), "ap_bottleneck64_nhwc")
        torch.cuda.synchronize()
        outs.append(y)
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


@pytest.mark.parametrize("y_even", [0, 1])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_fused_bottleneck_tail_equals_block_then_conv1(dev, prec, y_even):
    """bottleneck2.hip tail variant (layer1's last block + conv1 of layer2.0, model_copenet.py:27-47 then :29-31 of the next
    block): t1n must carry the bits of ap_bottleneck64_nhwc followed by the stand-alone 1x1 convolution, y the bits of the plain
    block -- everywhere (y_even = 0) or at the even pixels with the others untouched (y_even = 1).  37 images = 592 tiles on 256
    workgroups: every hand-counted wait of the persistent loop is met in its steady state and in a partial last round."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    bf = H16[prec]
    g = torch.Generator().manual_seed(177 + y_even)
    N, H = 37, 56
    x = torch.randn(N, H, H, 256, generator=g).to(bf).to(dev)
    w1 = (torch.randn(128, 256, generator=g) * (2.0 / 256) ** 0.5).to(bf).to(dev)
    w2 = (torch.randn(128, 576, generator=g) * (2.0 / 576) ** 0.5).to(bf).to(dev)
    w3 = (torch.randn(256, 64, generator=g) * (2.0 / 64) ** 0.5).to(bf).to(dev)
    w1n = (torch.randn(128, 256, generator=g) * (2.0 / 256) ** 0.5).to(bf).to(dev)
    sc = [(torch.rand(c, generator=g) + 0.5).to(dev) for c in (128, 128, 256, 128)]
    sh = [(torch.randn(c, generator=g) * 0.1).to(dev) for c in (128, 128, 256, 128)]
    y = torch.full((N, H, H, 256), float("nan"), dtype=bf, device=dev)
    t1n = torch.full((N, H, H, 128), float("nan"), dtype=bf, device=dev)
    y_ref = torch.empty_like(y)
    t1n_ref = torch.empty_like(t1n)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS[prec]
    Nn.check(L.ap_bottleneck64_tail_nhwc(B, p(x), p(w1), p(sc[0]), p(sh[0]), p(w2), p(sc[1]), p(sh[1]), p(w3), p(sc[2]), p(sh[2]),
                                         p(y), p(w1n), p(sc[3]), p(sh[3]), p(t1n), y_even, N, H, H, st), "ap_bottleneck64_tail_nhwc")
    Nn.check(L.ap_bottleneck64_nhwc(B, p(x), p(w1), p(sc[0]), p(sh[0]), p(w2), p(sc[1]), p(sh[1]), p(w3), p(sc[2]), p(sh[2]),
                                    p(y_ref), N, H, H, 256, 0, st), "ap_bottleneck64_nhwc")
    Nn.check(L.ap_conv2d_nhwc(B, p(y_ref), p(w1n), p(sc[3]), p(sh[3]), None, p(t1n_ref), N, H, H, 256, 128, 1, 1, 0, 1, st), "c1n")
    torch.cuda.synchronize()
    assert torch.isfinite(t1n.float()).all()
    assert torch.equal(t1n.view(torch.int16), t1n_ref.view(torch.int16))
    yi, ri = y.view(torch.int16), y_ref.view(torch.int16)
    if y_even:
        assert torch.equal(yi[:, ::2, ::2], ri[:, ::2, ::2])
        assert torch.isnan(y[:, 1::2].float()).all() and torch.isnan(y[:, :, 1::2].float()).all()   # untouched
    else:
        assert torch.equal(yi, ri)


@pytest.mark.parametrize("N", [1, 3, 300])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_block_img_equals_three_convs(dev, prec, N):
    """block_img.hip (one layer3 identity bottleneck per launch, an image per workgroup, t1 / t2 resident in LDS, weights streamed
    from L2 as MFMA fragments; Bottleneck.forward, model_copenet.py:27-47) against conv1 -> conv2 -> conv3(+identity) through the
    stand-alone kernels the trunk would run (ring kernel for the pointwise layers, slab kernel for conv2: the same K order per
    output element, the same rounding points): 1 image, 3 images, and 300 images on 256 workgroups (the persistent loop, the
    weight-stream wrap and the staging ring across images)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    bf = H16[prec]
    g = torch.Generator().manual_seed(900 + N)
    H = 14
    x = torch.randn(N, H, H, 1024, generator=g).to(bf).to(dev)
    w1 = (torch.randn(256, 1024, generator=g) * (2.0 / 1024) ** 0.5).to(bf).to(dev)
    w2 = (torch.randn(256, 2304, generator=g) * (2.0 / 2304) ** 0.5).to(bf).to(dev)
    w3 = (torch.randn(1024, 256, generator=g) * (2.0 / 256) ** 0.5).to(bf).to(dev)
    sc = [(torch.rand(c, generator=g) + 0.5).to(dev) for c in (256, 256, 1024)]
    sh = [(torch.randn(c, generator=g) * 0.1).to(dev) for c in (256, 256, 1024)]
    sc[2] = sc[2] * 0.5
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS[prec]
    ws = torch.empty(L.ap_block_img_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_block_img_pack(B, p(w1), p(w2), p(w3), p(ws), st), "ap_block_img_pack")
    y = torch.full((N, H, H, 1024), float("nan"), dtype=bf, device=dev)
    Nn.check(L.ap_block_img_nhwc(B, p(x), p(ws), p(sc[0]), p(sh[0]), p(sc[1]), p(sh[1]), p(sc[2]), p(sh[2]), p(y), N, st), "ap_block_img_nhwc")
    t1 = torch.empty(N, H, H, 256, dtype=bf, device=dev)
    t2 = torch.empty_like(t1)
    y2 = torch.empty_like(y)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w1), p(sc[0]), p(sh[0]), None, p(t1), N, H, H, 1024, 256, 1, 1, 0, 1, st), "c1")
    Nn.check(L.ap_conv2d_nhwc(B, p(t1), p(w2), p(sc[1]), p(sh[1]), None, p(t2), N, H, H, 256, 256, 3, 1, 1, 1, st), "c2")
    Nn.check(L.ap_conv2d_nhwc(B, p(t2), p(w3), p(sc[2]), p(sh[2]), p(x), p(y2), N, H, H, 256, 1024, 1, 1, 0, 1, st), "c3")
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    e = rel_err(y.float().cpu().numpy(), y2.float().cpu().numpy())
    nbad = int((y.view(torch.int16) != y2.view(torch.int16)).sum())
    print("block_img vs three convs: rel err %.3e, %d of %d values differ" % (e, nbad, y.numel()))
    assert e < (1.6e-2 if prec == "bf16" else 2e-3)          # one 16-bit step of an intermediate at most
    assert nbad == 0                                          # same K order per output element: the same bits


PW_CASES = [  # (M, Cin, Cout, identity): conv1 of layer4.0 / 4.1, conv3 of a layer4 identity block, conv1 / conv3 of layer3, ragged tile counts
    (196 * 8, 1024, 512, False), (196 * 3, 2048, 512, False), (196 * 5, 512, 2048, True), (196 * 9, 1024, 256, False),
    (196 * 2, 256, 1024, True), (196 * 300, 1024, 512, False), (196 * 67, 512, 2048, True)]


@pytest.mark.parametrize("case", PW_CASES)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_pw_equals_generic_kernels(dev, prec, case):
    """conv_pw.hip (pointwise conv + BN (+ identity) + ReLU, 196-pixel x 256-channel tiles, one wave per SIMD, weights streamed from
    L2 as MFMA fragments; conv1 / conv3 of Bottleneck.forward, model_copenet.py:29-31, 38-45) against ap_conv2d_nhwc's automatic
    kernel on the same operands: the same K order per output element, so every bit equal -- one tile group, ragged groups of eight,
    several tiles per workgroup (weight-stream wrap, staging ring and identity registers across tiles), 2 and 8 channel tiles."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    M, Cin, Cout, ident = case
    bf = H16[prec]
    g = torch.Generator().manual_seed(M + Cin)
    x = torch.randn(M, Cin, generator=g).to(bf).to(dev)
    w = (torch.randn(Cout, Cin, generator=g) * (2.0 / Cin) ** 0.5).to(bf).to(dev)
    res = torch.randn(M, Cout, generator=g).to(bf).to(dev) if ident else None
    sc, sh = (torch.rand(Cout, generator=g) * 0.5 + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS[prec]
    ws = torch.empty(L.ap_conv_pw_stream_bytes(Cin, Cout), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_pw_pack(B, p(w), Cin, Cout, p(ws), st), "ap_conv_pw_pack")
    y = torch.full((M, Cout), float("nan"), dtype=bf, device=dev)
    guard = torch.full((4096,), 7.0, dtype=bf, device=dev)   # (allocated right behind y: an out-of-tile store would land here or in y's NaNs)
    Nn.check(L.ap_conv_pw_nhwc(B, p(x), p(ws), p(sc), p(sh), p(res), p(y), M, Cin, Cout, st), "ap_conv_pw_nhwc")
    y2 = torch.empty_like(y)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w), p(sc), p(sh), p(res), p(y2), M // 196, 14, 14, Cin, Cout, 1, 1, 0, 1, st), "conv2d")
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and bool((guard == 7.0).all())
    nbad = int((y.view(torch.int16) != y2.view(torch.int16)).sum())
    print("conv_pw vs generic: %d of %d values differ (rel err %.3e)" % (nbad, y.numel(), rel_err(y.float().cpu().numpy(), y2.float().cpu().numpy())))
    assert nbad == 0
    with pytest.raises(RuntimeError):
        Nn.check(L.ap_conv_pw_nhwc(B, p(x), p(ws), p(sc), p(sh), p(res), p(y), M - 1, Cin, Cout, st), "ap_conv_pw_nhwc")


@pytest.mark.parametrize("case", [(8, 7, 512, 1024, 2048), (3, 14, 256, 512, 1024), (36, 7, 512, 1024, 2048)])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_pw_stage_first_block(dev, prec, case):
    """conv_pw.hip with the downsample branch as a second K segment (conv3 of a stage's first block: the block input read at the
    stride-2 pixel; model_copenet.py:38-45 with :41-42, 97-102) -- layer4.0's shape on one and on nine tiles, layer3.0's on three:
    against fp64 on identical operands, and, for layer3.0's shape, bit for bit against the pair kernel that runs it in the trunk."""
    from airpose_amd import _native as Nn
    n, Ho, P, P2, C3 = case
    L = Nn.lib()
    g = torch.Generator().manual_seed(17 + P + n)
    H2, M = 2 * Ho, n * Ho * Ho
    bf = H16[prec]
    t2 = torch.randn(M, P, generator=g).clamp_min(0).to(bf).to(dev)
    x = torch.randn(n, H2, H2, P2, generator=g).clamp_min(0).to(bf).to(dev)
    w3d = (torch.randn(C3, P + P2, generator=g) * (1.0 / (P + P2)) ** 0.5).to(bf).to(dev)
    h3 = (torch.randn(C3, generator=g) * 0.1).to(dev)
    ones = torch.ones(C3, device=dev)                        # the BatchNorm scales are folded into w3d (pack_c3_ds)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS[prec]
    ws = torch.empty(L.ap_conv_pw_stream_bytes(P + P2, C3), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_pw_pack(B, p(w3d), P + P2, C3, p(ws), st), "ap_conv_pw_pack")
    out = torch.full((M + 8, C3), float("nan"), dtype=bf, device=dev)
    Nn.check(L.ap_conv_pw_ds_nhwc(B, p(t2), p(x), p(ws), p(ones), p(h3), p(out), n, Ho, P, P2, C3, 2, st), "ap_conv_pw_ds_nhwc")
    torch.cuda.synchronize()
    assert torch.isnan(out[M:].float()).all() and torch.isfinite(out[:M].float()).all()
    xs = x[:, ::2, ::2, :].reshape(M, P2)
    want = (torch.cat([t2, xs], 1).double() @ w3d.double().T + h3.double()).clamp_min(0)
    assert rel_err(out[:M].double().cpu().numpy(), want.cpu().numpy()) < (6e-3 if prec == "bf16" else 8e-4)
    if (P, P2, C3) == (256, 512, 1024):
        wp = _pair_stream(dev, prec, w3d, None, P, P2, 0)
        ref = torch.empty(M, C3, dtype=bf, device=dev)
        Nn.check(L.ap_conv_pair_ds_nhwc(B, p(t2), p(x), p(wp), p(ones), p(h3), None, None, p(ref), None, n, Ho, P, P2, 2, 0, st), "ap_conv_pair_ds_nhwc")
        torch.cuda.synchronize()
        assert torch.equal(out[:M].view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("case", [(8, 14, 512, 512), (2, 28, 256, 256), (52, 14, 512, 512), (5, 28, 128, 256)])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_pw_3x3_stride2_equals_generic_kernel(dev, prec, case):
    """conv_pw.hip as nine pointwise taps (conv2 of a stage's first block: 3 x 3, stride 2, padding 1; model_copenet.py:32-34 with
    :18): layer4.0's shape on two and on thirteen tiles, layer3.0's on two, a 128-channel input -- every bit equal to
    ap_conv2d_nhwc's kernel for the same convolution (K in [tap][Cin] order on both; the zero padding of the top row / left column
    is where the two differ in mechanism)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    n, H, Cin, Cout = case
    bf = H16[prec]
    g = torch.Generator().manual_seed(31 + n + Cin)
    x = torch.randn(n, H, H, Cin, generator=g).to(bf).to(dev)
    w = (torch.randn(Cout, 9 * Cin, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(bf).to(dev)
    sc, sh = (torch.rand(Cout, generator=g) * 0.5 + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS[prec]
    ws = torch.empty(L.ap_conv_pw_stream_bytes(9 * Cin, Cout), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_pw_pack(B, p(w), 9 * Cin, Cout, p(ws), st), "ap_conv_pw_pack")
    Ho = H // 2
    y = torch.full((n, Ho, Ho, Cout), float("nan"), dtype=bf, device=dev)
    Nn.check(L.ap_conv_pw_k3s2_nhwc(B, p(x), p(ws), p(sc), p(sh), p(y), n, H, Cin, Cout, st), "ap_conv_pw_k3s2_nhwc")
    y2 = torch.empty_like(y)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w), p(sc), p(sh), None, p(y2), n, H, H, Cin, Cout, 3, 2, 1, 1, st), "conv2d")
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    nbad = int((y.view(torch.int16) != y2.view(torch.int16)).sum())
    print("conv_pw 3x3/2 vs generic: %d of %d values differ (rel err %.3e)" % (nbad, y.numel(), rel_err(y.float().cpu().numpy(), y2.float().cpu().numpy())))
    assert nbad == 0


def test_conv_pw_soak(dev):
    """Race screen of conv_pw.hip (every load and LDS read is an asm statement behind a hand-counted wait): 40 launches of the
    identity form on 67 x 8 tiles (three to four tiles per workgroup), odd ones beside a competing copy stream, every bit compared."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    bf, M, Cin, Cout = torch.float16, 196 * 67, 512, 2048
    g = torch.Generator().manual_seed(12)
    x = torch.randn(M, Cin, generator=g).to(bf).to(dev)
    w = (torch.randn(Cout, Cin, generator=g) * (2.0 / Cin) ** 0.5).to(bf).to(dev)
    res = torch.randn(M, Cout, generator=g).to(bf).to(dev)
    sc, sh = (torch.rand(Cout, generator=g) * 0.5 + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS["f16"]
    ws = torch.empty(L.ap_conv_pw_stream_bytes(Cin, Cout), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_pw_pack(B, p(w), Cin, Cout, p(ws), st), "pack")
    y2 = torch.empty(M, Cout, dtype=bf, device=dev)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w), p(sc), p(sh), p(res), p(y2), M // 196, 14, 14, Cin, Cout, 1, 1, 0, 1, st), "conv2d")
    noise = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream()
    bad = 0
    for rep in range(40):
        y = torch.full((M, Cout), float("nan"), dtype=bf, device=dev)
        if rep & 1:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                noise.add_(1.0)
        Nn.check(L.ap_conv_pw_nhwc(B, p(x), p(ws), p(sc), p(sh), p(res), p(y), M, Cin, Cout, st), "pw")
        bad += int((y.view(torch.int16) != y2.view(torch.int16)).sum())
    torch.cuda.synchronize()
    assert bad == 0, "%d values differ over 40 launches" % bad


def test_block_img_soak(dev):
    """Race screen of block_img.hip (every load and LDS read of it is an asm statement behind a hand-counted wait): 40 launches of
    300 images on 256 workgroups, odd ones beside a competing copy stream, every output bit compared with the three-convolution
    result.  (What this caught: an SGPR base restored by v_readlane right in front of an asm global_load -- VALU write of an SGPR
    -> VMEM read needs 5 wait states hipcc does not pad for asm -- one row's identity now and then came from the previous row.)"""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    bf, N, H = torch.float16, 300, 14
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, H, H, 1024, generator=g).to(bf).to(dev)
    w1 = (torch.randn(256, 1024, generator=g) * (2.0 / 1024) ** 0.5).to(bf).to(dev)
    w2 = (torch.randn(256, 2304, generator=g) * (2.0 / 2304) ** 0.5).to(bf).to(dev)
    w3 = (torch.randn(1024, 256, generator=g) * (2.0 / 256) ** 0.5).to(bf).to(dev)
    sc = [(torch.rand(c, generator=g) * 0.5 + 0.25).to(dev) for c in (256, 256, 1024)]
    sh = [(torch.randn(c, generator=g) * 0.1).to(dev) for c in (256, 256, 1024)]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    B = Nn.PRECISIONS["f16"]
    ws = torch.empty(L.ap_block_img_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_block_img_pack(B, p(w1), p(w2), p(w3), p(ws), st), "pack")
    t1 = torch.empty(N, H, H, 256, dtype=bf, device=dev)
    t2 = torch.empty_like(t1)
    ref = torch.empty_like(x)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w1), p(sc[0]), p(sh[0]), None, p(t1), N, H, H, 1024, 256, 1, 1, 0, 1, st), "c1")
    Nn.check(L.ap_conv2d_nhwc(B, p(t1), p(w2), p(sc[1]), p(sh[1]), None, p(t2), N, H, H, 256, 256, 3, 1, 1, 1, st), "c2")
    Nn.check(L.ap_conv2d_nhwc(B, p(t2), p(w3), p(sc[2]), p(sh[2]), p(x), p(ref), N, H, H, 256, 1024, 1, 1, 0, 1, st), "c3")
    torch.cuda.synchronize()
    junk = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    for r in range(40):
        y = torch.full((N, H, H, 1024), float("nan"), dtype=bf, device=dev)
        if r % 2:
            with torch.cuda.stream(side):
                junk[: 128 << 20].copy_(junk[128 << 20:], non_blocking=True)
        Nn.check(L.ap_block_img_nhwc(B, p(x), p(ws), p(sc[0]), p(sh[0]), p(sc[1]), p(sh[1]), p(sc[2]), p(sh[2]), p(y), N, st), "blk")
        torch.cuda.synchronize()
        nbad = int((y.view(torch.int16) != ref.view(torch.int16)).sum())
        assert nbad == 0, (r, nbad)


@pytest.mark.parametrize("n", [1, 3, 64])
def test_image_resident_layer3_blocks_match_the_convolutions(net16, dev, n):
    """layer3.1 .. 3.5 as image-resident kernels (block_img.hip; forced on: the automatic rule only takes them for passes that
    fill whole rounds of the chip) against conv2 (slab kernel) + fused conv3 -> conv1 pairs: every convolution sums in the same
    order on both paths, so the trunk features carry the same bits."""
    gen = torch.Generator(device="cpu").manual_seed(700 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    try:
        net16.set_img_block(0)
        ref = net16.forward_feat_ext(x).clone()
        net16.set_img_block(2)
        got = net16.forward_feat_ext(x).clone()
    finally:
        net16.set_img_block(1)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref)
    assert torch.equal(net16.forward_feat_ext(x), ref)      # automatic rule: whichever path it takes


@pytest.mark.parametrize("n", [4, 24])
def test_pointwise_kernel_in_the_trunk_is_bit_identical(net16, dev, n):
    """layer4's conv1 / conv3 + identity (and layer3's, with the image blocks off) on conv_pw.hip (forced on: the automatic rule only
    takes it for passes whose tiles fill the chip) against the generic kernels: the same K order per output element, so the trunk
    features carry the same bits (n = 4: one 196-pixel tile of 7 x 7 images; 24: six, and 24 whole 14 x 14 images)."""
    gen = torch.Generator(device="cpu").manual_seed(720 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    try:
        net16.set_pw_conv(0)
        ref = net16.forward_feat_ext(x).clone()
        net16.set_pw_conv(2)
        got = net16.forward_feat_ext(x).clone()
        net16.set_img_block(0)
        got2 = net16.forward_feat_ext(x).clone()
    finally:
        net16.set_pw_conv(1)
        net16.set_img_block(1)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref) and torch.equal(got2, ref)
    assert torch.equal(net16.forward_feat_ext(x), ref)      # automatic rule: whichever path it takes


def test_submit_keeps_converted_inputs_alive(netf16, body, dev):
    """submit() with crops that are NOT fp32-contiguous (half precision, a strided view): forward_feat_ext_twoview makes fp32
    copies, and in the asynchronous form the caller's stream is not behind the trunk passes -- the copies must outlive the call
    (record_stream on the pipeline's stream), or the caching allocator hands their blocks to the next allocation on the caller's
    stream while the passes still read them.  Allocations + fills of the same size right behind every submit try to provoke that."""
    from airpose_amd import pipeline, weights as W
    B = 64
    pipe = pipeline.TwoViewInference(netf16, body)
    base = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(640, B).items()}
    half = dict(base)
    half["im0"], half["im1"] = base["im0"].half(), base["im1"].half()
    ref_in = dict(base)
    ref_in["im0"], ref_in["im1"] = half["im0"].float(), half["im1"].float()
    want = {k: v.clone() for k, v in pipe(ref_in).items()}
    torch.cuda.synchronize()
    pend = []
    for i in range(6):
        pend.append(pipe.submit(half))
        junk = [torch.full((B, 3, 224, 224), float(i + 1), device=dev) for _ in range(2)]   # same size as the converted crops
        del junk
    for p in pend:
        got = p.synchronize()
        for k in ("pred_pose0", "pred_betas1", "pred_vertices_cam1"):
            assert torch.equal(got[k], want[k]), k
    big = torch.cat([base["im0"], base["im0"]], 0)           # strided view: every second image
    sv = dict(base)
    sv["im0"] = big[::2]
    assert not sv["im0"].is_contiguous() or B == 1
    ref2 = dict(base)
    ref2["im0"] = big[::2].contiguous()
    want2 = {k: v.clone() for k, v in pipe(ref2).items()}
    torch.cuda.synchronize()
    pend = []
    for i in range(4):
        pend.append(pipe.submit(sv))
        junk = torch.full((B, 3, 224, 224), -1.0, device=dev)
        del junk
    for p in pend:
        assert torch.equal(p.synchronize()["pred_vertices_cam0"], want2["pred_vertices_cam0"])


@pytest.mark.parametrize("n", [1, 3, 64])
def test_fused_tail_and_even_outputs_are_bit_identical(net16, dev, n):
    """conv1 of layer2.0 inside layer1's last kernel (ap_net_set_fuse_tail) and even-pixel-only stores of the block outputs whose
    one remaining reader is a stride-2 downsample branch (layer1.2, layer2.3: ap_net_set_even_out): same features, bit for bit,
    in every combination of the two knobs."""
    gen = torch.Generator(device="cpu").manual_seed(400 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    got = net16.forward_feat_ext(x).clone()
    assert torch.isfinite(got).all()
    try:
        for tail, even in ((0, 0), (1, 0), (0, 1)):
            net16.set_fuse_tail(tail)
            net16.set_even_out(even)
            assert torch.equal(net16.forward_feat_ext(x), got), (tail, even)
    finally:
        net16.set_fuse_tail(1)
        net16.set_even_out(1)
    assert torch.equal(net16.forward_feat_ext(x), got)


@pytest.mark.parametrize("n", [1, 2, 5, 6, 13, 64])
def test_fused_pool_is_bit_identical(net16, dev, n):
    """AvgPool2d(7) in the epilogue of layer4.2 conv3 (conv_lean.hip POOL variant: super-tiles of 5 images, the third one split
    over two sub-tiles) against conv3 + avgpool_kernel: the same bits for every batch size -- 1 image (a partly empty super-tile),
    2, exactly 5, 6 (one image in the second super-tile), 13, 64 -- and for an image wherever it sits in the batch."""
    gen = torch.Generator(device="cpu").manual_seed(100 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    ref = net16.forward_feat_ext(x).clone()
    try:
        net16.set_fuse_pool(1)
        got = net16.forward_feat_ext(x)
        assert torch.isfinite(ref).all()
        assert torch.equal(got, ref)
        if n >= 6:                                           # image 5 alone (first of a super-tile) == image 5 of the batch (sixth)
            assert torch.equal(net16.forward_feat_ext(x[5:6].contiguous()), ref[5:6])
    finally:
        net16.set_fuse_pool(0)


@pytest.mark.parametrize("n", [1, 3, 4, 64])
def test_tiled_intermediates_are_bit_identical(net16, dev, n):
    """Fragment-tiled storage of the pair-kernel-only tensors (default; ap_common.h ap_tiled_off: conv2's output of a pair block,
    identity/output between consecutive identity pair blocks) against NHWC everywhere: a pure relayout, so the features carry
    the same bits -- at 1 and 3 images (layer3 M = 196 / 588: a partly filled last micro-tile of 16 pixels), 4 and 64."""
    gen = torch.Generator(device="cpu").manual_seed(300 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    got = net16.forward_feat_ext(x).clone()
    try:
        net16.set_tiled(0)
        ref = net16.forward_feat_ext(x).clone()
    finally:
        net16.set_tiled(1)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref)
    assert torch.equal(net16.forward_feat_ext(x), ref)       # and back on


def test_fused_layer1_matches_separate_convs(net16, golden, copenet_inputs, dev):
    """Whole-bottleneck fusion of layer1 (default, bottleneck2.hip) vs its separate convolutions, through the trunk."""
    x = copenet_inputs["im0"].to(dev)
    try:
        net16.set_fuse_block(0)
        b = net16.forward_feat_ext(x).clone()
    finally:
        net16.set_fuse_block(1)
    c = net16.forward_feat_ext(x)
    assert torch.equal(b, c)           # same operands, rounding points and K order per output element
    assert rel_err(c.cpu().numpy(), golden["copenet_b2"]["xf0"]) < 3e-2


# ------------------------------------------------------------------------------------------------ trunk / IEF / forward
def test_trunk_fp32_matches_golden(golden, net32, copenet_inputs, dev):
    g = golden["copenet_b2"]
    xf0 = net32.forward_feat_ext(copenet_inputs["im0"].to(dev)).cpu().numpy()
    xf1 = net32.forward_feat_ext(copenet_inputs["im1"].to(dev)).cpu().numpy()
    e0, e1 = rel_err(xf0, g["xf0"]), rel_err(xf1, g["xf1"])
    print("trunk fp32 rel err %.3e %.3e" % (e0, e1))
    assert e0 < TOL32 and e1 < TOL32


def test_split_bf16_parity_mode_matches_golden(golden, netx2, copenet_inputs, dev):
    """bf16x2 = the fast parity mode: trunk features and the regressed theta / beta after 3 IEF iterations against the
    golden made by the imported reference.  north_star's bar (1e-4 on the outputs) with a wide margin; the features
    themselves carry the 2^-17 operand rounding of 53 layers (reported)."""
    g = golden["copenet_b2"]
    gin = {k: v.to(dev) for k, v in copenet_inputs.items()}
    xf0 = netx2.forward_feat_ext(gin["im0"])
    ef = rel_err(xf0.cpu().numpy(), g["xf0"])
    pos = torch.from_numpy(g["init_position"]).to(dev)
    p0, b0, p1, b1 = netx2(gin["im0"], gin["im1"], gin["bb0"], gin["bb1"], pos, pos, iters=3)
    errs = dict(pose_rel_errs(p0.cpu().numpy(), g["pose0_it3"]), betas0=rel_err(b0.cpu().numpy(), g["betas0_it3"]),
                betas1=rel_err(b1.cpu().numpy(), g["betas1_it3"]), pose1=pose_err(p1, g["pose1_it3"]))
    print("bf16x2 trunk features rel err %.3e; outputs %s" % (ef, errs))
    assert ef < 1e-4
    assert max(errs.values()) < 2e-5


# ------------------------------------------------------------------------------------------------ fp16 storage
def test_f16_throughput_mode_meets_the_parity_bar(golden, netf16, netbf, copenet_inputs, dev):
    """The throughput kernels with fp16 instead of bf16 storage (same kernels, same MFMA rate, 11 significand bits): theta /
    beta after 3 IEF iterations against the golden made by the imported reference are under north_star's 1e-4, where the
    bf16 storage of the same kernels is 3-6x over it (three quarters of that is the rounding of the weights)."""
    g = golden["copenet_b2"]
    gin = {k: v.to(dev) for k, v in copenet_inputs.items()}
    pos = torch.from_numpy(g["init_position"]).to(dev)
    worst = {}
    for name, net in (("f16", netf16), ("bf16", netbf)):
        ef = rel_err(net.forward_feat_ext(gin["im0"]).cpu().numpy(), g["xf0"])
        p0, b0, p1, b1 = net(gin["im0"], gin["im1"], gin["bb0"], gin["bb1"], pos, pos, iters=3)
        errs = dict(pose_rel_errs(p0.cpu().numpy(), g["pose0_it3"]), betas0=rel_err(b0.cpu().numpy(), g["betas0_it3"]),
                    betas1=rel_err(b1.cpu().numpy(), g["betas1_it3"]), pose1=pose_err(p1, g["pose1_it3"]))
        print("%s trunk features rel err %.3e; outputs %s" % (name, ef, errs))
        worst[name] = max(errs.values())
    assert worst["f16"] < 1e-4
    assert worst["f16"] < 0.5 * worst["bf16"]


def test_f16_whole_pipeline_matches_oracle(netf16, body, copenet_sd, copenet_inputs, smplx_model, dev):
    """The whole hot path (trunk, IEF, rot6d, SMPL-X, projection) in fp16 storage against the CPU oracle: 1e-4 per slice."""
    from airpose_amd import pipeline
    from oracle import pipeline_ref
    inp = copenet_inputs
    with torch.no_grad():
        want = pipeline_ref.infer(copenet_sd, smplx_model, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], inp["intr0"], inp["intr1"])
    got = pipeline.TwoViewInference(netf16, body)({k: v.to(dev) for k, v in inp.items()})
    for k in ("pred_pose0", "pred_pose1", "pred_betas0", "pred_betas1", "pred_vertices_cam0", "pred_j3d_cam1", "pred_j2d_cam0"):
        a, b = got[k].cpu().double().numpy(), want[k].double().numpy()
        parts = {"trans": (a[:, :3], b[:, :3]), "rot6d": (a[:, 3:], b[:, 3:])} if "pose" in k else {"": (a, b)}
        for nm, (x, y) in parts.items():
            e = float(np.abs(x - y).max() / np.abs(y).max())
            assert e < 1e-4, "%s %s rel err %.3e" % (k, nm, e)


@pytest.mark.parametrize("B", [3, 64])
def test_pipelined_submit_is_bit_identical_to_call(netf16, body, dev, B):
    """TwoViewInference.submit (trunk of batch i+1 on the caller's stream under the IEF loop + SMPL-X stage of batch i on a second
    stream; ap_trunk_fwd_twoview + ap_regressor_fwd + ap_smplx_fwd_twoview) against __call__ (ap_copenet_fwd +
    ap_smplx_fwd_twoview on one stream): the same kernels on the same data, so every output equal to the bit -- over six
    back-to-back submits of three different batches (the feature slots and their reused events go round twice;
    B = 64 takes the two-stream trunk)."""
    from airpose_amd import pipeline, weights as W
    pipe = pipeline.TwoViewInference(netf16, body)
    batches = [{k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(500 + i, B).items()} for i in range(3)]
    want = [{k: v.clone() for k, v in pipe(b, want_angles=True).items()} for b in batches]
    torch.cuda.synchronize()
    pend = [pipe.submit(batches[i % 3], want_angles=True) for i in range(6)]
    for i in (5, 0, 3, 1, 4, 2):                             # collected out of order
        got = pend[i].synchronize()
        assert set(got) == set(want[i % 3])
        for k, v in want[i % 3].items():
            assert torch.equal(got[k], v), (i, k)
    # wait(): the current stream is ordered behind the tail
    p = pipe.submit(batches[1])
    v = p.wait()["pred_vertices_cam0"] + 0.0
    assert torch.equal(v, want[1]["pred_vertices_cam0"])
    # soak: 45 submits without a host wait in between (the host only blocks when all DEPTH slots are taken), every result checked
    pend = [pipe.submit(batches[i % 3], want_rotmat=False) for i in range(45)]
    for i, p in enumerate(pend):
        got = p.synchronize()
        for k in ("pred_pose0", "pred_betas1", "pred_vertices_cam1", "pred_j2d_cam0"):
            assert torch.equal(got[k], want[i % 3][k]), (i, k)
    del pend
    # a stream-ordered call right behind submits (shared regressor / SMPL-X workspaces): ordered behind them by the pipeline
    pend = [pipe.submit(batches[i]) for i in range(3)]
    got = pipe(batches[0], want_angles=True)
    for k, v in want[0].items():
        assert torch.equal(got[k], v), k
    assert torch.equal(pend[2].synchronize()["pred_j2d_cam1"], want[2]["pred_j2d_cam1"])
    q = pipe.submit_net(*(batches[2][k] for k in ("im0", "im1", "bb0", "bb1"))).synchronize()
    assert torch.equal(q[0][:, 3:], want[2]["pred_pose0"][:, 3:]) and torch.equal(q[3], want[2]["pred_betas1"])
    f = netf16.forward_feat_ext_twoview(batches[0]["im0"], batches[0]["im1"])
    assert torch.equal(f[0], netf16.forward_feat_ext(batches[0]["im0"])) or B >= 64    # (one pass vs two: same kernels per image)
    assert torch.equal(f[1], netf16.forward_feat_ext(batches[0]["im1"])) or B >= 64
    with pytest.raises(RuntimeError):
        netf16.forward_feat_ext_twoview(batches[0]["im0"], batches[0]["im1"], out=torch.empty(2, B, 2047, device=dev))


def test_two_stream_trunk_in_slices_above_one_chunk(netf16, dev):
    """A two-view batch above one chunk keeps the two concurrent passes: each view goes through its stream in slices of chunk / 2
    images (here chunk = 128: 96 images per view = two slices of 48).  Features equal to the bit to the one-view calls (a
    feature row does not depend on the batch it arrives in)."""
    g = torch.Generator(device="cpu").manual_seed(11)
    x0 = torch.randn(96, 3, 224, 224, generator=g).to(dev)
    x1 = torch.randn(96, 3, 224, 224, generator=g).to(dev)
    want0, want1 = netf16.forward_feat_ext(x0).clone(), netf16.forward_feat_ext(x1).clone()
    try:
        netf16.set_chunk(128)
        for _ in range(2):
            f = netf16.forward_feat_ext_twoview(x0, x1)
            assert torch.equal(f[0], want0) and torch.equal(f[1], want1)
        side = torch.cuda.Stream(device=dev)
        f = netf16.forward_feat_ext_twoview(x0, x1, out_stream=side)
        side.synchronize()
        assert torch.equal(f[0], want0) and torch.equal(f[1], want1)
    finally:
        netf16.set_chunk(0)
    assert torch.equal(netf16.forward_feat_ext_twoview(x0, x1)[1], want1)


def test_f16_refuses_weights_outside_the_fp16_range(copenet_sd, dev):
    """A (BatchNorm-folded) weight above 65 504 would be inf in fp16 storage: AP_PREC_F16 refuses the checkpoint when it
    packs it, AP_PREC_BF16 (fp32's exponent range) takes it."""
    from airpose_amd import copenet_model
    sd = {k: v.clone() for k, v in copenet_sd.items()}
    sd["layer3.2.conv2.weight"][5, 7, 1, 1] = 3.0e5
    x = torch.zeros(1, 3, 224, 224, device=dev)
    bad = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    bad.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="fp16 range"):
        bad.forward_feat_ext(x)
    ok = copenet_model.getcopenet(MEAN_PARAMS, precision="bf16").eval()
    ok.load_state_dict(sd)
    assert torch.isfinite(ok.forward_feat_ext(x)).all()


def test_f16_activation_overflow_is_reported(copenet_sd, dev):
    """fp16 storage: a stored activation above 65 504 becomes inf.  Every kernel of the trunk tracks the packed values it stores
    (ap_common.h: ap_rng_note; the sentinel of include/airpose_hip.h, ap_net_set_range_check): with a checkpoint scaled to overflow (bn1 of the stem x 1e6: BatchNorm
    constants are fp32 epilogue parameters, so the fp16 weight check passes, and the stem's output is of order 3e5) the deferred mode (default) raises at range_status() and at the NEXT
    forward; the synchronous mode raises from the offending forward itself; a clean handle stays silent; bf16 storage takes the
    same checkpoint."""
    from airpose_amd import _native as Nn
    from airpose_amd import copenet_model
    sd = {k: v.clone() for k, v in copenet_sd.items()}
    sd["bn1.weight"] *= 1.0e6                                 # stem output ~ 3e5 |N(0, 1)|: most of it beyond 65 504
    sd["bn1.bias"] *= 1.0e6
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 224, 224, generator=g).to(dev)
    bad = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    bad.load_state_dict(sd)
    f = bad.forward_feat_ext(x)                              # deferred: the offending call itself returns
    torch.cuda.synchronize()
    # (the features themselves may well be finite: the NaNs an inf turns into in the next convolution are cleared by the ReLUs,
    #  which is why every epilogue tracks the values it stores instead of the pooling stage looking for inf at the end)
    with pytest.raises(Nn.RangeError, match="fp16 range"):
        bad.range_status()
    with pytest.raises(Nn.RangeError, match="fp16 range"):   # sticky: the next forward refuses
        bad.forward_feat_ext(x)
    with pytest.raises(Nn.RangeError):
        bad.range_status(reset=True)
    bad.set_range_check(2)                                   # synchronous: the forward raises for its own pass
    with pytest.raises(Nn.RangeError, match="fp16 range"):
        bad.forward_feat_ext(x)
    ok16 = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    ok16.load_state_dict(copenet_sd)
    ok16.set_range_check(2)
    assert torch.isfinite(ok16.forward_feat_ext(x)).all()
    ok16.range_status()
    okbf = copenet_model.getcopenet(MEAN_PARAMS, precision="bf16").eval()
    okbf.load_state_dict(sd)
    assert torch.isfinite(okbf.forward_feat_ext(x)).all()
    okbf.range_status()


def test_f16_fused_paths_are_bitwise(netf16, dev):
    """Every fused kernel in fp16 storage (the fused layer1 block, the conv3 -> conv1 pairs, the folded downsample, the fused
    stem) against its separate-kernel path through the trunk: same bits, as in bf16 storage."""
    from airpose_amd import weights as W
    x = torch.from_numpy(W.synthetic_inputs(11, 5)["im0"]).to(dev)
    ref = netf16.forward_feat_ext(x).clone()
    assert torch.isfinite(ref).all()
    try:
        for knob, vals in (("set_fuse_block", (0,)), ("set_fuse_pair", (0,)), ("set_fuse_stem", (0,)), ("set_fuse_ds", (0,))):
            for v in vals:
                getattr(netf16, knob)(v)
                got = netf16.forward_feat_ext(x)
                getattr(netf16, knob)(1)
                if knob == "set_fuse_ds":                    # the folded downsample re-associates the sum: close, not bitwise
                    assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) < 2e-3
                else:
                    assert torch.equal(got, ref), (knob, v)
    finally:
        netf16.set_fuse_block(1); netf16.set_fuse_pair(1); netf16.set_fuse_stem(1); netf16.set_fuse_ds(1)


def test_f16_two_stream_forward_is_bit_identical_to_single_pass(netf16, dev):
    B = 64
    gen = torch.Generator(device="cpu").manual_seed(32)
    x0, x1 = torch.randn(B, 3, 224, 224, generator=gen).to(dev), torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    bb0, bb1 = torch.rand(B, 3, generator=gen).to(dev), torch.rand(B, 3, generator=gen).to(dev)
    pos = torch.tensor([0.0, 0.0, 0.5], device=dev).expand(B, 3).contiguous()
    try:
        netf16.set_dual_stream(0)
        one = [t.clone() for t in netf16(x0, x1, bb0, bb1, pos, pos, iters=3)]
        netf16.set_dual_stream(1)
        for _ in range(3):
            two = netf16(x0, x1, bb0, bb1, pos, pos, iters=3)
            torch.cuda.synchronize()
            for a, b in zip(one, two):
                assert torch.equal(a, b)
    finally:
        netf16.set_dual_stream(1)


def test_split_bf16_whole_pipeline_matches_oracle(netx2, body, copenet_sd, copenet_inputs, smplx_model, dev):
    from airpose_amd import pipeline
    from oracle import pipeline_ref
    inp = copenet_inputs
    with torch.no_grad():
        want = pipeline_ref.infer(copenet_sd, smplx_model, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"],
                                  inp["intr0"], inp["intr1"])
    got = pipeline.TwoViewInference(netx2, body)({k: v.to(dev) for k, v in inp.items()}, want_angles=True)
    worst = 0.0
    for k in sorted(want):
        for nm, e in key_errs(k, got[k].cpu().numpy(), want[k].numpy()).items():
            worst = max(worst, e)
            assert e < TOL32, nm
    print("bf16x2 whole pipeline: worst per-slice rel err %.3e" % worst)


def test_regressor_fold_guard(golden, copenet_sd, copenet_inputs, dev):
    """ap_net_finalize checks the folded 145 x 2332 regressor map of the checkpoint it packs against the literal fc1 -> fc2 -> dec
    chain (fp64, fixed probe batch): the benchmark weights pass far below the 1e-5 bar; with the bar forced to 0 the same
    checkpoint is 'rejected' -- the handle then runs the literal chain (golden parity unchanged), says so, and keeps it when
    ap_net_set_fold(1) is (re-)applied (a remembered knob must not turn every later call into an error)."""
    import ctypes as C
    from airpose_amd import _native as Nn
    from airpose_amd import copenet_model
    g = golden["copenet_b2"]
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(copenet_sd)
    inp = {k: v.to(dev) for k, v in copenet_inputs.items()}
    pos = torch.tensor([0.0, 0.0, 10.0], device=dev).expand(inp["im0"].shape[0], 3).contiguous() * 0.05
    a = [t.clone() for t in net(inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], pos, pos, iters=3)]
    st, err = net.fold_status()
    assert st == 1 and err < 1e-6, (st, err)
    h = net._native(dev)
    Nn.check(Nn.lib().ap_net_set_fold_bar(h, C.c_double(0.0)), "ap_net_set_fold_bar")
    net.repack()                                            # next forward packs + finalises again, now with the bar at 0
    b = net(inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], pos, pos, iters=3)
    st, err2 = net.fold_status()
    assert st == 0 and err2 == err
    net.set_fold(1)                                         # a remembered knob on a rejected checkpoint: a warned no-op, not an error
    st2, _ = net.fold_status()
    assert st2 == 0                                         # ... and the literal chain stays
    c = net(inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], pos, pos, iters=3)
    assert all(torch.equal(x, y) for x, y in zip(b, c))
    for x, y, key in zip(a, b, ("pose0", "betas0", "pose1", "betas1")):
        assert pose_err(x, y) < 1e-5 if "pose" in key else rel_err(x.cpu().numpy(), y.cpu().numpy()) < 1e-5
        want = g[key + "_it3"] if (key + "_it3") in g.files else None
        if want is not None:
            e = pose_err(y, want) if "pose" in key else rel_err(y.cpu().numpy(), want)
            assert e < TOL32, (key, e)


def test_trunk_bf16_close_to_golden(golden, netbf, copenet_inputs, dev):
    g = golden["copenet_b2"]
    xf0 = netbf.forward_feat_ext(copenet_inputs["im0"].to(dev)).cpu().numpy()
    e0 = rel_err(xf0, g["xf0"])
    print("trunk bf16 rel err %.3e" % e0)
    assert e0 < TOLBF


@pytest.mark.parametrize("n", [1, 5, 64, 300])
def test_fused_stem_pool_is_bit_identical(net16, dev, n):
    """conv1+bn1+relu+maxpool fused kernel == stem kernel followed by the max-pool kernel, bit for bit, in both 16-bit types."""
    gen = torch.Generator(device="cpu").manual_seed(500 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    x[0, :, :9, :] = 3.0                                      # a flat top edge: the first strip's missing conv row must not win a maximum
    x[n - 1, :, -9:, :] = 3.0                                 # ... and the bottom, left and right edges (zero padding of the conv, the pool's
    x[n // 2, :, :, :7] = 3.0                                 # border columns: the persistent kernel computes conv column 0 twice instead
    x[n // 2, :, :, -7:] = 3.0                                # of padding, and carries each strip's last conv row into the next strip)
    try:
        net16.set_fuse_stem(0)
        ref = net16.forward_feat_ext(x).clone()
        net16.set_fuse_stem(2)                                # a workgroup per strip (round 4)
        strip = net16.forward_feat_ext(x).clone()
    finally:
        net16.set_fuse_stem(1)                                # persistent workgroups, waves split by role (round 6, default)
    got = net16.forward_feat_ext(x)
    assert torch.isfinite(ref).all()
    assert torch.equal(strip, ref)
    assert torch.equal(got, ref)


def test_fused_split_stem_pool_is_bit_identical(netx2, dev):
    """bf16x2: the fused split stem + max-pool (split rounding after the 3x3 maximum) == the split stem followed by the split
    max-pool, bit for bit, for the first / last strips (padding rows) and both views of a batch."""
    from airpose_amd import weights as W
    x = torch.from_numpy(W.synthetic_inputs(5, 3)["im1"]).to(dev)
    netx2.set_fuse_stem(1)
    a = netx2.forward_feat_ext(x)
    netx2.set_fuse_stem(0)
    b = netx2.forward_feat_ext(x)
    netx2.set_fuse_stem(1)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_folded_downsample_matches_separate_convs(net32, netbf, golden, copenet_inputs, dev):
    """Downsample branch folded into conv3 (second K segment) vs the two separate convolutions."""
    x = copenet_inputs["im0"].to(dev)
    g = golden["copenet_b2"]
    for net, tol in ((net32, 1e-5), (netbf, 2e-2)):
        net.set_fuse_ds(1)
        a = net.forward_feat_ext(x)
        net.set_fuse_ds(0)
        b = net.forward_feat_ext(x)
        net.set_fuse_ds(1)
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < tol
    net32.set_fuse_ds(0)
    assert rel_err(net32.forward_feat_ext(x).cpu().numpy(), g["xf0"]) < TOL32      # literal path still at parity
    net32.set_fuse_ds(1)


def test_trunk_batch_and_chunk_invariance(net32, dev):
    """Ragged batches and the depth-first chunking must not change any value (each output element has a
    fixed accumulation order)."""
    from airpose_amd import weights as W
    x = torch.from_numpy(W.synthetic_inputs(99, 5)["im0"]).to(dev)
    net32.set_chunk(0)
    full = net32.forward_feat_ext(x)
    net32.set_chunk(2)
    chunked = net32.forward_feat_ext(x)
    net32.set_chunk(0)
    single = torch.cat([net32.forward_feat_ext(x[i:i + 1]) for i in range(5)])
    assert rel_err(chunked.cpu().numpy(), full.cpu().numpy()) < 1e-6
    assert rel_err(single.cpu().numpy(), full.cpu().numpy()) < 1e-6


def test_bf16_trunk_batch_and_chunk_invariance_bitwise(netbf, dev):
    """bf16 throughput path (fused stem+pool, persistent fused layer1 bottlenecks, ring convs): a ragged batch, a
    chunked pass and single-image passes give bit-identical features -- every output element has a fixed accumulation
    order whatever the grid (1 image = 16 bottleneck tiles on 16 workgroups; 37 images = 592 tiles on 256)."""
    from airpose_amd import weights as W
    x = torch.from_numpy(W.synthetic_inputs(98, 5)["im1"]).to(dev)
    netbf.set_chunk(0)
    full = netbf.forward_feat_ext(x)
    netbf.set_chunk(3)
    chunked = netbf.forward_feat_ext(x)
    netbf.set_chunk(0)
    single = torch.cat([netbf.forward_feat_ext(x[i:i + 1]) for i in range(5)])
    big = netbf.forward_feat_ext(torch.cat([x] * 8)[:37])
    assert torch.equal(chunked, full) and torch.equal(single, full)
    assert torch.equal(big[:5], full) and torch.equal(big[35:37], full[:2])


def test_ief_ragged_batches(net32, copenet_sd, dev):
    """The one-workgroup-per-pair IEF kernel and its split-K feature kernel at batch sizes around their tile sizes
    (8 rows per feature workgroup): rows must equal the same rows of a larger batch."""
    g = torch.Generator().manual_seed(21)
    B = 13
    xf0, xf1 = torch.randn(B, 2048, generator=g).to(dev), torch.randn(B, 2048, generator=g).to(dev)
    bb0, bb1 = torch.rand(B, 3, generator=g).to(dev), torch.rand(B, 3, generator=g).to(dev)
    pos = (torch.tensor([0.0, 0.0, 10.0]) * 0.05).expand(B, -1).contiguous().to(dev)
    full = net32.forward_ief(xf0, xf1, bb0, bb1, pos, pos, iters=3)
    for n in (1, 3, 8, 9):
        part = net32.forward_ief(xf0[:n], xf1[:n], bb0[:n], bb1[:n], pos[:n], pos[:n], iters=3)
        for a, b in zip(part, full):
            assert torch.equal(a, b[:n]), n


@pytest.mark.parametrize("fold", [1, 0])
def test_ief_fp32_matches_golden(golden, net32, copenet_inputs, dev, fold):
    """fold = 1: fc1 -> fc2 -> dec evaluated as the folded affine map; fold = 0: the literal chain."""
    net32.set_fold(fold)
    g = golden["copenet_b2"]
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    pos = t("init_position")
    for it in (1, 2, 3):
        p0, b0, p1, b1 = net32.forward_ief(t("xf0"), t("xf1"), copenet_inputs["bb0"].to(dev),
                                           copenet_inputs["bb1"].to(dev), pos, pos, iters=it)
        for got, key in ((p0, "pose0"), (b0, "betas0"), (p1, "pose1"), (b1, "betas1")):
            assert rel_err(got.cpu().numpy(), g["%s_it%d" % (key, it)]) < TOL32, (key, it)
    p0, b0, p1, b1 = net32.forward_ief(t("xf0"), t("xf1"), copenet_inputs["bb0"].to(dev), copenet_inputs["bb1"].to(dev),
                                       pos, pos, init_theta0=t("ci_theta0"), init_theta1=t("ci_theta1"),
                                       init_shape0=t("ci_shape0"), init_shape1=t("ci_shape1"), iters=2)
    assert pose_err(p0, g["ci_pose0"]) < TOL32 and pose_err(p1, g["ci_pose1"]) < TOL32
    assert rel_err(b0.cpu().numpy(), g["ci_betas0"]) < TOL32 and rel_err(b1.cpu().numpy(), g["ci_betas1"]) < TOL32
    net32.set_fold(1)


def test_fused_ief_kernel_matches_gemm_chain(golden, net32, copenet_inputs, dev):
    """One-kernel IEF (split-K feature GEMM + all iterations in a workgroup per pair) vs one GEMM per iteration;
    the golden comparison of the fused path itself is test_ief_fp32_matches_golden[fold=1]."""
    g = golden["copenet_b2"]
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    pos = t("init_position")
    outs = []
    for on in (1, 0):
        net32.set_fuse_ief(on)
        outs.append(net32.forward_ief(t("xf0"), t("xf1"), copenet_inputs["bb0"].to(dev), copenet_inputs["bb1"].to(dev),
                                      pos, pos, init_theta0=t("ci_theta0"), init_theta1=t("ci_theta1"),
                                      init_shape0=t("ci_shape0"), init_shape1=t("ci_shape1"), iters=3))
    net32.set_fuse_ief(1)
    for a, b in zip(*outs):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-5


def test_forward_fp32_matches_golden(golden, net32, copenet_inputs, dev):
    g = golden["copenet_b2"]
    gin = {k: v.to(dev) for k, v in copenet_inputs.items()}
    pos = torch.from_numpy(g["init_position"]).to(dev)
    p0, b0, p1, b1 = net32(gin["im0"], gin["im1"], gin["bb0"], gin["bb1"], pos, pos, iters=3)
    errs = [pose_err(p0, g["pose0_it3"]), rel_err(b0.cpu().numpy(), g["betas0_it3"]),
            pose_err(p1, g["pose1_it3"]), rel_err(b1.cpu().numpy(), g["betas1_it3"])]
    print("forward fp32 rel errs", errs)
    assert max(errs) < TOL32


def test_forward_bf16_tolerance(golden, netbf, copenet_inputs, dev):
    g = golden["copenet_b2"]
    gin = {k: v.to(dev) for k, v in copenet_inputs.items()}
    pos = torch.from_numpy(g["init_position"]).to(dev)
    p0, b0, p1, b1 = netbf(gin["im0"], gin["im1"], gin["bb0"], gin["bb1"], pos, pos, iters=3)
    slices = dict(pose_rel_errs(p0.cpu().numpy(), g["pose0_it3"]), betas=rel_err(b1.cpu().numpy(), g["betas1_it3"]))
    slices["rot6d_elementwise(atol 1e-2)"] = elem_err(p0[:, 3:].cpu().numpy(), g["pose0_it3"][:, 3:], 1e-2)
    print("forward bf16 per-slice rel errs", slices)
    assert max(slices["trans"], slices["rot6d"], slices["betas"]) < TOLBF


def test_view_swap_symmetry_and_zero_decoder(net32, copenet_sd, dev):
    """SURVEY §8c (vi)/(vii) on the GPU path."""
    torch.manual_seed(3)
    B = 3
    xf0, xf1 = torch.randn(B, 2048, device=dev), torch.randn(B, 2048, device=dev)
    bb0, bb1 = torch.rand(B, 3, device=dev), torch.rand(B, 3, device=dev)
    pos0, pos1 = torch.randn(B, 3, device=dev), torch.randn(B, 3, device=dev)
    a = net32.forward_ief(xf0, xf1, bb0, bb1, pos0, pos1, iters=3)
    b = net32.forward_ief(xf1, xf0, bb1, bb0, pos1, pos0, iters=3)
    for x, y in zip(a, (b[2], b[3], b[0], b[1])):
        assert torch.equal(x, y)


def test_forward_reg_and_step_match_oracle(net32, copenet_sd, dev):
    from oracle import copenet_ref
    torch.manual_seed(5)
    B = 4
    xf0, xf1 = torch.randn(B, 2048), torch.randn(B, 2048)
    bb0, bb1 = torch.rand(B, 3), torch.rand(B, 3)
    pose0, pose1 = torch.randn(B, 135) * 0.5, torch.randn(B, 135) * 0.5
    s0, s1 = torch.randn(B, 10) * 0.5, torch.randn(B, 10) * 0.5
    with torch.no_grad():
        want = copenet_ref.forward_reg(copenet_sd, xf0, xf1, bb0, bb1, pose0[:, :3], pose1[:, :3], pose0[:, 3:9],
                                       pose1[:, 3:9], pose0[:, 9:], pose1[:, 9:], s0, s1)
    d = lambda t: t.to(dev)
    got = net32.forward_reg(d(xf0), d(xf1), d(bb0), d(bb1), d(pose0[:, :3]), d(pose1[:, :3]), d(pose0[:, 3:9]),
                            d(pose1[:, 3:9]), d(pose0[:, 9:]), d(pose1[:, 9:]), d(s0), d(s1))
    for g_, w_ in zip(got, want):
        assert (pose_err(g_, w_) if g_.shape[1] == 135 else rel_err(g_.cpu().numpy(), w_.numpy())) < TOL32
    # single-view step with the partner state supplied by the caller == the same numbers
    partner0 = torch.cat([pose1[:, 9:], s1], 1)
    p, s = net32.regressor_step(d(xf0), d(bb0), d(pose0), d(s0), d(partner0))
    assert pose_err(p, want[0]) < TOL32 and rel_err(s.cpu().numpy(), want[1].numpy()) < TOL32


# ------------------------------------------------------------------------------------------------ SMPL-X + geometry
def _rand_rot(n, gen):
    from oracle import geometry_ref
    return geometry_ref.rot6d_to_rotmat(torch.randn(n, 6, generator=gen))


def test_smplx_forward_matches_oracle(body, smplx_model, dev):
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(11)
    B = 5
    betas = torch.randn(B, 10, generator=gen)
    bp = _rand_rot(B * 21, gen).view(B, 21, 3, 3)
    go = _rand_rot(B, gen).view(B, 1, 3, 3)
    tr = torch.randn(B, 3, generator=gen)
    want_v, want_j = smplx_ref.smplx_forward(smplx_model, betas, bp, global_orient=go, transl=tr)
    out = body.forward(betas=betas.to(dev), body_pose=bp.to(dev), global_orient=go.to(dev), transl=tr.to(dev),
                       pose2rot=False)
    assert out.vertices.shape == (B, 10475, 3) and out.joints.shape == (B, 127, 3)
    ev, ej = rel_err(out.vertices.cpu().numpy(), want_v.numpy()), rel_err(out.joints.cpu().numpy(), want_j.numpy())
    print("smplx rel err verts %.3e joints %.3e" % (ev, ej))
    assert ev < TOL32 and ej < TOL32
    # the reference's own call: identity global_orient, zero transl
    eye = torch.eye(3).expand(B, 1, 3, 3)
    want_v, want_j = smplx_ref.smplx_forward(smplx_model, betas, bp, global_orient=eye, transl=torch.zeros(B, 3))
    out = body.forward(betas=betas.to(dev), body_pose=bp.to(dev), global_orient=eye.contiguous().to(dev),
                       transl=torch.zeros(B, 3, device=dev), pose2rot=False)
    assert rel_err(out.vertices.cpu().numpy(), want_v.numpy()) < TOL32
    assert rel_err(out.joints.cpu().numpy(), want_j.numpy()) < TOL32


@pytest.mark.parametrize("cut", [1, 4])                        # set_fused(1): the default; 4: joints stage inside the kernel
@pytest.mark.parametrize("B", [3, 32, 77])
def test_smplx_fused_lbs_matches_two_kernel_path(body, smplx_model, dev, B, cut):
    """smplx_lbs_fused_kernel (blend-shape contraction + skinning in one kernel, v_posed on chip) against the two-kernel path
    (contraction GEMM -> v_posed in HBM -> skinning kernel) and the CPU oracle: global orient, translation, expression; B = 3 /
    32 / 77 bodies = a partly filled body group, exactly one, and a ragged third one."""
    from oracle import geometry_ref, smplx_ref
    gen = torch.Generator().manual_seed(40 + B)
    betas, expr = torch.randn(B, 10, generator=gen), torch.randn(B, 10, generator=gen) * 0.5
    R = geometry_ref.rot6d_to_rotmat(torch.randn(B * 22, 6, generator=gen)).reshape(B, 22, 3, 3)
    tr = torch.randn(B, 3, generator=gen)
    kw = dict(betas=betas.to(dev), expression=expr.to(dev), body_pose=R[:, 1:].to(dev), global_orient=R[:, :1].to(dev),
              transl=tr.to(dev), pose2rot=False)
    try:
        body.set_fused(0)
        two = body.forward(**kw)
        v2, j2 = two.vertices.clone(), two.joints.clone()
        body.set_fused(cut)
        one = body.forward(**kw)
    finally:
        body.set_fused(1)
    assert torch.isfinite(one.vertices).all() and torch.isfinite(one.joints).all()
    assert rel_err(one.vertices.cpu().numpy(), v2.cpu().numpy()) < 2e-6
    assert rel_err(one.joints.cpu().numpy(), j2.cpu().numpy()) < 2e-6
    want_v, want_j = smplx_ref.smplx_forward(smplx_model, betas, R[:, 1:], global_orient=R[:, :1], transl=tr, expression=expr)
    assert rel_err(one.vertices.cpu().numpy(), want_v.numpy()) < TOL32
    assert rel_err(one.joints.cpu().numpy(), want_j.numpy()) < TOL32
    # the extra joints are vertices of the mesh: the side buffer must hand the joints kernel the same v_posed
    ev = torch.as_tensor(smplx_model["extra_joint_verts"]).long()
    assert rel_err(one.joints[:, 55:76].cpu().numpy(), one.vertices[:, ev.to(dev)].cpu().numpy()) < 1e-6


@pytest.mark.parametrize("mode", [1, 4])                       # 4: joints stage inside the kernel (hand-off between workgroups)
def test_smplx_fused_soak(body, smplx_model, dev, mode):
    """Soak of the fused contraction + skinning kernel (an intermittent, timing-dependent wrong vertex -- about one
    in 10^4, lanes 48-63 -- appeared in an SLP-vectorised build of this kernel; a single forward per body count cannot see a
    recurrence): 120 forwards of 512 bodies, each compared ELEMENT-WISE against the two-kernel path's vertices, with a second
    stream keeping the memory system busy on every other repeat so the timing varies.  Every repeat must be clean."""
    from oracle import geometry_ref
    B = 512
    gen = torch.Generator().manual_seed(40 + B)
    betas, expr = torch.randn(B, 10, generator=gen), torch.randn(B, 10, generator=gen) * 0.5
    R = geometry_ref.rot6d_to_rotmat(torch.randn(B * 22, 6, generator=gen)).reshape(B, 22, 3, 3)
    tr = torch.randn(B, 3, generator=gen)
    kw = dict(betas=betas.to(dev), expression=expr.to(dev), body_pose=R[:, 1:].to(dev), global_orient=R[:, :1].to(dev),
              transl=tr.to(dev), pose2rot=False)
    try:
        body.set_fused(0)
        o2 = body.forward(**kw)
        v2, j2 = o2.vertices.clone(), o2.joints.clone()
    finally:
        body.set_fused(1)
    noise = torch.empty(64 << 20, dtype=torch.float32, device=dev)      # 256 MiB: a copy stream beside the kernel
    side = torch.cuda.Stream()
    bad_runs, worst = 0, 0.0
    for rep in range(120):
        if rep & 1:
            with torch.cuda.stream(side):
                noise.add_(1.0)
        try:
            body.set_fused(mode)
            o1 = body.forward(**kw)
        finally:
            body.set_fused(1)
        v1 = o1.vertices
        # (mode 4: the joints come from the body group's LAST workgroup, across a write-through / acquire hand-off: every word
        # of them is checked on every repeat, under even and uneven memory load)
        err = max(float((v1 - v2).abs().max()), float((o1.joints - j2).abs().max()))
        worst = max(worst, err)
        bad_runs += err > 2e-5                              # vertices are O(1): fp32 re-association stays below 1e-6
    torch.cuda.synchronize()
    print("fused LBS soak: worst |diff| %.3e over 120 runs" % worst)
    assert bad_runs == 0, "%d of 120 repeats differ from the two-kernel path (worst %.3e)" % (bad_runs, worst)


def test_smplx_coefficient_padding_is_rewritten_every_call(body, smplx_model, dev):
    """The coefficient rows come from a raw allocation: with the workspace poisoned (0xFF = NaN patterns) a forward with hand /
    face poses (K = 512: the contraction multiplies the 6 pad coefficients by zero directions) and a body-only forward (fused
    kernel, K = 256) must both stay finite and equal the oracle -- i.e. every slot that is read was rewritten, both bf16 halves."""
    from airpose_amd import _native as Nn
    from oracle import geometry_ref, smplx_ref
    gen = torch.Generator().manual_seed(61)
    B = 5
    betas = torch.randn(B, 10, generator=gen)
    R = geometry_ref.rot6d_to_rotmat(torch.randn(B * 22, 6, generator=gen)).reshape(B, 22, 3, 3)
    lh = geometry_ref.rot6d_to_rotmat(torch.randn(B * 15, 6, generator=gen)).reshape(B, 15, 3, 3)
    h = body._native(dev)
    for hands in (True, False):
        Nn.check(Nn.lib().ap_smplx_debug_poison_workspace(h, 64), "poison")
        kw = dict(betas=betas.to(dev), body_pose=R[:, 1:].to(dev), global_orient=R[:, :1].to(dev), pose2rot=False)
        if hands:
            kw["left_hand_pose"] = lh.to(dev)
        out = body.forward(**kw)
        assert torch.isfinite(out.vertices).all() and torch.isfinite(out.joints).all(), hands
        want_v, want_j = smplx_ref.smplx_forward(smplx_model, betas, R[:, 1:], global_orient=R[:, :1],
                                                 left_hand_pose=lh if hands else None)
        assert rel_err(out.vertices.cpu().numpy(), want_v.numpy()) < TOL32
        assert rel_err(out.joints.cpu().numpy(), want_j.numpy()) < TOL32


def test_smplx_split_bf16_blend_matches_fp32_blend(body, smplx_model, dev):
    """The blend-shape contraction on the bf16 matrix pipe (split-bf16 operands, four-term products; the default)
    against the exact fp32 MFMA chain: <= 1e-5 of the vertex scale (measured ~1e-7), both <= 1e-4 of the oracle."""
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(13)
    B = 6
    betas, expr = torch.randn(B, 10, generator=gen) * 2, torch.randn(B, 10, generator=gen)
    bp = _rand_rot(B * 21, gen).view(B, 21, 3, 3)
    lh = _rand_rot(B * 15, gen).view(B, 15, 3, 3)
    kw = dict(betas=betas.to(dev), body_pose=bp.to(dev), expression=expr.to(dev), left_hand_pose=lh.to(dev), pose2rot=False)
    want_v, _ = smplx_ref.smplx_forward(smplx_model, betas, bp, expression=expr, left_hand_pose=lh)
    try:
        body.set_blend_precision("fp32")
        v32 = body.forward(**kw).vertices.cpu()
    finally:
        body.set_blend_precision("bf16x2")
    vx2 = body.forward(**kw).vertices.cpu()
    e = rel_err(vx2.numpy(), v32.numpy())
    print("split-bf16 blend vs fp32 blend: %.3e; vs oracle %.3e / %.3e" % (e, rel_err(vx2.numpy(), want_v.numpy()),
                                                                       rel_err(v32.numpy(), want_v.numpy())))
    assert e < 1e-5
    assert rel_err(vx2.numpy(), want_v.numpy()) < TOL32 and rel_err(v32.numpy(), want_v.numpy()) < TOL32


def test_smplx_hands_face_expression(body, smplx_model, dev):
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(12)
    B = 2
    betas, expr = torch.randn(B, 10, generator=gen), torch.randn(B, 10, generator=gen)
    bp = _rand_rot(B * 21, gen).view(B, 21, 3, 3)
    jaw = _rand_rot(B, gen).view(B, 1, 3, 3)
    lh = _rand_rot(B * 15, gen).view(B, 15, 3, 3)
    want_v, want_j = smplx_ref.smplx_forward(smplx_model, betas, bp, expression=expr, jaw_pose=jaw, left_hand_pose=lh)
    out = body.forward(betas=betas.to(dev), body_pose=bp.to(dev), expression=expr.to(dev), jaw_pose=jaw.to(dev),
                       left_hand_pose=lh.to(dev), pose2rot=False)
    assert rel_err(out.vertices.cpu().numpy(), want_v.numpy()) < TOL32
    assert rel_err(out.joints.cpu().numpy(), want_j.numpy()) < TOL32


def test_smplx_identity_is_template(body, smplx_model, dev):
    eye = torch.eye(3, device=dev).expand(1, 21, 3, 3).contiguous()
    out = body.forward(betas=torch.zeros(1, 10, device=dev), body_pose=eye, pose2rot=False)
    assert np.allclose(out.vertices[0].cpu().numpy(), smplx_model["v_template"], atol=2e-6)
    assert np.allclose(out.joints[0, :55].cpu().numpy(), smplx_model["J_regressor"] @ smplx_model["v_template"], atol=2e-6)


def test_geometry_helpers_match_golden(golden, dev):
    from airpose_amd import geometry, utils
    g = golden["geometry"]
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    R = geometry.rot6d_to_rotmat(t("rot6d_in"))
    assert np.allclose(R.cpu().numpy(), g["rot6d_out"], atol=1e-6)
    out = geometry.perspective_projection(t("proj_points"), torch.eye(3, device=dev).expand(3, 3, 3),
                                          torch.zeros(3, 3, device=dev), [1475, 1475], t("proj_center").unsqueeze(0))
    assert rel_err(out.cpu().numpy(), g["proj_out"]) < 1e-6
    out = geometry.perspective_projection(t("proj_points"), t("proj_rt_R"),
                                          t("proj_rt_t") + torch.tensor([0, 0, 5.0], device=dev), [1000.0, 1100.0],
                                          t("proj_center"))
    # random R, t put a few points near z = 0, where x/z amplifies the last-bit differences of R X + t
    assert rel_err(out.cpu().numpy(), g["proj_rt_out"]) < 1e-4
    v, j, _, _ = utils.transform_smpl(t("tf_mat"), t("tf_verts"), t("tf_joints"))
    assert rel_err(v.cpu().numpy(), g["tf_verts_out"]) < 1e-6 and rel_err(j.cpu().numpy(), g["tf_joints_out"]) < 1e-6


def test_singleview_on_gpu_matches_reference(golden, dev):
    """copenet_singleview baseline on the GPU (ap_singleview_fwd) vs the imported reference's forward."""
    from airpose_amd import copenet_singleview_model, weights as W
    g = golden["singleview_b1"]
    sd = W.to_torch(W.copenet_state_dict(int(g["weights_seed"]), MEAN_PARAMS, variant="singleview"))
    net = copenet_singleview_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    assert list(net.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    net.load_state_dict(sd)
    net.to(dev)
    inp = W.synthetic_inputs(int(g["inputs_seed"]), 1)
    pos = torch.from_numpy(g["init_position"]).to(dev)
    pose, betas = net(torch.from_numpy(inp["im0"]).to(dev), torch.from_numpy(inp["bb0"]).to(dev), pos, iters=3)
    assert pose_err(pose, g["pose"]) < TOL32 and rel_err(betas.cpu().numpy(), g["betas"]) < TOL32
    netb = copenet_singleview_model.getcopenet(MEAN_PARAMS, precision="bf16").eval()
    netb.load_state_dict(sd)
    netb.to(dev)
    pose_b, _ = netb(torch.from_numpy(inp["im0"]).to(dev), torch.from_numpy(inp["bb0"]).to(dev), pos, iters=3)
    assert pose_err(pose_b, g["pose"]) < TOLBF
    with pytest.raises(RuntimeError):      # a two-view entry point on a single-view handle is an error, not a fallback
        netb.forward_feat_ext(torch.zeros(1, 3, 224, 224, device=dev)) and None
        from airpose_amd import _native as Nn
        z = torch.zeros(1, 2048, device=dev)
        Nn.check(Nn.lib().ap_regressor_fwd(netb._native(dev), *[ctypes.c_void_p(z.data_ptr())] * 6, None, 0, None, 0, None, 0,
                                           None, 0, 1, 1, *[ctypes.c_void_p(z.data_ptr())] * 4, None), "ap_regressor_fwd")


def test_muhmr_on_gpu_matches_reference(golden, dev):
    """muhmr two-view baseline on the GPU (ap_muhmr_fwd: camera in the translation slot of the two-view kernels) vs the
    imported reference's forward; caller-supplied initial state vs the default one."""
    from airpose_amd import muhmr_model, weights as W
    g = golden["muhmr_b1"]
    sd = W.to_torch(W.copenet_state_dict(int(g["weights_seed"]), MEAN_PARAMS, variant="muhmr"))
    net = muhmr_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    assert list(net.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    net.load_state_dict(sd)
    net.to(dev)
    inp = W.synthetic_inputs(int(g["inputs_seed"]), 1)
    x0, x1 = torch.from_numpy(inp["im0"]).to(dev), torch.from_numpy(inp["im1"]).to(dev)
    out = net(x0, x1, iters=3)
    for got, key in zip(out, ("pose0", "betas0", "cam0", "pose1", "betas1", "cam1")):
        assert rel_err(got.cpu().numpy(), g[key]) < TOL32, key
    same = net(x0, x1, init_cam0=sd["init_cam"].to(dev), init_cam1=sd["init_cam"].to(dev),
               init_theta0=sd["init_pose"][:, :132].to(dev), init_shape1=sd["init_shape"].to(dev), iters=3)
    for a, b in zip(out, same):
        assert torch.equal(a, b)


def test_copenet_sep_matches_reference(golden, dev):
    """copenet_sep (two weight sets, asymmetric cross-view step) on the GPU vs the imported reference's forward."""
    from airpose_amd import copenet_sep_model, weights as W
    g, gs = golden["copenet_b2"], golden["copenet_sep_b2"]
    net = copenet_sep_model.getcopenet_sep(MEAN_PARAMS, precision="fp32")
    assert list(net.state_dict().keys()) == [str(k) for k in gs["state_dict_keys"]]
    net.copenet0.load_state_dict(W.to_torch(W.copenet_state_dict(int(gs["weights_seed0"]), MEAN_PARAMS)))
    net.copenet1.load_state_dict(W.to_torch(W.copenet_state_dict(int(gs["weights_seed1"]), MEAN_PARAMS)))
    net.eval().to(dev)
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    pos = t("init_position")
    for it in (1, 3):
        out = net.forward_ief(t("xf0"), t("xf1"), t("bb0"), t("bb1"), pos, pos, iters=it)
        for got, key in zip(out, ("pose0", "betas0", "pose1", "betas1")):
            assert rel_err(got.cpu().numpy(), gs["%s_it%d" % (key, it)]) < TOL32, (key, it)


def test_preprocess_crops_matches_oracle(dev):
    """GPU input pipeline (crop, letter-box bilinear resize, /255, normalise) vs the oracle restatement: up- and
    down-scaling, tall / wide / square crops, crops touching the frame border, per-sample and shared frames."""
    from airpose_amd.utils import preprocess_crops
    from oracle import preprocess_ref as P
    rs = np.random.RandomState(9)
    frames = (rs.rand(5, 270, 480, 3) * 255).astype(np.uint8)
    crops = np.array([[0, 270, 0, 480], [10, 110, 30, 80], [100, 212, 200, 424], [5, 229, 7, 231], [200, 270, 400, 480]])
    img, scale, pad = preprocess_crops(torch.from_numpy(frames).to(dev), torch.from_numpy(crops))
    for i in range(5):
        want, s, p = P.preprocess(frames[i], tuple(crops[i]))
        assert abs(scale[i].item() - s) < 1e-6 and pad[i].tolist() == p
        assert np.abs(img[i].cpu().numpy() - want).max() < 5e-5, i
    img1, _, _ = preprocess_crops(torch.from_numpy(frames[2]).to(dev), torch.from_numpy(crops[2:3]))
    assert torch.equal(img1[0], img[2])
    with pytest.raises(RuntimeError):
        preprocess_crops(torch.from_numpy(frames), torch.from_numpy(crops))                 # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        preprocess_crops(torch.from_numpy(frames).to(dev), torch.tensor([[0, 300, 0, 10]] * 5))   # outside the frame


PREPROCESS_CROPS = [  # (y0, y1, x0, x1) on a 1080 x 1920 frame
    (0, 1080, 0, 1920), (856, 1080, 1696, 1920),            # the whole frame; a 224 x 224 crop in the bottom right corner
    (300, 524, 800, 1024),                                   # exactly 224 x 224: an identity resample
    (0, 1, 0, 1), (5, 7, 9, 11), (100, 101, 200, 300), (100, 102, 200, 201), (500, 700, 1000, 1001), (40, 42, 60, 284),   # h or w of 1, 2
    (10, 235, 20, 243), (1, 450, 7, 10), (600, 1049, 3, 6),  # 225 x 223, 449 x 3: int(scale w) truncates
    (30, 254, 50, 271), (200, 300, 400, 437), (7, 230, 1000, 1223), (0, 333, 1700, 1920),   # odd padding (221, 82 -> 83 columns; 223; 148)
]


@pytest.mark.parametrize("bgr", [True, False])
def test_preprocess_crops_geometry_sweep(dev, bgr):
    """The input pipeline at the production frame size over crop geometries: one- and two-pixel crops, the identity resample,
    sizes at which int(scale w) truncates, odd padding; both channel orders; one shared frame and a frame per sample."""
    from airpose_amd.utils import preprocess_crops
    from oracle import preprocess_ref as P
    rs = np.random.RandomState(19)
    frame = (rs.rand(1080, 1920, 3) * 255).astype(np.uint8)
    crops = np.array(PREPROCESS_CROPS)
    as_bgr = lambda f: f if bgr else np.ascontiguousarray(f[:, :, ::-1])       # the oracle takes cv2.imread's order
    img, scale, pad = preprocess_crops(torch.from_numpy(frame).to(dev), torch.from_numpy(crops), bgr=bgr)
    for i, c in enumerate(PREPROCESS_CROPS):
        want, s, p = P.preprocess(as_bgr(frame), c)
        assert abs(scale[i].item() - s) < 1e-6 * max(1.0, s) and pad[i].tolist() == p, (i, c)
        assert np.abs(img[i].cpu().numpy() - want).max() < 5e-5, (i, c)
    # identity resample: the normalised pixels themselves, to fp32 rounding (three roundings of values below 4.5)
    y0, y1, x0, x1 = PREPROCESS_CROPS[2]
    px = frame[y0:y1, x0:x1, ::-1] if bgr else frame[y0:y1, x0:x1]
    exact = (px.astype(np.float64).transpose(2, 0, 1) / 255.0 - P.MEAN[:, None, None]) / P.STD[:, None, None]
    assert pad[2].tolist() == [0, 0] and np.abs(img[2].cpu().numpy() - exact).max() < 1e-6
    # a frame per sample: the same crops on four different frames
    sel = [0, 3, 9, 12]
    frames = (rs.rand(len(sel), 1080, 1920, 3) * 255).astype(np.uint8)
    img4, scale4, pad4 = preprocess_crops(torch.from_numpy(frames).to(dev), torch.from_numpy(crops[sel]), bgr=bgr)
    for j, i in enumerate(sel):
        want, s, p = P.preprocess(as_bgr(frames[j]), PREPROCESS_CROPS[i])
        assert abs(scale4[j].item() - s) < 1e-6 * max(1.0, s) and pad4[j].tolist() == p, (j, i)
        assert np.abs(img4[j].cpu().numpy() - want).max() < 5e-5, (j, i)


def test_rotation_matrix_to_angle_axis_matches_oracle(dev):
    """pred_angles conversion (tgm 0.1.2 semantics): all four trace branches, (N,3,3) and the caller's (N,3,4) form."""
    from airpose_amd.geometry import rotation_matrix_to_angle_axis
    from oracle import geometry_ref as G
    g = torch.Generator().manual_seed(3)
    aa = torch.randn(4000, 3, generator=g) * 1.6                       # angles up to ~2 pi: exercises every branch
    R = G.batch_rodrigues_quat(aa.double()).float()
    R = torch.cat([R, torch.eye(3).unsqueeze(0), torch.diag(torch.tensor([1.0, -1.0, -1.0])).unsqueeze(0)], 0)
    ref = G.rotation_matrix_to_angle_axis(R.double())
    got3 = rotation_matrix_to_angle_axis(R.to(dev)).cpu().double()
    got4 = rotation_matrix_to_angle_axis(torch.cat([R, torch.zeros(R.shape[0], 3, 1)], 2).to(dev)).cpu().double()
    assert torch.equal(got3, got4)
    # angle-axis is discontinuous at |angle| = pi (axis sign): compare the rotations they encode there
    err = (got3 - ref).abs().max(1).values
    near_pi = (ref.norm(dim=1) > 3.13)
    assert err[~near_pi].max() < 2e-5
    assert (G.batch_rodrigues_quat(got3[near_pi]) - G.batch_rodrigues_quat(ref[near_pi])).abs().max() < 1e-4


def test_batch_rodrigues_both_forms(golden, dev):
    """Axis-angle -> rotation matrix: the reference's own geometry.batch_rodrigues against the golden vectors of the imported
    reference, and the body-model package's lbs.batch_rodrigues against the CPU oracle and known answers."""
    from airpose_amd import geometry, lbs
    from oracle import fitting_ref as Fr
    g = golden["geometry"]
    got = geometry.batch_rodrigues(torch.from_numpy(g["rodrigues_in"]).to(dev)).cpu().numpy()
    assert np.allclose(got, g["rodrigues_out"], atol=1e-6)
    gen = torch.Generator().manual_seed(8)
    aa = torch.cat([torch.randn(3000, 3, generator=gen) * 1.5, torch.zeros(1, 3),
                    torch.tensor([[0.0, 0.0, np.pi / 2]]), torch.randn(8, 3, generator=gen) * 1e-6], 0)
    want = Fr.lbs_batch_rodrigues(aa.double())
    R = lbs.batch_rodrigues(aa.to(dev)).cpu().double()
    assert (R - want).abs().max() < 2e-6
    assert torch.allclose(R[3000], torch.eye(3, dtype=torch.float64), atol=1e-7)                       # zero vector -> I
    assert torch.allclose(R[3001], torch.tensor([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=torch.float64), atol=1e-6)
    assert (torch.bmm(R, R.transpose(1, 2)) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-5    # rotations
    with pytest.raises(RuntimeError):
        lbs.batch_rodrigues(aa)                                                                        # CPU tensor: no fallback


def test_smplx_forward_axis_angle_inputs(body, smplx_model, dev):
    """SMPLX.forward(pose2rot=True) with use_pca=False, flat_hand_mean=True: axis-angle pose inputs give what the
    rotation-matrix call gives on lbs.batch_rodrigues of them, and match the CPU oracle."""
    from airpose_amd import lbs
    from oracle import fitting_ref as Fr
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(13)
    B = 3
    betas = torch.randn(B, 10, generator=gen)
    bp, go, jaw = torch.randn(B, 63, generator=gen) * 0.6, torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen) * 0.3
    lh = torch.randn(B, 45, generator=gen) * 0.4
    tr = torch.randn(B, 3, generator=gen)
    old = (body.use_pca, body.flat_hand_mean)
    body.use_pca, body.flat_hand_mean = False, True
    try:
        out = body.forward(betas=betas.to(dev), body_pose=bp.to(dev), global_orient=go.to(dev), jaw_pose=jaw.to(dev),
                           left_hand_pose=lh.to(dev), transl=tr.to(dev), pose2rot=True)
    finally:
        body.use_pca, body.flat_hand_mean = old
    rm = lambda t, n: lbs.batch_rodrigues(t.to(dev).reshape(-1, 3)).reshape(B, n, 3, 3)
    ref = body.forward(betas=betas.to(dev), body_pose=rm(bp, 21), global_orient=rm(go, 1), jaw_pose=rm(jaw, 1),
                       left_hand_pose=rm(lh, 15), transl=tr.to(dev), pose2rot=False)
    assert torch.equal(out.vertices, ref.vertices) and torch.equal(out.joints, ref.joints)
    cr = lambda t, n: Fr.lbs_batch_rodrigues(t.reshape(-1, 3)).reshape(B, n, 3, 3)
    want_v, want_j = smplx_ref.smplx_forward(smplx_model, betas, cr(bp, 21), global_orient=cr(go, 1), jaw_pose=cr(jaw, 1),
                                             left_hand_pose=cr(lh, 15), transl=tr)
    assert rel_err(out.vertices.cpu().numpy(), want_v.numpy()) < TOL32
    assert rel_err(out.joints.cpu().numpy(), want_j.numpy()) < TOL32


@pytest.mark.parametrize("use_pca,flat", [(True, False), (True, True), (False, False)])
def test_smplx_forward_hand_pca_and_mean_pose(body, smplx_model, dev, use_pca, flat):
    """The upstream default calling convention of SMPLX.forward (pose2rot=True; the reference's dataset code,
    aerialpeople.py:56-64): hands as num_pca_comps PCA coefficients through hands_components, the model file's mean hand
    pose added unless flat_hand_mean, un-supplied hands = the mean pose -- against the oracle's restatement of smplx 0.1.28."""
    from oracle import smplx_ref
    gen = torch.Generator().manual_seed(29)
    B = 4
    betas, bp = torch.randn(B, 10, generator=gen), torch.randn(B, 63, generator=gen) * 0.5
    go, reye = torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen) * 0.2
    lh = torch.randn(B, 6 if use_pca else 45, generator=gen) * 0.5
    old = (body.use_pca, body.flat_hand_mean, body.num_pca_comps)
    body.use_pca, body.flat_hand_mean, body.num_pca_comps = use_pca, flat, 6
    try:
        out = body.forward(betas=betas.to(dev), body_pose=bp.to(dev), global_orient=go.to(dev), reye_pose=reye.to(dev),
                           left_hand_pose=lh.to(dev), pose2rot=True)                       # right hand: not supplied
        with pytest.raises(RuntimeError):                                               # the other convention's width
            body.forward(betas=betas.to(dev), body_pose=bp.to(dev), left_hand_pose=torch.zeros(B, 45 if use_pca else 6, device=dev),
                         pose2rot=True)
    finally:
        body.use_pca, body.flat_hand_mean, body.num_pca_comps = old
    want_v, want_j = smplx_ref.smplx_forward_axis_angle(smplx_model, betas, bp, global_orient=go, reye_pose=reye, left_hand_pose=lh,
                                                        use_pca=use_pca, num_pca_comps=6, flat_hand_mean=flat)
    assert rel_err(out.vertices.cpu().numpy(), want_v.numpy()) < TOL32
    assert rel_err(out.joints.cpu().numpy(), want_j.numpy()) < TOL32


def test_whole_pipeline_fp32_matches_oracle(net32, body, copenet_sd, copenet_inputs, smplx_model, dev):
    """BASELINE config 2 at test size: regressed theta/beta, 3-D joints/vertices, 2-D projection within 1e-4."""
    from airpose_amd import pipeline
    from oracle import pipeline_ref
    inp = copenet_inputs
    with torch.no_grad():
        want = pipeline_ref.infer(copenet_sd, smplx_model, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"],
                                  inp["intr0"], inp["intr1"])
    got = pipeline.TwoViewInference(net32, body)({k: v.to(dev) for k, v in inp.items()}, want_angles=True)
    for k in sorted(want):
        for nm, e in key_errs(k, got[k].cpu().numpy(), want[k].numpy()).items():
            print("%-28s rel err %.3e" % (nm, e))
            assert e < TOL32, nm


@pytest.mark.parametrize("wseed,wide", [(7, False), (99, False), (20240901, True)])
def test_f16_parity_on_other_checkpoints(body, smplx_model, dev, wseed, wide):
    """The 1e-4 bar of the fp16-storage throughput mode across checkpoints, not on the one synthetic checkpoint (seed 20240901,
    BatchNorm gamma / var ~ U(.5, 1.5)) the other parity numbers rest on: 16 pairs each, slice-max error of every output against
    the fp32 CPU oracle.
      * two more weight seeds of the same family: fp16 storage stays below 1e-4 (measured 2.6e-5 / 3.8e-5);
      * a second BatchNorm-statistics range (gamma, var ~ U(.25, 2)): that checkpoint is ~30x worse conditioned -- the exact-fp32
        mode itself lands at 4e-6 instead of 3e-7, split-bf16 at 2.4e-5 instead of 7.5e-7 -- and 11 significand bits of storage
        do NOT hold the bar there (1.8e-3; bf16: 1e-2).  What is asserted for it: the split-bf16 parity mode holds 1e-4, fp16
        storage stays within 5e-3 and finite (the range sentinel silent).  bench.py reports the same sweep for every mode."""
    from airpose_amd import copenet_model, pipeline
    from airpose_amd import weights as W
    from oracle import pipeline_ref
    sd = W.to_torch(W.copenet_state_dict(wseed, MEAN_PARAMS, wide_bn=wide))
    inp = {k: torch.from_numpy(v) for k, v in W.synthetic_inputs(31 + wseed % 1000, 16).items()}
    with torch.no_grad():
        want = pipeline_ref.infer(sd, smplx_model, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], inp["intr0"], inp["intr1"])
    gin = {k: v.to(dev) for k, v in inp.items()}
    for prec, bar in (("f16", 5e-3 if wide else 1e-4), ("bf16x2", TOL32)):
        net = copenet_model.getcopenet(MEAN_PARAMS, precision=prec).eval()
        net.load_state_dict(sd)
        got = pipeline.TwoViewInference(net, body)(gin)
        worst = 0.0
        for k in sorted(want):
            if k not in got:
                continue
            for nm, e in key_errs(k, got[k].float().cpu().numpy(), want[k].numpy()).items():
                worst = max(worst, e)
                assert e < bar, (prec, nm, e)
        if prec == "f16":
            net.range_status()
        print("%s seed %d wide %d: worst slice %.3e" % (prec, wseed, wide, worst))
        del net


def test_test_mode_input_meshes_match_oracle(net32, body, copenet_sd, copenet_inputs, smplx_model, dev):
    """The rest of the reference's test-mode dict (copenet_twoview.py:258-279, 330-331, 342-343): the beta = 0 meshes
    placed at in_smpltrans, produced by the same native call as 2B more bodies; and nothing but the two C-ABI calls
    runs on the stream (the translation un-scale and the camera centres are inside ap_smplx_fwd_twoview)."""
    from airpose_amd import pipeline
    from oracle import pipeline_ref
    inp = copenet_inputs
    with torch.no_grad():
        want = pipeline_ref.infer(copenet_sd, smplx_model, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"],
                                  inp["intr0"], inp["intr1"], want_input_mesh=True)
    pipe = pipeline.TwoViewInference(net32, body)
    gin = {k: v.to(dev) for k, v in inp.items()}
    got = pipe(gin, want_angles=True, want_input_mesh=True)
    assert set(want) <= set(got)
    for k in sorted(want):
        for nm, e in key_errs(k, got[k].cpu().numpy(), want[k].numpy()).items():
            assert e < TOL32, (nm, e)
    assert torch.equal(got["in_smpltrans0"].cpu(), want["in_smpltrans0"])
    # the un-scale happened in place on the network's own output buffer, as in the reference (:214-218)
    assert got["pred_smpltrans0"].data_ptr() == got["pred_pose0"].data_ptr()
    assert abs(float(got["pred_pose0"][0, 2]) - float(want["pred_pose0"][0, 2])) < 1e-3 and float(got["pred_pose0"][0, 2]) > 1.0
    # without the input meshes the other outputs are bit-identical (same bodies, same kernels)
    plain = pipe(gin, want_angles=True)
    for k in plain:
        assert torch.equal(plain[k], got[k]), k


def test_full_size_properties_16bit(net16, body, dev):
    """BASELINE size (B = 256 pairs) in both 16-bit storage types -- fp16 is the configuration the bench headline is quoted on:
    size-independent properties instead of a CPU oracle run -- finite outputs, exact view-swap symmetry, rows identical to a
    B = 2 run of the same inputs, the fused layer1 kernels bitwise against the separate convolutions, and (fp16) a silent
    range sentinel."""
    netbf = net16
    from airpose_amd import pipeline
    from airpose_amd import weights as W
    B = 256
    small = W.synthetic_inputs(1234, 2)
    gen = torch.Generator(device="cpu").manual_seed(7)
    im0 = torch.randn(B, 3, 224, 224, generator=gen)
    im1 = torch.randn(B, 3, 224, 224, generator=gen)
    im0[:2], im1[:2] = torch.from_numpy(small["im0"]), torch.from_numpy(small["im1"])
    bb0, bb1 = torch.rand(B, 3, generator=gen), torch.rand(B, 3, generator=gen)
    bb0[:2], bb1[:2] = torch.from_numpy(small["bb0"]), torch.from_numpy(small["bb1"])
    intr = torch.tensor([[1475.0, 0, 960], [0, 1475.0, 540], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    d = lambda t: t.to(dev)
    pipe = pipeline.TwoViewInference(netbf, body)
    out = pipe({"im0": d(im0), "im1": d(im1), "bb0": d(bb0), "bb1": d(bb1), "intr0": d(intr), "intr1": d(intr)})
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    assert out["pred_vertices_cam0"].shape == (B, 10475, 3) and out["pred_j2d_cam1"].shape == (B, 127, 2)
    swp = pipe({"im0": d(im1), "im1": d(im0), "bb0": d(bb1), "bb1": d(bb0), "intr0": d(intr), "intr1": d(intr)})
    assert torch.equal(out["pred_pose0"], swp["pred_pose1"]) and torch.equal(out["pred_betas1"], swp["pred_betas0"])
    assert torch.equal(out["pred_j3d_cam0"], swp["pred_j3d_cam1"])
    two = pipe({"im0": d(im0[:2]), "im1": d(im1[:2]), "bb0": d(bb0[:2]), "bb1": d(bb1[:2]), "intr0": d(intr[:2]),
                "intr1": d(intr[:2])})
    assert pose_err(two["pred_pose0"], out["pred_pose0"][:2]) < 1e-6
    assert rel_err(two["pred_vertices_cam1"].cpu().numpy(), out["pred_vertices_cam1"][:2].cpu().numpy()) < 1e-6
    # the persistent fused layer1 kernels at full size (512 images = 32 tiles per workgroup, hand-counted waits under
    # full memory load) against the separate-convolution path: bit-identical, on repeated runs
    x = d(torch.cat([im0, im1]))
    try:
        netbf.set_fuse_block(0)
        ref = netbf.forward_feat_ext(x).clone()
    finally:
        netbf.set_fuse_block(1)
    for _ in range(3):
        assert torch.equal(netbf.forward_feat_ext(x), ref)
    netbf.range_status()                                     # fp16 storage: no trunk pass above left the fp16 range


def test_hmr_config1_on_gpu_matches_reference(golden, dev):
    """BASELINE config 0 (hmr single view, batch 1, 3 iterations) through ap_hmr_fwd vs the reference's output."""
    from airpose_amd import hmr_model
    from airpose_amd import weights as W
    g = golden["hmr_b1"]
    sd = W.to_torch(W.copenet_state_dict(int(g["weights_seed"]), MEAN_PARAMS, variant="hmr"))
    x = torch.from_numpy(W.synthetic_inputs(int(g["inputs_seed"]), 1)["im0"]).to(dev)
    net = hmr_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(sd, strict=True)
    rot, betas, cam = net(x, iters=3)
    assert rot.shape == (1, 22, 3, 3)
    errs = [rel_err(rot.cpu().numpy(), g["rotmat"]), rel_err(betas.cpu().numpy(), g["betas"]), rel_err(cam.cpu().numpy(), g["cam"])]
    print("hmr fp32 rel errs", errs)
    assert max(errs) < TOL32
    netb = hmr_model.getcopenet(MEAN_PARAMS, precision="bf16").eval()
    netb.load_state_dict(sd, strict=True)
    rotb, betasb, camb = netb(x, iters=3)
    assert rel_err(betasb.cpu().numpy(), g["betas"]) < TOLBF and rel_err(rotb.cpu().numpy(), g["rotmat"]) < TOLBF
    neth = hmr_model.getcopenet(MEAN_PARAMS, precision="f16").eval()      # fp16 storage: under north_star's bar
    neth.load_state_dict(sd, strict=True)
    roth, betash, camh = neth(x, iters=3)
    errh = [rel_err(roth.cpu().numpy(), g["rotmat"]), rel_err(betash.cpu().numpy(), g["betas"]), rel_err(camh.cpu().numpy(), g["cam"])]
    print("hmr f16 rel errs", errh)
    assert max(errh) < 1e-4


def test_errors_are_loud(net32, dev):
    with pytest.raises(RuntimeError):
        net32.forward_feat_ext(torch.zeros(1, 3, 224, 224))          # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        net32.forward_feat_ext(torch.zeros(1, 3, 200, 200, device=dev))
    net32.train()
    with pytest.raises(RuntimeError):
        net32.forward_feat_ext(torch.zeros(1, 3, 224, 224, device=dev))
    net32.eval()


@pytest.mark.parametrize("iters", [1, 2, 5])
@pytest.mark.parametrize("fuse", [1, 0])
def test_ief_iteration_counts_and_caller_initialisation(net32, copenet_sd, dev, iters, fuse):
    """forward(..., iters=k) for k other than 3, with caller-supplied init_theta / init_shape for one view only
    (model_copenet.py:121-136 accepts either per view), against the oracle's IEF loop."""
    from oracle import copenet_ref
    g = torch.Generator().manual_seed(100 + iters)
    B = 5
    xf0, xf1 = torch.randn(B, 2048, generator=g), torch.randn(B, 2048, generator=g)
    bb0, bb1 = torch.rand(B, 3, generator=g), torch.rand(B, 3, generator=g)
    pos0, pos1 = torch.randn(B, 3, generator=g) * 0.3, torch.randn(B, 3, generator=g) * 0.3
    theta1 = torch.randn(B, 144, generator=g) * 0.5          # caller-supplied for view 1 only; [:, :132] is used
    shape0 = torch.randn(B, 10, generator=g) * 0.5           # caller-supplied for view 0 only
    sd64 = {k: v.double() for k, v in copenet_sd.items() if v.is_floating_point()}
    want = copenet_ref.ief(sd64, xf0.double(), xf1.double(), bb0.double(), bb1.double(), pos0.double(), pos1.double(),
                           init_theta1=theta1.double(), init_shape0=shape0.double(), iters=iters)
    d = lambda t: t.to(dev)
    net32.set_fuse_ief(fuse)
    try:
        got = net32.forward_ief(d(xf0), d(xf1), d(bb0), d(bb1), d(pos0), d(pos1), init_theta1=d(theta1),
                                init_shape0=d(shape0), iters=iters)
    finally:
        net32.set_fuse_ief(1)
    for a, b in zip(got, want):
        assert rel_err(a.cpu().numpy(), b.numpy()) < TOL32


def test_trunk_across_the_chunk_boundary(netbf, dev):
    """More images than one depth-first pass takes (512): 515 images run as passes of 512 + 3; every row must equal
    the row of a small run (bf16 kernels are batch-invariant bit for bit)."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(6, 3, 224, 224, generator=g).to(dev)
    big = torch.cat([x[:3], torch.zeros(509, 3, 224, 224, device=dev), x[3:]])      # rows 0-2 and 512-514 carry data
    f_big = netbf.forward_feat_ext(big)
    f_small = netbf.forward_feat_ext(x)
    assert f_big.shape == (515, 2048)
    assert torch.equal(f_big[:3], f_small[:3]) and torch.equal(f_big[512:], f_small[3:])
    assert torch.equal(f_big[3], f_big[511])                 # two all-zero images


def test_malformed_inputs_raise(net32, body, dev):
    """Shape / dtype / device mistakes raise instead of computing on garbage (the reference would raise inside torch)."""
    z = lambda *s: torch.zeros(*s, device=dev)
    pos = z(2, 3)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        net32(z(2, 3, 224, 224), z(3, 3, 224, 224), z(2, 3), z(2, 3), pos, pos)               # view batch mismatch
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        net32(z(2, 3, 224, 224), z(2, 3, 224, 224), z(2, 4), z(2, 3), pos, pos)               # bb is (B, 3)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        net32(z(2, 3, 224, 224), z(2, 3, 224, 224), z(2, 3), z(2, 3), pos, pos, iters=0)      # at least one evaluation
    # (other floating dtypes are accepted and converted to float32 on the way in: host-side plumbing)
    assert net32.forward_feat_ext(torch.zeros(2, 3, 224, 224, device=dev, dtype=torch.float64)).dtype == torch.float32
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        body(betas=z(2, 10), body_pose=z(2, 20, 3, 3), global_orient=z(2, 1, 3, 3), pose2rot=False)   # 21 body joints
    eye = torch.eye(3, device=dev)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        body(betas=z(2, 11), body_pose=eye.expand(2, 21, 3, 3), global_orient=eye.expand(2, 1, 3, 3), pose2rot=False)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        body(betas=z(2, 10), body_pose=eye.expand(2, 21, 3, 3), global_orient=eye.expand(2, 1, 3, 3), transl=z(2, 4),
             pose2rot=False)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        net32.forward_ief(z(2, 2047), z(2, 2047), z(2, 3), z(2, 3), pos, pos)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        net32.regressor_step(z(2, 2048), z(2, 2), z(2, 135), z(2, 10), z(2, 136))


# ------------------------------------------------------------------------------------------------ AirPose+ fitting loop
@pytest.fixture(scope="module")
def fit_problem(smplx_model):
    from oracle import fitting_ref
    return fitting_ref.synthetic_problem(smplx_model, L=20, seed=77, dtype=torch.float64)


def test_fitting_gradients_match_autograd_oracle(fit_problem, body, smplx_model, dev):
    """One evaluation of the AirPose+ objective (BASELINE config 5): the hand-written adjoints of the GPU path against
    torch autograd on the fp64 oracle restatement, for every optimised quantity, at iteration 0 and at iteration 150
    (hip weights 2^-151, decoder backward active)."""
    from airpose_amd.fitting import AirPosePlusFitter
    from oracle import fitting_ref
    vp, init, data, _ = fit_problem
    fitter = AirPosePlusFitter(vp, body, dev)
    for it in (0, 150):
        _, want, _ = fitting_ref.loss_and_grads(vp, smplx_model, init, data, it)
        _, got = fitter.run(init, data["j2d"], data["robust"], data["intr"], data["extr"][:, :3], n_iters=1, first_iter=it,
                            switch_iter=0, lr=0.0, want_grad=True)
        for k in ("z", "phi0", "phi1", "tau0", "tau1", "beta"):
            e = rel_err(got[k].cpu().numpy(), want[k].numpy())
            print("it %3d d%-5s rel err %.3e" % (it, k, e))
            assert e < 2e-4, (it, k)


def test_fitting_trajectory_follows_oracle(fit_problem, body, smplx_model, dev):
    """40 Adam steps straddling the optimiser switch (rigid-only, then all parameters with a fresh Adam): the GPU loop
    stays on the oracle's trajectory and the objective decreases."""
    from airpose_amd.fitting import AirPosePlusFitter
    from oracle import fitting_ref
    vp, init, data, _ = fit_problem
    fitter = AirPosePlusFitter(vp, body, dev)
    got, hist = fitter.run(init, data["j2d"], data["robust"], data["intr"], data["extr"][:, :3], n_iters=40, switch_iter=20,
                           want_loss=True)
    old = fitting_ref.SWITCH_ITER
    fitting_ref.SWITCH_ITER = 20
    try:
        want, losses = fitting_ref.fit(vp, smplx_model, init, data, n_iters=40)
    finally:
        fitting_ref.SWITCH_ITER = old
    for k in ("z", "phi0", "phi1", "tau0", "tau1", "beta"):
        e = rel_err(got[k].cpu().numpy(), want[k].numpy())
        print("after 40 steps %-5s rel err %.3e" % (k, e))
        assert e < 5e-3, k
    assert hist[-1, :3].sum().item() < hist[0, :3].sum().item()


def test_fitting_at_the_size_of_config_5(body, smplx_model, dev):
    """BASELINE config 5 at ITS OWN size (64 frames were only ever timed): the 64-frame problem, 30 Adam steps
    straddling the optimiser switch against the fp64 autograd oracle; then the full 300 iterations of the bench: finite,
    bit-deterministic over two runs, and the windowed objective (means over 50 iterations) never rises by more than 5 %."""
    from airpose_amd.fitting import AirPosePlusFitter
    from oracle import fitting_ref
    vp, init, data, _ = fitting_ref.synthetic_problem(smplx_model, L=64, seed=78, dtype=torch.float64)
    fitter = AirPosePlusFitter(vp, body, dev)
    args = (data["j2d"], data["robust"], data["intr"], data["extr"][:, :3])
    got, hist = fitter.run(init, *args, n_iters=30, switch_iter=15, want_loss=True)
    old = fitting_ref.SWITCH_ITER
    fitting_ref.SWITCH_ITER = 15
    try:
        want, _ = fitting_ref.fit(vp, smplx_model, init, data, n_iters=30)
    finally:
        fitting_ref.SWITCH_ITER = old
    for k in ("z", "phi0", "phi1", "tau0", "tau1", "beta"):
        e = rel_err(got[k].cpu().numpy(), want[k].numpy())
        print("L = 64, after 30 steps %-5s rel err %.3e" % (k, e))
        assert e < 5e-3, k
    runs = [fitter.run(init, *args, n_iters=300, want_loss=True) for _ in range(2)]
    for k in ("z", "phi0", "phi1", "tau0", "tau1", "beta"):
        assert torch.isfinite(runs[0][0][k]).all(), k
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    loss = runs[0][1][:, :3].sum(1).cpu().numpy()
    assert np.isfinite(loss).all()
    win = loss.reshape(6, 50).mean(1)
    print("L = 64, 300 iterations: windowed objective", ["%.3f" % w for w in win])
    assert all(win[i + 1] <= win[i] * 1.05 for i in range(5)) and win[-1] < 0.5 * win[0]


# ------------------------------------------------------------------------------------------------ K > 4 bones per vertex
@pytest.mark.parametrize("max_bones", [6, 9])
def test_smplx_more_than_four_bones_per_vertex(max_bones, dev):
    """A real SMPL-X weight matrix may carry more than 4 non-zeros per vertex: max_bones = 6 selects
    smplx_skin_kernel<8>, max_bones = 9 the dynamic-K instantiation (api_smplx.hip picks K from the packed model).
    Both the plain SMPLX.forward and the fused pose6d -> LBS -> transform -> projection entry are checked."""
    from airpose_amd import smplx, smplx_model as SM
    from oracle import geometry_ref, smplx_ref
    md = SM.make_synthetic_model(4321, max_bones=max_bones)
    assert (md["lbs_weights"] != 0).sum(1).max() == max_bones
    b = smplx.SMPLX(model_data=md).to(dev)
    gen = torch.Generator().manual_seed(40 + max_bones)
    B = 3
    betas = torch.randn(B, 10, generator=gen)
    bp = _rand_rot(B * 21, gen).view(B, 21, 3, 3)
    go = _rand_rot(B, gen).view(B, 1, 3, 3)
    tr = torch.randn(B, 3, generator=gen)
    lh = _rand_rot(B * 15, gen).view(B, 15, 3, 3)
    want_v, want_j = smplx_ref.smplx_forward(md, betas, bp, global_orient=go, transl=tr, left_hand_pose=lh)
    out = b.forward(betas=betas.to(dev), body_pose=bp.to(dev), global_orient=go.to(dev), transl=tr.to(dev),
                    left_hand_pose=lh.to(dev), pose2rot=False)
    ev, ej = rel_err(out.vertices.cpu().numpy(), want_v.numpy()), rel_err(out.joints.cpu().numpy(), want_j.numpy())
    print("K=%d smplx rel err verts %.3e joints %.3e" % (max_bones, ev, ej))
    assert ev < TOL32 and ej < TOL32
    # fused entry (the caller slice of copenet_twoview.py:222-223,237-246,307-311)
    pose = torch.randn(B, 135, generator=gen)
    pose[:, 2] += 10.0
    cc = torch.tensor([[960.0, 540.0]]).expand(B, 2).contiguous()
    R = geometry_ref.rot6d_to_rotmat(pose[:, 3:].reshape(-1, 6)).view(B, 22, 3, 3)
    v, j = smplx_ref.smplx_forward(md, betas, R[:, 1:], global_orient=torch.eye(3).expand(B, 1, 3, 3),
                                   transl=torch.zeros(B, 3))
    want_vc = torch.einsum("bij,bvj->bvi", R[:, 0], v) + pose[:, None, :3]
    want_jc = torch.einsum("bij,bvj->bvi", R[:, 0], j) + pose[:, None, :3]
    want_2d = geometry_ref.perspective_projection(want_jc, torch.eye(3).expand(B, 3, 3), torch.zeros(B, 3),
                                                  [1475.0, 1475.0], cc.unsqueeze(0))
    o = b.forward_fused(pose.to(dev), betas.to(dev), cc.to(dev))
    for nm, got, want in (("vertices_cam", o["vertices_cam"], want_vc), ("j3d_cam", o["j3d_cam"], want_jc),
                          ("j2d_cam", o["j2d_cam"], want_2d)):
        e = rel_err(got.cpu().numpy(), want.numpy())
        print("K=%d fused %s rel err %.3e" % (max_bones, nm, e))
        assert e < TOL32, nm


# ------------------------------------------------------------------------------------------------ BASELINE config 4
def _view_split_worker(rank, world, port, out_dir):
    """One rank of the view-split topology (view `rank` of every pair) on the ONE leased GPU: 2-rank gloo group,
    host-staged all_gather of the 136-float partner state, the real ap_regressor_step on cuda:0."""
    import os
    import sys
    from conftest import MEAN_PARAMS as MP, REPO
    sys.path.insert(0, REPO)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from airpose_amd import copenet_model, dist as D
    from airpose_amd import weights as W
    g = np.load(os.path.join(REPO, "tests", "golden", "copenet_b2.npz"))
    d = torch.device("cuda", 0)
    sd = W.to_torch(W.copenet_state_dict(int(g["weights_seed"]), MP))
    net = copenet_model.getcopenet(MP, precision="fp32").eval()
    net.load_state_dict(sd)
    inp = W.synthetic_inputs(int(g["inputs_seed"]), int(g["batch"]))
    im = torch.from_numpy(inp["im%d" % rank]).to(d)
    bb = torch.from_numpy(inp["bb%d" % rank]).to(d)
    pos = torch.from_numpy(g["init_position"]).to(d)
    xf = net.forward_feat_ext(im)                               # this rank's view only
    groups = D.make_pair_groups(world)
    ief = D.ViewSplitIEF(net.regressor_step, groups[0], (0, 1))
    pose, betas = ief.run(xf, bb, pos, sd["init_pose"].to(d), sd["init_shape"].to(d), iters=3, shared_init=True)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "vs%d.npz" % rank), pose=pose.cpu().numpy(), betas=betas.cpu().numpy(),
             xf=xf.cpu().numpy(), n_exchanges=ief.n_exchanges)
    dist.barrier()
    dist.destroy_process_group()


def test_view_split_two_processes_on_one_gpu_match_golden(golden, net32, copenet_inputs, dev, tmp_path):
    """BASELINE config 4 / SURVEY 8e at what a 1-GPU lease can reach: the two views of every pair live in two
    PROCESSES (ranks 0, 1; both on cuda:0), each runs the trunk on its own view and the IEF loop through
    dist.ViewSplitIEF with the real ap_regressor_step, exchanging [art_pose | shape] before iterations 2 and 3.
    Result = the single-process forward (golden `copenet_b2`, made by the imported reference)."""
    import torch.multiprocessing as mp
    from test_dist import _free_port
    world, port = 2, _free_port()
    mp.spawn(_view_split_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    g = golden["copenet_b2"]
    gin = {k: v.to(dev) for k, v in copenet_inputs.items()}
    pos = torch.from_numpy(g["init_position"]).to(dev)
    xf = [net32.forward_feat_ext(gin["im0"]), net32.forward_feat_ext(gin["im1"])]
    one = net32.forward_ief(xf[0], xf[1], gin["bb0"], gin["bb1"], pos, pos, iters=3)
    for r in range(world):
        d = np.load(str(tmp_path / ("vs%d.npz" % r)))
        assert int(d["n_exchanges"]) == 2
        assert np.array_equal(d["xf"], xf[r].cpu().numpy())                      # same trunk kernels, same bits
        ep = pose_err(d["pose"], g["pose%d_it3" % r])
        eb = rel_err(d["betas"], g["betas%d_it3" % r])
        print("view-split rank %d vs golden: pose %.3e betas %.3e" % (r, ep, eb))
        assert ep < TOL32 and eb < TOL32
        # and against the fused single-process IEF on the same GPU (different kernels: step chain vs fused loop)
        assert pose_err(d["pose"], one[2 * r]) < 1e-5 and rel_err(d["betas"], one[2 * r + 1].cpu().numpy()) < 1e-5


# ------------------------------------------------------------------------------------------------ forward_reg of the baseline heads
def test_baseline_heads_expose_forward_reg(golden, dev):
    """model_hmr.forward_reg (:160-172), model_copenet_singleview.forward_reg (:159-170) and model_muhmr.forward_reg
    (:177-203): ONE regressor evaluation from trunk features, as the reference modules expose it, against the oracle's
    linear layers on the same weights; and consistency with forward(): iterating forward_reg reproduces it."""
    from airpose_amd import copenet_singleview_model, hmr_model, muhmr_model, weights as W
    from oracle import copenet_ref
    gen = torch.Generator().manual_seed(77)
    B = 3
    xf0, xf1 = torch.randn(B, 2048, generator=gen), torch.randn(B, 2048, generator=gen)
    pose = torch.randn(B, 132, generator=gen) * 0.5
    pose1 = torch.randn(B, 132, generator=gen) * 0.5
    shape, shape1 = torch.randn(B, 10, generator=gen) * 0.5, torch.randn(B, 10, generator=gen) * 0.5
    cam, cam1 = torch.randn(B, 3, generator=gen) * 0.3, torch.randn(B, 3, generator=gen) * 0.3
    bb, pos = torch.rand(B, 3, generator=gen), torch.randn(B, 3, generator=gen) * 0.3
    d = lambda t: t.to(dev)
    # ---- hmr
    sd = W.to_torch(W.copenet_state_dict(int(golden["hmr_b1"]["weights_seed"]), MEAN_PARAMS, variant="hmr"))
    net = hmr_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(sd)
    with torch.no_grad():
        want = copenet_ref.hmr_forward_reg(sd, xf0, pose, shape, cam)
    got = net.forward_reg(d(xf0), d(pose), d(shape), d(cam))
    for g_, w_, nm in zip(got, want, ("pose", "shape", "cam")):
        assert rel_err(g_.cpu().numpy(), w_.numpy()) < TOL32, "hmr " + nm
    # ---- copenet_singleview
    sd = W.to_torch(W.copenet_state_dict(int(golden["singleview_b1"]["weights_seed"]), MEAN_PARAMS, variant="singleview"))
    net = copenet_singleview_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(sd)
    p135 = torch.cat([pos, pose], 1)
    with torch.no_grad():
        xc = copenet_ref._lin(copenet_ref._lin(torch.cat([xf0, bb, p135, shape], 1), sd, "fc1"), sd, "fc2")
        want = (copenet_ref._lin(xc, sd, "decpose") + p135, copenet_ref._lin(xc, sd, "decshape") + shape)
    got = net.forward_reg(d(xf0), d(bb), d(p135), d(shape))
    assert pose_err(got[0], want[0]) < TOL32 and rel_err(got[1].cpu().numpy(), want[1].numpy()) < TOL32
    # ---- muhmr
    sd = W.to_torch(W.copenet_state_dict(int(golden["muhmr_b1"]["weights_seed"]), MEAN_PARAMS, variant="muhmr"))
    net = muhmr_model.getcopenet(MEAN_PARAMS, precision="fp32").eval()
    net.load_state_dict(sd)
    with torch.no_grad():
        xc0 = copenet_ref._lin(copenet_ref._lin(torch.cat([xf0, cam, pose, shape, pose1[:, 6:], shape1], 1), sd, "fc1"), sd, "fc2")
        xc1 = copenet_ref._lin(copenet_ref._lin(torch.cat([xf1, cam1, pose1, shape1, pose[:, 6:], shape], 1), sd, "fc1"), sd, "fc2")
        want = (pose + copenet_ref._lin(xc0, sd, "decpose"), shape + copenet_ref._lin(xc0, sd, "decshape"),
                cam + copenet_ref._lin(xc0, sd, "deccam"), pose1 + copenet_ref._lin(xc1, sd, "decpose"),
                shape1 + copenet_ref._lin(xc1, sd, "decshape"), cam1 + copenet_ref._lin(xc1, sd, "deccam"))
    got = net.forward_reg(d(xf0), d(xf1), d(pose[:, :6]), d(pose1[:, :6]), d(pose[:, 6:]), d(pose1[:, 6:]), d(shape), d(shape1),
                          d(cam), d(cam1))
    for g_, w_, nm in zip(got, want, ("pose0", "shape0", "cam0", "pose1", "shape1", "cam1")):
        assert rel_err(g_.cpu().numpy(), w_.numpy()) < TOL32, "muhmr " + nm


# ------------------------------------------------------------------------------------------------ round 6: probe, auto, range slots, split step
def test_regressor_split_step_equals_step_and_oracle(net32, copenet_sd, dev):
    """ap_regressor_feat_part + _step_local + _step_finish (the view-split step in its partner-independent and partner-dependent
    halves, model_copenet.py:185-199) against ap_regressor_step and against the oracle's forward_reg."""
    from oracle import copenet_ref
    torch.manual_seed(8)
    B = 5
    xf0, xf1 = torch.randn(B, 2048).abs(), torch.randn(B, 2048).abs()
    bb0, bb1 = torch.rand(B, 3), torch.rand(B, 3)
    pose0, pose1 = torch.randn(B, 135) * 0.5, torch.randn(B, 135) * 0.5
    s0, s1 = torch.randn(B, 10) * 0.5, torch.randn(B, 10) * 0.5
    with torch.no_grad():
        want = copenet_ref.forward_reg(copenet_sd, xf0, xf1, bb0, bb1, pose0[:, :3], pose1[:, :3], pose0[:, 3:9],
                                       pose1[:, 3:9], pose0[:, 9:], pose1[:, 9:], s0, s1)
    d = lambda t: t.to(dev)
    assert net32.fold_status()[0] == 1
    for v, (xf, bb, pose, s, po, so) in enumerate(((xf0, bb0, pose0, s0, pose1, s1), (xf1, bb1, pose1, s1, pose0, s0))):
        partner = torch.cat([po[:, 9:], so], 1)
        hfeat = net32.regressor_feat_part(d(xf))
        partial = net32.regressor_step_local(hfeat, d(bb), d(pose), d(s))
        p, b = net32.regressor_step_finish(partial, d(pose), d(s), d(partner))
        p1, b1 = net32.regressor_step(d(xf), d(bb), d(pose), d(s), d(partner))
        assert pose_err(p, p1) < 2e-6 and rel_err(b.cpu().numpy(), b1.cpu().numpy()) < 2e-6
        assert pose_err(p, want[2 * v]) < TOL32 and rel_err(b.cpu().numpy(), want[2 * v + 1].numpy()) < TOL32
    # the halves need the folded map: a handle on the literal chain refuses (and steps through ap_regressor_step instead)
    net32.set_fold(0)
    try:
        with pytest.raises(RuntimeError, match="folded"):
            net32.regressor_feat_part(d(xf0))
    finally:
        net32.set_fold(1)


def test_parity_probe_measures_the_checkpoint(copenet_sd, dev):
    """ap_net_parity_probe: the handle's trunk against the exact-fp32 trunk of the same weights on a seeded probe batch, on the GPU.
    On the benchmark checkpoint fp16 storage holds 1e-4, bf16 storage does not, the parity-grade modes sit far below; repeated
    probes reuse the packed reference and cost milliseconds."""
    from airpose_amd import copenet_model
    got = {}
    for prec in ("f16", "bf16", "bf16x2", "fp32"):
        net = copenet_model.getcopenet(MEAN_PARAMS, precision=prec).eval()
        net.load_state_dict(copenet_sd)
        first = net.parity_probe(8)
        again = net.parity_probe(8)
        assert again["rel_err_by_slice"] == first["rel_err_by_slice"]          # seeded: the same batch, the same kernels
        got[prec] = (first, again)
        print("probe %s: %s first %.0f ms, again %.1f ms" % (prec, {k: "%.2e" % v for k, v in first["rel_err_by_slice"].items()},
                                                             first["ms"], again["ms"]))
        if prec in ("f16", "bf16"):
            assert net.parity_probe(4, seed=5)["max_rel_err"] > 0.0
        del net
    assert got["f16"][0]["max_rel_err"] < 1e-4
    assert got["bf16"][0]["max_rel_err"] > 1e-4
    assert got["bf16x2"][0]["max_rel_err"] < 1e-5
    assert got["fp32"][0]["max_rel_err"] == 0.0
    assert got["f16"][1]["ms"] < 50.0                        # with the reference trunk packed: 2 x 16 images + two IEF loops


@pytest.mark.parametrize("ckpt,want", [("default", "f16"), ("wide", "bf16x2"), ("survey", None)])
def test_precision_auto_picks_by_probe(body, smplx_model, dev, ckpt, want):
    """getcopenet(precision="auto"): the fastest mode whose probe holds 1e-4 on the LOADED checkpoint -- fp16 storage on the
    benchmark checkpoint, split-bf16 on the wide-BatchNorm one (where fp16 storage is 20x over the bar: VERDICT r5 'what is
    missing is the per-checkpoint guard'), and whatever holds on SURVEY 8(d)'s exact recipe (gamma ~ U(.5, 1.5) on every
    BatchNorm).  The chosen mode then meets the bar against the fp32 CPU oracle through the whole pipeline."""
    from airpose_amd import copenet_model, pipeline
    from airpose_amd import weights as W
    from oracle import pipeline_ref
    sd = W.to_torch(W.copenet_state_dict(20240901, MEAN_PARAMS, bn=ckpt))
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="auto").eval()
    net.load_state_dict(sd)
    inp = {k: torch.from_numpy(v) for k, v in W.synthetic_inputs(91, 8).items()}
    got = pipeline.TwoViewInference(net, body)({k: v.to(dev) for k, v in inp.items()})
    rep = net.auto_report
    print("auto on %s: chose %s; tried %s" % (ckpt, rep["chosen"], {k: ("%.2e" % v["max_rel_err"]) if "max_rel_err" in v else v["error"][:60]
                                                                    for k, v in rep["tried"].items()}))
    assert net.precision == rep["chosen"] and rep["tried"][rep["chosen"]]["holds"]
    if want is not None:
        assert rep["chosen"] == want
    else:
        assert rep["chosen"] in ("f16", "bf16x2", "fp32")
    for p, r in rep["tried"].items():                        # everything faster than the chosen mode was measured and rejected
        if p != rep["chosen"]:
            assert not r["holds"]
    with torch.no_grad():
        ref = pipeline_ref.infer(sd, smplx_model, inp["im0"], inp["im1"], inp["bb0"], inp["bb1"], inp["intr0"], inp["intr1"])
    for k in sorted(ref):
        if k in got:
            for nm, e in key_errs(k, got[k].float().cpu().numpy(), ref[k].numpy()).items():
                assert e < TOL32, (ckpt, rep["chosen"], nm, e)
    # a re-load re-runs the choice
    net.load_state_dict(W.to_torch(W.copenet_state_dict(20240901, MEAN_PARAMS)))
    net.forward_feat_ext(torch.zeros(1, 3, 224, 224, device=dev))
    assert net.precision == "f16" and net.auto_report["chosen"] == "f16"


def test_call_reports_the_overflow_of_its_own_pass(copenet_sd, body, dev):
    """TwoViewInference.__call__ with fp16 storage raises RangeError for ITS OWN forward (a one-shot
    stream-ordered forward that overflowed used to return AP_OK with garbage); check_range=False keeps the deferred behaviour."""
    from airpose_amd import _native as Nn
    from airpose_amd import copenet_model, pipeline
    from airpose_amd import weights as W
    sd = {k: v.clone() for k, v in copenet_sd.items()}
    sd["bn1.weight"] *= 1.0e6
    sd["bn1.bias"] *= 1.0e6
    bad = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    bad.load_state_dict(sd)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(3, 2).items()}
    pipe = pipeline.TwoViewInference(bad, body)
    out = pipe(batch)                                        # stream-ordered: returns at once ...
    with pytest.raises(Nn.RangeError, match="fp16 range"):   # ... and the first read of a result checks the forward's own snapshot
        out["pred_pose0"]
    with pytest.raises(Nn.RangeError):
        bad.range_status(reset=True)
    with pytest.raises(Nn.RangeError, match="fp16 range"):
        pipe(batch, check_range="sync")
    with pytest.raises(Nn.RangeError):
        bad.range_status(reset=True)
    pipe(batch)                                              # never read ...
    torch.cuda.synchronize()
    with pytest.raises(Nn.RangeError):                       # ... the next call tells
        pipe(batch)
    with pytest.raises(Nn.RangeError):
        bad.range_status(reset=True)
    pipe._unread.clear()
    pipe(batch, check_range=False)                           # deferred: returns ...
    torch.cuda.synchronize()
    with pytest.raises(Nn.RangeError):                       # ... and the next forward refuses
        pipe(batch, check_range=False)
    ok = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    ok.load_state_dict(copenet_sd)
    out = pipeline.TwoViewInference(ok, body)(batch)
    assert torch.isfinite(out["pred_vertices_cam0"]).all()


@pytest.mark.parametrize("B", [4, 64])
def test_pending_synchronize_blames_the_right_batch(copenet_sd, body, dev, B):
    """Pending.synchronize() reads the batch's own range snapshot (ap_net_range_mark_next: every pass stream snapshots its range
    word behind the batch's last kernel): a clean batch followed by an overflowing one (crops scaled by 1e7: the stem's output
    leaves the fp16 range) does not raise, the overflowing one does, and no stream is synchronised to find out (advisor r5).
    B = 64 takes the two concurrent pass streams."""
    from airpose_amd import _native as Nn
    from airpose_amd import copenet_model, pipeline
    from airpose_amd import weights as W
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()
    net.load_state_dict(copenet_sd)
    pipe = pipeline.TwoViewInference(net, body)
    good = {k: torch.from_numpy(v).to(dev) for k, v in W.synthetic_inputs(5, B).items()}
    hot = dict(good, im0=good["im0"] * 1.0e7, im1=good["im1"] * 1.0e7)   # (beyond fp16 at the stem's input conversion already)
    pipe.submit(good).synchronize()                          # warm-up (packs)
    for _ in range(3):
        p_good = pipe.submit(good)
        p_hot = pipe.submit(hot)
        p_good.synchronize()                                 # the batch BEHIND it overflows: not this one's business
        with pytest.raises(Nn.RangeError, match="fp16 range"):
            p_hot.synchronize()
        with pytest.raises(Nn.RangeError):                   # the handle's own flag is sticky until reset
            net.range_status(reset=True)
    assert torch.isfinite(pipe.submit(good).synchronize()["pred_j3d_cam0"]).all()


# ------------------------------------------------------------------------------------------------ round 6: half-image-resident 3x3 of layer2
def _img3_case(dev, N, seed, prec):
    bf = {"bf16": torch.bfloat16, "f16": torch.float16}[prec]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 28, 28, 128, generator=g).to(bf).to(dev)
    w = (torch.randn(128, 3, 3, 128, generator=g) * (2.0 / 1152) ** 0.5).to(bf).to(dev)     # [Cout][kh][kw][Cin]: K-contiguous rows
    sc = (torch.rand(128, generator=g) + 0.5).to(dev)
    sh = (torch.randn(128, generator=g) * 0.1).to(dev)
    return x, w, sc, sh


@pytest.mark.parametrize("N", [1, 3, 8, 21, 300])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_img3_equals_slab_kernel(dev, prec, N):
    """conv_img3.hip (layer2's 3x3 with half an image resident in LDS) against the stand-alone convolution of the same operands
    (ap_conv2d_nhwc: the slab kernel, whose K order it follows): the same bits, in NHWC and in the fragment-tiled output layout;
    N = 1 / 3 / 21: groups of 16 half images only partly filled; 300: the persistent loop (600 half images on 256 workgroups)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    B = Nn.PRECISIONS[prec]
    x, w, sc, sh = _img3_case(dev, N, 60 + N, prec)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    want = torch.empty_like(x)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w), p(sc), p(sh), None, p(want), N, 28, 28, 128, 128, 3, 1, 1, 1, st), "conv2d")
    ws = torch.empty(L.ap_conv_img3_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_img3_pack(B, p(w), p(ws), st), "pack")
    got = torch.full_like(x, 7.0)
    Nn.check(L.ap_conv_img3_nhwc(B, p(x), p(ws), p(sc), p(sh), p(got), N, 0, st), "img3")
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    bad = (got.view(torch.int16) != want.view(torch.int16))
    assert not bad.any(), "%d of %d values differ; first at %s" % (int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    tiled = torch.full_like(x, 7.0)
    Nn.check(L.ap_conv_img3_nhwc(B, p(x), p(ws), p(sc), p(sh), p(tiled), N, 1, st), "img3 tiled")
    torch.cuda.synchronize()
    M = N * 784
    back = tiled.view(M // 16, 16, 16, 8).permute(0, 2, 1, 3).reshape(N, 28, 28, 128)
    assert torch.equal(back.view(torch.int16), want.view(torch.int16))
    # against fp64 on the same operands
    ref = F.conv2d(x.double().permute(0, 3, 1, 2).cpu(), w.double().permute(0, 3, 1, 2).cpu(), padding=1)
    ref = torch.relu(ref * sc.double().cpu().view(1, -1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    assert rel_err(got.float().cpu().numpy(), ref.numpy()) < (2e-2 if prec == "bf16" else 3e-3)


def test_conv_img3_soak(dev):
    """The hand-counted waits of conv_img3.hip under a second stream that keeps the memory system busy: 40 launches of 512 images,
    each compared bit for bit with the first result."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    B = Nn.PRECISIONS["f16"]
    N = 512
    x, w, sc, sh = _img3_case(dev, N, 5, "f16")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    ws = torch.empty(L.ap_conv_img3_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_img3_pack(B, p(w), p(ws), st), "pack")
    want = torch.empty_like(x)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w), p(sc), p(sh), None, p(want), N, 28, 28, 128, 128, 3, 1, 1, 1, st), "conv2d")
    noise = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream()
    got = torch.empty_like(x)
    for rep in range(40):
        if rep & 1:
            with torch.cuda.stream(side):
                noise.add_(1.0)
        got.fill_(3.0)
        Nn.check(L.ap_conv_img3_nhwc(B, p(x), p(ws), p(sc), p(sh), p(got), N, 0, st), "img3")
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), rep


@pytest.mark.parametrize("n", [1, 3, 64, 130])
def test_half_image_resident_layer2_conv2_in_the_trunk_is_bit_identical(net16, dev, n):
    """layer2.1 .. 2.3 conv2 on conv_img3.hip (forced on: the automatic rule takes it for passes that fill whole rounds of the chip
    with half images; n = 130 does by itself: 260 half images, tiled and untiled t2 both occur in the trunk) against the slab kernel:
    the same K order, so the trunk features carry the same bits; with the fused pairs off the untiled-output form is exercised."""
    gen = torch.Generator(device="cpu").manual_seed(900 + n)
    x = torch.randn(n, 3, 224, 224, generator=gen).to(dev)
    try:
        net16.set_img3(0)
        ref = net16.forward_feat_ext(x).clone()
        net16.set_img3(2)
        got = net16.forward_feat_ext(x).clone()
        net16.set_fuse_pair(0)
        got_nopair = net16.forward_feat_ext(x).clone()
        net16.set_fuse_pair(1)
        net16.set_img3(1)
        auto = net16.forward_feat_ext(x).clone()
    finally:
        net16.set_img3(1)
        net16.set_fuse_pair(1)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref) and torch.equal(got_nopair, ref) and torch.equal(auto, ref)


def _s2p_case(dev, N, seed, prec):
    bf = {"bf16": torch.bfloat16, "f16": torch.float16}[prec]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 56, 56, 128, generator=g).to(bf).to(dev)
    w = (torch.randn(128, 3, 3, 128, generator=g) * (2.0 / 1152) ** 0.5).to(bf).to(dev)     # [Cout][kh][kw][Cin]: K-contiguous rows
    sc = (torch.rand(128, generator=g) + 0.5).to(dev)
    sh = (torch.randn(128, generator=g) * 0.1).to(dev)
    return x, w, sc, sh


@pytest.mark.parametrize("N", [1, 3, 8, 21, 150])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_s2p_equals_generic_stride2(dev, prec, N):
    """conv_s2p.hip (layer2.0's 3x3 / stride 2 in polyphase form, a quarter of an output image per workgroup, waves split into
    compute and DMA roles) against fp64 on the same operands and against the stand-alone convolution (ap_conv2d_nhwc: the ring
    kernel).  Its K order is its own (the taps phase by phase), so the comparison with the ring kernel is to fp32 summation order:
    every output within 2 ulp of the storage type, most of them equal; NHWC and fragment-tiled output; N = 1 / 3 / 21: groups of 32
    quarter images only partly filled, 150: the persistent loop (600 quarters on 256 workgroups)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    B = Nn.PRECISIONS[prec]
    x, w, sc, sh = _s2p_case(dev, N, 90 + N, prec)
    x[0, :3, :, :] = 2.0                                      # flat borders: the zero padding above / left of the first quarters
    x[0, :, :3, :] = -2.0
    x[N - 1, -3:, :, :] = 1.5
    x[N - 1, :, -3:, :] = -1.5
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    want = torch.empty(N, 28, 28, 128, dtype=x.dtype, device=dev)
    Nn.check(L.ap_conv2d_nhwc(B, p(x), p(w), p(sc), p(sh), None, p(want), N, 56, 56, 128, 128, 3, 2, 1, 1, st), "conv2d")
    ws = torch.empty(L.ap_conv_s2p_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_s2p_pack(B, p(w), p(ws), st), "pack")
    got = torch.full_like(want, 7.0)
    Nn.check(L.ap_conv_s2p_nhwc(B, p(x), p(ws), p(sc), p(sh), p(got), N, 0, st), "s2p")
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    ref = F.conv2d(x.double().permute(0, 3, 1, 2).cpu(), w.double().permute(0, 3, 1, 2).cpu(), stride=2, padding=1)
    ref = torch.relu(ref * sc.double().cpu().view(1, -1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    e_got, e_ring = rel_err(got.float().cpu().numpy(), ref.numpy()), rel_err(want.float().cpu().numpy(), ref.numpy())
    print("conv_s2p %s N=%d: rel err vs fp64 %.3e (ring kernel %.3e)" % (prec, N, e_got, e_ring))
    assert e_got < (2e-2 if prec == "bf16" else 3e-3) and e_got < 1.2 * e_ring + 1e-6
    d = (got.float() - want.float()).abs()
    ulp = (2.0 ** -7 if prec == "bf16" else 2.0 ** -10) * torch.clamp(want.float().abs(), min=2.0 ** -6)
    assert bool((d <= 2.0 * ulp).all()), "max %.3e at %s" % (float(d.max()), (d > 2.0 * ulp).nonzero()[0].tolist())
    tiled = torch.full_like(want, 7.0)
    Nn.check(L.ap_conv_s2p_nhwc(B, p(x), p(ws), p(sc), p(sh), p(tiled), N, 1, st), "s2p tiled")
    again = torch.full_like(want, 7.0)
    Nn.check(L.ap_conv_s2p_nhwc(B, p(x), p(ws), p(sc), p(sh), p(again), N, 0, st), "s2p again")
    torch.cuda.synchronize()
    if (N * 784) % 16 == 0:
        back = tiled.view(N * 784 // 16, 16, 16, 8).permute(0, 2, 1, 3).reshape(N, 28, 28, 128)
        assert torch.equal(back.view(torch.int16), got.view(torch.int16))
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))


def test_conv_s2p_soak(dev):
    """The hand-counted waits of conv_s2p.hip's compute waves and the role split under a second stream that keeps the memory system
    busy: 40 launches of 256 images, each compared bit for bit with the first result."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    B = Nn.PRECISIONS["f16"]
    N = 256
    x, w, sc, sh = _s2p_case(dev, N, 6, "f16")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = Nn.stream_ptr(dev)
    ws = torch.empty(L.ap_conv_s2p_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_s2p_pack(B, p(w), p(ws), st), "pack")
    first = torch.empty(N, 28, 28, 128, dtype=x.dtype, device=dev)
    Nn.check(L.ap_conv_s2p_nhwc(B, p(x), p(ws), p(sc), p(sh), p(first), N, 0, st), "s2p")
    torch.cuda.synchronize()
    noise = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream()
    got = torch.empty_like(first)
    for rep in range(40):
        if rep & 1:
            with torch.cuda.stream(side):
                noise.normal_()
        got.fill_(7.0)
        Nn.check(L.ap_conv_s2p_nhwc(B, p(x), p(ws), p(sc), p(sh), p(got), N, 0, st), "s2p")
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), first.view(torch.int16)), "launch %d differs" % rep


def test_trunk_with_polyphase_conv2_is_close_to_the_generic_path(netf16, dev):
    """layer2.0 conv2 on conv_s2p.hip (ap_net_set_s2p) against the generic stride-2 kernel through the whole trunk: the two K orders differ
    in fp32 summation order only -- pooled features agree to 1e-3 of the fp16 path's own distance from fp32 scale (2e-4 relative)."""
    gen = torch.Generator(device="cpu").manual_seed(77)
    x = torch.randn(5, 3, 224, 224, generator=gen).to(dev)
    ref = netf16.forward_feat_ext(x).clone()
    try:
        netf16.set_s2p(1)                                     # (off by default: faster alone, slower in the two-pass schedule)
        got = netf16.forward_feat_ext(x).clone()
        again = netf16.forward_feat_ext(x)
    finally:
        netf16.set_s2p(0)
    assert torch.isfinite(got).all()
    e = float((got - ref).abs().max() / ref.abs().max())
    print("trunk, polyphase conv2 vs generic: %.3e" % e)
    assert 0.0 < e < 2e-3                                     # (0: the knob did nothing)
    assert torch.equal(again, got)                            # and reproducible


# (knob, value, images) -> conv-stack launches of one 16-bit pass with every other knob at its default
LAUNCHES_16BIT = [
    (None, None, 2, 33),                  # 3 layer1 kernels + 4 x 2 (layer2) + 2 + 3 + 4 x 2 (layer3) + 3 x 3 (layer4)
    ("set_img_block", 2, 2, 27),          # layer3.1 .. 3.5 as one kernel each
    ("set_img_block", 0, 2, 33),
    ("set_fuse_pair", 0, 2, 41),
    ("set_fuse_block", 0, 2, 40),
    ("set_fuse_tail", 0, 2, 34),
    ("set_pw_conv", 0, 4, 33),            # 4 images: one 196-pixel tile at 7 x 7
    ("set_pw_conv", 2, 4, 33),
    ("set_img3", 0, 2, 33),
    ("set_img3", 2, 2, 33),
    ("set_s2p", 1, 2, 33),
    ("set_fuse_pool", 1, 2, 33),
]
KNOB_DEFAULTS = {"set_img_block": 1, "set_fuse_pair": 1, "set_fuse_block": 1, "set_fuse_tail": 1, "set_pw_conv": 1, "set_img3": 1,
                 "set_s2p": 0, "set_fuse_pool": 0}


def test_conv_launch_counts_of_one_pass(net32, netbf, netf16, dev):
    """What ap_net_last_conv_launches reports after ONE trunk pass (set_dual_stream(0)) is pinned: it is the number bench.py prints
    and the only outside view of which kernels the schedule chose.  fp32: every block as three convolutions, 48, and 52 with the
    four downsample convolutions unfused.  16-bit: 27 when the pass fills whole rounds of the chip with the image-resident layer3
    blocks (n * 8 >= ceil(n / CUs) * CUs * 7: the two batch sizes on either side of the first threshold), 33 when it does not
    (54 / 66 for two passes).  The rows of LAUNCHES_16BIT that neither follows from are what the library returned through
    this call before the schedule was split into a plan and a launching loop -- equalities, no margin."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n_fill = (cus * 7 + 7) // 8                               # smallest n with n * 8 >= cus * 7 (224 on 256 CUs)
    x = torch.randn(n_fill, 3, 224, 224, generator=torch.Generator(device="cpu").manual_seed(2700)).to(dev)

    def count(net, n):
        net.forward_feat_ext(x[:n])
        return net.last_conv_launches()

    got, want = {}, {}
    try:
        for net in (net32, netbf, netf16):
            net.set_dual_stream(0)
        got["fp32"], want["fp32"] = count(net32, 2), 48
        net32.set_fuse_ds(0)
        got["fp32 fuse_ds 0"], want["fp32 fuse_ds 0"] = count(net32, 2), 52
        for name, net in (("bf16", netbf), ("f16", netf16)):
            got[name, "fills", n_fill], want[name, "fills", n_fill] = count(net, n_fill), 27
            got[name, "fills", n_fill - 1], want[name, "fills", n_fill - 1] = count(net, n_fill - 1), 33
            for knob, value, n, launches in LAUNCHES_16BIT:
                if knob:
                    getattr(net, knob)(value)
                got[name, knob, value, n], want[name, knob, value, n] = count(net, n), launches
                if knob:
                    getattr(net, knob)(KNOB_DEFAULTS[knob])
    finally:
        net32.set_fuse_ds(1)
        for net in (net32, netbf, netf16):
            net.set_dual_stream(1)
        for net in (netbf, netf16):
            for knob, value in KNOB_DEFAULTS.items():
                getattr(net, knob)(value)
    torch.cuda.synchronize()
    for k in got:
        print("conv launches", k, got[k], "want", want[k])
    assert got == want
