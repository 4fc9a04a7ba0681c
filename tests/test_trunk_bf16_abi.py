"""CPU checks of the bf16 training mode's entry points in libairpose_grad.so (trunk_grad_bf16.hip) and of its Python switch: the
capability query, host-side refusal of bad arguments (null pointers, bad geometry, misaligned pointers, channel counts that are not
a multiple of 8, a too-small workspace) before any launch, the workspace size against a restatement of the buffer list, and
copenet.set_trunk_trainable(precision=...).  No compute calls: there is no GPU here."""
import ctypes
import os

import pytest

from conftest import MEAN_PARAMS

EINVAL, ENOMEM = -1, -4
FP32, BF16 = 0, 1


def _lib():
    from airpose_amd import _native_grad
    if not os.path.isfile(_native_grad.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native_grad.lib()


def _err(L):
    return L.apg_last_error().decode()


def test_capability_query_reports_bf16():
    from airpose_amd import _native_grad
    L = _lib()
    assert L.apg_trunk_precisions() == (1 << FP32) | (1 << BF16)
    assert _native_grad.PRECISIONS == {"fp32": FP32, "bf16": BF16}
    assert L.apg_abi_version() == 2                                  # additive: the ABI number stays


def test_bf16_primitives_refuse_bad_arguments():
    L = _lib()
    ok = ctypes.c_void_p(4096)                   # never dereferenced: every call below fails its host-side checks
    odd = ctypes.c_void_p(4096 + 8)              # 8-byte aligned only
    # weight pack: null, Cp < C, Cp not a multiple of 8, C_out not a multiple of 8, misaligned output
    assert L.apg_pack_weights_bf16(None, 16, 16, 16, 3, 3, ok, ok, None) == EINVAL and "apg_pack_weights_bf16" in _err(L)
    assert L.apg_pack_weights_bf16(ok, 16, 16, 16, 3, 3, None, None, None) == EINVAL
    assert L.apg_pack_weights_bf16(ok, 16, 16, 8, 3, 3, ok, ok, None) == EINVAL
    assert L.apg_pack_weights_bf16(ok, 16, 3, 4, 3, 3, ok, ok, None) == EINVAL
    assert L.apg_pack_weights_bf16(ok, 12, 16, 16, 3, 3, ok, ok, None) == EINVAL
    assert L.apg_pack_weights_bf16(ok, 16, 16, 16, 3, 3, odd, ok, None) == EINVAL
    # conv forward: null, stride 0, empty output, kernel larger than the padded input, C not a multiple of 8, misaligned x / wf / y
    assert L.apg_conv_fwd_bf16(None, 1, 8, 8, 16, ok, 16, 3, 3, 1, 1, ok, None) == EINVAL and "apg_conv_fwd_bf16" in _err(L)
    assert L.apg_conv_fwd_bf16(ok, 1, 8, 8, 16, ok, 16, 3, 3, 0, 1, ok, None) == EINVAL
    assert L.apg_conv_fwd_bf16(ok, 1, 2, 2, 16, ok, 16, 7, 7, 1, 0, ok, None) == EINVAL
    assert L.apg_conv_fwd_bf16(ok, 1, 2, 2, 16, ok, 16, 3, 3, 2, 0, ok, None) == EINVAL
    assert L.apg_conv_fwd_bf16(ok, 1, 8, 8, 12, ok, 16, 3, 3, 1, 1, ok, None) == EINVAL
    assert L.apg_conv_fwd_bf16(ok, 1, 8, 8, 16, ok, 12, 3, 3, 1, 1, ok, None) == EINVAL
    for args in ((odd, ok, ok), (ok, odd, ok), (ok, ok, odd)):
        assert L.apg_conv_fwd_bf16(args[0], 1, 8, 8, 16, args[1], 16, 3, 3, 1, 1, args[2], None) == EINVAL
        assert "aligned" in _err(L)
    # conv backward
    geo = (1, 8, 8, 16, 16, 1, 1, 1, 0)
    n, H, W, C, K, R, S, st, pad = geo
    nb = L.apg_conv_bwd_bf16_workspace_bytes(*geo)
    assert nb > 0 and nb % (4 * K * C * R * S) == 0
    assert L.apg_conv_bwd_bf16_workspace_bytes(1, 8, 8, 12, 16, 1, 1, 1, 0) < 0
    assert L.apg_conv_bwd_bf16_workspace_bytes(1, 2, 2, 16, 16, 3, 3, 2, 0) < 0
    bwd = lambda x, wd, gy, add, gx, f32, gw, gwc, ws, wsb, g=geo: L.apg_conv_bwd_bf16(x, g[0], g[1], g[2], g[3], wd, g[4], g[5], g[6],
                                                                                    g[7], g[8], gy, add, 0, gx, f32, gw, gwc, ws, wsb, None)
    assert bwd(ok, ok, None, None, ok, 0, ok, C, ok, nb) == EINVAL and "apg_conv_bwd_bf16" in _err(L)     # no gy
    assert bwd(ok, ok, ok, None, None, 0, None, C, ok, nb) == EINVAL                                       # no output asked for
    assert bwd(ok, None, ok, None, ok, 0, None, C, ok, nb) == EINVAL                                       # gx without weights
    assert bwd(None, ok, ok, None, None, 0, ok, C, ok, nb) == EINVAL                                       # gw without x
    assert bwd(ok, ok, odd, None, ok, 0, ok, C, ok, nb) == EINVAL                                          # misaligned gy
    assert bwd(ok, ok, ok, odd, ok, 0, ok, C, ok, nb) == EINVAL                                            # misaligned add
    assert bwd(ok, ok, ok, ok, ok, 1, ok, C, ok, nb) == EINVAL                                             # add with an fp32 gx
    assert bwd(ok, ok, ok, None, ok, 0, ok, C + 1, ok, nb) == EINVAL                                       # gw_channels > C
    assert L.apg_conv_bwd_bf16(ok, n, H, W, C, ok, K, R, S, st, pad, ok, ok, 1, ok, 0, None, 0, None, 0, None) == EINVAL   # fp32 add over gx
    assert bwd(ok, ok, ok, None, ok, 0, ok, C, ok, nb, g=(1, 2, 2, 16, 16, 3, 3, 2, 0)) == EINVAL          # bad geometry
    assert bwd(ok, ok, ok, None, ok, 0, ok, C, None, 0) == ENOMEM and "needed" in _err(L)
    assert bwd(ok, ok, ok, None, ok, 0, ok, C, ok, nb - 4) == ENOMEM
    # BatchNorm
    wsb = L.apg_bn_bf16_workspace_bytes(64, 16)
    assert wsb > 0 and L.apg_bn_bf16_workspace_bytes(0, 16) < 0 and L.apg_bn_bf16_workspace_bytes(64, 12) < 0
    assert wsb == L.apg_bn_workspace_bytes(64, 16)                   # the fp32 partials of the fp32 path: same tiles
    bnf = lambda x, C_, rm, train, res, y, ws, b: L.apg_bn_fwd_bf16(x, 64, C_, ok, ok, rm, rm, train, 0.1, 1e-5, res, 1, y, ok, ok, ws, b,
                                                                   None)
    assert bnf(None, 16, None, 1, None, ok, ok, wsb) == EINVAL and "apg_bn_fwd_bf16" in _err(L)
    assert bnf(ok, 12, None, 1, None, ok, ok, wsb) == EINVAL
    assert bnf(ok, 16, None, 0, None, ok, ok, wsb) == EINVAL         # eval mode needs the running statistics
    assert bnf(odd, 16, None, 1, None, ok, ok, wsb) == EINVAL
    assert bnf(ok, 16, None, 1, odd, ok, ok, wsb) == EINVAL
    assert bnf(ok, 16, None, 1, None, odd, ok, wsb) == EINVAL
    assert bnf(ok, 16, ok, 1, None, ok, None, 0) == ENOMEM
    assert bnf(ok, 16, ok, 1, None, ok, ok, wsb - 4) == ENOMEM
    bnb = lambda gy, y, x, C_, gx, gres, ws, b: L.apg_bn_bwd_bf16(gy, y, x, 64, C_, ok, ok, ok, 1, gx, gres, None, None, ws, b, None)
    assert bnb(None, None, ok, 16, ok, None, ok, wsb) == EINVAL and "apg_bn_bwd_bf16" in _err(L)
    assert bnb(ok, None, ok, 12, ok, None, ok, wsb) == EINVAL
    assert bnb(ok, odd, ok, 16, ok, None, ok, wsb) == EINVAL
    assert bnb(ok, None, ok, 16, odd, None, ok, wsb) == EINVAL
    assert bnb(ok, None, ok, 16, ok, odd, ok, wsb) == EINVAL
    assert bnb(ok, None, ok, 16, ok, None, ok, 8) == ENOMEM
    # pools
    assert L.apg_maxpool_fwd_bf16(None, 1, 8, 8, 16, ok, None) == EINVAL and "apg_maxpool_fwd_bf16" in _err(L)
    assert L.apg_maxpool_fwd_bf16(ok, 1, 8, 8, 12, ok, None) == EINVAL
    assert L.apg_maxpool_fwd_bf16(ok, 1, 8, 8, 16, odd, None) == EINVAL
    assert L.apg_maxpool_bwd_bf16(ok, 1, 8, 8, 16, None, ok, None) == EINVAL and "apg_maxpool_bwd_bf16" in _err(L)
    assert L.apg_maxpool_bwd_bf16(ok, 1, 0, 8, 16, ok, ok, None) == EINVAL
    assert L.apg_maxpool_bwd_bf16(ok, 1, 8, 8, 16, odd, ok, None) == EINVAL
    assert L.apg_avgpool_fwd_bf16(ok, 0, 16, ok, None) == EINVAL and "apg_avgpool_fwd_bf16" in _err(L)
    assert L.apg_avgpool_fwd_bf16(None, 1, 16, ok, None) == EINVAL
    assert L.apg_avgpool_bwd_bf16(None, 1, 16, ok, None) == EINVAL and "apg_avgpool_bwd_bf16" in _err(L)
    assert L.apg_avgpool_bwd_bf16(ok, 1, 12, ok, None) == EINVAL
    assert L.apg_avgpool_bwd_bf16(ok, 1, 16, odd, None) == EINVAL


def test_bf16_walker_refuses_bad_arguments():
    L = _lib()
    ok = ctypes.c_void_p(4096)
    full = (ctypes.c_void_p * (53 * 5))(*([4096] * (53 * 5)))
    holey = (ctypes.c_void_p * (53 * 5))(*([4096] * (53 * 5)))
    holey[17] = None
    grads = (ctypes.c_void_p * (53 * 3))()
    big = L.apg_trunk_workspace_bytes_p(2, 1, BF16)
    assert big > 0
    assert L.apg_trunk_workspace_bytes_p(0, 1, BF16) < 0 and L.apg_trunk_workspace_bytes_p(2, 1, 7) < 0
    assert L.apg_trunk_fwd_p(7, 2, ok, full, 1, 0.1, 1e-5, ok, 1, ok, big, None) == EINVAL and "precision" in _err(L)
    assert L.apg_trunk_fwd_p(BF16, 0, ok, full, 1, 0.1, 1e-5, ok, 1, ok, big, None) == EINVAL and "apg_trunk_fwd_p" in _err(L)
    assert L.apg_trunk_fwd_p(BF16, 2, None, full, 1, 0.1, 1e-5, ok, 1, ok, big, None) == EINVAL
    assert L.apg_trunk_fwd_p(BF16, 2, ok, None, 1, 0.1, 1e-5, ok, 1, ok, big, None) == EINVAL
    assert L.apg_trunk_fwd_p(BF16, 2, ok, holey, 1, 0.1, 1e-5, ok, 1, ok, big, None) == EINVAL and "entry 17" in _err(L)
    assert L.apg_trunk_fwd_p(BF16, 2, ok, full, 1, 1.5, 1e-5, ok, 1, ok, big, None) == EINVAL
    assert L.apg_trunk_fwd_p(BF16, 2, ok, full, 1, 0.1, 1e-5, ok, 1, ctypes.c_void_p(4096 + 16), big, None) == EINVAL
    assert "aligned" in _err(L)
    assert L.apg_trunk_fwd_p(BF16, 2, ok, full, 1, 0.1, 1e-5, ok, 1, ok, big - 4, None) == ENOMEM and "needed" in _err(L)
    assert L.apg_trunk_bwd_p(7, 2, full, 1, ok, grads, None, ok, big, None) == EINVAL
    assert L.apg_trunk_bwd_p(BF16, 2, full, 1, None, grads, None, ok, big, None) == EINVAL and "apg_trunk_bwd_p" in _err(L)
    assert L.apg_trunk_bwd_p(BF16, 2, holey, 1, ok, grads, None, ok, big, None) == EINVAL
    assert L.apg_trunk_bwd_p(BF16, 2, full, 1, ok, grads, None, ctypes.c_void_p(4096 + 16), big, None) == EINVAL
    assert L.apg_trunk_bwd_p(BF16, 2, full, 1, ok, grads, None, ok, L.apg_trunk_workspace_bytes_p(2, 0, BF16), None) == ENOMEM
    # APG_PREC_FP32 is the fp32 walker: same sizes, same refusals
    for n in (1, 4):
        for save in (0, 1):
            assert L.apg_trunk_workspace_bytes_p(n, save, FP32) == L.apg_trunk_workspace_bytes(n, save)
    assert L.apg_trunk_fwd_p(FP32, 0, ok, full, 1, 0.1, 1e-5, ok, 1, ok, big, None) == EINVAL and "apg_trunk_fwd:" in _err(L)


def _trunk_layers():
    """(H, C, K, R, stride, pad) of the 53 conv + BN pairs in the walker's order"""
    out = [(224, 3, 64, 7, 2, 3)]
    H, C = 56, 64
    for li, (nb, p) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512))):
        for b in range(nb):
            st = 2 if (b == 0 and li > 0) else 1
            Ho = (H + 2 - 3) // st + 1
            out += [(H, C, p, 1, 1, 0), (H, p, p, 3, st, 1), (Ho, p, 4 * p, 1, 1, 0)]
            if b == 0:
                out.append((H, C, 4 * p, 1, st, 0))
            H, C = Ho, 4 * p
    assert len(out) == 53 and H == 7
    return out


def _expected_bytes(L, n, bf16, with_part=True):
    """save = 1 workspace from the buffer list: per layer z and a (n Ho Wo K elements each) and fp32 mean / invstd;
    the crops (fp32: 3 channels; bf16: 8 channels); the max-pool output; six gradient buffers of the largest activation
    (n 112 112 64 elements); the fp32 partials (the largest split-K / BatchNorm need of any layer); bf16 only: two packed copies of
    every conv weight.  Elements are 4 / 2 bytes, buffers are rounded up to 256 bytes (64 floats in the fp32 plan)."""
    el = 2 if bf16 else 4
    up = lambda b: (b + 255) // 256 * 256
    tot, part = up(n * 224 * 224 * (8 if bf16 else 3) * el) + up(n * 56 * 56 * 64 * el) + 6 * up(n * 112 * 112 * 64 * el), 0
    for H, C, K, R, st, pad in _trunk_layers():
        Ho = (H + 2 * pad - R) // st + 1
        Cp = (C + 7) // 8 * 8 if bf16 else C
        tot += 2 * up(n * Ho * Ho * K * el) + 2 * up(K * 4)
        if bf16:
            tot += 2 * up(K * R * R * Cp * 2)                        # wf and wd
            part = max(part, L.apg_conv_bwd_bf16_workspace_bytes(n, H, H, Cp, K, R, R, st, pad), L.apg_bn_bf16_workspace_bytes(n * Ho * Ho, K))
        else:
            part = max(part, L.apg_conv_bwd_workspace_bytes(n, H, H, C, K, R, R, st, pad), L.apg_bn_workspace_bytes(n * Ho * Ho, K))
    return tot + (up(part) if with_part else 0)


def test_bf16_workspace_matches_the_buffer_list_and_is_about_half():
    """Per crop the bf16 plan keeps the fp32 plan's activations at half the bytes, except the crops (8 bf16 channels = 16 bytes per
    pixel against 3 fp32 = 12); on top come 2 x 23.5 M packed bf16 weights (94 MB, independent of n) and the fp32 partials.  So the
    ratio to the fp32 workspace tends to 0.5 + (0.8 - 0.3) MB / 110 MB = 0.505 from above as n grows: 0.51 - 0.53 at n = 64,
    asserted below against the restated lists, not guessed."""
    L = _lib()
    weights = sum(2 * K * R * R * ((C + 7) // 8 * 8) * 2 for H, C, K, R, st, pad in _trunk_layers())
    for n in (1, 4, 64):
        b, f = L.apg_trunk_workspace_bytes_p(n, 1, BF16), L.apg_trunk_workspace_bytes(n, 1)
        eb, ef = _expected_bytes(L, n, True), _expected_bytes(L, n, False)
        assert f == ef, (n, f, ef)                                   # the restatement reproduces the fp32 plan exactly ...
        assert b == eb, (n, b, eb)                                   # ... and the bf16 one
        assert b < f or n == 1
        # save = 0: five rotating buffers, one packed copy (wf) of every weight, statistics, partials: no wd
        small = L.apg_trunk_workspace_bytes_p(n, 0, BF16)
        up = lambda v: (v + 255) // 256 * 256
        per_layer = sum(up(K * R * R * ((C + 7) // 8 * 8) * 2) + 2 * up(K * 4) for H, C, K, R, st, pad in _trunk_layers())
        part = eb - _expected_bytes(L, n, True, with_part=False)
        assert small == 5 * up(n * 112 * 112 * 64 * 2) + per_layer + part < b, (n, small)
    b, f = L.apg_trunk_workspace_bytes_p(64, 1, BF16), L.apg_trunk_workspace_bytes(64, 1)
    weights = sum(2 * K * R * R * ((C + 7) // 8 * 8) * 2 for H, C, K, R, st, pad in _trunk_layers())
    assert 93e6 < weights < 96e6
    assert 0.505 < b / f < 0.53, b / f
    assert b < 3.8e9                                                 # the header documents 3.7 GB at n = 64
    sizes = [L.apg_trunk_workspace_bytes_p(n, 1, BF16) for n in (1, 2, 4, 32, 64)]
    assert sizes == sorted(set(sizes))


def test_precision_keyword_and_property():
    from airpose_amd import copenet_model, hmr_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="fp32")
    keys = list(net.state_dict())
    assert net.trunk_precision == "fp32"
    assert net.set_trunk_trainable(True) is net and net.trunk_precision == "fp32"
    assert net.set_trunk_trainable(True, precision="bf16").trunk_precision == "bf16"
    assert net.set_trunk_trainable(True).trunk_precision == "fp32"   # the default is fp32 on every call
    for bad in ("fp16", "bf16x2", None, 16):
        with pytest.raises(RuntimeError, match="precision"):
            net.set_trunk_trainable(True, precision=bad)
    assert net.trunk_precision == "fp32"
    with pytest.raises(AttributeError):
        net.trunk_precision = "bf16"                                 # read-only
    net.set_trunk_trainable(True, "bf16")
    assert list(net.state_dict()) == keys                            # a runtime switch, not a parameter or buffer
    with pytest.raises(RuntimeError, match="two-view"):
        hmr_model.getcopenet(MEAN_PARAMS).set_trunk_trainable(True, precision="bf16")
