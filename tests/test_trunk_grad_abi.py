"""CPU checks of the trunk entry points of libairpose_grad.so (ABI 2): every one refuses bad arguments on the host, before any
launch, with a message in apg_last_error(); the workspace queries are positive and grow with the batch (no compute calls: there
is no GPU here)."""
import ctypes
import os
import re

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL, ENOMEM = -1, -4


def _lib():
    from airpose_amd import _native_grad
    if not os.path.isfile(_native_grad.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native_grad.lib()


def _err(L):
    return L.apg_last_error().decode()


def test_abi_version_is_2():
    from airpose_amd import _native_grad
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert _native_grad.ABI_VERSION == 2 and _lib().apg_abi_version() == 2


def test_primitives_refuse_bad_arguments():
    L = _lib()
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every call below fails its host-side checks
    assert L.apg_conv_fwd(None, 1, 8, 8, 16, fake, 16, 3, 3, 1, 1, fake, None) == EINVAL
    assert "apg_conv_fwd" in _err(L)
    assert L.apg_conv_fwd(fake, 1, 8, 8, 16, fake, 16, 3, 3, 0, 1, fake, None) == EINVAL          # stride 0
    assert L.apg_conv_fwd(fake, 1, 2, 2, 16, fake, 16, 7, 7, 1, 0, fake, None) == EINVAL          # empty output
    # C_out not a multiple of 16; no output asked for; weight gradient without workspace
    assert L.apg_conv_bwd(fake, 1, 8, 8, 16, fake, 12, 1, 1, 1, 0, fake, fake, None, None, 0, None) == EINVAL
    assert "apg_conv_bwd" in _err(L)
    assert L.apg_conv_bwd(fake, 1, 8, 8, 16, fake, 16, 1, 1, 1, 0, fake, None, None, None, 0, None) == EINVAL
    assert L.apg_conv_bwd(fake, 1, 8, 8, 16, fake, 16, 1, 1, 1, 0, fake, None, fake, None, 0, None) == ENOMEM
    assert "needed" in _err(L)
    assert L.apg_bn_fwd(None, 64, 16, fake, fake, None, None, 1, 0.1, 1e-5, None, 1, fake, fake, fake, fake, 1 << 20, None) == EINVAL
    assert "apg_bn_fwd" in _err(L)
    # eval mode needs the running statistics; train mode needs the workspace
    assert L.apg_bn_fwd(fake, 64, 16, fake, fake, None, None, 0, 0.1, 1e-5, None, 1, fake, fake, fake, None, 0, None) == EINVAL
    assert L.apg_bn_fwd(fake, 64, 16, fake, fake, fake, fake, 1, 0.1, 1e-5, None, 1, fake, fake, fake, None, 0, None) == ENOMEM
    assert L.apg_bn_bwd(fake, None, fake, 0, 16, fake, fake, fake, 1, fake, None, None, None, fake, 1 << 20, None) == EINVAL
    assert "apg_bn_bwd" in _err(L)
    assert L.apg_bn_bwd(fake, None, fake, 64, 16, fake, fake, fake, 1, fake, None, None, None, fake, 8, None) == ENOMEM
    assert L.apg_maxpool_fwd(None, 1, 8, 8, 16, fake, None) == EINVAL and "apg_maxpool_fwd" in _err(L)
    assert L.apg_maxpool_bwd(fake, 1, 8, 8, 16, None, fake, None) == EINVAL and "apg_maxpool_bwd" in _err(L)
    assert L.apg_avgpool_fwd(fake, 0, 16, fake, None) == EINVAL and "apg_avgpool_fwd" in _err(L)
    assert L.apg_avgpool_bwd(None, 1, 16, fake, None) == EINVAL and "apg_avgpool_bwd" in _err(L)


def test_trunk_walker_refuses_bad_arguments():
    L = _lib()
    fake = ctypes.c_void_p(4096)
    full = (ctypes.c_void_p * (53 * 5))(*([4096] * (53 * 5)))
    holey = (ctypes.c_void_p * (53 * 5))(*([4096] * (53 * 5)))
    holey[17] = None
    grads = (ctypes.c_void_p * (53 * 3))()
    big = L.apg_trunk_workspace_bytes(2, 1)
    assert L.apg_trunk_fwd(0, fake, full, 1, 0.1, 1e-5, fake, 1, fake, big, None) == EINVAL
    assert "apg_trunk_fwd" in _err(L)
    assert L.apg_trunk_fwd(2, fake, None, 1, 0.1, 1e-5, fake, 1, fake, big, None) == EINVAL
    assert L.apg_trunk_fwd(2, fake, holey, 1, 0.1, 1e-5, fake, 1, fake, big, None) == EINVAL
    assert "entry 17" in _err(L)
    assert L.apg_trunk_fwd(2, fake, full, 1, 1.5, 1e-5, fake, 1, fake, big, None) == EINVAL             # momentum outside [0, 1]
    assert L.apg_trunk_fwd(2, fake, full, 1, 0.1, 1e-5, fake, 1, fake, big - 4, None) == ENOMEM
    assert "needed" in _err(L)
    assert L.apg_trunk_bwd(2, full, 1, None, grads, None, fake, big, None) == EINVAL
    assert "apg_trunk_bwd" in _err(L)
    assert L.apg_trunk_bwd(2, holey, 1, fake, grads, None, fake, big, None) == EINVAL
    assert L.apg_trunk_bwd(2, full, 1, fake, grads, None, fake, L.apg_trunk_workspace_bytes(2, 0), None) == ENOMEM


def test_workspace_queries_are_positive_and_grow_with_n():
    L = _lib()
    for save in (0, 1):
        sizes = [L.apg_trunk_workspace_bytes(n, save) for n in (1, 2, 4, 32, 64)]
        assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)), sizes
        assert L.apg_trunk_workspace_bytes(0, save) < 0
    assert L.apg_trunk_workspace_bytes(64, 1) > L.apg_trunk_workspace_bytes(64, 0)
    assert L.apg_trunk_workspace_bytes(64, 1) < 8 * 1024 ** 3            # the header documents 7.0 GB at n = 64
    c = [L.apg_conv_bwd_workspace_bytes(n, 56, 56, 64, 64, 3, 3, 1, 1) for n in (1, 4, 64)]
    assert c[0] > 0 and c == sorted(c)
    assert L.apg_conv_bwd_workspace_bytes(1, 8, 8, 16, 16, 3, 3, 0, 1) < 0
    b = [L.apg_bn_workspace_bytes(m, 64) for m in (49, 3136, 802816)]
    assert b[0] > 0 and b == sorted(b) and L.apg_bn_workspace_bytes(0, 64) < 0


def test_conv_refuses_a_kernel_larger_than_the_padded_input():
    """(H + 2 pad - R) / stride truncates toward zero, so a kernel wider than the padded input would pass as a 1 x 1 output at
    stride >= 2 (F.conv2d refuses it).  Every conv entry point must refuse it at every stride; H + 2 pad == R stays valid."""
    L = _lib()
    fake = ctypes.c_void_p(4096)
    bad = [  # (n, H, W, C, K, R, S, stride, pad)
        (1, 2, 2, 16, 16, 3, 3, 2, 0),
        (1, 2, 2, 16, 16, 3, 3, 1, 0),
        (1, 4, 4, 16, 16, 7, 7, 2, 1),
        (1, 4, 4, 16, 16, 7, 7, 3, 1),
        (1, 8, 2, 16, 16, 3, 3, 2, 0),           # only the width is too small
        (1, 2, 8, 16, 16, 3, 3, 2, 0),           # only the height
        (1, 8, 2, 16, 16, 1, 5, 2, 1),           # R != S: W + 2 pad = 4 < S = 5
    ]
    for n, H, W, C, K, R, S, st, pad in bad:
        geom = (n, H, W, C, K, R, S, st, pad)
        assert L.apg_conv_bwd_workspace_bytes(*geom) < 0, geom       # first: the calls below must never reach a launch
        assert L.apg_conv_fwd(fake, n, H, W, C, fake, K, R, S, st, pad, fake, None) == EINVAL, geom
        assert "apg_conv_fwd" in _err(L)
        assert L.apg_conv_bwd(fake, n, H, W, C, fake, K, R, S, st, pad, fake, fake, fake, fake, 1 << 30, None) == EINVAL, geom
        assert "apg_conv_bwd" in _err(L)
    # the boundary: the kernel exactly covers the padded input -> Ho = Wo = 1, valid at stride 1 and 2
    for geom in [(1, 1, 1, 16, 16, 3, 3, 2, 1), (1, 3, 3, 16, 16, 3, 3, 2, 0), (1, 4, 4, 16, 16, 6, 6, 2, 1),
                 (1, 3, 3, 16, 16, 3, 3, 1, 0), (2, 2, 6, 16, 16, 4, 8, 2, 1)]:
        n, H, W, C, K, R, S, st, pad = geom
        nb = L.apg_conv_bwd_workspace_bytes(*geom)
        assert nb > 0 and nb % (4 * K * C * R * S) == 0, geom                # accepted: whole split-K chunks of gw
