"""CPU checks of the generic view-local head's C ABI (apg_head_local_fwd / apg_head_local_bwd, head_local_grad.hip): the header,
the library's exports and the ctypes table agree on the new entries, the ABI numbers did not move, and bad layouts or a short
workspace are refused on the host before any launch (there is no GPU here)."""
import ctypes
import os
import re
import subprocess

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
NEW = ("apg_head_local_bwd", "apg_head_local_bwd_workspace_bytes", "apg_head_local_fwd")
APG_EINVAL, APG_ENOMEM = -1, -4
FAKE = ctypes.c_void_p(4096)                                  # a non-NULL "device pointer": refused calls never touch it


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def test_header_exports_and_binding_agree_on_the_new_entries():
    G, L = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(apg_[a-z0-9_]+)\s*\(", src))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(apg_[a-z0-9_]+)$", syms, flags=re.M))
    for n in NEW:
        assert n in declared and n in exported and n in G.SIGNATURES, n
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(G.SIGNATURES[n][1]), (n, "argument count of the header and of the ctypes table")
        assert getattr(L, n).argtypes == G.SIGNATURES[n][1]
    assert declared == exported == set(G.SIGNATURES)
    assert "#define APG_HEAD_LOCAL_MAX_SEG 8" in src and "#define APG_HEAD_LOCAL_MAX_DEC 3" in src


def test_abi_numbers_did_not_move():
    from airpose_amd import _native
    G, L = _lib()
    assert L.apg_abi_version() == 2 == G.ABI_VERSION
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert _native.ABI_VERSION == 13 and not any(n.startswith("apg_") for n in _native.SIGNATURES)


def _fwd(L, G, R, seg_w, dec_n, dec_res, nseg=None, ndec=None):
    nseg = len(seg_w) if nseg is None else nseg
    ndec = len(dec_n) if ndec is None else ndec
    segs = (ctypes.c_void_p * max(len(seg_w), 1))(*[4096] * len(seg_w))
    decs = (ctypes.c_void_p * max(len(dec_n), 1))(*[4096] * len(dec_n))
    return L.apg_head_local_fwd(R, FAKE, nseg, segs, G.ints(list(seg_w)), G.ints(list(seg_w)), FAKE, FAKE, FAKE, FAKE, ndec, decs,
                                decs, G.ints(list(dec_n)), G.ints(list(dec_res)), 1, 0.0, 0.0, FAKE, FAKE, FAKE, FAKE, decs, None)


def _bwd(L, G, R, seg_w, dec_n, dec_res, ws_bytes, nseg=None, ndec=None):
    nseg = len(seg_w) if nseg is None else nseg
    ndec = len(dec_n) if ndec is None else ndec
    gseg = (ctypes.c_void_p * max(len(seg_w), 1))()
    gout = (ctypes.c_void_p * max(len(dec_n), 1))()
    gpar = (ctypes.c_void_p * (4 + 2 * max(len(dec_n), 1)))()
    return L.apg_head_local_bwd(R, nseg, G.ints(list(seg_w)), G.ints([0] * len(seg_w)), ndec, G.ints(list(dec_n)),
                                G.ints(list(dec_res)), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 0.0, 0.0, gout, gpar, None, gseg,
                                FAKE, ws_bytes, None)


HMR = ((132, 10, 3), (132, 10, 3), (0, 132, 142))


def test_bad_descriptors_are_refused_on_the_host():
    G, L = _lib()
    big = 1 << 40
    for call in (lambda *a, **k: _fwd(L, G, *a, **k), lambda *a, **k: _bwd(L, G, *a, ws_bytes=big, **k)):
        assert call(4, (3,) * 9, (3,), (0,)) == APG_EINVAL                       # more than 8 segments
        assert b"segments" in L.apg_last_error()
        assert call(4, (3,), (1,), (0,), nseg=0) == APG_EINVAL
        assert call(4, (135,), (3, 3, 3, 3), (0, 3, 6, 9)) == APG_EINVAL        # more than 3 decoders
        assert b"decoders" in L.apg_last_error()
        assert call(4, (135,), (3,), (0,), ndec=0) == APG_EINVAL
        assert call(4, (132, 10, 3), (132, 10, 3), (0, 132, 143)) == APG_EINVAL  # the last residual range ends one past the segments
        assert b"residual" in L.apg_last_error()
        assert call(4, (132, 10, 3), (132, 10, 3), (-1, 132, 142)) == APG_EINVAL
        assert call(0, *HMR) == APG_EINVAL                                       # R < 1
        assert b"R < 1" in L.apg_last_error()
        assert call(-3, *HMR) == APG_EINVAL
        assert call(4, (132, 0, 3), (3,), (0,)) == APG_EINVAL                    # an empty segment
    assert L.apg_head_local_fwd(4, None, 1, None, None, G.ints([3]), None, None, None, None, 1, None, None, G.ints([3]), G.ints([0]),
                                1, 0.0, 0.0, None, None, None, None, None, None) == APG_EINVAL           # NULL pointers


def test_workspace_query_and_short_workspace():
    G, L = _lib()
    q = L.apg_head_local_bwd_workspace_bytes
    assert q(0, 2193, 145, 0) < 0 and q(4, 2048, 145, 0) < 0 and q(4, 2193, 0, 0) < 0
    for K1, N in ((2193, 145), (2329, 145), (2196, 145), (2332, 145)):
        for R in (1, 5, 33, 65):
            a, b = q(R, K1, N, 0), q(R, K1, N, 1)
            assert 0 < a < b and a % 4 == 0
            assert b - a >= R * 2048 * 4                                         # the feature columns of g_xc
            assert a >= 4 * R * (N + 2 * 1024 + 2 * (K1 - 2048))
    need = q(5, 2193, 145, 0)
    assert _bwd(L, G, 5, *HMR, ws_bytes=need - 1) == APG_ENOMEM
    assert b"workspace" in L.apg_last_error()
    assert _bwd(L, G, 5, *HMR, ws_bytes=0) == APG_ENOMEM


def test_workspace_sizes_of_both_heads_are_pinned():
    """The byte counts are ABI (callers allocate by them): the closed form, a(n) = n rounded up to 64 floats, and the answers of
    the library before the heads shared their chain."""
    G, L = _lib()
    a = lambda n: (n + 63) // 64 * 64
    part = lambda R: a((R + 31) // 32 * 1024)
    two = {1: (617984, 634368), 33: (1260288, 1800960), 257: (5756416, 9967104)}
    for B, want in two.items():
        R = 2 * B
        for gxf in (0, 1):
            form = 4 * (a(145 * R) + a(145 * 1024) + 2 * a(1024 * R) + a(R * (2332 - (0 if gxf else 2048))) + part(R))
            assert L.apg_head_bwd_workspace_bytes(B, gxf) == form == want[gxf], (B, gxf)
    local = {(2193, 145): {1: (14592, 22784), 33: (336128, 606464), 65: (658432, 1190912)},
             (2332, 145): {1: (15616, 23808), 33: (372992, 643328), 65: (730624, 1263104)}}
    for (K1, N), rows in local.items():
        for R, want in rows.items():
            for gxf in (0, 1):
                form = 4 * (a(R * N) + 2 * a(1024 * R) + a(R * (K1 - (0 if gxf else 2048))) + a(R * (K1 - 2048)) + part(R))
                assert L.apg_head_local_bwd_workspace_bytes(R, K1, N, gxf) == form == want[gxf], (K1, N, R, gxf)
