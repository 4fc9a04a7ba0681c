"""CPU checks of libairpose_grad.so's C ABI: the header's declarations, the library's exports and the ctypes table agree one to
one, and the library reports the header's ABI number and its target (no compute calls: there is no GPU here)."""
import ctypes
import os
import re
import subprocess

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(apg_[a-z0-9_]+)\s*\(", src)))


def _lib_path():
    from airpose_amd import _native_grad
    if not os.path.isfile(_native_grad.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native_grad.LIB_PATH


def test_header_exports_and_binding_agree():
    from airpose_amd import _native_grad
    path = _lib_path()
    names = _declared()
    assert len(names) >= 10
    syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_[a-z0-9_]+)$", syms, flags=re.M)))
    assert exported == names
    assert sorted(_native_grad.SIGNATURES) == names
    L = _native_grad.lib()
    for n in names:
        assert getattr(L, n).argtypes is not None or _native_grad.SIGNATURES[n][1] == [], n


def test_abi_version_and_target():
    from airpose_amd import _native_grad
    want = int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    L = ctypes.CDLL(_lib_path())
    L.apg_abi_version.restype = ctypes.c_int
    L.apg_version.restype = ctypes.c_char_p
    assert L.apg_abi_version() == want == _native_grad.ABI_VERSION
    assert b"gfx950" in L.apg_version()
    assert ("abi %d" % want).encode() in L.apg_version()


def test_argument_checks_run_on_the_host():
    """Bad arguments are refused before any launch, with a message in apg_last_error()."""
    from airpose_amd import _native_grad as G
    L = G.lib()
    assert L.apg_dropout_mask(1, 1, 0, 4, 0.5, None, None) == -1
    assert b"apg_dropout_mask" in L.apg_last_error()
    assert L.apg_rot6d_to_rotmat_bwd(None, 4, None, None, None) == -1
    assert L.apg_head_bwd_workspace_bytes(0, 0) < 0
    assert L.apg_head_bwd_workspace_bytes(8, 1) > L.apg_head_bwd_workspace_bytes(8, 0) > 0


def test_inference_library_is_untouched_by_the_grad_entry_points():
    from airpose_amd import _native
    assert _native.ABI_VERSION == 13                                # (13: the trunk-form operator entries; no apg_ entry ever moved it)
    assert not any(n.startswith("apg_") for n in _native.SIGNATURES)
