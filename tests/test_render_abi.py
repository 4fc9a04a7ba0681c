"""CPU checks of the apg_render_* entry points of libairpose_grad.so (airpose_amd/csrc/render.hip): declared == exported == bound, the
two ABI numbers stay where they are, and every refusal happens on the host -- the pointers below are made-up addresses that are never
dereferenced (there is no GPU here), the result is APG_EINVAL / APG_ENOMEM and the message names the argument."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL, ENOMEM = -1, -4
FAKE = 0x7f0000001000                                    # 4096-aligned and never touched
PTRS = ("vertices", "faces", "csr_offsets", "csr_faces", "R", "t", "background", "out_rgb", "out_depth", "out_face", "workspace")
INF, NAN = float("inf"), float("nan")


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _args(**over):
    """a valid argument set of apg_render_overlay on made-up addresses; `over` replaces entries"""
    a = dict(n=2, V=100, F=196, H=48, W=64, csr_len=588, fx=60.0, fy=55.0, cx=31.5, cy=24.25, znear=0.05, zfar=100.0, base_r=0.8,
             base_g=0.3, base_b=0.3, ambient=0.5, diffuse=0.76, workspace_bytes=1 << 24)
    a.update({p: FAKE + 0x100000 * (k + 1) for k, p in enumerate(PTRS)})
    a.update(over)
    return a


def _call(a):
    G, L = _lib()
    vp = ctypes.c_void_p
    rc = L.apg_render_overlay(a["n"], a["V"], a["F"], a["H"], a["W"], vp(a["vertices"]), vp(a["faces"]), vp(a["csr_offsets"]),
                              vp(a["csr_faces"]), a["csr_len"], vp(a["R"]), vp(a["t"]), a["fx"], a["fy"], a["cx"], a["cy"], a["znear"],
                              a["zfar"], vp(a["background"]), a["base_r"], a["base_g"], a["base_b"], a["ambient"], a["diffuse"],
                              vp(a["out_rgb"]), vp(a["out_depth"]), vp(a["out_face"]), vp(a["workspace"]), a["workspace_bytes"], None)
    return rc, L.apg_last_error().decode()


REFUSALS = [
    ("n_negative", dict(n=-1), "n "),
    ("n_too_large", dict(n=65536), "n "),
    ("V_zero", dict(V=0), "V "),
    ("V_too_large", dict(V=(1 << 24) + 1), "V "),
    ("F_zero", dict(F=0), "F "),
    ("F_too_large", dict(F=(1 << 24) + 1, csr_len=0), "F "),
    ("H_zero", dict(H=0), "H "),
    ("H_too_large", dict(H=16385), "H "),
    ("W_zero", dict(W=0), "W "),
    ("W_negative", dict(W=-5), "W "),
    ("csr_len_negative", dict(csr_len=-1), "csr_len"),
    ("csr_len_above_3F", dict(csr_len=589), "csr_len"),
    ("null_vertices", dict(vertices=None), "vertices"),
    ("null_faces", dict(faces=None), "faces"),
    ("null_csr_offsets", dict(csr_offsets=None), "csr_offsets"),
    ("null_csr_faces", dict(csr_faces=None), "csr_faces"),
    ("null_out_rgb", dict(out_rgb=None), "out_rgb"),
    ("null_workspace", dict(workspace=None), "workspace"),
    ("fx_zero", dict(fx=0.0), "fx"),
    ("fx_nan", dict(fx=NAN), "fx"),
    ("fy_negative", dict(fy=-1.0), "fy"),
    ("fy_inf", dict(fy=INF), "fy"),
    ("cx_nan", dict(cx=NAN), "cx"),
    ("cy_inf", dict(cy=INF), "cy"),
    ("znear_zero", dict(znear=0.0), "znear"),
    ("zfar_below_znear", dict(zfar=0.01), "zfar"),
    ("zfar_inf", dict(zfar=INF), "zfar"),
    ("base_r_negative", dict(base_r=-0.1), "base_r"),
    ("base_g_nan", dict(base_g=NAN), "base_g"),
    ("base_b_inf", dict(base_b=INF), "base_b"),
    ("ambient_negative", dict(ambient=-1.0), "ambient"),
    ("diffuse_nan", dict(diffuse=NAN), "diffuse"),
    ("out_rgb_is_background", dict(out_rgb=FAKE + 0x700000), "background"),
    ("workspace_8_mod_16", dict(workspace=FAKE + 0x100000 * 11 + 8), "workspace"),
] + [("misaligned_" + p, {p: FAKE + 0x100000 * (k + 1) + 2}, p) for k, p in enumerate(PTRS)]


def test_header_exports_and_binding_agree_on_the_render_names():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_render_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_render_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_render_"))
    assert declared == exported == bound == ["apg_render_overlay", "apg_render_workspace_bytes"]


def test_abi_numbers_stay():
    from airpose_amd import _native
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2
    assert _native.ABI_VERSION == 13
    assert not any(n.startswith("apg_") for n in _native.SIGNATURES)


def test_the_valid_argument_set_is_only_refused_for_what_a_case_changes():
    """n = 0 with the same made-up pointers succeeds (no launch), so each refusal below is due to its own change"""
    rc, msg = _call(_args(n=0))
    assert rc == 0, msg
    rc, msg = _call(_args(n=0, R=None, t=None, background=None, out_depth=None, out_face=None))
    assert rc == 0, msg


@pytest.mark.parametrize("over,names", [(r[1], r[2]) for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _call(_args(**over))
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_render_overlay: ") and names in msg[len("apg_render_overlay: "):], msg


def test_a_workspace_one_byte_short_is_refused():
    _, L = _lib()
    need = L.apg_render_workspace_bytes(2, 48, 64, 100, 196)
    rc, msg = _call(_args(workspace_bytes=need - 1))
    assert rc == ENOMEM and "workspace" in msg, (rc, msg)
    rc, msg = _call(_args(n=0, workspace_bytes=L.apg_render_workspace_bytes(0, 48, 64, 100, 196) - 1))
    assert rc == ENOMEM and "workspace" in msg, (rc, msg)


def test_the_workspace_query_is_monotone():
    _, L = _lib()
    q = lambda n, H, W, V, F: L.apg_render_workspace_bytes(n, H, W, V, F)
    base = dict(n=2, H=48, W=64, V=100, F=196)
    for key, values in (("n", [0, 1, 2, 3, 8, 64, 1000]), ("H", [1, 2, 47, 48, 49, 224, 1080, 16384]), ("W", [1, 63, 64, 65, 1920, 16384]),
                        ("V", [1, 99, 100, 101, 10475, 1 << 24]), ("F", [1, 195, 196, 197, 20908, 1 << 24])):
        prev = 0
        for x in values:
            b = q(**dict(base, **{key: x}))
            assert b > 0 and b % 8 == 0 and b >= prev, (key, x, b, prev)
            prev = b
        assert prev > q(**dict(base, **{key: values[1]})), key
    for bad in (dict(n=-1), dict(n=65536), dict(H=0), dict(W=16385), dict(V=0), dict(F=(1 << 24) + 1), dict(n=65535, H=16384, W=16384)):
        assert q(**dict(base, **bad)) < 0, bad
