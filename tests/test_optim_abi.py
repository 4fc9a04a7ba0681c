"""CPU checks of apg_adam_step's C ABI (airpose_amd/csrc/optim.hip, include/airpose_grad.h): the export, the header's text, the ctypes
signature, and every refusal -- each returns APG_EINVAL on the host, before any GPU call (there is no GPU here: a call that got as
far as a launch would return a HIP error code instead), and leaves a message that names the argument."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
APG_EINVAL = -1
C = ctypes


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G.lib()


def test_export_header_and_signature():
    from airpose_amd import _native_grad as G
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\sT\s+apg_adam_step$", syms, flags=re.M)
    text = open(HEADER).read()
    decl = re.search(r"int apg_adam_step\((.*?)\);", text, flags=re.S)
    assert decl, "include/airpose_grad.h does not declare apg_adam_step"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["int ntensors", "const void* const* p", "const void* const* g", "const void* const* m", "const void* const* v",
                    "const void* const* vmax", "const int64_t* numel", "const int64_t* step", "double lr", "double beta1", "double beta2",
                    "double eps", "double weight_decay", "void* stream"]
    for phrase in ("must not overlap", "step count AFTER this update", "_single_tensor_adam", "apg_adam_step"):
        assert phrase in text, phrase
    res, argtypes = G.SIGNATURES["apg_adam_step"]
    vpp, i64p = C.POINTER(C.c_void_p), C.POINTER(C.c_int64)
    assert res is C.c_int
    assert argtypes == [C.c_int] + [vpp] * 5 + [i64p] * 2 + [C.c_double] * 5 + [C.c_void_p]
    assert L.apg_adam_step.argtypes == argtypes and L.apg_adam_step.restype is C.c_int
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", text).group(1)) == 2 == G.ABI_VERSION      # additive under ABI 2


def _call(L, n=2, tables=None, numel=(8, 8), step=(1, 1), lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, null=()):
    """apg_adam_step on made-up, never dereferenced device addresses; tables: per name a list of addresses; null: tables passed as NULL"""
    t = dict(p=[0x1000, 0x2000], g=[0x3000, 0x4000], m=[0x5000, 0x6000], v=[0x7000, 0x8000], vmax=[0x9000, 0xa000])
    t.update(tables or {})
    arr = {k: None if k in null else (C.c_void_p * max(n, 1))(*[a or None for a in t[k]][:max(n, 1)]) for k in t}
    ne = None if "numel" in null else (C.c_int64 * max(n, 1))(*numel[:max(n, 1)])
    st = None if "step" in null else (C.c_int64 * max(n, 1))(*step[:max(n, 1)])
    rc = L.apg_adam_step(n, arr["p"], arr["g"], arr["m"], arr["v"], arr["vmax"], ne, st, lr, b1, b2, eps, wd, None)
    return rc, L.apg_last_error().decode()


REFUSALS = [
    ("ntensors", dict(n=-1)),
    ("p table", dict(null=("p",))), ("g table", dict(null=("g",))), ("m table", dict(null=("m",))), ("v table", dict(null=("v",))),
    ("numel", dict(null=("numel",))), ("step", dict(null=("step",))),
    ("p of tensor 1", dict(tables=dict(p=[0x1000, 0]))), ("g of tensor 0", dict(tables=dict(g=[0, 0x4000]))),
    ("m of tensor 1", dict(tables=dict(m=[0x5000, 0]))), ("v of tensor 0", dict(tables=dict(v=[0, 0x8000]))),
    ("vmax of tensor 1", dict(tables=dict(vmax=[0x9000, 0]))),
    ("step of tensor 1", dict(step=(1, 0))), ("step of tensor 0", dict(step=(-3, 1))),
    ("lr", dict(lr=-1e-3)), ("lr", dict(lr=float("nan"))),
    ("eps", dict(eps=-1e-8)),
    ("beta1", dict(b1=1.0)), ("beta1", dict(b1=-0.1)), ("beta2", dict(b2=1.0)), ("beta2", dict(b2=-1e-3)), ("beta2", dict(b2=float("nan"))),
    ("weight_decay", dict(wd=-1e-4)),
    ("numel of tensor 1", dict(numel=(8, -1))),
    ("p of tensor 0 is not 4-byte aligned", dict(tables=dict(p=[0x1002, 0x2000]))),
    ("g of tensor 1 is not 4-byte aligned", dict(tables=dict(g=[0x3000, 0x4001]))),
    ("m of tensor 0 is not 4-byte aligned", dict(tables=dict(m=[0x5003, 0x6000]))),
    ("v of tensor 1 is not 4-byte aligned", dict(tables=dict(v=[0x7000, 0x8002]))),
    ("vmax of tensor 0 is not 4-byte aligned", dict(tables=dict(vmax=[0x9001, 0xa000]))),
]


@pytest.mark.parametrize("names,kw", REFUSALS, ids=["%s-%d" % (r[0].replace(" ", "_"), i) for i, r in enumerate(REFUSALS)])
def test_refusals_run_on_the_host_and_name_the_argument(names, kw):
    L = _lib()
    rc, msg = _call(L, **kw)
    assert rc == APG_EINVAL, (rc, msg)
    assert msg.startswith("apg_adam_step:") and names in msg, msg


def test_accepted_without_a_launch():
    """no tensor, or only tensors without elements (their pointers may be NULL): APG_OK and nothing to launch"""
    L = _lib()
    assert _call(L, n=0)[0] == 0
    assert _call(L, n=0, null=("vmax",))[0] == 0
    assert _call(L, n=2, numel=(0, 0), tables=dict(p=[0, 0], g=[0, 0], m=[0, 0], v=[0, 0], vmax=[0, 0]))[0] == 0
    # a NULL pointer under a tensor with elements is refused even next to empty ones, and a refused vmax pointer needs the vmax table
    assert _call(L, n=2, numel=(0, 8), tables=dict(m=[0, 0]))[0] == APG_EINVAL
    assert _call(L, n=2, numel=(0, 0), tables=dict(vmax=[0, 0x9002]), null=("vmax",))[0] == 0
