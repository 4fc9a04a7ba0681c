"""CPU checks of the gradient-norm entries' C ABI (airpose_amd/csrc/guard/grad_guard.hip, include/airpose_grad.h): apg_grad_norm,
apg_grad_norm_workspace_bytes, apg_grad_scale and apg_adam_step_guarded -- the exports, the header's text, the ctypes signatures, and
every refusal: each returns APG_EINVAL on the host, before any GPU call (there is no GPU here: a call that got as far as a launch would
return a HIP error code instead), on made-up addresses that are never dereferenced, and leaves a message that names the argument.
Then the Python side without a GPU: the refusals of airpose_amd.clip_grad_norm_ and of FusedAdam's new options, and that the options
at their defaults leave the call FusedAdam builds, and its param groups, as they were."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
APG_EINVAL = -1
C = ctypes
ENTRIES = ("apg_grad_norm", "apg_grad_norm_workspace_bytes", "apg_grad_scale", "apg_adam_step_guarded")


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G.lib()


def test_exports_header_and_signatures():
    from airpose_amd import _native_grad as G
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"\sT\s+%s$" % name, syms, flags=re.M), name
        assert name in G.SIGNATURES and getattr(L, name).argtypes == G.SIGNATURES[name][1], name

    def args(name, ret):
        decl = re.search(r"%s %s\((.*?)\);" % (ret, name), text, flags=re.S)
        assert decl, "include/airpose_grad.h does not declare %s" % name
        return [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args("apg_grad_norm_workspace_bytes", "int64_t") == ["int ntensors", "const int64_t* numel"]
    assert args("apg_grad_norm", "int") == ["int ntensors", "const void* const* g", "const int64_t* numel", "double max_norm",
                                            "int skip_nonfinite", "void* workspace", "int64_t workspace_bytes", "void* guard",
                                            "float* per_tensor", "int64_t* counters", "void* stream"]
    assert args("apg_grad_scale", "int") == ["int ntensors", "const void* const* g", "const int64_t* numel", "const void* guard", "void* stream"]
    assert args("apg_adam_step_guarded", "int") == args("apg_adam_step", "int")[:-1] + ["const void* guard", "void* stream"]
    vpp, i64p, vp = C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p
    assert G.SIGNATURES["apg_grad_norm_workspace_bytes"] == (C.c_int64, [C.c_int, i64p])
    assert G.SIGNATURES["apg_grad_norm"] == (C.c_int, [C.c_int, vpp, i64p, C.c_double, C.c_int, vp, C.c_int64, vp, vp, vp, vp])
    assert G.SIGNATURES["apg_grad_scale"] == (C.c_int, [C.c_int, vpp, i64p, vp, vp])
    assert G.SIGNATURES["apg_adam_step_guarded"] == (C.c_int, G.SIGNATURES["apg_adam_step"][1][:-1] + [vp, vp])
    for phrase in ("accumulated in fp64", "clip_coef_clamped", "offset 8   int32   skip", "coef is written as NaN", "the record is always written",
                   "No floating-point atomics", "step[i] is the host's count"):
        assert phrase in text, phrase
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", text).group(1)) == 2 == G.ABI_VERSION      # additive under ABI 2
    assert int(re.search(r"#define\s+APG_GUARD_BYTES\s+(\d+)", text).group(1)) == G.GUARD_BYTES == 16
    assert int(re.search(r"#define\s+APG_GRAD_NORM_BATCH\s+(\d+)", text).group(1)) == G.GRAD_NORM_BATCH


def test_workspace_bytes():
    L = _lib()
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    assert L.apg_grad_norm_workspace_bytes(0, None) == 0
    assert L.apg_grad_norm_workspace_bytes(3, i64(0, 0, 0)) == 3 * 8
    assert L.apg_grad_norm_workspace_bytes(4, i64(1, 4096, 4097, 0)) == (1 + 1 + 2 + 0 + 4) * 8      # a chunk is 4096 elements
    assert L.apg_grad_norm_workspace_bytes(-1, i64(1)) < 0
    assert L.apg_grad_norm_workspace_bytes(1, None) < 0
    assert L.apg_grad_norm_workspace_bytes(2, i64(8, -1)) < 0


def _norm(L, n=2, g=(0x1000, 0x2000), numel=(8, 8), max_norm=1.0, skip=0, ws=0x10000, ws_bytes=None, guard=0x20000, pt=0x30000,
          counters=0x40000, null=()):
    gt = None if "g" in null else (C.c_void_p * max(n, 1))(*[a or None for a in g][:max(n, 1)])
    ne = None if "numel" in null else (C.c_int64 * max(n, 1))(*numel[:max(n, 1)])
    if ws_bytes is None:
        ws_bytes = max(L.apg_grad_norm_workspace_bytes(n, ne), 0) if ne is not None else 64
    rc = L.apg_grad_norm(n, gt, ne, max_norm, skip, ws or None, ws_bytes, guard or None, pt or None, counters or None, None)
    return rc, L.apg_last_error().decode()


NORM_REFUSALS = [
    ("ntensors", dict(n=-1)),
    ("g table is NULL", dict(null=("g",))),
    ("numel array is NULL", dict(null=("numel",))),
    ("numel of tensor 1 is negative", dict(numel=(8, -1))),
    ("g of tensor 0 is NULL", dict(g=(0, 0x2000))),
    ("g of tensor 1 is not 4-byte aligned", dict(g=(0x1000, 0x2002))),
    ("g of tensor 0 is not 4-byte aligned", dict(g=(0x1001, 0x2000), numel=(0, 8))),
    ("max_norm", dict(max_norm=-1.0)),
    ("max_norm", dict(max_norm=float("nan"))),
    ("guard record is NULL", dict(guard=0)),
    ("guard record is not 4-byte aligned", dict(guard=0x20002)),
    ("workspace", dict(ws_bytes=8)),
    ("workspace", dict(ws=0)),
    ("workspace is not 8-byte aligned", dict(ws=0x10004)),
]


@pytest.mark.parametrize("names,kw", NORM_REFUSALS, ids=["%s-%d" % (r[0].replace(" ", "_"), i) for i, r in enumerate(NORM_REFUSALS)])
def test_grad_norm_refusals_run_on_the_host_and_name_the_argument(names, kw):
    L = _lib()
    rc, msg = _norm(L, **kw)
    assert rc == APG_EINVAL, (rc, msg)
    assert msg.startswith("apg_grad_norm:") and names in msg, msg


def test_grad_norm_workspace_message_states_both_sizes():
    rc, msg = _norm(_lib(), numel=(4097, 8), ws_bytes=32)
    assert rc == APG_EINVAL and "32 bytes" in msg and "asks for 40" in msg, msg


SCALE_REFUSALS = [
    ("ntensors", dict(n=-1)),
    ("g table is NULL", dict(null=("g",))),
    ("numel array is NULL", dict(null=("numel",))),
    ("numel of tensor 0 is negative", dict(numel=(-2, 8))),
    ("g of tensor 1 is NULL", dict(g=(0x1000, 0))),
    ("g of tensor 0 is not 4-byte aligned", dict(g=(0x1003, 0x2000))),
    ("guard record is NULL", dict(guard=0)),
    ("guard record is not 4-byte aligned", dict(guard=0x20001)),
]


@pytest.mark.parametrize("names,kw", SCALE_REFUSALS, ids=["%s-%d" % (r[0].replace(" ", "_"), i) for i, r in enumerate(SCALE_REFUSALS)])
def test_grad_scale_refusals(names, kw):
    L = _lib()
    n, g, numel, guard, null = kw.get("n", 2), kw.get("g", (0x1000, 0x2000)), kw.get("numel", (8, 8)), kw.get("guard", 0x20000), kw.get("null", ())
    gt = None if "g" in null else (C.c_void_p * 2)(*[a or None for a in g])
    ne = None if "numel" in null else (C.c_int64 * 2)(*numel)
    rc = L.apg_grad_scale(n, gt, ne, guard or None, None)
    msg = L.apg_last_error().decode()
    assert rc == APG_EINVAL and msg.startswith("apg_grad_scale:") and names in msg, (rc, msg)
    # no tensor with elements: accepted, and nothing to launch
    assert L.apg_grad_scale(0, gt or (C.c_void_p * 1)(), ne or (C.c_int64 * 1)(), 0x20000, None) == 0
    assert L.apg_grad_scale(2, (C.c_void_p * 2)(), (C.c_int64 * 2)(0, 0), 0x20000, None) == 0


def _guarded(L, guard=0x20000, **kw):
    """apg_adam_step_guarded on test_optim_abi's made-up tables"""
    t = dict(p=[0x1000, 0x2000], g=[0x3000, 0x4000], m=[0x5000, 0x6000], v=[0x7000, 0x8000], vmax=[0x9000, 0xa000])
    t.update(kw.get("tables", {}))
    null = kw.get("null", ())
    arr = {k: None if k in null else (C.c_void_p * 2)(*[a or None for a in t[k]]) for k in t}
    ne, st = (C.c_int64 * 2)(*kw.get("numel", (8, 8))), (C.c_int64 * 2)(*kw.get("step", (1, 1)))
    rc = L.apg_adam_step_guarded(kw.get("n", 2), arr["p"], arr["g"], arr["m"], arr["v"], arr["vmax"], ne, st, kw.get("lr", 1e-3), 0.9, 0.999,
                                 1e-8, kw.get("wd", 0.0), guard or None, None)
    return rc, L.apg_last_error().decode()


GUARDED_REFUSALS = [
    ("guard record is NULL", dict(guard=0)),
    ("guard record is not 4-byte aligned", dict(guard=0x20002)),
    ("ntensors", dict(n=-1)), ("lr", dict(lr=-1.0)), ("weight_decay", dict(wd=-1e-4)),
    ("m table", dict(null=("m",))), ("step of tensor 1", dict(step=(1, 0))), ("numel of tensor 0", dict(numel=(-1, 8))),
    ("g of tensor 1 is not 4-byte aligned", dict(tables=dict(g=[0x3000, 0x4001]))),
    ("vmax of tensor 0 is NULL", dict(tables=dict(vmax=[0, 0xa000]))),
]


@pytest.mark.parametrize("names,kw", GUARDED_REFUSALS, ids=["%s-%d" % (r[0].replace(" ", "_"), i) for i, r in enumerate(GUARDED_REFUSALS)])
def test_guarded_step_refusals(names, kw):
    rc, msg = _guarded(_lib(), **kw)
    assert rc == APG_EINVAL, (rc, msg)
    assert msg.startswith("apg_adam_step_guarded:") and names in msg, msg


def test_guarded_step_without_elements_is_accepted_without_a_launch():
    L = _lib()
    z = dict(p=[0, 0], g=[0, 0], m=[0, 0], v=[0, 0], vmax=[0, 0])
    assert _guarded(L, n=0)[0] == 0
    assert _guarded(L, numel=(0, 0), tables=z)[0] == 0
    # the unguarded entry still words its refusals with its own name
    rc = L.apg_adam_step(-1, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None)
    assert rc == APG_EINVAL and L.apg_last_error().decode().startswith("apg_adam_step: ntensors")


def test_the_guard_source_is_scanned_here_and_optim_still_scans_as_the_committed_list_says():
    """tests/packed_math_scan.json (SRCS and GRAD_SRCS) and tests/test_roll_abi.py (roll.hip the one source linked apart, every
    csrc/*.hip in one of the two) are existing test files and stay as they are, so guard/grad_guard.hip is linked through GUARD_UNITS
    from a directory of its own and held HERE to what the list holds the others to: the scan tool sees it (linked_below), every .hip
    file below csrc is named by that variable, the kernels that read LDS carry no packed fp32 math at all -- so none has the SUSPECT
    signature of tests/test_packed_math_scan.py (packed fp32 math with op_sel in a kernel that reads LDS) --, and the scan is not blind
    to the source (it does see the guarded Adam kernels' packed math).  optim.hip, which now shares adam_seq.inc with it, still scans
    exactly as the committed list says: the two kernels of before, name for name and count for count."""
    import glob
    import json
    import shutil
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import packed_math_scan as S
    csrc = os.path.join(REPO, "airpose_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^GUARD_UNITS\s*=\s*guard/grad_guard\.hip\s*$", text, re.M)
    assert re.search(r"^GRAD_OBJS\s*=.*\$\(GUARD_UNITS:\.hip=\.o\)", text, re.M)
    assert re.search(r"^GRAD_HDRS\s*=.*\badam_seq\.inc\b", text, re.M)
    assert "FLAGS_guard" not in text and "FLAGS_optim" not in text          # neither source needs a flag, and optim.hip gained none
    hipcc, _, flags, _, listed = S.makefile()
    assert shutil.which(hipcc), "%s: the scan needs the compiler the build uses" % hipcc
    below = S.linked_below()
    assert below == ["guard/grad_guard"] and "guard/grad_guard" not in listed and S.linked_apart() == ["roll"]
    deeper = sorted(os.path.relpath(f, csrc)[:-4] for f in glob.glob(os.path.join(csrc, "*", "**", "*.hip"), recursive=True))
    assert deeper == below, "a kernel source below csrc that neither a committed list nor this test scans"
    rows = {r["kernel"]: r for r in S.scan_sources(below)}
    assert sorted(rows) == ["adam_guarded_kernel<false>", "adam_guarded_kernel<true>", "grad_norm_chunk_kernel", "grad_norm_final_kernel",
                            "grad_norm_tensor_kernel", "grad_scale_kernel"]
    for name, r in rows.items():
        assert r["flags"] == "" and not (r["op_sel"] > 0 and r["ds_reads"] > 0), r     # not the signature
        if name.startswith("grad_norm"):
            assert r["ds_reads"] > 0 and r["packed"] == 0, r                # fp64 accumulation: no packed fp32 math beside the LDS reads
        else:
            assert r["ds_reads"] == 0 and r["packed"] > 0, r                # the detector is not blind to this source
    with open(S.OUT) as f:
        d = json.load(f)
    want = [dict(zip(d["columns"], r)) for r in d["kernels"] if r[0] == "optim.hip"]
    assert [r["kernel"] for r in want] == ["adam_kernel<false>", "adam_kernel<true>"]
    assert S.scan_sources(["optim"]) == want
    G = __import__("airpose_amd._native_grad", fromlist=["x"])
    _lib()                                                                    # ... and the built library is the one with these kernels in it
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "apg_grad_norm" in syms and "apg_adam_step_guarded" in syms


# ------------------------------------------------------------------------------------------------ Python, without a GPU
def _with_grad(t, g=None):
    p = torch.nn.Parameter(t)
    p.grad = torch.zeros_like(t) if g is None else g
    return p


def test_clip_grad_norm_refusals_by_name():
    import airpose_amd
    clip = airpose_amd.clip_grad_norm_
    from airpose_amd.optim import clip_grad_norm_
    assert clip is clip_grad_norm_
    p = _with_grad(torch.randn(4, 3))
    for bad in (1.0, 3, float("inf"), "inf"):
        with pytest.raises((ValueError, TypeError), match="norm_type"):
            clip([p], 1.0, norm_type=bad)
    with pytest.raises(ValueError, match="max_norm"):
        clip([p], -1.0)
    with pytest.raises(ValueError, match="max_norm"):
        clip([p], float("nan"))
    with pytest.raises(TypeError, match="max_norm"):
        clip([p], torch.tensor(1.0))
    with pytest.raises(ValueError, match="cpu"):                               # a CPU gradient: there is no fallback
        clip([p], 1.0)
    with pytest.raises(ValueError, match="cpu"):
        clip(p, 1.0)                                                          # a single tensor, as torch takes it
    sp = torch.nn.Parameter(torch.randn(4, 3))
    sp.grad = torch.randn(4, 3).to_sparse()
    with pytest.raises(ValueError, match="sparse"):
        clip([sp], 1.0)
    # parameters without a gradient are left out, and an empty list returns a zero: no library call, no GPU
    out = clip([torch.nn.Parameter(torch.randn(3))], 1.0)
    assert torch.is_tensor(out) and out.dim() == 0 and float(out) == 0.0 and out.dtype == torch.float32
    assert float(clip([], 1.0)) == 0.0


def test_grad_table_refusals_are_worded_per_property():
    from airpose_amd.optim import _grad_tables
    for g, exc, word in ((torch.randn(4, dtype=torch.float64), ValueError, "cpu"), (torch.randn(6, 4).t(), ValueError, "cpu"),
                         (3.0, TypeError, "tensors")):
        with pytest.raises(exc, match=word):
            _grad_tables([g], "clip_grad_norm_")

    class Fake(object):                                                       # a CUDA gradient's properties, without a GPU
        def __init__(self, **kw):
            self.is_sparse, self.layout, self.is_cuda, self.dtype, self.shape = False, torch.strided, True, torch.float32, (6, 4)
            self.device, self._contig = torch.device("cuda", 0), True
            self.__dict__.update(kw)

        def is_contiguous(self):
            return self._contig

        def stride(self):
            return (1, 6)

        def numel(self):
            return 24

        def data_ptr(self):
            return 0x1000
    real = torch.is_tensor
    torch.is_tensor = lambda x: isinstance(x, Fake) or real(x)
    try:
        with pytest.raises(TypeError, match="float16"):
            _grad_tables([Fake(dtype=torch.float16)], "clip_grad_norm_")
        with pytest.raises(ValueError, match="not contiguous"):
            _grad_tables([Fake(_contig=False)], "clip_grad_norm_")
        with pytest.raises(ValueError, match="more than one device"):
            _grad_tables([Fake(), Fake(device=torch.device("cuda", 1))], "clip_grad_norm_")
        dev, n, gtab, numel = _grad_tables([Fake(), Fake()], "clip_grad_norm_")
        assert n == 2 and list(numel) == [24, 24] and list(gtab) == [0x1000, 0x1000]
    finally:
        torch.is_tensor = real


class _Recorder(object):
    """stands in for the library: records the entry points a step calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("apg_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 8 * 64 if name.endswith("workspace_bytes") else 0
        return call


def test_fused_adam_options_are_attributes_and_the_defaults_build_the_same_call(monkeypatch):
    """No GPU: the parameters are CPU tensors smuggled past the constructor's device check, and the library is a recorder.  With the
    options at their defaults step() makes exactly one apg_adam_step call per group and nothing else; the options never show in
    param_groups, defaults or state_dict()."""
    from airpose_amd import _native_grad as G
    from airpose_amd import optim as O
    rec = _Recorder()
    monkeypatch.setattr(G, "lib", lambda: rec)
    monkeypatch.setattr(G, "stream", lambda dev: None)
    monkeypatch.setattr(O, "_check_param", lambda p: None)

    class _NoDevice(object):
        def __init__(self, dev):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False
    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    ps = [_with_grad(torch.randn(5)), _with_grad(torch.randn(2, 3))]
    plain = O.FusedAdam(ps, lr=1e-3, amsgrad=True)
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False and plain.grad_norm is None and plain.skipped_steps() == 0
    plain.step()
    assert [c[0] for c in rec.calls] == ["apg_adam_step"]
    name, args = rec.calls[0]
    assert len(args) == 14 and args[0] == 2 and list(args[6]) == [5, 6] and list(args[7]) == [1, 1] and args[8:13] == (1e-3, 0.9, 0.999, 1e-8, 0.0)
    torch_keys = torch.optim.Adam([torch.nn.Parameter(torch.randn(2))]).state_dict()["param_groups"][0].keys()
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(max_grad_norm=0.5, skip_nonfinite=True)):
        opt = O.FusedAdam([_with_grad(torch.randn(5))], amsgrad=True, **kw)
        assert opt.max_grad_norm == kw.get("max_grad_norm") and opt.skip_nonfinite == kw.get("skip_nonfinite", False)
        for d in (opt.defaults, opt.param_groups[0], opt.state_dict()["param_groups"][0]):
            assert "max_grad_norm" not in d and "skip_nonfinite" not in d
        assert opt.state_dict()["param_groups"][0].keys() == plain.state_dict()["param_groups"][0].keys() == torch_keys
    for bad, exc in ((-1.0, ValueError), (float("nan"), ValueError), (torch.tensor(1.0), TypeError), (True, TypeError)):
        with pytest.raises(exc, match="max_norm"):
            O.FusedAdam([_with_grad(torch.randn(5))], max_grad_norm=bad)
