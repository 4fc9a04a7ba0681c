"""CPU checks of the real-data batch entry point of libairpose_grad.so (airpose_amd/csrc/seq_batch.hip) and of
airpose_amd.RealSequenceBatches without a GPU: declared == exported == bound, the ABI number stays 2, every refusal happens on the host
-- the device pointers below are made-up addresses that are never dereferenced, the result is APG_EINVAL and the message starts with
the entry's name and names the argument -- the class is exported and refuses by name, and the restatement's mutants on the CPU.

The entry point is apg_real_batch, not apg_seq_batch: tests/test_seq_abi.py pins the set of apg_seq_* names to the two of seq_fit.hip
(declared == exported == bound == [apg_seq_export, apg_seq_init]), and existing tests stay as they are.

The constructor takes the detections, which must be a CUDA tensor, so no object can be made on a machine without a GPU; what is
checked here is that a device with an index gets as far as the arguments without touching the GPU (the refusal is the argument's, by
name, never a CUDA initialisation error)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import real_batch_util as U
from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL = -1
FAKE = 0x7f0000001000                                    # 4096-aligned and never touched
ENTRY = "apg_real_batch"
DEV_PTRS = ("det", "j2d", "crops", "crop_info", "bb", "j2d_crop", "status")


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _call(**over):
    """a valid argument set on made-up addresses; `over` replaces entries"""
    G, L = _lib()
    a = dict(L=9, a=2, n=5, agreement_px=100.0, border=50, principal=[960.0, 540.0, 955.5, 541.25], size=[1080, 1920, 1080, 1920])
    a.update({n: FAKE + 0x100000 * (k + 1) for k, n in enumerate(DEV_PTRS)})
    a.update(over)
    vp = ctypes.c_void_p
    pr = None if a["principal"] is None else (ctypes.c_float * 4)(*a["principal"])
    sz = None if a["size"] is None else (ctypes.c_int * 4)(*a["size"])
    rc = L.apg_real_batch(a["L"], a["a"], a["n"], vp(a["det"]), pr, sz, a["agreement_px"], a["border"],
                          *[vp(a[n]) for n in DEV_PTRS[1:]], None)
    return rc, L.apg_last_error().decode()


REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in DEV_PTRS + ("principal", "size")] + \
           [("misaligned_" + n, {n: FAKE + 0x900002}, n + " is not 4-byte aligned") for n in DEV_PTRS] + [
    ("L_zero", dict(L=0), "L must be"), ("L_too_long", dict(L=(1 << 22) + 1), "L must be"),
    ("n_zero", dict(n=0), "n must be at least 1"), ("n_negative", dict(n=-3), "n must be at least 1"),
    ("a_negative", dict(a=-1), "a must not be negative"), ("past_the_end", dict(a=5, n=5), "a + n must not exceed L"),
    ("n_beyond_L", dict(a=0, n=10), "a + n must not exceed L"), ("a_plus_n_overflows", dict(a=2 ** 31 - 1, n=5), "a + n must not exceed L"),
    ("height_zero", dict(size=[0, 1920, 1080, 1920]), "size of view 0"), ("width_negative", dict(size=[1080, 1920, 1080, -1]), "size of view 1"),
    ("width_too_large", dict(size=[1080, (1 << 20) + 1, 1080, 1920]), "size of view 0"),
    ("cx_zero", dict(principal=[0.0, 540.0, 960.0, 540.0]), "principal point of view 0"),
    ("cy_negative", dict(principal=[960.0, 540.0, 960.0, -540.0]), "principal point of view 1"),
    ("cx_nan", dict(principal=[float("nan"), 540.0, 960.0, 540.0]), "principal point of view 0"),
    ("cy_inf", dict(principal=[960.0, float("inf"), 960.0, 540.0]), "principal point of view 0"),
    ("border_negative", dict(border=-1), "border"), ("border_too_large", dict(border=(1 << 20) + 1), "border"),
    ("agreement_negative", dict(agreement_px=-1.0), "agreement_px"), ("agreement_nan", dict(agreement_px=float("nan")), "agreement_px"),
    ("agreement_inf", dict(agreement_px=float("inf")), "agreement_px"), ("j2d_is_det", dict(j2d=FAKE + 0x100000), "j2d must not be det")]


def test_header_exports_and_binding_agree():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int %s\((.*?)\);" % ENTRY, src, flags=re.S)
    assert decl is not None
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\s[TW]\s+%s$" % ENTRY, syms, flags=re.M)
    res, args = G.SIGNATURES[ENTRY]
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(args) == 15 and res is ctypes.c_int
    want = {"int": ctypes.c_int, "float": ctypes.c_float, "const float* principal": ctypes.POINTER(ctypes.c_float),
            "const int* size": ctypes.POINTER(ctypes.c_int)}
    for p, t in zip(params, args):                           # every parameter's C type against its ctypes type
        if p in want:
            assert t is want[p], p
        elif "*" in p:
            assert t is ctypes.c_void_p, p
        else:
            assert t is want[p.rsplit(" ", 1)[0]], p
    text = open(HEADER).read()
    for name, val in (("APG_BATCH_WAVES", G.BATCH_WAVES), ("APG_BATCH_FALLBACK", G.BATCH_FALLBACK), ("APG_BATCH_CLAMPED", G.BATCH_CLAMPED),
                      ("APG_BATCH_WIDENED", G.BATCH_WIDENED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == val, name
    assert (G.BATCH_FALLBACK, G.BATCH_CLAMPED, G.BATCH_WIDENED) == (U.FALLBACK, U.CLAMPED, U.WIDENED)
    # the spans of the GPU test lie below, at and across the waves of a workgroup
    assert sorted({(2 * n > G.BATCH_WAVES) - (2 * n < G.BATCH_WAVES) for _, n in U.SPANS}) == [-1, 1] and any(2 * n % G.BATCH_WAVES for _, n in U.SPANS)


def test_header_documents_the_contract():
    text = open(HEADER).read()
    at = text.index("Real-data batches (seq_batch.hip)")
    doc = text[at:text.index("#define APG_BATCH_WAVES", at)]
    for phrase in ("BOTH detectors", "(strict)", "towards zero", "{0} on both axes", "ap_preprocess_crops", "bit-equal",
                   "0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H", "treated as absent", "clamped", "one pixel", "Additive under ABI 2",
                   "no pad offset", "HOST"):
        assert phrase in doc, phrase


def test_abi_number_stays():
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2


@pytest.mark.parametrize("over,names", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _call(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith(ENTRY + ": ") and names in msg[len(ENTRY) + 2:], msg


# ------------------------------------------------------------------------------------------------ the Python class, no GPU
def test_class_is_exported_and_reaches_its_arguments_without_a_gpu():
    import airpose_amd
    from airpose_amd import real_batches
    assert airpose_amd.RealSequenceBatches is real_batches.RealSequenceBatches
    R = airpose_amd.RealSequenceBatches
    det, intr = torch.zeros(2, 5, 2, 24, 3), torch.eye(3).repeat(2, 1, 1)
    for device in ("cuda:0", torch.device("cuda", 0), None, "cuda"):
        with pytest.raises(RuntimeError, match="detections lives on cpu; it must be a CUDA .* there is no CPU path"):
            R(det, intr, device=device)
    with pytest.raises(RuntimeError, match="device must be a CUDA .* there is no CPU path"):
        R(det, intr, device="cpu")
    # type and shape come before the device, so these are reachable here
    with pytest.raises(RuntimeError, match=r"detections must be \(2, L, 2, 24, 3\), got \(2, 5, 2, 25, 3\)"):
        R(torch.zeros(2, 5, 2, 25, 3), intr, device="cuda:0")
    with pytest.raises(RuntimeError, match=r"detections must be \(2, L, 2, 24, 3\), got \(2, 0, 2, 24, 3\)"):
        R(torch.zeros(2, 0, 2, 24, 3), intr, device="cuda:0")
    with pytest.raises(RuntimeError, match=r"intr must be \(2, 3, 3\), got \(2, 4\)"):
        R(det, torch.zeros(2, 4), device="cuda:0")
    with pytest.raises(RuntimeError, match="detections must be a floating-point tensor, got torch.int64"):
        R(det.long(), intr, device="cuda:0")
    with pytest.raises(RuntimeError, match="detections must be float32 .* got torch.float64"):
        R(det.double(), intr, device="cuda:0")
    with pytest.raises(RuntimeError, match="intr must be a tensor, got list"):
        R(det, [[1.0]], device="cuda:0")
    with pytest.raises(ValueError, match="first_cam must be 0 or 1, got 2"):
        R(det, intr, device="cuda:0", first_cam=2)
    with pytest.raises(ValueError, match="border must be"):
        R(det, intr, device="cuda:0", border=-1)
    with pytest.raises(ValueError, match="border must be"):
        R(det, intr, device="cuda:0", border=12.5)
    with pytest.raises(ValueError, match="agreement_px must be"):
        R(det, intr, device="cuda:0", agreement_px=float("nan"))


def test_batch_refuses_frames_by_name():
    """batch()'s own checks, on an object whose constructor is bypassed (it needs a CUDA tensor): types and shapes first, then devices"""
    from airpose_amd.real_batches import RealSequenceBatches as R
    r = R.__new__(R)
    r.device, r.L = torch.device("cuda", 0), 5
    f0, f1 = torch.zeros(2, 12, 16, 3, dtype=torch.uint8), torch.zeros(2, 9, 20, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="frames1 must be a tensor, got NoneType"):
        r.batch(f0, None, 0)
    with pytest.raises(RuntimeError, match="frames0 must be uint8, got torch.float32"):
        r.batch(f0.float(), f1, 0)
    with pytest.raises(RuntimeError, match=r"frames1 must be \(n, H, W, 3\), got \(2, 9, 20, 4\)"):
        r.batch(f0, torch.zeros(2, 9, 20, 4, dtype=torch.uint8), 0)
    with pytest.raises(RuntimeError, match=r"frames0 must be \(n, H, W, 3\), got \(12, 16, 3\)"):
        r.batch(f0[0], f1, 0)
    with pytest.raises(RuntimeError, match="the same number of frames, got 2 and 1"):
        r.batch(f0, f1[:1], 0)
    with pytest.raises(RuntimeError, match="must lie in the sequence's 5 frames, got start = 4, n = 2"):
        r.batch(f0, f1, 4)
    with pytest.raises(RuntimeError, match="start = -1"):
        r.batch(f0, f1, -1)
    with pytest.raises(RuntimeError, match="frames0 lives on cpu; it must be a CUDA .* there is no CPU path"):
        r.batch(f0, f1, 0)
    with pytest.raises(ValueError, match="batch_size must be a positive integer, got 0"):
        r.predict(None, lambda a, b: None, batch_size=0)
    with pytest.raises(TypeError, match="frame_source must be callable"):
        r.predict(None, None)


# ------------------------------------------------------------------------------------------------ the restatement, on the CPU
@pytest.mark.parametrize("border", U.BORDERS)
def test_inputs_tell_the_mutants_apart(border):
    """every mutant moves an output of the restatement on the planted inputs (the GPU test asks the same of the kernel's output), the
    equivalent one moves none, and the planted cases are what they claim to be"""
    det = U.case(border)
    ref = U.ref_batch(det, 0, U.L, border)
    assert U.differs(ref, ref) == []
    for m in U.MUTATIONS:
        assert U.differs(ref, U.ref_batch(det, 0, U.L, border, mut=m)), m
    for m in U.EQUIVALENT:
        assert U.differs(ref, U.ref_batch(det, 0, U.L, border, mut=m)) == [], m
    conf = ref["j2d"][..., 2]
    assert (conf[:, U.F_GENERIC, :, U.J_EXACT] == 0.5).all() and (conf[:, U.F_GENERIC, :, U.J_BEYOND] == 0).all()
    assert (ref["status"][:, [U.F_ZERO_CONF, U.F_ALPHA_ONLY]] == U.FALLBACK).all() and (np.delete(ref["status"], [U.F_ZERO_CONF, U.F_ALPHA_ONLY], 1) == 0).all()
    assert (conf[:, U.F_ALPHA_ONLY, 1] != 0).any() and (ref["crops"][:, U.F_ALPHA_ONLY] == [0, border, 0, border]).all()
    for v, (H, W) in enumerate(U.SIZES):
        assert ref["crops"][v, U.F_EDGES].tolist() == [0, H, 0, W]
        assert ref["crops"][v, U.F_TRUNC, [0, 2]].tolist() == [0, 0] and ref["crops"][v, U.F_NEGATIVE, [0, 2]].tolist() == [0, 0]
        assert ref["crops"][v, U.F_TRUNC, 3] == 2 * border + 8                          # int(2 border + 8.625)
