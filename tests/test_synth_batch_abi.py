"""CPU checks of the synthetic-data batch entry points of libairpose_grad.so (airpose_amd/csrc/synth_batch.hip) without a GPU:
declared == exported == bound for apg_synth_*, the ABI number stays 2, every refusal happens on the host -- the device pointers below
are made-up addresses that are never dereferenced, the result is APG_EINVAL and the message starts with the entry's name and names the
argument -- and the restatement of synth_batch_util.py on its own: its Philox against Random123's known answers, its offsets (below
the range, uniform), its agreement with the pieces oracle/ already states, its mutants, and its bars against the host's own fp32
evaluation of the same chains (the floor), which a bar may exceed 16 times at the most."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import synth_batch_util as U
from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL = -1
FAKE = 0x7f0000001000                                        # 4096-aligned and never touched
IN_PTRS = ("index", "bb_in", "intr", "extr", "pose", "verts", "joints", "orient", "trans")
OUT_PTRS = ("crops", "crop_info", "status", "flip", "bb", "intr_out", "extr_out", "verts_rel", "joints_rel", "orient_rel", "trans_rel",
            "j2d", "j2d_crop", "pose_rotmat")
BATCH_INTS = ("n", "V", "J", "H", "W", "Hc", "Wc", "margin", "origin", "jitter", "shuffle")
CROPS_PTRS = ("frames", "crops", "flip", "im", "scale", "pad")


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _batch(**over):
    """apg_synth_batch on a valid argument set of made-up addresses; `over` replaces entries"""
    G, L = _lib()
    a = dict(n=5, V=67, J=22, H=120, W=160, Hc=96, Wc=128, margin=20, origin=0, jitter=1, shuffle=1, fx=1475.0, fy=1475.0, seed=3,
             epoch=1)
    a.update({n: FAKE + 0x100000 * (k + 1) for k, n in enumerate(IN_PTRS + OUT_PTRS)})
    a.update(over)
    vp = ctypes.c_void_p
    rc = L.apg_synth_batch(*[a[k] for k in BATCH_INTS], a["fx"], a["fy"], a["seed"], a["epoch"], *[vp(a[k]) for k in IN_PTRS + OUT_PTRS],
                           None)
    return rc, L.apg_last_error().decode()


def _crops(**over):
    G, L = _lib()
    a = dict(n=5, Hc=96, Wc=128, bgr=1)
    a.update({n: FAKE + 0x100000 * (k + 1) for k, n in enumerate(CROPS_PTRS)})
    a.update(over)
    rc = L.apg_synth_crops(a["n"], a["Hc"], a["Wc"], a["bgr"], *[ctypes.c_void_p(a[k]) for k in CROPS_PTRS], None)
    return rc, L.apg_last_error().decode()


BIG = (1 << 20) + 1
BATCH_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in IN_PTRS + OUT_PTRS] + \
                 [("misaligned_" + n, {n: FAKE + 0x900002}, n + " is not 4-byte aligned") for n in IN_PTRS + OUT_PTRS] + [
    ("n_zero", dict(n=0), "n must be in"), ("n_negative", dict(n=-1), "n must be in"), ("n_too_large", dict(n=65536), "n must be in"),
    ("V_zero", dict(V=0), "V must be in"), ("V_too_large", dict(V=(1 << 24) + 1), "V must be in"),
    ("J_zero", dict(J=0), "J must be in"), ("J_too_large", dict(J=(1 << 16) + 1), "J must be in"),
    ("H_zero", dict(H=0), "H must be in"), ("W_too_large", dict(W=BIG), "W must be in"),
    ("Hc_negative", dict(Hc=-4), "Hc must be in"), ("Wc_too_large", dict(Wc=BIG), "Wc must be in"),
    ("margin_negative", dict(margin=-1), "margin must be in"), ("margin_too_large", dict(margin=BIG), "margin must be in"),
    ("origin_other", dict(origin=2), "origin must be"), ("jitter_other", dict(jitter=2), "jitter must be 0 or 1"),
    ("shuffle_other", dict(shuffle=-1), "shuffle must be 0 or 1"), ("fx_nan", dict(fx=float("nan")), "fx and fy must be finite"),
    ("fy_inf", dict(fy=float("inf")), "fx and fy must be finite"),
    ("verts_rel_is_verts", dict(verts_rel=FAKE + 0x100000 * 6), "verts_rel must not be verts"),
    ("intr_out_is_intr", dict(intr_out=FAKE + 0x100000 * 3), "intr_out must not be intr")]
CROPS_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in CROPS_PTRS] + \
                 [("misaligned_" + n, {n: FAKE + 0x900002}, n + " is not 4-byte aligned") for n in CROPS_PTRS[1:]] + [
    ("n_zero", dict(n=0), "n must be in"), ("n_too_large", dict(n=65536), "n must be in"), ("Hc_zero", dict(Hc=0), "Hc must be in"),
    ("Wc_too_large", dict(Wc=BIG), "Wc must be in"), ("bgr_other", dict(bgr=2), "bgr must be 0 or 1"),
    ("im_is_frames", dict(im=FAKE + 0x100000), "im must not be frames")]


def test_header_exports_and_binding_agree():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_synth_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_synth_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_synth_"))
    assert declared == exported == bound == ["apg_synth_batch", "apg_synth_crops"]
    want = {"int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    for entry, count in (("apg_synth_batch", 39), ("apg_synth_crops", 11)):
        decl = re.search(r"int %s\((.*?)\);" % entry, src, flags=re.S)
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        res, args = G.SIGNATURES[entry]
        assert len(params) == len(args) == count and res is ctypes.c_int, entry
        for p, t in zip(params, args):                       # every parameter's C type against its ctypes type
            assert t is (ctypes.c_void_p if "*" in p else want[p.rsplit(" ", 1)[0]]), (entry, p)
    text = open(HEADER).read()
    for name, val in (("APG_SYNTH_ORIGIN_REGION", G.SYNTH_ORIGINS["region"]), ("APG_SYNTH_ORIGIN_FRAME", G.SYNTH_ORIGINS["frame"]),
                      ("APG_SYNTH_CLAMPED", G.SYNTH_CLAMPED), ("APG_SYNTH_WIDENED", G.SYNTH_WIDENED), ("APG_SYNTH_OUTSIDE", G.SYNTH_OUTSIDE),
                      ("APG_SYNTH_THREADS", G.SYNTH_THREADS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == val, name
    assert (G.SYNTH_CLAMPED, G.SYNTH_WIDENED, G.SYNTH_OUTSIDE) == (U.CLAMPED, U.WIDENED, U.OUTSIDE) and G.SYNTH_ORIGINS == U.ORIGINS
    # the shapes of the GPU test lie below and above a workgroup of the sample kernel (J) and of the vertex kernel (V), off its multiples
    assert min(U.JS) < G.SYNTH_THREADS < max(U.JS) + 2 and max(U.JS) % G.SYNTH_THREADS and min(U.VS) < 256 < max(U.VS) and max(U.VS) % 256


def test_the_inference_library_gains_no_symbol():
    from airpose_amd import _native
    syms = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "synth" not in syms and not any(n.startswith("apg_") for n in _native.SIGNATURES)


def test_header_documents_the_contract():
    text = open(HEADER).read()
    at = text.index("Synthetic-data batches (synth_batch.hip)")
    doc = text[at:text.index("#define APG_SYNTH_ORIGIN_REGION", at)]
    for phrase in ("Additive under ABI 2", "Philox4x32-10", "mulhi32(word, r)", "ymin side, ymax side, xmin side, xmax side",
                   "bit 31 of word 0", "the region, as in the reference, NOT the crop", "0 <= y0' < y1' <= Hc and 0 <= x0' < x1' <= Wc",
                   "for ANY bb_in", "identity wherever the", "camera flip[i] ^ s", "((R0 x + R1 y) + R2 z) + t", "no pad offset",
                   "ap_preprocess_crops", "bit-equal", "preprocess_px.inc", "bit-identical from run to run", "read once"):
        assert phrase in doc, phrase


def test_abi_number_stays():
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2


@pytest.mark.parametrize("over,names", [r[1:] for r in BATCH_REFUSALS], ids=[r[0] for r in BATCH_REFUSALS])
def test_batch_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _batch(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_synth_batch: ") and names in msg[len("apg_synth_batch: "):], msg


@pytest.mark.parametrize("over,names", [r[1:] for r in CROPS_REFUSALS], ids=[r[0] for r in CROPS_REFUSALS])
def test_crops_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _crops(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_synth_crops: ") and names in msg[len("apg_synth_crops: "):], msg


# ------------------------------------------------------------------------------------------------ the restatement, on the CPU
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    ones = 0xffffffff
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                           ((ones,) * 4, (ones, ones), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % w for w in U.philox(ctr, key)) == want
    many = U.philox((np.arange(3), 0, 0, 0), (0, 0))         # vectorised over the counter
    assert many.shape == (3, 4) and " ".join("%08x" % w for w in many[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert not np.array_equal(many[1], many[2])


def test_offsets_are_below_the_range_and_uniform():
    n, r = 100000, 7
    words = U.draws(U.SEED, 0, np.arange(n), 0).astype(np.uint64)
    for rr in (1, 2, r, 199, 200, 1 << 20):
        off = (words * np.uint64(rr)) >> np.uint64(32)
        assert int(off.max()) < rr and int(U.offset(0xffffffff, rr)) == rr - 1 and U.offset(0, rr) == 0
    assert U.offset(0xdeadbeef, 0) == 0 and U.offset(0xffffffff, 1) == 0
    sigma = (n * (1 / r) * (1 - 1 / r)) ** 0.5
    for k in range(4):                                       # each of the four words, over 1e5 dataset indices
        counts = np.bincount(((words[:, k] * np.uint64(r)) >> np.uint64(32)).astype(np.int64), minlength=r)
        assert counts.shape == (r,) and np.abs(counts - n / r).max() < 5 * sigma, (k, counts)
    flips = U.draws(U.SEED, 0, np.arange(n), 2)[:, 0] >> 31
    assert abs(int(flips.sum()) - n / 2) < 5 * (n / 4) ** 0.5
    # another epoch, seed or camera is another stream
    for other in (U.draws(U.SEED, 1, np.arange(n), 0), U.draws(U.SEED + 1, 0, np.arange(n), 0), U.draws(U.SEED, 0, np.arange(n), 1),
                  U.draws(U.SEED + (1 << 32), 0, np.arange(n), 0)):
        assert (other[:, 0] == words[:, 0]).mean() < 1e-3


@pytest.mark.parametrize("origin", ["region", "frame"])
def test_inputs_tell_the_mutants_apart(origin):
    """every mutant moves an output of the restatement on the planted records (the GPU test asks the same of the kernel's output),
    the equivalent one moves none, and the planted boxes are what they claim to be"""
    rec, index = U.case(5, 67, 22)
    ref = U.ref_batch(rec, index, origin=origin)
    assert U.differs(ref, ref) == []
    for m in U.MUTATIONS:
        assert U.differs(ref, U.ref_batch(rec, index, origin=origin, mut=m)), m
    for m in U.EQUIVALENT:                                   # (synth_batch_util's docstring: why this one cannot differ)
        assert U.differs(ref, U.ref_batch(rec, index, origin=origin, mut=m)) == [], m
    flip = ref["flip"]
    assert set(flip.tolist()) == {0, 1}                      # both orders occur among the five samples
    crops, info, status = (U.by_camera(ref[k], flip) for k in ("crops", "crop_info", "status"))
    at = lambda a, b: a[b[1], b[0]]                          # planted (sample, camera) -> row
    base = lambda b: at(info, b)[0] if origin == "region" else np.zeros(2, np.int32)
    assert at(info, U.B_TOP_LEFT).tolist() == [[0, 0], [50, 60]] and at(crops, U.B_TOP_LEFT)[[0, 2]].tolist() == [0, 0]
    assert at(info, U.B_BOTTOM_RIGHT).tolist() == [[U.H - 50, U.W - 60], [U.H, U.W]]
    assert (at(crops, U.B_BOTTOM_RIGHT)[[1, 3]] + base(U.B_BOTTOM_RIGHT)).tolist() == [U.H, U.W]         # range 0 -> offset 0
    assert at(crops, U.B_RANGE1_LOW)[[0, 2]].tolist() == [0, 0] and at(info, U.B_RANGE1_LOW)[0].tolist() == [0, 0]  # range 1 -> offset 0
    assert (at(crops, U.B_RANGE1_HIGH)[[1, 3]] + base(U.B_RANGE1_HIGH)).tolist() == [U.H, U.W]
    assert at(info, U.B_EXACT).tolist() == [[0, 60], [80, U.W]] and at(info, U.B_ONE_OFF).tolist() == [[1, 60], [81, U.W - 1]]
    y0, y1, x0, x1 = at(crops, U.B_DEGENERATE) + np.repeat(base(U.B_DEGENERATE), 2)
    assert y0 < 50 < y1 and x0 < 70 < x1 and at(status, U.B_DEGENERATE) == 0
    want = np.zeros_like(status)
    if origin == "region":
        want[U.B_FULL[1], U.B_FULL[0]] = U.OUTSIDE           # the whole frame does not fit the canvas
    assert np.array_equal(status, want)
    jit = U.ref_batch(rec, index, origin=origin, jitter=False)
    jc, ji = U.by_camera(jit["crops"], jit["flip"]), U.by_camera(jit["crop_info"], jit["flip"])
    region = np.stack([ji[..., 0, 0], ji[..., 1, 0], ji[..., 0, 1], ji[..., 1, 1]], -1)                # ymin, ymax, xmin, xmax
    moved = jc + (region[..., [0, 0, 2, 2]] if origin == "region" else 0)
    assert np.array_equal(moved[status == 0], region[status == 0])                                      # no jitter: the crop is the region
    assert not U.ref_batch(rec, index, origin=origin, shuffle=False)["flip"].any()


@pytest.mark.parametrize("margin", [20, 0])
@pytest.mark.parametrize("origin", ["region", "frame"])
def test_hostile_boxes_keep_the_invariant_in_the_restatement(origin, margin):
    rec, index = U.hostile()
    ref = U.ref_batch(rec, index, origin=origin, margin=margin, boxes_only=True)
    Hc, Wc = (U.HC, U.WC) if origin == "region" else (U.H, U.W)
    y0, y1, x0, x1 = ref["crops"].reshape(-1, 4).T.astype(np.int64)
    assert (0 <= y0).all() and (y0 < y1).all() and (y1 <= Hc).all() and (0 <= x0).all() and (x0 < x1).all() and (x1 <= Wc).all()
    seen = np.bitwise_or.reduce(ref["status"].ravel())
    assert seen & U.CLAMPED and seen & U.WIDENED and (origin == "frame" or seen & U.OUTSIDE)


def test_restatement_agrees_with_the_oracle_s_pieces():
    for n, V, J in ((1, 1, 22), (5, 67, 127)):
        rec, index = U.case(n, V, J)
        ref, orc = U.ref_batch(rec, index), U.oracle_pieces(rec)
        for k in ("verts_rel", "joints_rel", "j2d"):
            assert np.abs(U.by_camera(ref[k], ref["flip"]) - orc[k]).max() < 1e-9, k        # (j2d is about 1e3 pixels)
        assert np.abs(ref["pose_rotmat"] - orc["pose_rotmat"]).max() < 1e-14
        assert (U.by_camera(ref["joints_rel"], ref["flip"])[..., 2] >= 2).all()


@pytest.mark.parametrize("n", U.NS)
@pytest.mark.parametrize("J", U.JS)
def test_the_bars_hold_the_host_s_fp32_evaluation_and_are_not_loose(n, J):
    """the same chains in numpy fp32 (one rounding per operation) must pass every bar, and no bar may exceed 16 times that floor"""
    rec, index = U.case(n, 67, J)
    ref, r32 = U.ref_batch(rec, index), U.ref_batch(rec, index, dtype=np.float32)
    for k in U.INT_KEYS:
        assert np.array_equal(r32[k], ref[k]), k
    for chain, err, bar in U.chain_checks(rec, r32, ref):
        w = U.worst(err, bar)
        print("n = %d, J = %d, %s: the fp32 evaluation's worst error / bar %.3f" % (n, J, chain, w))
        assert 1 / 16 <= w <= 1, chain
