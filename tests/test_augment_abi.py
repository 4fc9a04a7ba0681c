"""CPU checks of the crop augmentation (airpose_amd/csrc/augment.hip, airpose_amd/augment.py) without a GPU: declared == exported ==
bound for apg_augment_*, the ABI number stays 2, every refusal of the two entries happens on the host -- the device pointers below are
made-up addresses that are never dereferenced -- and names its argument, no kernel of the new source holds packed fp32 math, the
oracle and the restatement of augment_util.py hold on their own, and CropAugment refuses its arguments by name."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import augment_util as U
from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL = -1
FAKE = 0x7f0000001000                                        # 4096-aligned and never touched
DRAW_PTRS = ("index", "cam", "blur_taps", "color", "gamma", "noise_sigma", "rects", "rect_rgb", "status")
CROPS_PTRS = ("index", "cam", "im", "crops", "blur_taps", "color", "gamma", "noise_sigma", "rects", "rect_rgb", "out", "status")
CFG = [0.5, 0.0, 2.0, 30 / 255, 35.0, 0.6, 1.4, 0.8, 1.2, 0.5, 2.0, 0.0, 1.0, 0.0, 0.03, 2.0, 0.1, 0.4]
IMAGE_BYTES = 2 * 5 * 3 * 224 * 224 * 4                      # of the n = 5 below


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _draw(cfg=None, **over):
    G, L = _lib()
    a = dict(n=5, seed=3, epoch=1, cam_all=0)
    a.update({n: FAKE + 0x10000000 * (k + 1) for k, n in enumerate(DRAW_PTRS)})
    a.update(over)
    vp = ctypes.c_void_p
    c = None if cfg == "null" else (ctypes.c_float * G.AUG_CFG)(*(cfg or CFG))
    rc = L.apg_augment_draw(a["n"], a["seed"], a["epoch"], vp(a["index"]), vp(a["cam"]), a["cam_all"], c, *[vp(a[k]) for k in DRAW_PTRS[2:]], None)
    return rc, L.apg_last_error().decode()


def _crops(**over):
    G, L = _lib()
    a = dict(n=5, seed=3, epoch=1, cam_all=0)
    a.update({n: FAKE + 0x10000000 * (k + 1) for k, n in enumerate(CROPS_PTRS)})
    a.update(over)
    vp = ctypes.c_void_p
    rc = L.apg_augment_crops(a["n"], a["seed"], a["epoch"], vp(a["index"]), vp(a["cam"]), a["cam_all"], *[vp(a[k]) for k in CROPS_PTRS[2:]], None)
    return rc, L.apg_last_error().decode()


def _cfg(k, v):
    c = list(CFG)
    c[k] = v
    return c


IM = FAKE + 0x10000000 * 3                                   # CROPS_PTRS' made-up im
DRAW_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in DRAW_PTRS if n != "cam"] + \
                [("misaligned_" + n, {n: FAKE + 0x900002}, n + " is not 4-byte aligned") for n in DRAW_PTRS] + [
    ("n_zero", dict(n=0), "n must be in 1 .. 65535"), ("n_negative", dict(n=-1), "n must be in"), ("n_too_large", dict(n=65536), "n must be in"),
    ("cam_all_other", dict(cam_all=2), "cam_all must be 0 or 1"), ("cfg_null", dict(cfg="null"), "cfg is NULL"),
    ("cfg_nan", dict(cfg=_cfg(4, float("nan"))), "cfg[4] must be finite"), ("cfg_inf", dict(cfg=_cfg(14, float("inf"))), "cfg[14] must be finite"),
    ("p_above_one", dict(cfg=_cfg(0, 1.5)), "cfg[0] (p) must be in 0 .. 1"), ("occluders_five", dict(cfg=_cfg(15, 5.0)), "cfg[15] (occluders)"),
    ("occluders_fraction", dict(cfg=_cfg(15, 1.5)), "cfg[15] (occluders)"), ("side_above_one", dict(cfg=_cfg(17, 1.25)), "cfg[16], cfg[17] (occluder side)")]
CROPS_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in CROPS_PTRS if n != "cam"] + \
                 [("misaligned_" + n, {n: FAKE + 0x900002}, n + " is not 4-byte aligned") for n in CROPS_PTRS] + [
    ("n_zero", dict(n=0), "n must be in 1 .. 65535"), ("n_too_large", dict(n=65536), "n must be in"),
    ("cam_all_other", dict(cam_all=-1), "cam_all must be 0 or 1"),
    ("out_is_im", dict(out=IM), "out must not overlap im"),
    ("out_starts_inside_im", dict(out=IM + IMAGE_BYTES - 16), "out must not overlap im"),
    ("out_ends_inside_im", dict(out=IM - IMAGE_BYTES + 16), "out must not overlap im")]


def test_header_exports_and_binding_agree():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_augment_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_augment_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_augment_"))
    assert declared == exported == bound == ["apg_augment_crops", "apg_augment_draw"]
    want = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64}
    for entry, count in (("apg_augment_draw", 15), ("apg_augment_crops", 17)):
        decl = re.search(r"int %s\((.*?)\);" % entry, src, flags=re.S)
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        res, args = G.SIGNATURES[entry]
        assert len(params) == len(args) == count and res is ctypes.c_int, entry
        for p, t in zip(params, args):                       # every parameter's C type against its ctypes type; cfg is a HOST array
            assert t is (ctypes.POINTER(ctypes.c_float) if p.endswith("* cfg") else ctypes.c_void_p if "*" in p else want[p.rsplit(" ", 1)[0]]), (entry, p)
    text = open(HEADER).read()
    for name, val in (("APG_AUG_TILE", G.AUG_TILE), ("APG_AUG_THREADS", G.AUG_THREADS), ("APG_AUG_MAX_RADIUS", G.AUG_MAX_RADIUS),
                      ("APG_AUG_MAX_RECTS", G.AUG_MAX_RECTS), ("APG_AUG_CFG", G.AUG_CFG), ("APG_AUG_BLUR_CLAMPED", G.AUG_BLUR_CLAMPED),
                      ("APG_AUG_NONFINITE", G.AUG_NONFINITE), ("APG_AUG_RECT_CLIPPED", G.AUG_RECT_CLIPPED), ("APG_AUG_BAD_BOX", G.AUG_BAD_BOX)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == val, name
    assert (G.AUG_MAX_RADIUS, G.AUG_MAX_RECTS, G.AUG_CFG) == (U.RMAX, U.NRECT, U.NCFG)
    assert (G.AUG_BLUR_CLAMPED, G.AUG_NONFINITE, G.AUG_RECT_CLIPPED, G.AUG_BAD_BOX) == (U.BLUR_CLAMPED, U.NONFINITE, U.RECT_CLIPPED, U.BAD_BOX)


def test_abi_number_stays_and_the_inference_library_gains_no_symbol():
    from airpose_amd import _native
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2
    syms = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "augment" not in syms and not any(n.startswith("apg_") for n in _native.SIGNATURES)


def test_header_documents_the_contract():
    text = open(HEADER).read()
    at = text.index("Crop augmentation (augment.hip)")
    doc = text[at:text.index("#define APG_AUG_TILE", at)]
    for phrase in ("Additive under ABI 2", "UNPINNED", "Philox4x32-10", "copied bit for bit", "clamped to the content rectangle", "preprocess_px.inc",
                   "0x80000000", "k >= 1", "(word >> 8) * 2^-24", "rounded once", "out must not overlap im", "APG_AUG_NONFINITE",
                   "APG_AUG_RECT_CLIPPED", "APG_AUG_BLUR_CLAMPED", "a later one covers an earlier one", "no fused multiply-add"):
        assert phrase in doc, phrase


@pytest.mark.parametrize("over,names", [r[1:] for r in DRAW_REFUSALS], ids=[r[0] for r in DRAW_REFUSALS])
def test_draw_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _draw(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_augment_draw: ") and names in msg[len("apg_augment_draw: "):], msg


@pytest.mark.parametrize("over,names", [r[1:] for r in CROPS_REFUSALS], ids=[r[0] for r in CROPS_REFUSALS])
def test_crops_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _crops(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_augment_crops: ") and names in msg[len("apg_augment_crops: "):], msg


def test_the_source_is_one_of_grad_srcs_and_the_committed_scan_lists_its_kernels():
    """augment.hip is a source like the others: tests/test_packed_math_scan.py holds the committed rows below to the live scan, and
    the source, one of its GUARDED, to "no packed fp32 math with the flag, some without it" """
    text = open(os.path.join(REPO, "airpose_amd", "csrc", "Makefile")).read()
    grad = re.search(r"^GRAD_SRCS\s*=\s*(.*)$", text, re.M).group(1).split()
    assert "augment.hip" in grad and "AUG_SRCS" not in text
    with open(os.path.join(REPO, "tests", "packed_math_scan.json")) as f:
        d = json.load(f)
    rows = [dict(zip(d["columns"], r)) for r in d["kernels"] if r[0] == "augment.hip"]
    assert sorted(r["kernel"] for r in rows) == ["augment_crops_kernel", "augment_draw_kernel"]
    for r in rows:
        assert r["flags"] == "-ffp-contract=off -fno-slp-vectorize" and r["packed"] == 0 and r["op_sel"] == 0, r
    assert max(r["ds_reads"] for r in rows) > 0              # (the scan did read the tile kernel's body)
    import test_packed_math_scan                             # (beside this file, as augment_util is)
    assert "augment" in test_packed_math_scan.GUARDED


# ------------------------------------------------------------------------------------------------ the oracle, on the CPU
def _small():
    x = U.planted_images()
    return x, U.BOXES, U.planted_params()


def test_neutral_parameters_give_an_identical_array():
    x, boxes, _ = _small()
    P = U.neutral(3)
    for s in (0, 1):
        for i in range(3):
            for T in (np.float32, np.float64):
                r = U.chain(x[s, i], boxes[s, i], U.image_params(P, s, i), dtype=T)
                assert r["copied"] and r["out"].dtype == np.float32 and np.array_equal(r["out"].view(np.uint32), x[s, i].view(np.uint32))
    # the empty content is a copy whatever the parameters
    r = U.chain(x[1, 1], U.BOX_EMPTY, U.image_params(U.planted_params(), 1, 1), dtype=np.float32)
    assert r["copied"] and r["rect"] == (0, 0, 0, 0)
    assert U.content_rect(U.BOX_WIDE) == (75, 149, 0, 224) and U.content_rect(U.BOX_TALL) == (0, 224, 78, 145)
    assert U.content_rect(U.BOX_SQUARE) == (0, 224, 0, 224) and U.content_rect(U.BOX_ONE_ROW) == (111, 112, 0, 224)
    assert U.content_rect(U.BOX_NARROW) == (0, 224, 110, 113) and U.content_rect((5, 5, 0, 9)) == (0, 0, 0, 0)


def test_colour_matrix_identities():
    ulp1 = 2.0 ** -23
    full = U.compose(theta=2 * np.pi).astype(np.float32)     # a hue of 360 degrees: the identity to 1 ulp of fp32
    assert np.abs(full.astype(np.float64) - np.eye(3)).max() <= ulp1
    deg = U.compose(theta=float(np.float32(360.0)) * (3.141592653589793 / 180.0)).astype(np.float32)
    assert np.abs(deg.astype(np.float64) - np.eye(3)).max() <= ulp1
    assert np.array_equal(U.compose(sat=0.0), U.compose(gray=1.0))                         # saturation 0 == grayscale 1
    assert np.allclose(U.compose(sat=0.0), np.tile(U.LUMA, (3, 1)), atol=1e-16)
    assert np.array_equal(U.compose(), np.eye(3)) and np.array_equal(U.compose(sat=1.0), np.eye(3)) and np.array_equal(U.compose(gray=0.0), np.eye(3))
    grey = U.compose(theta=1.0) @ np.ones(3)                 # a hue rotation keeps the greys
    assert np.abs(grey - 1).max() < 4e-3                     # (K is given to three decimals: its rows sum to 0.003 at most)
    h = U.hue_matrix(0.7)
    assert np.abs(U.LUMA @ h - U.LUMA).max() < 4e-3          # ... and the luma


def test_taps_are_normalised_and_their_radius_is_capped():
    for sigma in (0.05, 0.3, 0.34, 1.0, 1.7, 2.0, 2.5, 40.0):
        w, clamped = U.gauss_taps(sigma)
        total = float(w[0]) + 2.0 * float(w[1:].astype(np.float64).sum())
        assert abs(total - 1) <= 2.0 ** -23, (sigma, total)
        assert U.radius(w) <= min(int(np.ceil(3 * sigma)), 6) and clamped == (3 * sigma > 6) and (np.diff(w[:U.radius(w) + 1]) <= 0).all()
    assert U.gauss_taps(0.0)[0].tolist() == [1, 0, 0, 0, 0, 0, 0] and U.radius(U.gauss_taps(2.0)[0]) == 6


def _aug(**kw):
    from airpose_amd import CropAugment
    return CropAugment(device="cuda:0", **kw)                # (a given index constructs without a GPU)


def test_draws_lie_in_their_ranges_and_depend_on_their_key_alone():
    a = _aug(seed=U.SEED, occluders=4)
    cfg = list(a._cfg)
    n = 400
    index = np.arange(1000, 1000 + n)
    P = U.draw(U.SEED, 3, index, np.zeros(n, np.int32), cfg)
    rad = np.asarray([U.radius(w) for w in P["blur_taps"].reshape(-1, 7)])
    assert set(rad) <= set(range(7)) and rad.max() == 6 and (rad == 0).mean() > 0.3 and not P["status"].any()
    assert (np.abs(P["blur_taps"][..., 0].astype(np.float64) + 2 * P["blur_taps"][..., 1:].astype(np.float64).sum(-1) - 1) <= 2.0 ** -23).all()
    b = P["color"][..., 3]
    assert (np.abs(b) <= np.float32(30 / 255)).all() and (b[..., 0] == b[..., 1]).all() and (b != 0).mean() > 0.3
    g = P["gamma"]
    assert ((g >= 0.5) & (g <= 2.0)).all() and 0.3 < (g[..., 0] != 1).mean() < 0.7
    assert ((P["noise_sigma"] >= 0) & (P["noise_sigma"] <= np.float32(0.03))).all()
    assert ((P["rect_rgb"] >= 0) & (P["rect_rgb"] < 1)).all()
    r = P["rects"].reshape(-1, 4)
    side = np.stack([r[:, 1] - r[:, 0], r[:, 3] - r[:, 2]], 1)
    live = side[:, 0] > 0
    assert 0.3 < live.mean() < 0.7 and (side[live] >= int(0.1 * 224)).all() and (side[live] <= int(0.4 * 224) + 1).all()
    centre = np.stack([r[:, 0] + side[:, 0] // 2, r[:, 2] + side[:, 1] // 2], 1)[live]
    assert (centre >= 0).all() and (centre < 224).all()
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    plain = (P["color"] == ident).all((-1, -2))
    assert 0 < plain.mean() < 0.2                            # five colour gates at p = 0.5: all off one time in 32
    # the key is (seed, index, epoch, camera): the row and the batch do not matter, each of the four does
    one = U.draw(U.SEED, 3, index[7:8], np.zeros(1, np.int32), cfg)
    for k in U.KEYS:
        assert np.array_equal(one[k][:, 0], P[k][:, 7]), k
    flipped = U.draw(U.SEED, 3, index[7:8], np.ones(1, np.int32), cfg)           # the other camera first: the suffixes trade draws
    for k in U.KEYS:
        assert np.array_equal(flipped[k][0, 0], P[k][1, 7]) and np.array_equal(flipped[k][1, 0], P[k][0, 7]), k
    for other in (U.draw(U.SEED + 1, 3, index[:50], np.zeros(50, np.int32), cfg), U.draw(U.SEED, 4, index[:50], np.zeros(50, np.int32), cfg),
                  U.draw(U.SEED, 3, index[:50] + 1000, np.zeros(50, np.int32), cfg)):
        assert not np.array_equal(other["gamma"], P["gamma"][:, :50]) and not np.array_equal(other["color"], P["color"][:, :50])
    # a stage switched off leaves its exact neutral value; p = 1 draws every stage; p = 0 none
    off = U.draw(U.SEED, 3, index[:50], np.zeros(50, np.int32), list(_aug(blur_sigma=None, gamma=(1.0, 1.0), noise_sigma=0, occluders=0)._cfg))
    assert (off["blur_taps"][..., 1:] == 0).all() and (off["gamma"] == 1).all() and (off["noise_sigma"] == 0).all() and not off["rects"].any()
    none = U.draw(U.SEED, 3, index[:50], np.zeros(50, np.int32), list(_aug(p=0.0)._cfg))
    for k, v in U.neutral(50).items():
        assert np.array_equal(none[k], v), k
    every = U.draw(U.SEED, 3, index[:50], np.zeros(50, np.int32), list(_aug(p=1.0, blur_sigma=(0.5, 2.0), noise_sigma=(0.01, 0.03))._cfg))
    assert (every["blur_taps"][..., 1] > 0).all() and (every["noise_sigma"] > 0).all() and (every["gamma"] != 1).mean() > 0.99
    wide = U.draw(U.SEED, 3, index[:50], np.zeros(50, np.int32), list(_aug(p=1.0, blur_sigma=(3.0, 4.0))._cfg))
    assert (wide["status"] == U.BLUR_CLAMPED).all() and all(U.radius(w) == 6 for w in wide["blur_taps"].reshape(-1, 7))


def test_restatement_passes_the_oracle_s_bar_and_the_bar_is_not_loose():
    """the libm-free planted images in numpy fp32 against fp64: inside the derived bar, and no further below it than 1 / 64"""
    x, boxes, P = _small()
    for (s, i) in ((0, 0), (1, 0)):
        p = U.image_params(P, s, i)
        r32, r64 = U.chain(x[s, i], boxes[s, i], p, dtype=np.float32), U.chain(x[s, i], boxes[s, i], p, dtype=np.float64)
        assert not r32["libm"] and not r32["copied"]
        cy0, cy1, cx0, cx1 = r64["rect"]
        box = (slice(None), slice(cy0, cy1), slice(cx0, cx1))
        w = U.worst(np.abs(r32["out"][box].astype(np.float64) - r64["out"][box]), r64["bar"][box])
        print("image (%d, %d): the fp32 restatement's worst error / bar %.3f" % (s, i, w))
        assert 1 / 64 <= w <= 1
        inner = r64["out"][:, cy0:cy1, cx0:cx1] * U.STD[:, None, None].astype(np.float64) + U.MEAN[:, None, None]
        assert inner.min() > -1e-6 and inner.max() < 1 + 1e-6
        if (s, i) == (0, 0):                                 # the strong matrix does drive values past both clamps
            assert (np.abs(inner) < 1e-6).mean() > 0.05 and (np.abs(inner - 1) < 1e-6).mean() > 0.05
    # the libm stages: the host's own powf / logf / cosf stay inside the libm bars too
    for (s, i), kind in (((0, 1), "gamma"), ((0, 2), "noise"), ((1, 2), "gamma+noise")):
        p = U.image_params(P, s, i)
        cam = (int(U.CAM0[i]) & 1) ^ s
        r32 = U.chain(x[s, i], boxes[s, i], p, U.SEED, 3, U.INDEX[i], cam, np.float32)
        got_kind, w = U.check_image(r32["out"], x[s, i], boxes[s, i], p, U.SEED, 3, U.INDEX[i], cam)
        print("image (%d, %d): %s, the host libm's worst error / bar %.3f" % (s, i, kind, w))
        assert got_kind == kind and w <= 1
    # noise: mean 0, variance sigma^2, R and G and B uncorrelated; another pixel, another draw
    wd = U._noise_words(U.SEED, 3, 7, 0, (0, 224, 0, 224))
    z, _ = U.box_muller(wd, np.float64)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01 and np.abs(np.corrcoef(z.reshape(3, -1)) - np.eye(3)).max() < 0.02


# ------------------------------------------------------------------------------------------------ the class
def test_class_is_exported_and_refuses_by_name_without_a_gpu():
    import airpose_amd
    from airpose_amd import augment
    assert airpose_amd.CropAugment is augment.CropAugment
    C = airpose_amd.CropAugment
    assert "UNPINNED" in augment.__doc__ and "UNPINNED" in C.__doc__
    with pytest.raises(RuntimeError, match="device must be a CUDA .* there is no CPU path"):
        C(device="cpu")
    with pytest.raises(ValueError, match="seed must be a whole number"):
        C(device="cuda:0", seed=-1)
    with pytest.raises(ValueError, match="p must be in 0 .. 1, got 1.5"):
        C(device="cuda:0", p=1.5)
    with pytest.raises(ValueError, match=r"blur_sigma must be a range \(lo, hi\), None or 0, got 2.0"):
        C(device="cuda:0", blur_sigma=2.0)
    with pytest.raises(ValueError, match="saturation must be lo <= hi"):
        C(device="cuda:0", saturation=(1.4, 0.6))
    with pytest.raises(ValueError, match=r"gamma\[1\] must be a finite number"):
        C(device="cuda:0", gamma=(0.5, float("nan")))
    with pytest.raises(ValueError, match="grayscale must be lo <= hi within 0.0 .. 1.0"):
        C(device="cuda:0", grayscale=(0.0, 1.5))
    with pytest.raises(ValueError, match="hue_deg must be >= 0"):
        C(device="cuda:0", hue_deg=-5.0)
    with pytest.raises(ValueError, match="occluders must be a whole number in 0 .. 4, got 5"):
        C(device="cuda:0", occluders=5)
    a = C(device=torch.device("cuda", 0))
    assert list(a._cfg) == [np.float32(v) for v in CFG] and a.seed == 0
    off = C(device="cuda:0", blur_sigma=None, brightness=0, hue_deg=None, saturation=(1, 1), channel_gain=0, gamma=None, grayscale=0,
            noise_sigma=(0, 0), occluders=0)
    assert list(off._cfg) == [0.5, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, np.float32(0.1), np.float32(0.4)]


def test_methods_refuse_their_arguments_by_name():
    """types and shapes first, the devices last: all reachable with CPU tensors"""
    a = _aug()
    n = 3
    index = torch.arange(n, dtype=torch.int32)
    im, crops = torch.zeros(2, n, 3, 224, 224), torch.zeros(2, n, 4, dtype=torch.int32)
    P = {k: torch.from_numpy(v) for k, v in U.neutral(n).items()}
    with pytest.raises(RuntimeError, match="index must be a tensor, got list"):
        a.draw([1, 2, 3])
    with pytest.raises(RuntimeError, match="index must be int32 .* got torch.int64"):
        a.draw(index.long())
    with pytest.raises(RuntimeError, match=r"index must be \(n,\), got \(3, 1\)"):
        a.draw(index[:, None])
    with pytest.raises(RuntimeError, match="epoch must be an integer, got float"):
        a.draw(index, epoch=0.5)
    with pytest.raises(RuntimeError, match="epoch must be in"):
        a.draw(index, epoch=-1)
    with pytest.raises(RuntimeError, match="cam must be None, 0, 1 or an"):
        a.draw(index, cam=2)
    with pytest.raises(RuntimeError, match="cam must be int32"):
        a.draw(index, cam=torch.zeros(n))
    with pytest.raises(RuntimeError, match=r"cam must be \(n,\) with n = 3, got \(2,\)"):
        a.draw(index, cam=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="index lives on cpu; it must be a CUDA .* there is no CPU path"):
        a.draw(index)
    with pytest.raises(RuntimeError, match="im must be a tensor, got ndarray"):
        a.apply(im.numpy(), crops, P, index)
    with pytest.raises(RuntimeError, match="im must be float32 .* got torch.float64"):
        a.apply(im.double(), crops, P, index)
    with pytest.raises(RuntimeError, match=r"im must be \(2, n, 3, 224, 224\), got \(3, 3, 224, 224\)"):
        a.apply(im[0], crops, P, index)
    with pytest.raises(RuntimeError, match=r"index must be \(n,\) with n = 3, got \(2,\)"):
        a.apply(im, crops, P, index[:2])
    with pytest.raises(RuntimeError, match="crops must be int32"):
        a.apply(im, crops.float(), P, index)
    with pytest.raises(RuntimeError, match=r"crops must be \(2, n, 4\) with n = 3, got \(2, 3, 2, 2\)"):
        a.apply(im, crops.reshape(2, n, 2, 2), P, index)
    with pytest.raises(RuntimeError, match="params must be the dict draw"):
        a.apply(im, crops, None, index)
    with pytest.raises(RuntimeError, match="params has no 'gamma'"):
        a.apply(im, crops, {k: v for k, v in P.items() if k != "gamma"}, index)
    with pytest.raises(RuntimeError, match=r"params\['rects'\] must be int32 .* got torch.int64"):
        a.apply(im, crops, dict(P, rects=P["rects"].long()), index)
    with pytest.raises(RuntimeError, match=r"params\['color'\] must be .* with n = 3, got \(2, 3, 3, 3\)"):
        a.apply(im, crops, dict(P, color=P["color"][..., :3]), index)
    with pytest.raises(RuntimeError, match="out must be a contiguous float32 tensor of im's shape"):
        a.apply(im, crops, P, index, out=torch.zeros(2, n, 3, 224, 223))
    with pytest.raises(RuntimeError, match="index lives on cpu; it must be a CUDA .* there is no CPU path"):
        a.apply(im, crops, P, index)
    with pytest.raises(RuntimeError, match="batch must be the dict"):
        a([im], index)
    with pytest.raises(RuntimeError, match="batch has no 'crops1'"):
        a({"im0": im[0], "im1": im[1], "crops0": crops[0]}, index)
    with pytest.raises(RuntimeError, match=r"batch\['im1'\] must be \(n, 3, 224, 224\)"):
        a({"im0": im[0], "im1": im[1, :2], "crops0": crops[0], "crops1": crops[1]}, index)
    with pytest.raises(RuntimeError, match="index lives on cpu; it must be a CUDA .* there is no CPU path"):
        a({"im0": im[0], "im1": im[1], "crops0": crops[0], "crops1": crops[1]}, index)
