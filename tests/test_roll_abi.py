"""CPU checks of the camera roll (airpose_amd/csrc/roll.hip, airpose_amd/roll.py) without a GPU: declared == exported == bound for
apg_roll_*, the ABI number stays 2 and the inference library gains nothing, the header states the contract, every refusal of the three
entries happens on the host -- the device pointers below are made-up addresses that are never dereferenced -- and names its argument,
the source is built like augment.hip and carries no packed fp32 math, and the restatement of roll_util.py holds against its own
oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import roll_util as U
from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL = -1
FAKE = 0x7f0000001000                                        # 4096-aligned and never touched
N = 5
DRAW_PTRS = ("index", "cam", "rot")
LABEL_IN = ("rot", "intr", "bb", "crops", "verts", "joints", "orient", "trans", "extr", "j2d", "j2d_crop")
LABEL_OUT = ("rot_used", "bb_out", "status", "verts_out", "joints_out", "orient_out", "trans_out", "extr_out", "j2d_out", "j2d_crop_out")
LABEL_PTRS = ("cam",) + LABEL_IN + LABEL_OUT
OPTIONAL = ("verts", "joints", "orient", "trans", "extr", "j2d", "j2d_crop")
CROPS_PTRS = ("frames0", "frames1", "cam", "crops", "intr", "rot_used", "im")
SPACING = 0x10000000                                         # between the made-up arrays: more than any of them holds


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _fake(names):
    return {n: FAKE + SPACING * (k + 1) for k, n in enumerate(names)}


def _draw(**over):
    _, L = _lib()
    a = dict(n=N, seed=3, epoch=1, cam_all=0, p=0.5, max_rad=0.5)
    a.update(_fake(DRAW_PTRS))
    a.update(over)
    vp = ctypes.c_void_p
    rc = L.apg_roll_draw(a["n"], a["seed"], a["epoch"], vp(a["index"]), vp(a["cam"]), a["cam_all"], a["p"], a["max_rad"], vp(a["rot"]), None)
    return rc, L.apg_last_error().decode()


def _labels(**over):
    _, L = _lib()
    a = dict(n=N, V=7, J=3, P=4, pstride=3, Hc0=96, Wc0=128, Hc1=61, Wc1=47, cam_all=0)
    a.update(_fake(LABEL_PTRS))
    a.update(over)
    vp = ctypes.c_void_p
    rc = L.apg_roll_labels(a["n"], a["V"], a["J"], a["P"], a["pstride"], a["Hc0"], a["Wc0"], a["Hc1"], a["Wc1"], vp(a["cam"]), a["cam_all"],
                           *[vp(a[k]) for k in LABEL_IN], *[vp(a[k]) for k in LABEL_OUT], None)
    return rc, L.apg_last_error().decode()


def _crops(**over):
    _, L = _lib()
    a = dict(n=N, Hc0=96, Wc0=128, Hc1=61, Wc1=47, bgr=1, cam_all=0)
    a.update(_fake(CROPS_PTRS))
    a.update(over)
    vp = ctypes.c_void_p
    rc = L.apg_roll_crops(a["n"], a["Hc0"], a["Wc0"], a["Hc1"], a["Wc1"], a["bgr"], vp(a["frames0"]), vp(a["frames1"]), vp(a["cam"]),
                          a["cam_all"], vp(a["crops"]), vp(a["intr"]), vp(a["rot_used"]), vp(a["im"]), None)
    return rc, L.apg_last_error().decode()


ODD = FAKE + 0x900002
SIDES = [("%s_%s" % (k, w), {k: v}, k + " must be in 1 .. 1048576") for k in ("Hc0", "Wc0", "Hc1", "Wc1") for w, v in (("zero", 0), ("huge", (1 << 20) + 1))]
N_CAM = [("n_zero", dict(n=0), "n must be in 1 .. 65535"), ("n_negative", dict(n=-1), "n must be in"), ("n_too_large", dict(n=65536), "n must be in"),
         ("cam_all_other", dict(cam_all=2), "cam_all must be 0 or 1"), ("misaligned_cam", dict(cam=ODD), "cam is not 4-byte aligned")]
DRAW_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in ("index", "rot")] + \
                [("misaligned_" + n, {n: ODD}, n + " is not 4-byte aligned") for n in ("index", "rot")] + N_CAM + [
    ("p_negative", dict(p=-0.1), "p must be in 0 .. 1"), ("p_above_one", dict(p=1.5), "p must be in 0 .. 1"), ("p_nan", dict(p=float("nan")), "p must be in"),
    ("max_rad_negative", dict(max_rad=-0.1), "max_rad must be in 0 .. pi"), ("max_rad_above_pi", dict(max_rad=3.2), "max_rad must be in 0 .. pi"),
    ("max_rad_inf", dict(max_rad=float("inf")), "max_rad must be in")]
LAB = _fake(LABEL_PTRS)
ROWS = 2 * N
LABEL_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in ("rot", "intr", "bb", "crops", "rot_used", "bb_out", "status")] + \
                 [("null_%s_out" % n, {n + "_out": None}, n + "_out is NULL") for n in OPTIONAL] + \
                 [("misaligned_" + n, {n: ODD}, n + " is not 4-byte aligned") for n in LABEL_IN + LABEL_OUT] + N_CAM + SIDES + [
    ("V_zero", dict(V=0), "V must be in 1 .. 16777216"), ("V_huge", dict(V=(1 << 24) + 1), "V must be in"), ("J_zero", dict(J=0), "J must be in 1 .. 65536"),
    ("J_huge", dict(J=(1 << 16) + 1), "J must be in"), ("P_zero", dict(P=0), "P must be in 1 .. 65536"), ("pstride_four", dict(pstride=4), "pstride must be 2 or 3"),
    ("pstride_one", dict(pstride=1), "pstride must be 2 or 3"),
    ("verts_out_is_verts", dict(verts_out=LAB["verts"]), "verts_out must not overlap verts"),
    ("verts_out_ends_inside_verts", dict(verts_out=LAB["verts"] - ROWS * 7 * 12 + 4), "verts_out must not overlap verts"),
    ("joints_out_starts_inside_joints", dict(joints_out=LAB["joints"] + ROWS * 3 * 12 - 4), "joints_out must not overlap joints"),
    ("orient_out_is_orient", dict(orient_out=LAB["orient"]), "orient_out must not overlap orient"),
    ("trans_out_is_trans", dict(trans_out=LAB["trans"]), "trans_out must not overlap trans"),
    ("extr_out_is_extr", dict(extr_out=LAB["extr"]), "extr_out must not overlap extr"),
    ("j2d_out_is_j2d", dict(j2d_out=LAB["j2d"]), "j2d_out must not overlap j2d"),
    ("j2d_crop_out_inside", dict(j2d_crop_out=LAB["j2d_crop"] + ROWS * 4 * 12 - 4), "j2d_crop_out must not overlap j2d_crop"),
    ("rot_used_is_rot", dict(rot_used=LAB["rot"]), "rot_used must not overlap rot"), ("bb_out_is_bb", dict(bb_out=LAB["bb"] + 8), "bb_out must not overlap bb")]
CR = _fake(CROPS_PTRS)
IM_BYTES = 2 * N * 3 * 224 * 224 * 4
CROPS_REFUSALS = [("null_" + n, {n: None}, n + " is NULL") for n in CROPS_PTRS if n != "cam"] + \
                 [("misaligned_" + n, {n: ODD}, n + " is not 4-byte aligned") for n in ("crops", "intr", "rot_used", "im")] + N_CAM + SIDES + [
    ("bgr_two", dict(bgr=2), "bgr must be 0 or 1"), ("im_is_frames0", dict(im=CR["frames0"]), "im must not overlap frames0"),
    ("im_ends_inside_frames1", dict(im=CR["frames1"] - IM_BYTES + 4), "im must not overlap frames1"),
    ("im_starts_inside_frames1", dict(im=CR["frames1"] + N * 61 * 47 * 3 - 1), "im must not overlap frames1")]


def test_header_exports_and_binding_agree():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_roll_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_roll_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_roll_"))
    assert declared == exported == bound == ["apg_roll_crops", "apg_roll_draw", "apg_roll_labels"]
    want = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    for entry, count in (("apg_roll_draw", 10), ("apg_roll_labels", 33), ("apg_roll_crops", 15)):
        decl = re.search(r"int %s\((.*?)\);" % entry, src, flags=re.S)
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        res, args = G.SIGNATURES[entry]
        assert len(params) == len(args) == count and res is ctypes.c_int, entry
        for p, t in zip(params, args):                       # every parameter's C type against its ctypes type
            assert t is (ctypes.c_void_p if "*" in p else want[p.rsplit(" ", 1)[0]]), (entry, p)
    text = open(HEADER).read()
    for name, val in (("APG_ROLL_THREADS", G.ROLL_THREADS), ("APG_ROLL_CENTRE_OUT", G.ROLL_CENTRE_OUT), ("APG_ROLL_OFF_CANVAS", G.ROLL_OFF_CANVAS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == val, name
    assert (G.ROLL_CENTRE_OUT, G.ROLL_OFF_CANVAS) == (U.CENTRE_OUT, U.OFF_CANVAS)


def test_abi_number_stays_and_the_inference_library_gains_no_symbol():
    from airpose_amd import _native
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2
    syms = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "roll" not in syms and not any(n.startswith("apg_") for n in _native.SIGNATURES)
    inf = open(os.path.join(REPO, "include", "airpose_hip.h")).read()
    assert "roll" not in inf


def test_header_and_draws_inc_document_the_contract():
    text = open(HEADER).read()
    at = text.index("Camera roll (roll.hip)")
    doc = " ".join(text[at:text.index("#define APG_ROLL_THREADS", at)].replace("\n *", " ").split())      # one line, the comment's margin gone
    for phrase in ("Additive under ABI 2", "ROLL OF THE CAMERA ABOUT ITS OPTICAL AXIS", "block 15, camera 0 / 1", "Philox4x32-10", "zero continuation",
                   "a tap outside the canvas contributes 0", "The refusal rule", "|bb'_x| <= 1 and |bb'_y| <= 1", "(c, sn) := (1, 0) exactly",
                   "APG_ROLL_CENTRE_OUT", "APG_ROLL_OFF_CANVAS", "no fused multiply-add", "preprocess_px.inc", "copied bit for bit",
                   "rows 2 and 3 copied", "A(-theta)", "(word >> 8) * 2^-24", "taken in fp64 and rounded once", "not overlap its input",
                   "plain vector stores", "NOT changed", "Flips (a mirrored body", "zoom (it changes the depth"):
        assert phrase in doc, phrase
    inc = open(os.path.join(REPO, "airpose_amd", "csrc", "draws.inc")).read()
    assert re.search(r"block 15, camera 0 / 1\s+apg_roll_draw", inc)


@pytest.mark.parametrize("over,names", [r[1:] for r in DRAW_REFUSALS], ids=[r[0] for r in DRAW_REFUSALS])
def test_draw_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _draw(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_roll_draw: ") and names in msg[len("apg_roll_draw: "):], msg


@pytest.mark.parametrize("over,names", [r[1:] for r in LABEL_REFUSALS], ids=[r[0] for r in LABEL_REFUSALS])
def test_labels_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _labels(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_roll_labels: ") and names in msg[len("apg_roll_labels: "):], msg


@pytest.mark.parametrize("over,names", [r[1:] for r in CROPS_REFUSALS], ids=[r[0] for r in CROPS_REFUSALS])
def test_crops_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _crops(**over)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_roll_crops: ") and names in msg[len("apg_roll_crops: "):], msg


def test_an_absent_label_needs_neither_its_output_nor_its_count():
    """NULL = the dict has no such key: the refusals of its count and of its output do not fire (the call is then refused further on, by
    a count that IS looked at, so that nothing is launched from here)"""
    rc, msg = _labels(verts=None, verts_out=None, V=0, joints=None, joints_out=None, J=-3, pstride=7)
    assert rc == EINVAL and "pstride must be 2 or 3" in msg, msg
    rc, msg = _labels(j2d=None, j2d_out=None, j2d_crop=None, j2d_crop_out=None, P=0, pstride=0, V=0)
    assert rc == EINVAL and "V must be in" in msg, msg


def test_the_source_is_built_like_augment_and_its_kernels_carry_no_packed_math():
    """tests/packed_math_scan.json, the committed scan of SRCS and GRAD_SRCS, is an existing test file and stays as it is, so roll.hip is
    linked into libairpose_grad.so through ROLL_SRCS and held HERE to what the list holds the others to: the scan tool sees it
    (linked_apart), every .hip file of csrc is either in the committed list or scanned live below -- nothing that ships is outside
    both --, its flags are augment.hip's, and its kernels carry no packed fp32 math, hence not the SUSPECT signature of
    tests/test_packed_math_scan.py; without the flags the scan still reads the kernels (it is not blind to this source)"""
    import glob
    import shutil
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import packed_math_scan as S
    text = open(os.path.join(REPO, "airpose_amd", "csrc", "Makefile")).read()
    assert re.search(r"^ROLL_SRCS\s*=\s*roll\.hip\s*$", text, re.M) and re.search(r"^GRAD_OBJS\s*=.*\$\(ROLL_SRCS:\.hip=\.o\)", text, re.M)
    assert re.search(r"^FLAGS_roll\s*=\s*-ffp-contract=off -fno-slp-vectorize\s*$", text, re.M)
    hipcc, _, flags, _, listed = S.makefile()
    assert shutil.which(hipcc), "%s: the scan needs the compiler the build uses" % hipcc
    apart = S.linked_apart()
    assert apart == ["roll"] and flags["roll"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    on_disk = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(REPO, "airpose_amd", "csrc", "*.hip")))
    host = [s[:-4] for s in re.search(r"^APISRCS\s*=\s*(.*)$", text, re.M).group(1).split()]            # the host layer: no kernel
    assert on_disk == sorted(set(listed) | set(apart) | set(host)), "a kernel source that neither the committed list nor this test scans"
    assert not [s for s in host if "__global__" in open(os.path.join(REPO, "airpose_amd", "csrc", s + ".hip")).read()]
    rows = S.scan_sources(apart)
    assert sorted(r["kernel"] for r in rows) == ["roll_crops_kernel", "roll_draw_kernel", "roll_labels_kernel"]
    for r in rows:
        assert r["flags"] == "-ffp-contract=off -fno-slp-vectorize" and r["packed"] == 0 and r["op_sel"] == 0 and r["ds_reads"] == 0, r
    bare = S.scan_sources(apart, drop_flags=True)
    assert sorted(r["kernel"] for r in bare) == sorted(r["kernel"] for r in rows) and all(r["flags"] == "" for r in bare)
    G, _ = _lib()                                            # ... and the built library is the one with these kernels in it
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "apg_roll_crops" in syms


# ------------------------------------------------------------------------------------------------ the oracle, on the CPU
def test_restatement_passes_the_oracle_s_bar_and_the_bar_is_not_loose():
    c = U.case()
    r = U.restate(c)
    assert r["status"].tolist() == [[U.CENTRE_OUT, 0, U.OFF_CANVAS], [0, 0, 0]]
    assert r["rot_used"][0, 0].tolist() == [1, 0] and r["rot_used"][1, 2].tolist() == [1, 0]
    worst_label = worst_px = 0.0
    for s in (0, 1):
        for i in range(U.N):
            cu, su = r["rot_used"][s, i]
            K = c["intr"][s, i]
            lab = {k: v[s, i] for k, v in c["labels"].items()}
            o = U.roll_labels(cu, su, K, lab, oracle=True)
            if cu == 1 and su == 0:                          # un-rolled: the input's bits, -0.0 included
                for k in lab:
                    assert np.array_equal(r["labels"][k][s, i].view(np.uint32), lab[k].view(np.uint32)), (s, i, k)
                assert np.array_equal(r["bb_out"][s, i].view(np.uint32), c["bb"][s, i].view(np.uint32))
                continue
            for k in o:
                worst_label = max(worst_label, U.worst(np.abs(r["labels"][k][s, i].astype(np.float64) - o[k].v), o[k].e))
            cam = U.camera_of(s, i)
            a = U.roll_image(c["frames"][cam][i], c["crops"][s, i], cu, su, K, 1)
            v, bar = U.roll_image(c["frames"][cam][i], c["crops"][s, i], cu, su, K, 1, oracle=True)
            worst_px = max(worst_px, U.worst(np.abs(a.astype(np.float64) - v), bar))
            assert a.dtype == np.float32 and np.isfinite(a).all()
    print("the fp32 restatement's worst error / bar: labels %.3f, pixels %.3f" % (worst_label, worst_px))
    assert 1 / 64 <= worst_label <= 1 and 1 / 64 <= worst_px <= 1
    # a quarter turn of a square focal length sends (x, y, z) to (-y, x, z) up to cos(90 degrees) = 6e-17 in fp32
    q = U.roll_labels(r["rot_used"][0, 2, 0], r["rot_used"][0, 2, 1], c["intr"][0, 2], {"trans": np.asarray([1, 2, 3], np.float32)})["trans"]
    assert np.allclose(q, (-2, 1, 3), atol=1e-6)
    # the rolled image of a constant canvas is that constant wherever all four taps lie on the canvas, and 0's value beyond it
    flat = np.full((96, 128, 3), 200, np.uint8)
    img = U.roll_image(flat, (20, 70, 30, 100), np.float32(np.cos(0.3)), np.float32(np.sin(0.3)), c["intr"][0, 2], 1)
    inner = img[:, 100:124, 60:160].astype(np.float64) * U.STD[:, None, None] + U.MEAN[:, None, None]
    assert np.abs(inner - 200 / 255).max() < 1e-6


def test_draws_gate_and_angles():
    n = 2000
    index = np.arange(100, 100 + n)
    gate, ang, cs = U.draw(U.SEED, 2, index, np.zeros(n, np.int32), 0.5, np.float32(np.pi / 6))
    assert 0.45 < gate.mean() < 0.55 and np.abs(ang).max() <= np.float32(np.pi / 6) and abs(ang[gate].mean()) < 0.03
    assert (cs[~gate] == (1, 0)).all() and np.abs((cs ** 2).sum(-1) - 1).max() < 1e-15
    one = U.draw(U.SEED, 2, index[7:8], np.ones(1, np.int32), 0.5, np.float32(np.pi / 6))
    assert np.array_equal(one[1][0, 0], ang[1, 7]) and np.array_equal(one[1][1, 0], ang[0, 7])      # the suffixes trade draws
    for other in (U.draw(U.SEED + 1, 2, index, np.zeros(n, np.int32), 0.5, 0.5), U.draw(U.SEED, 3, index, np.zeros(n, np.int32), 0.5, 0.5)):
        assert not np.array_equal(other[0], gate)
    # block 15 is the roll's own: the augmentation's blocks 1 .. 14 and the batches' block 0 draw other words
    from synth_batch_util import philox
    key = (U.SEED & 0xFFFFFFFF, U.SEED >> 32)
    words = [philox((7, 2, 0, b), key) for b in range(16)]
    assert len({tuple(w.tolist()) for w in words}) == 16


# ------------------------------------------------------------------------------------------------ the class
def test_class_is_exported_and_refuses_by_name_without_a_gpu():
    import torch
    import airpose_amd
    from airpose_amd import roll
    assert airpose_amd.CameraRoll is roll.CameraRoll
    C = airpose_amd.CameraRoll
    assert "NOBODY HAS MEASURED" in roll.__doc__ and "unmeasured" in C.__doc__ and "NOT built" in roll.__doc__
    with pytest.raises(RuntimeError, match="device must be a CUDA .* there is no CPU path"):
        C(device="cpu")
    with pytest.raises(ValueError, match="seed must be a whole number"):
        C(device="cuda:0", seed=-1)
    with pytest.raises(ValueError, match="p must be in 0 .. 1, got 1.5"):
        C(device="cuda:0", p=1.5)
    with pytest.raises(ValueError, match="max_deg must be in 0 .. 180, got 181"):
        C(device="cuda:0", max_deg=181)
    with pytest.raises(ValueError, match="max_deg must be a finite number"):
        C(device="cuda:0", max_deg=float("nan"))
    a = C(device=torch.device("cuda", 0))
    assert (a.seed, a.p, a.max_deg) == (0, 0.5, 30.0) and abs(a.max_rad - np.pi / 6) < 1e-15
