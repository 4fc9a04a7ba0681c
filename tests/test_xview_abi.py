"""CPU checks of the apg_xview_* entry points of libairpose_grad.so (airpose_amd/csrc/xview_metrics.hip): declared == exported ==
bound, the header documents the accumulator, the skip rule, the validity rule and the angle formula, the two ABI numbers stay where
they are, and every refusal happens on the host -- the pointers below are made-up addresses that are never dereferenced (there is no
GPU here), the result is APG_EINVAL (APG_ENOMEM for the workspace's size, as in every other entry) and the message names the
argument."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL, ENOMEM = -1, -4
FAKE = 0x7f0000001000                                    # 4096-aligned and never touched
NAMES = ["apg_xview_acc_doubles", "apg_xview_triangulate", "apg_xview_update", "apg_xview_workspace_bytes"]
ENTRIES = ("joints", "extr", "vertices", "root", "trans", "rot", "j2d", "keypoints", "intr")
STRIDES = dict(joints=66, extr=16, vertices=120, root=3, trans=3, rot=198, j2d=44, keypoints=144, intr=9)


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _table(**entries):
    """the eighteen per-view pointers with entries (name + view, e.g. root1) replaced"""
    t = [FAKE + 0x100000 * (k + 1) for k in range(18)]
    for k, val in entries.items():
        t[int(k[-1]) * 9 + ENTRIES.index(k[:-1])] = val
    return t


def _strides(**over):
    s = dict(STRIDES)
    s.update(over)
    return [s[k] for k in ENTRIES]


def _args(**over):
    """a valid argument set of apg_xview_update on made-up addresses; `over` replaces entries"""
    a = dict(B=4, views=2, n_joints=22, N=40, flags=1, strides=_strides(), per_view=_table(), min_sin2=3e-4, per_sample=FAKE + 0x21000,
             tri=FAKE + 0x22000, acc=FAKE + 0x24000, workspace=FAKE + 0x25000, workspace_bytes=1 << 20)
    a.update(over)
    return a


def _call(a):
    _, L = _lib()
    vp = ctypes.c_void_p
    table = None if a["per_view"] is None else (ctypes.c_void_p * len(a["per_view"]))(*a["per_view"])
    strides = None if a["strides"] is None else (ctypes.c_int64 * len(a["strides"]))(*a["strides"])
    rc = L.apg_xview_update(a["B"], a["views"], a["n_joints"], a["N"], a["flags"], strides, table, a["min_sin2"], vp(a["per_sample"]),
                            vp(a["tri"]), vp(a["acc"]), vp(a["workspace"]), a["workspace_bytes"], None)
    return rc, L.apg_last_error().decode()


def _without(*names):
    """both views' pointers of the named entries NULL"""
    return _table(**{n + str(v): None for n in names for v in range(2)})


REFUSALS = [
    ("B_zero", dict(B=0), "B"),
    ("B_negative", dict(B=-1), "B"),
    ("B_large", dict(B=(1 << 22) + 1), "B"),
    ("views_1", dict(views=1), "views"),
    ("views_3", dict(views=3), "views"),
    ("n_joints_zero", dict(n_joints=0), "n_joints"),
    ("N_negative", dict(N=-3), "N"),
    ("N_large", dict(N=(1 << 24) + 1), "N"),
    ("flags_2", dict(flags=2), "flags"),
    ("min_sin2_negative", dict(min_sin2=-0.1), "min_sin2"),
    ("min_sin2_nan", dict(min_sin2=float("nan")), "min_sin2"),
    ("null_strides", dict(strides=None), "strides"),
    ("null_per_view", dict(per_view=None), "per_view"),
    ("null_acc", dict(acc=None), "acc"),
    ("null_workspace", dict(workspace=None), "workspace"),
    ("null_joints0", dict(per_view=_table(joints0=None)), "joints of view 0"),
    ("null_joints1", dict(per_view=_table(joints1=None)), "joints of view 1"),
    ("null_extr0", dict(per_view=_table(extr0=None)), "extr of view 0"),
    ("null_extr1", dict(per_view=_table(extr1=None)), "extr of view 1"),
    ("vertices_one_view", dict(per_view=_table(vertices1=None)), "vertices of view 0 is given for one view only"),
    ("root_one_view", dict(per_view=_table(root0=None)), "root of view 1 is given for one view only"),
    ("trans_one_view", dict(per_view=_table(trans1=None)), "trans of view 0 is given for one view only"),
    ("rot_one_view", dict(per_view=_table(rot0=None)), "rot of view 1 is given for one view only"),
    ("j2d_one_view", dict(per_view=_table(j2d1=None)), "j2d of view 0 is given for one view only"),
    ("keypoints_one_view", dict(per_view=_table(keypoints0=None)), "keypoints of view 1 is given for one view only"),
    ("intr_one_view", dict(per_view=_table(intr1=None)), "intr of view 0 is given for one view only"),
    ("vertices_without_N", dict(N=0), "vertices"),
    ("N_without_vertices", dict(per_view=_without("vertices")), "without vertices"),
    ("j2d_without_keypoints", dict(per_view=_without("keypoints", "intr"), tri=None), "j2d is given without keypoints"),
    ("intr_without_keypoints", dict(per_view=_without("keypoints", "j2d"), tri=None), "intr is given without keypoints"),
    ("keypoints_alone", dict(per_view=_without("j2d", "intr"), tri=None), "keypoints are given without"),
    ("tri_without_intr", dict(per_view=_without("intr")), "tri is asked for without intr"),
    ("misaligned_joints0", dict(per_view=_table(joints0=FAKE + 2)), "joints of view 0"),
    ("misaligned_extr1", dict(per_view=_table(extr1=FAKE + 0x600001)), "extr of view 1"),
    ("misaligned_vertices1", dict(per_view=_table(vertices1=FAKE + 0x700003)), "vertices of view 1"),
    ("misaligned_keypoints0", dict(per_view=_table(keypoints0=FAKE + 0x800002)), "keypoints of view 0"),
    ("misaligned_per_sample", dict(per_sample=FAKE + 0x21002), "per_sample"),
    ("misaligned_tri", dict(tri=FAKE + 0x22001), "tri"),
    ("misaligned_acc", dict(acc=FAKE + 0x24004), "acc"),
    ("misaligned_workspace", dict(workspace=FAKE + 0x25004), "workspace"),
    ("joints_stride_short", dict(strides=_strides(joints=65)), "joints_stride"),
    ("extr_stride_short", dict(strides=_strides(extr=11)), "extr_stride"),
    ("vertices_stride_short", dict(strides=_strides(vertices=119)), "vertices_stride"),
    ("root_stride_short", dict(strides=_strides(root=2)), "root_stride"),
    ("trans_stride_short", dict(strides=_strides(trans=0)), "trans_stride"),
    ("rot_stride_short", dict(strides=_strides(rot=197)), "rot_stride"),
    ("rot_stride_short_aa", dict(strides=_strides(rot=65), flags=0), "rot_stride"),
    ("j2d_stride_short", dict(strides=_strides(j2d=43)), "j2d_stride"),
    ("keypoints_stride_short", dict(strides=_strides(keypoints=65)), "keypoints_stride"),
    ("intr_stride_short", dict(strides=_strides(intr=8)), "intr_stride"),
    ("joints_stride_short_for_tri", dict(n_joints=1, strides=_strides(joints=3)), "joints_stride must be at least 66"),
]


def test_header_exports_and_binding_agree_on_the_xview_names():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_xview_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_xview_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_xview_"))
    assert declared == exported == bound == NAMES
    decl = re.search(r"int apg_xview_update\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(G.SIGNATURES["apg_xview_update"][1]) == 14
    decl = re.search(r"int apg_xview_triangulate\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(G.SIGNATURES["apg_xview_triangulate"][1]) == 11
    assert len(G.SIGNATURES["apg_xview_workspace_bytes"][1]) == 3 and G.SIGNATURES["apg_xview_acc_doubles"][1] == []


def test_header_documents_the_accumulator_and_the_rules():
    text = open(HEADER).read()
    at = text.index("Cross-view metrics (xview_metrics.hip)")
    doc = text[at:text.index("int64_t apg_xview_workspace_bytes", at)]
    for phrase in ("ADDED to", "[0] samples seen", "[1] skipped", "[2] sum of joint_gap_world", "[3] sum of joint_gap_root",
                   "[4] samples that", "[5] sum of vertex_gap_world", "[6] sum of vertex_gap_root", "[9] sum of trans_gap",
                   "[11] sum of orient_gap_deg", "sum of\n *     pose_gap_deg", "[14] [15] sum of reproj_px", "[18] [19] sum of reproj_n",
                   "[23] tri_n", "[25] reserved",
                   "skip rule:", "max |R_v^T R_v - I| > 1e-3", "design constant",
                   "validity rule:", "both confidences are > 0", ">= min_sin2",
                   "angle formula:", "atan2(|(D21 - D12, D02 - D20, D10 - D01)|, tr D - 1)", "not acos",
                   "Additive under ABI 2"):
        assert phrase in doc, phrase
    assert int(re.search(r"#define\s+APG_XVIEW_ACC\s+(\d+)", text).group(1)) == 26
    assert int(re.search(r"#define\s+APG_XVIEW_PER_VIEW\s+(\d+)", text).group(1)) == 9
    assert int(re.search(r"#define\s+APG_XVIEW_PER_SAMPLE\s+(\d+)", text).group(1)) == 16


def test_abi_numbers_stay():
    from airpose_amd import _native
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2
    assert _native.ABI_VERSION == 13
    assert not any(n.startswith("apg_") for n in _native.SIGNATURES)


@pytest.mark.parametrize("over,names", [(r[1], r[2]) for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _call(_args(**over))
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_xview_update: ") and names in msg[len("apg_xview_update: "):], msg


def test_only_the_changed_argument_is_what_a_refusal_is_about():
    """the valid set differs from each refusal in one entry; its own checks pass up to the launch, which this machine cannot make --
    so the valid set is checked through the one refusal that comes last, the workspace's size"""
    _, L = _lib()
    need = L.apg_xview_workspace_bytes(4, 2, 40)
    rc, msg = _call(_args(workspace_bytes=need - 1))
    assert rc == ENOMEM and "workspace" in msg and str(need) in msg, (rc, msg)
    lean = _without("vertices", "root", "trans", "rot", "j2d", "keypoints", "intr")          # nothing optional: no stride is looked at
    rc, msg = _call(_args(N=0, per_view=lean, per_sample=None, tri=None, n_joints=1, strides=[3, 12, 0, 0, 0, 0, 0, 0, 0],
                          workspace_bytes=L.apg_xview_workspace_bytes(4, 2, 0) - 1))
    assert rc == ENOMEM, (rc, msg)
    rc, msg = _call(_args(workspace_bytes=need - 1, flags=0, strides=_strides(joints=1000, extr=12, rot=66, keypoints=66, j2d=45)))
    assert rc == ENOMEM, (rc, msg)


TRI_REFUSALS = [("B_zero", dict(B=0), "B"), ("J_zero", dict(J=0), "J"), ("min_sin2", dict(min_sin2=1.5), "min_sin2"),
                ("null_kp0", dict(kp0=None), "kp0"), ("null_kp1", dict(kp1=None), "kp1"), ("null_intr0", dict(intr0=None), "intr0"),
                ("null_intr1", dict(intr1=None), "intr1"), ("null_extr0", dict(extr0=None), "extr0"), ("null_extr1", dict(extr1=None), "extr1"),
                ("null_out", dict(out=None), "out"), ("misaligned_kp1", dict(kp1=FAKE + 2), "kp1"), ("misaligned_out", dict(out=FAKE + 0x7001), "out")]


@pytest.mark.parametrize("over,names", [(r[1], r[2]) for r in TRI_REFUSALS], ids=[r[0] for r in TRI_REFUSALS])
def test_triangulate_refusals(over, names):
    _, L = _lib()
    a = dict(B=3, J=22, kp0=FAKE + 0x1000, kp1=FAKE + 0x2000, intr0=FAKE + 0x3000, intr1=FAKE + 0x4000, extr0=FAKE + 0x5000,
             extr1=FAKE + 0x6000, min_sin2=0.0, out=FAKE + 0x7000)
    a.update(over)
    vp = ctypes.c_void_p
    rc = L.apg_xview_triangulate(a["B"], a["J"], vp(a["kp0"]), vp(a["kp1"]), vp(a["intr0"]), vp(a["intr1"]), vp(a["extr0"]),
                                 vp(a["extr1"]), a["min_sin2"], vp(a["out"]), None)
    msg = L.apg_last_error().decode()
    assert rc == EINVAL and msg.startswith("apg_xview_triangulate: ") and names in msg[len("apg_xview_triangulate: "):], (rc, msg)


def test_size_queries():
    _, L = _lib()
    assert L.apg_xview_acc_doubles() == 26
    for B in (1, 2, 30, 256, 1 << 16):                       # B * chunks stays below 2^31
        for N, chunks in ((0, 1), (1, 1), (1024, 1), (1025, 2), (10475, 11), (1 << 24, 1 << 14)):
            assert L.apg_xview_workspace_bytes(B, 2, N) == B * (24 + 2 * chunks) * 8
    for bad in ((0, 2, 22), (-1, 2, 22), (4, 0, 22), (4, 1, 22), (4, 3, 22), (4, 2, -1), ((1 << 22) + 1, 2, 22), (4, 2, (1 << 24) + 1),
                (1 << 22, 2, 1 << 24)):
        assert L.apg_xview_workspace_bytes(*bad) < 0, bad
