"""CPU checks of the apg_eval_* entry points of libairpose_grad.so (airpose_amd/csrc/eval_metrics.hip): declared == exported ==
bound, the two ABI numbers stay where they are, and every refusal happens on the host -- the pointers below are made-up addresses
that are never dereferenced (there is no GPU here), the result is APG_EINVAL and the message names the argument."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL, ENOMEM = -1, -4
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19]
FAKE = 0x7f0000001000                                    # 4096-aligned and never touched


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _args(**over):
    """a valid argument set of apg_eval_update on made-up addresses; `over` replaces entries"""
    a = dict(B=4, views=2, flags=0, j_rest=FAKE, parents=list(PARENTS),
             per_view=[FAKE + 0x1000 * (k + 1) for k in range(10)], gt_body=FAKE + 0x20000, joint_err=FAKE + 0x21000,
             trans_err=FAKE + 0x22000, angle_err=FAKE + 0x23000, acc=FAKE + 0x24000, workspace=FAKE + 0x25000, workspace_bytes=1 << 20)
    a.update(over)
    return a


def _call(a):
    G, L = _lib()
    vp = ctypes.c_void_p
    table = None if a["per_view"] is None else (ctypes.c_void_p * len(a["per_view"]))(*a["per_view"])
    parents = None if a["parents"] is None else G.ints(a["parents"])
    rc = L.apg_eval_update(a["B"], a["views"], a["flags"], vp(a["j_rest"]), parents, table, vp(a["gt_body"]), vp(a["joint_err"]),
                           vp(a["trans_err"]), vp(a["angle_err"]), vp(a["acc"]), vp(a["workspace"]), a["workspace_bytes"], None)
    return rc, L.apg_last_error().decode()


def _table(**entries):
    """the ten per-view pointers with entries (name + view, e.g. pred_trans1) replaced"""
    names = ("gt_orient", "pred_rot", "gt_trans", "pred_trans", "gt_angles")
    t = [FAKE + 0x1000 * (k + 1) for k in range(10)]
    for k, val in entries.items():
        t[int(k[-1]) * 5 + names.index(k[:-1])] = val
    return t


def _bad_parents(j, val):
    p = list(PARENTS)
    p[j] = val
    return p


REFUSALS = [
    ("B_negative", dict(B=-1), "B"),
    ("views_0", dict(views=0), "views"),
    ("views_3", dict(views=3), "views"),
    ("flag_unknown", dict(flags=2), "flags"),
    ("flag_negative", dict(flags=-1), "flags"),
    ("null_j_rest", dict(j_rest=None), "j_rest"),
    ("null_parents", dict(parents=None), "parents"),
    ("null_per_view", dict(per_view=None), "per_view"),
    ("null_gt_body", dict(gt_body=None), "gt_body"),
    ("null_acc", dict(acc=None), "acc"),
    ("null_workspace", dict(workspace=None), "workspace"),
    ("null_gt_orient0", dict(per_view=_table(gt_orient0=None)), "gt_orient of view 0"),
    ("null_gt_orient1", dict(per_view=_table(gt_orient1=None)), "gt_orient of view 1"),
    ("null_pred_rot0", dict(per_view=_table(pred_rot0=None)), "pred_rot of view 0"),
    ("null_pred_rot1", dict(per_view=_table(pred_rot1=None)), "pred_rot of view 1"),
    ("misaligned_j_rest", dict(j_rest=FAKE + 2), "j_rest"),
    ("misaligned_gt_body", dict(gt_body=FAKE + 0x20001), "gt_body"),
    ("misaligned_pred_rot1", dict(per_view=_table(pred_rot1=FAKE + 0x7002)), "pred_rot of view 1"),
    ("misaligned_gt_trans0", dict(per_view=_table(gt_trans0=FAKE + 0x3003)), "gt_trans of view 0"),
    ("misaligned_gt_angles1", dict(per_view=_table(gt_angles1=FAKE + 0xa001)), "gt_angles of view 1"),
    ("misaligned_joint_err", dict(joint_err=FAKE + 0x21002), "joint_err"),
    ("misaligned_trans_err", dict(trans_err=FAKE + 0x22001), "trans_err"),
    ("misaligned_angle_err", dict(angle_err=FAKE + 0x23003), "angle_err"),
    ("misaligned_acc", dict(acc=FAKE + 0x24004), "acc"),
    ("misaligned_workspace", dict(workspace=FAKE + 0x25004), "workspace"),
    ("parents_root", dict(parents=_bad_parents(0, 0)), "parents[0]"),
    ("parents_self", dict(parents=_bad_parents(5, 5)), "parents[5]"),
    ("parents_forward", dict(parents=_bad_parents(3, 7)), "parents[3]"),
    ("parents_negative", dict(parents=_bad_parents(21, -1)), "parents[21]"),
    ("pred_trans_without_gt", dict(per_view=_table(gt_trans1=None), trans_err=None), "pred_trans of view 1"),
    ("gt_trans_without_pred", dict(per_view=_table(pred_trans0=None), trans_err=None), "gt_trans of view 0"),
    ("gt_angles_with_matrices", dict(flags=1, angle_err=None), "gt_angles of view 0"),
    ("trans_err_without_trans", dict(per_view=_table(gt_trans1=None, pred_trans1=None)), "trans_err"),
    ("angle_err_without_angles", dict(per_view=_table(gt_angles0=None)), "angle_err"),
]


def test_header_exports_and_binding_agree_on_the_eval_names():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_eval_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_eval_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_eval_"))
    assert declared == exported == bound == ["apg_eval_acc_doubles", "apg_eval_update", "apg_eval_workspace_bytes"]


def test_abi_numbers_stay():
    from airpose_amd import _native
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2
    assert _native.ABI_VERSION == 13
    assert not any(n.startswith("apg_") for n in _native.SIGNATURES)


def test_the_valid_argument_set_is_only_refused_for_what_a_case_changes():
    """B = 0 with the same made-up pointers succeeds (no launch), so each refusal below is due to its own change"""
    rc, msg = _call(_args(B=0))
    assert rc == 0, msg
    rc, msg = _call(_args(B=0, views=1, flags=1, per_view=_table(gt_angles0=None)[:5], angle_err=None))
    assert rc == 0, msg
    rc, msg = _call(_args(B=0, per_view=_table(gt_trans0=None, pred_trans0=None, gt_trans1=None, pred_trans1=None, gt_angles0=None,
                                               gt_angles1=None), trans_err=None, angle_err=None, joint_err=None))
    assert rc == 0, msg


@pytest.mark.parametrize("over,names", [(r[1], r[2]) for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_happen_on_the_host_and_name_the_argument(over, names):
    rc, msg = _call(_args(**over))
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("apg_eval_update: ") and names in msg, msg


def test_a_small_workspace_is_refused():
    _, L = _lib()
    rc, msg = _call(_args(B=100, workspace_bytes=L.apg_eval_workspace_bytes(100, 2) - 1))
    assert rc == ENOMEM and "workspace" in msg, (rc, msg)


def test_size_queries():
    _, L = _lib()
    assert L.apg_eval_acc_doubles() == 56
    for views in (1, 2):
        prev = 0
        for B in list(range(0, 200)) + [1000, 10 ** 6, 2 ** 31 - 1]:
            n = L.apg_eval_workspace_bytes(B, views)
            assert n > 0 and n >= prev and n % 8 == 0, (B, views, n)
            prev = n
        assert L.apg_eval_workspace_bytes(10 ** 6, views) > L.apg_eval_workspace_bytes(1, views)
    assert L.apg_eval_workspace_bytes(-1, 2) < 0
    assert L.apg_eval_workspace_bytes(4, 0) < 0 and L.apg_eval_workspace_bytes(4, 3) < 0
