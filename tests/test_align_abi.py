"""CPU checks of the apg_align_* entry points of libairpose_grad.so (airpose_amd/csrc/eval_align.hip): declared == exported ==
bound, the header documents the accumulator, the two ABI numbers stay where they are, and every refusal happens on the host -- the
pointers below are made-up addresses that are never dereferenced (there is no GPU here), the result is APG_EINVAL (APG_ENOMEM for
the workspace's size, as in every other entry) and the message names the argument."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL, ENOMEM = -1, -4
FAKE = 0x7f0000001000                                    # 4096-aligned and never touched
NAMES = ["apg_align_acc_doubles", "apg_align_update", "apg_align_workspace_bytes"]


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _table(**entries):
    """the eight per-view pointers with entries (name + view, e.g. gt_root1) replaced"""
    names = ("pred", "gt", "pred_root", "gt_root")
    t = [FAKE + 0x100000 * (k + 1) for k in range(8)]
    for k, val in entries.items():
        t[int(k[-1]) * 4 + names.index(k[:-1])] = val
    return t


def _args(**over):
    """a valid argument set of apg_align_update on made-up addresses; `over` replaces entries"""
    a = dict(B=4, views=2, N=22, pred_stride=66, gt_stride=66, pred_root_stride=3, gt_root_stride=3, per_view=_table(),
             err=FAKE + 0x21000, transform=FAKE + 0x22000, acc=FAKE + 0x24000, workspace=FAKE + 0x25000, workspace_bytes=1 << 20)
    a.update(over)
    return a


def _call(a):
    _, L = _lib()
    vp = ctypes.c_void_p
    table = None if a["per_view"] is None else (ctypes.c_void_p * len(a["per_view"]))(*a["per_view"])
    rc = L.apg_align_update(a["B"], a["views"], a["N"], a["pred_stride"], a["gt_stride"], a["pred_root_stride"], a["gt_root_stride"],
                            table, vp(a["err"]), vp(a["transform"]), vp(a["acc"]), vp(a["workspace"]), a["workspace_bytes"], None)
    return rc, L.apg_last_error().decode()


REFUSALS = [
    ("B_zero", dict(B=0), "B"),
    ("B_negative", dict(B=-1), "B"),
    ("N_zero", dict(N=0), "N"),
    ("N_negative", dict(N=-3), "N"),
    ("views_0", dict(views=0), "views"),
    ("views_3", dict(views=3), "views"),
    ("pred_stride_short", dict(pred_stride=65), "pred_stride"),
    ("gt_stride_short", dict(gt_stride=3), "gt_stride"),
    ("pred_root_stride_short", dict(pred_root_stride=2), "pred_root_stride"),
    ("gt_root_stride_short", dict(gt_root_stride=0), "gt_root_stride"),
    ("null_per_view", dict(per_view=None), "per_view"),
    ("null_acc", dict(acc=None), "acc"),
    ("null_workspace", dict(workspace=None), "workspace"),
    ("null_pred0", dict(per_view=_table(pred0=None)), "pred of view 0"),
    ("null_pred1", dict(per_view=_table(pred1=None)), "pred of view 1"),
    ("null_gt0", dict(per_view=_table(gt0=None)), "gt of view 0"),
    ("null_gt1", dict(per_view=_table(gt1=None)), "gt of view 1"),
    ("pred_root_without_gt_root", dict(per_view=_table(gt_root0=None)), "pred_root of view 0 is given without gt_root"),
    ("gt_root_without_pred_root", dict(per_view=_table(pred_root1=None)), "gt_root of view 1 is given without pred_root"),
    ("misaligned_pred0", dict(per_view=_table(pred0=FAKE + 2)), "pred of view 0"),
    ("misaligned_gt1", dict(per_view=_table(gt1=FAKE + 0x600001)), "gt of view 1"),
    ("misaligned_pred_root1", dict(per_view=_table(pred_root1=FAKE + 0x700003)), "pred_root of view 1"),
    ("misaligned_err", dict(err=FAKE + 0x21002), "err"),
    ("misaligned_transform", dict(transform=FAKE + 0x22001), "transform"),
    ("misaligned_acc", dict(acc=FAKE + 0x24004), "acc"),
    ("misaligned_workspace", dict(workspace=FAKE + 0x25004), "workspace"),
]


def test_header_exports_and_binding_agree_on_the_align_names():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_align_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_align_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_align_"))
    assert declared == exported == bound == NAMES
    decl = re.search(r"int apg_align_update\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(G.SIGNATURES["apg_align_update"][1]) == 14
    assert len(G.SIGNATURES["apg_align_workspace_bytes"][1]) == 3 and G.SIGNATURES["apg_align_acc_doubles"][1] == []


def test_header_documents_the_accumulator_and_the_degenerate_rule():
    text = open(HEADER).read()
    at = text.index("Mesh metrics (eval_align.hip)")
    doc = text[at:text.index("int64_t apg_align_workspace_bytes", at)]
    for phrase in ("[0] samples", "[1] sum of abs", "[2] sum of root", "[3] sum of pa", "[4] samples that had roots", "ADDED to",
                   "det R = +1", "s = 0, R = I", "sign(det U det V)", "Additive under ABI 2"):
        assert phrase in doc, phrase
    assert int(re.search(r"#define\s+APG_ALIGN_ACC_PER_VIEW\s+(\d+)", text).group(1)) == 5
    assert int(re.search(r"#define\s+APG_ALIGN_PER_VIEW\s+(\d+)", text).group(1)) == 4


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
    assert msg.startswith("apg_align_update: ") and names in msg[len("apg_align_update: "):], msg


def test_only_the_changed_argument_is_what_a_refusal_is_about():
    """the valid set differs from each refusal in one entry; its own size checks pass up to the launch, which this machine cannot
    make -- so the valid set is checked through the one refusal that comes last, the workspace's size"""
    _, L = _lib()
    need = L.apg_align_workspace_bytes(4, 2, 22)
    rc, msg = _call(_args(workspace_bytes=need - 1))
    assert rc == ENOMEM and "workspace" in msg and str(need) in msg, (rc, msg)
    rc, msg = _call(_args(workspace_bytes=need // 2 - 1, views=1, per_view=_table(pred_root0=None, gt_root0=None)[:4], err=None, transform=None,
                          pred_root_stride=0, gt_root_stride=0))          # no roots: their strides are not looked at
    assert rc == ENOMEM, (rc, msg)
    rc, msg = _call(_args(workspace_bytes=need - 1, pred_stride=1000, gt_stride=67, pred_root_stride=66, gt_root_stride=1000))
    assert rc == ENOMEM, (rc, msg)


def test_size_queries():
    _, L = _lib()
    assert L.apg_align_acc_doubles() == 10
    for views in (1, 2):
        for B in (1, 2, 30, 256, 1 << 22):
            for N in (1, 22, 10475, 1 << 24):
                assert L.apg_align_workspace_bytes(B, views, N) == B * views * 24
    for bad in ((0, 2, 22), (-1, 1, 22), (4, 0, 22), (4, 3, 22), (4, 2, 0), (4, 2, -1), ((1 << 22) + 1, 1, 22), (4, 1, (1 << 24) + 1)):
        assert L.apg_align_workspace_bytes(*bad) < 0, bad


# ------------------------------------------------------------------------------------------------ the Python class, no GPU
def _dicts(B=3, J=25, V=40, n=22):
    import torch
    out = {"pred_j3d_cam0": torch.zeros(B, J, 3), "pred_j3d_cam1": torch.zeros(B, J, 3),
           "pred_vertices_cam0": torch.zeros(B, V, 3), "pred_vertices_cam1": torch.zeros(B, V, 3)}
    batch = {"smpl_joints_rel0": torch.zeros(B, 1, n, 3), "smpl_joints_rel1": torch.zeros(B, 1, n, 3),
             "smpl_vertices_rel0": torch.zeros(B, 1, V, 3), "smpl_vertices_rel1": torch.zeros(B, V, 3)}
    return out, batch


def test_class_is_exported_and_constructed_without_a_gpu():
    import airpose_amd
    from airpose_amd import mesh_metrics
    assert airpose_amd.MeshMetrics is mesh_metrics.MeshMetrics
    m = airpose_amd.MeshMetrics(kind="muhmr", device="cuda:0")
    assert m.views == 2 and m.n_joints == 22
    assert airpose_amd.MeshMetrics(kind="hmr", n_joints=14, device="cuda:0").views == 1
    with pytest.raises(ValueError, match="kind"):
        airpose_amd.MeshMetrics(kind="spin")
    with pytest.raises(ValueError, match="n_joints"):
        airpose_amd.MeshMetrics(n_joints=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        airpose_amd.MeshMetrics(device="cpu")
    assert m.compute()["count"] == 0 and "pve_abs0" not in m.compute()


def test_class_refuses_by_name():
    import torch
    from airpose_amd import MeshMetrics
    m = MeshMetrics(kind="twoview", device="cuda:0")
    out, batch = _dicts()

    def without(*keys, **repl):
        d = {k: t for k, t in list(out.items()) + list(batch.items()) if k not in keys}
        d.update(repl)
        return d
    got = m.gather(out, batch)
    assert got[1]["pred_vertices"][1] is out["pred_vertices_cam1"] and got[0]["gt_joints"][1] is batch["smpl_joints_rel0"]
    assert m.gather(without("pred_vertices_cam0", "pred_vertices_cam1", "smpl_vertices_rel0", "smpl_vertices_rel1"))[0]["gt_vertices"] is None
    with pytest.raises(RuntimeError, match="pred_j3d_cam1"):
        m.update(without("pred_j3d_cam1"))
    with pytest.raises(RuntimeError, match="smpl_joints_rel0"):
        m.update(out, {k: t for k, t in batch.items() if k != "smpl_joints_rel0"})
    with pytest.raises(RuntimeError, match="pred_vertices_cam0 is given without smpl_vertices_rel0"):
        m.update(without("smpl_vertices_rel0"))
    with pytest.raises(RuntimeError, match="smpl_vertices_rel1 is given without pred_vertices_cam1"):
        m.update(without("pred_vertices_cam1"))
    with pytest.raises(RuntimeError, match="pred_vertices_cam0 is given for one view only .pred_vertices_cam1 is missing"):
        m.update(without("pred_vertices_cam1", "smpl_vertices_rel1"))
    with pytest.raises(RuntimeError, match="pred_j3d_cam0 must be a tensor"):
        m.update(without(pred_j3d_cam0=[1.0]))
    with pytest.raises(RuntimeError, match=r"pred_j3d_cam1 must be \(3, at least 22, 3\), got \(3, 21, 3\)"):
        m.update(without(pred_j3d_cam1=torch.zeros(3, 21, 3)))
    with pytest.raises(RuntimeError, match=r"smpl_joints_rel1 must be \(3, at least 22, 3\), got \(2, 1, 22, 3\)"):
        m.update(without(smpl_joints_rel1=torch.zeros(2, 1, 22, 3)))
    with pytest.raises(RuntimeError, match=r"smpl_vertices_rel1 must be \(3, 40, 3\), got \(3, 41, 3\)"):
        m.update(without(smpl_vertices_rel1=torch.zeros(3, 41, 3)))
    with pytest.raises(RuntimeError, match=r"pred_vertices_cam1 must be \(3, 40, 3\), got \(3, 40, 2\)"):
        m.update(without(pred_vertices_cam1=torch.zeros(3, 40, 2)))
    with pytest.raises(RuntimeError, match="smpl_vertices_rel0 must be a floating-point tensor, got torch.int32"):
        m.update(without(smpl_vertices_rel0=torch.zeros(3, 1, 40, 3, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="pred_j3d_cam0 lives on cpu"):                    # the first tensor looked at
        m.update(out, batch)
    # one-view kinds read the names without an index, or with 0
    s = MeshMetrics(kind="singleview", device="cuda:0")
    with pytest.raises(RuntimeError, match="pred_j3d_cam / pred_j3d_cam0"):
        s.update({"smpl_joints_rel": batch["smpl_joints_rel0"]})
    assert s.gather({"pred_j3d_cam": out["pred_j3d_cam0"]}, {"smpl_joints_rel0": batch["smpl_joints_rel0"]})[0]["gt_joints"][0] == "smpl_joints_rel0"


def test_state_round_trip_without_a_gpu():
    import torch
    from airpose_amd import MeshMetrics
    from airpose_amd.mesh_metrics import summarise
    m = MeshMetrics(kind="twoview", device="cuda:0")
    acc = torch.zeros(2, 2, 5, dtype=torch.float64)
    acc[0, :, 0], acc[0, :, 4] = 4, 4
    acc[0, 0, 1:4] = torch.tensor([0.4, 0.2, 0.1], dtype=torch.float64)
    acc[0, 1, 1:4] = torch.tensor([0.8, 0.6, 0.3], dtype=torch.float64)
    m.load_state({"kind": "twoview", "n_joints": 22, "acc": acc})
    got = m.compute()
    assert got == summarise(acc, 2) and got["count"] == 4 and "pve_abs0" not in got
    assert got["mpjpe_abs0"] == 0.4 / 4 and got["mpjpe_root1"] == 0.6 / 4 and got["pa_mpjpe1"] == 0.3 / 4
    assert torch.equal(m.state()["acc"], acc)
    with pytest.raises(RuntimeError, match="kind"):
        m.load_state({"kind": "hmr", "acc": acc})
    with pytest.raises(RuntimeError, match="joints"):
        m.load_state({"kind": "twoview", "n_joints": 14, "acc": acc})
    with pytest.raises(RuntimeError, match=r"\(2, 2, 5\) float64"):
        m.load_state({"acc": acc.float()})
    m.reset()
    assert m.compute()["count"] == 0
