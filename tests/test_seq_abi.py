"""CPU checks of the apg_seq_* entry points of libairpose_grad.so (airpose_amd/csrc/seq_fit.hip) and of airpose_amd.AirPosePlusSequence
without a GPU: declared == exported == bound, the two ABI numbers stay where they are, every refusal happens on the host -- the
pointers below are made-up addresses that are never dereferenced (there is no GPU here), the result is APG_EINVAL and the message
starts with the entry's name and names the argument -- the class is exported, constructed and refuses by name, and the window
arithmetic."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
EINVAL = -1
FAKE = 0x7f0000001000                                    # 4096-aligned and never touched
NAMES = ["apg_seq_export", "apg_seq_init"]
INIT_PTRS = ("angles0", "angles1", "trans0", "trans1", "det", "W1", "b1", "Wmu", "bmu", "z", "phi", "tau", "j2d", "robust")
EXPORT_PTRS = ("z", "phi", "tau", "w1", "b1", "w2", "b2", "w3", "b3", "thetas", "root_rot", "smpl_wrt_cam", "cam1_wrt_cam0")
ALIGN16 = {"apg_seq_init": ("Wmu",), "apg_seq_export": ("w1", "w2", "w3")}


def _lib():
    from airpose_amd import _native_grad as G
    if not os.path.isfile(G.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return G, G.lib()


def _args(entry, **over):
    """a valid argument set on made-up addresses; `over` replaces entries"""
    names = INIT_PTRS if entry == "apg_seq_init" else EXPORT_PTRS
    a = dict(L=9, agreement_px=100.0, robust_conf=14.0)
    a.update({n: FAKE + 0x100000 * (k + 1) for k, n in enumerate(names)})
    a.update(over)
    return a


def _call(entry, a):
    _, L = _lib()
    vp = ctypes.c_void_p
    if entry == "apg_seq_init":
        rc = L.apg_seq_init(a["L"], *[vp(a[n]) for n in INIT_PTRS[:9]], a["agreement_px"], a["robust_conf"],
                            *[vp(a[n]) for n in INIT_PTRS[9:]], None)
    else:
        rc = L.apg_seq_export(a["L"], *[vp(a[n]) for n in EXPORT_PTRS], None)
    return rc, L.apg_last_error().decode()


def _refusals(entry, names):
    out = [("L_zero", dict(L=0), "L"), ("L_negative", dict(L=-5), "L"), ("L_too_long", dict(L=(1 << 22) + 1), "L")]
    for n in names:
        out.append(("null_" + n, {n: None}, n + " is NULL"))
        out.append(("misaligned_" + n, {n: FAKE + 0x900002}, n + " is not"))
    for n in ALIGN16[entry]:
        out.append(("align4_only_" + n, {n: FAKE + 0x900004}, n + " is not 16-byte aligned"))
    if entry == "apg_seq_init":
        out += [("agreement_negative", dict(agreement_px=-1.0), "agreement_px"), ("agreement_nan", dict(agreement_px=float("nan")), "agreement_px"),
                ("agreement_inf", dict(agreement_px=float("inf")), "agreement_px"), ("robust_conf_nan", dict(robust_conf=float("nan")), "robust_conf"),
                ("robust_conf_inf", dict(robust_conf=float("-inf")), "robust_conf"), ("j2d_is_det", dict(j2d=FAKE + 0x100000 * 5), "j2d must not be det")]
    return [(entry, i, o, m) for i, o, m in out]


REFUSALS = _refusals("apg_seq_init", INIT_PTRS) + _refusals("apg_seq_export", EXPORT_PTRS)


def test_header_exports_and_binding_agree_on_the_seq_names():
    G, _ = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(apg_seq_[a-z0-9_]+)\s*\(", src)))
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\s[TW]\s+(apg_seq_[a-z0-9_]+)$", syms, flags=re.M)))
    bound = sorted(n for n in G.SIGNATURES if n.startswith("apg_seq_"))
    assert declared == exported == bound == NAMES
    for name, n in (("apg_seq_init", 18), ("apg_seq_export", 15)):
        decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(G.SIGNATURES[name][1]) == n
    assert int(re.search(r"#define\s+APG_SEQ_ROWS\s+(\d+)", open(HEADER).read()).group(1)) == G.SEQ_ROWS


def test_header_documents_the_conventions():
    text = open(HEADER).read()
    at = text.index("AirPose+ on a whole sequence (seq_fit.hip)")
    doc = text[at:text.index("#define APG_SEQ_ROWS", at)]
    for phrase in ("first two ROWS", "1/2 - t^2 / 48", "identity exactly", "BOTH detectors", "(strict)", "detector 1 AlphaPose",
                   "view 0 joint 0 .. 23, view 1 joint 0 .. 23", "[R^T | -R^T t]", "Additive under ABI 2", "bit-identical"):
        assert phrase in doc, phrase


def test_abi_numbers_stay():
    from airpose_amd import _native
    G, L = _lib()
    assert int(re.search(r"#define\s+APG_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2
    assert _native.ABI_VERSION == 13
    assert not any(n.startswith("apg_") for n in _native.SIGNATURES)


@pytest.mark.parametrize("entry,over,names", [r[0:1] + r[2:] for r in REFUSALS], ids=["%s-%s" % (r[0][8:], r[1]) for r in REFUSALS])
def test_refusals_happen_on_the_host_and_name_the_argument(entry, over, names):
    rc, msg = _call(entry, _args(entry, **over))
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith(entry + ": ") and names in msg[len(entry) + 2:], msg


# ------------------------------------------------------------------------------------------------ the Python class, no GPU
def _vposer():
    import seq_util as U
    return U.state_dict(U.export_case(3, "body")[0])


class _Body(object):
    num_verts = 10475


def test_class_is_exported_and_constructed_without_a_gpu():
    import airpose_amd
    from airpose_amd import sequence
    assert airpose_amd.AirPosePlusSequence is sequence.AirPosePlusSequence
    sd = _vposer()
    s = airpose_amd.AirPosePlusSequence(sd, _Body(), device="cuda:0")
    assert s.chunk == 2000 and s.device == torch.device("cuda", 0)
    assert airpose_amd.AirPosePlusSequence({"vp_model." + k: v for k, v in sd.items()}, _Body(), device="cuda:0", chunk=7).chunk == 7
    assert [tuple(t.shape) for t in s._enc_host] == [(512, 63), (512,), (32, 512), (32,)] and all(t.dtype == torch.float32 for t in s._enc_host)
    with pytest.raises(RuntimeError, match="no CPU path"):
        airpose_amd.AirPosePlusSequence(sd, _Body(), device="cpu")
    with pytest.raises(ValueError, match="chunk"):
        airpose_amd.AirPosePlusSequence(sd, _Body(), device="cuda:0", chunk=0)


@pytest.mark.parametrize("key", ["decoder_net.3.weight", "decoder_net.5.bias", "encoder_net.8.mu.weight", "encoder_net.1.running_var"])
def test_constructor_refuses_the_state_dict_by_name(key):
    from airpose_amd import AirPosePlusSequence
    sd = _vposer()
    with pytest.raises(KeyError, match=re.escape(key)):
        AirPosePlusSequence({k: v for k, v in sd.items() if k != key}, _Body(), device="cuda:0")
    bad = dict(sd)
    bad[key] = torch.zeros(tuple(sd[key].shape) + (2,))
    with pytest.raises(ValueError, match=re.escape(key)):
        AirPosePlusSequence(bad, _Body(), device="cuda:0")


def test_class_refuses_by_name():
    from airpose_amd import AirPosePlusSequence
    s = AirPosePlusSequence(_vposer(), _Body(), device="cuda:0", chunk=4)
    L = 5
    pred = {"pred_angles0": torch.zeros(L, 22, 3), "pred_angles1": torch.zeros(L, 22, 3), "pred_smpltrans0": torch.zeros(L, 3),
            "pred_smpltrans1": torch.zeros(L, 3), "pred_betas0": torch.zeros(L, 10)}
    det = torch.zeros(2, L, 2, 24, 3)
    with pytest.raises(RuntimeError, match="pred has no 'pred_smpltrans1'"):
        s.prepare({k: v for k, v in pred.items() if k != "pred_smpltrans1"}, det)
    with pytest.raises(RuntimeError, match="pred_angles0 lives on cpu"):
        s.prepare(pred, det)
    # (a tensor's type and shape are looked at before its device, so these refusals are reachable without a GPU)
    with pytest.raises(RuntimeError, match=r"detections must be \(2, 5, 2, 24, 3\), got \(2, 5, 2, 25, 3\)"):
        s.prepare(pred, torch.zeros(2, L, 2, 25, 3))
    with pytest.raises(RuntimeError, match=r"pred_angles1 must be \(5, 22, 3\), got \(5, 21, 3\)"):
        s.prepare(dict(pred, pred_angles1=torch.zeros(L, 21, 3)), det)
    with pytest.raises(RuntimeError, match=r"pred_smpltrans0 must be \(5, 3\), got \(4, 3\)"):
        s.prepare(dict(pred, pred_smpltrans0=torch.zeros(4, 3)), det)
    with pytest.raises(RuntimeError, match="pred_angles1 must be a floating-point tensor, got torch.int64"):
        s.prepare(dict(pred, pred_angles1=torch.zeros(L, 22, 3, dtype=torch.int64)), det)
    with pytest.raises(RuntimeError, match="pred_smpltrans1 must be a tensor, got list"):
        s.prepare(dict(pred, pred_smpltrans1=[1.0]), det)
    state = {"z": torch.zeros(L, 32), "phi0": torch.zeros(L, 6), "phi1": torch.zeros(L, 6), "tau0": torch.zeros(L, 3), "tau1": torch.zeros(L, 3)}
    data = {"j2d": det, "robust": torch.ones(L, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="state has no 'phi1'"):
        s.fit({k: v for k, v in state.items() if k != "phi1"}, data, torch.zeros(2, 4))
    with pytest.raises(TypeError, match="unknown argument 'sigma2d'"):
        s.fit(state, data, torch.zeros(2, 4), sigma2d=40.0)
    with pytest.raises(RuntimeError, match="z lives on cpu"):
        s.fit(state, data, torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match=r"tau1 must be \(5, 3\), got \(5, 4\)"):
        s.fit(dict(state, tau1=torch.zeros(L, 4)), data, torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="result has no 'chunks'"):
        s.export(dict(state, beta=torch.zeros(2, 10)))
    with pytest.raises(RuntimeError, match="z lives on cpu"):
        s.export(dict(state, beta=torch.zeros(2, 10), chunks=[(0, 4), (4, 5)]))


@pytest.mark.parametrize("L,want", [(1, [(0, 1)]), (1999, [(0, 1999)]), (2000, [(0, 2000)]), (2001, [(0, 2000), (2000, 2001)]),
                                    (6990, [(0, 2000), (2000, 4000), (4000, 6000), (6000, 6990)])])
def test_window_arithmetic(L, want):
    from airpose_amd.sequence import windows
    assert windows(L, 2000) == want
    got = windows(L, 7)
    assert got[0][0] == 0 and got[-1][1] == L and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert all(0 < b - a <= 7 for a, b in got) and all(b - a == 7 for a, b in got[:-1]) and len(got) == -(-L // 7)
    with pytest.raises(ValueError, match="at least one frame"):
        windows(0, 2000)
