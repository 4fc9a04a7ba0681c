"""CPU checks of the real-data loss's entry points (include/airpose_grad.h: apg_real_loss_*) and of RealDataLoss's construction:
header, exports and binding agree; the host-side refusals (no launch, so no GPU is needed); the size queries; the trainers'
defaults; the fp64 fold of the encoder against the literal layer chain."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from real_loss_util import encoder_chain, make_encoder

NAMES = ("apg_real_loss_workspace_bytes", "apg_real_loss_encoder_bytes", "apg_real_loss_pack_encoder", "apg_real_loss_fwd_bwd")
EINVAL, ENOMEM = -1, -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "airpose_grad.h")

# add_model_specific_args of the five copenet_real trainers, typed in from their argparse defaults and restricted to what get_loss
# reads.  hmr.py, hmr_camswap_difffl.py and spin.py read limbs2d_loss_weight and vposer_loss_weight without declaring either.
TRAINER_DEFAULTS = {
    "twoview": dict(keypoint2d_loss_weight=0.001, limbs2d_loss_weight=1.5, pose_loss_weight=1, beta_loss_weight=1, vposer_loss_weight=1),
    "twoview_sep": dict(keypoint2d_loss_weight=0.001, pose_loss_weight=1, beta_loss_weight=1, vposer_loss_weight=1),
    "hmr": dict(keypoint2d_loss_weight=0.001, beta_loss_weight=1),
    "hmr_camswap": dict(keypoint2d_loss_weight=0.001, beta_loss_weight=1),
    "spin": dict(keypoint2d_loss_weight=0.001, beta_loss_weight=1),
}
UNDECLARED = dict(limbs2d_loss_weight=1.5, vposer_loss_weight=1.0)


def _lib():
    from airpose_amd import _native_grad as G
    return G, G.lib()


def test_header_exports_and_table_agree():
    G, L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], check=True, capture_output=True, text=True).stdout
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(apg_real_loss_\w+)\(", text, re.M))
    assert declared == set(NAMES)
    assert {n for n in G.SIGNATURES if n.startswith("apg_real_loss_")} == set(NAMES)
    assert set(re.findall(r" T (apg_real_loss_\w+)\n", syms)) == set(NAMES)
    for n in NAMES:
        assert getattr(L, n).argtypes == G.SIGNATURES[n][1] and getattr(L, n).restype is G.SIGNATURES[n][0]
        proto = re.search(r"^(?:int|int64_t)\s+%s\((.*?)\);" % n, text, re.M | re.S).group(1)
        nargs = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert nargs == len(G.SIGNATURES[n][1]), n
    assert re.search(r"#define APG_ABI_VERSION 2\b", text)
    assert G.ABI_VERSION == 2 and L.apg_abi_version() == 2        # additive under ABI 2


def test_size_queries():
    _, L = _lib()
    q = L.apg_real_loss_workspace_bytes
    assert q(0) < 0 and q(-1) < 0 and q(2 ** 30 + 1) < 0 and q(2 ** 31 - 1) < 0
    assert q(1) > 0 and q(2 ** 30) > 0
    sizes = [q(B) for B in (1, 2, 3, 33, 64, 256, 257)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    assert q(64) >= 2 * 64 * 6 * 4                                # six partial sums per (view, body) row
    e = L.apg_real_loss_encoder_bytes()
    assert e >= 4 * (512 * 63 + 512 + 64 * 512 + 64) and e < 2 ** 20


FAKE = 0x100000                                                   # made-up pointers, 16 MB apart: nothing here is ever read


def _call(L, nviews=2, cross=12, B=2, J=22, Jg=22, col=2, gain=1.0, weights=True, enc=True, pred=True, gt=True, terms=True, grads=None,
          ws=True, ws_bytes=None, null_pred=(), null_gt=(), terms_at=None):
    """apg_real_loss_fwd_bwd with made-up non-NULL pointers: every case here is refused before anything is read or launched"""
    w = (ctypes.c_float * 6)(*([1.0] * 6))
    nv = max(1, min(2, nviews))
    addr = lambda k: FAKE + (k << 24)
    P = (ctypes.c_void_p * (4 * nv))(*[None if k in null_pred else addr(k) for k in range(4 * nv)])
    Gt = (ctypes.c_void_p * (2 * nv))(*[None if k in null_gt else addr(8 + k) for k in range(2 * nv)])
    if ws_bytes is None:
        ws_bytes = max(0, L.apg_real_loss_workspace_bytes(B))
    return L.apg_real_loss_fwd_bwd(nviews, cross, B, J, Jg, col, gain, w if weights else None, ctypes.c_void_p(addr(12)) if enc else None,
                                   P if pred else None, Gt if gt else None,
                                   ctypes.c_void_p(addr(13) if terms_at is None else terms_at) if terms else None, grads,
                                   ctypes.c_void_p(addr(14)) if ws else None, ws_bytes, None)


@pytest.mark.parametrize("what,kw,word", [
    ("B < 1", dict(B=0), "B"), ("J < 22", dict(J=21), "J"), ("Jg < 22", dict(Jg=21), "Jg"),
    ("nviews = 0", dict(nviews=0, cross=0), "nviews"), ("nviews = 3", dict(nviews=3), "nviews"),
    ("cross bits with one view", dict(nviews=1, cross=4), "cross"), ("cross bits of the synthetic loss", dict(cross=15), "cross"),
    ("col = -1", dict(col=-1), "depth_col"), ("col = 3", dict(col=3), "depth_col"),
    ("weights NULL", dict(weights=False), "weights"), ("encoder NULL", dict(enc=False), "encoder"), ("pred NULL", dict(pred=False), "pred"),
    ("gt NULL", dict(gt=False), "gt"), ("terms NULL", dict(terms=False), "terms"), ("workspace NULL", dict(ws=False), "workspace"),
    ("rotmat of view 0 NULL", dict(null_pred=(0,)), "rotmat of view 0"), ("betas of view 1 NULL", dict(null_pred=(5,)), "betas of view 1"),
    ("j2d of view 0 NULL", dict(null_pred=(2,)), "j2d of view 0"), ("depth of view 1 NULL", dict(null_pred=(7,)), "depth of view 1"),
    ("gt of view 1 NULL", dict(null_gt=(2,)), "gt of view 1"), ("eps of view 0 NULL", dict(null_gt=(1,)), "eps of view 0"),
])
def test_host_side_refusals(what, kw, word):
    _, L = _lib()
    assert _call(L, **kw) == EINVAL, what
    msg = L.apg_last_error().decode()
    assert "apg_real_loss_fwd_bwd" in msg and word in msg, (what, msg)


def test_small_workspace_is_enomem():
    _, L = _lib()
    need = L.apg_real_loss_workspace_bytes(2)
    assert _call(L, ws_bytes=need - 1) == ENOMEM
    msg = L.apg_last_error()
    assert b"apg_real_loss_fwd_bwd" in msg and b"workspace" in msg and str(need).encode() in msg


def test_an_output_overlapping_an_input_is_refused():
    _, L = _lib()
    addr = lambda k: FAKE + (k << 24)
    assert _call(L, terms_at=addr(1) + 8) == EINVAL                        # terms inside betas of view 0
    msg = L.apg_last_error().decode()
    assert "terms" in msg and "overlaps" in msg, msg
    grads = (ctypes.c_void_p * 8)(*([None] * 8))
    grads[2] = addr(10) + 4 * 31                                           # g_j2d of view 0 starts inside gt of view 1
    assert _call(L, grads=grads) == EINVAL
    msg = L.apg_last_error().decode()
    assert "j2d" in msg and "overlaps" in msg, msg
    grads[2] = addr(0)                                                     # a gradient written over its own input
    assert _call(L, grads=grads) == EINVAL


def test_pack_encoder_refusals():
    _, L = _lib()
    p = ctypes.c_void_p(FAKE)
    need = L.apg_real_loss_encoder_bytes()
    for k, name in enumerate(("W1", "b1", "W2", "b2", "packed")):
        a = [p] * 5
        a[k] = None
        assert L.apg_real_loss_pack_encoder(*a, need, None) == EINVAL
        assert name in L.apg_last_error().decode()
    assert L.apg_real_loss_pack_encoder(p, p, p, p, p, need - 1, None) == ENOMEM
    assert b"packed" in L.apg_last_error()


@pytest.mark.parametrize("kind", sorted(TRAINER_DEFAULTS))
def test_defaults_are_the_trainers(kind):
    import airpose_amd
    from airpose_amd import loss_real
    sd = make_encoder()
    extra = UNDECLARED if kind in ("hmr", "hmr_camswap", "spin") else {}
    m = airpose_amd.RealDataLoss(kind, sd, **extra)
    assert isinstance(m, loss_real.RealDataLoss) and not list(m.parameters())
    d = dict(TRAINER_DEFAULTS[kind], **extra)
    assert m.weights == {k: float(v) for k, v in d.items()}
    assert m.weight_vector() == [d["keypoint2d_loss_weight"], d["beta_loss_weight"], d["vposer_loss_weight"], d.get("pose_loss_weight", 0.0),
                                 d.get("limbs2d_loss_weight", 1.0), 60.0]
    assert loss_real.RealDataLoss(kind, sd, **dict(extra, beta_loss_weight=7)).weights["beta_loss_weight"] == 7.0
    if extra:                                                              # read by the trainer, declared nowhere: no default here either
        for n in extra:
            with pytest.raises(ValueError, match=n):
                loss_real.RealDataLoss(kind, sd, **{k: v for k, v in extra.items() if k != n})
    with pytest.raises(ValueError, match="shape_loss_weight"):
        loss_real.RealDataLoss(kind, sd, shape_loss_weight=1.0, **extra)
    assert loss_real.TERM_NAMES == ("loss", "loss_regul_vposer", "loss_regr_pose", "loss_keypoints", "loss_regul_betas", "loss_depth")


def test_twoview_sep_has_no_limb_weight():
    from airpose_amd.loss_real import RealDataLoss
    with pytest.raises(ValueError, match="limbs2d_loss_weight"):
        RealDataLoss("twoview_sep", make_encoder(), limbs2d_loss_weight=1.5)


def test_unknown_kind_and_missing_key_are_refused_by_name():
    from airpose_amd.loss_real import ENCODER_KEYS, RealDataLoss
    with pytest.raises(ValueError, match="threeview"):
        RealDataLoss("threeview", make_encoder())
    sd = make_encoder()
    assert set(ENCODER_KEYS) <= set(sd)
    for k in ("encoder_net.4.running_var", "encoder_net.8.logvar.bias"):
        bad = dict(sd)
        del bad[k]
        with pytest.raises(KeyError, match=re.escape(k)):
            RealDataLoss("twoview", bad)
    bad = dict(sd)
    bad["encoder_net.2.weight"] = bad["encoder_net.2.weight"].t()
    with pytest.raises(ValueError, match=re.escape("encoder_net.2.weight")):
        RealDataLoss("twoview", bad)


def test_predictions_on_the_cpu_are_refused():
    from airpose_amd.loss_real import RealDataLoss
    m = RealDataLoss("spin", make_encoder(), **UNDECLARED)
    B = 2
    batch = {"smpl_joints_2d_crop0": torch.rand(B, 1, 24, 3)}
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(batch, torch.rand(B, 3), torch.rand(B, 22, 3, 3), torch.rand(B, 10), None, torch.rand(B, 25, 2))
    with pytest.raises(RuntimeError, match="5 predictions"):
        m(batch, torch.rand(B, 3), torch.rand(B, 22, 3, 3))


@pytest.mark.parametrize("prefix", ["", "vp_model."])
def test_fp64_fold_reproduces_the_layer_chain(prefix):
    from airpose_amd.loss_real import fold_encoder
    sd = make_encoder(3)
    W1, b1, W2, b2 = fold_encoder({prefix + k: v for k, v in sd.items()})
    assert W1.dtype == torch.float64 and W1.shape == (512, 63) and b1.shape == (512,) and W2.shape == (64, 512) and b2.shape == (64,)
    g = torch.Generator().manual_seed(11)
    aa = torch.randn(37, 63, generator=g, dtype=torch.float64) * 1.5
    sd64 = {k: v.double() for k, v in sd.items()}
    mu, s = encoder_chain(sd64, aa)
    out = torch.nn.functional.leaky_relu(aa @ W1.t() + b1, 0.01) @ W2.t() + b2
    want = torch.cat([mu, s], 1)
    err = float((out - want).abs().max() / want.abs().max())
    print("fold against the layer chain: max-norm relative error %.3e" % err)
    assert err <= 1e-12
    # the fold is what eval mode computes: a wrong eps is seen
    mu2, _ = encoder_chain(sd64, aa, bn_eps=1e-3)
    assert float((mu2 - mu).abs().max() / mu.abs().max()) > 1e-6
