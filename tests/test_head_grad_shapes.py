"""The IEF head's kernels through the C ABI (apg_head_fwd / apg_head_bwd, head_grad.hip) against an fp64 restatement at the row
counts, workspace layouts, NULL patterns, strides and dropout rates where they can go wrong without tests/test_head_grad.py
noticing (its bar is one number per tensor, 1e-4, at R = 2, 10, 128 rows with every output requested).

Every case: fp32 inputs, the same operation in fp64 on the same fp32 values with the masks of apg_dropout_mask
(test_head_grad._ref_reg, restated here so that xc, h1d and h2d are returned too, and held against it), outputs inside
NaN-filled arenas, two identical calls compared with torch.equal, and per tensor the two bars of test_trunk_grad_shapes.py:
  - rel_err <= 1e-5;
  - element-wise |got - ref| <= 1e-5 A, exactly 0 where A == 0.
A: the head is linear with no subtractions, so A is the same restatement with the same masks on the absolute values of every
input, weight, bias and output gradient; its outputs and autograd gradients bound every term of every element.
xc is a copy and must match bit for bit.

Cases: B in {1, 2, 31, 32, 33, 64, 65, 100, 257} (R = 2B on each side of the 64-row tile, of 128 rows and of the 32-row
column-sum chunk, up to 17 chunks; K = R off multiples of 4 and 16 in the weight-gradient products), each in both workspace
layouts (need_gxf = 1, and need_gxf = 0 on exactly apg_head_bwd_workspace_bytes(B, 0) bytes); a workspace one byte short;
NULL g_out / g_param / g_in patterns; state inputs with row stride 0 and 135; (p1, p2) in {(0, 0), (0.5, 0.5), (0.1, 0.7),
(0, 0.5)}.  Nothing of the issue's list was trimmed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from grad_shapes_util import Arena, check, report
from test_head_grad import PNAMES, _ref_reg

pytestmark = pytest.mark.gpu
APG_ENOMEM = -4
STATE = (("bb", 3), ("pos", 3), ("orient", 6), ("art", 126), ("shape", 10))
PSHAPES = ((1024, 2332), (1024,), (1024, 1024), (1024,), (135, 1024), (135,), (10, 1024), (10,))
GIN = ["g_%s%d" % (n, v) for v in (0, 1) for n in ("xf",) + tuple(n for n, _ in STATE)]          # the order of apg_head_bwd's g_in
GPAR = ["g_" + n for n in PNAMES]
ALL_OUT = (True,) * 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def params(copenet_sd):
    """the eight head parameters of the synthetic checkpoint, fp32"""
    return [copenet_sd[n].detach().float().contiguous() for n in PNAMES]


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"xf0": torch.relu(torch.randn(B, 2048, generator=g)), "xf1": torch.relu(torch.randn(B, 2048, generator=g))}
    for v in "01":
        d["bb" + v] = torch.rand(B, 3, generator=g) + 0.2
        d["pos" + v] = torch.randn(B, 3, generator=g) * 0.3 + torch.tensor([0., 0., 10.])
        d["orient" + v] = torch.randn(B, 6, generator=g)
        d["art" + v] = torch.randn(B, 126, generator=g)
        d["shape" + v] = torch.randn(B, 10, generator=g) * 0.5
    gout = [torch.randn(B, 135, generator=g), torch.randn(B, 10, generator=g), torch.randn(B, 135, generator=g),
            torch.randn(B, 10, generator=g)]
    return d, gout


ORDER = ("xf0", "xf1", "bb0", "bb1", "pos0", "pos1", "orient0", "orient1", "art0", "art1", "shape0", "shape1")


def _ref_full(P, d, masks):
    """_ref_reg with the intermediates: -> xc, h1d, h2d (2B rows, view 0 first) and (pose0, betas0, pose1, betas1).
    masks: (m1, m2) fp64 (2B, 1024), already multiplied by the keep scale."""
    B = d["xf0"].shape[0]
    W1, b1, W2, b2, Wp, bp, Ws, bs = P
    xc = torch.cat([torch.cat([d["xf%d" % v]] + [d[n + str(v)] for n, _ in STATE] + [d["art%d" % (1 - v)], d["shape%d" % (1 - v)]], 1)
                    for v in (0, 1)], 0)
    h1d = F.linear(xc, W1, b1) * masks[0]
    h2d = F.linear(h1d, W2, b2) * masks[1]
    pose = xc[:, 2051:2186] + F.linear(h2d, Wp, bp)
    betas = xc[:, 2186:2196] + F.linear(h2d, Ws, bs)
    return xc, h1d, h2d, (pose[:B], betas[:B], pose[B:], betas[B:])


def _reference(params, d, gout, masks, out_mask, absolute):
    """fp64 forward and autograd gradients (of sum_i <out_i, gout_i> over the outputs in out_mask) of the restatement; with
    absolute = True on |.| of every operand: the bound A"""
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    P = [f(p).requires_grad_(True) for p in params]
    L = {k: f(v).requires_grad_(True) for k, v in d.items()}
    xc, h1d, h2d, outs = _ref_full(P, L, masks)
    sd = dict(zip(PNAMES, P))
    same = _ref_reg(sd, *[L[k] for k in ORDER], masks=masks, scale=1.0)
    for a, b in zip(outs, same):                             # the restatement here is test_head_grad's, up to the rounding of
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12), "the two fp64 restatements differ"      # one 2B-row product against two
    loss = sum((o * f(g)).sum() for o, g, m in zip(outs, gout, out_mask) if m)
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    r = {"xc": xc.detach(), "h1d": h1d.detach(), "h2d": h2d.detach()}
    for v in (0, 1):
        r["pose%d" % v], r["betas%d" % v] = outs[2 * v].detach(), outs[2 * v + 1].detach()
        r["g_xf%d" % v] = zero(L["xf%d" % v])
        for n, _ in STATE:
            r["g_%s%d" % (n, v)] = zero(L[n + str(v)])
    for n, p in zip(PNAMES, P):
        r["g_" + n] = zero(p)
    return r


def _scale32(p):
    """the kernels' keep scale: 1 / (1 - p) in fp32"""
    return float(np.float32(1) / (np.float32(1) - np.float32(p))) if p > 0 else 1.0


class _Head(object):
    """One forward on the device and everything the backward calls of a case share."""

    def __init__(self, dev, params, B, seed, p1, p2, stride=None):
        from airpose_amd import _native as N
        from airpose_amd import _native_grad as G
        self.dev, self.B, self.p, self.seed = dev, B, (p1, p2), 1000003 * seed + 17
        self.N, self.G, self.L, self.s = N, G, G.lib(), N.stream_ptr(dev)
        self.params = params
        self.pd = [p.to(dev) for p in params]
        d, gout = _inputs(B, seed)
        ld = {n + str(v): w for v in (0, 1) for n, w in STATE}
        dd = {k: v.to(dev) for k, v in d.items()}
        if stride == 0:                                      # one row broadcast to the B samples
            for k in ld:
                d[k] = d[k][:1].expand(B, -1).contiguous()
                dd[k], ld[k] = d[k][:1].to(dev), 0
        elif stride == 135:                                  # pos | orient | art as slices of a previous pred_pose
            for v in "01":
                pp = torch.cat([d["pos" + v], d["orient" + v], d["art" + v]], 1).to(dev)
                dd["pos" + v], dd["orient" + v], dd["art" + v] = pp[:, :3], pp[:, 3:9], pp[:, 9:]
                assert dd["art" + v].stride(0) == 135 and dd["art" + v].data_ptr() == pp.data_ptr() + 36
                ld["pos" + v] = ld["orient" + v] = ld["art" + v] = 135
        self.d, self.gout = d, gout
        self.goutd = [g.to(dev) for g in gout]
        state = [dd[n + str(v)] for v in (0, 1) for n, _ in STATE]
        lds = [ld[n + str(v)] for v in (0, 1) for n, _ in STATE]
        R = 2 * B
        self.fwd = Arena(dev, {"xc": (R, 2332), "h1d": (R, 1024), "h2d": (R, 1024), "pose0": (B, 135), "betas0": (B, 10),
                               "pose1": (B, 135), "betas1": (B, 10)})
        a = self.fwd
        G.check(self.L.apg_head_fwd(B, N.dptr(dd["xf0"]), N.dptr(dd["xf1"]), G.ptrs(state), G.ints(lds), *(N.dptr(p) for p in self.pd),
                                    self.seed, p1, p2, N.dptr(a["xc"]), N.dptr(a["h1d"]), N.dptr(a["h2d"]),
                                    G.ptrs([a["pose0"], a["pose1"]]), G.ptrs([a["betas0"], a["betas1"]]), self.s), "apg_head_fwd")
        torch.cuda.synchronize()
        a.untouched(a.names, "apg_head_fwd")
        self.m8 = [G.dropout_mask(self.seed, l, R, 1024, p, dev).cpu() for l, p in ((1, p1), (2, p2))]
        self.masks = [m.double() / (1.0 - float(np.float32(p))) for m, p in zip(self.m8, (p1, p2))]
        self._refs = {}

    def ref(self, out_mask=ALL_OUT):
        if out_mask not in self._refs:
            self._refs[out_mask] = (_reference(self.params, self.d, self.gout, self.masks, out_mask, False),
                                    _reference(self.params, self.d, self.gout, self.masks, out_mask, True))
        return self._refs[out_mask]

    def check_forward(self, ratios):
        ref, A = self.ref()
        a = self.fwd
        assert torch.equal(a["xc"].cpu().double(), ref["xc"]), "xc is a copy of the inputs"
        for k in ("h1d", "h2d", "betas0", "betas1"):
            check(self.B, k[:-1] if k[-1] in "01" else k, a[k], ref[k], A[k], ratios)
        for v in "01":                                       # translation (z ~ 10) and 6-D rotations: one rel_err each
            check(self.B, "pose.trans", a["pose" + v][:, :3], ref["pose" + v][:, :3], A["pose" + v][:, :3], ratios)
            check(self.B, "pose.rot6d", a["pose" + v][:, 3:], ref["pose" + v][:, 3:], A["pose" + v][:, 3:], ratios)
        for k, m in zip(("h1d", "h2d"), self.m8):            # the mask entry point agrees with what the kernels dropped
            assert not (a[k].cpu()[m == 0] != 0).any(), (k, "a dropped entry is not zero")
            assert float((a[k].cpu()[m == 1] == 0).float().mean()) < 1e-3, (k, "kept entries are zero")

    def workspace(self, need_gxf, short=0):
        nb = self.L.apg_head_bwd_workspace_bytes(self.B, need_gxf)
        assert nb > 0 and nb % 4 == 0
        ws = Arena(self.dev, {"ws": (nb // 4,)})
        return ws, nb - short

    def backward(self, what, ratios, out_mask=ALL_OUT, gpar=GPAR, gin=GIN, expect=0):
        """two identical apg_head_bwd calls writing the outputs named in gpar / gin; expect = 0: compares them with each other
        and with fp64; expect = APG_ENOMEM: the call must refuse and write nothing"""
        N, G = self.N, self.G
        need_gxf = int("g_xf0" in gin or "g_xf1" in gin)
        shapes = dict(zip(GPAR, PSHAPES))
        for v in (0, 1):
            shapes["g_xf%d" % v] = (self.B, 2048)
            for n, w in STATE:
                shapes["g_%s%d" % (n, v)] = (self.B, w)
        asked = list(gpar) + list(gin)
        runs = []
        for _ in range(2):
            out = Arena(self.dev, shapes)
            ws, nb = self.workspace(need_gxf, short=1 if expect else 0)
            rc = self.L.apg_head_bwd(self.B, N.dptr(self.fwd["xc"]), N.dptr(self.fwd["h1d"]), N.dptr(self.fwd["h2d"]),
                                     N.dptr(self.pd[0]), N.dptr(self.pd[2]), N.dptr(self.pd[4]), N.dptr(self.pd[6]), self.seed,
                                     self.p[0], self.p[1], G.ptrs([g if m else None for g, m in zip(self.goutd, out_mask)]),
                                     G.ptrs([out[k] if k in gpar else None for k in GPAR]),
                                     G.ptrs([out[k] if k in gin else None for k in GIN]), N.dptr(ws["ws"]), nb, self.s)
            torch.cuda.synchronize()
            assert rc == expect, (what, rc, self.L.apg_last_error())
            if expect:
                out.untouched((), what)
                ws.untouched((), what)
                return
            out.untouched(asked, what)
            ws.untouched(("ws",), what)                      # nothing past the workspace's last byte
            runs.append(out)
        ref, A = self.ref(out_mask)
        for k in asked:
            assert torch.equal(runs[0][k], runs[1][k]), (what, k, "two identical calls differ")
            check(what, k[:-1] if k in GIN else k, runs[0][k], ref[k], A[k], ratios)


LAYOUTS = {"need_gxf=1": GIN, "need_gxf=0": [k for k in GIN if not k.startswith("g_xf")]}


# ------------------------------------------------------------------------------------------------ row counts, both layouts
@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 64, 65, 100, 257])
def test_row_counts_in_both_workspace_layouts(dev, params, B):
    h = _Head(dev, params, B, seed=40 + B, p1=0.5, p2=0.5)
    ratios = {}
    h.check_forward(ratios)
    report("head fwd B=%d (R=%d)" % (B, 2 * B), ratios)
    assert h.L.apg_head_bwd_workspace_bytes(B, 0) < h.L.apg_head_bwd_workspace_bytes(B, 1)
    for name, gin in LAYOUTS.items():
        ratios = {}
        h.backward((B, name), ratios, gin=gin)
        report("head bwd B=%d %s, %d colsum chunks" % (B, name, (2 * B + 31) // 32), ratios)


@pytest.mark.parametrize("B", [1, 33, 65])
def test_workspace_one_byte_short_is_refused_and_nothing_is_written(dev, params, B):
    h = _Head(dev, params, B, seed=3 + B, p1=0.5, p2=0.5)
    for name, gin in LAYOUTS.items():
        h.backward((B, name, "short"), {}, gin=gin, expect=APG_ENOMEM)
        assert "workspace" in h.L.apg_last_error().decode()


# ------------------------------------------------------------------------------------------------ NULL patterns
OUT_MASKS = [tuple(i != k for i in range(4)) for k in range(4)] + [tuple(i == k for i in range(4)) for k in range(4)]


@pytest.mark.parametrize("B", [33, 65])
def test_null_output_gradients(dev, params, B):
    """a NULL g_out entry is a zero gradient: its rows of g_delta are zero and its residual term is absent"""
    h = _Head(dev, params, B, seed=70 + B, p1=0.5, p2=0.5)
    for mask in OUT_MASKS:
        for name, gin in LAYOUTS.items():
            ratios = {}
            h.backward((B, name, mask), ratios, out_mask=mask, gin=gin)
            report("head bwd B=%d %s g_out %s" % (B, name, "".join("x" if m else "0" for m in mask)), ratios)


def test_parameter_gradient_subsets(dev, params):
    B = 33
    h = _Head(dev, params, B, seed=81, p1=0.5, p2=0.5)
    for gpar in [GPAR[0::2], GPAR[1::2]] + [[k] for k in GPAR]:
        for gin in ((), LAYOUTS["need_gxf=0"]):
            ratios = {}
            h.backward((B, tuple(gpar), len(gin)), ratios, gpar=gpar, gin=gin)
            report("head bwd B=%d g_param %s, %d g_in" % (B, ",".join(k[2:] for k in gpar), len(gin)), ratios)


def test_single_input_gradient(dev, params):
    """one state tensor of one view (need_gxf = 0), or one feature tensor (need_gxf = 1), and no parameter gradient"""
    B = 33
    h = _Head(dev, params, B, seed=82, p1=0.5, p2=0.5)
    ratios = {}
    for k in GIN:
        h.backward((B, k), ratios, gpar=(), gin=[k])
    report("head bwd B=%d one g_in at a time" % B, ratios)


# ------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize("stride", [0, 135])
@pytest.mark.parametrize("B", [5, 33])
def test_state_row_strides(dev, params, B, stride):
    h = _Head(dev, params, B, seed=90 + B + stride, p1=0.5, p2=0.5, stride=stride)
    ratios = {}
    h.check_forward(ratios)
    for name, gin in LAYOUTS.items():
        h.backward((B, stride, name), ratios, gin=gin)
    report("head B=%d state row stride %d" % (B, stride), ratios)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p1,p2", [(0.0, 0.0), (0.5, 0.5), (0.1, 0.7), (0.0, 0.5)])
def test_dropout_rates(dev, params, p1, p2):
    B = 33
    h = _Head(dev, params, B, seed=7, p1=p1, p2=p2)
    ratios = {}
    h.check_forward(ratios)
    for name, gin in LAYOUTS.items():
        h.backward((B, p1, p2, name), ratios, gin=gin)
    report("head B=%d p1 %.1f p2 %.1f" % (B, p1, p2), ratios)
    # kept values are scaled by exactly 1 / (1 - p): against the same forward without dropout, bit for bit (h2d only when
    # drop1 is off, so that both runs feed fc2 the same h1d)
    h0 = _Head(dev, params, B, seed=7, p1=0.0, p2=0.0)
    for k, m, p, comparable in (("h1d", h.m8[0], p1, True), ("h2d", h.m8[1], p2, p1 == 0.0)):
        keep_rate = float(m.float().mean())
        assert abs(keep_rate - (1 - p)) < 0.02, (k, keep_rate)
        if comparable:
            want = torch.where(m.bool(), h0.fwd[k].cpu() * torch.tensor(_scale32(p)), torch.zeros(()))
            assert torch.equal(h.fwd[k].cpu(), want), (k, "kept values are not the undropped ones times 1 / (1 - p)")
            assert torch.equal(h.fwd[k].cpu() != 0, m.bool() & (h0.fwd[k].cpu() != 0)), (k, "zeros differ from apg_dropout_mask")
