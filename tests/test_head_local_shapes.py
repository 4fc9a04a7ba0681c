"""The generic view-local head's kernels through the C ABI (apg_head_local_fwd / apg_head_local_bwd, head_local_grad.hip) against
an fp64 restatement, at the smallest shapes where they can go wrong.

Every case: synthetic fp32 weights and inputs, the same operation in fp64 on the same fp32 values with the masks of
apg_dropout_mask (rows [0, R)), outputs inside NaN-filled arenas, two identical calls compared with torch.equal, and per tensor
the two bars of DESIGN 4.3.3 / 4.3.5 through grad_shapes_util.check:
  - rel_err <= 1e-5;
  - element-wise |got - ref| <= 1e-5 A, exactly 0 where A == 0.
A: the head is linear with no subtractions, so A is the same restatement with the same masks on the absolute values of every
input, weight, bias and output gradient.  xc and the packed decoder weights are copies and must match bit for bit.

Cases: R in {1, 5, 33, 65} (below one tile, one past the 32-row column-sum chunk, one past the 64-row tile) in the four layouts
(hmr: K1 = 2193 odd, 3 decoders, no partner; muhmr: 2329 odd, 3 decoders, partner; single-view: 2196, 2 decoders; copenet step:
2332, 2 decoders, partner), the feature gradient requested and not; stride-0 broadcast segments whose gradient is requested; NULL
output gradients and NULL parameter gradients; p in {0, 0.5}; and a row of R = 65 against the same row alone at R = 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from grad_shapes_util import Arena, check, report

pytestmark = pytest.mark.gpu
MODELS = ("hmr", "muhmr", "singleview", "step")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _layout(model):
    from airpose_amd.head_local_grad import LAYOUTS
    segs, decs = LAYOUTS[model]
    return [w for _, w in segs], [n for _, n, _ in decs], [r for _, _, r in decs]


def _params(model, seed):
    """synthetic head: fc1, fc2 and the decoders at scales that keep every layer O(1)"""
    seg_w, dec_n, _ = _layout(model)
    K1 = 2048 + sum(seg_w)
    g = torch.Generator().manual_seed(seed)
    P = [torch.randn(1024, K1, generator=g) * 0.02, torch.randn(1024, generator=g) * 0.1,
         torch.randn(1024, 1024, generator=g) * 0.03, torch.randn(1024, generator=g) * 0.1]
    for n in dec_n:
        P += [torch.randn(n, 1024, generator=g) * 0.03, torch.randn(n, generator=g) * 0.1]
    return P


def _restate(P, xf, segs, masks, dec_n, dec_res, R):
    xc = torch.cat([xf] + [s.expand(R, -1) for s in segs], 1)
    h1d = F.linear(xc, P[0], P[1]) * masks[0]
    h2d = F.linear(h1d, P[2], P[3]) * masks[1]
    outs = [xc[:, 2048 + r:2048 + r + n] + F.linear(h2d, P[4 + 2 * e], P[5 + 2 * e]) for e, (n, r) in enumerate(zip(dec_n, dec_res))]
    return xc, h1d, h2d, outs


class _Case(object):
    """One forward on the device and everything the backward calls of a case share."""

    def __init__(self, dev, model, R, seed, p1, p2, bcast=()):
        from airpose_amd import _native as N
        from airpose_amd import _native_grad as G
        self.N, self.G, self.L, self.s, self.dev = N, G, G.lib(), N.stream_ptr(dev), dev
        self.model, self.R, self.p, self.seed = model, R, (p1, p2), 1000003 * seed + 29
        self.seg_w, self.dec_n, self.dec_res = _layout(model)
        self.K1, self.Nd = 2048 + sum(self.seg_w), sum(self.dec_n)
        self.bcast = [int(k in bcast) for k in range(len(self.seg_w))]
        self.P = _params(model, 7)
        g = torch.Generator().manual_seed(seed)
        self.xf = torch.relu(torch.randn(R, 2048, generator=g))
        self.segs = [torch.randn(1 if b else R, w, generator=g) for w, b in zip(self.seg_w, self.bcast)]
        self.gout = [torch.randn(R, n, generator=g) for n in self.dec_n]
        self.Pd = [p.to(dev) for p in self.P]
        self.xfd, self.segd, self.goutd = self.xf.to(dev), [s.to(dev) for s in self.segs], [t.to(dev) for t in self.gout]
        self.onames = ["out%d" % e for e in range(len(self.dec_n))]
        shapes = {"xc": (R, self.K1), "h1d": (R, 1024), "h2d": (R, 1024), "wdec": (self.Nd * 1025,)}
        shapes.update({k: (R, n) for k, n in zip(self.onames, self.dec_n)})
        self.runs = []
        for _ in range(2):
            a = Arena(dev, shapes)
            G.check(self.L.apg_head_local_fwd(
                R, N.dptr(self.xfd), len(self.seg_w), G.ptrs(self.segd), G.ints([0 if b else w for w, b in zip(self.seg_w, self.bcast)]),
                G.ints(self.seg_w), *(N.dptr(p) for p in self.Pd[:4]), len(self.dec_n), G.ptrs(self.Pd[4::2]), G.ptrs(self.Pd[5::2]),
                G.ints(self.dec_n), G.ints(self.dec_res), self.seed, p1, p2, N.dptr(a["xc"]), N.dptr(a["h1d"]), N.dptr(a["h2d"]),
                N.dptr(a["wdec"]), G.ptrs([a[k] for k in self.onames]), self.s), "apg_head_local_fwd")
            torch.cuda.synchronize()
            a.untouched(a.names, "apg_head_local_fwd")
            self.runs.append(a)
        self.fwd = self.runs[0]
        self.m8 = [G.dropout_mask(self.seed, l, R, 1024, p, dev).cpu() for l, p in ((1, p1), (2, p2))]
        self.masks = [m.double() / (1.0 - float(np.float32(p))) for m, p in zip(self.m8, (p1, p2))]
        self._refs = {}

    def ref(self, out_mask):
        """fp64 forward and autograd gradients of sum_d <out_d, gout_d> over the decoders in out_mask, and the bound A"""
        if out_mask not in self._refs:
            both = []
            for absolute in (False, True):
                f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
                P = [f(p).requires_grad_(True) for p in self.P]
                xf = f(self.xf).requires_grad_(True)
                segs = [f(s).requires_grad_(True) for s in self.segs]
                xc, h1d, h2d, outs = _restate(P, xf, segs, self.masks, self.dec_n, self.dec_res, self.R)
                sum((o * f(g)).sum() for o, g, m in zip(outs, self.gout, out_mask) if m).backward()
                z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
                r = {"xc": xc.detach(), "h1d": h1d.detach(), "h2d": h2d.detach(), "g_xf": z(xf)}
                r.update({k: o.detach() for k, o in zip(self.onames, outs)})
                r.update({"g_seg%d" % k: z(s) for k, s in enumerate(segs)})
                r.update({"g_par%d" % k: z(p) for k, p in enumerate(P)})
                both.append(r)
            self._refs[out_mask] = tuple(both)
        return self._refs[out_mask]

    def check_forward(self, ratios):
        ref, A = self.ref((True,) * len(self.dec_n))
        a = self.fwd
        for k in a.names:
            assert torch.equal(a[k], self.runs[1][k]), (k, "two identical forward calls differ")
        assert torch.equal(a["xc"].cpu().double(), ref["xc"]), "xc is a copy of the inputs"
        want = torch.cat([p.reshape(-1) for p in self.P[4::2]] + list(self.P[5::2]))
        assert torch.equal(a["wdec"].cpu(), want), "wdec is [W_0; W_1; ..] then the biases"
        for k in ["h1d", "h2d"] + self.onames:
            check((self.model, self.R), k, a[k], ref[k], A[k], ratios)
        for k, m in zip(("h1d", "h2d"), self.m8):            # the mask entry point (rows [0, R)) agrees with what the kernels dropped
            assert not (a[k].cpu()[m == 0] != 0).any(), (k, "a dropped entry is not zero")
            assert float((a[k].cpu()[m == 1] == 0).float().mean()) < 1e-3, (k, "kept entries are zero")

    def backward(self, what, ratios, gxf=True, out_mask=None, gpar=None, gseg=None):
        """two identical apg_head_local_bwd calls on exactly the queried workspace; compares them with each other and with fp64"""
        N, G = self.N, self.G
        nseg, ndec = len(self.seg_w), len(self.dec_n)
        out_mask = (True,) * ndec if out_mask is None else tuple(out_mask)
        gpar = list(range(4 + 2 * ndec)) if gpar is None else list(gpar)
        gseg = list(range(nseg)) if gseg is None else list(gseg)
        shapes = {"g_xf": (self.R, 2048)}
        shapes.update({"g_seg%d" % k: (1 if b else self.R, w) for k, (w, b) in enumerate(zip(self.seg_w, self.bcast))})
        shapes.update({"g_par%d" % k: tuple(p.shape) for k, p in enumerate(self.P)})
        asked = (["g_xf"] if gxf else []) + ["g_seg%d" % k for k in gseg] + ["g_par%d" % k for k in gpar]
        nb = self.L.apg_head_local_bwd_workspace_bytes(self.R, self.K1, self.Nd, int(gxf))
        assert nb > 0 and nb % 4 == 0
        runs = []
        for _ in range(2):
            out = Arena(self.dev, shapes)
            ws = Arena(self.dev, {"ws": (nb // 4,)})
            f = self.fwd
            rc = self.L.apg_head_local_bwd(
                self.R, nseg, G.ints(self.seg_w), G.ints(self.bcast), ndec, G.ints(self.dec_n), G.ints(self.dec_res), N.dptr(f["xc"]),
                N.dptr(f["h1d"]), N.dptr(f["h2d"]), N.dptr(f["wdec"]), N.dptr(self.Pd[0]), N.dptr(self.Pd[2]), self.seed, self.p[0],
                self.p[1], G.ptrs([g if m else None for g, m in zip(self.goutd, out_mask)]),
                G.ptrs([out["g_par%d" % k] if k in gpar else None for k in range(4 + 2 * ndec)]),
                N.dptr(out["g_xf"]) if gxf else None,
                G.ptrs([out["g_seg%d" % k] if k in gseg else None for k in range(nseg)]), N.dptr(ws["ws"]), nb, self.s)
            torch.cuda.synchronize()
            assert rc == 0, (what, rc, self.L.apg_last_error())
            out.untouched(asked, what)
            ws.untouched(("ws",), what)                      # nothing past the workspace's last byte
            runs.append(out)
        ref, A = self.ref(out_mask)
        for k in asked:
            assert torch.equal(runs[0][k], runs[1][k]), (what, k, "two identical calls differ")
            check(what, k, runs[0][k], ref[k], A[k], ratios)
        return runs[0]


# ------------------------------------------------------------------------------------------------ row counts x layouts
@pytest.mark.parametrize("R", [1, 5, 33, 65])
@pytest.mark.parametrize("model", MODELS)
def test_row_counts_and_layouts(dev, model, R):
    c = _Case(dev, model, R, seed=10 + R, p1=0.5, p2=0.5)
    assert c.K1 == {"hmr": 2193, "muhmr": 2329, "singleview": 2196, "step": 2332}[model]
    assert c.Nd == 145
    ratios = {}
    c.check_forward(ratios)
    report("local head fwd %s R=%d" % (model, R), ratios)
    for gxf in (True, False):
        ratios = {}
        c.backward((model, R, gxf), ratios, gxf=gxf)
        report("local head bwd %s R=%d g_xf=%d" % (model, R, gxf), ratios)


# ------------------------------------------------------------------------------------------------ broadcast segments
@pytest.mark.parametrize("R", [5, 33, 65])
@pytest.mark.parametrize("model,bcast", [("hmr", (0, 1, 2)), ("muhmr", (1, 3)), ("singleview", (2,)), ("step", (0, 3))])
def test_broadcast_segments_sum_their_gradient_over_the_rows(dev, model, bcast, R):
    c = _Case(dev, model, R, seed=20 + R, p1=0.5, p2=0.5, bcast=bcast)
    ratios = {}
    c.check_forward(ratios)
    for gxf in (True, False):
        out = c.backward((model, R, "bcast", gxf), ratios, gxf=gxf)
        for k in bcast:
            assert tuple(out["g_seg%d" % k].shape) == (1, c.seg_w[k])
    report("local head %s R=%d broadcast %s" % (model, R, bcast), ratios)


# ------------------------------------------------------------------------------------------------ NULL patterns
@pytest.mark.parametrize("model", ["hmr", "step"])
def test_null_output_and_parameter_gradients(dev, model):
    R = 33
    c = _Case(dev, model, R, seed=31, p1=0.5, p2=0.5)
    nd, ns = len(c.dec_n), len(c.seg_w)
    ratios = {}
    masks = [tuple(i != k for i in range(nd)) for k in range(nd)] + [tuple(i == k for i in range(nd)) for k in range(nd)]
    for mask in masks:                                       # a NULL g_out entry is a zero gradient, its residual term is absent
        c.backward((model, "g_out", mask), ratios, gxf=False, out_mask=mask)
    npar = 4 + 2 * nd
    for gpar in [list(range(0, npar, 2)), list(range(1, npar, 2)), []] + [[k] for k in range(npar)]:
        c.backward((model, "g_param", tuple(gpar)), ratios, gxf=False, gpar=gpar, gseg=[] if len(gpar) == 1 else None)
    for k in range(ns):                                      # one segment gradient alone; then the features alone
        c.backward((model, "g_seg", k), ratios, gxf=False, gpar=[], gseg=[k])
    c.backward((model, "g_xf alone"), ratios, gxf=True, gpar=[], gseg=[])
    report("local head %s R=%d NULL patterns" % (model, R), ratios)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("model", MODELS)
def test_dropout_rates(dev, model, p):
    R = 33
    c = _Case(dev, model, R, seed=41, p1=p, p2=p)
    ratios = {}
    c.check_forward(ratios)
    c.backward((model, p), ratios)
    report("local head %s R=%d p=%.1f" % (model, R, p), ratios)
    for m in c.m8:
        assert abs(float(m.float().mean()) - (1 - p)) < 0.02


# ------------------------------------------------------------------------------------------------ a row depends on itself only
@pytest.mark.parametrize("model", MODELS)
def test_a_row_of_65_equals_the_same_row_alone(dev, model):
    big = _Case(dev, model, 65, seed=51, p1=0.0, p2=0.0)
    gb = big.backward((model, 65), {}, gpar=[])
    for r in (0, 31, 64):
        one = _Case(dev, model, 1, seed=52, p1=0.0, p2=0.0)
        one.xf, one.segs, one.gout = big.xf[r:r + 1], [s[r:r + 1] for s in big.segs], [g[r:r + 1] for g in big.gout]
        one.xfd, one.segd, one.goutd = one.xf.to(dev), [s.to(dev) for s in one.segs], [g.to(dev) for g in one.gout]
        N, G = one.N, one.G
        a = one.fwd
        G.check(one.L.apg_head_local_fwd(
            1, N.dptr(one.xfd), len(one.seg_w), G.ptrs(one.segd), G.ints(one.seg_w), G.ints(one.seg_w),
            *(N.dptr(p) for p in one.Pd[:4]), len(one.dec_n), G.ptrs(one.Pd[4::2]), G.ptrs(one.Pd[5::2]), G.ints(one.dec_n),
            G.ints(one.dec_res), one.seed, 0.0, 0.0, N.dptr(a["xc"]), N.dptr(a["h1d"]), N.dptr(a["h2d"]), N.dptr(a["wdec"]),
            G.ptrs([a[k] for k in one.onames]), one.s), "apg_head_local_fwd")
        torch.cuda.synchronize()
        one._refs = {}
        for k in ["xc", "h1d", "h2d"] + one.onames:
            assert torch.equal(a[k][0], big.fwd[k][r]), (model, r, k, "the row's forward depends on the batch")
        go = one.backward((model, 1, r), {}, gpar=[])
        for k in ["g_xf"] + ["g_seg%d" % i for i in range(len(one.seg_w))]:
            assert torch.equal(go[k][0], gb[k][r]), (model, r, k, "the row's input gradient depends on the batch")
