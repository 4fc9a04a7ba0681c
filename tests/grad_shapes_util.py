"""Helpers shared by the *_grad_shapes test files: the two bars of tests/test_trunk_grad_shapes.py (rel_err per tensor and the
element-wise |got - ref| <= TAU A), NaN-filled arenas that show a write outside the requested outputs, and the per-slice bar of
the SMPL-X files (four times the fp32 CPU oracle's own error, floor 1e-5)."""
import torch

from conftest import rel_err

TAU = 1e-5
REL_BAR = 1e-5
SLICE_FLOOR = 1e-5


def check(what, name, got, ref, A, out, rel_bar=REL_BAR):
    """rel_err(got, ref) <= rel_bar and |got - ref| <= TAU A element-wise, exactly 0 where A == 0; records the worst
    err / (TAU A) in out[name] (the maximum over the calls that share the name)"""
    got = got.detach().cpu().double()
    ref, A = ref.detach().cpu().double(), A.detach().cpu().double()
    assert got.shape == ref.shape == A.shape, (what, name, got.shape, ref.shape, A.shape)
    assert torch.isfinite(got).all(), (what, name, "non-finite output (an element never written?)")
    assert (A >= ref.abs() * (1 - 1e-12)).all(), (what, name, "the bound A is below |ref|: the test's own magnitudes are wrong")
    e = rel_err(got.numpy(), ref.numpy())
    err, lim = (got - ref).abs(), TAU * A
    zero = lim == 0
    assert not (err[zero] > 0).any(), (what, name, "%d elements nonzero where every term is 0" % int((err[zero] > 0).sum()))
    ratio = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    out[name] = max(out.get(name, 0.0), ratio)
    out[name + " rel"] = max(out.get(name + " rel", 0.0), e / rel_bar)
    assert e <= rel_bar, (what, name, "rel_err %.3e" % e)
    assert ratio <= 1.0, (what, name, "worst |err| / (tau A) %.3f at tau %.0e" % (ratio, TAU))


def report(what, ratios, extra=""):
    el = {k: v for k, v in ratios.items() if not k.endswith(" rel")}
    rl = {k[:-4]: v for k, v in ratios.items() if k.endswith(" rel")}
    print("%-44s %s worst err/(tau A): %s | worst rel_err/1e-5: %s" % (
        what, extra, "  ".join("%s %.4f" % kv for kv in el.items()), "  ".join("%s %.4f" % kv for kv in rl.items())))


class Arena(object):
    """One NaN-filled fp32 device buffer cut into named tensors with NaN guards between them.  A kernel is handed pointers to
    some of the tensors; untouched() then asserts that every other tensor and every guard still holds NaN only, so a write
    to an output that was not asked for, or past the end of one that was, is seen."""
    GUARD = 64

    def __init__(self, dev, shapes):
        self.names = list(shapes)
        n = self.GUARD
        self.off = {}
        for k, s in shapes.items():
            cnt = 1
            for d in s:
                cnt *= d
            self.off[k] = (n, cnt, tuple(s))
            n += (cnt + self.GUARD + 63) // 64 * 64          # every tensor starts 256-byte aligned
        self.buf = torch.full((n,), float("nan"), device=dev)

    def __getitem__(self, k):
        o, cnt, s = self.off[k]
        return self.buf[o:o + cnt].view(s)

    def untouched(self, written, what):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for k in written:
            o, cnt, _ = self.off[k]
            keep[o:o + cnt] = False
        bad = int((~torch.isnan(self.buf[keep])).sum())
        assert bad == 0, (what, "%d floats written outside the requested outputs %s" % (bad, sorted(written)))


def slice_errs(got, ref, dim):
    """max |got - ref| / max |ref| of every slice along `dim` (a joint's 3 x 3 block over the batch, or one column); a slice
    whose reference is all zero must be exactly zero (reported as 0 or inf)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = []
    for g, r in zip(got.unbind(dim), ref.unbind(dim)):
        den, num = float(r.abs().max()), float((g - r).abs().max())
        out.append(num / den if den > 0 else (0.0 if num == 0 else float("inf")))
    return out


def check_slices(what, name, got, ref64, cpu32, dim, out):
    """Per-slice bar: a slice's error against fp64 may be at most four times the fp32 CPU oracle's error on the same slice, with
    a floor of 1e-5 (the rule of tests/test_trunk_grad.py's n = 1 statistics).  Records the worst err / bar in out[name]."""
    assert torch.isfinite(got).all(), (what, name, "non-finite gradient")
    eg, ec = slice_errs(got, ref64, dim), slice_errs(cpu32, ref64, dim)
    worst, worst_e = 0.0, 0.0
    for i, (g, c) in enumerate(zip(eg, ec)):
        bar = max(4.0 * c, SLICE_FLOOR)
        worst, worst_e = max(worst, g / bar), max(worst_e, g)
        assert g <= bar, (what, name, "slice %d: err %.3e, bar %.3e (fp32 CPU oracle %.3e)" % (i, g, bar, c))
    out[name] = max(out.get(name, 0.0), worst)
    out[name + " err"] = max(out.get(name + " err", 0.0), worst_e)
