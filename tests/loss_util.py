"""Shared by the test_loss_* and test_real_loss_* files: the emulation of a workgroup's summation order, NaN-guarded device buffers
for the C-ABI runs, the bitwise comparison of two runs and the dev fixture of the GPU tests."""
import pytest
import torch

U32 = 2.0 ** -24
LT = 256                                                      # loss_common.inc: LT
GUARD = 512


# ------------------------------------------------------------------------------------------------ fp32 emulation in the kernels' order
def tree(s):
    s = s.clone()
    h = LT // 2
    while h:
        s[..., :h] = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def strided_sum(vals):
    """a workgroup's sum of a list in loop order: thread t adds elements t, t + 256, .. in order, then the tree"""
    n = vals.numel()
    ch = max(1, -(-n // LT))
    x = torch.zeros(ch * LT, dtype=vals.dtype)
    x[:n] = vals
    x = x.view(ch, LT)
    acc = torch.zeros(LT, dtype=vals.dtype)
    for i in range(ch):
        acc = acc + x[i]
    return tree(acc)


# ------------------------------------------------------------------------------------------------ the C ABI on the GPU
class Buf(object):
    """n floats in a NaN-filled device buffer with NaN guard bands, `off` floats past a 16-byte boundary"""

    def __init__(self, dev, n, off=0):
        self.n, self.off = n, off
        self.buf = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.buf[GUARD + off:GUARD + off + n]

    def values(self, shape, what):
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        assert torch.isnan(self.buf[:lo]).all() and torch.isnan(self.buf[hi:]).all(), (what, "a guard band was written")
        assert not torch.isnan(self.out).any(), (what, "%d elements never written" % int(torch.isnan(self.out).sum()))
        return self.out.view(*shape).cpu()


def place(t, dev, off=0):
    """a device copy of t starting `off` floats past a 16-byte boundary"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    out = buf[off:off + t.numel()]
    out.copy_(t.reshape(-1))
    return out


def bit_equal(a, b):
    """two runs' (terms, per view a dict of gradients or None) agree bit for bit, absent gradients included"""
    ta, ga = a
    tb, gb = b
    if not torch.equal(ta.view(torch.int32), tb.view(torch.int32)):
        return False
    for x, y in zip(ga, gb):
        for n in x:
            if (x[n] is None) != (y[n] is None) or (x[n] is not None and not torch.equal(x[n].view(torch.int32), y[n].view(torch.int32))):
                return False
    return True


def run_twice(run, what):
    """run() twice, the two results bit-equal -> the first"""
    got = run()
    again = run()
    assert bit_equal(got, again), (what, "two runs differ")
    return got


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)
