"""Element-wise fp64 ground truth for every kernel of airpose_amd/csrc/stem.hip that a trunk pass can launch, through the
operator entries ap_stem_pack / ap_stem_nhwc / ap_maxpool_nhwc / ap_avgpool_nhwc (include/airpose_hip.h).  ap_stem_pack runs the
packing of ap_net_finalize (api_net.hip: pack_stem), so the k' = r*32 + s*4 + c layout the trunk runs on is what is tested.

Kernel -> test
  stem_direct_kernel            test_stem_split_and_fp32[fp32]            form 0
  stem_mfma_kernel              test_stem_16bit_every_walk_regime[*]      form 0 (N <= UNPOOLED_MAX_N, then bit-compared through the pool)
  stem_pool_kernel              test_stem_16bit_every_walk_regime[*]      form 1 (strip)
  stem_pool2_kernel             test_stem_16bit_every_walk_regime[*]      form 2 (persistent), every regime, every n_split
  stem_mfma_split_kernel        test_stem_split_and_fp32[bf16x2]          form 0
  stem_pool_split_kernel        test_stem_split_and_fp32[bf16x2]          form 1
  maxpool_kernel<bf16/f16/f32>  test_maxpool_is_exact[bf16 | f16 | fp32]
  maxpool_split_kernel          test_maxpool_is_exact[bf16x2]
  avgpool_kernel<bf16/f16/f32>  test_avgpool[bf16 | f16 | fp32]
  avgpool_split_kernel          test_avgpool[bf16x2]
(stem_direct_kernel had a bf16 and a split-bf16 instantiation that no precision could reach; they are removed, not tested.)

Reference: torch fp64 on the CPU on the operands the kernel sees -- crops and weights rounded to the storage type with .to(dtype)
(bf16x2: the values hi + lo of test_gpu_parity._split_parts) -- F.conv2d(stride 2, padding 3), scale / shift, ReLU,
F.max_pool2d(3, 2, 1); a second fp64 convolution on |x|, |w| gives the magnitude A = |scale| conv(|x|, |w|) + |shift|.

Bars (derived, none measured).  Per element of the stem  |got - ref| <= u |ref| + gamma A  with
  gamma   (224 + 2) 2^-24: an fp32 accumulation over the MFMA K extent 7 x 32 (zero slots included), + 2 for the BatchNorm fma.
  u fp32  0: the stored value is the fp32 result itself (its rounding is one of the "+ 2").
  u bf16  2^-8, the unit roundoff of 8 significand bits (round to nearest even).
  u f16   2^-11, plus 2^-25 absolute: half the subnormal spacing 2^-24 (below 2^-14 fp16 rounds to a multiple of 2^-24).
  u bf16x2  2^-16 + 2^-16.  First term, the loss of _split_parts: hi = rne8(v) leaves |v - hi| <= 2^(e-8) for v in [2^e, 2^(e+1)),
          the difference is exact in fp32 (at most 16 significant bits), lo = rne8(v - hi) leaves at most 2^-8 of that:
          |v - (hi + lo)| <= 2^(e-16) <= 2^-16 |v|.  Second term, the dropped lo*lo product: |lo| <= 2^-8 |hi|, so every dropped
          product is at most 2^-16 (1 - 2^-8)^-2 |x| |w|.  The issue puts both under u, i.e. on |ref|; under cancellation (|ref| << A)
          the dropped products are formally bounded by 2^-16 A only, which is the size of gamma A itself -- of which the accumulation
          uses a small part (measured ratios below), and three MFMAs per product (K extent 3 x 224) stay inside the same gamma.
          The bar is kept as the issue states it, the stricter reading.
  pooled  the maximum of the element bounds over the 3 x 3 window (max is 1-Lipschitz in the sup norm).
  zero    where the bound is 0 (A = 0: no input, no shift) the output must be exactly 0.
Max-pool operators: exactly max_pool2d of the stored values (a maximum does not round; inputs >= 0 as in the trunk).
Average-pool operators: |got - ref| <= 50 2^-24 mean|x| + 2^-24 |ref| (49 additions and the division, one rounding of the result).
Every output lies in a NaN-filled buffer between NaN guard bands: every element written, no guard touched.

Batch sizes of the persistent kernel come from the CU count (walk_regimes); on 256 CUs: 1, 2 (per = 1, every walk but the first
starts inside an image), 9 (252 strips), 10 (per = 2), 37 (per = 5: walks cross image boundaries at every phase), 64 (per = 7:
walks aligned to images), 150 (per = 17).

The CPU self-check (no GPU) holds an fp32 emulation of the operation to the same bars on every input family and demands that six
seeded mutations of it fail.  The crop-truncation mutation applies to the 16-bit types only: fp32 converts nothing, and a
truncated hi part of a split pair is made up by its lo part to 2^-15, inside the bar by design.

Measured on an MI355X (256 CUs), worst err / bound per kernel (python -m pytest tests/test_stem_pool_fp64.py -m gpu -s):
  stem_pool2_kernel        bf16  per=1 0.9924  per=2 0.9881  per=5 0.9925  per=7 0.9917  per=17 0.9919
                           f16   per=1 0.9660  per=2 0.9579  per=5 0.9711  per=7 0.9619  per=17 0.9629
  stem_pool_kernel         bf16 0.9925   f16 0.9711
  stem_mfma_kernel         bf16 0.9925   f16 0.9724
  stem_direct_kernel       fp32 0.0257 (0.0246 through maxpool_kernel<float>)
  stem_mfma_split_kernel   bf16x2 0.1688
  stem_pool_split_kernel   bf16x2 0.1675
  maxpool_kernel / maxpool_split_kernel   exact in all four storage types
  avgpool_kernel           fp32 0.0654   bf16 0.0192   f16 0.0317;   avgpool_split_kernel  bf16x2 0.0724
The 16-bit ratios near 1 are the stored type's rounding alone, not accumulated error: u |ref| is the half-ulp of a value at the
bottom of its binade, and among 10^7 outputs some lie that close to a rounding tie just above a power of two.  The fp32
emulation of the CPU self-check, which shares nothing with the kernels but that final rounding, measures the same (bf16 0.992,
f16 0.968); with the rounding taken out (fp32 storage, same gamma) the accumulation uses 0.026 of gamma A.  The whole file
takes 37 s on the MI355X (the 16-bit walk-regime tests 13 s each, the fp64 references included).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import _split_parts, _split_unpack

GAMMA = (224 + 2) * 2.0 ** -24
U = {"fp32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11, "bf16x2": 2.0 ** -16 + 2.0 ** -16}
U_ABS = {"fp32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25, "bf16x2": 0.0}
DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}
FAMILIES = ("randn", "frame", "alt4", "impulse")
MIX = ("randn", "plus4", "minus4", "frame", "impulse", "minus4", "plus4")   # 7 images: coprime to every walk length used
UNPOOLED_MAX_N = 37


# ------------------------------------------------------------------------------------------------ inputs
def _one_image(kind, gen, k):
    if kind == "randn":
        return torch.randn(3, 224, 224, generator=gen)
    if kind in ("plus4", "minus4"):
        return torch.full((3, 224, 224), 4.0 if kind == "plus4" else -4.0)
    if kind == "frame":
        # zero except a 3-pixel frame of large values on all four borders.  The magnitudes sit at 8 (1 + 6.9 2^-10): rounding to
        # nearest moves them up in bf16 (0.86 of a 2^-7 step) and in fp16 (6.9 -> 7 steps of 2^-10), truncation moves them down
        big = 8.0 * (1.0 + 6.9 * 2.0 ** -10)
        v = big * (torch.randint(0, 2, (3, 224, 224), generator=gen).float() * 2 - 1)
        x = torch.zeros(3, 224, 224)
        for sl in ((slice(None), slice(0, 3)), (slice(None), slice(221, 224)), (slice(0, 3), slice(None)), (slice(221, 224), slice(None))):
            x[:, sl[0], sl[1]] = v[:, sl[0], sl[1]]
        return x
    if kind == "impulse":
        # single pixels at the four corners and the four mid-edges, one channel each (rotating with k): every output near one is a
        # single tap times scale plus shift
        x = torch.zeros(3, 224, 224)
        for j, (iy, ix) in enumerate(((0, 0), (0, 223), (223, 0), (223, 223), (0, 112), (112, 0), (223, 111), (111, 223))):
            x[(j + k) % 3, iy, ix] = (2.0, -3.0, 1.5)[(j + k // 3) % 3]
        return x
    raise ValueError(kind)


def make_images(N, family, seed):
    """family: one of FAMILIES ("alt4": image k is all +4, image k + 1 all -4) or "mix" (MIX, cyclically from `seed`)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    kinds = []
    for k in range(N):
        if family == "mix":
            kinds.append(MIX[(k + seed) % len(MIX)])
        elif family == "alt4":
            kinds.append("plus4" if k % 2 == 0 else "minus4")
        else:
            kinds.append(family)
    return torch.stack([_one_image(kd, gen, k) for k, kd in enumerate(kinds)])


def make_weights(regime, seed, copenet_sd=None):
    if regime == "ckpt":
        return copenet_sd["conv1.weight"].float().clone()
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(64, 3, 7, 7, generator=gen) * (2.0 / 147) ** 0.5


def make_bn(seed):
    """All BatchNorm regimes in one vector, 16 channels each under a seeded permutation: ordinary (scale in [.5, 1.5], |shift| in
    [.05, .15]; two of them with shift exactly 0), negative scale, shift << 0 (large regions exactly 0), shift >> 0 (nothing clipped)"""
    gen = torch.Generator().manual_seed(3000 + seed)
    perm = torch.randperm(64, generator=gen)
    scale = torch.rand(64, generator=gen) + 0.5
    shift = (0.05 + 0.1 * torch.rand(64, generator=gen)) * (torch.randint(0, 2, (64,), generator=gen).float() * 2 - 1)
    reg = torch.empty(64, dtype=torch.long)
    reg[perm] = torch.arange(64) // 16
    scale[reg == 1] *= -1.0
    shift[reg == 2] = -3.0 - 3.0 * torch.rand(int((reg == 2).sum()), generator=gen)
    shift[reg == 3] = 20.0 + 20.0 * torch.rand(int((reg == 3).sum()), generator=gen)
    shift[perm[:2]] = 0.0
    return scale, shift


# ------------------------------------------------------------------------------------------------ number formats
def _truncate(t, prec):
    """t rounded TOWARDS ZERO to the 16-bit type (the crop-conversion mutation)"""
    if prec == "bf16":
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    h = t.to(torch.float16)
    over = h.float().abs() > t.abs()
    return (h.view(torch.int16) - over.to(torch.int16)).view(torch.float16).float()


def operands(t, prec, trunc=False):
    """fp32 tensor holding exactly the values the kernel computes with"""
    if prec == "fp32":
        return t.clone()
    if prec == "bf16x2":
        return _split_parts(t)[2]
    return _truncate(t, prec) if trunc else t.to(DT16[prec]).float()


def stored(y, prec):
    return operands(y, prec)


# ------------------------------------------------------------------------------------------------ reference and checker
def reference(x, w, scale, shift, prec, want_full=True, chunk=8):
    """fp64: (ref, bound) un-pooled [N][112][112][64] (None unless want_full) and pooled [N][56][56][64], channels last"""
    xq, wq = operands(x, prec).double(), operands(w, prec).double()
    s, h = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    full_r, full_b, pool_r, pool_b = [], [], [], []
    for i in range(0, x.shape[0], chunk):
        c = F.conv2d(xq[i:i + chunk], wq, stride=2, padding=3)
        a = F.conv2d(xq[i:i + chunk].abs(), wq.abs(), stride=2, padding=3)
        ref = (c * s + h).clamp_min(0)
        A = s.abs() * a + h.abs()
        bound = U[prec] * ref + GAMMA * A
        bound = torch.where(bound > 0, bound + U_ABS[prec], bound)
        pool_r.append(F.max_pool2d(ref, 3, 2, 1).permute(0, 2, 3, 1).contiguous())
        pool_b.append(F.max_pool2d(bound, 3, 2, 1).permute(0, 2, 3, 1).contiguous())   # (bounds are >= 0: the -inf padding never wins)
        if want_full:
            full_r.append(ref.permute(0, 2, 3, 1).contiguous())
            full_b.append(bound.permute(0, 2, 3, 1).contiguous())
    cat = lambda l: torch.cat(l) if l else None
    return {"full": (cat(full_r), cat(full_b)), "pool": (cat(pool_r), cat(pool_b))}


def evaluate(got, ref, bound):
    """(ok, worst err / bound, elements nonzero where the bound is 0, message)"""
    got = got.double()
    if got.shape != ref.shape:
        return False, float("inf"), 0, "shape %s against %s" % (tuple(got.shape), tuple(ref.shape))
    if not torch.isfinite(got).all():
        return False, float("inf"), 0, "%d non-finite elements (never written?)" % int((~torch.isfinite(got)).sum())
    err = (got - ref).abs()
    zero = bound == 0
    nz = int((err[zero] > 0).sum())
    q = torch.where(zero, torch.zeros_like(err), err / torch.where(zero, torch.ones_like(bound), bound))
    ratio = float(q.max())
    msg = ""
    if ratio > 1 or nz:
        i = int(q.argmax())
        idx = []
        for d in reversed(got.shape):
            idx.append(i % d)
            i //= d
        msg = "worst err / bound %.3f at [n, y, x, c] = %s (got %.9g, ref %.9g); %d nonzero where the bound is 0" % (
            ratio, idx[::-1], float(got.flatten()[int(q.argmax())]), float(ref.flatten()[int(q.argmax())]), nz)
    return ratio <= 1 and nz == 0, ratio, nz, msg


def check(what, name, got, ref, bound, ratios):
    ok, ratio, _, msg = evaluate(got, ref, bound)
    ratios[name] = max(ratios.get(name, 0.0), ratio)
    assert ok, (what, name, msg)


def report(what, ratios):
    print("%-34s worst err / bound: %s" % (what, "  ".join("%s %.4f" % kv for kv in ratios.items())))


# ------------------------------------------------------------------------------------------------ persistent kernel's walks
def walk_plan(N, n_cu):
    """ap_launch_stem_pool, form 2: (strips per workgroup, workgroups, sorted set of the phases within an image at which walks start)"""
    total = 28 * N
    per = (total + n_cu - 1) // n_cu
    grid = (total + per - 1) // per
    return per, grid, sorted({(b * per) % 28 for b in range(grid)})


def walk_regimes(n_cu):
    """Batch sizes that put the persistent kernel's walks in each regime on a chip of n_cu CUs (256: 1, 2, 9, 10, 37, 64, 150)"""
    full = n_cu // 28                                        # images that fit at one strip per workgroup
    Ns = [1, 2, full, full + 1, 4 * n_cu // 28 + 1, n_cu // 4, 33 * n_cu // 56]
    assert n_cu >= 112 and Ns == sorted(set(Ns)), (n_cu, Ns)
    per = [walk_plan(N, n_cu)[0] for N in Ns]
    assert per[:4] == [1, 1, 1, 2], per                      # one strip per walk: every walk but each image's first starts inside an image
    assert walk_plan(Ns[2], n_cu)[1] > n_cu - 28             # ... on (nearly) every CU
    p5, _, ph5 = walk_plan(Ns[4], n_cu)
    assert p5 == 5 and len(ph5) == 28, (p5, ph5)             # walks start at every phase: image boundaries at every position of a walk
    p7, _, ph7 = walk_plan(Ns[5], n_cu)
    assert 28 % p7 == 0 and p7 > 1 and all(p % p7 == 0 for p in ph7), (p7, ph7)   # no walk crosses an image boundary
    assert per[6] > 14, per                                  # walks longer than half an image
    return Ns


def test_walk_regimes_on_256_cus():
    assert walk_regimes(256) == [1, 2, 9, 10, 37, 64, 150]
    assert [walk_plan(N, 256)[0] for N in (1, 2, 9, 10, 37, 64, 150)] == [1, 1, 1, 2, 5, 7, 17]
    assert walk_plan(9, 256)[1] == 252
    walk_regimes(304)
    walk_regimes(128)


# ------------------------------------------------------------------------------------------------ CPU self-check
MUTATIONS = ("swap_taps", "carry_row", "no_left_pad", "relu_first", "trunc_crop", "drop_shift")


def emulate(x, w, scale, shift, prec, pooled, mut=None, seed=0):
    """fp32 emulation: fp32 conv on the rounded operands -> BatchNorm -> ReLU -> rounding -> max_pool2d; channels last.
    mut: one of MUTATIONS, seeded."""
    gen = torch.Generator().manual_seed(4000 + seed)
    xq, wq = operands(x, prec, trunc=(mut == "trunc_crop")), operands(w, prec)
    scale, shift = scale.clone(), shift.clone()
    if mut == "swap_taps":                                   # two taps of the packed weight swapped (all output channels)
        k = torch.randperm(147, generator=gen)[:2]
        flat = wq.reshape(64, 147)
        flat[:, k] = flat[:, k.flip(0)]
        wq = flat.reshape(64, 3, 7, 7)
    if mut == "no_left_pad":                                 # the left border reads the edge column instead of padding
        xp = F.pad(xq, (3, 3, 3, 3))
        xp[:, :, 3:227, :3] = xq[:, :, :, :1]
        c = F.conv2d(xp, wq, stride=2)
    else:
        c = F.conv2d(xq, wq, stride=2, padding=3)
    if mut == "drop_shift":
        shift[int(torch.randint(0, 64, (1,), generator=gen))] = 0.0
    s, h = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    y = c.clamp_min(0) * s + h if mut == "relu_first" else (c * s + h).clamp_min(0)
    if mut == "carry_row":                                   # the first conv row of image k + 1 taken from image k (its last row)
        y = y.clone()
        y[1:, :, 0, :] = y[:-1, :, 111, :]
    y = stored(y, prec)
    if pooled:
        y = F.max_pool2d(y, 3, 2, 1)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "f16", "bf16x2"])
def test_cpu_emulation_is_inside_the_bars_and_mutations_are_not(prec, copenet_sd):
    """The reference alone stays inside every bar on every input family, un-pooled and pooled, with both weight regimes; each
    mutation of the emulation is rejected (on the mixed batch, pooled and un-pooled)."""
    ratios = {}
    scale, shift = make_bn(1)
    for family, N in [(f, 2) for f in FAMILIES] + [("mix", 7)]:
        for regime in ("he", "ckpt"):
            if regime == "ckpt" and family not in ("randn", "mix"):
                continue
            x, w = make_images(N, family, 3), make_weights(regime, 5, copenet_sd)
            R = reference(x, w, scale, shift, prec)
            for pooled in (False, True):
                ref, bound = R["pool" if pooled else "full"]
                check(prec, "%s/%s/%s" % (family, regime, "pool" if pooled else "full"), emulate(x, w, scale, shift, prec, pooled), ref,
                      bound, ratios)
            if family == "frame":                            # the interior sees no input: channels without a shift are exactly 0
                assert (R["full"][1] == 0).any()
            if family != "mix" or regime != "he":
                continue
            for mut in MUTATIONS:
                if mut == "trunc_crop" and prec not in DT16:
                    continue
                for pooled in (False, True):
                    ref, bound = R["pool" if pooled else "full"]
                    ok, ratio, nz, _ = evaluate(emulate(x, w, scale, shift, prec, pooled, mut=mut, seed=11), ref, bound)
                    assert not ok, (prec, mut, pooled, "the checker accepts this mutation: worst err / bound %.3f" % ratio)
                    ratios["!" + mut + ("/pool" if pooled else "/full")] = ratio
    report("emulation " + prec, ratios)


# ------------------------------------------------------------------------------------------------ GPU side
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Guarded(object):
    """n elements of the storage of `prec` in a NaN-filled device buffer with NaN guard bands before and after"""
    GUARD = 512

    def __init__(self, dev, prec, n):
        self.prec, self.n = prec, n
        dt = DT16.get(prec, torch.bfloat16 if prec == "bf16x2" else torch.float32)
        self.m = 2 * n if prec == "bf16x2" else n            # a split pair = two bf16
        self.buf = torch.full((self.m + 2 * self.GUARD,), float("nan"), dtype=dt, device=dev)
        self.out = self.buf[self.GUARD:self.GUARD + self.m]

    def values(self, shape, what):
        """fp32 values of the output (on the device); asserts that the guards are intact and every element was written"""
        G = self.GUARD
        assert torch.isnan(self.buf[:G]).all() and torch.isnan(self.buf[G + self.m:]).all(), (what, "a guard band was written")
        assert not torch.isnan(self.out).any(), (what, "%d storage elements never written" % int(torch.isnan(self.out).sum()))
        if self.prec == "bf16x2":
            return _split_unpack(self.out.view(torch.int32).view(*shape))
        return self.out.float().view(*shape)

    def bits(self):
        return self.out.view(torch.int16) if self.out.dtype != torch.float32 else self.out.view(torch.int32)


class Stem(object):
    def __init__(self, dev, prec, w, scale, shift):
        from airpose_amd import _native as Nn
        self.Nn, self.L, self.dev, self.prec = Nn, Nn.lib(), dev, prec
        self.P = Nn.PRECISIONS[prec]
        nb = self.L.ap_stem_pack_bytes(self.P)
        assert nb == {"fp32": 147 * 64 * 4, "bf16": 64 * 240 * 2, "f16": 64 * 240 * 2, "bf16x2": 2 * 64 * 240 * 2}[prec]
        self.wd = w.contiguous().to(dev)
        self.wpk = torch.zeros(nb, dtype=torch.uint8, device=dev)
        Nn.check(self.L.ap_stem_pack(self.P, _p(self.wd), _p(self.wpk), Nn.stream_ptr(dev)), "ap_stem_pack")
        self.scale, self.shift = scale.contiguous().to(dev), shift.contiguous().to(dev)

    def run(self, form, xd, n_split):
        """-> Guarded output; xd: the crops on the device, handed over as two allocations of their own"""
        N = xd.shape[0]
        S = 112 if form == 0 else 56
        nanimg = torch.full((1, 3, 224, 224), float("nan"), device=self.dev)     # a view without images: never read
        x0 = xd[:n_split].clone() if n_split else nanimg
        x1 = xd[n_split:].clone() if n_split < N else nanimg
        g = Guarded(self.dev, self.prec, N * S * S * 64)
        rc = self.L.ap_stem_nhwc(self.P, form, _p(x0), _p(x1), n_split, _p(self.wpk), _p(self.scale), _p(self.shift), _p(g.out), N,
                                 self.Nn.stream_ptr(self.dev))
        self.Nn.check(rc, "ap_stem_nhwc")
        torch.cuda.synchronize()
        return g

    def maxpool(self, gin, N):
        g = Guarded(self.dev, self.prec, N * 56 * 56 * 64)
        self.Nn.check(self.L.ap_maxpool_nhwc(self.P, _p(gin.out), _p(g.out), N, self.Nn.stream_ptr(self.dev)), "ap_maxpool_nhwc")
        torch.cuda.synchronize()
        return g


def _splits(N):
    return sorted({0, 1, N // 2, N})


@gpu
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_stem_16bit_every_walk_regime(dev, prec, copenet_sd):
    """stem_pool2_kernel (persistent, the trunk's default) at every walk regime and every n_split, stem_pool_kernel (strips) and
    stem_mfma_kernel (un-pooled) against fp64; then the three forms bit for bit (the un-pooled one through ap_maxpool_nhwc)."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    regimes = walk_regimes(n_cu)
    scale, shift = make_bn(2)
    r2, r1, r0 = {}, {}, {}
    cases = [(N, f, "he") for N in regimes[:2] for f in FAMILIES] + [(N, "mix", "he") for N in regimes[2:]]
    cases += [(regimes[1], "mix", "ckpt"), (regimes[4], "mix", "ckpt")]
    stems = {rg: Stem(dev, prec, make_weights(rg, 6, copenet_sd), scale, shift) for rg in ("he", "ckpt")}
    for ci, (N, family, regime) in enumerate(cases):
        what = "%s N=%d %s %s" % (prec, N, family, regime)
        x, st = make_images(N, family, ci), stems[regime]
        full = N <= UNPOOLED_MAX_N
        R = reference(x, st.wd.cpu(), scale, shift, prec, want_full=full)
        xd = x.to(dev)
        pref, pbound = R["pool"]
        bits = None
        for ns in _splits(N):
            g = st.run(2, xd, ns)
            check(what + " n_split=%d" % ns, "per=%d" % walk_plan(N, n_cu)[0], g.values((N, 56, 56, 64), what).cpu(), pref, pbound, r2)
            assert bits is None or torch.equal(g.bits(), bits), (what, ns, "the result depends on n_split")
            bits = g.bits()
        for ns in (_splits(N) if N <= regimes[3] else [N // 2]):
            g1 = st.run(1, xd, ns)
            if full:
                check(what + " n_split=%d" % ns, "strip", g1.values((N, 56, 56, 64), what).cpu(), pref, pbound, r1)
            else:
                g1.values((N, 56, 56, 64), what)
            assert torch.equal(g1.bits(), bits), (what, ns, "stem_pool_kernel and stem_pool2_kernel differ")
            g0 = st.run(0, xd, ns)
            if full:
                check(what + " n_split=%d" % ns, "un-pooled", g0.values((N, 112, 112, 64), what).cpu(), R["full"][0], R["full"][1], r0)
            else:
                g0.values((N, 112, 112, 64), what)
            assert torch.equal(st.maxpool(g0, N).bits(), bits), (what, ns, "stem_mfma_kernel + maxpool_kernel and stem_pool2_kernel differ")
    report("stem_pool2_kernel " + prec, r2)
    report("stem_pool_kernel " + prec, r1)
    report("stem_mfma_kernel " + prec, r0)


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16x2"])
def test_stem_split_and_fp32(dev, prec, copenet_sd):
    """fp32: stem_direct_kernel.  bf16x2: stem_mfma_split_kernel and stem_pool_split_kernel, then the two bit for bit."""
    scale, shift = make_bn(3)
    r0, r1 = {}, {}
    stems = {rg: Stem(dev, prec, make_weights(rg, 7, copenet_sd), scale, shift) for rg in ("he", "ckpt")}
    cases = [(1, f, "he") for f in FAMILIES] + [(2, "alt4", "he"), (5, "mix", "he"), (5, "mix", "ckpt"), (37, "mix", "he")]
    for ci, (N, family, regime) in enumerate(cases):
        what = "%s N=%d %s %s" % (prec, N, family, regime)
        x, st = make_images(N, family, 20 + ci), stems[regime]
        R = reference(x, st.wd.cpu(), scale, shift, prec)
        xd = x.to(dev)
        for ns in _splits(N):
            g0 = st.run(0, xd, ns)
            check(what + " n_split=%d" % ns, "un-pooled", g0.values((N, 112, 112, 64), what).cpu(), R["full"][0], R["full"][1], r0)
            if prec == "bf16x2":
                g1 = st.run(1, xd, ns)
                check(what + " n_split=%d" % ns, "strip", g1.values((N, 56, 56, 64), what).cpu(), R["pool"][0], R["pool"][1], r1)
                assert torch.equal(st.maxpool(g0, N).bits(), g1.bits()), (what, ns, "split stem + split max-pool and the fused kernel differ")
            else:
                pooled = st.maxpool(g0, N).values((N, 56, 56, 64), what).cpu()
                check(what + " n_split=%d" % ns, "un-pooled + maxpool", pooled, R["pool"][0], R["pool"][1], r1)
    if prec == "fp32":
        report("stem_direct_kernel fp32", r0)
        report("stem_direct_kernel + maxpool fp32", r1)
    else:
        report("stem_mfma_split_kernel bf16x2", r0)
        report("stem_pool_split_kernel bf16x2", r1)


def _to_storage(v, prec, dev):
    """fp32 values (channels last) -> (device tensor in the storage of prec, the fp32 values it stands for)"""
    from test_gpu_parity import _split_pack
    if prec == "bf16x2":
        word, val = _split_pack(v)
        return word.to(dev), val
    if prec == "fp32":
        return v.contiguous().to(dev), v
    q = v.to(DT16[prec])
    return q.contiguous().to(dev), q.float()


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16", "f16", "bf16x2"])
def test_maxpool_is_exact(dev, prec):
    """ap_maxpool_nhwc == max_pool2d of the stored values, exactly (inputs >= 0: the operator's domain)"""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    for N in (1, 5, 37):
        gen = torch.Generator().manual_seed(600 + N)
        v = torch.randn(N, 112, 112, 64, generator=gen).clamp_min(0) * 3.0      # half the elements exactly 0, as after a ReLU
        v[0, 0, :, :] = 7.0                                                      # maxima on the border rows / columns
        v[N - 1, :, 111, :] = 9.0
        v[N // 2, 111, :, :8] = 11.0
        if N > 1:
            v[1] = 0.0
            v[1, ::2, ::2, :] = torch.rand(56, 56, 64, generator=gen)            # only window CENTRES are nonzero ...
            v[N - 1, 1::2, 1::2, :] += 1.0                                       # ... and window corners
        xd, val = _to_storage(v, prec, dev)
        g = Guarded(dev, prec, N * 56 * 56 * 64)
        Nn.check(L.ap_maxpool_nhwc(Nn.PRECISIONS[prec], _p(xd), _p(g.out), N, Nn.stream_ptr(dev)), "ap_maxpool_nhwc")
        torch.cuda.synchronize()
        got = g.values((N, 56, 56, 64), "maxpool %s N=%d" % (prec, N)).cpu()
        want = F.max_pool2d(val.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(got.double(), want), (prec, N, int((got.double() != want).sum()))
    print("%-34s exact" % ("maxpool " + prec))


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16", "f16", "bf16x2"])
def test_avgpool(dev, prec):
    """ap_avgpool_nhwc against the fp64 mean: 50 2^-24 mean|x| + one fp32 rounding of the result"""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    ratios = {}
    for N, C in ((1, 2048), (5, 2048), (37, 2048), (3, 256), (2, 128 if prec == "fp32" else 512)):
        gen = torch.Generator().manual_seed(700 + N + C)
        v = torch.randn(N, 49, C, generator=gen) * 2.0
        v[0, :, : C // 2].clamp_min_(0)                                          # post-ReLU values, as in the trunk
        v[N - 1, 48, :] = 50.0                                                   # the 49th pixel (a partition of its own in the kernel)
        xd, val = _to_storage(v, prec, dev)
        buf = torch.full((N * C + 1024,), float("nan"), device=dev)
        out = buf[512:512 + N * C]
        Nn.check(L.ap_avgpool_nhwc(Nn.PRECISIONS[prec], _p(xd), _p(out), N, C, Nn.stream_ptr(dev)), "ap_avgpool_nhwc")
        torch.cuda.synchronize()
        assert torch.isnan(buf[:512]).all() and torch.isnan(buf[512 + N * C:]).all() and not torch.isnan(out).any()
        ref = val.double().mean(1)
        bound = 50 * 2.0 ** -24 * val.double().abs().mean(1) + 2.0 ** -24 * ref.abs()
        check("avgpool %s" % prec, "N=%d C=%d" % (N, C), out.view(N, C).cpu(), ref, bound, ratios)
    report("avgpool " + prec, ratios)
    assert L.ap_avgpool_nhwc(Nn.PRECISIONS[prec], _p(xd), _p(out), 1, 64, Nn.stream_ptr(dev)) != 0      # refused before any launch


def test_operator_entries_check_their_arguments():
    """Host only: the argument check comes before any launch (no GPU needed)."""
    from airpose_amd import _native as Nn
    L = Nn.lib()
    one = ctypes.c_void_p(256)
    assert L.ap_stem_pack_bytes(7) < 0 and L.ap_stem_pack_bytes(Nn.AP_PREC_FP32) == 147 * 64 * 4
    assert L.ap_stem_pack(Nn.AP_PREC_BF16, None, one, None) == -1
    for prec, form in ((Nn.AP_PREC_FP32, 1), (Nn.AP_PREC_BF16X2, 2), (Nn.AP_PREC_BF16, 3), (Nn.AP_PREC_F16, -1), (9, 0)):
        assert L.ap_stem_nhwc(prec, form, one, one, 1, one, one, one, one, 2, None) == -1, (prec, form)
    assert L.ap_stem_nhwc(Nn.AP_PREC_BF16, 2, one, one, 3, one, one, one, one, 2, None) == -1               # n_split > N
    assert L.ap_stem_nhwc(Nn.AP_PREC_BF16, 2, None, one, 1, one, one, one, one, 2, None) == -1              # a view with images is NULL
    assert L.ap_maxpool_nhwc(Nn.AP_PREC_BF16, None, one, 1, None) == -1 and L.ap_maxpool_nhwc(Nn.AP_PREC_F16, one, one, 0, None) == -1
    assert L.ap_avgpool_nhwc(Nn.AP_PREC_FP32, one, one, 1, 64, None) != 0 and L.ap_avgpool_nhwc(Nn.AP_PREC_BF16, one, None, 1, 2048, None) == -1
