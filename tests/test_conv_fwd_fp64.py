"""Element-wise fp64 ground truth for the forward convolution kernels of Bottleneck.forward, through the C ABI operator entries
(include/airpose_hip.h).  Companion of test_stem_pool_fp64.py, whose evaluate / check / report / Guarded / operands / U / U_ABS it reuses.

Kernel -> test
  conv_pipe_kernel (conv_pipe.hip)     test_conv2d_every_configuration[*-0 .. *-13]      every tile / wave / ring / epilogue variant
                                       ([fp32 | bf16 | f16 | bf16x2]-[-1 | 11 | 12]; 14 and 17 on the shapes they do not take)
  conv_slab_kernel (conv_slab.hip)     test_conv2d_every_configuration[bf16-14 | f16-14 | *--1]   the 3 x 3 / stride 1 shapes, W <= 30
  conv_lean_kernel (conv_lean.hip)     test_conv2d_every_configuration[bf16-17 | f16-17]          every pointwise stride-1 shape
  conv_igemm_kernel (conv_igemm.hip)   test_conv2d_every_configuration[*-100 | *--1]     (-1: every shape of the list is small enough)
  conv_pw_kernel (conv_pw.hip)         test_conv_pw / test_conv_pw_ds / test_conv_pw_k3s2     (bit-equal to ap_conv2d_nhwc where documented)
  conv_img3_kernel (conv_img3.hip)     test_conv_img3_and_s2p[img3-*]      NHWC and fragment-tiled output
  conv_s2p_kernel (conv_s2p.hip)       test_conv_img3_and_s2p[s2p-*]       NHWC and fragment-tiled output
  conv_pair_kernel (conv_pair.hip)     test_conv_pair / test_conv_pair_ds  every (P, N1) / (P, P2, N1) of the header
  bottleneck2 kernels (bottleneck2.hip) test_bottleneck64_identity (bit-equal chain, every stage against fp64), test_bottleneck64_downsample
                                       (propagated bound), test_bottleneck64_tail (bit-equal chain, y_even 0 and 1)
  block_img_kernel (block_img.hip)     test_block_img          bit-equal chain, every stage of the chain against fp64

Reference.  torch fp64 on the CPU on exactly the values the kernel sees: operands rounded to the storage type with .to(dtype)
(bf16x2: the values hi + lo of test_gpu_parity._split_parts), F.conv2d, scale and shift, + res, ReLU where asked.  A second fp64
convolution on the absolute values gives the magnitude  A = |scale| conv(|x|, |w|) + |shift| + |res|.

Bars (derived, none measured).  Per element  |got - ref| <= u |ref| + gamma A  (+ U_ABS where that is not 0)  with
  gamma   (K + 3) 2^-24.  An fp32 sum of K products in ANY order is within (K - 1) 2^-24 sum|x w| of the exact sum when the products
          are exact (MFMA, fma) and within K 2^-24 when they are rounded; the epilogue adds three roundings, each of a value that A
          bounds: the multiplication by scale and the addition of shift (one rounding where they contract to an fma), the addition
          of the residual.  K is the contraction length the kernel runs: k k Cin, + Cin2 for the downsample-folded forms.
  bf16x2  K is three times that: every product is hi*hi + hi*lo + lo*hi, three MFMA terms.  The dropped lo*lo term is at most
          2^-18 |x w| (|lo| <= 2^-9 |hi|), a fraction (K + 3)^-1 2^6 <= 1/3 of gamma A at K >= 3 * 64; it lives inside gamma A.
  u, U_ABS  those of test_stem_pool_fp64 (fp32 0; bf16 2^-8; f16 2^-11 and 2^-25 absolute; bf16x2 2^-15): the one rounding of the
          stored value.  (It rounds the COMPUTED value; u |got - ref| is second order and far inside the unused part of gamma A.)
  zero    where the bound is 0 (no input under the taps, shift 0, no residual) the output must be exactly 0.
  t1n of the pair kernels is held against fp64 evaluated on the kernel's OWN stored `out` (the value its second GEMM reads), so
          no term is propagated there.
  hidden 16-bit intermediate m (ap_bottleneck64_nhwc with downsample = 1, whose chain has no operator entry: the second K segment
          is not part of ap_conv2d_nhwc's ABI).  The reference chain rounds m to the storage type where the kernel does.  The
          kernel's pre-rounding value is within gamma_m A_m (+ what the previous stage propagated) of the reference's, and both are
          then rounded: |m_kernel - m_ref| <= d_m = 2 u |m_ref| + U_ABS' + gamma_m A_m + propagated  (two roundings of values of
          nearly that magnitude: the intermediate may land on the neighbouring 16-bit value; ReLU is 1-Lipschitz).  The next stage
          sees its input moved by d_m, i.e. its output by at most |scale| conv(d_m, |w|): that term is added to the next stage's
          bound, stage by stage.  (U_ABS' = 2 U_ABS for the two roundings.)
Every output lies in a NaN-filled buffer between NaN guard bands (Guarded): every element written, no guard touched.

Inputs.  Each image of a batch is one of: randn; constant +4 / -4 images alternating ("alt": shows a carry between images); "frame":
zero except a one-pixel border of +-8 (1 + 6.9 2^-10), where round-to-nearest and truncation differ in bf16 and fp16; "impulse":
single pixels at the four corners and the four mid-edges, one channel each.  The BatchNorm vectors mix five regimes per channel
under a seeded permutation: ordinary, negative scale, shift exactly 0, shift strongly negative (regions exactly 0 after the
ReLU), shift strongly positive.  The padding rows of scale / shift ([Cout, Cout_pad)) hold 777 / -555: a kernel that reads a
tail channel's constants from a neighbour shows.  Residual on and off, ReLU on and off; every magnitude stays inside fp16.

Shapes of ap_conv2d_nhwc (SHAPES): 1 x 1 at M = 15 (one K step, fewer than the ring stages), M = 127, 128, 129, 255, 256, 257 from
non-square images; Cout = 8, 72, 136, 192 (fp32: 4 too) across the 64- and 128-wide tiles; Cin = 64, 128, 192 (1 x 1) and 64, 128
(3 x 3); 3 x 3 / 1 / 1 at (H, W) = (5, 9), (9, 5), (1, 7), (7, 1), (2, 2) and W = 29, 30, 31 (the slab kernel takes W <= 30:
130 + 2 W slab rows <= 190; configuration 14 and the automatic choice switch kernels between 30 and 31), seven pixel tiles of
9 x 29 images; 3 x 3 / 2 / 1 at H = 7, 6 and (7, 10); 1 x 1 / 2 at (7, 5); five 6 x 6 images per pixel tile (alternating signs:
a halo must never come from the neighbouring image); Cin 128 -> Cout 520 for the lean kernel.  The automatic choice takes the
slab kernel (16-bit, 3 x 3 / 1 / 1, W <= 30) and otherwise, at these sizes, the register-staged kernel; its large-grid branches
(11, 12, 17) are the forced configurations of the same kernels, and test_gpu_parity.test_conv_primitive runs them at production size.

Documented refusals (REFUSALS).  None: every configuration of ALL_CFGS / F16_CFGS / (-1, 11, 12, 100) runs every shape of the
list in its precision (14 and 17 run configuration 11 on the shapes they do not take, as the header says).  A nonzero status
is therefore a failure.

Finding.  The header gave the slab kernel's limit as "image rows of at most 29 pixels"; ap_conv_slab_supported takes W <= 30
(128 + 2 W + 2 <= 190 slab rows in front of the two zero rows) and W = 30 passes element-wise here, so the header now says 30.

CPU self-check (no GPU): an fp32 emulation (tap by tap over the flat pixel index, as the kernels address) of conv, BatchNorm,
residual, ReLU and storage rounding sits inside every bar on every shape x family x (ReLU, residual) in all four precisions,
and eight seeded mutations of it are each rejected (MUTATIONS).

Measured on an MI355X, worst err / bound (python -m pytest tests/test_conv_fwd_fp64.py -m gpu -s): see MEASURED below.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import ALL_CFGS, F16_CFGS
from test_stem_pool_fp64 import DT16, Guarded, U, U_ABS, _to_storage, check, evaluate, operands, report

MEASURED = """
Worst err / bound on an MI355X (256 CUs), per kernel and precision, over every shape, family and (ReLU, residual):
  ap_conv2d_nhwc, every configuration of its precision (they agree bitwise; 14 / -1 differ on the slab shapes, same maxima):
      fp32    1x1 0.0654   1x1/2 0.0334   3x3 0.0095   3x3/2 0.0056       (conv_pipe 0..13, conv_igemm 100 / -1; 14, 17 -> 11)
      bf16    1x1 0.9942   1x1/2 0.9749   3x3 0.9836   3x3/2 0.9676       (+ conv_slab 14 / -1, conv_lean 17)
      f16     1x1 0.9852   1x1/2 0.9565   3x3 0.9305   3x3/2 0.8803
      bf16x2  1x1 0.1894   1x1/2 0.1697   3x3 0.0567   3x3/2 0.0527
  conv_pw_kernel            bf16 0.9917   f16 0.9651;   3x3/2 form  bf16 0.9633   f16 0.8437;   ds form  bf16 0.9885   f16 0.9546
  conv_img3_kernel          bf16 0.9680   f16 0.8633
  conv_s2p_kernel           bf16 0.9658   f16 0.8583
  conv_pair_kernel          out  bf16 0.9938   f16 0.9805;   t1n (on the stored out)  bf16 0.9666   f16 0.8160
  conv_pair_kernel (ds)     out  bf16 0.9853   f16 0.9355;   t1n (on the stored out)  bf16 0.9628   f16 0.8078
  bottleneck2 (identity, tail: bit-equal to the chain)   chain stages  bf16 0.9928   f16 0.9774
  bottleneck2 (downsample, propagated bound)             bf16 0.0573   f16 0.0515
  block_img (bit-equal to the chain)                     chain stages  bf16 0.9776   f16 0.9096
As in the stem file, the 16-bit ratios near 1 are the stored type's rounding alone (u |ref| is the half-ulp of a value at the
bottom of its binade); the CPU emulation, which shares only that rounding with the kernels, measures the same (bf16 0.994,
f16 0.988), and with fp32 storage the accumulation uses 0.07 of gamma A.  No refusal occurred.  The whole file takes 7 s on the
MI355X (test_stem_pool_fp64.py: 37 s), no test more than 0.4 s (77 GPU tests).
"""

PRECS = ("fp32", "bf16", "f16", "bf16x2")
FAMILIES = ("randn", "alt", "frame", "impulse")
VARIANTS = ((1, 0), (1, 1), (0, 0), (0, 1))                  # (relu, residual)
SPLIT_CFGS = (-1, 11, 12, 100)
REFUSALS = {}                                                # (precision, configuration, shape name) -> documented reason: none
PAD_SCALE, PAD_SHIFT = 777.0, -555.0


def gamma(K, prec):
    return ((3 * K if prec == "bf16x2" else K) + 3) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ inputs
def _image(kind, H, W, C, gen, k):
    if kind == "randn":
        return torch.randn(H, W, C, generator=gen)
    if kind in ("plus", "minus"):
        return torch.full((H, W, C), 4.0 if kind == "plus" else -4.0)
    if kind == "frame":
        # 8 (1 + 6.9 2^-10): rounding to nearest moves it up in bf16 (0.86 of a 2^-7 step) and in fp16 (6.9 -> 7 steps), truncation down
        v = 8.0 * (1.0 + 6.9 * 2.0 ** -10) * (torch.randint(0, 2, (H, W, C), generator=gen).float() * 2 - 1)
        x = torch.zeros(H, W, C)
        for sl in ((slice(None), slice(0, 1)), (slice(None), slice(W - 1, W)), (slice(0, 1), slice(None)), (slice(H - 1, H), slice(None))):
            x[sl[0], sl[1]] = v[sl[0], sl[1]]
        return x
    if kind == "impulse":
        x = torch.zeros(H, W, C)
        spots = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, (W - 1) // 2), ((H - 1) // 2, W - 1))
        for j, (iy, ix) in enumerate(spots):
            x[iy, ix, (7 * j + k) % C] = (2.0, -3.0, 1.5)[(j + k // 3) % 3]
        return x
    raise ValueError(kind)


def make_input(N, H, W, C, family, seed):
    """[N][H][W][C] fp32; family: one of FAMILIES ("alt": image k all +4, image k + 1 all -4)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    kinds = [("plus" if k % 2 == 0 else "minus") if family == "alt" else family for k in range(N)]
    return torch.stack([_image(kd, H, W, C, gen, k) for k, kd in enumerate(kinds)])


def make_weight(Cout, k, Cin, seed):
    """[Cout][k][k][Cin] fp32 (K-contiguous rows)"""
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(Cout, k, k, Cin, generator=gen) * (2.0 / (k * k * Cin)) ** 0.5


def make_bn(C, seed):
    """Five regimes per channel under a seeded permutation: 0 ordinary (scale in [.5, 1.5], |shift| in [.05, .15]), 1 negative
    scale, 2 shift exactly 0, 3 shift << 0 (regions exactly 0 after the ReLU), 4 shift >> 0 (nothing clipped)"""
    gen = torch.Generator().manual_seed(3000 + seed)
    perm = torch.randperm(C, generator=gen)
    scale = torch.rand(C, generator=gen) + 0.5
    shift = (0.05 + 0.1 * torch.rand(C, generator=gen)) * (torch.randint(0, 2, (C,), generator=gen).float() * 2 - 1)
    reg = torch.empty(C, dtype=torch.long)
    reg[perm] = torch.arange(C) % 5
    scale[reg == 1] *= -1.0
    shift[reg == 2] = 0.0
    shift[reg == 3] = -3.0 - 3.0 * torch.rand(int((reg == 3).sum()), generator=gen)
    shift[reg == 4] = 20.0 + 20.0 * torch.rand(int((reg == 4).sum()), generator=gen)
    return scale, shift


def make_res(shape, seed):
    gen = torch.Generator().manual_seed(5000 + seed)
    return torch.randn(*shape, generator=gen)


# ------------------------------------------------------------------------------------------------ reference and bars
def conv_sums(xv, wv, stride, pad):
    """fp64 (conv(x, w), conv(|x|, |w|)), channels last; xv [N][H][W][Cin], wv [Cout][k][k][Cin]: the values the kernel sees"""
    xd, wd = xv.double().permute(0, 3, 1, 2), wv.double().permute(0, 3, 1, 2)
    c = F.conv2d(xd, wd, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    a = F.conv2d(xd.abs(), wd.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    return c, a


def finish(c, a, scale, shift, resv, relu, prec, K, extra=None):
    """(ref, bound) from the two sums; extra: a propagated term (>= 0) added to the bound"""
    s, h = scale.double(), shift.double()
    ref, A = c * s + h, s.abs() * a + h.abs()
    if resv is not None:
        ref, A = ref + resv.double(), A + resv.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    bound = U[prec] * ref.abs() + gamma(K, prec) * A
    if extra is not None:
        bound = bound + extra
    return ref, torch.where(bound > 0, bound + U_ABS[prec], bound)


def stage(xv, wv, scale, shift, resv, relu, stride, pad, prec, extra_in=None):
    """One conv + BN (+ res) (+ ReLU) stage on the values xv: (ref, bound).  extra_in: bound on the error of xv itself (a hidden
    intermediate), propagated as |scale| conv(extra_in, |w|)."""
    c, a = conv_sums(xv, wv, stride, pad)
    extra = None
    if extra_in is not None:
        e = F.conv2d(extra_in.double().permute(0, 3, 1, 2), wv.double().abs().permute(0, 3, 1, 2), stride=stride, padding=pad)
        extra = scale.double().abs() * e.permute(0, 2, 3, 1)
    return finish(c, a, scale, shift, resv, relu, prec, wv.shape[1] * wv.shape[2] * wv.shape[3], extra)


def drift(ref, bound, prec):
    """d_m of the docstring for a hidden intermediate whose pre-rounding bound is `bound` - u |ref| (both rounded to storage)"""
    return bound + U[prec] * ref.abs() + U_ABS[prec]


# ------------------------------------------------------------------------------------------------ shapes of ap_conv2d_nhwc
#          name          N  H    W   Cin  Cout k  s  p
SHAPES = [("p1_tiny",    1, 5,   3,  64,  8,   1, 1, 0),
          ("p1_m127",    1, 1,   127, 64, 72,  1, 1, 0),
          ("p1_m128",    2, 4,   16, 64,  136, 1, 1, 0),
          ("p1_m129",    1, 3,   43, 64,  192, 1, 1, 0),
          ("p1_m255",    3, 5,   17, 128, 8,   1, 1, 0),
          ("p1_m256",    2, 8,   16, 64,  72,  1, 1, 0),
          ("p1_m257",    1, 257, 1,  64,  136, 1, 1, 0),
          ("p1_c136",    1, 3,   43, 64,  136, 1, 1, 0),
          ("p1_k192",    1, 7,   19, 192, 72,  1, 1, 0),
          ("p1_lean",    1, 3,   43, 128, 520, 1, 1, 0),
          ("p1_s2",      2, 7,   5,  64,  72,  1, 2, 0),
          ("r3_5x9",     2, 5,   9,  64,  72,  3, 1, 1),
          ("r3_9x5",     2, 9,   5,  64,  136, 3, 1, 1),
          ("r3_1x7",     3, 1,   7,  64,  8,   3, 1, 1),
          ("r3_7x1",     3, 7,   1,  64,  8,   3, 1, 1),
          ("r3_2x2",     2, 2,   2,  64,  192, 3, 1, 1),
          ("r3_w29",     2, 3,   29, 64,  72,  3, 1, 1),
          ("r3_w30",     2, 3,   30, 64,  72,  3, 1, 1),
          ("r3_w31",     2, 3,   31, 64,  72,  3, 1, 1),
          ("r3_7tiles",  3, 9,   29, 64,  136, 3, 1, 1),
          ("r3_k128",    1, 5,   9,  128, 72,  3, 1, 1),
          ("r3_5img",    5, 6,   6,  64,  72,  3, 1, 1),
          ("r3s2_h7",    2, 7,   7,  64,  72,  3, 2, 1),
          ("r3s2_h6",    2, 6,   6,  128, 8,   3, 2, 1),
          ("r3s2_7x10",  1, 7,   10, 64,  136, 3, 2, 1)]
SHAPE_FP32_ONLY = ("p1_c4", 1, 3, 43, 64, 4, 1, 1, 0)
# the family every shape runs on the GPU besides "randn" (the CPU self-check runs all four on every shape)
GPU_FAMILY = {"r3_5img": "alt", "r3_7tiles": "alt", "p1_m255": "alt", "p1_m128": "alt", "p1_s2": "alt"}


def shapes_of(prec):
    return SHAPES + ([SHAPE_FP32_ONLY] if prec == "fp32" else [])


_CASES = {}


def case(prec, shp, family):
    """The operands of (precision, shape, family) as the kernel sees them, and the two fp64 sums: computed once, then shared"""
    key = (prec, shp[0], family)
    if key not in _CASES:
        name, N, H, W, Cin, Cout, k, s, p = shp
        seed = sum(ord(ch) for ch in name) + 31 * FAMILIES.index(family)
        xv = operands(make_input(N, H, W, Cin, family, seed), prec)
        wv = operands(make_weight(Cout, k, Cin, seed), prec)
        scale, shift = make_bn(Cout, seed)
        c, a = conv_sums(xv, wv, s, p)
        resv = operands(make_res(tuple(c.shape), seed), prec)
        _CASES[key] = dict(xv=xv, wv=wv, scale=scale, shift=shift, resv=resv, c=c, a=a, K=k * k * Cin)
    return _CASES[key]


def case_ref(cs, relu, res, prec):
    return finish(cs["c"], cs["a"], cs["scale"], cs["shift"], cs["resv"] if res else None, relu, prec, cs["K"])


# ------------------------------------------------------------------------------------------------ CPU self-check
MUTATIONS = {            # mutation -> (shape it must be rejected on, family)
    "drop_right":     ("r3_5x9", "randn"),      # one tap dropped where it reads the right border column only
    "swap_hw":        ("r3_9x5", "randn"),      # H and W swapped in the border mask
    "carry_halo":     ("r3_5img", "alt"),       # the first halo row of image k + 1 taken from image k
    "trunc_store":    ("p1_m129", "randn"),     # storage truncated instead of rounded (16-bit types)
    "res_after_relu": ("p1_m129", "randn"),     # the residual added after the ReLU
    "abs_scale":      ("p1_m129", "randn"),     # |scale| used for scale
    "shift_nbr":      ("p1_c136", "randn"),     # the shift of a channel of the Cout tail tile taken from its neighbour
    "skip_k":         ("r3_k128", "randn"),     # one chunk of 64 channels skipped on the last K step
}


def emulate(xv, wv, scale, shift, resv, relu, stride, pad, prec, mut=None, seed=0):
    """fp32 emulation, tap by tap over the flat pixel index n H W + hi W + wi as the kernels address it (a tap outside the image is
    masked, its address clamped into the tensor): fp32 GEMM per tap -> BatchNorm -> + res -> ReLU -> storage rounding."""
    gen = torch.Generator().manual_seed(4000 + seed)
    N, H, W, Cin = xv.shape
    Cout, k = wv.shape[0], wv.shape[1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xf, wv, scale, shift = xv.reshape(N * H * W, Cin), wv.clone(), scale.clone(), shift.clone()
    if mut == "skip_k":
        wv[:, k - 1, k - 1, Cin - 64:] = 0.0
    if mut == "abs_scale":
        scale = scale.abs()
    if mut == "shift_nbr":
        tail = [c for c in range(Cout // 128 * 128 + 1, Cout) if shift[c] != shift[c - 1]]
        c = tail[int(torch.randint(0, len(tail), (1,), generator=gen))]
        shift[c] = shift[c - 1]
    n, ho, wo = torch.meshgrid(torch.arange(N), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    n, ho, wo = n.reshape(-1), ho.reshape(-1), wo.reshape(-1)
    Hm, Wm = (W, H) if mut == "swap_hw" else (H, W)
    drop = None
    if mut == "drop_right":                                  # a tap that reads column W - 1 for some output column
        cand = [s for s in range(k) if bool(((wo * stride - pad + s) == W - 1).any())]
        drop = (int(torch.randint(0, k, (1,), generator=gen)), cand[-1])
    acc = torch.zeros(N * Ho * Wo, Cout)
    for r in range(k):
        for s in range(k):
            hi, wi = ho * stride - pad + r, wo * stride - pad + s
            ok = (hi >= 0) & (hi < Hm) & (wi >= 0) & (wi < Wm)
            if drop == (r, s):
                ok = ok & (wi != W - 1)
            if mut == "carry_halo" and r == 0:
                ok = ok | ((n >= 1) & (hi == -1) & (wi >= 0) & (wi < W))
            idx = (n * H * W + hi * W + wi).clamp(0, N * H * W - 1)
            acc += (xf[idx] * ok[:, None].float()) @ wv[:, r, s, :].t()
    y = acc * scale + shift
    rv = resv.reshape(-1, Cout) if resv is not None else None
    if mut == "res_after_relu":
        y = y.clamp_min(0) + rv
    else:
        if rv is not None:
            y = y + rv
        if relu:
            y = y.clamp_min(0)
    return operands(y, prec, trunc=(mut == "trunc_store")).view(N, Ho, Wo, Cout)


@pytest.mark.parametrize("prec", PRECS)
def test_cpu_emulation_is_inside_the_bars_and_mutations_are_not(prec):
    """The fp32 emulation stays inside every bar on every shape x family x (ReLU, residual); each mutation is rejected."""
    ratios = {}
    saw_zero_bound = False
    for shp in shapes_of(prec):
        for family in FAMILIES:
            cs = case(prec, shp, family)
            for relu, res in VARIANTS:
                ref, bound = case_ref(cs, relu, res, prec)
                got = emulate(cs["xv"], cs["wv"], cs["scale"], cs["shift"], cs["resv"] if res else None, relu, shp[7], shp[8], prec)
                check("%s %s %s relu=%d res=%d" % (prec, shp[0], family, relu, res), family, got, ref, bound, ratios)
                saw_zero_bound |= bool((bound == 0).any())
    assert saw_zero_bound                                    # frame / impulse interiors, shift exactly 0, no residual
    by_name = {s[0]: s for s in shapes_of(prec)}
    for mut, (name, family) in MUTATIONS.items():
        if mut == "trunc_store" and prec not in DT16:
            continue                                         # fp32 stores what it computed; a truncated hi part is made up by its lo part
        shp = by_name[name]
        cs = case(prec, shp, family)
        ref, bound = case_ref(cs, 1, 1, prec)
        got = emulate(cs["xv"], cs["wv"], cs["scale"], cs["shift"], cs["resv"], 1, shp[7], shp[8], prec, mut=mut, seed=11)
        ok, ratio, nz, _ = evaluate(got, ref, bound)
        assert not ok, (prec, mut, "the checker accepts this mutation: worst err / bound %.3f" % ratio)
        ratios["!" + mut] = ratio
    report("emulation " + prec, ratios)


def test_shape_list_has_the_properties_the_kernels_need():
    """The shape list against the tile constants it is built around (host only)."""
    M = {s[0]: s[1] * ((s[2] + 2 * s[8] - s[6]) // s[7] + 1) * ((s[3] + 2 * s[8] - s[6]) // s[7] + 1) for s in SHAPES}
    assert [M["p1_m%d" % m] for m in (127, 128, 129, 255, 256, 257)] == [127, 128, 129, 255, 256, 257] and M["p1_tiny"] < 64
    assert all(s[2] != s[3] for s in SHAPES if s[0].startswith("p1_m"))
    assert {s[5] for s in SHAPES} >= {8, 72, 136, 192, 520} and SHAPE_FP32_ONLY[5] == 4
    assert {s[4] for s in SHAPES if s[6] == 1} >= {64, 128, 192} and {s[4] for s in SHAPES if s[6] == 3} >= {64, 128}
    assert {(s[2], s[3]) for s in SHAPES if s[6] == 3 and s[7] == 1} >= {(5, 9), (9, 5), (1, 7), (7, 1), (2, 2)}
    assert {s[3] for s in SHAPES if s[6] == 3 and s[7] == 1} >= {29, 30, 31}         # 128 + 2 W + 2 <= 190 holds up to W = 30
    assert M["r3_7tiles"] > 6 * 128 and M["r3_5img"] > 128 > 3 * 36
    assert not REFUSALS


# ------------------------------------------------------------------------------------------------ GPU side
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from airpose_amd import _native as Nn
    return Nn, Nn.lib()


def _pad_rows(v, rows, fill=0.0):
    """v [C][...] -> [rows][...] with the padding rows filled"""
    out = torch.full((rows,) + tuple(v.shape[1:]), fill, dtype=v.dtype)
    out[:v.shape[0]] = v
    return out


def _cpad(C):
    return (C + 127) // 128 * 128


def _bn_dev(scale, shift, dev):
    C = scale.shape[0]
    return _pad_rows(scale, _cpad(C), PAD_SCALE).to(dev), _pad_rows(shift, _cpad(C), PAD_SHIFT).to(dev)


def _w_dev(wv, prec, dev):
    """[Cout][k][k][Cin] values -> the padded K-contiguous rows in the storage of prec"""
    return _to_storage(_pad_rows(wv, _cpad(wv.shape[0])), prec, dev)[0]


def _guards_ok(g):
    G = g.GUARD
    return bool(torch.isnan(g.buf[:G]).all() and torch.isnan(g.buf[G + g.m:]).all())


def conv2d(dev, prec, xd, wd, sd, hd, rd, N, H, W, Cin, Cout, k, stride, pad, relu):
    """ap_conv2d_nhwc into a guarded buffer: (status, Guarded, output shape)"""
    Nn, L = _lib()
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = Guarded(dev, prec, N * Ho * Wo * Cout)
    rc = L.ap_conv2d_nhwc(Nn.PRECISIONS[prec], _p(xd), _p(wd), _p(sd), _p(hd), _p(rd), _p(g.out), N, H, W, Cin, Cout, k, stride, pad,
                          int(relu), Nn.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, g, (N, Ho, Wo, Cout)


@gpu
@pytest.mark.parametrize("prec,cfg", [(pr, c) for pr in ("fp32", "bf16") for c in ALL_CFGS] + [("f16", c) for c in F16_CFGS] +
                         [("bf16x2", c) for c in SPLIT_CFGS])
def test_conv2d_every_configuration(dev, prec, cfg):
    """ap_conv2d_nhwc under one configuration on every shape of the list: "randn" and a second family per shape, ReLU and residual
    on and off, element-wise against fp64."""
    Nn, L = _lib()
    ratios = {}
    Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
    try:
        for si, shp in enumerate(shapes_of(prec)):
            name, N, H, W, Cin, Cout, k, s, p = shp
            for fi, family in enumerate(("randn", GPU_FAMILY.get(name, FAMILIES[1 + si % 3]))):
                cs = case(prec, shp, family)
                xd = _to_storage(cs["xv"], prec, dev)[0]
                wd = _w_dev(cs["wv"], prec, dev)
                sd, hd = _bn_dev(cs["scale"], cs["shift"], dev)
                rd = _to_storage(cs["resv"], prec, dev)[0]
                for relu, res in (VARIANTS if fi == 0 else VARIANTS[si % 2::2]):
                    what = "%s cfg=%d %s %s relu=%d res=%d" % (prec, cfg, name, family, relu, res)
                    rc, g, oshape = conv2d(dev, prec, xd, wd, sd, hd, rd if res else None, N, H, W, Cin, Cout, k, s, p, relu)
                    if rc != 0:
                        assert (prec, cfg, name) in REFUSALS, (what, "undocumented refusal, status %d" % rc)
                        assert torch.isnan(g.buf.float()).all(), (what, "refused, but the output buffer was written")
                        continue
                    ref, bound = case_ref(cs, relu, res, prec)
                    check(what, "k%ds%d" % (k, s), g.values(oshape, what).cpu(), ref, bound, ratios)
    finally:
        L.ap_set_conv_config(-1)
    report("ap_conv2d_nhwc %s cfg=%d" % (prec, cfg), ratios)


# ---- the specialised kernels (16-bit storage) at their smallest shapes
P16 = ("bf16", "f16")


def _rows16(v, prec, dev):
    return v.to(DT16[prec]).contiguous().to(dev)


def _untile(t, M, C):
    """fragment-tiled [M/16][C/8][16 pixels][8 channels] -> [M][C]"""
    return t.view(M // 16, C // 8, 16, 8).permute(0, 2, 1, 3).reshape(M, C)


def _generic_bits(dev, prec, xd, wd, sd, hd, rd, N, H, W, Cin, Cout, k, stride, pad, relu=1):
    rc, g, oshape = conv2d(dev, prec, xd, wd, sd, hd, rd, N, H, W, Cin, Cout, k, stride, pad, relu)
    assert rc == 0
    g.values(oshape, "ap_conv2d_nhwc")
    return g.bits()


@gpu
@pytest.mark.parametrize("prec", P16)
def test_conv_pw(dev, prec):
    """ap_conv_pw_nhwc at M = 196 and 392 (7 x 7 images in fours), Cin 256, Cout 256 and 512, with and without identity: against
    fp64, and bit for bit against ap_conv2d_nhwc as the header documents."""
    Nn, L = _lib()
    ratios = {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    Cin = 256
    for M in (196, 392):
        for Cout in (256, 512):
            wv = operands(make_weight(Cout, 1, Cin, M + Cout), prec)
            scale, shift = make_bn(Cout, M + Cout)
            wd = _rows16(wv.reshape(Cout, Cin), prec, dev)
            ws = torch.empty(L.ap_conv_pw_stream_bytes(Cin, Cout), dtype=torch.uint8, device=dev)
            Nn.check(L.ap_conv_pw_pack(PR, _p(wd), Cin, Cout, _p(ws), st), "ap_conv_pw_pack")
            sd, hd = scale.to(dev), shift.to(dev)
            for fi, family in enumerate(FAMILIES):
                xv = operands(make_input(M // 49, 7, 7, Cin, family, M + fi), prec)
                resv = operands(make_res((M // 49, 7, 7, Cout), M + fi), prec)
                xd, rd = _rows16(xv, prec, dev), _rows16(resv, prec, dev)
                for ident in (0, 1):
                    what = "conv_pw %s M=%d Cout=%d %s identity=%d" % (prec, M, Cout, family, ident)
                    g = Guarded(dev, prec, M * Cout)
                    Nn.check(L.ap_conv_pw_nhwc(PR, _p(xd), _p(ws), _p(sd), _p(hd), _p(rd) if ident else None, _p(g.out), M, Cin, Cout, st), what)
                    torch.cuda.synchronize()
                    ref, bound = stage(xv, wv, scale, shift, resv if ident else None, 1, 1, 0, prec)
                    check(what, family, g.values(tuple(ref.shape), what).cpu(), ref, bound, ratios)
                    want = _generic_bits(dev, prec, xd, wd, sd, hd, rd if ident else None, M // 49, 7, 7, Cin, Cout, 1, 1, 0)
                    assert torch.equal(g.bits(), want), (what, "differs from ap_conv2d_nhwc")
    report("conv_pw_kernel " + prec, ratios)


@gpu
@pytest.mark.parametrize("prec", P16)
def test_conv_pw_ds(dev, prec):
    """ap_conv_pw_ds_nhwc (second K segment read at the strided pixel) at (N, Ho) = (4, 7) and (1, 14): against fp64 on [t2 | x sampled]"""
    Nn, L = _lib()
    ratios = {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    Cout = 256
    for N, Ho in ((4, 7), (1, 14)):
        for Cin, Cin2 in ((128, 128), (64, 192)):
            wv = operands(make_weight(Cout, 1, Cin + Cin2, N + Cin), prec)
            scale, shift = make_bn(Cout, N + Cin)
            wd = _rows16(wv.reshape(Cout, Cin + Cin2), prec, dev)
            ws = torch.empty(L.ap_conv_pw_stream_bytes(Cin + Cin2, Cout), dtype=torch.uint8, device=dev)
            Nn.check(L.ap_conv_pw_pack(PR, _p(wd), Cin + Cin2, Cout, _p(ws), st), "ap_conv_pw_pack")
            sd, hd = scale.to(dev), shift.to(dev)
            for fi, family in enumerate(FAMILIES):
                what = "conv_pw_ds %s N=%d Ho=%d Cin=%d+%d %s" % (prec, N, Ho, Cin, Cin2, family)
                t2v = operands(make_input(N, Ho, Ho, Cin, family, 7 * N + fi), prec)
                xv = operands(make_input(N, 2 * Ho, 2 * Ho, Cin2, FAMILIES[(fi + 1) % 4], 9 * N + fi), prec)
                g = Guarded(dev, prec, N * Ho * Ho * Cout)
                t2d, xd = _rows16(t2v, prec, dev), _rows16(xv, prec, dev)
                Nn.check(L.ap_conv_pw_ds_nhwc(PR, _p(t2d), _p(xd), _p(ws), _p(sd), _p(hd), _p(g.out),
                                              N, Ho, Cin, Cin2, Cout, 2, st), what)
                torch.cuda.synchronize()
                ref, bound = stage(torch.cat([t2v, xv[:, ::2, ::2, :]], 3), wv, scale, shift, None, 1, 1, 0, prec)
                check(what, family, g.values(tuple(ref.shape), what).cpu(), ref, bound, ratios)
    report("conv_pw_kernel (ds) " + prec, ratios)


@gpu
@pytest.mark.parametrize("prec", P16)
def test_conv_pw_k3s2(dev, prec):
    """ap_conv_pw_k3s2_nhwc at H = 14 (N = 4) and H = 28 (N = 1), the smallest N allowed: against fp64, and bit for bit against
    ap_conv2d_nhwc(3, 2, 1) as the header documents."""
    Nn, L = _lib()
    ratios = {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    Cin, Cout = 128, 256
    wv = operands(make_weight(Cout, 3, Cin, 77), prec)
    scale, shift = make_bn(Cout, 77)
    wd = _rows16(wv.reshape(Cout, 9 * Cin), prec, dev)
    ws = torch.empty(L.ap_conv_pw_stream_bytes(9 * Cin, Cout), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_pw_pack(PR, _p(wd), 9 * Cin, Cout, _p(ws), st), "ap_conv_pw_pack")
    sd, hd = scale.to(dev), shift.to(dev)
    for N, H in ((4, 14), (1, 28)):
        for fi, family in enumerate(FAMILIES):
            what = "conv_pw_k3s2 %s N=%d H=%d %s" % (prec, N, H, family)
            xv = operands(make_input(N, H, H, Cin, family, H + fi), prec)
            xd = _rows16(xv, prec, dev)
            g = Guarded(dev, prec, N * (H // 2) ** 2 * Cout)
            Nn.check(L.ap_conv_pw_k3s2_nhwc(PR, _p(xd), _p(ws), _p(sd), _p(hd), _p(g.out), N, H, Cin, Cout, st), what)
            torch.cuda.synchronize()
            ref, bound = stage(xv, wv, scale, shift, None, 1, 2, 1, prec)
            check(what, family, g.values(tuple(ref.shape), what).cpu(), ref, bound, ratios)
            want = _generic_bits(dev, prec, xd, wd, sd, hd, None, N, H, H, Cin, Cout, 3, 2, 1)
            assert torch.equal(g.bits(), want), (what, "differs from ap_conv2d_nhwc")
    report("conv_pw_kernel (3x3/2) " + prec, ratios)


@gpu
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("kernel", ["img3", "s2p"])
def test_conv_img3_and_s2p(dev, prec, kernel):
    """ap_conv_img3_nhwc (28 x 28, stride 1: the column where the two half images meet is the edge) and ap_conv_s2p_nhwc (56 x 56,
    stride 2: the quarter borders), N = 1 and 2, NHWC and fragment-tiled: against fp64."""
    Nn, L = _lib()
    ratios = {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    H, stride = (28, 1) if kernel == "img3" else (56, 2)
    nbytes, pack, run = ((L.ap_conv_img3_stream_bytes, L.ap_conv_img3_pack, L.ap_conv_img3_nhwc) if kernel == "img3" else
                         (L.ap_conv_s2p_stream_bytes, L.ap_conv_s2p_pack, L.ap_conv_s2p_nhwc))
    wv = operands(make_weight(128, 3, 128, 55 + stride), prec)
    scale, shift = make_bn(128, 55 + stride)
    ws = torch.empty(nbytes(), dtype=torch.uint8, device=dev)
    wd = _rows16(wv, prec, dev)
    Nn.check(pack(PR, _p(wd), _p(ws), st), "pack")
    sd, hd = scale.to(dev), shift.to(dev)
    for N in (1, 2):
        for fi, family in enumerate(FAMILIES):
            xv = operands(make_input(N, H, H, 128, family, 3 * N + fi), prec)
            xd = _rows16(xv, prec, dev)
            ref, bound = stage(xv, wv, scale, shift, None, 1, stride, 1, prec)
            M = N * 28 * 28
            for tiled in (0, 1):
                what = "conv_%s %s N=%d %s tiled=%d" % (kernel, prec, N, family, tiled)
                g = Guarded(dev, prec, M * 128)
                Nn.check(run(PR, _p(xd), _p(ws), _p(sd), _p(hd), _p(g.out), N, tiled, st), what)
                torch.cuda.synchronize()
                got = g.values((M, 128), what)
                got = _untile(got, M, 128) if tiled else got
                check(what, family, got.reshape(N, 28, 28, 128).cpu(), ref, bound, ratios)
    report("conv_%s_kernel %s" % (kernel, prec), ratios)


def _pair_stream(dev, prec, w3d, w1d, P, P2, N1):
    Nn, L = _lib()
    nb = L.ap_conv_pair_stream_bytes(P, P2, N1)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    Nn.check(L.ap_conv_pair_pack(Nn.PRECISIONS[prec], _p(w3d), _p(w1d) if N1 else None, P, P2, N1, _p(ws), Nn.stream_ptr(dev)), "ap_conv_pair_pack")
    return ws


@gpu
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("P,N1", [(128, 128), (128, 256), (256, 256)])
def test_conv_pair(dev, prec, P, N1):
    """ap_conv_pair_nhwc at M = 49, 196 and the ragged 5 * 49: `out` against fp64, `t1n` against fp64 on the kernel's own stored `out`"""
    Nn, L = _lib()
    r_out, r_t1 = {}, {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    C3 = 4 * P
    w3v, w1v = operands(make_weight(C3, 1, P, P + N1), prec), operands(make_weight(N1, 1, C3, P + N1 + 1), prec)
    (s3, h3), (s1, h1) = make_bn(C3, P + N1), make_bn(N1, P + N1 + 1)
    ws = _pair_stream(dev, prec, _rows16(w3v.reshape(C3, P), prec, dev), _rows16(w1v.reshape(N1, C3), prec, dev), P, 0, N1)
    dv = [t.to(dev) for t in (s3, h3, s1, h1)]
    for M in (49, 196, 245):
        for fi, family in enumerate(FAMILIES):
            what = "conv_pair %s P=%d N1=%d M=%d %s" % (prec, P, N1, M, family)
            t2v = operands(make_input(M // 49, 7, 7, P, family, M + fi), prec)
            resv = operands(make_res((M // 49, 7, 7, C3), M + fi), prec)
            go, gt = Guarded(dev, prec, M * C3), Guarded(dev, prec, M * N1)
            t2d, rd = _rows16(t2v, prec, dev), _rows16(resv, prec, dev)
            Nn.check(L.ap_conv_pair_nhwc(PR, _p(t2d), _p(ws), _p(dv[0]), _p(dv[1]), _p(rd), _p(dv[2]),
                                         _p(dv[3]), _p(go.out), _p(gt.out), M, P, N1, st), what)
            torch.cuda.synchronize()
            ref, bound = stage(t2v, w3v, s3, h3, resv, 1, 1, 0, prec)
            out = go.values(tuple(ref.shape), what).cpu()
            check(what, family, out, ref, bound, r_out)
            ref1, bound1 = stage(out, w1v, s1, h1, None, 1, 1, 0, prec)
            check(what + " t1n", family, gt.values(tuple(ref1.shape), what).cpu(), ref1, bound1, r_t1)
    report("conv_pair_kernel out %s (%d, %d)" % (prec, P, N1), r_out)
    report("conv_pair_kernel t1n %s (%d, %d)" % (prec, P, N1), r_t1)


@gpu
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("P,P2,N1", [(128, 256, 128), (256, 512, 0)])
def test_conv_pair_ds(dev, prec, P, P2, N1):
    """ap_conv_pair_ds_nhwc (w3 = [conv3 | downsample], scales folded: s3 = 1) at M = 49, 196 and 5 * 49: `out` against fp64 on
    [t2 | x sampled], `t1n` against fp64 on the kernel's own stored `out`"""
    Nn, L = _lib()
    r_out, r_t1 = {}, {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    C3 = 4 * P
    w3v = operands(make_weight(C3, 1, P + P2, P + 3), prec)
    w1v = operands(make_weight(max(N1, 8), 1, C3, P + 4), prec)
    s3, h3 = torch.ones(C3), make_bn(C3, P + 3)[1]
    s1, h1 = make_bn(max(N1, 8), P + 4)
    ws = _pair_stream(dev, prec, _rows16(w3v.reshape(C3, P + P2), prec, dev), _rows16(w1v.reshape(-1, C3), prec, dev), P, P2, N1)
    dv = [t.to(dev) for t in (s3, h3, s1, h1)]
    for N, Ho in ((1, 7), (1, 14), (5, 7)):
        for fi, family in enumerate(FAMILIES):
            what = "conv_pair_ds %s P=%d N=%d Ho=%d %s" % (prec, P, N, Ho, family)
            M = N * Ho * Ho
            t2v = operands(make_input(N, Ho, Ho, P, family, M + fi), prec)
            xv = operands(make_input(N, 2 * Ho, 2 * Ho, P2, FAMILIES[(fi + 1) % 4], M + fi + 50), prec)
            go, gt = Guarded(dev, prec, M * C3), Guarded(dev, prec, M * max(N1, 8))
            t2d, xd = _rows16(t2v, prec, dev), _rows16(xv, prec, dev)
            Nn.check(L.ap_conv_pair_ds_nhwc(PR, _p(t2d), _p(xd), _p(ws), _p(dv[0]), _p(dv[1]),
                                            _p(dv[2]) if N1 else None, _p(dv[3]) if N1 else None, _p(go.out), _p(gt.out) if N1 else None,
                                            N, Ho, P, P2, 2, N1, st), what)
            torch.cuda.synchronize()
            ref, bound = stage(torch.cat([t2v, xv[:, ::2, ::2, :]], 3), w3v, s3, h3, None, 1, 1, 0, prec)
            out = go.values(tuple(ref.shape), what).cpu()
            check(what, family, out, ref, bound, r_out)
            if N1:
                ref1, bound1 = stage(out, w1v, s1, h1, None, 1, 1, 0, prec)
                check(what + " t1n", family, gt.values(tuple(ref1.shape), what).cpu(), ref1, bound1, r_t1)
    report("conv_pair_kernel (ds) out %s P=%d" % (prec, P), r_out)
    if N1:
        report("conv_pair_kernel (ds) t1n %s P=%d" % (prec, P), r_t1)


class Block(object):
    """The operands of one bottleneck (planes, Cin -> 4 planes) and its stage-by-stage chain through ap_conv2d_nhwc, each stage of
    which is held against fp64 on its own stored input"""

    def __init__(self, dev, prec, planes, cin, seed, cin2=0):
        self.dev, self.prec, self.planes, self.cin, self.cin2 = dev, prec, planes, cin, cin2
        self.w = [operands(make_weight(planes, 1, cin, seed), prec), operands(make_weight(planes, 3, planes, seed + 1), prec),
                  operands(make_weight(4 * planes, 1, planes + cin2, seed + 2), prec)]
        self.bn = [make_bn(planes, seed), make_bn(planes, seed + 1), make_bn(4 * planes, seed + 2)]
        if cin2:
            self.bn[2] = (torch.ones(4 * planes), self.bn[2][1])                   # both BatchNorm scales are folded into the rows
        self.wd = [_w_dev(w, prec, dev) for w in self.w]
        self.bnd = [_bn_dev(s, h, dev) for s, h in self.bn]

    def chain(self, xv, what, ratios):
        """conv1 -> conv2 -> conv3 (+ x) through ap_conv2d_nhwc (identity form): the bits of the block output"""
        N, H, W, _ = xv.shape
        pl, dev, prec = self.planes, self.dev, self.prec
        xd = _rows16(xv, prec, dev)
        cur_v, cur_d = xv, xd
        for i, (cin, cout, k, pad, res) in enumerate(((self.cin, pl, 1, 0, False), (pl, pl, 3, 1, False), (pl, 4 * pl, 1, 0, True))):
            rc, g, oshape = conv2d(dev, prec, cur_d, self.wd[i], self.bnd[i][0], self.bnd[i][1], xd if res else None, N, H, W, cin, cout, k, 1, pad, 1)
            assert rc == 0, (what, "chain stage %d refused" % (i + 1))
            ref, bound = stage(cur_v, self.w[i], self.bn[i][0], self.bn[i][1], xv if res else None, 1, 1, pad, prec)
            cur_v = g.values(oshape, what).cpu()
            check(what, "chain conv%d" % (i + 1), cur_v, ref, bound, ratios)
            cur_d = g.out
            keep = g
        return keep

    def args(self):
        a = []
        for i in range(3):
            a += [_p(self.wd[i]), _p(self.bnd[i][0]), _p(self.bnd[i][1])]
        return a


BNECK_SHAPES = ((1, 14, 14), (1, 14, 28), (2, 28, 14))


@gpu
@pytest.mark.parametrize("prec", P16)
def test_bottleneck64_identity(dev, prec):
    """ap_bottleneck64_nhwc, downsample = 0: the bits of conv1 -> conv2 -> conv3 (+ x) through ap_conv2d_nhwc, every stage of which
    is element-wise inside its fp64 bar on its own stored input: together an element-wise statement for the fused kernel."""
    Nn, L = _lib()
    ratios = {}
    blk = Block(dev, prec, 64, 256, 400)
    for N, H, W in BNECK_SHAPES:
        for fi, family in enumerate(FAMILIES):
            what = "bottleneck64 %s %dx%dx%d %s" % (prec, N, H, W, family)
            xv = operands(make_input(N, H, W, 256, family, H + W + fi), prec)
            want = blk.chain(xv, what, ratios)
            g = Guarded(dev, prec, N * H * W * 256)
            xd = _rows16(xv, prec, dev)
            Nn.check(L.ap_bottleneck64_nhwc(Nn.PRECISIONS[prec], _p(xd), *blk.args(), _p(g.out), N, H, W, 256, 0,
                                            Nn.stream_ptr(dev)), what)
            torch.cuda.synchronize()
            g.values((N, H, W, 256), what)
            assert torch.equal(g.bits(), want.bits()), (what, "%d values differ from the chain" % int((g.bits() != want.bits()).sum()))
    report("bottleneck2 (identity) chain " + prec, ratios)


@gpu
@pytest.mark.parametrize("prec", P16)
def test_bottleneck64_downsample(dev, prec):
    """ap_bottleneck64_nhwc, downsample = 1 (w3 = [conv3 | downsample], s3 = 1): two hidden 16-bit intermediates and no operator
    entry for the chain's last stage, so the propagated bound of the docstring, stage by stage."""
    Nn, L = _lib()
    ratios = {}
    blk = Block(dev, prec, 64, 64, 500, cin2=64)
    (s1, h1), (s2, h2), (s3, h3) = blk.bn
    for N, H, W in BNECK_SHAPES:
        for fi, family in enumerate(FAMILIES):
            what = "bottleneck64 ds %s %dx%dx%d %s" % (prec, N, H, W, family)
            xv = operands(make_input(N, H, W, 64, family, H + W + fi + 9), prec)
            m1, b1 = stage(xv, blk.w[0], s1, h1, None, 1, 1, 0, prec)
            m1q = m1.to(DT16[prec]).float()                  # rounded where the kernel rounds it
            d1 = drift(m1, b1, prec)
            m2, b2 = stage(m1q, blk.w[1], s2, h2, None, 1, 1, 1, prec, extra_in=d1)
            m2q = m2.to(DT16[prec]).float()
            d2 = drift(m2, b2, prec)
            extra_in = torch.cat([d2, torch.zeros_like(xv, dtype=torch.float64)], 3)
            ref, bound = stage(torch.cat([m2q, xv], 3), blk.w[2], s3, h3, None, 1, 1, 0, prec, extra_in=extra_in)
            g = Guarded(dev, prec, N * H * W * 256)
            xd = _rows16(xv, prec, dev)
            Nn.check(L.ap_bottleneck64_nhwc(Nn.PRECISIONS[prec], _p(xd), *blk.args(), _p(g.out), N, H, W, 64, 1,
                                            Nn.stream_ptr(dev)), what)
            torch.cuda.synchronize()
            check(what, family, g.values((N, H, W, 256), what).cpu(), ref, bound, ratios)
    report("bottleneck2 (downsample) " + prec, ratios)


@gpu
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("y_even", [0, 1])
def test_bottleneck64_tail(dev, prec, y_even):
    """ap_bottleneck64_tail_nhwc: y carries the bits of the chain (y_even = 1: at the even pixels, the others untouched), t1n the
    bits of ap_conv2d_nhwc on that y, which is held against fp64 on the stored y."""
    Nn, L = _lib()
    ratios = {}
    blk = Block(dev, prec, 64, 256, 600)
    w1n, (s1n, h1n) = operands(make_weight(128, 1, 256, 601), prec), make_bn(128, 601)
    w1nd, (s1nd, h1nd) = _w_dev(w1n, prec, dev), _bn_dev(s1n, h1n, dev)
    for N, H, W in ((1, 14, 14), (2, 28, 14)):
        for fi, family in enumerate(FAMILIES):
            what = "bottleneck64_tail %s y_even=%d %dx%dx%d %s" % (prec, y_even, N, H, W, family)
            xv = operands(make_input(N, H, W, 256, family, H + W + fi + 3), prec)
            want = blk.chain(xv, what, ratios)
            yv = want.values((N, H, W, 256), what).cpu()
            rc, gt_ref, oshape = conv2d(dev, prec, want.out, w1nd, s1nd, h1nd, None, N, H, W, 256, 128, 1, 1, 0, 1)
            assert rc == 0
            ref, bound = stage(yv, w1n, s1n, h1n, None, 1, 1, 0, prec)
            check(what, "chain conv1n", gt_ref.values(oshape, what).cpu(), ref, bound, ratios)
            gy, gt = Guarded(dev, prec, N * H * W * 256), Guarded(dev, prec, N * H * W * 128)
            xd = _rows16(xv, prec, dev)
            Nn.check(L.ap_bottleneck64_tail_nhwc(Nn.PRECISIONS[prec], _p(xd), *blk.args(), _p(gy.out), _p(w1nd), _p(s1nd),
                                                 _p(h1nd), _p(gt.out), y_even, N, H, W, Nn.stream_ptr(dev)), what)
            torch.cuda.synchronize()
            gt.values(oshape, what)
            assert torch.equal(gt.bits(), gt_ref.bits()), (what, "t1n differs from ap_conv2d_nhwc on the block output")
            assert _guards_ok(gy), (what, "a guard band of y was written")
            yb, wb = gy.bits().view(N, H, W, 256), want.bits().view(N, H, W, 256)
            if y_even:
                assert torch.equal(yb[:, ::2, ::2], wb[:, ::2, ::2]), (what, "y differs from the chain at the even pixels")
                yf = gy.out.view(N, H, W, 256)
                assert torch.isnan(yf[:, 1::2].float()).all() and torch.isnan(yf[:, :, 1::2].float()).all(), (what, "an odd pixel of y was written")
            else:
                assert torch.equal(yb, wb), (what, "y differs from the chain")
    report("bottleneck2 (tail) chain %s y_even=%d" % (prec, y_even), ratios)


@gpu
@pytest.mark.parametrize("prec", P16)
def test_block_img(dev, prec):
    """ap_block_img_nhwc, N = 1 and 2: the bits of conv1 -> conv2 -> conv3 (+ x) through ap_conv2d_nhwc (automatic configuration:
    conv2 on the slab kernel, whose K order the block kernel follows), every stage of which is held against fp64."""
    Nn, L = _lib()
    ratios = {}
    st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[prec]
    blk = Block(dev, prec, 256, 1024, 700)
    ws = torch.empty(L.ap_block_img_stream_bytes(), dtype=torch.uint8, device=dev)
    Nn.check(L.ap_block_img_pack(PR, _p(blk.wd[0]), _p(blk.wd[1]), _p(blk.wd[2]), _p(ws), st), "ap_block_img_pack")
    for N in (1, 2):
        for fi, family in enumerate(FAMILIES):
            what = "block_img %s N=%d %s" % (prec, N, family)
            xv = operands(make_input(N, 14, 14, 1024, family, 40 * N + fi), prec)
            want = blk.chain(xv, what, ratios)
            g = Guarded(dev, prec, N * 196 * 1024)
            b = blk.bnd
            xd = _rows16(xv, prec, dev)
            Nn.check(L.ap_block_img_nhwc(PR, _p(xd), _p(ws), _p(b[0][0]), _p(b[0][1]), _p(b[1][0]), _p(b[1][1]), _p(b[2][0]),
                                         _p(b[2][1]), _p(g.out), N, st), what)
            torch.cuda.synchronize()
            g.values((N, 14, 14, 1024), what)
            assert torch.equal(g.bits(), want.bits()), (what, "%d values differ from the chain" % int((g.bits() != want.bits()).sum()))
    report("block_img chain " + prec, ratios)
