"""Element-wise fp64 ground truth for the forms of the generic and pair kernels that only a trunk pass used to select, through the
operator entries of ABI 13 (include/airpose_hip.h).  Companion of test_conv_fwd_fp64.py, whose inputs (make_input / make_weight /
make_bn / make_res), reference (stage / finish / gamma), shape list and packing helpers it reuses, with Guarded / operands / check /
report of test_stem_pool_fp64.py.

Form -> entry -> test
  second K segment (folded downsample) of conv_pipe's 128-wide tiles and conv_igemm     ap_conv2d_fold_nhwc      test_fold
  fragment-tiled output of conv_slab / conv_pipe / conv_igemm                             ap_conv2d_tiled_nhwc     test_tiled, test_tiled_refusals
  pooling variant of conv_lean (conv3 + identity + ReLU + AvgPool2d(7))                   ap_conv2d_pool_nhwc      test_pool
  pair-kernel layouts (t2_tiled, res_tiled, out_tiled, out_even)                          ap_conv_pair_layout_nhwc test_pair_layouts[identity | ds]

Every output lies in a NaN-filled Guarded buffer of exactly the documented size: every element that must be written is written,
nothing else is (the pixels M .. ceil16(M) - 1 of a tiled tensor, the odd pixels under out_even), and no guard band is touched.

Bars (derived, none measured): those of test_conv_fwd_fp64.py, u |ref| + gamma(K) A (+ U_ABS), with K the contraction actually
run -- Cin + Cin2 for the fold.  The tiled output and the pair layouts are pure relayouts: their gather must equal the plain entry's
BITS, and the plain result is then held against fp64.  The pooling kernel pools the values it would have stored, so its reference
is the mean over the 49 pixels of finish()'s fp64 reference, and its bound the mean of the 49 element bounds plus the avg-pool bar
of test_stem_pool_fp64.py (50 2^-24 mean|x| + 2^-24 |ref|) on the stored magnitudes, which |ref| + bound bounds from above.

Fold and ap_conv_pw_ds_nhwc.  The header does not promise bit-equality between the two (it says so), so none is asserted here; both
are held against the same fp64 reference (test_conv_pw_ds for the other).

Documented refusals, each asserted with the buffer still all NaN; any other nonzero status fails the test:
  fold    AP_ESHAPE: configurations 2, 3, 6, 7, 9, 12, 13 (64-wide tiles; bf16x2: 12), and 12 as the automatic choice for Cout <= 64 on
          256 or more rows of tiles (test_automatic_choice_refusals); an x2 of 4 GiB or more (tests/test_abi.py: host only)
  tiled   AP_ESHAPE: AP_PREC_FP32, AP_PREC_BF16X2; configurations 4-7 and 17, and 17 as the automatic choice (the same test)
  pool    AP_ESHAPE for fp32 / bf16x2, Cin % 64, Cout % 8 (tests/test_abi.py: host only)
  pair    AP_ESHAPE for res_tiled with P2 > 0, out_even with out_tiled, out_even with N1 = 0

CPU self-check (no GPU): fp32 emulations of the four forms (the tiled scatter and gather; the fold's sampling; the pool's eight
partitions with the carry of a super-tile's third image; the even-pixel mask) sit inside every bar on every shape, and ten seeded
mutations are each rejected by the assertions the GPU tests use (MUTATIONS).

Measured on an MI355X: see MEASURED below.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from test_conv_fwd_fp64 import (GPU_FAMILY, SHAPES, VARIANTS, _bn_dev, _guards_ok, _pair_stream, _rows16, _w_dev, case, case_ref, conv2d,
                                conv_sums, emulate, finish, make_bn, make_input, make_res, make_weight, stage)
from test_gpu_parity import ALL_CFGS
from test_stem_pool_fp64 import DT16, Guarded, _to_storage, check, evaluate, operands, report

MEASURED = """
Worst err / bound on an MI355X (256 CUs), per form and precision (python -m pytest tests/test_trunk_forms_fp64.py -m gpu -s):
  ap_conv2d_fold_nhwc       fp32 0.0332   bf16 0.9914   f16 0.9753   bf16x2 0.1268   (stride2 1 and 2, every family pair; the configurations
                            that run agree bitwise: -1, 0, 1, 4, 5, 8, 10, 11, 14, 17, 100 in fp32, bf16 and f16 alike; bf16x2: -1, 11,
                            100 -- and 2, 3, 6, 7, 9, 12, 13 -- bf16x2: 12 -- refuse with AP_ESHAPE and the buffer untouched)
  ap_conv2d_tiled_nhwc      bf16 3x3 0.9869  3x3/2 0.9676  1x1 0.9929;  f16 3x3 0.9246  3x3/2 0.9009  1x1 0.9834  (the plain entry's bits under
                            -1, 11, 12, 14 and 100; the refusals of the docstring all occurred)
  ap_conv2d_pool_nhwc       bf16 0.6043   f16 0.4749   (bit-equal to ap_conv2d_nhwc + ap_avgpool_nhwc in all 36 cases with Cout = 256 or 512
                            per precision; images 2 and 5 of N = 6 equal the same image alone)
  ap_conv_pair_layout_nhwc  out  bf16 0.9918   f16 0.9766;   t1n (on the stored out)  bf16 0.9712   f16 0.8572  (the plain entries' results;
                            every layout carries their bits)
The 16-bit ratios near 1 are the stored type's rounding alone, as in test_conv_fwd_fp64.py; the CPU emulations measure the same
(fold bf16 0.9914, f16 0.9753; pool bf16 0.6043, f16 0.4749 -- the same bits).  The pooling bound is used to 0.6 because the mean of
49 half-ulp bounds is not reached by 49 independent roundings.  No undocumented refusal occurred and no kernel needed a change for this
file.  test_automatic_choice_refusals: under -1 both calls return AP_ESHAPE with the buffer untouched; under 11 the tiled call carries
ap_conv2d_nhwc's bits and the fold equals configuration 100 bit for bit.  29 GPU tests, 7 s together, none above 1 s; the 7 CPU tests
take 6 s.
"""

P16 = ("bf16", "f16")
PRECS = ("fp32", "bf16", "f16", "bf16x2")

# ------------------------------------------------------------------------------------------------ shape lists
FOLD_CH = ((64, 64, 136), (128, 64, 72), (64, 192, 256))     # (Cin, Cin2, Cout)
FOLD_NHO = ((1, 3), (3, 7), (2, 8))                          # M = 9 (fewer K chunks in flight than the ring is deep), 147 (two M tiles, the second ragged), 128
FOLD_WIDE = (0, 1, 4, 5, 8, 10, 11)                          # conv_pipe's 128-wide tiles
FOLD_NARROW = (2, 3, 6, 7, 9, 12, 13)                        # its 64-wide tiles: no second K segment
TILED_SHAPES = [s for s in SHAPES if s[6] == 3] + [s for s in SHAPES if s[0] in ("p1_m129", "p1_m257")]
TILED_CFGS = (-1, 11, 12, 14, 100)
TILED_REFUSED_CFGS = (4, 5, 6, 7, 17)
POOL_N = (1, 2, 4, 5, 6, 11)
POOL_CH = ((64, 256), (128, 72), (512, 136), (256, 512))     # (Cin, Cout)
POOL_FAMILIES = ("randn", "alt", "frame")
PAIR_NHO = ((1, 7), (5, 7), (1, 14))                         # M = 49, 245 (ragged for the micro-tile and for the workgroup), 196
PAIR_ID = ((128, 0, 128), (128, 0, 256), (256, 0, 256))      # (P, P2, N1) of the header
PAIR_DS = ((128, 256, 128), (256, 512, 0))
AUTO_TILED = (16, 56, 64, 256)                               # (N, H, Cin, Cout), 1 x 1: the automatic choice takes conv_lean (17), which has no tiled form
AUTO_FOLD = (11, 56, 64, 64, 64)                             # (N, Ho, Cin, Cin2, Cout), stride2 1: the automatic choice takes the 64-wide tile 12
T2, RES, OUT_T, OUT_E = (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)
PLAN_ID = ((1, 1, 1, 0), (1, 1, 0, 1))                       # what plan_pass produces for an identity pair block
PLAN_DS = ((1, 0, 1, 0),)                                    # ... and for a stage-first one


def fold_geoms():
    """(N, Ho, stride2, H2): stride 1 reads x2 at the output's own size; stride 2 from an even and from an odd image"""
    return [(N, Ho, s2, H2) for N, Ho in FOLD_NHO for s2, H2 in ((1, Ho), (2, 2 * Ho), (2, 2 * Ho - 1))]


def fold_cfgs(prec):
    """(configurations that run, configurations that must refuse) in a precision"""
    if prec == "bf16x2":
        return (-1, 11, 100), (12,)
    cfgs = ALL_CFGS                                          # fp32, bf16 and f16 alike: the f16 kernel set has every configuration
    return tuple(c for c in cfgs if c not in FOLD_NARROW), tuple(c for c in cfgs if c in FOLD_NARROW)


def ceil16(M):
    return (M + 15) // 16 * 16


def tiled_index(M, C, mut=None):
    """ap_tiled_off (ap_common.h) of every element of an [M][C] tensor: [M][C] offsets into [ceil(M / 16)][C / 8][16][8]"""
    m, ch = torch.arange(M)[:, None], torch.arange(C)[None, :]
    hi, lo = (m & 15, m >> 4) if mut == "swap_pixel" else (m >> 4, m & 15)
    groups = (C >> 3) + (1 if mut == "group_stride" else 0)
    return (hi * groups + (ch >> 3)) * 128 + lo * 8 + (ch & 7)


def tile_rows(v, fill=float("nan")):
    """[M][C] -> the flat fragment-tiled tensor; the pixels past M hold `fill` (a kernel that reads them shows)"""
    M, C = v.shape
    out = torch.full((ceil16(M) * C,), fill, dtype=v.dtype)
    out[tiled_index(M, C).reshape(-1)] = v.reshape(-1)
    return out


def _bits16(v, prec):
    """fp32 values that are representable in the 16-bit storage of prec -> their bit patterns"""
    return v.to(DT16[prec]).contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ the assertions (GPU tests and self-check)
def assert_tiled(what, bits, written, plain_bits, M, C):
    """bits / written: the flat tiled buffer (int16 patterns; which elements were written).  Gathered through tiled_index it
    equals the plain entry's bits, and exactly the elements of the pixels < M are written."""
    assert bits.numel() == ceil16(M) * C, (what, "buffer of %d elements, the layout has %d" % (bits.numel(), ceil16(M) * C))
    idx = tiled_index(M, C).to(bits.device)
    want_written = torch.zeros(bits.numel(), dtype=torch.bool, device=bits.device)
    want_written[idx.reshape(-1)] = True
    assert bool(written[want_written].all()), (what, "%d elements of pixels < M never written" % int((~written[want_written]).sum()))
    assert not bool(written[~want_written].any()), (what, "%d elements of the pixels past M written" % int(written[~want_written].sum()))
    got = bits[idx]
    assert torch.equal(got, plain_bits.view(M, C)), (what, "%d gathered elements differ from the plain layout" % int((got != plain_bits.view(M, C)).sum()))


def assert_even(what, bits, written, plain_bits, N, Ho, C):
    """out_even: bits / written of the NHWC `out` [N][Ho][Ho][C]: the pixels with even ho and even wo carry the plain form's bits,
    every other pixel is untouched"""
    b, w, p = bits.view(N, Ho, Ho, C), written.view(N, Ho, Ho, C), plain_bits.view(N, Ho, Ho, C)
    assert bool(w[:, ::2, ::2].all()), (what, "an even pixel was not stored")
    assert torch.equal(b[:, ::2, ::2], p[:, ::2, ::2]), (what, "out differs from the plain form at the even pixels")
    assert not bool(w[:, 1::2].any()) and not bool(w[:, :, 1::2].any()), (what, "an odd pixel of out was written")


def assert_pool_bits(what, got, want, counter=None):
    """the pooled features equal conv + avgpool bit for bit"""
    same = torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    if counter is not None:
        counter.append(same)
    assert same, (what, "%d pooled features differ from conv + avgpool" % int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ references (computed once, shared)
_FOLD, _POOL, _PAIR = {}, {}, {}


def fold_case(prec, ch, geom, fam_t, fam_x):
    key = (prec, ch, geom, fam_t, fam_x)
    if key not in _FOLD:
        (Cin, Cin2, Cout), (N, Ho, s2, H2) = ch, geom
        seed = Cin + 3 * Cin2 + 5 * Cout
        gs = seed + 7 * N + 11 * Ho + 13 * s2 + 17 * H2
        tv = operands(make_input(N, Ho, Ho, Cin, fam_t, gs), prec)
        xv = operands(make_input(N, H2, H2, Cin2, fam_x, gs + 1), prec)
        wv = operands(make_weight(Cout, 1, Cin + Cin2, seed), prec)
        scale, shift = make_bn(Cout, seed)
        cat = torch.cat([tv, xv[:, ::s2, ::s2, :]], 3)       # as test_conv_pw_ds builds it
        assert cat.shape[1] == Ho
        c, a = conv_sums(cat, wv, 1, 0)
        resv = operands(make_res(tuple(c.shape), gs), prec)
        _FOLD[key] = dict(tv=tv, xv=xv, wv=wv, cat=cat, scale=scale, shift=shift, resv=resv, c=c, a=a, K=Cin + Cin2)
    return _FOLD[key]


def fold_ref(cs, relu, res, prec):
    return finish(cs["c"], cs["a"], cs["scale"], cs["shift"], cs["resv"] if res else None, relu, prec, cs["K"])


def fold_runs():
    """(channels, geometry, family of t, family of x2, variants): all four (relu, res) on randn; "alt" for t and for x2 independently
    and together (a sample taken from the neighbouring image shows)"""
    out = []
    for ci, ch in enumerate(FOLD_CH):
        for gi, geom in enumerate(fold_geoms()):
            out.append((ch, geom, "randn", "randn", VARIANTS))
            for ai, (ft, fx) in enumerate((("alt", "randn"), ("randn", "alt"), ("alt", "alt"))):
                out.append((ch, geom, ft, fx, (VARIANTS[(ci + gi + ai) % 4],)))
    return out


def pool_case(prec, ch, N, family):
    key = (prec, ch, N, family)
    if key not in _POOL:
        Cin, Cout = ch
        seed = Cin + 3 * Cout
        xv = operands(make_input(N, 7, 7, Cin, family, seed + N), prec)
        wv = operands(make_weight(Cout, 1, Cin, seed), prec)
        scale, shift = make_bn(Cout, seed)
        resv = operands(make_res((N, 7, 7, Cout), seed + N), prec)
        ref, bound = stage(xv, wv, scale, shift, resv, 1, 1, 0, prec)
        mag = (ref.abs() + bound).reshape(N, 49, Cout)       # bounds the magnitude of every stored value from above
        pref = ref.reshape(N, 49, Cout).mean(1)
        pbound = bound.reshape(N, 49, Cout).mean(1) + 50 * 2.0 ** -24 * mag.mean(1) + 2.0 ** -24 * pref.abs()
        _POOL[key] = dict(xv=xv, wv=wv, scale=scale, shift=shift, resv=resv, ref=ref, bound=bound, pref=pref, pbound=pbound)
    return _POOL[key]


# ------------------------------------------------------------------------------------------------ fp32 emulations
MUTATIONS = ("drop_segment", "sample_stride1", "sample_prev_image", "group_stride", "swap_pixel", "drop_carry", "div48", "pool_unrounded",
             "store_odd", "even_ho_only")
POOL_IMGS, POOL_PIX, POOL_BM = 5, 49, 128                    # conv_lean.hip: images per super-tile, pixels per image, rows per sub-tile


def emulate_fold(cs, geom, relu, res, prec, mut=None):
    """[t | x2 sampled at (ho stride2, wo stride2) of the same image] through the fp32 emulation of a pointwise convolution"""
    N, Ho, s2, H2 = geom
    tv, xv, wv = cs["tv"], cs["xv"], cs["wv"]
    n, ho, wo = torch.meshgrid(torch.arange(N), torch.arange(Ho), torch.arange(Ho), indexing="ij")
    st = 1 if mut == "sample_stride1" else s2
    if mut == "sample_prev_image":
        n = (n - 1).clamp_min(0)
    samp = xv[n, ho * st, wo * st]
    if mut == "drop_segment":
        samp = torch.zeros_like(samp)
    return emulate(torch.cat([tv, samp], 3), wv, cs["scale"], cs["shift"], cs["resv"] if res else None, relu, 1, 0, prec)


def emulate_tiled(stored, prec, mut=None):
    """the scatter of an epilogue that stores [M][C] values through ap_tiled_off: (bits, written) of the flat buffer, and of whatever
    lies behind it (a mutated offset may leave the tensor)"""
    M, C = stored.shape
    idx = tiled_index(M, C, mut).reshape(-1)
    n = max(int(idx.max()) + 1, ceil16(M) * C)
    bits, written = torch.zeros(n, dtype=torch.int16), torch.zeros(n, dtype=torch.bool)
    bits[idx] = _bits16(stored, prec).reshape(-1)
    written[idx] = True
    return bits, written


def avgpool_order(v, mut=None):
    """avgpool_kernel's order (stem.hip) on [N][49][C] fp32: eight partitions p, p + 8, ... summed serially, then the partitions in
    order, / 49.  The pooling epilogue of conv_lean.hip follows it; the third image of a super-tile of five straddles the two
    128-row sub-tiles at pixel 30, and its partitions are carried across (the order of the additions does not change)."""
    N, _, C = v.shape
    split = POOL_BM - 2 * POOL_PIX
    out = torch.empty(N, C)
    for n in range(N):
        parts = []
        for k in range(8):
            acc = torch.zeros(C)
            for px in range(k, POOL_PIX, 8):
                if mut == "drop_carry" and n % POOL_IMGS == 2 and px < split:
                    continue                                 # the second sub-tile starts from 0 instead of the carried partial sums
                acc = acc + v[n, px]
            parts.append(acc)
        t = parts[0]
        for k in range(1, 8):
            t = t + parts[k]
        out[n] = t / (48.0 if mut == "div48" else 49.0)
    return out


def emulate_pool(cs, prec, mut=None):
    """(pooled features of the fused form, of conv + avgpool): fp32 conv + BN + identity + ReLU, rounded to storage, pooled"""
    N, Cout = cs["xv"].shape[0], cs["wv"].shape[0]
    y = cs["xv"].reshape(N * 49, -1) @ cs["wv"].reshape(Cout, -1).t()
    y = (y * cs["scale"] + cs["shift"] + cs["resv"].reshape(N * 49, Cout)).clamp_min(0)
    st = operands(y, prec).view(N, 49, Cout)
    return avgpool_order(y.view(N, 49, Cout) if mut == "pool_unrounded" else st, mut), avgpool_order(st)


def emulate_even(stored, N, Ho, prec, mut=None):
    """(bits, written) of an NHWC out [N][Ho][Ho][C] stored at the even pixels only"""
    C = stored.shape[-1]
    ho, wo = torch.meshgrid(torch.arange(Ho), torch.arange(Ho), indexing="ij")
    keep = ((ho if mut == "even_ho_only" else (ho | wo)) & 1) == 0
    if mut == "store_odd":
        keep = torch.ones_like(keep)
    written = keep[None, :, :, None].expand(N, Ho, Ho, C).contiguous()
    bits = torch.where(written, _bits16(stored, prec).view(N, Ho, Ho, C), torch.zeros((), dtype=torch.int16))
    return bits.reshape(-1), written.reshape(-1)


def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("prec", PRECS)
def test_cpu_fold_emulation_and_mutations(prec):
    """The fold emulation is inside every bar on every run of test_fold; the three sampling mutations are rejected."""
    ratios = {}
    for ch, geom, ft, fx, variants in fold_runs():
        cs = fold_case(prec, ch, geom, ft, fx)
        for relu, res in variants:
            ref, bound = fold_ref(cs, relu, res, prec)
            check("%s %s %s %s/%s" % (prec, ch, geom, ft, fx), ft + "/" + fx, emulate_fold(cs, geom, relu, res, prec), ref, bound, ratios)
    # drop_segment: any shape; sample_stride1: a stride-2 geometry; sample_prev_image: x2 "alt" with more than one image
    for mut, geom, fx in (("drop_segment", (3, 7, 1, 7), "randn"), ("sample_stride1", (3, 7, 2, 14), "randn"), ("sample_prev_image", (3, 7, 2, 13), "alt")):
        cs = fold_case(prec, FOLD_CH[0], geom, "randn", fx)
        ref, bound = fold_ref(cs, 1, 1, prec)
        ok, ratio, _, _ = evaluate(emulate_fold(cs, geom, 1, 1, prec, mut=mut), ref, bound)
        assert not ok, (prec, mut, "the checker accepts this mutation: worst err / bound %.3f" % ratio)
        ratios["!" + mut] = ratio
    report("fold emulation " + prec, ratios)


@pytest.mark.parametrize("prec", P16)
def test_cpu_tiled_pool_even_emulations_and_mutations(prec):
    """Tiled scatter / gather on every shape of test_tiled, the pooling order on every case of test_pool, the even-pixel mask on
    the pair shapes: inside the bars, accepted by the assertions of the GPU tests; the seven mutations are rejected by them."""
    ratios = {}
    guard_hits = 0
    for shp in TILED_SHAPES:
        name = shp[0]
        cs = case(prec, shp, "randn")
        ref, bound = case_ref(cs, 1, 1, prec)
        st = emulate(cs["xv"], cs["wv"], cs["scale"], cs["shift"], cs["resv"], 1, shp[7], shp[8], prec)
        M, C = st.numel() // shp[5], shp[5]
        st = st.reshape(M, C)
        bits, written = emulate_tiled(st, prec)
        assert_tiled("emulation " + name, bits, written, _bits16(st, prec), M, C)
        check("tiled emulation " + name, "tiled", bits[tiled_index(M, C)].view(DT16[prec]).float().view(ref.shape), ref, bound, ratios)
        for mut in ("group_stride", "swap_pixel"):
            if M <= 16:
                continue                                     # one group of 16 pixels: the group stride is never applied
            b, w = emulate_tiled(st, prec, mut)
            n = ceil16(M) * C
            # the tensor itself is rejected by the GPU tests' assertion, whether or not the mutation also stores behind it (what
            # lies behind is a guard band on the GPU: _guards_ok there, w[n:] here)
            assert _rejected(assert_tiled, mut, b[:n], w[:n], _bits16(st, prec), M, C), (prec, name, mut, "accepted")
            guard_hits += int(w[n:].any())
    assert guard_hits > 0                                    # (some mutated scatters also leave the tensor: the guard bands are needed)
    bit_checks = []
    for ch in POOL_CH:
        for N in POOL_N:
            for family in POOL_FAMILIES:
                cs = pool_case(prec, ch, N, family)
                got, want = emulate_pool(cs, prec)
                check("pool emulation %s N=%d %s" % (ch, N, family), "pool " + family, got, cs["pref"], cs["pbound"], ratios)
                assert_pool_bits("pool emulation", got, want)
    cs = pool_case(prec, POOL_CH[0], 6, "randn")
    for mut in ("drop_carry", "div48"):
        got, _ = emulate_pool(cs, prec, mut)
        ok, ratio, _, _ = evaluate(got, cs["pref"], cs["pbound"])
        assert not ok, (prec, mut, "the checker accepts this mutation: worst err / bound %.3f" % ratio)
        ratios["!" + mut] = ratio
    got, want = emulate_pool(cs, prec, "pool_unrounded")
    assert _rejected(assert_pool_bits, "pool_unrounded", got, want, bit_checks) and bit_checks == [False], (prec, "pool_unrounded accepted")
    ratios["!pool_unrounded (inside the bar: %s)" % evaluate(got, cs["pref"], cs["pbound"])[0]] = evaluate(got, cs["pref"], cs["pbound"])[1]
    for N, Ho in PAIR_NHO:
        P = 128
        t2v = operands(make_input(N, Ho, Ho, P, "randn", N + Ho), prec)
        w3v, (s3, h3) = operands(make_weight(4 * P, 1, P, 5), prec), make_bn(4 * P, 5)
        resv = operands(make_res((N, Ho, Ho, 4 * P), N + Ho), prec)
        ref, bound = stage(t2v, w3v, s3, h3, resv, 1, 1, 0, prec)
        st = emulate(t2v, w3v, s3, h3, resv, 1, 1, 0, prec)
        check("even emulation N=%d Ho=%d" % (N, Ho), "even", st, ref, bound, ratios)
        bits, written = emulate_even(st, N, Ho, prec)
        assert_even("emulation", bits, written, _bits16(st, prec), N, Ho, 4 * P)
        for mut in ("store_odd", "even_ho_only"):
            b, w = emulate_even(st, N, Ho, prec, mut)
            assert _rejected(assert_even, mut, b, w, _bits16(st, prec), N, Ho, 4 * P), (prec, mut, "accepted")
    report("tiled / pool / even emulation " + prec, ratios)


def test_shape_lists_match_the_tile_constants():
    """The shape lists against the constants of the kernels they are built around (host only)."""
    src = open(os.path.join(REPO, "airpose_amd", "csrc", "conv_lean.hip")).read()
    const = lambda n: int(re.search(r"\b%s = (\d+)" % n, src).group(1))
    assert (const("POOL_IMGS"), const("POOL_PIX"), const("BM")) == (POOL_IMGS, POOL_PIX, POOL_BM)
    rows = POOL_IMGS * POOL_PIX
    assert rows == 245 and 2 * POOL_BM - rows == 11 and POOL_BM - 2 * POOL_PIX == 30      # 11 unused rows; image 2 splits at pixel 30
    assert "p0 = (sub == 1 && seg == 0) ? 30 : 0" in src
    st = {N: ((N + POOL_IMGS - 1) // POOL_IMGS, N % POOL_IMGS) for N in POOL_N}
    assert st[1] == (1, 1) and st[2] == (1, 2)               # a partly empty super-tile, without / ...
    assert st[4] == (1, 4)                                   # ... with the image that is carried across the sub-tiles
    assert st[5] == (1, 0) and st[6] == (2, 1) and st[11] == (3, 1)
    assert {c[1] % 256 == 0 for c in POOL_CH} == {True, False} and {c[1] % 128 == 0 for c in POOL_CH} == {True, False}
    assert "((m >> 4) * (size_t)(C >> 3) + (size_t)(ch >> 3)) * 128 + (m & 15) * 8" in open(os.path.join(REPO, "airpose_amd", "csrc", "ap_common.h")).read()
    Ms = {s[0]: s[1] * ((s[2] + 2 * s[8] - s[6]) // s[7] + 1) * ((s[3] + 2 * s[8] - s[6]) // s[7] + 1) for s in TILED_SHAPES}
    assert any(m % 16 == 0 for m in Ms.values()) and sum(m % 16 != 0 for m in Ms.values()) >= 8 and Ms["p1_m129"] == 129 and Ms["p1_m257"] == 257
    assert {s[3] for s in TILED_SHAPES if s[6] == 3 and s[7] == 1} >= {29, 30, 31}           # slab up to W = 30, the ring kernel above
    assert {s[7] for s in TILED_SHAPES if s[6] == 3} == {1, 2} and len([s for s in SHAPES if s[6] == 3]) + 2 == len(TILED_SHAPES)
    assert [N * Ho * Ho for N, Ho in FOLD_NHO] == [9, 147, 128] and [N * Ho * Ho for N, Ho in PAIR_NHO] == [49, 245, 196]
    assert 245 % 16 and 245 % 64 and 196 % 16                # ragged for the 16-pixel micro-tile and for the 64-pixel workgroup
    assert set(fold_cfgs("bf16")[0]) == {-1, 100, 14, 17} | set(FOLD_WIDE) and set(fold_cfgs("bf16")[1]) == set(FOLD_NARROW)
    assert fold_cfgs("f16") == fold_cfgs("bf16") == fold_cfgs("fp32") and fold_cfgs("bf16x2") == ((-1, 11, 100), (12,)) and len(MUTATIONS) == 10
    # the automatic-mode refusals of the header (test_automatic_choice_refusals): conv_lean from 768 tiles of 128 x 128, tile 12 from 256 rows of tiles
    (N, H, Cin, Cout), (fN, fHo, _, _, fCout) = AUTO_TILED, AUTO_FOLD
    assert (N * H * H + 127) // 128 * ((Cout + 127) // 128) >= 768 and Cin <= 512 and Cout >= 256
    assert (fN * fHo * fHo + 127) // 128 >= 256 and fCout <= 64


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


def _untouched(g):
    return bool(torch.isnan(g.buf.float()).all())


def _written(g):
    return ~torch.isnan(g.out)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_fold(dev, prec):
    """ap_conv2d_fold_nhwc under every configuration of the precision: the first one element-wise against fp64 on
    [t | x2 sampled], the others bit-equal to it; the 64-wide tiles refuse and leave the buffer alone."""
    Nn, L = _lib()
    ratios = {}
    PR, st = Nn.PRECISIONS[prec], Nn.stream_ptr(dev)
    run_cfgs, refuse_cfgs = fold_cfgs(prec)
    wcache = {}
    try:
        for ch, geom, ft, fx, variants in fold_runs():
            (Cin, Cin2, Cout), (N, Ho, s2, H2) = ch, geom
            cs = fold_case(prec, ch, geom, ft, fx)
            if ch not in wcache:
                wcache[ch] = (_w_dev(cs["wv"], prec, dev),) + _bn_dev(cs["scale"], cs["shift"], dev)
            wd, sd, hd = wcache[ch]
            td, xd, rd = (_to_storage(cs[k], prec, dev)[0] for k in ("tv", "xv", "resv"))
            for relu, res in variants:
                what = "fold %s %s N=%d Ho=%d s=%d H2=%d %s/%s relu=%d res=%d" % (prec, ch, N, Ho, s2, H2, ft, fx, relu, res)
                first = None
                for cfg in run_cfgs + refuse_cfgs:
                    Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
                    g = Guarded(dev, prec, N * Ho * Ho * Cout)
                    rc = L.ap_conv2d_fold_nhwc(PR, _p(td), _p(xd), _p(wd), _p(sd), _p(hd), _p(rd) if res else None, _p(g.out), N, Ho, H2,
                                               Cin, Cin2, Cout, s2, relu, st)
                    torch.cuda.synchronize()
                    if cfg in refuse_cfgs:
                        assert rc == -2, (what, cfg, "a 64-wide tile did not refuse a second K segment with AP_ESHAPE: status %d" % rc)
                        assert _untouched(g), (what, cfg, "refused, but the output buffer was written")
                        continue
                    assert rc == 0, (what, cfg, "undocumented refusal, status %d" % rc)
                    got = g.values((N, Ho, Ho, Cout), what)
                    if first is None:
                        first = g.bits().clone()
                        ref, bound = fold_ref(cs, relu, res, prec)
                        check(what, "s%d %s/%s" % (s2, ft, fx), got.cpu(), ref, bound, ratios)
                    else:
                        assert torch.equal(g.bits(), first), (what, "configuration %d differs from %d in %d elements" % (
                            cfg, run_cfgs[0], int((g.bits() != first).sum())))
    finally:
        L.ap_set_conv_config(-1)
    report("ap_conv2d_fold_nhwc " + prec, ratios)


def conv2d_tiled(dev, prec, xd, wd, sd, hd, rd, shp, relu):
    Nn, L = _lib()
    name, N, H, W, Cin, Cout, k, s, p = shp
    M = N * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    g = Guarded(dev, prec, ceil16(M) * Cout)
    rc = L.ap_conv2d_tiled_nhwc(Nn.PRECISIONS[prec], _p(xd), _p(wd), _p(sd), _p(hd), _p(rd), _p(g.out), N, H, W, Cin, Cout, k, s, p, int(relu),
                                Nn.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, g, M


@gpu
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("cfg", TILED_CFGS)
def test_tiled(dev, prec, cfg):
    """ap_conv2d_tiled_nhwc: gathered through tiled_index, the bits of ap_conv2d_nhwc under the same configuration, which sit inside
    the fp64 bar; the pixels M .. ceil16(M) - 1 of the last micro-tile and the guards untouched."""
    Nn, L = _lib()
    ratios = {}
    Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
    try:
        for si, shp in enumerate(TILED_SHAPES):
            name, N, H, W, Cin, Cout, k, s, p = shp
            for fi, family in enumerate(("randn", GPU_FAMILY.get(name, ("alt", "frame", "impulse")[si % 3]))):
                cs = case(prec, shp, family)
                xd, rd = _to_storage(cs["xv"], prec, dev)[0], _to_storage(cs["resv"], prec, dev)[0]
                wd = _w_dev(cs["wv"], prec, dev)
                sd, hd = _bn_dev(cs["scale"], cs["shift"], dev)
                for relu, res in (VARIANTS if fi == 0 else VARIANTS[si % 2::2]):
                    what = "tiled %s cfg=%d %s %s relu=%d res=%d" % (prec, cfg, name, family, relu, res)
                    rc, gp, oshape = conv2d(dev, prec, xd, wd, sd, hd, rd if res else None, N, H, W, Cin, Cout, k, s, p, relu)
                    assert rc == 0, (what, "ap_conv2d_nhwc refused")
                    ref, bound = case_ref(cs, relu, res, prec)
                    check(what, "k%ds%d" % (k, s), gp.values(oshape, what).cpu(), ref, bound, ratios)
                    rc, g, M = conv2d_tiled(dev, prec, xd, wd, sd, hd, rd if res else None, shp, relu)
                    assert rc == 0, (what, "undocumented refusal, status %d" % rc)
                    assert _guards_ok(g), (what, "a guard band was written")
                    assert_tiled(what, g.bits(), _written(g), gp.bits(), M, Cout)
    finally:
        L.ap_set_conv_config(-1)
    report("ap_conv2d_tiled_nhwc %s cfg=%d" % (prec, cfg), ratios)


@gpu
def test_tiled_refusals(dev):
    """fp32, bf16x2 (every configuration) and configurations 4-7 and 17 (16-bit) are refused with the buffer untouched"""
    Nn, L = _lib()
    shp = [s for s in SHAPES if s[0] == "p1_m129"][0]
    try:
        for prec, cfgs in (("fp32", (-1, 11, 100)), ("bf16x2", (-1, 11, 100)), ("bf16", TILED_REFUSED_CFGS), ("f16", TILED_REFUSED_CFGS)):
            cs = case(prec, shp, "randn")
            xd, wd = _to_storage(cs["xv"], prec, dev)[0], _w_dev(cs["wv"], prec, dev)
            sd, hd = _bn_dev(cs["scale"], cs["shift"], dev)
            for cfg in cfgs:
                Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
                rc, g, M = conv2d_tiled(dev, prec, xd, wd, sd, hd, None, shp, 1)
                assert rc == -2, (prec, cfg, "a tiled output was not refused with AP_ESHAPE: status %d" % rc)
                assert _untouched(g), (prec, cfg, "refused, but the output buffer was written")
    finally:
        L.ap_set_conv_config(-1)


@gpu
@pytest.mark.parametrize("prec", P16)
def test_automatic_choice_refusals(dev, prec):
    """The two refusals the header lists for the AUTOMATIC choice, at the smallest sizes that reach them: a 1 x 1 tiled call that
    the choice hands to conv_lean, a fold with Cout = 64 that it hands to tile 12.  AP_ESHAPE with the buffer untouched under -1;
    under 11 both run: the tiled call carries ap_conv2d_nhwc's bits, the fold agrees bitwise with configuration 100."""
    Nn, L = _lib()
    PR, st = Nn.PRECISIONS[prec], Nn.stream_ptr(dev)
    gen = torch.Generator(device="cpu").manual_seed(99)
    N, H, Cin, Cout = AUTO_TILED
    shp = ("auto_tiled", N, H, H, Cin, Cout, 1, 1, 0)
    xd = _rows16(torch.randn(N, H, H, Cin, generator=gen), prec, dev)
    wd = _w_dev(operands(make_weight(Cout, 1, Cin, 9), prec), prec, dev)
    sd, hd = _bn_dev(*make_bn(Cout, 9), dev)
    fN, fHo, fCin, fCin2, fCout = AUTO_FOLD
    td = _rows16(torch.randn(fN, fHo, fHo, fCin, generator=gen), prec, dev)
    x2d = _rows16(torch.randn(fN, fHo, fHo, fCin2, generator=gen), prec, dev)
    fwd = _w_dev(operands(make_weight(fCout, 1, fCin + fCin2, 10), prec), prec, dev)
    fsd, fhd = _bn_dev(*make_bn(fCout, 10), dev)

    def fold(cfg):
        Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
        g = Guarded(dev, prec, fN * fHo * fHo * fCout)
        rc = L.ap_conv2d_fold_nhwc(PR, _p(td), _p(x2d), _p(fwd), _p(fsd), _p(fhd), None, _p(g.out), fN, fHo, fHo, fCin, fCin2, fCout, 1, 1, st)
        torch.cuda.synchronize()
        return rc, g
    try:
        rc, g, M = conv2d_tiled(dev, prec, xd, wd, sd, hd, None, shp, 1)
        assert rc == -2 and _untouched(g), (prec, "automatic choice, 1 x 1 tiled on conv_lean's shapes: status %d" % rc)
        rc, g = fold(-1)
        assert rc == -2 and _untouched(g), (prec, "automatic choice, fold with Cout = 64: status %d" % rc)
        Nn.check(L.ap_set_conv_config(11), "ap_set_conv_config")
        rc, gp, oshape = conv2d(dev, prec, xd, wd, sd, hd, None, N, H, H, Cin, Cout, 1, 1, 0, 1)
        assert rc == 0
        gp.values(oshape, "auto_tiled plain")
        rc, g, M = conv2d_tiled(dev, prec, xd, wd, sd, hd, None, shp, 1)
        assert rc == 0 and _guards_ok(g), (prec, "configuration 11 refused the tiled call: status %d" % rc)
        assert_tiled("auto_tiled cfg=11", g.bits(), _written(g), gp.bits(), M, Cout)
        (rc11, g11), (rc100, g100) = fold(11), fold(100)
        assert rc11 == 0 and rc100 == 0, (prec, rc11, rc100)
        g11.values((fN * fHo * fHo, fCout), "auto_fold 11")
        assert torch.equal(g11.bits(), g100.bits()), (prec, "fold: configuration 11 differs from 100")
    finally:
        L.ap_set_conv_config(-1)


def pool(dev, prec, xd, wd, sd, hd, rd, N, Cin, Cout):
    """ap_conv2d_pool_nhwc into a guarded fp32 buffer: the pooled features [N][Cout] (device)"""
    Nn, L = _lib()
    g = Guarded(dev, "fp32", N * Cout)
    Nn.check(L.ap_conv2d_pool_nhwc(Nn.PRECISIONS[prec], _p(xd), _p(wd), _p(sd), _p(hd), _p(rd), _p(g.out), N, Cin, Cout, Nn.stream_ptr(dev)),
             "ap_conv2d_pool_nhwc")
    torch.cuda.synchronize()
    return g.values((N, Cout), "pool %s N=%d %d -> %d" % (prec, N, Cin, Cout))


@gpu
@pytest.mark.parametrize("prec", P16)
def test_pool(dev, prec):
    """ap_conv2d_pool_nhwc against the fp64 mean of the stored values' reference; bit-equal to ap_conv2d_nhwc + ap_avgpool_nhwc where
    Cout is a multiple of 256; an image's pooled row does not depend on its position in the batch."""
    Nn, L = _lib()
    ratios = {}
    PR, st = Nn.PRECISIONS[prec], Nn.stream_ptr(dev)
    nbits = 0
    for ch in POOL_CH:
        Cin, Cout = ch
        for N in POOL_N:
            for family in POOL_FAMILIES:
                what = "pool %s %s N=%d %s" % (prec, ch, N, family)
                cs = pool_case(prec, ch, N, family)
                xd, rd = _rows16(cs["xv"], prec, dev), _rows16(cs["resv"], prec, dev)
                wd = _w_dev(cs["wv"], prec, dev)
                sd, hd = _bn_dev(cs["scale"], cs["shift"], dev)
                got = pool(dev, prec, xd, wd, sd, hd, rd, N, Cin, Cout)
                check(what, "%d->%d %s" % (Cin, Cout, family), got.cpu(), cs["pref"], cs["pbound"], ratios)
                if Cout % 256 == 0:
                    rc, gy, oshape = conv2d(dev, prec, xd, wd, sd, hd, rd, N, 7, 7, Cin, Cout, 1, 1, 0, 1)
                    assert rc == 0
                    gy.values(oshape, what)
                    ga = Guarded(dev, "fp32", N * Cout)
                    Nn.check(L.ap_avgpool_nhwc(PR, _p(gy.out), _p(ga.out), N, Cout, st), "ap_avgpool_nhwc")
                    torch.cuda.synchronize()
                    assert_pool_bits(what, got, ga.values((N, Cout), what))
                    nbits += 1
                if N == 6:                                   # image 5: first of the second super-tile in the batch, first of the first alone
                    alone = pool(dev, prec, xd[5:6].contiguous(), wd, sd, hd, rd[5:6].contiguous(), 1, Cin, Cout)
                    assert torch.equal(alone.view(torch.int32), got[5:6].contiguous().view(torch.int32)), (what, "image 5 depends on its position")
                    alone2 = pool(dev, prec, xd[2:3].contiguous(), wd, sd, hd, rd[2:3].contiguous(), 1, Cin, Cout)
                    assert torch.equal(alone2.view(torch.int32), got[2:3].contiguous().view(torch.int32)), (what, "the carried image depends on its position")
    assert nbits == 2 * len(POOL_N) * len(POOL_FAMILIES)
    report("ap_conv2d_pool_nhwc " + prec, ratios)


def _pair_case(prec, P, P2, N1, N, Ho, family, fi):
    key = (prec, P, P2, N1, N, Ho, family)
    if key not in _PAIR:
        C3, M = 4 * P, N * Ho * Ho
        t2v = operands(make_input(N, Ho, Ho, P, family, M + fi), prec)
        if P2:
            inv = operands(make_input(N, 2 * Ho, 2 * Ho, P2, ("alt", "randn")[fi], M + fi + 50), prec)
        else:
            inv = operands(make_res((N, Ho, Ho, C3), M + fi), prec)
        _PAIR[key] = (t2v, inv)
    return _PAIR[key]


def _pair_run(dev, prec, ws, dv, t2d, ind, N, Ho, P, P2, N1, flags, plain=False):
    """one pair launch into guarded buffers sized for the layouts asked for: (status, out, t1n)"""
    Nn, L = _lib()
    PR, st = Nn.PRECISIONS[prec], Nn.stream_ptr(dev)
    M, C3 = N * Ho * Ho, 4 * P
    go = Guarded(dev, prec, (ceil16(M) if flags[2] else M) * C3)
    gt = Guarded(dev, prec, M * max(N1, 8))
    s1, h1, t1 = (_p(dv[2]), _p(dv[3]), _p(gt.out)) if N1 else (None, None, None)
    if plain and P2:
        rc = L.ap_conv_pair_ds_nhwc(PR, _p(t2d), _p(ind), _p(ws), _p(dv[0]), _p(dv[1]), s1, h1, _p(go.out), t1, N, Ho, P, P2, 2, N1, st)
    elif plain:
        rc = L.ap_conv_pair_nhwc(PR, _p(t2d), _p(ws), _p(dv[0]), _p(dv[1]), _p(ind), s1, h1, _p(go.out), t1, M, P, N1, st)
    else:
        rc = L.ap_conv_pair_layout_nhwc(PR, _p(t2d), _p(ind), _p(ws), _p(dv[0]), _p(dv[1]), s1, h1, _p(go.out), t1, N, Ho, P, P2, 2, N1,
                                        flags[0], flags[1], flags[2], flags[3], st)
    torch.cuda.synchronize()
    return rc, go, gt


def _or(*fl):
    return tuple(int(any(f[i] for f in fl)) for i in range(4))


@gpu
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("P,P2,N1", PAIR_ID + PAIR_DS)
def test_pair_layouts(dev, prec, P, P2, N1):
    """ap_conv_pair_layout_nhwc: every flag alone where it is accepted and the combinations plan_pass produces, on host-tiled inputs:
    `out` (gathered) and `t1n` carry the plain entry's bits -- which are held against fp64 as test_conv_pair does; out_even leaves
    every odd pixel alone; out_tiled leaves the pixels past M alone; the three undefined combinations are refused."""
    Nn, L = _lib()
    r_out, r_t1 = {}, {}
    C3 = 4 * P
    w3v = operands(make_weight(C3, 1, P + P2, P + N1 + 3), prec)
    w1v = operands(make_weight(max(N1, 8), 1, C3, P + N1 + 4), prec)
    s3, h3 = make_bn(C3, P + N1 + 3)
    if P2:
        s3 = torch.ones(C3)                                  # both BatchNorm scales are folded into the rows
    s1, h1 = make_bn(max(N1, 8), P + N1 + 4)
    ws = _pair_stream(dev, prec, _rows16(w3v.reshape(C3, P + P2), prec, dev), _rows16(w1v.reshape(-1, C3), prec, dev), P, P2, N1)
    dv = [t.to(dev) for t in (s3, h3, s1, h1)]
    singles = [T2, OUT_T] + ([RES] if not P2 else []) + ([OUT_E] if N1 else [])
    layouts = [(0, 0, 0, 0)] + singles + list(PLAN_DS if P2 else PLAN_ID)
    refused = ([RES, _or(T2, RES)] if P2 else []) + [_or(OUT_T, OUT_E)] + ([OUT_E] if not N1 else [])
    for N, Ho in PAIR_NHO:
        M = N * Ho * Ho
        for fi, family in enumerate(("randn", "alt")):
            what = "pair %s (%d, %d, %d) N=%d Ho=%d %s" % (prec, P, P2, N1, N, Ho, family)
            t2v, inv = _pair_case(prec, P, P2, N1, N, Ho, family, fi)
            t2d, ind = _rows16(t2v, prec, dev), _rows16(inv, prec, dev)
            rc, po, pt = _pair_run(dev, prec, ws, dv, t2d, ind, N, Ho, P, P2, N1, (0, 0, 0, 0), plain=True)
            assert rc == 0, (what, "the plain entry refused")
            xin = torch.cat([t2v, inv[:, ::2, ::2, :]], 3) if P2 else t2v
            ref, bound = stage(xin, w3v, s3, h3, None if P2 else inv, 1, 1, 0, prec)
            out = po.values(tuple(ref.shape), what).cpu()
            check(what, family, out, ref, bound, r_out)
            if N1:
                ref1, bound1 = stage(out, w1v, s1, h1, None, 1, 1, 0, prec)
                check(what + " t1n", family, pt.values(tuple(ref1.shape), what).cpu(), ref1, bound1, r_t1)
            t2t = tile_rows(t2v.reshape(M, P).to(DT16[prec])).to(dev)
            rest = tile_rows(inv.reshape(M, C3).to(DT16[prec])).to(dev) if not P2 else None
            for lay in layouts:
                w = what + " layout %s" % (lay,)
                rc, go, gt = _pair_run(dev, prec, ws, dv, t2t if lay[0] else t2d, rest if lay[1] else ind, N, Ho, P, P2, N1, lay)
                assert rc == 0, (w, "undocumented refusal, status %d" % rc)
                assert _guards_ok(go) and _guards_ok(gt), (w, "a guard band was written")
                if N1:
                    gt.values((M, N1), w)
                    assert torch.equal(gt.bits(), pt.bits()), (w, "t1n differs from the plain entry in %d elements" % int((gt.bits() != pt.bits()).sum()))
                else:
                    assert _untouched(gt), (w, "t1n written without a next conv1")
                if lay[2]:
                    assert_tiled(w, go.bits(), _written(go), po.bits(), M, C3)
                elif lay[3]:
                    assert_even(w, go.bits(), _written(go), po.bits(), N, Ho, C3)
                else:
                    go.values((M, C3), w)
                    assert torch.equal(go.bits(), po.bits()), (w, "out differs from the plain entry")
            for lay in refused:
                rc, go, gt = _pair_run(dev, prec, ws, dv, t2t if lay[0] else t2d, ind, N, Ho, P, P2, N1, lay)
                assert rc == -2, (what, lay, "an undefined layout combination was not refused with AP_ESHAPE: status %d" % rc)
                assert _untouched(go) and _untouched(gt), (what, lay, "refused, but an output buffer was written")
    report("conv_pair layouts out %s (%d, %d, %d)" % (prec, P, P2, N1), r_out)
    if N1:
        report("conv_pair layouts t1n %s (%d, %d, %d)" % (prec, P, P2, N1), r_t1)
