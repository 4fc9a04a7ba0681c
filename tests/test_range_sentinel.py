"""The fp16 range sentinel, kernel by kernel, through the C ABI operator entries (include/airpose_hip.h) and the debug hook
ap_debug_set_range_hook / ap_debug_range_status that connects the library's own host-mapped word to them.  Companion of
test_conv_fwd_fp64.py and test_stem_pool_fp64.py, whose Guarded / operands / _to_storage / shape list / packing helpers it reuses.

The contract (ap_common.h, airpose_hip.h): every epilogue of the fp16 kernel set folds the packed values it STORES (the LDS-resident
intermediates of the fused kernels included) into a per-thread maximum (ap_rng_note*) and sets the word at its exit (ap_rng_flush)
when a value reached 0x7c00.  test_gpu_parity.py::test_f16_activation_overflow_is_reported overflows the stem, after which every
later kernel stores inf as well: the sentinel of any one kernel of layer1 .. layer4 could be deleted under it.  Here each kernel
stands alone.

Kernel -> test
  conv_pipe_kernel  (conv_pipe.hip)    test_conv2d_sentinel[0 .. 13]    LDS-staged epilogues (0-3, 8-13: 16-bit stage with ReLU and no
                                                                        residual, fp32 stage otherwise) and the register epilogue (4-7)
  conv_slab_kernel  (conv_slab.hip)    test_conv2d_sentinel[14 | -1]    (-1 takes it on the 3 x 3 / 1 / 1 shapes of the silent list)
  conv_lean_kernel  (conv_lean.hip)    test_conv2d_sentinel[17]; pooling variant: test_conv_pool_sentinel[1 | 4 | 6] (ap_conv2d_pool_nhwc)
  ... fragment-tiled output, second K segment of conv_slab / conv_pipe / conv_igemm     test_conv2d_forms_sentinel[tiled | fold - -1 | 11 | 100]
  conv_igemm_kernel (conv_igemm.hip)   test_conv2d_sentinel[100 | -1]   64 x 64 tiles; test_conv_igemm_large_tiles: 128 x 64, 128 x 128
  conv_pw_kernel    (conv_pw.hip)      test_conv_pw_sentinel[plain | ds | k3s2]
  conv_img3_kernel / conv_s2p_kernel   test_img3_s2p_sentinel[img3 | s2p - NHWC | fragment-tiled]
  conv_pair_kernel  (conv_pair.hip)    test_conv_pair_sentinel[(P, N1) | ds (P, P2, N1)]   `out` and `t1n` isolated
                                       test_conv_pair_layout_sentinel: the same under the three layout combinations of a trunk pass
  bottleneck2 kernels                  test_bottleneck64_sentinel[identity | downsample | tail | tail y_even]   y, t1n, hidden t1, hidden t2
  block_img_kernel  (block_img.hip)    test_block_img_sentinel          y, hidden t1, hidden t2
  stem_pool_kernel / stem_pool2_kernel test_stem_sentinel[1 | 2]        pooled maxima and the converted crop values
  stem_mfma_kernel + maxpool_kernel    test_stem_unpooled_then_maxpool  (the un-pooled kernel has no sentinel: its max-pool reports)
  maxpool_kernel / avgpool_kernel      test_maxpool_sentinel, test_avgpool_sentinel
  bf16 storage                         test_other_precisions_are_silent
  api_trunk.hip (run_* plumbing)       test_trunk_reports_one_masked_site[layerX.Y-bnZ]

Inputs are exact, so every expectation is derived, none measured.  fp16's largest finite value is 65504, its ulp there 32; the
midpoint 65520 ties to the even mantissa, i.e. to inf.  TOP = 65520 - 2^-8 is the largest fp32 below 65520: it must store 65504
and leave the word 0; OVF = 65520 must store inf and set it.  They are produced exactly: the activation is zero except single
pixels with value 1 in one input channel, the weights are 1 on that input channel (centre tap) and 0 elsewhere, so the fp32
accumulator is exactly 1 there; shift = 0; scale = 1 except the target channel, where it is the boundary value -- BatchNorm scale
and shift are fp32 epilogue parameters, nothing large passes through an fp16 operand.  The reference is the same data through
torch fp64, then .to(torch.float16): it says which stored elements are non-finite; the word must equal "any stored element is
non-finite", and the stored tensor must equal the reference bit for bit in value (exact inputs: no tolerance), inside Guarded
buffers.  In the one-overflow sweeps the per-launch check is the closed form of that reference (exactly one non-finite element, at
the target); the full comparison runs on a subset of the launches.

Per kernel: silent at the top of the range on ragged shapes (the false-alarm direction), with three baits: "rowbait" -- scale -16,
shift 65520 on an accumulator of 1 stores fma(1, -16, 65520) = 65504 everywhere, while a masked row, halo lane or padding unit
(accumulator 0) computes 65520; the channel padding of scale / shift computes 1e6; and, where the kernel has a residual, the two
pixels a clamped tail load can alias store 65520 - 16 while a masked copy without its residual would compute 65520; one overflow at a time over every store slot (exhaustive over (pixel, channel) where
M Cout <= 32768, otherwise one seeded element per cell of (pixel mod tile rows) x (channel pair mod tile width), tile sizes from
each kernel's header comment: TILES; the CPU self-check proves the coverage); -inf without ReLU and 0 with it; the residual add;
every output of the multi-output kernels in isolation (w1 = -1 on every input channel: t1n = relu(-inf) = 0); the hidden
intermediates of the fused kernels (t1 overflows in channel c, conv2 carries -1 on that input channel: t2 = relu(-inf) = 0, the
output is finite everywhere and the word is set; likewise t2 through conv3).

Residual boundary.  The issue's text names 16 - 2^-11 as the conv result that must stay silent on top of res = 65504.  That
value is not the boundary of an fp32 epilogue: 65504 + (16 - 2^-11) rounds, in fp32 (ulp 2^-8 there), to 65520 and stores inf, while
the exact sum, rounded once, would give 65504 -- a double rounding (torch's own fp64 -> fp16 conversion passes through fp32 as well and
gives inf).  The silent case here is therefore 16 - 2^-8, whose fp32 sum is TOP exactly; 16 - 2^-11 is kept as a case of its own in
which the word must equal the STORED pattern and the stored value must equal the fp32 emulation (inf).

Block outputs in the trunk test.  An overflow born at a block OUTPUT cannot be masked from later blocks (the residual carries it
to the features), so the net-level test covers the bn1 / bn2 sites only; block outputs are covered by the operator tests above.

Findings (each observed on the MI355X before its fix, see MEASURED; every fix leaves the stored outputs bit-identical -- the bitwise
tests of test_gpu_parity.py and the fp64 files pass -- and the benchmark unchanged):
  1. conv_pipe.hip, missed report: the register-epilogue (DIRECT) branch of conv_pipe_kernel -- configurations 4-7 -- noted into its
     per-thread maximum and left through a `return` with no ap_rng_flush: ap_set_conv_config(4..7) switched the sentinel off for
     every generic convolution of an fp16 handle.  Fix: the one missing flush.
  2. conv_pipe.hip / conv_slab.hip, false alarm: the 16-bit LDS-staged epilogues (ReLU, no residual: configurations 0-3, 8-13, 14 and
     the automatic choice; the slab kernel's fragment-tiled form too) noted when they WROTE THE STAGE, i.e. the whole tile with the
     rows past M and the channels past Cout, whose values (relu(shift), the padding's constants) are never stored.  Fix: the note
     moved to the masked 16-byte store (the same number of instructions).
  3. conv_img3.hip, conv_s2p.hip, block_img.hip, bottleneck2.hip, false alarm: the lanes of the padding / halo slots (columns 14, 15
     of a 16-slot row; halo row and column 0 / 15 of a 16 x 16 tile, which hold PARTIAL conv2 sums; a padding half image / quarter
     of the last group; t1 of a halo pixel outside the image, noted before it was replaced by zero) went into the maximum.  Fix: a
     per-unit maximum folded in only for stored units, the lane condition applied once at the flush, t1 noted after the zeroing.
  4. conv_lean.hip, pooling variant (ap_net_set_fuse_pool(1), off by default; reachable through ap_conv2d_pool_nhwc since ABI 13), false
     alarm: conv_lean_kernel<true> skipped the row / channel test in front of its note and so noted the 11 unused rows of a 5-image
     super-tile, the images past N and the channels past Cout -- finding 2 left in the one kernel no entry reached.  Fix: the note
     stands under the condition the stand-alone path stores under (row < M, channel < Cout, row of the super-tile < 245); pooled
     values and the stand-alone variant's stored bits are unchanged (the bitwise tests of test_trunk_forms_fp64.py and
     test_gpu_parity.py::test_fused_pool_is_bit_identical pass).

Not stored, but read by the next stage.  A value that a fused kernel does not store but hands to its next stage counts as stored:
the hidden t1 / t2 of the bottleneck kernels, y at the odd pixels under y_even (test_bottleneck64_sentinel[tail-1]) and, by the same
rule, `out` of the pair kernel at the odd pixels under out_even, which feeds conv1 of the next block (test_conv_pair_layout_sentinel):
nothing stored is non-finite there and the word must still be set.  conv_pair.hip keeps the rule as it is (its note sits in the
epilogue that packs `out`, before the store's mask).

CPU self-check (no GPU): an fp32 emulation of a tiled epilogue (fma, residual, ReLU, fp16 RNE, note per 16-byte store, flush)
reproduces the expected word on every case, and five seeded mutations of it are each rejected by the same assertions (MUTATIONS).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import MEAN_PARAMS
from test_conv_fwd_fp64 import SHAPES, _bn_dev, _cpad, _pad_rows, _pair_stream, _rows16, _untile, _w_dev, conv_sums
from test_stem_pool_fp64 import Guarded, _to_storage, operands

MEASURED = """
On an MI355X (256 CUs), python -m pytest tests/test_range_sentinel.py -m gpu -s: 62 GPU tests in 90 s, the slowest 5.9 s
(test_bottleneck64_sentinel[tail-0]), then 3.7 s; a launch of a sweep with its three device-side checks and the read of the word
costs about 0.12 ms.  Single overflows launched, each reported and each stored as exactly the one target element:
  ap_conv2d_nhwc       exhaustive: 17680 (128 x 128 tiles: 1, 5, 8, 10, 11, 14, 17), 9360 (128 x 64: 2, 6, 9, 12, 13), 18576 (256 x 64:
                       3, 7), 4752 (64 x 64: 100, -1); stratified 16388 (256 x 128: 0, 4); + 28 probes x 6 sign / residual variants and
                       25 silent shapes x 3 per configuration
  conv_pw_kernel       25091 per form      conv_img3_kernel 25092 per layout      conv_s2p_kernel 12548 per layout
  conv_pair_kernel     4100 in out and 4100 in t1n per (P, P2, N1)
  bottleneck2          25089 in y per variant, 12548 in t1n, 224 hidden-intermediate cases per variant     block_img 12548 in y, 902 hidden
  stem_pool(2)_kernel  3588 per form
Before the fixes (Findings), same tests: with the parent commit's conv_pipe.hip in the library configurations 4, 5, 6 and 7 each
failed at the first launch of their sweep ("word 0, but 1 stored elements are non-finite"); the silent cases failed with "word 1, but
0 stored elements are non-finite" under configurations -1, 0-3, 8-14 and 17 (17 on the stride-2 shape it hands to 11), and with
the masked-row bait in conv_img3 and conv_s2p (both layouts), all four bottleneck2 variants and block_img.  conv_pw, conv_pair,
conv_lean, conv_igemm, the stem and the pools passed unchanged.
The forms of ABI 13 (17 GPU tests, 10.5 s together, the slowest 1.4 s): test_conv_pool_sentinel 24 / 96 / 144 single overflows at N = 1 /
4 / 6; test_conv2d_forms_sentinel 44-56 per form and configuration; test_conv_pair_layout_sentinel 4100 in out (513 under out_even, odd
pixels included) and 4099-4100 in t1n per combination, with the full comparison against reference() on every 3001st launch and, for
the identity form, the residual boundary (65504 + 16 reported, 65504 + RES_LO silent) through the host-tiled residual.  Before the fix of finding 4, with the parent commit's conv_lean.hip in the
library, test_conv_pool_sentinel failed at its first silent case for N = 1, 4 and 6 alike:
("conv_pool N=1", "top", "word 1, but 0 stored elements are non-finite"); every other new case passed on the first run.
"""

PREC = "f16"
F16_MAX = 65504.0
OVF = 65520.0                                                # the midpoint above 65504: ties to even = inf
TOP = 65520.0 - 2.0 ** -8                                    # the largest fp32 below it: stores 65504
RES_LO = 16.0 - 2.0 ** -8                                    # 65504 + RES_LO = TOP exactly in fp32
RES_ISSUE = 16.0 - 2.0 ** -11                                # 65504 + this rounds to 65520 in fp32 (docstring: Residual boundary)
ALL_F16_CFGS = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 17, 100)

# (tile rows, tile width in channels) of every kernel, from its header comment / launch table
PIPE_TILES = {0: (256, 128), 1: (128, 128), 2: (128, 64), 3: (256, 64), 4: (256, 128), 5: (128, 128), 6: (128, 64), 7: (256, 64),
              8: (128, 128), 9: (128, 64), 10: (128, 128), 11: (128, 128), 12: (128, 64), 13: (128, 64),
              14: (128, 128), 17: (128, 128), 100: (64, 64), -1: (64, 64)}
DIRECT_CFGS = (4, 5, 6, 7)
TILES = {
    "conv_pw": (196, 256),        # 196 pixels x 256 channels, 64 per wave
    "conv_img3": (392, 128),      # half an image (28 rows x 14 columns) x 128 channels
    "conv_s2p": (196, 128),       # a quarter of an output image x 128 channels
    "conv_pair": (64, 128),       # four waves x 16 pixels; conv3 in chunks of 128 channels
    "bottleneck64": (196, 256),   # 14 x 14 output pixels x all 256 channels
    "bottleneck64_t1n": (196, 128),
    "block_img": (196, 128),      # an image x (conv3: 32 channels per wave, four waves)
    "stem_pool": (112, 64),       # a strip of two pooled rows x 64 channels
}


# ------------------------------------------------------------------------------------------------ positions
def exhaustive(M, C):
    return [(m, c) for m in range(M) for c in range(C)]


def stratified(M, C, rows, width, seed, pix_cell=None):
    """One stored element per cell of (pixel mod rows) x (channel pair mod width / 2), drawn with a seeded generator among the
    elements of the cell, plus the last pixel and the last channel pair (the ragged corner); sorted by pixel.
    pix_cell: pixel -> cell row, where the kernel's tile is not a run of consecutive pixels."""
    gen = torch.Generator().manual_seed(seed)
    pix_cell = pix_cell or (lambda m: m % rows)
    by_row = {}
    for m in range(M):
        by_row.setdefault(pix_cell(m), []).append(m)
    hw = width // 2
    out = set()
    for r, ms in sorted(by_row.items()):
        pm = torch.randint(0, len(ms), (hw,), generator=gen).tolist()
        for p in range(min(hw, C // 2)):
            pairs = list(range(p, C // 2, hw))
            q = pairs[int(torch.randint(0, len(pairs), (1,), generator=gen))]
            out.add((ms[pm[p]], 2 * q + int(torch.randint(0, 2, (1,), generator=gen))))
    out.update({(M - 1, C - 1), (M - 1, 0), (0, C - 1), (0, 0)})
    return sorted(out)


def cells_of(positions, rows, width, pix_cell=None):
    pix_cell = pix_cell or (lambda m: m % rows)
    return {(pix_cell(m), (c // 2) % (width // 2)) for m, c in positions}


def probes(M, C, rows, width):
    """A handful of positions for the variants that are not swept: tile corners, the first and last element of the ragged tail in
    both directions, and every position of a 16-byte store (channel mod 8)"""
    ms = sorted({0, 1, min(rows, M) - 1, (M - 1) // rows * rows, M - 1})
    cs = sorted({0, 1, 2, 3, 4, 5, 6, 7, min(width, C) - 1, (C - 1) // width * width, C - 2, C - 1})
    return [(m, cs[(i + j) % len(cs)]) for i, m in enumerate(ms) for j in range(0, len(cs), 3)] + [(ms[-1], c) for c in cs[:8]]


def img3_cell(m):
    """conv_img3: a workgroup owns 14 of the 28 columns over all rows -> cell row = (image row, column mod 14)"""
    r, c = divmod(m % 784, 28)
    return r * 14 + c % 14


def quarter_cell(m):
    """conv_s2p: a workgroup owns a 14 x 14 quarter of the 28 x 28 output image"""
    r, c = divmod(m % 784, 28)
    return (r % 14) * 14 + c % 14


def tile14_cell(W):
    """bottleneck2: 14 x 14 tiles of an H x W image"""
    def f(m):
        r, c = divmod(m, W)
        return (r % 14) * 14 + c % 14
    return f


def strip_cell(m):
    """stem + max-pool: a strip of two pooled rows of 56 pixels"""
    return m % 112


# the sweeps of the fixed-shape kernels: name -> (M, C, rows, width, seed, pixel -> cell row)
SWEEPS = {
    "conv_pw": (392, 512, 196, 256, 11, None),
    "conv_img3": (2 * 784, 128, 392, 128, 12, img3_cell),
    "conv_s2p": (2 * 784, 128, 196, 128, 13, quarter_cell),
    "conv_pair_512": (245, 512, 64, 128, 14, None),
    "conv_pair_1024": (245, 1024, 64, 128, 15, None),
    "conv_pair_t1n_128": (245, 128, 64, 128, 16, None),
    "conv_pair_t1n_256": (245, 256, 64, 128, 17, None),
    "bottleneck64": (14 * 28, 256, 196, 256, 18, tile14_cell(28)),
    "bottleneck64_t1n": (14 * 28, 128, 196, 128, 19, tile14_cell(28)),
    "block_img": (2 * 196, 1024, 196, 128, 20, None),
    "stem_pool": (2 * 56 * 56, 64, 112, 64, 21, strip_cell),
}
_SAMPLES = {}


def sample(name):
    if name not in _SAMPLES:
        M, C, rows, width, seed, cell = SWEEPS[name]
        _SAMPLES[name] = stratified(M, C, rows, width, seed, cell)
    return _SAMPLES[name]


def conv2d_sweep_shape(cfg):
    """(shape, positions) of the one-overflow sweep of a configuration: one full tile and a ragged tail in both directions"""
    rows, width = PIPE_TILES[cfg]
    M, C = rows + 2, width + 8
    k = 3 if cfg == 14 else 1                                # the slab kernel takes 3 x 3 / 1 / 1 only (other shapes run configuration 11)
    H, W = {66: (6, 11), 130: (10, 13), 258: (6, 43)}[M]
    shp = ("sweep_%d" % cfg, 1, H, W, 64, C, k, 1, k // 2)
    pos = exhaustive(M, C) if M * C <= 32768 else stratified(M, C, rows, width, 100 + cfg)
    return shp, pos


# ------------------------------------------------------------------------------------------------ reference and emulation (CPU)
def conv_case(shp, kind, pos=None, relu=1):
    """The operands of one ap_conv2d_nhwc case as fp32 tensors holding exactly representable values.
    kind: top | rowbait | bait | one | neg | res_hi | res_lo | res_issue (docstring)"""
    name, N, H, W, Cin, Cout, k, s, p = shp
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    M = N * Ho * Wo
    x = torch.zeros(N * H * W, Cin)
    w = torch.zeros(Cout, k, k, Cin)
    w[:, k // 2, k // 2, 0] = 1.0
    scale, shift, res = torch.ones(Cout), torch.zeros(Cout), None

    def in_pixel(m):
        n, r = divmod(m, Ho * Wo)
        ho, wo = divmod(r, Wo)
        return (n * H + ho * s) * W + wo * s                 # the centre tap of output pixel m (pad = k // 2)
    if kind == "top":
        x[:, 0] = 1.0
        scale[:] = TOP
    elif kind == "rowbait":                                  # stored: fma(1, -16, 65520) = 65504; a masked row (accumulator 0): 65520
        x[:, 0] = 1.0
        scale[:] = -16.0
        shift[:] = OVF
    elif kind == "bait":
        res = torch.zeros(M, Cout)
        for m in (0, M - 1):
            x[in_pixel(m), 0] = 1.0
            res[m] = -16.0
        scale[:] = OVF
    else:
        m, c = pos
        x[in_pixel(m), 0] = 1.0
        if kind == "one":
            scale[c] = OVF
        elif kind == "neg":
            scale[c] = -OVF
        else:
            res = torch.zeros(M, Cout)
            res[m, c] = F16_MAX
            scale[c] = {"res_hi": 16.0, "res_lo": RES_LO, "res_issue": RES_ISSUE}[kind]
    return dict(shp=shp, M=M, Ho=Ho, Wo=Wo, x=x.view(N, H, W, Cin), w=w, scale=scale, shift=shift, res=res, relu=relu, kind=kind)


def reference(cs):
    """torch fp64 on the same data, then ONE rounding to fp16: [M][Cout] float16"""
    s, p = cs["shp"][7], cs["shp"][8]
    c, _ = conv_sums(cs["x"], cs["w"], s, p)
    v = c.reshape(cs["M"], -1) * cs["scale"].double() + cs["shift"].double()
    if cs["res"] is not None:
        v = v + cs["res"].double()
    if cs["relu"]:
        v = v.clamp_min(0)
    return v.to(torch.float16)


SILENT = ("top", "rowbait", "bait")
MUTATIONS = ("drop_flush_direct", "drop_dword", "drop_sign_mask", "note_before_mask", "gt_not_ge")


def emulate(cs, rows, width, direct=False, mut=None):
    """fp32 emulation of a tiled epilogue on the tiles of (rows x width): the rows past M have the accumulator 0 (loads predicated to
    a zero line) and no residual, the channels past Cout carry the padding's constants; fma, + residual, ReLU, fp16 round-to-nearest-
    even, one note per 16-byte store of the STORED elements (sign bits masked when there is no ReLU), flush on >= 0x7c00.
    Returns (word, stored [M][Cout] float16)."""
    s, p = cs["shp"][7], cs["shp"][8]
    M, Cout = cs["M"], cs["shp"][5]
    Mp, Cp = (M + rows - 1) // rows * rows, (Cout + width - 1) // width * width
    acc = conv_sums(cs["x"], cs["w"], s, p)[0].float().reshape(M, Cout)              # (exact: one product per element)
    accp = torch.zeros(Mp, Cp)
    accp[:M, :Cout] = acc
    scale, shift = torch.ones(Cp), torch.full((Cp,), 1.0e6)
    scale[:Cout], shift[:Cout] = cs["scale"], cs["shift"]
    v = accp * scale + shift                                 # fp32
    if cs["res"] is not None:
        v[:M, :Cout] = v[:M, :Cout] + cs["res"]
    if cs["relu"]:
        v = v.clamp_min(0)
    h = v.to(torch.float16)
    bits = h.view(torch.int16).to(torch.int32) & 0xffff
    noted = torch.zeros(Mp, Cp, dtype=torch.bool)
    noted[:M, :Cout] = True
    if mut == "note_before_mask":
        noted[:] = True
    if mut == "drop_dword":
        noted[:, (torch.arange(Cp) % 8) // 2 == 3] = False
    if cs["relu"] or mut == "drop_sign_mask":                # signed 16-bit maximum: a set sign bit never wins
        key = torch.where(bits >= 0x8000, torch.zeros_like(bits), bits)
    else:
        key = bits & 0x7fff
    m = int(key[noted].max())
    word = (m > 0x7c00) if mut == "gt_not_ge" else (m >= 0x7c00)
    if mut == "drop_flush_direct" and direct:
        word = False
    return bool(word), h[:M, :Cout]


def assert_case(what, word, stored, ref):
    """The assertions of every case: the stored tensor equals the reference (same non-finite pattern, same finite values), and the
    word says whether any stored element is non-finite"""
    bad, rbad = ~torch.isfinite(stored.float()), ~torch.isfinite(ref.float())
    assert torch.equal(bad, rbad), (what, "stored non-finite at %d elements, reference at %d" % (int(bad.sum()), int(rbad.sum())))
    assert torch.equal(stored.float()[~bad], ref.float()[~rbad]), (what, "finite values differ from the reference")
    assert torch.equal(stored.float()[bad], ref.float()[rbad]), (what, "non-finite values differ from the reference (sign, NaN)")
    assert bool(word) == bool(rbad.any()), (what, "word %d, but %d stored elements are non-finite" % (int(word), int(rbad.sum())))


def cpu_cases(cfg):
    """The cases of a configuration the CPU self-check runs: every kind, the sweep thinned to the probes"""
    rows, width = PIPE_TILES[cfg]
    shp, _ = conv2d_sweep_shape(cfg)
    M, C = rows + 2, width + 8
    out = [conv_case(shp, "top"), conv_case(shp, "rowbait"), conv_case(shp, "bait")]
    for pos in probes(M, C, rows, width):
        out.append(conv_case(shp, "one", pos))
        for relu in (0, 1):
            out += [conv_case(shp, kind, pos, relu) for kind in ("neg", "res_hi", "res_lo")]
    return out


@pytest.mark.parametrize("cfg", [1, 5, 100])
def test_cpu_emulation_reproduces_the_word_and_mutations_are_rejected(cfg):
    """The fp32 emulation passes the assertions of the GPU tests on every case of a staged (1), a register-epilogue (5) and a
    64 x 64-tile (100) configuration plus the ragged tails of the silent list; each mutation fails them on at least one case."""
    rows, width = PIPE_TILES[cfg]
    direct = cfg in DIRECT_CFGS
    cases = cpu_cases(cfg) + [conv_case(s, k) for s in SHAPES[:6] for k in SILENT]
    refs = [reference(cs) for cs in cases]
    for cs, ref in zip(cases, refs):
        word, stored = emulate(cs, rows, width, direct)
        assert_case((cfg, cs["shp"][0], cs["kind"]), word, stored, ref)
    for mut in MUTATIONS:
        if mut == "drop_flush_direct" and not direct:
            continue
        rejected = 0
        for cs, ref in zip(cases, refs):
            word, stored = emulate(cs, rows, width, direct, mut)
            try:
                assert_case((cfg, mut), word, stored, ref)
            except AssertionError:
                rejected += 1
        assert rejected > 0, (cfg, mut, "no case rejects this mutation")
    # the issue's residual value: fp32 stores inf where fp64 + one rounding stores 65504 (docstring: Residual boundary)
    cs = conv_case(conv2d_sweep_shape(cfg)[0], "res_issue", (3, 5))
    word, stored = emulate(cs, rows, width, direct)
    assert word and bool(torch.isinf(stored[3, 5])) and F16_MAX + RES_ISSUE < OVF          # (the exact sum is below the midpoint)
    for kind, want in (("res_lo", F16_MAX), ("res_hi", float("inf"))):
        cs = conv_case(conv2d_sweep_shape(cfg)[0], kind, (3, 5))
        assert float((torch.tensor(F16_MAX) + cs["scale"][5]).to(torch.float16)) == want      # the fp32 sum, rounded once


def test_boundary_values_are_exact():
    """TOP and OVF as fp32 and as fp16: the derivation of the docstring on the host's own conversions"""
    t, o = torch.tensor(TOP, dtype=torch.float32), torch.tensor(OVF, dtype=torch.float32)
    assert float(t) == TOP and float(o) == OVF and float(torch.nextafter(t, o)) == OVF
    assert float(t.to(torch.float16)) == F16_MAX and bool(torch.isinf(o.to(torch.float16)))
    assert float((-t).to(torch.float16)) == -F16_MAX and float((-o).to(torch.float16)) == float("-inf")
    assert float(torch.tensor(F16_MAX) + torch.tensor(RES_LO)) == TOP and float(torch.tensor(F16_MAX) + torch.tensor(16.0)) == OVF
    assert float(torch.tensor(F16_MAX) + torch.tensor(RES_ISSUE)) == OVF         # fp32: the sum rounds up to the midpoint
    assert torch.finfo(torch.float16).max == F16_MAX


def test_samples_cover_every_store_slot():
    """Every sweep hits every cell of (pixel mod tile rows) x (channel pair mod tile width) of its kernel, both ends of the ragged
    tail, and -- where the kernel stores 16 bytes at a time -- every dword of the store"""
    for cfg in ALL_F16_CFGS:
        rows, width = PIPE_TILES[cfg]
        shp, pos = conv2d_sweep_shape(cfg)
        M, C = rows + 2, width + 8
        assert shp[1] * shp[2] * shp[3] == M and shp[5] == C and M > rows and C > width
        assert cells_of(pos, rows, width) == {(r, p) for r in range(rows) for p in range(width // 2)}, cfg
        assert any(m >= rows for m, _ in pos) and any(c >= width for _, c in pos) and (M - 1, C - 1) in pos
        assert M * C > 32768 or len(pos) == M * C
    for name, (M, C, rows, width, _, cell) in SWEEPS.items():
        pos = sample(name)
        want = {(r, p) for r in range(rows) for p in range(min(width, C) // 2)}
        assert cells_of(pos, rows, width, cell) == want, name
        assert {c % 8 for _, c in pos} == set(range(8)) and all(0 <= m < M and 0 <= c < C for m, c in pos), name
        assert len(pos) <= len(want) + 4 and M > rows, name
    for name, (rows, width) in TILES.items():
        hits = [v for k, v in SWEEPS.items() if k == name or k.startswith(name + "_")]
        assert hits and all(v[2] == rows and v[3] <= width for v in hits), name


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


class Hook(object):
    """The range hook switched on for a block of code; word() = synchronise, read and clear"""

    def __init__(self, dev, prec=PREC):
        self.Nn, self.L = _lib()
        self.dev, self.PR = dev, self.Nn.PRECISIONS[prec]

    def __enter__(self):
        self.Nn.check(self.L.ap_debug_set_range_hook(1), "ap_debug_set_range_hook")
        return self

    def __exit__(self, *exc):
        self.L.ap_debug_set_range_hook(0)

    def word(self):
        rc = self.L.ap_debug_range_status(self.PR, self.Nn.stream_ptr(self.dev), 1)
        assert rc in (0, self.Nn.AP_ERANGE), rc
        return rc != 0


def h16(t, dev):
    return t.to(torch.float16).contiguous().to(dev)


class Op(object):
    """One operator entry on one set of device buffers.  Subclasses provide launch() and the index maps; the tests move the
    impulse (x_flat), single BatchNorm entries and single residual elements between launches."""
    out_layout = None                                        # None: NHWC rows [M][C]; "tiled": fragment-tiled

    def in_index(self, m):
        raise NotImplementedError

    def out_index(self, m, c):
        if self.out_layout == "tiled":
            return ((m >> 4) * (self.C >> 3) + (c >> 3)) * 128 + (m & 15) * 8 + (c & 7)
        return m * self.C + c

    def stored(self, what):
        """[M][C] float16 on the host; guards intact, every element written"""
        v = self.g.values((self.M * self.C,), what)
        t = self.g.out.view(self.M, self.C)
        if self.out_layout == "tiled":
            t = _untile(self.g.out, self.M, self.C)
        return t.cpu()


def sweep(hook, op, positions, what, scale, val=OVF, base=1.0, full=None, full_every=3001, other=()):
    """One launch per position: the impulse at pixel m, scale[c] = val; exactly one stored element must be non-finite -- the target --
    and the word must be set.  full(m, c) -> reference [M][C] float16 for the complete comparison on every full_every-th launch.
    other: further Ops-like outputs (Guarded) that must stay finite."""
    words, cnts, hits, extra = [], [], [], []
    cur = None
    hook.word()
    for i, (m, c) in enumerate(positions):
        if m != cur:
            if cur is not None:
                op.x_flat[op.in_index(cur)] = 0.0
            op.x_flat[op.in_index(m)] = op.impulse
            cur = m
        scale[c] = val
        op.launch()
        bad = ~torch.isfinite(op.g.out)
        cnts.append(bad.sum())
        hits.append(bad[op.out_index(m, c)])
        for g in other:
            extra.append((~torch.isfinite(g.out)).sum())
        words.append(hook.word())
        if full is not None and i % full_every == 0:
            assert_case((what, m, c), words[-1], op.stored(what), full(m, c))
        scale[c] = base
    if cur is not None:
        op.x_flat[op.in_index(cur)] = 0.0
    cnts, hits = torch.stack(cnts).cpu(), torch.stack(hits).cpu()
    missed = [positions[i] for i, w in enumerate(words) if not w]
    assert not missed, (what, "%d of %d single overflows not reported, first (pixel, channel): %s" % (len(missed), len(words), missed[:6]))
    wrong = [positions[i] for i in range(len(positions)) if int(cnts[i]) != 1 or not bool(hits[i])]
    assert not wrong, (what, "stored pattern is not the one target element at (pixel, channel): %s" % wrong[:6])
    if extra:
        assert int(torch.stack(extra).sum()) == 0, (what, "the other output holds non-finite values")
    op.g.values((op.M * op.C,), what)
    return len(positions)


def one_by_one(hook, op, positions, what, setup, want_word, want_bad, other=()):
    """The variants that are not swept: per position, setup(m, c) -> undo(); launch; assert the word and the number of non-finite
    stored elements (and that the target is among them)"""
    hook.word()
    for m, c in positions:
        op.x_flat[op.in_index(m)] = op.impulse
        undo = setup(m, c)
        op.launch()
        w = hook.word()
        bad = ~torch.isfinite(op.g.out)
        assert int(bad.sum()) == want_bad and (not want_bad or bool(bad[op.out_index(m, c)])), (what, m, c, int(bad.sum()))
        assert w == want_word, (what, m, c, "word %d" % w)
        for g in other:
            assert bool(torch.isfinite(g.out).all()), (what, m, c, "the other output holds non-finite values")
        undo()
        op.x_flat[op.in_index(m)] = 0.0


# ---- ap_conv2d_nhwc
class Conv2d(Op):
    impulse = 1.0

    def __init__(self, dev, shp):
        name, N, H, W, Cin, Cout, k, s, p = shp
        self.shp, self.dev = shp, dev
        self.Ho, self.Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.M, self.C = N * self.Ho * self.Wo, Cout
        self.x = torch.zeros(N * H * W, Cin, dtype=torch.float16, device=dev)
        self.x_flat = self.x.view(-1)
        w = torch.zeros(Cout, k, k, Cin)
        w[:, k // 2, k // 2, 0] = 1.0
        self.w = _w_dev(w, PREC, dev)
        # the channel padding computes 1e6 (never stored): a kernel that notes a masked channel raises a false alarm
        self.scale = _pad_rows(torch.ones(Cout), _cpad(Cout), 1.0).to(dev)
        self.shift = _pad_rows(torch.zeros(Cout), _cpad(Cout), 1.0e6).to(dev)
        self.res = torch.zeros(self.M, Cout, dtype=torch.float16, device=dev)
        self.g = Guarded(dev, PREC, self.M * Cout)
        self.relu, self.use_res = 1, False

    def in_index(self, m):
        name, N, H, W, Cin, Cout, k, s, p = self.shp
        n, r = divmod(m, self.Ho * self.Wo)
        ho, wo = divmod(r, self.Wo)
        return ((n * H + ho * s) * W + wo * s) * Cin

    def launch(self):
        Nn, L = _lib()
        name, N, H, W, Cin, Cout, k, s, p = self.shp
        rc = L.ap_conv2d_nhwc(Nn.PRECISIONS[PREC], _p(self.x), _p(self.w), _p(self.scale), _p(self.shift), _p(self.res) if self.use_res else None,
                              _p(self.g.out), N, H, W, Cin, Cout, k, s, p, self.relu, Nn.stream_ptr(self.dev))
        assert rc == 0, (self.shp, "ap_conv2d_nhwc status %d" % rc)

    def load(self, cs):
        """the operands of a conv_case"""
        self.x.copy_(cs["x"].reshape(self.x.shape).to(torch.float16))
        self.scale[:self.C] = cs["scale"].to(self.dev)
        self.shift[:self.C] = cs["shift"].to(self.dev)
        self.use_res = cs["res"] is not None
        if self.use_res:
            self.res.copy_(cs["res"].to(torch.float16))
        self.relu = cs["relu"]

    def clear(self):
        self.x.zero_(); self.res.zero_()
        self.scale[:self.C] = 1.0
        self.shift[:self.C] = 0.0
        self.relu, self.use_res = 1, False


_REFS = {}


def run_case(hook, op, cs, what, key=None):
    """key: the reference of this case does not depend on the configuration -- computed once, then shared"""
    op.load(cs)
    hook.word()
    op.launch()
    w = hook.word()
    if key is None or key not in _REFS:
        ref = reference(cs)
        if key is not None:
            _REFS[key] = ref
    else:
        ref = _REFS[key]
    assert_case(what, w, op.stored(what), ref)
    op.clear()


@gpu
@pytest.mark.parametrize("cfg", ALL_F16_CFGS)
def test_conv2d_sentinel(dev, cfg):
    """ap_conv2d_nhwc under one configuration: silent at the top of the range (and with the bait) on every shape of
    test_conv_fwd_fp64.SHAPES; one overflow at every store slot; both signs; the residual add, with and without ReLU."""
    Nn, L = _lib()
    rows, width = PIPE_TILES[cfg]
    Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
    try:
        with Hook(dev) as hook:
            for shp in SHAPES:
                op = Conv2d(dev, shp)
                for kind in SILENT:
                    run_case(hook, op, conv_case(shp, kind), "cfg=%d %s %s" % (cfg, shp[0], kind), key=(shp[0], kind))
            shp, pos = conv2d_sweep_shape(cfg)
            op = Conv2d(dev, shp)
            what = "cfg=%d %s" % (cfg, shp[0])
            n = sweep(hook, op, pos, what, op.scale, full=lambda m, c: reference(conv_case(shp, "one", (m, c))))
            few = probes(op.M, op.C, rows, width)
            for relu in (0, 1):
                for kind in ("neg", "res_hi", "res_lo"):
                    for pp in few:
                        run_case(hook, op, conv_case(shp, kind, pp, relu), "%s %s relu=%d %s" % (what, kind, relu, pp))
            # the issue's residual value: the word must equal the STORED pattern, which is the fp32 epilogue's (docstring)
            cs = conv_case(shp, "res_issue", few[3])
            op.load(cs)
            op.launch()
            w, st = hook.word(), op.stored(what)
            assert torch.equal(st, emulate(cs, rows, width)[1]) and w == bool((~torch.isfinite(st.float())).any()) and w, (what, "res_issue")
            op.clear()
        print("%-34s %d single overflows, %d probes x 6 variants, %d silent shapes x 3" % ("ap_conv2d_nhwc f16 cfg=%d" % cfg, n, len(few), len(SHAPES)))
    finally:
        L.ap_set_conv_config(-1)


@gpu
@pytest.mark.parametrize("shp", [("igemm_128x64", 1, 2, 6145, 64, 8, 1, 1, 0), ("igemm_128x128", 1, 2, 8193, 64, 136, 1, 1, 0)], ids=lambda s: s[0])
def test_conv_igemm_large_tiles(dev, shp):
    """The two larger instantiations of conv_igemm_kernel (configuration 100: 128 x 64 tiles when Cout <= 64 and M > 12288,
    128 x 128 when there are 256 tiles of that size), at the smallest sizes that select them: silent, and single overflows at the
    probes of the first, an inner and the last (ragged) tile."""
    Nn, L = _lib()
    rows, width = (128, 64) if shp[5] <= 64 else (128, 128)
    Nn.check(L.ap_set_conv_config(100), "ap_set_conv_config")
    try:
        with Hook(dev) as hook:
            op = Conv2d(dev, shp)
            for kind in SILENT:
                run_case(hook, op, conv_case(shp, kind), "%s %s" % (shp[0], kind))
            M, C = op.M, op.C
            base = probes(rows + 2, C, rows, width)
            pos = sorted(set(base + [(m + 37 * rows, c) for m, c in base] + [(M - 1 - m, c) for m, c in base if m < 2 * rows]))
            sweep(hook, op, pos, shp[0], op.scale, full=lambda m, c: reference(conv_case(shp, "one", (m, c))), full_every=41)
    finally:
        L.ap_set_conv_config(-1)


# ---- conv_pw.hip
class ConvPw(Op):
    """ap_conv_pw_nhwc (plain, with a residual on request), ap_conv_pw_ds_nhwc, ap_conv_pw_k3s2_nhwc at M = 392 = two pixel tiles,
    Cout = 512 = two channel tiles"""
    impulse = 1.0

    def __init__(self, dev, form):
        Nn, L = _lib()
        self.dev, self.form = dev, form
        self.M, self.C = 392, 512
        st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[PREC]
        if form == "plain":
            self.Cin, K = 256, 256
            self.x = torch.zeros(392, 256, dtype=torch.float16, device=dev)
            w = torch.zeros(512, K); w[:, 0] = 1.0
        elif form == "ds":
            self.Cin, self.Cin2, K = 128, 128, 256
            self.x = torch.zeros(392, 128, dtype=torch.float16, device=dev)                  # t2 [2][14][14][128]
            self.x2 = torch.zeros(2 * 28 * 28, 128, dtype=torch.float16, device=dev)
            w = torch.zeros(512, K); w[:, 0] = 1.0
        else:
            self.Cin, K = 128, 9 * 128
            self.x = torch.zeros(2 * 28 * 28, 128, dtype=torch.float16, device=dev)
            w = torch.zeros(512, 3, 3, 128); w[:, 1, 1, 0] = 1.0
            w = w.reshape(512, K)
        self.x_flat = self.x.view(-1)
        self.w_rows = w
        wd = h16(w, dev)
        self.ws = torch.empty(L.ap_conv_pw_stream_bytes(K, 512), dtype=torch.uint8, device=dev)
        Nn.check(L.ap_conv_pw_pack(PR, _p(wd), K, 512, _p(self.ws), st), "ap_conv_pw_pack")
        self.scale, self.shift = torch.ones(512, device=dev), torch.zeros(512, device=dev)
        self.res = torch.zeros(392, 512, dtype=torch.float16, device=dev)
        self.use_res = False
        self.g = Guarded(dev, PREC, 392 * 512)

    def in_index(self, m):
        if self.form == "k3s2":
            n, r = divmod(m, 196)
            ho, wo = divmod(r, 14)
            return ((n * 28 + 2 * ho) * 28 + 2 * wo) * 128
        return m * self.Cin

    def launch(self):
        Nn, L = _lib()
        st, PR = Nn.stream_ptr(self.dev), Nn.PRECISIONS[PREC]
        if self.form == "plain":
            rc = L.ap_conv_pw_nhwc(PR, _p(self.x), _p(self.ws), _p(self.scale), _p(self.shift), _p(self.res) if self.use_res else None,
                                   _p(self.g.out), 392, 256, 512, st)
        elif self.form == "ds":
            rc = L.ap_conv_pw_ds_nhwc(PR, _p(self.x), _p(self.x2), _p(self.ws), _p(self.scale), _p(self.shift), _p(self.g.out), 2, 14, 128, 128, 512, 2, st)
        else:
            rc = L.ap_conv_pw_k3s2_nhwc(PR, _p(self.x), _p(self.ws), _p(self.scale), _p(self.shift), _p(self.g.out), 2, 28, 128, 512, st)
        assert rc == 0, (self.form, rc)

    def reference(self):
        """fp64 + one rounding on the operands as they are on the device: [M][C] float16"""
        xs = self.x.cpu().double()
        if self.form == "k3s2":
            acc = conv_sums(xs.view(2, 28, 28, 128), self.w_rows.view(512, 3, 3, 128), 2, 1)[0].reshape(392, 512)
        elif self.form == "ds":
            x2 = self.x2.cpu().double().view(2, 28, 28, 128)[:, ::2, ::2].reshape(392, 128)
            acc = torch.cat([xs, x2], 1) @ self.w_rows.double().t()
        else:
            acc = xs @ self.w_rows.double().t()
        v = acc * self.scale.cpu().double() + self.shift.cpu().double()
        if self.use_res:
            v = v + self.res.cpu().double()
        return v.clamp_min(0).to(torch.float16)


def check_now(hook, op, what):
    """launch on the operands as they are; the full assertions against the fp64 reference of those operands"""
    hook.word()
    op.launch()
    assert_case(what, hook.word(), op.stored(what), op.reference())


@gpu
@pytest.mark.parametrize("form", ["plain", "ds", "k3s2"])
def test_conv_pw_sentinel(dev, form):
    """conv_pw_kernel in its three operand forms: silent at the top; one overflow per store slot (stratified: TILES); plain form:
    the residual add at the probes"""
    with Hook(dev) as hook:
        op = ConvPw(dev, form)
        what = "conv_pw " + form
        if form == "k3s2":
            op.x.view(2, 28, 28, 128)[:, ::2, ::2, 0] = 1.0
        else:
            op.x[:, 0] = 1.0
        op.scale[:] = TOP
        check_now(hook, op, what + " top")
        assert bool((op.g.out == F16_MAX).all())
        op.scale[:] = -16.0; op.shift[:] = OVF              # 65504 stored; a junk slot of the 208-slot tile (accumulator 0) computes 65520
        check_now(hook, op, what + " rowbait")
        assert bool((op.g.out == F16_MAX).all())
        op.x.zero_(); op.scale[:] = 1.0; op.shift[:] = 0.0
        pos = sample("conv_pw")

        def full(m, c):
            return op.reference()
        n = sweep(hook, op, pos, what, op.scale, full=full)
        if form == "plain":
            op.use_res = True
            few = probes(392, 512, 196, 256)
            for sval, word, nbad in ((16.0, True, 1), (RES_LO, False, 0)):
                def setup(m, c):
                    op.res[m, c] = F16_MAX
                    op.scale[c] = sval

                    def undo():
                        op.res[m, c] = 0.0
                        op.scale[c] = 1.0
                    return undo
                one_by_one(hook, op, few, "%s res + %r" % (what, sval), setup, word, nbad)
            m, c = few[5]
            op.x_flat[op.in_index(m)] = 1.0; op.res[m, c] = F16_MAX; op.scale[c] = RES_LO
            check_now(hook, op, what + " res_lo full")
            # the bait: the stored rows hold 65520 - 16, a copy of them without the residual would overflow
            op.x.zero_(); op.res.zero_(); op.scale[:] = OVF
            for mm in (0, 391):
                op.x[mm, 0] = 1.0; op.res[mm] = -16.0
            check_now(hook, op, what + " bait")
        print("%-34s %d single overflows" % (what, n))


# ---- conv_img3.hip / conv_s2p.hip
class ConvImg(Op):
    impulse = 1.0

    def __init__(self, dev, kernel, tiled):
        Nn, L = _lib()
        self.dev, self.kernel, self.tiled = dev, kernel, tiled
        self.out_layout = "tiled" if tiled else None
        self.H = 28 if kernel == "img3" else 56
        self.M, self.C = 2 * 784, 128
        st, PR = Nn.stream_ptr(dev), Nn.PRECISIONS[PREC]
        self.x = torch.zeros(2 * self.H * self.H, 128, dtype=torch.float16, device=dev)
        self.x_flat = self.x.view(-1)
        self.w = torch.zeros(128, 3, 3, 128); self.w[:, 1, 1, 0] = 1.0
        nbytes, pack, self.run = ((L.ap_conv_img3_stream_bytes, L.ap_conv_img3_pack, L.ap_conv_img3_nhwc) if kernel == "img3" else
                                  (L.ap_conv_s2p_stream_bytes, L.ap_conv_s2p_pack, L.ap_conv_s2p_nhwc))
        self.ws = torch.empty(nbytes(), dtype=torch.uint8, device=dev)
        Nn.check(pack(PR, _p(h16(self.w, dev)), _p(self.ws), st), "pack")
        self.scale, self.shift = torch.ones(128, device=dev), torch.zeros(128, device=dev)
        self.g = Guarded(dev, PREC, self.M * 128)

    def in_index(self, m):
        s = 1 if self.kernel == "img3" else 2
        n, r = divmod(m, 784)
        ho, wo = divmod(r, 28)
        return ((n * self.H + s * ho) * self.H + s * wo) * 128

    def launch(self):
        Nn, L = _lib()
        rc = self.run(Nn.PRECISIONS[PREC], _p(self.x), _p(self.ws), _p(self.scale), _p(self.shift), _p(self.g.out), 2, self.tiled, Nn.stream_ptr(self.dev))
        assert rc == 0, (self.kernel, rc)

    def reference(self):
        s = 1 if self.kernel == "img3" else 2
        acc = conv_sums(self.x.cpu().double().view(2, self.H, self.H, 128), self.w, s, 1)[0].reshape(self.M, 128)
        return (acc * self.scale.cpu().double() + self.shift.cpu().double()).clamp_min(0).to(torch.float16)


@gpu
@pytest.mark.parametrize("tiled", [0, 1], ids=["nhwc", "tiled"])
@pytest.mark.parametrize("kernel", ["img3", "s2p"])
def test_img3_s2p_sentinel(dev, kernel, tiled):
    """conv_img3_kernel / conv_s2p_kernel, NHWC and fragment-tiled output, two images: silent at the top; one overflow per store
    slot of the half image / quarter (stratified: TILES)"""
    with Hook(dev) as hook:
        op = ConvImg(dev, kernel, tiled)
        what = "conv_%s tiled=%d" % (kernel, tiled)
        s = 1 if kernel == "img3" else 2
        op.x.view(2, op.H, op.H, 128)[:, ::s, ::s, 0] = 1.0
        op.scale[:] = TOP
        check_now(hook, op, what + " top")
        assert bool((op.g.out == F16_MAX).all())
        op.scale[:] = -16.0; op.shift[:] = OVF              # 65504 stored; a halo / junk slot (accumulator 0) computes 65520
        check_now(hook, op, what + " rowbait")
        assert bool((op.g.out == F16_MAX).all())
        op.x.zero_(); op.scale[:] = 1.0; op.shift[:] = 0.0
        n = sweep(hook, op, sample("conv_" + kernel), what, op.scale, full=lambda m, c: op.reference())
        print("%-34s %d single overflows" % (what, n))


# ---- conv_pair.hip
class Pair(Op):
    """ap_conv_pair_nhwc / ap_conv_pair_ds_nhwc at M = 245 = three 64-pixel tiles and a ragged one.  which = "out": the overflow is
    born in `out` (w3 = 1 on input channel 0; w1 = -1 on EVERY input channel, so t1n = relu(-inf) = 0); which = "t1n": it is born in
    t1n (w3 row 0 only: out[m][0] = 1; w1 = 1 on input channel 0: the accumulator of conv1 is 1; s1 carries the boundary)"""
    impulse = 1.0

    def __init__(self, dev, P, P2, N1, which):
        Nn, L = _lib()
        self.dev, self.P, self.P2, self.N1, self.which = dev, P, P2, N1, which
        C3 = 4 * P
        self.M, self.C = 245, (C3 if which == "out" else N1)
        self.x = torch.zeros(245, P, dtype=torch.float16, device=dev)                        # t2
        self.x_flat = self.x.view(-1)
        self.x2 = torch.zeros(5 * 14 * 14, max(P2, 8), dtype=torch.float16, device=dev)
        w3, w1 = torch.zeros(C3, P + P2), torch.zeros(max(N1, 8), C3)
        if which == "out":
            w3[:, 0] = 1.0
            w1[:] = -1.0
        else:
            w3[0, 0] = 1.0
            w1[:, 0] = 1.0
        self.w3, self.w1 = w3, w1
        self.ws = _pair_stream(dev, PREC, h16(w3, dev), h16(w1, dev), P, P2, N1)
        self.s3, self.h3 = torch.ones(C3, device=dev), torch.zeros(C3, device=dev)
        self.s1, self.h1 = torch.ones(max(N1, 8), device=dev), torch.zeros(max(N1, 8), device=dev)
        self.res = torch.zeros(245, C3, dtype=torch.float16, device=dev)
        self.go, self.gt = Guarded(dev, PREC, 245 * C3), Guarded(dev, PREC, 245 * max(N1, 8))
        self.g = self.go if which == "out" else self.gt

    def in_index(self, m):
        return m * self.P

    def launch(self):
        Nn, L = _lib()
        st, PR = Nn.stream_ptr(self.dev), Nn.PRECISIONS[PREC]
        if self.P2:
            n1 = self.N1 > 0
            rc = L.ap_conv_pair_ds_nhwc(PR, _p(self.x), _p(self.x2), _p(self.ws), _p(self.s3), _p(self.h3), _p(self.s1) if n1 else None,
                                        _p(self.h1) if n1 else None, _p(self.go.out), _p(self.gt.out) if n1 else None, 5, 7, self.P, self.P2, 2, self.N1, st)
        else:
            rc = L.ap_conv_pair_nhwc(PR, _p(self.x), _p(self.ws), _p(self.s3), _p(self.h3), _p(self.res), _p(self.s1), _p(self.h1),
                                     _p(self.go.out), _p(self.gt.out), 245, self.P, self.N1, st)
        assert rc == 0, ("conv_pair", self.P, self.P2, self.N1, rc)

    def reference(self):
        """(out, t1n) float16: fp64 + one rounding, t1n from the ROUNDED out (the value the second GEMM reads)"""
        k = self.x.cpu().double()
        if self.P2:
            k = torch.cat([k, self.x2.cpu().double().view(5, 14, 14, -1)[:, ::2, ::2].reshape(245, -1)], 1)
        v = (k @ self.w3.double().t()) * self.s3.cpu().double() + self.h3.cpu().double()
        if not self.P2:
            v = v + self.res.cpu().double()
        out = v.clamp_min(0).to(torch.float16)
        if not self.N1:
            return out, None
        with torch.no_grad():
            a = out.double() @ self.w1.double().t()              # (inf * -1 = -inf; no 0 * inf: w1 has no zero where out is inf)
        t1 = (a * self.s1.cpu().double() + self.h1.cpu().double()).clamp_min(0).to(torch.float16)
        return out, t1


@gpu
@pytest.mark.parametrize("P,P2,N1", [(128, 0, 128), (128, 0, 256), (256, 0, 256), (128, 256, 128), (256, 512, 0)])
def test_conv_pair_sentinel(dev, P, P2, N1):
    """conv_pair_kernel, identity and stage-first forms: silent at the top in both outputs at once; the overflow born in `out` only
    (t1n finite) and in `t1n` only (out finite), one per store slot; identity form: the residual add"""
    C3 = 4 * P
    with Hook(dev) as hook:
        what = "conv_pair (%d, %d, %d)" % (P, P2, N1)
        op = Pair(dev, P, P2, N1, "out")
        # silent: out = 65504 everywhere; t1n = relu(-sum) = 0
        op.x[:, 0] = 1.0
        op.s3[:] = TOP
        hook.word()
        op.launch()
        w = hook.word()
        ro, rt = op.reference()
        assert_case(what + " top out", w, op.go.values((245, C3), what).cpu().to(torch.float16), ro)
        if N1:
            assert_case(what + " top t1n", w, op.gt.values((245, N1), what).cpu().to(torch.float16), rt)
        op.s3[:] = -16.0; op.h3[:] = OVF                     # 65504 stored; a masked pixel of the ragged tile (accumulator 0): 65520
        hook.word()
        op.launch()
        assert not hook.word() and bool((op.go.out == F16_MAX).all()) and bool(torch.isfinite(op.gt.out[:245 * N1]).all()), what + " rowbait out"
        op.x.zero_(); op.s3[:] = 1.0; op.h3[:] = 0.0

        def full_out(m, c):
            return op.reference()[0]
        n_out = sweep(hook, op, sample("conv_pair_%d" % C3), what + " out", op.s3, full=full_out, other=(op.gt,) if N1 else ())
        if not P2:
            few = probes(245, C3, 64, 128)
            for sval, word, nbad in ((16.0, True, 1), (RES_LO, False, 0)):
                def setup(m, c):
                    op.res[m, c] = F16_MAX
                    op.s3[c] = sval

                    def undo():
                        op.res[m, c] = 0.0
                        op.s3[c] = 1.0
                    return undo
                one_by_one(hook, op, few, "%s res + %r" % (what, sval), setup, word, nbad, other=(op.gt,))
        n_t1 = 0
        if N1:
            op = Pair(dev, P, P2, N1, "t1n")
            op.x[:, 0] = 1.0
            op.s1[:N1] = TOP
            hook.word()
            op.launch()
            w = hook.word()
            ro, rt = op.reference()
            assert_case(what + " top(t1n) out", w, op.go.values((245, C3), what).cpu().to(torch.float16), ro)
            assert_case(what + " top(t1n) t1n", w, op.gt.values((245, N1), what).cpu().to(torch.float16), rt)
            assert bool((op.gt.out == F16_MAX).all())
            op.s1[:N1] = -16.0; op.h1[:N1] = OVF
            hook.word()
            op.launch()
            assert not hook.word() and bool((op.gt.out == F16_MAX).all()) and bool(torch.isfinite(op.go.out).all()), what + " rowbait t1n"
            op.x.zero_(); op.s1[:] = 1.0; op.h1[:] = 0.0
            n_t1 = sweep(hook, op, sample("conv_pair_t1n_%d" % N1), what + " t1n", op.s1, full=lambda m, c: op.reference()[1], other=(op.go,))
        print("%-34s %d single overflows in out, %d in t1n" % (what, n_out, n_t1))


# ---- the forms a trunk pass selects (ABI 13): pooling epilogue, fragment-tiled output, second K segment, pair layouts
class Marked(Guarded):
    """Guarded whose payload starts as a finite marker instead of NaN, for an output that is written in part (the pixels past M of
    a fragment-tiled tensor, the odd pixels under out_even): the non-finite counts of sweep() then see stored elements only, and
    untouched() says whether the elements that must not be written still hold the marker"""
    MARK = 0.5

    def __init__(self, dev, prec, n):
        super().__init__(dev, prec, n)
        self.out.fill_(self.MARK)

    def values(self, shape, what):
        """the guards are intact and nothing is NaN; the payload flat where `shape` counts the stored elements only"""
        v = super().values((self.n,), what)
        n = 1
        for d in shape:
            n *= d
        return v.view(*shape) if n == self.n else v

    def untouched(self, keep):
        """keep: bool mask over the payload, True where the kernel must not store"""
        return bool((self.out[keep] == self.MARK).all())


class PoolOp(Op):
    """ap_conv2d_pool_nhwc: N 7 x 7 images, accumulator = x[m][0]; the `stored` elements are the 49 N x Cout values the pooling
    epilogue rounds to fp16 and sums, the visible output their mean [N][Cout] fp32 (inf as soon as one of them is)"""
    impulse = 1.0

    def __init__(self, dev, N, Cin, Cout):
        self.dev, self.N, self.Cin, self.C = dev, N, Cin, Cout
        self.M = N                                           # rows of the visible output (sweep() sizes its last check with it)
        self.x = torch.zeros(N * 49, Cin, dtype=torch.float16, device=dev)
        self.x_flat = self.x.view(-1)
        w = torch.zeros(Cout, 1, 1, Cin)
        w[:, 0, 0, 0] = 1.0
        self.w = _w_dev(w, PREC, dev)
        self.scale = _pad_rows(torch.ones(Cout), _cpad(Cout), 1.0).to(dev)         # the channel padding computes 1e6, as in Conv2d
        self.shift = _pad_rows(torch.zeros(Cout), _cpad(Cout), 1.0e6).to(dev)
        self.res = torch.zeros(N * 49, Cout, dtype=torch.float16, device=dev)
        self.g = Guarded(dev, "fp32", N * Cout)

    def in_index(self, m):
        return m * self.Cin

    def out_index(self, m, c):
        return (m // 49) * self.C + c

    def launch(self):
        Nn, L = _lib()
        rc = L.ap_conv2d_pool_nhwc(Nn.PRECISIONS[PREC], _p(self.x), _p(self.w), _p(self.scale), _p(self.shift), _p(self.res), _p(self.g.out),
                                   self.N, self.Cin, self.C, Nn.stream_ptr(self.dev))
        assert rc == 0, ("ap_conv2d_pool_nhwc", self.N, self.Cin, self.C, rc)

    def reference(self):
        """(the 49 N x Cout values the stand-alone path would store: fp64 + one rounding to fp16; their mean, fp32)"""
        C = self.C
        v = self.x.cpu().double()[:, :1] * self.scale.cpu().double()[:C] + self.shift.cpu().double()[:C] + self.res.cpu().double()
        st = v.clamp_min(0).to(torch.float16)
        return st, (st.double().view(self.N, 49, C).sum(1) / 49.0).float()


def pool_strata(N, Cout):
    """One position per (image, sub-tile of the 128-row halves of a 5-image super-tile, channel tile): pixels 0, 29, 30, 48 of every
    image (image 2 of a super-tile changes sub-tile between 29 and 30), channels at both ends of every 64-channel half"""
    cs = sorted({c for c in (0, 63, 64, 127, 128, 191, 192, 255, Cout - 8, Cout - 1) if c < Cout})
    return [(n * 49 + px, c) for n in range(N) for px in (0, 29, 30, 48) for c in cs]


def test_pool_strata_cover_every_stratum():
    """Host only: the positions of test_conv_pool_sentinel hit every (image of a 5-image super-tile, 128-row sub-tile, 128-channel
    tile and 64-channel half of it), image 2 on both sides of its split, and the ragged last channel group"""
    pos = pool_strata(6, 136)
    rows = {(m // 49 % 5, (m % 245) // 128, c // 64) for m, c in pos}
    assert rows == {(i, s, h) for i, s in ((0, 0), (1, 0), (2, 0), (2, 1), (3, 1), (4, 1)) for h in (0, 1, 2)}
    assert {m // 245 for m, _ in pos} == {0, 1} and (5 * 49 + 48, 135) in pos and all(c < 136 for _, c in pos)
    assert [m for m, _ in pos] == sorted(m for m, _ in pos)                    # sweep() moves the impulse pixel by pixel


@gpu
@pytest.mark.parametrize("N", [1, 4, 6])
def test_conv_pool_sentinel(dev, N):
    """conv_lean_kernel<POOL>: silent at the top of the range under the row bait (the rows past N 49, the 11 unused rows of a
    super-tile: accumulator 0) and the channel-padding bait; one overflow per (image, sub-tile, channel tile) sets the word"""
    Cin, Cout = 64, 136
    with Hook(dev) as hook:
        op = PoolOp(dev, N, Cin, Cout)
        what = "conv_pool N=%d" % N
        for kind in SILENT:
            op.x.zero_(); op.res.zero_()
            op.scale[:Cout] = 1.0; op.shift[:Cout] = 0.0
            if kind == "top":
                op.x[:, 0] = 1.0; op.scale[:Cout] = TOP
            elif kind == "rowbait":
                op.x[:, 0] = 1.0; op.scale[:Cout] = -16.0; op.shift[:Cout] = OVF
            else:
                for m in (0, N * 49 - 1):
                    op.x[m, 0] = 1.0; op.res[m] = -16.0
                op.scale[:Cout] = OVF
            hook.word()
            op.launch()
            w = hook.word()
            st, pooled = op.reference()
            nbad = int((~torch.isfinite(st.float())).sum())
            assert nbad == 0 and float(st.max()) == F16_MAX
            got = op.g.values((N, Cout), what).cpu()
            assert torch.equal(got, pooled), (what, kind, "pooled features differ from the mean of the reference's stored values")
            assert bool(w) == bool(nbad), (what, kind, "word %d, but %d stored elements are non-finite" % (int(w), nbad))
        op.x.zero_(); op.res.zero_()
        op.scale[:Cout] = 1.0; op.shift[:Cout] = 0.0
        n = sweep(hook, op, pool_strata(N, Cout), what, op.scale)
    print("%-34s %d single overflows, 3 silent cases" % (what, n))


class Conv2dTiled(Conv2d):
    """ap_conv2d_tiled_nhwc on a ragged M: the pixels M .. ceil16(M) - 1 of the last micro-tile must keep the marker"""
    out_layout = "tiled"

    def __init__(self, dev, shp):
        super().__init__(dev, shp)
        self.g = Marked(dev, PREC, (self.M + 15) // 16 * 16 * self.C)
        m, c = torch.arange(self.M, device=dev)[:, None], torch.arange(self.C, device=dev)[None, :]
        self.idx = self.out_index(m, c)

    def launch(self):
        Nn, L = _lib()
        name, N, H, W, Cin, Cout, k, s, p = self.shp
        rc = L.ap_conv2d_tiled_nhwc(Nn.PRECISIONS[PREC], _p(self.x), _p(self.w), _p(self.scale), _p(self.shift),
                                    _p(self.res) if self.use_res else None, _p(self.g.out), N, H, W, Cin, Cout, k, s, p, self.relu,
                                    Nn.stream_ptr(self.dev))
        assert rc == 0, (self.shp, "ap_conv2d_tiled_nhwc status %d" % rc)

    def stored(self, what):
        self.g.values((self.g.n,), what)
        keep = torch.ones(self.g.n, dtype=torch.bool, device=self.dev)
        keep[self.idx.reshape(-1)] = False
        assert self.g.untouched(keep), (what, "a pixel past M of the last micro-tile was written")
        return self.g.out[self.idx].cpu()


class Conv2dFold(Op):
    """ap_conv2d_fold_nhwc: accumulator = t[m][0] + x2[sampled pixel of m][0] (w = 1 on the first channel of either segment)"""
    impulse = 1.0

    def __init__(self, dev, N, Ho, Cin, Cin2, Cout, s2):
        self.dev, self.N, self.Ho, self.Cin, self.Cin2, self.s2 = dev, N, Ho, Cin, Cin2, s2
        self.H2 = 2 * Ho - 1 if s2 == 2 else Ho
        self.M, self.C = N * Ho * Ho, Cout
        self.x = torch.zeros(self.M, Cin, dtype=torch.float16, device=dev)           # t
        self.x_flat = self.x.view(-1)
        self.x2 = torch.zeros(N, self.H2, self.H2, Cin2, dtype=torch.float16, device=dev)
        w = torch.zeros(Cout, 1, 1, Cin + Cin2)
        w[:, 0, 0, 0] = w[:, 0, 0, Cin] = 1.0
        self.w = _w_dev(w, PREC, dev)
        self.scale = _pad_rows(torch.ones(Cout), _cpad(Cout), 1.0).to(dev)
        self.shift = _pad_rows(torch.zeros(Cout), _cpad(Cout), 1.0e6).to(dev)
        self.g = Guarded(dev, PREC, self.M * Cout)

    def in_index(self, m):
        return m * self.Cin

    def fill_alt(self):
        """x2: image k all +4, image k + 1 all -4 (the "alt" family, sampled and unsampled pixels alike); t = 1 - x2 at the sampled
        pixel, so the accumulator of every stored row is exactly 1 -- and that of a masked row which aliases a row of x2 is not"""
        sign = torch.tensor([4.0 if n % 2 == 0 else -4.0 for n in range(self.N)], device=self.dev)
        self.x2[..., 0] = sign.view(-1, 1, 1).to(torch.float16)
        self.x.view(self.N, self.Ho * self.Ho, self.Cin)[:, :, 0] = (1.0 - sign).view(-1, 1).to(torch.float16)

    def launch(self):
        Nn, L = _lib()
        rc = L.ap_conv2d_fold_nhwc(Nn.PRECISIONS[PREC], _p(self.x), _p(self.x2), _p(self.w), _p(self.scale), _p(self.shift), None, _p(self.g.out),
                                   self.N, self.Ho, self.H2, self.Cin, self.Cin2, self.C, self.s2, 1, Nn.stream_ptr(self.dev))
        assert rc == 0, ("ap_conv2d_fold_nhwc", rc)


FORM_CFGS = (-1, 11, 100)
TILED_SENTINEL_SHAPES = ("p1_m129", "r3_5x9")                # M = 129 and 90: ragged for the 16-pixel micro-tile and for every tile
FOLD_SENTINEL_SHAPES = ((3, 7, 64, 64, 136, 2), (3, 5, 128, 64, 72, 1))   # (N, Ho, Cin, Cin2, Cout, stride2): M = 147 and 75


@gpu
@pytest.mark.parametrize("cfg", FORM_CFGS)
@pytest.mark.parametrize("form", ["tiled", "fold"])
def test_conv2d_forms_sentinel(dev, form, cfg):
    """The fragment-tiled output and the second K segment of the generic kernels on two ragged shapes each: silent at the top of the
    range under the baits, one overflow at a time over the probes of the configuration's tile"""
    Nn, L = _lib()
    rows, width = PIPE_TILES[cfg]
    Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
    n = 0
    try:
        with Hook(dev) as hook:
            if form == "tiled":
                for shp in [s for s in SHAPES if s[0] in TILED_SENTINEL_SHAPES]:
                    op = Conv2dTiled(dev, shp)
                    what = "tiled cfg=%d %s" % (cfg, shp[0])
                    for kind in SILENT:
                        run_case(hook, op, conv_case(shp, kind), "%s %s" % (what, kind), key=(shp[0], kind))
                    n += sweep(hook, op, probes(op.M, op.C, rows, width), what, op.scale)
                    op.stored(what)
            else:
                for N, Ho, Cin, Cin2, Cout, s2 in FOLD_SENTINEL_SHAPES:
                    op = Conv2dFold(dev, N, Ho, Cin, Cin2, Cout, s2)
                    what = "fold cfg=%d M=%d" % (cfg, op.M)
                    op.fill_alt()
                    for sc, sh in ((TOP, 0.0), (-16.0, OVF)):                        # top; rowbait
                        op.scale[:Cout] = sc; op.shift[:Cout] = sh
                        hook.word()
                        op.launch()
                        w = hook.word()
                        st = op.g.values((op.M, Cout), what)
                        assert bool((st == F16_MAX).all()), (what, sc, "a stored value is not 65504")
                        assert not w, (what, sc, "word 1, but 0 stored elements are non-finite")
                    op.x.zero_(); op.x2.zero_()
                    op.scale[:Cout] = 1.0; op.shift[:Cout] = 0.0
                    n += sweep(hook, op, probes(op.M, op.C, rows, width), what, op.scale)
    finally:
        L.ap_set_conv_config(-1)
    print("%-34s %d single overflows" % ("generic kernels, %s form, cfg=%d" % (form, cfg), n))


class PairL(Pair):
    """Pair through ap_conv_pair_layout_nhwc with the layouts of one plan combination (t2_tiled, res_tiled, out_tiled, out_even).
    Tiled inputs are laid out on the host; a partly written `out` starts as Marked"""

    def __init__(self, dev, P, P2, N1, which, lay):
        super().__init__(dev, P, P2, N1, which)
        self.lay, C3 = lay, 4 * P
        if lay[0]:
            self.x = torch.zeros(256 * P, dtype=torch.float16, device=dev)
            self.x_flat = self.x
        if lay[1]:
            self.res = torch.zeros(256 * C3, dtype=torch.float16, device=dev)
        if lay[2] or lay[3]:
            self.go = Marked(dev, PREC, (256 if lay[2] else 245) * C3)
        self.g = self.go if which == "out" else self.gt
        if which == "out" and lay[2]:
            self.out_layout = "tiled"
        m = torch.arange(245, device=dev)
        self.in0 = (((m >> 4) * (P >> 3)) * 128 + (m & 15) * 8) if lay[0] else m * P                  # channel 0 of every pixel of t2
        c = torch.arange(C3, device=dev)[None, :]
        mm = m[:, None]
        self.oidx = (((mm >> 4) * (C3 >> 3) + (c >> 3)) * 128 + (mm & 15) * 8 + (c & 7)) if lay[2] else mm * C3 + c
        self.even = ((m % 49) // 7 % 2 == 0) & ((m % 7) % 2 == 0)                                       # pixels out_even stores
        k = torch.arange(P, device=dev)[None, :]
        self.xidx = (((mm >> 4) * (P >> 3) + (k >> 3)) * 128 + (mm & 15) * 8 + (k & 7)) if lay[0] else mm * P + k
        self.ridx = (((mm >> 4) * (C3 >> 3) + (c >> 3)) * 128 + (mm & 15) * 8 + (c & 7)) if lay[1] else mm * C3 + c

    def reference(self):
        """Pair.reference on the NHWC rows the (host-tiled) inputs stand for"""
        x, res = self.x, self.res
        self.x, self.res = x.view(-1)[self.xidx], res.view(-1)[self.ridx]
        try:
            return Pair.reference(self)
        finally:
            self.x, self.res = x, res

    def set_res(self, m, c, v):
        self.res.view(-1)[int(self.ridx[m, c])] = v

    def stored(self, what):
        """[245][C] float16 on the host (not for `out` under out_even, whose odd pixels are not stored)"""
        if self.which == "out":
            assert not self.lay[3]
            return self.out_rows(what).cpu()
        return self.gt.values((245, self.N1), what).cpu().to(torch.float16)

    def in_index(self, m):
        return int(self.in0[m])

    def set_all(self, v):
        self.x_flat[self.in0] = v

    def launch(self):
        Nn, L = _lib()
        n1 = self.N1 > 0
        rc = L.ap_conv_pair_layout_nhwc(Nn.PRECISIONS[PREC], _p(self.x), _p(self.x2 if self.P2 else self.res), _p(self.ws), _p(self.s3), _p(self.h3),
                                        _p(self.s1) if n1 else None, _p(self.h1) if n1 else None, _p(self.go.out), _p(self.gt.out) if n1 else None,
                                        5, 7, self.P, self.P2, 2, self.N1, self.lay[0], self.lay[1], self.lay[2], self.lay[3], Nn.stream_ptr(self.dev))
        assert rc == 0, ("ap_conv_pair_layout_nhwc", self.P, self.P2, self.N1, self.lay, rc)

    def out_rows(self, what):
        """the stored pixels of `out` as rows [.][C3]; the elements that must not be written still hold the marker"""
        self.go.values((self.go.n,), what)
        rows = self.go.out[self.oidx]
        if isinstance(self.go, Marked):
            keep = torch.ones(self.go.n, dtype=torch.bool, device=self.dev)
            keep[(self.oidx[self.even] if self.lay[3] else self.oidx).reshape(-1)] = False
            assert self.go.untouched(keep), (what, "an element of out that must not be stored was written")
        return rows[self.even] if self.lay[3] else rows


PAIR_PLAN = [(128, 256, 128, (1, 0, 1, 0)), (256, 512, 0, (1, 0, 1, 0)),
             (128, 0, 128, (1, 1, 1, 0)), (128, 0, 256, (1, 1, 1, 0)), (256, 0, 256, (1, 1, 1, 0)),
             (128, 0, 128, (1, 1, 0, 1)), (128, 0, 256, (1, 1, 0, 1)), (256, 0, 256, (1, 1, 0, 1))]


@gpu
@pytest.mark.parametrize("P,P2,N1,lay", PAIR_PLAN, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv_pair_layout_sentinel(dev, P, P2, N1, lay):
    """test_conv_pair_sentinel's `out` / `t1n` isolation under the three layout combinations plan_pass produces (ds form:
    t2_tiled + out_tiled; identity form: t2_tiled + res_tiled + out_tiled, and + out_even).
    The rule for out_even is the one this file applies to hidden intermediates and to y_even of test_bottleneck64_sentinel[tail-1]: a
    value that is not stored but is the operand of the kernel's next stage counts as stored.  An odd pixel of `out` is not written,
    yet its packed value feeds conv1 of the next block: nothing stored is non-finite there (t1n = relu(-inf) = 0), and the word
    must still be set."""
    C3 = 4 * P
    with Hook(dev) as hook:
        what = "conv_pair layout (%d, %d, %d) %s" % (P, P2, N1, lay)
        op = PairL(dev, P, P2, N1, "out", lay)
        op.set_all(1.0)
        for s, h in ((TOP, 0.0), (-16.0, OVF)):              # top; rowbait (a masked pixel of the ragged tile with accumulator 0: 65520)
            op.s3[:] = s; op.h3[:] = h
            hook.word()
            op.launch()
            assert not hook.word(), (what, s, "word 1, but 0 stored elements are non-finite")
            assert bool((op.out_rows(what) == F16_MAX).all()) and bool(torch.isfinite(op.gt.out[:245 * N1]).all()), (what, s)
        op.x.zero_(); op.s3[:] = 1.0; op.h3[:] = 0.0
        pos = sample("conv_pair_%d" % C3)
        if not lay[3]:
            n_out = sweep(hook, op, pos, what + " out", op.s3, full=lambda m, c: op.reference()[0], other=(op.gt,) if N1 else ())
            op.out_rows(what)
        else:
            pos = pos[::8]
            assert any(bool(op.even[m]) for m, _ in pos) and any(not bool(op.even[m]) for m, _ in pos)
            for m, c in pos:
                op.x_flat[op.in_index(m)] = 1.0; op.s3[c] = OVF
                hook.word()
                op.launch()
                assert hook.word(), (what, "out overflow at pixel %d (even pixels stored) not reported" % m)
                bad = ~torch.isfinite(op.go.out)
                even = bool(op.even[m])
                assert int(bad.sum()) == int(even) and (not even or bool(bad[m * C3 + c])), (what, m, c, int(bad.sum()))
                assert bool(torch.isfinite(op.gt.out).all()), (what, m, c, "t1n holds non-finite values")
                op.x_flat[op.in_index(m)] = 0.0; op.s3[c] = 1.0
            op.launch()
            op.out_rows(what)
            n_out = len(pos)
        if not P2:
            # the residual add at the boundary, as in test_conv_pair_sentinel: with res_tiled the only sentinel check of the tiled read
            few = [q for q in probes(245, C3, 64, 128) if not lay[3] or bool(op.even[q[0]])]
            assert len(few) >= 8
            for sval, word, nbad in ((16.0, True, 1), (RES_LO, False, 0)):
                def setup(m, c):
                    op.set_res(m, c, F16_MAX)
                    op.s3[c] = sval

                    def undo():
                        op.set_res(m, c, 0.0)
                        op.s3[c] = 1.0
                    return undo
                one_by_one(hook, op, few, "%s res + %r" % (what, sval), setup, word, nbad, other=(op.gt,))
            op.launch()
            op.out_rows(what)
        n_t1 = 0
        if N1:
            op = PairL(dev, P, P2, N1, "t1n", lay)
            op.set_all(1.0)
            for s, h in ((TOP, 0.0), (-16.0, OVF)):
                op.s1[:N1] = s; op.h1[:N1] = h
                hook.word()
                op.launch()
                assert not hook.word(), (what, s, "t1n: word 1, but 0 stored elements are non-finite")
                assert bool((op.gt.values((245, N1), what) == F16_MAX).all()) and bool(torch.isfinite(op.go.out).all()), (what, s)
            op.x.zero_(); op.s1[:] = 1.0; op.h1[:] = 0.0
            n_t1 = sweep(hook, op, sample("conv_pair_t1n_%d" % N1), what + " t1n", op.s1, full=lambda m, c: op.reference()[1], other=(op.go,))
        print("%-34s %d single overflows in out, %d in t1n" % (what, n_out, n_t1))


# ---- bottleneck2.hip / block_img.hip: three convolutions, two hidden intermediates
class Fused3(Op):
    """A fused bottleneck on impulse operands.  The input listens on channels 0 and 1 (w1 = 1 there), so the impulse can avoid
    the target channel of an identity block (the identity adds x to y).
    mode "y":  t1 = t2 = 1 at the impulse pixel (all channels), w3 = 1 on input channel 0: acc3 = 1; s3 carries the boundary
    mode "t1": s1 carries the boundary; w2 = -1 on EVERY input channel and tap (t1 >= 0, so t2 = relu(-sum) = 0); w3 = 0
    mode "t2": t1 = 1; w2 = 1 (centre tap, input 0): acc2 = 1; s2 carries the boundary; w3 = -1 on every input channel
    mode "t1n" (tail): w3 = 0, y = x; w1n = 1 on input channel 0 and 1; s1n carries the boundary
    mode "y_tail": as "y" with w1n = -1 everywhere: t1n = relu(-inf) = 0"""

    def __init__(self, dev, kind, mode, y_even=0):
        Nn, L = _lib()
        self.dev, self.kind, self.mode, self.y_even = dev, kind, mode, y_even
        img = kind == "block_img"
        self.pl = pl = 256 if img else 64
        self.cin = (1024 if img else 64 if kind == "downsample" else 256)
        self.cin2 = 64 if kind == "downsample" else 0
        self.N, self.H, self.W = (2, 14, 14) if img else (1, 14, 28)
        self.M = self.N * self.H * self.W
        Cy = 4 * pl
        self.C = {"t1n": 128}.get(mode, Cy)
        w1, w2, w3 = torch.zeros(pl, 1, 1, self.cin), torch.zeros(pl, 3, 3, pl), torch.zeros(Cy, 1, 1, pl + self.cin2)
        w1[:, 0, 0, 0:2] = 1.0
        if mode in ("y", "y_tail"):
            w2[:, 1, 1, 0] = 1.0; w3[:, 0, 0, 0] = 1.0
        elif mode == "t1":
            w2[:] = -1.0
        elif mode == "t2":
            w2[:, 1, 1, 0] = 1.0; w3[:, 0, 0, :pl] = -1.0
        elif mode == "t1n":
            w2[:, 1, 1, 0] = 1.0
        self.wv = [w1, w2, w3]
        self.wd = [_w_dev(w, PREC, dev) for w in self.wv]
        self.bn = [[torch.ones(_cpad(c), device=dev), torch.zeros(_cpad(c), device=dev)] for c in (pl, pl, Cy)]
        self.x = torch.zeros(self.M, self.cin, dtype=torch.float16, device=dev)
        self.x_flat = self.x.view(-1)
        self.gy = Guarded(dev, PREC, self.M * Cy)
        self.gt = None
        if kind == "tail":
            w1n = torch.zeros(128, 1, 1, 256)
            if mode == "t1n":
                w1n[:, 0, 0, 0:2] = 1.0
            else:
                w1n[:] = -1.0
            self.w1n, self.w1nd = w1n, _w_dev(w1n, PREC, dev)
            self.bn1n = [torch.ones(128, device=dev), torch.zeros(128, device=dev)]
            self.gt = Guarded(dev, PREC, self.M * 128)
        if img:
            self.ws = torch.empty(L.ap_block_img_stream_bytes(), dtype=torch.uint8, device=dev)
            Nn.check(L.ap_block_img_pack(Nn.PRECISIONS[PREC], _p(self.wd[0]), _p(self.wd[1]), _p(self.wd[2]), _p(self.ws), Nn.stream_ptr(dev)), "ap_block_img_pack")
        self.g = self.gt if mode == "t1n" else self.gy
        self.impulse_ch = 0

    def in_index(self, m):
        return m * self.cin + self.impulse_ch

    @property
    def impulse(self):
        return 1.0

    def launch(self):
        Nn, L = _lib()
        st, PR = Nn.stream_ptr(self.dev), Nn.PRECISIONS[PREC]
        b = self.bn
        if self.kind == "block_img":
            rc = L.ap_block_img_nhwc(PR, _p(self.x), _p(self.ws), _p(b[0][0]), _p(b[0][1]), _p(b[1][0]), _p(b[1][1]), _p(b[2][0]), _p(b[2][1]),
                                     _p(self.gy.out), self.N, st)
        else:
            args = []
            for i in range(3):
                args += [_p(self.wd[i]), _p(b[i][0]), _p(b[i][1])]
            if self.kind == "tail":
                rc = L.ap_bottleneck64_tail_nhwc(PR, _p(self.x), *args, _p(self.gy.out), _p(self.w1nd), _p(self.bn1n[0]), _p(self.bn1n[1]),
                                                 _p(self.gt.out), self.y_even, self.N, self.H, self.W, st)
            else:
                rc = L.ap_bottleneck64_nhwc(PR, _p(self.x), *args, _p(self.gy.out), self.N, self.H, self.W, self.cin, 1 if self.kind == "downsample" else 0, st)
        assert rc == 0, (self.kind, rc)

    def reference(self):
        """fp64 with one rounding to fp16 at each of the kernel's rounding points: (t1, t2, y, t1n) float16"""
        def bn(acc, i, res=None):
            C = acc.shape[-1]
            v = acc * self.bn[i][0].cpu().double()[:C] + self.bn[i][1].cpu().double()[:C]
            if res is not None:
                v = v + res
            return v.clamp_min(0).to(torch.float16)

        def conv(xv, w, pad):
            # inf * 0 would be NaN in a plain convolution; the kernel never multiplies an inf by a zero WEIGHT here (the -1 planes
            # are dense), but zero ACTIVATIONS meet nonzero weights: mask the non-finite inputs and add them back with their sign
            fin = torch.where(torch.isfinite(xv), xv, torch.zeros_like(xv))
            inf = torch.where(torch.isfinite(xv), torch.zeros_like(xv), torch.sign(xv))
            c = conv_sums(fin, w, 1, pad)[0]
            ci = conv_sums(inf, w, 1, pad)[0]
            return torch.where(ci != 0, ci * float("inf"), c)
        xv = self.x.cpu().double().view(self.N, self.H, self.W, self.cin)
        t1 = bn(conv(xv, self.wv[0], 0), 0)
        t2 = bn(conv(t1.double(), self.wv[1], 1), 1)
        k3 = torch.cat([t2.double(), xv], 3) if self.cin2 else t2.double()
        y = bn(conv(k3, self.wv[2], 0), 2, None if self.cin2 else xv)
        t1n = None
        if self.kind == "tail":
            a = conv(y.double(), self.w1n, 0)
            t1n = (a * self.bn1n[0].cpu().double() + self.bn1n[1].cpu().double()).clamp_min(0).to(torch.float16)
        return t1, t2, y, t1n

    def y_stored(self, what):
        """y [M][Cy] float16 on the host (y_even: the even pixels, the others NaN = untouched)"""
        if self.y_even:
            return self.gy.out.view(self.N, self.H, self.W, -1).cpu()
        return self.gy.values((self.N, self.H, self.W, 4 * self.pl), what).cpu().to(torch.float16)


def fused_check(hook, op, what, want_word, hidden=None):
    """launch; every output equals the fp64 chain; the word equals "a stored or LDS-resident fp16 value is non-finite" (hidden:
    the intermediate that must hold the overflow while every output is finite)"""
    hook.word()
    op.launch()
    w = hook.word()
    t1, t2, y, t1n = op.reference()
    got = op.y_stored(what)
    if op.y_even:
        ge, ye = got[:, ::2, ::2].float(), y[:, ::2, ::2].float()
        assert torch.equal(torch.isfinite(ge), torch.isfinite(ye)) and torch.equal(ge[torch.isfinite(ge)], ye[torch.isfinite(ye)]), (what, "y (even pixels)")
        assert bool(torch.isnan(got[:, 1::2].float()).all() and torch.isnan(got[:, :, 1::2].float()).all()), (what, "an odd pixel of y was written")
        y = ye
    else:
        assert_case(what + " y", bool((~torch.isfinite(y.float())).any()), got.reshape(op.M, -1), y.reshape(op.M, -1))
    outs_bad = bool((~torch.isfinite(y.float())).any())
    if t1n is not None:
        g = op.gt.values((op.M, 128), what).cpu().to(torch.float16)
        assert_case(what + " t1n", bool((~torch.isfinite(t1n.float())).any()), g, t1n.reshape(op.M, 128))
        outs_bad |= bool((~torch.isfinite(t1n.float())).any())
    any_bad = outs_bad or bool((~torch.isfinite(t1.float())).any()) or bool((~torch.isfinite(t2.float())).any())
    if hidden is not None:
        assert not outs_bad and bool((~torch.isfinite({"t1": t1, "t2": t2}[hidden].float())).any()), (what, "the case does not isolate " + hidden)
    assert any_bad == want_word, (what, "the case is not what it claims")
    assert w == want_word, (what, "word %d" % w)


def fused_fast(hook, op, what, want_word):
    """launch; every stored output finite (checked on the device); the word as expected"""
    hook.word()
    op.launch()
    w = hook.word()
    y = op.gy.out.view(op.N, op.H, op.W, -1)
    assert bool(torch.isfinite(y[:, ::2, ::2] if op.y_even else y).all()), (what, "y is not finite")
    assert op.gt is None or bool(torch.isfinite(op.gt.out).all()), (what, "t1n is not finite")
    assert w == want_word, (what, "word %d" % w)


def fused_hidden(hook, dev, kind, what, y_even=0):
    """hidden t1 and t2: every channel of the intermediate at a few pixels (tile corners, centre, the second tile); the output finite"""
    n = 0
    for mode in ("t1", "t2"):
        op = Fused3(dev, kind, mode, y_even)
        sc = op.bn[0 if mode == "t1" else 1][0]
        px = sorted({0, op.W - 1, 7 * op.W + 6, op.M - op.W, op.M - 1, 14 if kind != "block_img" else 196})
        for i, m in enumerate(px):
            op.x_flat[op.in_index(m)] = 1.0
            for c in (range(op.pl) if i == 0 else range(i, op.pl, 9)):
                for val, word in ((OVF, True), (TOP, False)):
                    if not word and c % 8 != i % 8:
                        continue
                    sc[c] = val
                    w2 = "%s hidden %s pixel %d channel %d scale %r" % (what, mode, m, c, val)
                    if c in (i, op.pl - 1):                 # the complete comparison with the fp64 chain on a few, the rest on the device
                        fused_check(hook, op, w2, word, mode if word else None)
                    else:
                        fused_fast(hook, op, w2, word)
                    n += 1
                sc[c] = 1.0
            op.x_flat[op.in_index(m)] = 0.0
    return n


@gpu
@pytest.mark.parametrize("kind,y_even", [("identity", 0), ("downsample", 0), ("tail", 0), ("tail", 1)])
def test_bottleneck64_sentinel(dev, kind, y_even):
    """ap_bottleneck64_nhwc (identity, downsample) and ap_bottleneck64_tail_nhwc on a 14 x 28 image = two tiles: silent at the
    top; one overflow per store slot of y (tail: with t1n finite) and of t1n (y finite); the hidden t1 and t2"""
    with Hook(dev) as hook:
        what = "bottleneck64 %s y_even=%d" % (kind, y_even)
        op = Fused3(dev, kind, "y_tail" if kind == "tail" else "y", y_even)
        # silent: y = 65504 everywhere (identity forms: 65000 + 1 on the impulse channel, which the identity adds to)
        op.x[:, 0] = 1.0
        op.bn[2][0][:] = TOP
        if kind != "downsample":
            op.bn[2][0][0] = 65000.0
        fused_check(hook, op, what + " top", False)
        op.bn[2][0][:] = -16.0; op.bn[2][1][:] = OVF        # 65504 (+ x) stored; a halo lane of the 16 x 16 tile (accumulator 0): 65520
        fused_check(hook, op, what + " rowbait", False)
        op.x.zero_(); op.bn[2][0][:] = 1.0; op.bn[2][1][:] = 0.0
        n_y = n_t = 0
        if not y_even:
            pos = sample("bottleneck64")
            # the impulse avoids the target channel: channel 1 for target 0
            for ch, part in ((0, [p for p in pos if p[1] != 0]), (1, [p for p in pos if p[1] == 0])):
                op.impulse_ch = ch
                n_y += sweep(hook, op, part, what + " y", op.bn[2][0], other=(op.gt,) if op.gt is not None else ())
            op.impulse_ch = 0
            m, c = pos[len(pos) // 2]
            op.x_flat[op.in_index(m)] = 1.0; op.bn[2][0][c] = OVF
            fused_check(hook, op, what + " y full", True)
        else:
            # y is stored at the even pixels only, but every pixel's packed y is the operand of conv1n: at an odd pixel it is a
            # hidden intermediate -- nothing stored is non-finite there, and the word must still be set
            for m, c in ((0, 5), (2 * 28 + 4, 255), (1, 5), (28 + 3, 77), (13 * 28 + 27, 128)):
                op.x_flat[op.in_index(m)] = 1.0; op.bn[2][0][c] = OVF
                hook.word()
                op.launch()
                assert hook.word(), (what, "y overflow at pixel %d (even pixels stored)" % m)
                even = (m // 28) % 2 == 0 and (m % 28) % 2 == 0
                ye = op.gy.out.view(1, 14, 28, 256)[:, ::2, ::2]
                assert int((~torch.isfinite(ye)).sum()) == int(even) and bool(torch.isfinite(op.gt.out).all()), (what, m, c)
                op.x_flat[op.in_index(m)] = 0.0; op.bn[2][0][c] = 1.0
                n_y += 1
        if kind == "tail":
            op = Fused3(dev, kind, "t1n", y_even)
            op.x[:, 0] = 1.0
            op.bn1n[0][:] = TOP
            fused_check(hook, op, what + " top t1n", False)
            assert bool((op.gt.out == F16_MAX).all())
            op.x.zero_(); op.bn1n[0][:] = 1.0
            n_t = sweep(hook, op, sample("bottleneck64_t1n"), what + " t1n", op.bn1n[0])
            m, c = sample("bottleneck64_t1n")[7]
            op.x_flat[op.in_index(m)] = 1.0; op.bn1n[0][c] = OVF
            fused_check(hook, op, what + " t1n full", True)
        n_h = fused_hidden(hook, dev, kind, what, y_even)
        print("%-34s %d single overflows in y, %d in t1n, %d hidden-intermediate cases" % (what, n_y, n_t, n_h))


@gpu
def test_block_img_sentinel(dev):
    """ap_block_img_nhwc on two images: silent at the top; one overflow per store slot of y; the hidden t1 and t2"""
    with Hook(dev) as hook:
        what = "block_img"
        op = Fused3(dev, "block_img", "y")
        op.x[:, 0] = 1.0
        op.bn[2][0][:] = TOP
        op.bn[2][0][0] = 65000.0
        fused_check(hook, op, what + " top", False)
        op.bn[2][0][:] = -16.0; op.bn[2][1][:] = OVF        # 65504 (+ x) stored; a zero slot of the 16-slot rows (accumulator 0): 65520
        fused_check(hook, op, what + " rowbait", False)
        op.x.zero_(); op.bn[2][0][:] = 1.0; op.bn[2][1][:] = 0.0
        pos = sample("block_img")
        n_y = 0
        for ch, part in ((0, [p for p in pos if p[1] != 0]), (1, [p for p in pos if p[1] == 0])):
            op.impulse_ch = ch
            n_y += sweep(hook, op, part, what + " y", op.bn[2][0])
        op.impulse_ch = 0
        m, c = pos[len(pos) // 2]
        op.x_flat[op.in_index(m)] = 1.0; op.bn[2][0][c] = OVF
        fused_check(hook, op, what + " y full", True)
        n_h = fused_hidden(hook, dev, "block_img", what)
        print("%-34s %d single overflows in y, %d hidden-intermediate cases" % (what, n_y, n_h))


# ---- stem.hip
class StemOp(Op):
    """ap_stem_nhwc forms 1 / 2 on two crops (one per view): a crop impulse at (4 py, 4 px) of plane 0 meets the centre tap of the conv
    pixel (2 py, 2 px), which only the pooling window centred on it covers: one pooled element per impulse"""
    impulse = 1.0

    def __init__(self, dev, form):
        from test_stem_pool_fp64 import Stem
        self.dev, self.form = dev, form
        self.M, self.C = 2 * 56 * 56, 64
        w = torch.zeros(64, 3, 7, 7)
        w[:, 0, 3, 3] = 1.0
        self.st = Stem(dev, PREC, w, torch.ones(64), torch.zeros(64))
        self.scale = self.st.scale
        self.x = torch.zeros(2, 3, 224, 224, device=dev)
        self.x_flat = self.x.view(-1)
        self.g = Guarded(dev, PREC, self.M * 64)

    def in_index(self, m):
        n, r = divmod(m, 56 * 56)
        py, px = divmod(r, 56)
        return (n * 3 * 224 + 4 * py) * 224 + 4 * px

    def launch(self):
        s = self.st
        rc = s.L.ap_stem_nhwc(s.P, self.form, _p(self.x[0:1]), _p(self.x[1:2]), 1, _p(s.wpk), _p(s.scale), _p(s.shift), _p(self.g.out), 2,
                              s.Nn.stream_ptr(self.dev))
        assert rc == 0, ("ap_stem_nhwc", self.form, rc)

    def reference(self):
        w = torch.zeros(64, 3, 7, 7, dtype=torch.float64)
        w[:, 0, 3, 3] = 1.0
        c = F.conv2d(self.x.cpu().to(torch.float16).double(), w, stride=2, padding=3)
        v = (c * self.scale.cpu().double().view(1, -1, 1, 1)).clamp_min(0).to(torch.float16)
        return F.max_pool2d(v.double(), 3, 2, 1).permute(0, 2, 3, 1).reshape(self.M, 64).to(torch.float16)


@gpu
@pytest.mark.parametrize("form", [1, 2])
def test_stem_sentinel(dev, form):
    """stem_pool_kernel (form 1) and stem_pool2_kernel (form 2): silent at the top; one overflow per store slot of a strip; the
    conversion of the crop itself (watched like a store: stem.hip): a crop value of 65520 on a plane with zero weights sets the word,
    TOP leaves it 0"""
    with Hook(dev) as hook:
        op = StemOp(dev, form)
        what = "stem form %d" % form
        op.x[:, 0, ::4, ::4] = 1.0
        op.scale[:] = TOP
        check_now(hook, op, what + " top")
        assert bool((op.g.out == F16_MAX).all())
        op.x.zero_(); op.scale[:] = 1.0
        n = sweep(hook, op, sample("stem_pool"), what, op.scale, full=lambda m, c: op.reference(), full_every=1201)
        for n_img, y, x in ((0, 0, 0), (1, 223, 223), (0, 100, 57), (1, 5, 222)):
            for val, word in ((TOP, False), (-TOP, False), (OVF, True), (-OVF, True)):
                op.x[n_img, 1, y, x] = val
                hook.word()
                op.launch()
                assert hook.word() == word, (what, "crop value %r at" % val, (n_img, y, x))
                op.x[n_img, 1, y, x] = 0.0
        print("%-34s %d single overflows" % (what, n))


@gpu
def test_stem_unpooled_then_maxpool(dev):
    """ap_stem_nhwc form 0 (stem_mfma_kernel) carries no sentinel of its own (airpose_hip.h): the inf it stores is reported by the
    max-pool that follows it, as in a trunk pass with the fused stem off"""
    from test_stem_pool_fp64 import Stem
    w = torch.zeros(64, 3, 7, 7)
    w[:, 0, 3, 3] = 1.0
    with Hook(dev) as hook:
        st = Stem(dev, PREC, w, torch.ones(64), torch.zeros(64))
        x = torch.zeros(2, 3, 224, 224, device=dev)
        for val, word in ((TOP, False), (OVF, True)):
            for n_img, oy, ox, c in ((0, 0, 0, 0), (1, 111, 111, 63), (0, 55, 2, 31), (1, 1, 110, 7)):
                x[n_img, 0, 2 * oy, 2 * ox] = 1.0
                st.scale[c] = val
                hook.word()
                g0 = st.run(0, x, 1)
                assert not hook.word(), "the un-pooled stem kernel has no sentinel"
                v0 = g0.values((2, 112, 112, 64), "stem form 0")
                assert bool(torch.isinf(v0[n_img, oy, ox, c])) == word and int((~torch.isfinite(v0)).sum()) == int(word)
                g1 = st.maxpool(g0, 2)
                assert hook.word() == word, ("maxpool after the un-pooled stem", val, (n_img, oy, ox, c))
                assert bool((~torch.isfinite(g1.values((2, 56, 56, 64), "maxpool"))).any()) == word
                x[n_img, 0, 2 * oy, 2 * ox] = 0.0
                st.scale[c] = 1.0


@gpu
def test_maxpool_sentinel(dev):
    """ap_maxpool_nhwc carries an inf from each of the nine window positions (and from every position of a 16-byte store) to the
    word; 65504 everywhere leaves it 0; the result is max_pool2d of the input"""
    Nn, L = _lib()
    with Hook(dev) as hook:
        N = 2
        x = torch.full((N, 112, 112, 64), 3.0, dtype=torch.float16, device=dev)
        g = Guarded(dev, PREC, N * 56 * 56 * 64)

        def run(what, word):
            hook.word()
            Nn.check(L.ap_maxpool_nhwc(Nn.PRECISIONS[PREC], _p(x), _p(g.out), N, Nn.stream_ptr(dev)), "ap_maxpool_nhwc")
            w = hook.word()
            want = F.max_pool2d(x.cpu().double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(torch.float16)
            assert_case(what, w, g.values((N, 56, 56, 64), what).cpu().to(torch.float16), want)
            assert w == word, what
        x[:] = F16_MAX
        run("maxpool top", False)
        x[:] = 3.0
        k = 0
        for n_img, py, px in ((0, 0, 0), (1, 55, 55), (0, 17, 40), (1, 31, 0)):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    iy, ix = 2 * py + dy, 2 * px + dx
                    if not (0 <= iy < 112 and 0 <= ix < 112):
                        continue
                    c = (11 * k) % 64
                    k += 1
                    x[n_img, iy, ix, c] = float("inf")
                    run("maxpool inf at window (%d, %d) of pooled pixel %s channel %d" % (dy, dx, (n_img, py, px), c), True)
                    x[n_img, iy, ix, c] = 3.0
        assert k >= 24


@gpu
def test_avgpool_sentinel(dev):
    """ap_avgpool_nhwc sets the word for an inf or NaN feature (any pixel, any channel) and stays silent at 65504"""
    Nn, L = _lib()
    with Hook(dev) as hook:
        for N, C in ((1, 2048), (3, 256)):
            x = torch.full((N, 49, C), F16_MAX, dtype=torch.float16, device=dev)
            out = torch.empty(N, C, device=dev)

            def run():
                hook.word()
                Nn.check(L.ap_avgpool_nhwc(Nn.PRECISIONS[PREC], _p(x), _p(out), N, C, Nn.stream_ptr(dev)), "ap_avgpool_nhwc")
                return hook.word()
            assert not run() and bool((out == F16_MAX).all()), "silent at 65504"
            for n_img, pix, c in ((0, 0, 0), (N - 1, 48, C - 1), (N // 2, 24, C // 2 + 3), (0, 48, 7)):
                for val in (float("inf"), float("-inf"), float("nan")):
                    x[n_img, pix, c] = val
                    assert run(), ("avgpool", N, C, val, (n_img, pix, c))
                    bad = ~torch.isfinite(out)
                    assert int(bad.sum()) == 1 and bool(bad[n_img, c])
                    x[n_img, pix, c] = F16_MAX


@gpu
def test_other_precisions_are_silent(dev):
    """bf16 storage: values of 1e6 are ordinary; the hook hands the bf16 kernels no word, its status is AP_OK for bf16, bf16x2 and
    fp32, and the word itself (read through the fp16 status) was never set"""
    Nn, L = _lib()
    with Hook(dev) as hook:
        hook.word()
        name, N, H, W, Cin, Cout, k, s, p = shp = SHAPES[3]
        x = torch.zeros(N, H, W, Cin); x[..., 0] = 1.0
        w = torch.zeros(Cout, k, k, Cin); w[:, k // 2, k // 2, 0] = 1.0
        xd, wd = _to_storage(x, "bf16", dev)[0], _w_dev(w, "bf16", dev)
        sd, hd = _bn_dev(torch.full((Cout,), 1.0e6), torch.zeros(Cout), dev)
        g = Guarded(dev, "bf16", N * H * W * Cout)
        for cfg in (-1, 5, 11):
            Nn.check(L.ap_set_conv_config(cfg), "ap_set_conv_config")
            try:
                Nn.check(L.ap_conv2d_nhwc(Nn.PRECISIONS["bf16"], _p(xd), _p(wd), _p(sd), _p(hd), None, _p(g.out), N, H, W, Cin, Cout, k, s, p, 1,
                                          Nn.stream_ptr(dev)), "ap_conv2d_nhwc")
            finally:
                L.ap_set_conv_config(-1)
            for prec in ("bf16", "bf16x2", "fp32"):
                assert L.ap_debug_range_status(Nn.PRECISIONS[prec], Nn.stream_ptr(dev), 1) == 0
            torch.cuda.synchronize()
            assert bool((g.values((N * H * W, Cout), "bf16 1e6") == float(operands(torch.tensor(1.0e6), "bf16"))).all())
            assert not hook.word()
        xp = torch.full((1, 49, 256), 1.0e6, dtype=torch.bfloat16, device=dev)
        out = torch.empty(1, 256, device=dev)
        Nn.check(L.ap_avgpool_nhwc(Nn.PRECISIONS["bf16"], _p(xp), _p(out), 1, 256, Nn.stream_ptr(dev)), "ap_avgpool_nhwc")
        assert L.ap_debug_range_status(Nn.PRECISIONS["bf16"], Nn.stream_ptr(dev), 0) == 0 and not hook.word()
    # hook off: the fp16 entries pass no word, nothing is reported
    op = Conv2d(dev, SHAPES[3])
    op.load(conv_case(SHAPES[3], "one", (5, 9)))
    op.launch()
    torch.cuda.synchronize()
    assert int(torch.isinf(op.g.out).sum()) == 1
    assert L.ap_debug_range_status(Nn.PRECISIONS[PREC], Nn.stream_ptr(dev), 1) == 0
    with Hook(dev) as hook:
        assert not hook.word(), "a launch with the hook off reached the word"


# ---- api_trunk.hip: the range word reaches the kernel the plan chose for each site
SITES = ["layer1.0", "layer1.1", "layer1.2", "layer2.0", "layer2.1", "layer3.0", "layer3.2", "layer4.0", "layer4.2"]
KNOBS_DEFAULT = dict(set_fuse_block=1, set_fuse_pair=1, set_fuse_tail=1, set_fuse_ds=1, set_fuse_stem=1, set_pw_conv=1, set_img3=1,
                     set_img_block=1, set_s2p=0)
KNOB_SETS = [("default", {}),
             ("unfused", dict(set_fuse_block=0, set_fuse_pair=0, set_fuse_tail=0, set_fuse_ds=0, set_fuse_stem=0, set_pw_conv=0, set_img3=0,
                              set_img_block=0)),
             ("s2p", dict(set_s2p=1)),
             ("image kernels forced", dict(set_img3=2, set_img_block=2, set_pw_conv=2))]


@pytest.fixture(scope="module")
def sentinel_net(dev):
    from airpose_amd import copenet_model
    return copenet_model.getcopenet(MEAN_PARAMS, precision="f16").eval()


@gpu
@pytest.mark.parametrize("bn", ["bn1", "bn2"])
@pytest.mark.parametrize("site", SITES)
def test_trunk_reports_one_masked_site(dev, copenet_sd, sentinel_net, site, bn):
    """One bottleneck per distinct kernel path of the fp16 plan, and in it bn1 or bn2: that BatchNorm overflows in one channel c
    (weight 0, bias 1e6: +inf at every pixel, whatever the checkpoint's statistics), the
    consuming convolution carries -1 on input channel c (every tap, every output) under a positive BatchNorm weight, so the next
    stored tensor is relu(-inf or finite) -- finite -- and so are the features: the average pool cannot have raised the flag, nothing
    downstream saw an inf, and range_status() must raise because of the ONE kernel the plan chose for that site.  Default knobs, every
    fusion off (the generic kernels), the polyphase conv2 of layer2.0 on, and the image-resident kernels forced.
    (Block outputs: the residual carries an overflow to the features; the operator tests above cover them.)"""
    from airpose_amd import _native as Nn
    net = sentinel_net
    c = 5
    sd = {k: v.clone() for k, v in copenet_sd.items()}
    sd[site + "." + bn + ".weight"][c] = 0.0                  # the channel is its bias wherever the normalised input is finite: 1e6 -> +inf
    sd[site + "." + bn + ".bias"][c] = 1.0e6
    conv, nbn = ("conv2", "bn2") if bn == "bn1" else ("conv3", "bn3")
    sd["%s.%s.weight" % (site, conv)][:, c] = -1.0
    sd["%s.%s.weight" % (site, nbn)] = sd["%s.%s.weight" % (site, nbn)].abs().clamp_min(0.05)
    net.load_state_dict(sd)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(17)).to(dev)
    try:
        for name, knobs in KNOB_SETS:
            for k, v in dict(KNOBS_DEFAULT, **knobs).items():
                getattr(net, k)(v)
            feat = net.forward_feat_ext(x)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(feat).all()), (site, bn, name, "the overflow was not masked: the features are not finite")
            raised = False
            try:
                net.range_status(reset=True)
            except Nn.RangeError:
                raised = True
            assert raised, (site, bn, name, "the overflow of this site was not reported")
            net.range_status()                               # cleared
    finally:
        for k, v in KNOBS_DEFAULT.items():
            getattr(net, k)(v)
        try:
            net.range_status(reset=True)
        except Nn.RangeError:
            pass


@gpu
def test_trunk_clean_checkpoint_is_silent_under_every_knob_set(dev, copenet_sd, sentinel_net):
    """The same four schedules on the unmodified checkpoint: finite features, no report"""
    net = sentinel_net
    net.load_state_dict(copenet_sd)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(17)).to(dev)
    try:
        for name, knobs in KNOB_SETS:
            for k, v in dict(KNOBS_DEFAULT, **knobs).items():
                getattr(net, k)(v)
            assert bool(torch.isfinite(net.forward_feat_ext(x)).all()), name
            net.range_status()
    finally:
        for k, v in KNOBS_DEFAULT.items():
            getattr(net, k)(v)
