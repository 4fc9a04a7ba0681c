"""Element-wise fp64 ground truth for the inference regressor heads: the 13 kernels of airpose_amd/csrc/regressor.hip and their
drivers in api_heads.hip (the IEF loop of forward / forward_ief / forward_reg, regressor_step, the view-split halves, the hmr,
copenet_singleview and muhmr heads), and the linear-layer use of conv_igemm.hip under them.  Companion of test_smplx_fwd_fp64.py and
test_conv_fwd_fp64.py; evaluate / check / report of test_stem_pool_fp64.py, Arena / check_slices of grad_shapes_util.py, the
references, emulation and inputs of reg_util.py.

Kernel -> test
  reg_init_kernel, reg_update_assemble_kernel,   test_two_view_paths[*-gemm | *-literal], test_step_paths (single-view form with a partner
    reg_output_kernel                            buffer), test_singleview_paths (no partner), test_descending_batches_reuse_the_workspace
  reg_feat_splitk_kernel, reg_fold_ief_kernel    test_two_view_paths[*-fused] (two views, contiguous and separate feature allocations, NULL /
                                                 (1, w) / (B, w) initial states, w = 132 and 144), test_step_paths[fused] (partner_ld 136
                                                 and 144), test_singleview_paths[fused], test_step_is_the_matching_view_of_forward_reg
  reg_feat_sum_kernel,                           test_split_step (B = 1, 7, 8, 9, 63, 64, 65; partner_ld 136 and 144; every stage on the
    reg_step_half_kernel<0, 148, false>,         kernel's own stored input and end to end)
    reg_step_half_kernel<148, 136, true>
  hmr_init_kernel, hmr_update_kernel             test_hmr_reg (NULL, (1, w), (B, w) initial states; iters 1, 2, 3, 5)
  hmr_output_kernel                              test_hmr_output
  probe_normal_kernel, probe_bb_kernel           test_probe_is_seeded (through ap_net_parity_probe: the same seed twice is bit-equal,
                                                 another seed differs; no more is asserted)
  word_copy_kernel                               covered by the range-slot tests of test_gpu_parity.py
  conv_igemm_kernel<float, 64, 64> as a linear   fold = 1 / fuse_ief = 0: Cout 148, K 2048 and 288, ldy = ldr = 160 != Cout; hmr: K 160,
    layer                                        ldx 160; fold = 0: Cout 1024 and 148, K 2048, 288, 1024, a residual with its own leading
                                                 dimension; M = 2 .. 106 around its 64-row tile (rows 64 and 66 at B = 32, 33)

Reference.  The literal chain of the reference model in fp64 -- model_copenet.py forward / forward_reg as restated in
oracle/copenet_ref -- on exactly the fp32 values the kernel receives, written in reg_util.py from the state dict with the
assembled 2332-column row per view and iteration exposed.  test_reference_is_the_oracle holds it to oracle/copenet_ref (cast to
fp64) at 1e-12, the re-mapped muhmr / singleview / hmr layouts included; test_fold_is_the_chain holds the fp64 fold Wf = Wd W2 W1,
bf = Wd (W2 b1 + b2) + bd to it within 1e-3 u A (measured on the CPU: about 2e-9 u A), so the two are interchangeable as references.

Bars of the folded paths (derived, none measured).  |got - ref| <= g(D) A,  g(D) = D u / (1 - D u),  u = 2^-24,
A = |state| + |bf| + |Wf| |row|  (the folded map on absolute values, formed in fp64).  D counts the roundings one product passes
through, from the code:
  fused    regressor.hip, reg_feat_splitk_kernel / reg_fold_ief_kernel:  1  (float)row[j] of api_net.hip's fold (Wf; bf alike)
           + 64  `acc[r] = fmaf(wv[u], xs[r][...], acc[r])`, KPT = KCH / KQ = 64 per thread  (state columns: 72, `d0 = fmaf(wv[u], S[0][...], d0)`)
           + 2   `(red[0] + red[1]) + (red[2] + red[3])`, the quarter tree
           + 8   `for (ks < KSPLIT) h += part[...]`, eight partial sums onto the bias  (state columns: none)
           + 2   `st[v][oo] += H[v][oo] + (...)`:  D = 1 + max(64 + 2 + 8, 72 + 2) + 2 = 77
  split    hfeat: 1 + 64 + 2 + 8 = 75 (on |bf| + |Wf| |xf|).  partial on the kernel's own hfeat: 1 + 37 (`d = fmaf(w[k * OLD],
           S[q * KPT + k], d)`, KPT = 37 of reg_step_half_kernel<0, 148>) + 2 + 1 (`base[...] + (...)`) = 41.  out on the kernel's own
           partial: 1 + 34 (<148, 136>) + 2 + 1 + 1 (`pose_in[...] + v`) = 39.  End to end a feature product passes 75 + 3 = 78.
  gemm     api_heads.hip, regressor_run: 1 (Wf) + (2048 + 3) (run_gemm(Lf, xf): an fp32 MFMA chain of K products in index order and
           the scale / shift / residual epilogue, the count of test_conv_fwd_fp64.py) + (288 + 3) (run_gemm(fold_state, S, ..., Hb):
           H is its residual) + 1 (`val += delta[...]` of reg_update_assemble_kernel) = 2344
  hmr      hmr_ief: 1 + (2048 + 3) + (160 + 3) + 1 (hmr_update_kernel) = 2216
  zero     where A is 0 the output must be exactly 0 (evaluate()).
Iterations.  The bar is a recurrence in fp64 on absolute matrices (reg_util.ief_bounds): E_0 = 0; the state of iteration t is
within E_t of the reference's, so E_(t+1) = E_t + |Wf[:, state columns]| E_t (own view) + |Wf[:, partner columns]| E_t (other
view) + g(D) A(|s_t| + E_t).  Derived, not fitted.
Literal chain (set_fold(0), the fallback the fold guard selects): the WEAKER bar.  Its worst-case bound runs over |Wd| |W2| |W1|,
about 3e4 |y| on the synthetic checkpoint against about 35 |y| for the folded A, which bounds nothing.  It gets the project's
per-slice rule instead (grad_shapes_util.check_slices): per output column over the batch, the error against fp64 may be at most
4 x the fp32 CPU oracle's own error on that column, floor 1e-5 of the column's scale.  The fp32 oracle's error is about 1.3e-6
worst, 2e-7 median (CPU), so the floor decides.
hmr_output_kernel: the rotation matrices get test_smplx_fwd_fp64.py's rot6d bar (its Gram-Schmidt derivation), evaluated on the
pose that ap_hmr_reg itself returned for the same features (nothing propagates); betas and cam are bit-equal to ap_hmr_reg's.
Bit-equalities, each where the code guarantees it: every GPU call twice; rows of a batch against the same rows of a larger batch,
in each path (a row's sums run over k only); view-swap symmetry; contiguous against separate feature allocations on the fused path;
regressor_step against the matching view of forward_reg on the fused path (the same fma chains on the same values); partner_ld 136
against 144; the Python wrappers against the C ABI; a descending batch sequence against a fresh handle.

Inputs, mixed within a batch (reg_util.make_inputs): randn (features |randn| 0.8, pooled post-ReLU; state around the mean
parameters; bb U(-.5, .5)^2 x U(.2, 1)); one-hot (everything zero, caller-supplied zero initial theta / shape / position included,
one element 3.0 at a seam: feature columns 0, 63 | 64, 255 | 256, 2047; state-row columns 0, 2 | 3, 5 | 6, 11 | 12, 71 | 72, 137 | 138,
143 | 144, 147 | 148, 215 | 216, 273 | 274, 283, in each view, so that view 1's art column j is seen through view 0's partner column
148 + j; each one-hot's column exceeds 8 x the bar on some output, asserted on the CPU -- by orders of magnitude); alt (neighbouring
samples and the two views: opposite sign, x 4 / x -4 and x 0.5); bcast ((1, w) initial theta / shape against per-row (B, w), w = 132 and
144, NaN in the padding columns).  A batch of 52 one-hots and one randn per path places every seam in every view.
Shapes.  Two views: B = 1, 3, 4, 5, 8, 9, 13 (rows 2 B around FROWS = 8; B = 4 is one tile), 32, 33 on the GEMM paths (rows 64, 66:
conv_igemm's M tile is 64 here -- launch_T takes <64, 64> below 256 tiles of 128), 53.  Single view: B = 1, 7, 8, 9, 63, 64, 65.
iters 1, 2, 3, 5.  Both launch branches of regressor_run (xf1 == xf0 + B 2048 or not).  Outputs live in NaN-filled arenas, which is
why the calls go through the C ABI (the Python wrappers allocate their own outputs); the knobs go through set_fold / set_fuse_ief and
are restored in `finally`, and each wrapper (forward_ief, forward_reg of every variant, regressor_step, the three halves) is held to
the bits of the ABI call.

Finding.  No kernel bug was found: every path sits inside its derived bar (MEASURED below), every guaranteed bit-equality holds.

CPU self-check (no GPU): an fp32 emulation of each path in its own summation order (split-K, k-quarters, tree for the fused
kernel and the split step; index order for the GEMM) sits inside every bar on every family and shape; each of reg_util.MUTATIONS
is rejected by the same check.

MEASURED (below) holds the worst err / bound per kernel path on an MI355X; none of it is used as a bar.
"""
import ctypes

import pytest
import torch

import reg_util as RU
from conftest import MEAN_PARAMS
from grad_shapes_util import Arena, check_slices
from test_stem_pool_fp64 import check, evaluate, report

MEASURED = """
Worst err / bound on an MI355X (256 CUs) per kernel path, over every batch size, iteration count, family and kind of initial state
(python -m pytest tests/test_reg_fwd_fp64.py -m gpu -s); none of it is used as a bar:
  fused IEF (reg_feat_splitk + reg_fold_ief)      copenet 0.0238   muhmr 0.0220   singleview 0.0243   regressor_step 0.0235
  folded map on the GEMM (reg_init / reg_update_assemble / reg_output + conv_igemm)
                                                  copenet 0.0011   muhmr 0.0010   singleview 0.0010   regressor_step 0.0011
  literal chain, per-slice rule (floor 1e-5)      copenet 0.4085   muhmr 0.1403   singleview 0.4036   regressor_step 0.0928
  view-split step                                 hfeat 0.0215   partial 0.0268   finish 0.0276   end to end 0.0232
  hmr head (hmr_init / hmr_update + conv_igemm)   0.0011          hmr_output_kernel rotmat 0.4867 (betas, cam: the bits of ap_hmr_reg)
The fused kernel's figure is the CPU emulation's to four digits (0.0238): split-K, k-quarters and tree are what the kernel runs.  The
GEMM paths use a thousandth of their bar: D = 2344 is a worst case over a chain whose roundings mostly cancel.  The literal chain's
error is 4e-6 of a column's scale at worst, under a floor of 1e-5.  Every bit-equality held.  The 19 GPU tests take 6.4 s together
on the MI355X (four fp32 handles, a fresh one and a bf16 one included), none more than 1.2 s; the CPU tests take 13 s.
"""

SEEDS = {"copenet": 11, "hmr": 12, "singleview": 13, "muhmr": 14}
B_TWO = (1, 3, 4, 5, 8, 9, 13)
B_GEMM = (32, 33)
B_ONE = (1, 7, 8, 9, 63, 64, 65)
ITERS = (1, 2, 3, 5)
D_OF = {"fused": RU.D_FUSED, "gemm": RU.D_GEMM, "split": RU.D_SPLIT, "hmr": RU.D_HMR, "literal": RU.D_GEMM}
KNOBS = {"fused": (1, 1), "gemm": (1, 0), "literal": (0, 0)}

_LAYOUTS, _SDS = {}, {}


def sd_of(variant):
    from airpose_amd import weights as W
    if variant not in _SDS:
        _SDS[variant] = W.to_torch(W.copenet_state_dict(SEEDS[variant], MEAN_PARAMS, variant=variant))
    return _SDS[variant]


def layout_of(variant):
    if variant not in _LAYOUTS:
        _LAYOUTS[variant] = RU.layout(sd_of(variant), variant)
    return _LAYOUTS[variant]


def two_view_cases(path):
    """(B, iters, init, w, shift, all_onehot, contiguous) of a two-view sweep: every B, every iteration count, every kind of
    initial state, both feature layouts; the last case places all 52 one-hots"""
    Bs = B_TWO + (B_GEMM if path != "fused" else ())
    inits = ("rows", "rows", "bcast", "rows", "none")
    out = []
    for i, B in enumerate(Bs):
        out.append((B, ITERS[i % 4], inits[i % 5], (132, 144)[i % 2], i, False, i % 2 == 0))
    out.append((13, 5, "bcast", 144, 1, False, False))
    out.append((53, 2, "rows", 144, 0, True, True))
    return out


def one_view_cases():
    return [(B, ITERS[i % 4], ("rows", "rows", "bcast", "none")[i % 4], (132, 144)[i % 2], i, False) for i, B in enumerate(B_ONE)] + \
        [(27, 1, "rows", 132, 0, True)]


def final_bar(ref):
    return ref["bounds"][-1]


# ------------------------------------------------------------------------------------------------ CPU: the references
def test_reference_is_the_oracle():
    """reg_util's chain (with its exposed rows) reproduces oracle/copenet_ref in fp64: forward_reg and the IEF loop of the two-view
    model, hmr_forward_reg, and the muhmr / singleview literal evaluations on their ORIGINAL column order (the re-mapping of
    finalize_regressor restated in reg_util.layout)."""
    from oracle import copenet_ref
    B = 5
    for variant in ("copenet", "muhmr", "singleview", "hmr"):
        L = layout_of(variant)
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd_of(variant).items()}
        V = 2 if variant in ("copenet", "muhmr") else 1
        inp = RU.make_inputs(L, V, B, 3, init="rows")
        ref = RU.reference(L, inp, 3, 1)
        st0, xf, bb = ref["st0"], ref["xf"], ref["bb"]
        s1, s3 = ref["states"][1], ref["states"][3]
        if variant == "copenet":
            sl = lambda a, b: (st0[0][:, a:b], st0[1][:, a:b])
            one = copenet_ref.forward_reg(sd, xf[0], xf[1], bb[0], bb[1], *sl(0, 3), *sl(3, 9), *sl(9, 135), *sl(135, 145))
            many = copenet_ref.ief(sd, xf[0], xf[1], bb[0], bb[1], *sl(0, 3), st0[0][:, 3:135], st0[1][:, 3:135], *sl(135, 145), iters=3)
            for got, want in ((s1, one), (s3, many)):
                for v in (0, 1):
                    assert float((got[v][:, :135] - want[2 * v]).abs().max()) < 1e-12
                    assert float((got[v][:, 135:] - want[2 * v + 1]).abs().max()) < 1e-12
            assert ref["rows"][0].shape == (2, B, 2332)
            assert torch.equal(ref["rows"][1][0][:, 2048 + 148:], s1[1][:, 9:145])          # the cross-view swap, exposed
        elif variant == "muhmr":                             # model_muhmr.py:163-197 as in copenet_ref.muhmr_forward
            cam, pose, shape = [st0[v][:, :3] for v in (0, 1)], [st0[v][:, 3:135] for v in (0, 1)], [st0[v][:, 135:] for v in (0, 1)]
            for v in (0, 1):
                xc = copenet_ref._lin(copenet_ref._lin(torch.cat([xf[v], cam[v], pose[v], shape[v], pose[1 - v][:, 6:], shape[1 - v]], 1), sd, "fc1"), sd, "fc2")
                want = torch.cat([cam[v] + copenet_ref._lin(xc, sd, "deccam"), pose[v] + copenet_ref._lin(xc, sd, "decpose"),
                                  shape[v] + copenet_ref._lin(xc, sd, "decshape")], 1)
                assert float((s1[v] - want).abs().max()) < 1e-12
        elif variant == "singleview":                        # model_copenet_singleview.py:156-168 as in copenet_ref.singleview_forward
            pose, shape = st0[0][:, :135], st0[0][:, 135:]
            for _ in range(3):
                xc = copenet_ref._lin(copenet_ref._lin(torch.cat([xf[0], bb[0], pose, shape], 1), sd, "fc1"), sd, "fc2")
                pose, shape = copenet_ref._lin(xc, sd, "decpose") + pose, copenet_ref._lin(xc, sd, "decshape") + shape
            assert float((s3[0] - torch.cat([pose, shape], 1)).abs().max()) < 1e-12
        else:
            p, s, c = copenet_ref.hmr_forward_reg(sd, xf[0], st0[0][:, :132], st0[0][:, 132:142], st0[0][:, 142:])
            assert float((s1[0] - torch.cat([p, s, c], 1)).abs().max()) < 1e-12


def test_fold_is_the_chain():
    """the fp64 fold differs from the literal chain by less than 1e-3 u A: the two references are interchangeable"""
    ratios = {}
    for variant in ("copenet", "muhmr", "singleview", "hmr"):
        L = layout_of(variant)
        V = 2 if variant in ("copenet", "muhmr") else 1
        inp = RU.make_inputs(L, V, 9, 5, init="rows")
        ref = RU.reference(L, inp, 1, 1)
        fold = RU.ief_ref(L, ref["xf"], ref["bb"], ref["st0"], 1, fold=True)[0][1]
        check("fold " + variant, variant, fold, ref["states"][1], 1e-3 * RU.U32 * ref["A0"], ratios)
        assert bool((ref["A0"] >= ref["states"][1].abs() * (1 - 1e-12)).all())
    report("fold against chain, bar 1e-3 u A", ratios)
    assert (RU.D_FEAT, RU.D_FUSED, RU.D_LOCAL, RU.D_FINISH, RU.D_SPLIT, RU.D_GEMM, RU.D_HMR) == (75, 77, 41, 39, 78, 2344, 2216)


def test_every_seam_is_placed():
    """the sweeps place every one-hot of reg_util.ONEHOTS in every view, per path"""
    L = layout_of("copenet")
    for path in ("fused", "gemm"):
        seen = set()
        for B, iters, init, w, shift, allone, contig in two_view_cases(path):
            seen |= set(RU.make_inputs(L, 2, B, shift, init, w, shift, allone)["onehots"].values())
        assert seen >= {(k, c, v) for k, c in RU.ONEHOTS for v in (0, 1)}
    seen = set()
    for B, iters, init, w, shift, allone in one_view_cases():
        seen |= set(RU.make_inputs(L, 1, B, shift, "rows", w, shift, allone, partner=True)["onehots"].values())
    assert seen >= {(k, c, 0) for k, c in RU.ONEHOTS}
    Lh = layout_of("hmr")
    seen = set()
    for B, iters, init, w, shift, allone in one_view_cases():
        seen |= set(RU.make_inputs(Lh, 1, B, shift, init, w, shift, allone)["onehots"].values())
    assert seen >= {(k, c, 0) for k, c in RU.HMR_ONEHOTS}


# ------------------------------------------------------------------------------------------------ CPU: self-check
APPLIES = {
    "fused": ("swap_partner_blocks", "own_art", "shift_state", "drop_last_chunk", "quarter_280", "skip_out_144", "view1_bb0",
              "bcast_per_row", "rows_as_bcast", "drop_last_residual", "H_only_iter2"),
    "gemm": ("swap_partner_blocks", "own_art", "shift_state", "skip_out_144", "view1_bb0", "bcast_per_row", "rows_as_bcast",
             "drop_last_residual", "H_only_iter2"),
    "split": ("shift_state", "drop_last_chunk", "quarter_280"),
    "hmr": ("hmr_stride_145", "bcast_per_row", "rows_as_bcast"),
}


def _cpu_cases(path):
    if path == "split":
        return [(1, B, 1, "rows", w, shift, allone, True) for B, _, _, w, shift, allone in one_view_cases() if B in (1, 9, 27)]
    if path == "hmr":
        return [(1, B, iters, init, w, shift, allone, False) for B, iters, init, w, shift, allone in one_view_cases() if B in (7, 8, 9, 27)]
    keep = (1, 4, 5, 8, 13, 33, 53) if path != "literal" else (3, 5)
    return [(2, B, iters, init, w, shift, allone, False) for B, iters, init, w, shift, allone, _ in two_view_cases(path) if B in keep]


@pytest.mark.parametrize("path", ["fused", "gemm", "split", "hmr", "literal"])
def test_cpu_emulation_is_inside_the_bars_and_mutations_are_not(path):
    """The fp32 emulation of the path, in its own summation order, sits inside the bar on every case; every one-hot's column
    exceeds 8 x the bar on some output; each mutation that the path can suffer is rejected by the same check (in the batch of all
    seams at the least; a case may leave a mutation without effect, as the mean initial state of both views does to own_art)."""
    L = layout_of("hmr" if path == "hmr" else "copenet")
    ratios, rejected = {}, {}
    for V, B, iters, init, w, shift, allone, partner in _cpu_cases(path):
        inp = RU.make_inputs(L, V, B, shift, init, w, shift, allone, partner=partner)
        ref = RU.reference(L, inp, iters, D_OF[path])
        what = "%s B=%d iters=%d %s" % (path, B, iters, init)
        marg = [m for m in RU.onehot_margins(L, inp, ref).values() if m is not None]
        assert not marg or min(marg) > 8, (what, marg)
        if marg:
            ratios["min one-hot / bar"] = min(ratios.get("min one-hot / bar", float("inf")), min(marg))
        if path == "literal":                                # the per-slice rule; the fp32 CPU oracle is torch's own fp32 chain
            L32 = RU.cast(L, torch.float32)
            cpu32 = RU.ief_ref(L32, inp["xf"], inp["bb"], ref["st0"].float(), iters)[0][-1]
            emu = RU.emulate(L, path, ref["xf"], ref["bb"], ref["st0"], iters)
            check_slices(what, "literal", emu.reshape(-1, 145), ref["states"][-1].reshape(-1, 145), cpu32.reshape(-1, 145), 1, ratios)
            continue
        if path == "split":
            emu, (hfeat, partial) = RU.emulate(L, path, ref["xf"], ref["bb"], ref["st0"], 1, ref["partner"])
            _check_split_stages(L, what, ref, hfeat, partial, emu[0], ratios)
        else:
            emu = RU.emulate(L, path, ref["xf"], ref["bb"], ref["st0"], iters, ref["partner"])
        check(what, path, emu, ref["states"][-1], final_bar(ref), ratios)
        for mut in APPLIES[path]:
            if mut == "H_only_iter2" and iters < 2:
                continue
            if mut == "bcast_per_row" and (init != "bcast" or B < 2):
                continue
            if mut == "rows_as_bcast" and (init != "rows" or B < 2):
                continue
            if mut == "hmr_stride_145" and B < 2:
                continue
            st0 = RU.state0(L, inp, mut)
            bad = RU.emulate(L, path, ref["xf"], ref["bb"], st0, iters, ref["partner"], mut=mut)
            bad = bad[0] if path == "split" else bad
            ok, r, _, _ = evaluate(bad, ref["states"][-1], final_bar(ref))
            rejected.setdefault(mut, []).append((what, ok, r))
    if path == "literal":
        report("emulation " + path, {k: v for k, v in ratios.items()})
        return
    for mut in APPLIES[path]:
        runs = rejected.get(mut, [])
        assert runs, (path, mut, "no case exercises this mutation")
        assert not runs[-1][1], (path, mut, "the checker accepts this mutation on the batch of all seams", runs[-1])
        ratios["!%s (%d of %d cases)" % (mut, sum(not ok for _, ok, _ in runs), len(runs))] = max(r for _, _, r in runs)
    report("emulation " + path, ratios)


def _check_split_stages(L, what, ref, hfeat, partial, out, ratios):
    """the three stages of the view-split step, each on the stored output of the one before (fp32 values in fp64 tensors)"""
    Wa, xf, st = L["Wf"].abs(), ref["xf"][0], ref["st0"][0]
    row = ref["rows"][0][0]
    loc, par = row[:, RU.NF:RU.NF + 148], row[:, RU.NF + 148:]
    h_ref = L["bf"] + xf @ L["Wf"][:, :RU.NF].t()
    check(what, "hfeat", hfeat[:, :145], h_ref, RU.g(RU.D_FEAT) * (L["bf"].abs() + xf.abs() @ Wa[:, :RU.NF].t()), ratios)
    p_ref = hfeat[:, :145].double() + loc @ L["Wf"][:, RU.NF:RU.NF + 148].t()
    check(what, "partial", partial[:, :145], p_ref,
          RU.g(RU.D_LOCAL) * (hfeat[:, :145].double().abs() + loc.abs() @ Wa[:, RU.NF:RU.NF + 148].t()), ratios)
    o_ref = st + partial[:, :145].double() + par @ L["Wf"][:, RU.NF + 148:].t()
    check(what, "finish", out, o_ref,
          RU.g(RU.D_FINISH) * (st.abs() + partial[:, :145].double().abs() + par.abs() @ Wa[:, RU.NF + 148:].t()), ratios)


def test_rot6d_mutation_is_rejected():
    """hmr_output_kernel's Gram-Schmidt in fp32 sits inside test_smplx_fwd_fp64's rot6d bar; reading rows instead of the interleaved
    columns does not"""
    from test_smplx_fwd_fp64 import rot6d_ref
    L = layout_of("hmr")
    x6 = (L["mean_theta"].float() + 0.3 * torch.randn(9, 132, generator=torch.Generator().manual_seed(1))).reshape(-1, 6)
    r64, bar = rot6d_ref(x6)
    ratios = {}
    check("rot6d", "rot6d", RU.rot6d_fp32(x6), r64, bar, ratios)
    ok, r, _, _ = evaluate(RU.rot6d_fp32(x6, "rot6d_rows"), r64, bar)
    assert not ok, ("rot6d_rows", r)
    ratios["!rot6d_rows"] = r
    report("rot6d emulation", ratios)
    assert set(RU.MUTATIONS) == {m for ms in APPLIES.values() for m in ms} | {"rot6d_rows"}


# ------------------------------------------------------------------------------------------------ GPU side
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(t):
    return t.contiguous().view(torch.int32)


class Head(object):
    """One fp32 handle of a variant and the C ABI on it: every output in a NaN-filled Arena, every call twice, bit-equal"""
    MODULES = {"copenet": "copenet_model", "hmr": "hmr_model", "singleview": "copenet_singleview_model", "muhmr": "muhmr_model"}

    def __init__(self, dev, variant):
        import importlib
        from airpose_amd import _native as Nn
        self.Nn, self.lib, self.dev, self.variant = Nn, Nn.lib(), dev, variant
        self.net = importlib.import_module("airpose_amd." + self.MODULES[variant]).getcopenet(MEAN_PARAMS, precision="fp32").eval()
        self.net.load_state_dict(sd_of(variant))
        with torch.cuda.device(dev):
            self.h = self.net._native(dev)
        self.L = layout_of(variant)
        self.st = Nn.stream_ptr(dev)

    def path(self, path):
        fold, fuse = KNOBS[path]
        self.net.set_fold(fold)
        self.net.set_fuse_ief(fuse)
        assert self.net.fold_status()[0] == (1 if fold else 2), "the fold guard rejected the synthetic checkpoint"

    def restore(self):
        self.net.set_fold(1)
        self.net.set_fuse_ief(1)

    def d(self, t):
        return None if t is None else t.float().contiguous().to(self.dev)

    def twice(self, what, shapes, call):
        """call(arena) -> status, twice on fresh arenas; -> the outputs on the CPU"""
        res = []
        for _ in range(2):
            ar = Arena(self.dev, shapes)
            self.Nn.check(call(ar), what)
            torch.cuda.synchronize()
            ar.untouched(list(shapes), what)
            res.append(ar)
        for k in shapes:
            assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), (what, k, "two identical calls differ")
        return {k: res[1][k].cpu() for k in shapes}

    @staticmethod
    def _init(ts, init):
        return [(t, 0 if init == "bcast" else (0 if t is None else t.shape[1])) for t in ts]

    def fwd2(self, inp, iters, contiguous=True, what="ap_regressor_fwd"):
        """ap_regressor_fwd -> final states [2][B][145] (pose | betas)"""
        B = inp["xf"].shape[1]
        if contiguous:
            xf = self.d(inp["xf"])
            x0, x1 = xf[0], xf[1]
        else:                                                # a NaN row between the views: xf1 != xf0 + B 2048
            xf = torch.full((2 * B + 1, 2048), float("nan"), device=self.dev)
            xf[:B], xf[B + 1:] = self.d(inp["xf"][0]), self.d(inp["xf"][1])
            x0, x1 = xf[:B], xf[B + 1:]
        bb, pos = self.d(inp["bb"]), self.d(inp["pos"])
        th = self._init([self.d(t) for t in inp["theta"]], inp["init"])
        sh = self._init([self.d(t) for t in inp["shape"]], inp["init"])
        call = lambda ar: self.lib.ap_regressor_fwd(
            self.h, _p(x0), _p(x1), _p(bb[0]), _p(bb[1]), _p(pos[0]), _p(pos[1]), _p(th[0][0]), th[0][1], _p(th[1][0]), th[1][1],
            _p(sh[0][0]), sh[0][1], _p(sh[1][0]), sh[1][1], B, iters, _p(ar["pose0"]), _p(ar["betas0"]), _p(ar["pose1"]), _p(ar["betas1"]), self.st)
        o = self.twice(what, {"pose0": (B, 135), "betas0": (B, 10), "pose1": (B, 135), "betas1": (B, 10)}, call)
        return torch.stack([torch.cat([o["pose0"], o["betas0"]], 1), torch.cat([o["pose1"], o["betas1"]], 1)])

    def _pose_in(self, inp):
        return self.d(torch.cat([inp["pos"][0], inp["theta"][0][:, :132]], 1)), self.d(inp["shape"][0])

    def _partner(self, inp, ld):
        pt = torch.full((inp["partner"].shape[1], ld), float("nan"))
        pt[:, :136] = inp["partner"][0]
        return self.d(pt)

    def step(self, inp, ld=136, what="ap_regressor_step"):
        B = inp["xf"].shape[1]
        xf, bb, pt = self.d(inp["xf"][0]), self.d(inp["bb"][0]), self._partner(inp, ld)
        pose, betas = self._pose_in(inp)
        call = lambda ar: self.lib.ap_regressor_step(self.h, _p(xf), _p(bb), _p(pose), _p(betas), _p(pt), ld, B, _p(ar["pose"]), _p(ar["betas"]), self.st)
        o = self.twice(what, {"pose": (B, 135), "betas": (B, 10)}, call)
        return torch.cat([o["pose"], o["betas"]], 1)[None]

    def split_step(self, inp, ld=136):
        """ap_regressor_feat_part, _step_local, _step_finish -> (hfeat [B][148], partial [B][148], out [B][145]); the finish reads a
        partial whose columns 145 .. 147 hold NaN"""
        B = inp["xf"].shape[1]
        xf, bb, pt = self.d(inp["xf"][0]), self.d(inp["bb"][0]), self._partner(inp, ld)
        pose, betas = self._pose_in(inp)
        hf = self.twice("ap_regressor_feat_part", {"hfeat": (B, 148)}, lambda ar: self.lib.ap_regressor_feat_part(self.h, _p(xf), B, _p(ar["hfeat"]), self.st))["hfeat"]
        hfd = self.d(hf)
        res = []
        for _ in range(2):                                   # (partial[:, 145:148] is unspecified: not a requested output)
            ar = Arena(self.dev, {"partial": (B, 148)})
            self.Nn.check(self.lib.ap_regressor_step_local(self.h, _p(hfd), _p(bb), _p(pose), _p(betas), B, _p(ar["partial"]), self.st), "ap_regressor_step_local")
            torch.cuda.synchronize()
            ar.untouched(["partial"], "ap_regressor_step_local")
            res.append(ar["partial"].cpu())
        assert torch.equal(_bits(res[0][:, :145]), _bits(res[1][:, :145])), "two identical ap_regressor_step_local calls differ"
        partial = res[1]
        pin = partial.clone()
        pin[:, 145:] = float("nan")
        pd = self.d(pin)
        o = self.twice("ap_regressor_step_finish", {"pose": (B, 135), "betas": (B, 10)},
                       lambda ar: self.lib.ap_regressor_step_finish(self.h, _p(pd), _p(pose), _p(betas), _p(pt), ld, B, _p(ar["pose"]), _p(ar["betas"]), self.st))
        return hf, partial, torch.cat([o["pose"], o["betas"]], 1)

    def singleview(self, inp, iters, what="ap_singleview_reg"):
        B = inp["xf"].shape[1]
        xf, bb, pos = self.d(inp["xf"][0]), self.d(inp["bb"][0]), self.d(inp["pos"][0])
        (th, ths), = self._init([self.d(inp["theta"][0])], inp["init"])
        (sh, shs), = self._init([self.d(inp["shape"][0])], inp["init"])
        call = lambda ar: self.lib.ap_singleview_reg(self.h, _p(xf), _p(bb), _p(pos), _p(th), ths, _p(sh), shs, B, iters, _p(ar["pose"]), _p(ar["betas"]), self.st)
        o = self.twice(what, {"pose": (B, 135), "betas": (B, 10)}, call)
        return torch.cat([o["pose"], o["betas"]], 1)[None]

    def hmr_reg(self, inp, iters, what="ap_hmr_reg"):
        B = inp["xf"].shape[1]
        xf = self.d(inp["xf"][0])
        (th, ths), = self._init([self.d(inp["theta"][0])], inp["init"])
        (sh, shs), = self._init([self.d(inp["shape"][0])], inp["init"])
        (cm, cms), = self._init([self.d(inp["cam"][0])], inp["init"])
        call = lambda ar: self.lib.ap_hmr_reg(self.h, _p(xf), B, iters, _p(th), ths, _p(sh), shs, _p(cm), cms, _p(ar["pose"]), _p(ar["shape"]), _p(ar["cam"]), self.st)
        o = self.twice(what, {"pose": (B, 132), "shape": (B, 10), "cam": (B, 3)}, call)
        return torch.cat([o["pose"], o["shape"], o["cam"]], 1)[None]


_HEADS = {}


@pytest.fixture(scope="module")
def heads(dev):
    """the four fp32 handles, each built once, on first use"""
    def get(variant):
        if variant not in _HEADS:
            _HEADS[variant] = Head(dev, variant)
        return _HEADS[variant]
    yield get
    _HEADS.clear()


def _check_path(H, path, what, got, ref, ratios, name=None):
    """a path's bar on the final states: the derived recurrence, or (literal chain) the per-slice rule against the fp32 CPU oracle"""
    name = name or path
    if path != "literal":
        check(what, name, got, ref["states"][-1], final_bar(ref), ratios)
        return
    L32 = RU.cast(H.L, torch.float32)
    f = lambda x: None if x is None else x.float()
    cpu32 = RU.ief_ref(L32, f(ref["xf"]), f(ref["bb"]), ref["st0"].float(), len(ref["rows"]), f(ref["partner"]))[0][-1]
    check_slices(what, name, got.reshape(-1, 145), ref["states"][-1].reshape(-1, 145), cpu32.reshape(-1, 145), 1, ratios)


def _swap_views(inp):
    out = dict(inp)
    for k in ("xf", "bb", "pos"):
        out[k] = inp[k].flip(0)
    for k in ("theta", "shape", "cam"):
        out[k] = inp[k][::-1]
    return out


def _subset(inp, n):
    out = dict(inp)
    for k in ("xf", "bb", "pos"):
        out[k] = inp[k][:, :n]
    for k in ("theta", "shape", "cam"):
        out[k] = [None if t is None else (t if t.shape[0] == 1 else t[:n]) for t in inp[k]]
    if inp["partner"] is not None:
        out["partner"] = inp["partner"][:, :n]
    return out


@gpu
@pytest.mark.parametrize("path", ["fused", "gemm", "literal"])
@pytest.mark.parametrize("variant", ["copenet", "muhmr"])
def test_two_view_paths(dev, heads, variant, path):
    """ap_regressor_fwd on each evaluation path: every B, iteration count, kind of initial state and both feature layouts against
    the path's bar; rows of a smaller batch, the swapped views and (fused) the other feature layout bit for bit"""
    H = heads(variant)
    ratios = {}
    try:
        H.path(path)
        for B, iters, init, w, shift, allone, contig in two_view_cases(path):
            inp = RU.make_inputs(H.L, 2, B, shift, init, w, shift, allone)
            ref = RU.reference(H.L, inp, iters, D_OF[path])
            what = "%s %s B=%d iters=%d %s w=%d %s" % (variant, path, B, iters, init, w, "contiguous" if contig else "separate")
            got = H.fwd2(inp, iters, contig, what)
            _check_path(H, path, what, got, ref, ratios)
            if variant == "muhmr" and iters == 1 and init == "rows" and w == 132:
                # the wrapper hands the feature rows in as bb (zero weight in the re-mapped fc1): the same bits
                d, th, sh = H.d, inp["theta"], inp["shape"]
                p0, s0, c0, p1, s1, c1 = H.net.forward_reg(d(inp["xf"][0]), d(inp["xf"][1]), d(th[0][:, :6]), d(th[1][:, :6]), d(th[0][:, 6:]),
                                                           d(th[1][:, 6:]), d(sh[0]), d(sh[1]), d(inp["pos"][0]), d(inp["pos"][1]))
                wr = torch.stack([torch.cat([c0, p0, s0], 1), torch.cat([c1, p1, s1], 1)]).cpu()
                assert torch.equal(_bits(wr), _bits(got)), (what, "the Python wrapper differs from the C ABI")
            if B in (5, 13, 33):
                if path == "fused":
                    assert torch.equal(_bits(H.fwd2(inp, iters, not contig, what)), _bits(got)), (what, "the feature layout changes the bits")
                sw = H.fwd2(_swap_views(inp), iters, contig, what + " swapped")
                assert torch.equal(_bits(sw.flip(0)), _bits(got)), (what, "the views are not symmetric")
                n = {5: 3, 13: 8, 33: 32}[B]
                sub = H.fwd2(_subset(inp, n), iters, contig, what + " subset")
                assert torch.equal(_bits(sub), _bits(got[:, :n])), (what, "rows depend on the batch they are in")
    finally:
        H.restore()
    report("%s two-view %s" % (variant, path), ratios)


@gpu
def test_step_is_the_matching_view_of_forward_reg(dev, heads):
    """fused path: ap_regressor_step with the partner's art | shape is bit-equal to the matching view of a one-iteration
    ap_regressor_fwd (the same fma chains on the same values); so is the Python wrapper"""
    H = heads("copenet")
    for B in (1, 9, 13):
        inp = RU.make_inputs(H.L, 2, B, 40 + B, "rows", 132, B)
        both = H.fwd2(inp, 1)
        for v in (0, 1):
            one = dict(inp, xf=inp["xf"][v:v + 1], bb=inp["bb"][v:v + 1], pos=inp["pos"][v:v + 1], theta=[inp["theta"][v]], shape=[inp["shape"][v]],
                       partner=torch.cat([inp["theta"][1 - v][:, 6:132], inp["shape"][1 - v]], 1)[None])
            got = H.step(one)
            assert torch.equal(_bits(got[0]), _bits(both[v])), (B, v)
            pose, betas = H._pose_in(one)
            p, b = H.net.regressor_step(H.d(one["xf"][0]), H.d(one["bb"][0]), pose, betas, H.d(one["partner"][0]))
            assert torch.equal(_bits(torch.cat([p, b], 1).cpu()), _bits(got[0]))
        d = H.d
        p0, b0, p1, b1 = H.net.forward_ief(d(inp["xf"][0]), d(inp["xf"][1]), d(inp["bb"][0]), d(inp["bb"][1]), d(inp["pos"][0]), d(inp["pos"][1]),
                                           d(inp["theta"][0]), d(inp["theta"][1]), d(inp["shape"][0]), d(inp["shape"][1]), iters=1)
        assert torch.equal(_bits(torch.stack([torch.cat([p0, b0], 1), torch.cat([p1, b1], 1)]).cpu()), _bits(both))


@gpu
@pytest.mark.parametrize("path", ["fused", "gemm", "literal"])
def test_step_paths(dev, heads, path):
    """ap_regressor_step (single-view form with a partner buffer) on each path, partner_ld 136 and 144 with NaN in the padding"""
    H = heads("copenet")
    ratios = {}
    try:
        H.path(path)
        for B, _, _, w, shift, allone in one_view_cases():
            inp = RU.make_inputs(H.L, 1, B, shift, "rows", 132, shift, allone, partner=True)
            ref = RU.reference(H.L, inp, 1, D_OF[path])
            what = "step %s B=%d" % (path, B)
            got = H.step(inp, 136, what)
            _check_path(H, path, what, got, ref, ratios)
            assert torch.equal(_bits(H.step(inp, 144, what + " ld=144")), _bits(got)), (what, "partner_ld changes the bits")
    finally:
        H.restore()
    report("regressor_step %s" % path, ratios)


@gpu
def test_split_step(dev, heads):
    """ap_regressor_feat_part / _step_local / _step_finish: every stage on the kernel's own stored input, the whole step end to
    end, hfeat[:, 145:148] exactly 0, a NaN partial[:, 145:148] not read, partner_ld 136 against 144"""
    H = heads("copenet")
    ratios = {}
    for B, _, _, w, shift, allone in one_view_cases():
        inp = RU.make_inputs(H.L, 1, B, shift, "rows", 132, shift, allone, partner=True)
        ref = RU.reference(H.L, inp, 1, RU.D_SPLIT)
        what = "split step B=%d" % B
        hf, partial, out = H.split_step(inp, 136)
        assert bool((hf[:, 145:] == 0).all()), (what, "hfeat[:, 145:148] is not 0")
        _check_split_stages(H.L, what, ref, hf, partial, out, ratios)
        check(what, "end to end", out[None], ref["states"][-1], final_bar(ref), ratios)
        hf2, partial2, out2 = H.split_step(inp, 144)
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(hf2), _bits(hf)), (what, "partner_ld changes the bits")
        if B == 9:
            p, b = H.net.regressor_step_finish(H.net.regressor_step_local(H.net.regressor_feat_part(H.d(inp["xf"][0])), H.d(inp["bb"][0]), *H._pose_in(inp)),
                                               *H._pose_in(inp), H.d(inp["partner"][0]))
            assert torch.equal(_bits(torch.cat([p, b], 1).cpu()), _bits(out)), "the Python wrappers differ from the C ABI"
    report("view-split step", ratios)


@gpu
@pytest.mark.parametrize("path", ["fused", "gemm", "literal"])
def test_singleview_paths(dev, heads, path):
    """ap_singleview_reg (no partner columns) on each path; the wrapper bit for bit"""
    H = heads("singleview")
    ratios = {}
    try:
        H.path(path)
        for B, iters, init, w, shift, allone in one_view_cases():
            inp = RU.make_inputs(H.L, 1, B, shift, init, w, shift, allone)
            ref = RU.reference(H.L, inp, iters, D_OF[path])
            what = "singleview %s B=%d iters=%d %s" % (path, B, iters, init)
            got = H.singleview(inp, iters, what)
            _check_path(H, path, what, got, ref, ratios)
            if B == 9:
                sub = H.singleview(_subset(inp, 7), iters, what + " subset")
                assert torch.equal(_bits(sub), _bits(got[:, :7])), (what, "rows depend on the batch they are in")
            if init == "rows" and w == 132:
                p, b = H.net.forward_reg(H.d(inp["xf"][0]), H.d(inp["bb"][0]), H._pose_in(inp)[0], H.d(inp["shape"][0]), iters=iters)
                assert torch.equal(_bits(torch.cat([p, b], 1).cpu()), _bits(got[0])), "the Python wrapper differs from the C ABI"
    finally:
        H.restore()
    report("singleview %s" % path, ratios)


@gpu
def test_hmr_reg(dev, heads):
    """ap_hmr_reg: hmr_init_kernel (NULL, (1, w), (B, w) initial states), the folded map on the GEMM at K = 160, hmr_update_kernel"""
    H = heads("hmr")
    ratios = {}
    for B, iters, init, w, shift, allone in one_view_cases():
        inp = RU.make_inputs(H.L, 1, B, shift, init, w, shift, allone)
        ref = RU.reference(H.L, inp, iters, RU.D_HMR)
        what = "hmr B=%d iters=%d %s w=%d" % (B, iters, init, w)
        got = H.hmr_reg(inp, iters, what)
        check(what, "hmr", got, ref["states"][-1], final_bar(ref), ratios)
        if B == 9:
            sub = H.hmr_reg(_subset(inp, 7), iters, what + " subset")
            assert torch.equal(_bits(sub), _bits(got[:, :7])), (what, "rows depend on the batch they are in")
        if init == "rows" and w == 132:
            p, s, c = H.net.forward_reg(H.d(inp["xf"][0]), H.d(inp["theta"][0]), H.d(inp["shape"][0]), H.d(inp["cam"][0]), iters=iters)
            assert torch.equal(_bits(torch.cat([p, s, c], 1).cpu()), _bits(got[0])), "the Python wrapper differs from the C ABI"
    report("hmr head", ratios)


@gpu
def test_hmr_output(dev, heads):
    """hmr_output_kernel through ap_hmr_fwd: the rotation matrices against fp64 Gram-Schmidt of the pose ap_hmr_reg returns for the
    same features (rot6d's bar of test_smplx_fwd_fp64); betas and cam bit-equal to ap_hmr_reg's"""
    from test_smplx_fwd_fp64 import rot6d_ref
    H = heads("hmr")
    ratios = {}
    for B, iters in ((1, 3), (3, 1)):
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        xf = H.net.forward_feat_ext(x)
        L = H.L
        init = [t.float()[None].to(dev) for t in (L["mean_theta"], L["mean_shape"], L["mean_cam"])]
        pose, shape, cam = H.net.forward_reg(xf, *[t.expand(B, -1).contiguous() for t in init], iters=iters)
        call = lambda ar: H.lib.ap_hmr_fwd(H.h, _p(x), B, iters, None, 0, None, 0, None, 0, _p(ar["rotmat"]), _p(ar["betas"]), _p(ar["cam"]), H.st)
        o = H.twice("ap_hmr_fwd", {"rotmat": (B, 22, 3, 3), "betas": (B, 10), "cam": (B, 3)}, call)
        assert torch.equal(_bits(o["betas"]), _bits(shape.cpu())) and torch.equal(_bits(o["cam"]), _bits(cam.cpu()))
        r64, bar = rot6d_ref(pose.cpu().reshape(-1, 6))
        check("ap_hmr_fwd B=%d" % B, "rotmat", o["rotmat"].reshape(-1, 3, 3), r64, bar, ratios)
    report("hmr_output_kernel", ratios)


@gpu
def test_descending_batches_reuse_the_workspace(dev, heads):
    """B = 33, then 3, then 1 on one handle, in each path, equal bit for bit what a handle that never ran a larger batch returns
    (the fresh handle runs B = 1 on every path, then 3, then 33: its workspaces only ever grow)"""
    H, F = heads("copenet"), Head(dev, "copenet")
    cases = [(B, RU.make_inputs(H.L, 2, B, 90 + B, "rows", 132, B)) for B in (33, 3, 1)]
    want = {}
    try:
        for B, inp in reversed(cases):
            for path in KNOBS:
                F.path(path)
                want[path, B] = F.fwd2(inp, 3)
        for path in KNOBS:
            H.path(path)
            for B, inp in cases:
                assert torch.equal(_bits(H.fwd2(inp, 3)), _bits(want[path, B])), (path, B)
    finally:
        H.restore()


@gpu
def test_probe_is_seeded(dev):
    """probe_normal_kernel / probe_bb_kernel through ap_net_parity_probe: the same seed twice is bit-equal, another seed differs"""
    from airpose_amd import copenet_model
    net = copenet_model.getcopenet(MEAN_PARAMS, precision="bf16").eval()
    net.load_state_dict(sd_of("copenet"))
    a, b, c = net.parity_probe(1, seed=5), net.parity_probe(1, seed=5), net.parity_probe(1, seed=6)
    assert a["rel_err_by_slice"] == b["rel_err_by_slice"] and a["elementwise_err_by_slice"] == b["elementwise_err_by_slice"]
    assert a["rel_err_by_slice"] != c["rel_err_by_slice"]
    assert all(0 < v < float("inf") for v in a["rel_err_by_slice"].values())


@gpu
def test_entries_refuse_what_they_cannot_run(dev, heads):
    """the error codes the ABI already has: no kernel is launched on a refused call"""
    H, Hh, Hs = heads("copenet"), heads("hmr"), heads("singleview")
    z = torch.zeros(4, 2048, device=dev)
    p = _p(z)
    L = H.lib
    assert L.ap_regressor_step(H.h, p, p, p, p, p, 135, 1, p, p, H.st) != 0                     # partner_ld < 136
    assert L.ap_regressor_step_finish(H.h, p, p, p, p, 135, 1, p, p, H.st) != 0
    assert L.ap_regressor_step(H.h, p, p, p, p, None, 136, 1, p, p, H.st) != 0
    assert L.ap_regressor_feat_part(H.h, p, 0, p, H.st) != 0
    assert L.ap_regressor_fwd(H.h, p, p, p, p, p, p, None, 0, None, 0, None, 0, None, 0, 1, 0, p, p, p, p, H.st) != 0     # iters < 1
    assert L.ap_regressor_fwd(Hh.h, p, p, p, p, p, p, None, 0, None, 0, None, 0, None, 0, 1, 1, p, p, p, p, H.st) != 0    # hmr handle
    assert L.ap_regressor_fwd(Hs.h, p, p, p, p, p, p, None, 0, None, 0, None, 0, None, 0, 1, 1, p, p, p, p, H.st) != 0    # single-view handle
    assert L.ap_hmr_reg(H.h, p, 1, 1, None, 0, None, 0, None, 0, p, p, p, H.st) != 0
    assert L.ap_hmr_reg(Hh.h, p, 1, 0, None, 0, None, 0, None, 0, p, p, p, H.st) != 0
    assert L.ap_singleview_reg(H.h, p, p, p, None, 0, None, 0, 1, 1, p, p, H.st) != 0
    try:
        H.path("literal")
        assert L.ap_regressor_feat_part(H.h, p, 1, p, H.st) != 0                                # the halves need the folded map
    finally:
        H.restore()
    torch.cuda.synchronize()
    assert bool((z == 0).all())
