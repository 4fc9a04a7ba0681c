// The trunk schedule of libairpose_hip.so: the tile configuration of the generic kernels (dispatch_conv), the chip-fill rule
// (fills_chip), what runs each block of one depth-first pass (plan_pass: decisions only) and the loop that launches it through the
// launch functions of api_ops.hip (trunk_chunk), the concurrent passes of a call (trunk_passes, trunk_fwd) and the process-wide
// tuning knobs.
#include "api_internal.h"

unsigned long long* ap_internal::g_conv_dbg = nullptr;

namespace {
// Tuning knob of ap_set_conv_config, process-wide: ONE atomic word holding the raw value (-1 automatic, -4 automatic
// without the slab / lean kernels, -5 automatic without the lean kernel, 0..14 / 17 / 100 one explicit configuration);
// conv_mode() reads it, once per launch (dispatch_conv's three-argument form) or once per pass (trunk_chunk, which hands the value
// down), so handles on different threads never see a torn setting.
std::atomic<int> g_conv_mode{-1};
// ap_debug_set_range_hook: one host-mapped word for the process, allocated on first use and kept; g_ops_range is that word while
// the hook is on and NULL while it is off (one atomic pointer: a launch sees the old or the new value)
int* g_ops_word = nullptr;
std::atomic<int*> g_ops_range{nullptr};
}  // namespace

int* ap_internal::ops_range_word(int prec) {
    return prec == AP_PREC_F16 ? g_ops_range.load(std::memory_order_relaxed) : nullptr;
}

int ap_internal::conv_mode() { return g_conv_mode.load(std::memory_order_relaxed); }

namespace {
// choose the tile configuration: large tiles need enough tiles to fill 256 CUs (1 workgroup per CU)
int conv_config(const ConvArgs& a, int is_bf16 /* K_F32 / K_BF16 (16-bit) / K_SPLIT */, int mode /* conv_mode() */) {
    const bool use_slab = mode == -1 || mode == -5, use_lean = mode == -1;
    int cfg = mode < 0 ? -1 : mode;
    if (cfg < 0) {
        // Measured on MI355X at 512 images (tools/conv_bench.py): the 2-stage
        // LDS-DMA ring with 8 waves per 128-row tile wins on every trunk layer -- two workgroups (16 waves) per CU
        // run out of phase, so one tile's HBM-bound prologue/epilogue overlaps the other's MFMA loop:
        //   11  128x128 tile, waves 2(M) x 4(N)   C_out >= 128
        //   12  128x64  tile, waves 4(M) x 2(N)   C_out <= 64 (layer1 conv1/conv2)
        //   100 register-staged kernel, 64x64 tiles: problems too small to fill the chip with 128-row tiles
        //   grids below one workgroup per CU with 128x128 tiles (e.g. layer4 conv1/conv2 at 128 images: 196 tiles) take
        //   the 128x64 tiles (twice the workgroups; 46-48 us against 72-83 us for the register-staged kernel there)
        const long mt128 = (a.M + 127) / 128, nt128 = (a.Cout + 127) / 128, nt64 = (a.Cout + 63) / 64;
        //   (a folded downsample = second K segment needs the 128-wide tiles or the register-staged kernel)
        //   14  the same 128x128 tile with the nine taps of a stride-1 3x3 read from one LDS slab per channel chunk: every
        //       shape it can run, at EVERY size (it is the one kernel whose fp32 summation order differs from the others',
        //       so a size-dependent choice would make a pair's result depend on the batch it arrives in; measured equal or
        //       faster than the small-problem configurations from 2 to 512 images)
        //   17  pointwise layers with a short contraction and several channel tiles (conv3 of layer2-4, layer3.0 conv1: K <= 512,
        //       C_out >= 256)
        //       on three lean workgroups per CU (conv_lean.hip, bit-identical to 11): -4..6 % there, +20 % on K >= 1024
        if (use_slab && k_bf16::ap_conv_slab_supported(a, is_bf16)) cfg = 14;
        else if (use_lean && a.Cin <= 512 && a.Cout >= 256 && mt128 * nt128 >= 768 && k_bf16::ap_conv_lean_supported(a, is_bf16)) cfg = 17;
        else if (mt128 * nt128 >= 256) cfg = a.Cout <= 64 ? 12 : 11;
        else if (mt128 * nt64 >= 128) cfg = a.x2 ? (mt128 * nt128 >= 64 ? 11 : 100) : 12;
        else cfg = 100;
    }
    return cfg;
}
}  // namespace

// The forms dispatch_conv cannot run under the configuration `mode` selects, found WITHOUT a launch (NULL: it runs): one rule for
// the trunk pass and for the operator entries, which turn it into AP_ESHAPE with this text
const char* ap_internal::conv_refusal(const ConvArgs& a, int prec, int mode) {
    const int is_bf16 = prec_kind(prec), cfg = conv_config(a, is_bf16, mode);
    // the fragment-tiled output exists in the LDS-staged 16-bit epilogues only (trunk_chunk asks for it in the automatic modes)
    if (a.y_tiled && (is_bf16 != 1 || cfg == 17 || (cfg >= 4 && cfg <= 7) || (a.Cout & 7)))
        return "no fragment-tiled output in this precision / configuration (16-bit only; not 4-7, not 17, which the automatic choice takes for "
               "1 x 1 / stride 1 with Cin <= 512, Cout >= 256 on 768 or more 128 x 128 tiles)";
    // (the split-bf16 set ships the configurations the automatic choice uses: 11, 12, 100; 14 and 17 run 11)
    if (is_bf16 == K_SPLIT && cfg != 11 && cfg != 12 && cfg != 14 && cfg != 17 && cfg != 100) return "split-bf16 runs configurations 11, 12 and 100 only";
    if (a.x2 && cfg != 100) {
        // the 64-wide tiles of conv_pipe.hip carry no second K segment (14 and 17 hand such a call to 11)
        if (cfg == 2 || cfg == 3 || cfg == 6 || cfg == 7 || cfg == 9 || cfg == 12 || cfg == 13)
            return "no second K segment on the 64-wide tiles (2, 3, 6, 7, 9, 12, 13; the automatic choice takes 12 for Cout <= 64 on 256 or more "
                   "128-row tiles)";
        // ... and the ring kernel addresses x2 with 32-bit byte offsets
        if ((size_t)a.N * a.H2 * a.W2 * a.ldx2 * (is_bf16 == 1 ? 2 : 4) >= 0xffffffffull) return "second K segment of 4 GiB or more";
    }
    return nullptr;
}

hipError_t ap_internal::dispatch_conv(ConvArgs& a, int prec /* AP_PREC_* */, hipStream_t st, int mode /* conv_mode() */) {
    const int is_bf16 = prec_kind(prec);                     // storage kind inside the kernel set: K_F32 / K_BF16 (16-bit) / K_SPLIT
    const int cfg = conv_config(a, is_bf16, mode);
    if (conv_refusal(a, prec, mode)) return hipErrorInvalidValue;
    if (cfg == 100) return H16(prec, ap_launch_conv)(a, is_bf16, st);
    hipError_t e = ap_zero_line(&a.zero);
    if (e != hipSuccess) return e;
    a.dbg = g_conv_dbg;
    if (cfg == 17) {                                         // lean pointwise kernel; other shapes: the ring kernel's tile
        if (!k_bf16::ap_conv_lean_supported(a, is_bf16)) return H16(prec, ap_launch_conv_pipe)(a, is_bf16, 11, st);
        return H16(prec, ap_launch_conv_lean)(a, st);
    }
    if (cfg == 14) {
        // explicit 14 on a shape the slab kernel cannot run: the ring kernel's tile of the same shape
        if (!k_bf16::ap_conv_slab_supported(a, is_bf16)) return H16(prec, ap_launch_conv_pipe)(a, is_bf16, 11, st);
        return H16(prec, ap_launch_conv_slab)(a, st);
    }
    return H16(prec, ap_launch_conv_pipe)(a, is_bf16, cfg, st);
}

namespace {

// T units of work on a grid of at most G per round: does the launch fill the chip?  Whole rounds (the last one counted as whole)
// to num / den; a launch of less than one round to part_num / part_den of it (part_den 0: never)
bool fills_chip(long T, long G, int num, int den, int part_num, int part_den) {
    if (T < G) return part_den && T * part_den >= G * part_num;
    return T * den >= (T + G - 1) / G * G * num;
}

// What runs one block of a pass
enum : uint8_t { B_BNECK, B_IMG, B_CONVS };                  // form: fused layer1 bottleneck / image-resident layer3 block / separate convolutions
enum : uint8_t { C1_READY, C1_CONV, C1_PW };                 // conv1: the previous kernel produced it / generic kernels / conv_pw.hip
enum : uint8_t { C2_CONV, C2_PW, C2_IMG3, C2_S2P };          // conv2: generic / conv_pw.hip 3 x 3 / conv_img3.hip / conv_s2p.hip
// how the block ends: pair kernel / folded downsample on the generic kernels or conv_pw.hip / conv3 + average pool / conv3 +
// identity on the generic kernels or conv_pw.hip / downsample, then conv3
enum : uint8_t { E_PAIR, E_FOLD, E_FOLD_PW, E_POOL, E_C3, E_C3_PW, E_DS_C3 };
struct BlockPlan {
    uint8_t form, c1, c2, end;
    bool tail, y_even;                                       // B_BNECK: conv1 of the next block in the kernel; output at the even pixels only
    bool t2_tiled, res_tiled, out_tiled, out_even;           // layouts: t2 of the block; E_PAIR: the block input and output
};
constexpr size_t MAX_BLOCKS = 16;

// The schedule of one pass over n images, decisions only (no HIP call, no launch): knobs and packed streams of h, the CU count, the
// conv mode as read once for the pass, and whether a sibling pass shares the chip.
// Fragment-tiled intermediates (ap_common.h: ap_tiled_off): a tensor whose ONLY reader is the fused pair kernel is stored
// as [M/16][C/8][16 pixels][8 channels], the order the pair kernel's lanes fetch it in -- t2 of every pair block, and a
// pair block's output when the next block is an identity pair block that also got its conv1 from this kernel.  Same
// values, same arithmetic: the features are bit-identical with the layout off (ap_net_set_tiled).
void plan_pass(const ap_net* h, int n, int cus, int mode, bool shared, BlockPlan* plan) {
    const bool bf = h->half(), automatic = mode == -1;       // bf gates the fused kernels of the 16-bit throughput modes
    const bool tiling = bf && h->tiled && mode < 0;
    // conv_pw.hip: automatic rule = conv1 only (layer4 at 512 images: 156 / 70 / 71 -> 136 / 60 / 61 us; whole bench +1.0 % single
    // pass, +0.6 % with two concurrent passes).  conv3 + identity (2: forced) is 3-9 us slower than the lean kernel and, beside a
    // concurrent pass, turns the gain into -0.5 %: a one-wave-per-SIMD kernel keeps the other pass's workgroups off its CUs.
    // Same bits as the generic kernels, so the choice may depend on the problem size: its 196-pixel x 256-channel tiles fill whole
    // rounds of the chip to 80 % or (part) half a round at least; 2 / 3 force it
    const int pw = h->pw_conv;
    auto pw_fills = [&](long M, int cout, bool part) {
        const int NN = cout >> 8, gmax = k_bf16::ap_conv_pw_grid(1L << 40, cout, cus);
        return pw == 2 || pw == 3 || fills_chip(((M / 196 + 7) & ~7L) * NN, gmax, 4, 5, 1, part ? 2 : 0);
    };
    auto pw_1x1 = [&](const Layer& L, long M) {
        return pw && L.pw.p && bf && L.k == 1 && L.stride == 1 && automatic && k_bf16::ap_conv_pw_supported(M, L.cin, L.cout) &&
               pw_fills(M, L.cout, true);
    };
    // an image (half an image) per CU: 256 (512) images = one (two) full rounds; 300 = two rounds 59 % full
    const bool img_fit = h->img_block == 2 || (h->img_block == 1 && fills_chip(n, cus, 7, 8, 7, 8));
    const bool img3_fit = h->img3 == 2 || (h->img3 == 1 && fills_chip(2L * n, cus, 7, 8, 7, 8));
    auto is_pair = [&](const ap_net::Block& X) {
        return bf && h->fuse_pair && X.pair_p && &X != &h->blocks.back() && (!X.has_down || h->fuse_ds);
    };
    bool t1_ready = false, cur_tiled = false;                // ws_t1 already holds this block's conv1 output; layout of the block input
    int H = 56;
    for (size_t i = 0; i < h->blocks.size(); ++i) {
        const ap_net::Block& B = h->blocks[i];
        const ap_net::Block* Nx = i + 1 < h->blocks.size() ? &B + 1 : nullptr;
        BlockPlan& p = plan[i] = BlockPlan{};
        const int Ho = (H + 2 - 3) / B.c2.stride + 1;
        if (bf && h->fuse_block && B.c2.cout == 64 && B.c2.stride == 1 && H % 14 == 0 && (!B.has_down || B.c1.cin == 64)) {
            // layer1: conv1 -> conv2 -> conv3 (+identity | folded downsample) in one kernel, intermediates in LDS.
            // last block of layer1: conv1 of layer2.0 (model_copenet.py:29-31) on the block output while it is in registers; what
            // is left to read of that output is layer2.0's stride-2 downsample branch (:41-42, :97-102) -> even pixels only
            p.form = B_BNECK;
            p.tail = h->fuse_tail && !B.has_down && Nx && Nx->has_down && Nx->c1.cin == 256 && Nx->c1.cout == 128 &&
                     Nx->c2.stride == 2 && Nx->down.stride == 2 && mode < 0;
            p.y_even = p.tail && h->even_out;
            t1_ready = p.tail;
            continue;
        }
        if (bf && img_fit && B.imgw.p && H == 14 && !t1_ready && !cur_tiled && automatic) {
            p.form = B_IMG;                                  // layer3 identity block: one kernel, an image per workgroup, t1 / t2 in LDS
            continue;
        }
        p.form = B_CONVS;
        p.c1 = t1_ready ? C1_READY : pw_1x1(B.c1, (long)n * H * H) ? C1_PW : C1_CONV;
        const bool pair = is_pair(B);
        // conv2 of layer2.0 on the polyphase kernel (conv_s2p.hip; ap_net_set_s2p, off by default): its K order is its own, so when on it
        // takes the layer at EVERY batch size.
        // conv2 of a stage's first block (model_copenet.py:32-34, :18) on conv_pw.hip (nine taps): it writes NHWC rows, so t2 stays
        // untiled for that block's pair kernel.  Automatic rule: only for a pass that has the chip to itself (l4.0.c2 164 -> 149 us,
        // l3.0.c2 168 -> 157: +0.55 % of the whole bench there, -0.45 % beside a concurrent pass, whose workgroups a one-wave-per-SIMD
        // kernel keeps off its CUs)
        const Layer& L2 = B.c2;
        if (bf && h->s2p && B.c2s2.p && H == 56 && L2.stride == 2 && automatic) p.c2 = C2_S2P;
        else if (pw && pw != 4 && !(pw == 1 && shared) && automatic && bf && L2.pw.p && L2.k == 3 && L2.stride == 2 && L2.pad == 1 &&
                 conv_pw_k3_fits(L2.desc(true), n, H) && pw_fills((long)n * (H / 2) * (H / 2), L2.cout, true))
            p.c2 = C2_PW;
        else if (bf && img3_fit && B.c2img.p && H == 28 && L2.stride == 1 && automatic) p.c2 = C2_IMG3;
        p.t2_tiled = pair && tiling && p.c2 != C2_PW;
        t1_ready = false;
        if (pair) {
            // conv3 (+ identity | + folded downsample, ReLU) AND -- where the pair carries it -- the next block's conv1 in one
            // kernel: the block output is written once and not read back for conv1 (model_copenet.py:38-45 of this block,
            // :29-31 of the next)
            p.end = E_PAIR;
            p.res_tiled = cur_tiled;
            cur_tiled = p.out_tiled = p.t2_tiled && B.pair_n1 > 0 && is_pair(*Nx) && !Nx->has_down;
            // the next block is a stage's first one and got its conv1 from this kernel: all that is read of `out` is that block's
            // stride-2 downsample branch (model_copenet.py:41-42, :97-102) -- the even pixels
            p.out_even = h->even_out && !p.out_tiled && B.pair_n1 > 0 && Nx->has_down && Nx->down.stride == 2 && Nx->c2.stride == 2;
            t1_ready = B.pair_n1 > 0;
        } else if (B.has_down && h->fuse_ds) {
            // (conv_pw.hip, whole rounds only: at half a round -- 64 pairs -- the generic kernel beside the other pass is faster: -0.8 % of that bench)
            const Layer& L = B.c3ds;
            p.end = pw && L.pw.p && bf && automatic && conv_pw_ds_fits(L.desc(true), n, Ho, H) && pw_fills((long)n * Ho * Ho, L.cout, false)
                        ? E_FOLD_PW : E_FOLD;
        } else if (bf && h->fuse_pool && !Nx && !B.has_down && Ho == 7 && automatic) {
            p.end = E_POOL;                                  // last convolution of the trunk, with AvgPool2d(7) + view in its epilogue
        } else {
            // (conv3 + identity on conv_pw.hip: 89-95 us against the lean kernel's 86: only when forced)
            p.end = B.has_down ? E_DS_C3 : pw == 2 && pw_1x1(B.c3, (long)n * Ho * Ho) ? E_C3_PW : E_C3;
        }
        H = Ho;
    }
}

// workspace of one pass over n images (a grow may synchronise the device and free: never while a sibling pass is in flight)
int reserve_trunk_ws(ap_net* h, ap_net::TrunkWs& w, int n) {
    const bool bf = h->half();
    const size_t es = h->esize();
    if (!(h->fuse_stem && (bf || h->prec == AP_PREC_BF16X2))) HIP_TRY(w.ws_stem.reserve((size_t)n * 112 * 112 * 64 * es));
    HIP_TRY(w.ws_a.reserve((size_t)n * 802816 * es));
    HIP_TRY(w.ws_b.reserve((size_t)n * 802816 * es));
    HIP_TRY(w.ws_ds.reserve((size_t)n * 802816 * es));
    HIP_TRY(w.ws_t1.reserve((size_t)n * 401408 * es));
    HIP_TRY(w.ws_t2.reserve((size_t)n * 200704 * es));
    return AP_OK;
}

// one depth-first pass over n = n0 + n1 images: the first n0 from x0, the rest from x1 (two views, one pass).  shared: a sibling
// pass runs beside this one.  The loop walks the plan: it owns the buffers and their swaps, the timing marks and ev_skew
int trunk_chunk(ap_net* h, ap_net::TrunkWs& w, const float* x0, int n0, const float* x1, int n1, float* feat, hipStream_t st,
                bool shared, size_t* ev_out = nullptr, int signal_at = 0) {
    const int bf = h->half();
    const int prec = h->prec;                                // selects the kernel set (H16) and, as prec_kind, the storage kind
    const int n = n0 + n1;
    const int mode = conv_mode();                            // ONE schedule for the whole pass, whatever a setter does meanwhile
    int dev = 0, cus = 0;
    HIP_TRY(ap_device(&dev, &cus));
    if (h->blocks.size() > MAX_BLOCKS) return fail(AP_ESTATE, "trunk: more bottleneck blocks than a pass plans");
    BlockPlan plan[MAX_BLOCKS];
    plan_pass(h, n, cus, mode, shared, plan);
    { int rc0 = reserve_trunk_ws(h, w, n); if (rc0) return rc0; }
    size_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
    if (h->tm.on == 1) HIP_TRY(h->tm.rec(st, &e0));
    const bool stem_pools = h->fuse_stem && (bf || prec == AP_PREC_BF16X2);
    HIP_TRY(launch_stem(prec, !stem_pools ? 0 : !bf || h->fuse_stem == 2 ? 1 : 2, x0, x1, n0, n, prec == AP_PREC_FP32 ? h->stem_w.p : h->stem_wpk.p,
                        h->stem_wpk_lo.p, h->stem_scale.as<float>(), h->stem_shift.as<float>(), stem_pools ? w.ws_a.p : w.ws_stem.p, w.rflag, st));
    if (!stem_pools) HIP_TRY(launch_maxpool(w.ws_stem.p, w.ws_a.p, n, prec, w.rflag, st));
    if (h->tm.on) HIP_TRY(h->tm.rec(st, &e1));
    if (signal_at == 1) HIP_TRY(hipEventRecord(h->ev_skew, st));
    void *cur = w.ws_a.p, *nxt = w.ws_b.p, *t1 = w.ws_t1.p, *t2 = w.ws_t2.p;
    int H = 56;
    bool cur_tiled = false;                                  // layout of `cur`
    bool pooled = false;                                     // the last convolution wrote the pooled features itself
#define LAUNCH(expr) do { HIP_TRY(expr); ++h->conv_launches; } while (0)   /* a launch of the conv stack: counted where it is issued */
    // a convolution + BN (+ residual) (+ ReLU) on the generic kernels
    auto conv = [&](const Layer& L, const void* x, int Hin, const void* res, void* y, int relu, int y_tiled) {
        return launch_conv(L.desc(), x, n, Hin, Hin, res, y, relu, y_tiled, nullptr, 0, nullptr, nullptr, prec, mode, w.rflag, st);
    };
    for (size_t i = 0; i < h->blocks.size(); ++i) {
        const ap_net::Block& B = h->blocks[i];
        const BlockPlan& p = plan[i];
        if (signal_at >= 2 && (int)i == signal_at - 2) HIP_TRY(hipEventRecord(h->ev_skew, st));
        const int Ho = (H + 2 - 3) / B.c2.stride + 1;
        const Layer& L3 = B.has_down ? B.c3ds : B.c3;
        if (p.form == B_BNECK) {
            const Layer* c1n = p.tail ? &h->blocks[i + 1].c1 : nullptr;
            if (B.c1.cin != (B.has_down ? 64 : 256) || (c1n && (c1n->k != 1 || c1n->stride != 1)))
                return fail(AP_ESHAPE, "fused layer1 bottleneck: C_in 256 (identity) or 64 (first block); next conv1: 1x1, 256 -> 128");
            const ConvDesc d1n = c1n ? c1n->desc() : ConvDesc{};
            LAUNCH(launch_bneck2(B.c1.desc(), B.c2.desc(), L3.desc(), B.has_down, cur, nxt, n, H, H, c1n ? &d1n : nullptr, t1, p.y_even, prec, w.rflag, st));
            std::swap(cur, nxt);
            continue;
        }
        if (p.form == B_IMG) {
            LAUNCH(launch_block_img(cur, B.imgw.p, B.c1.scale.as<float>(), B.c1.shift.as<float>(), B.c2.scale.as<float>(), B.c2.shift.as<float>(),
                                    B.c3.scale.as<float>(), B.c3.shift.as<float>(), nxt, n, prec, w.rflag, st));
            std::swap(cur, nxt);
            continue;
        }
        if (p.c1 != C1_READY && cur_tiled) return fail(AP_ESTATE, "trunk: conv1 of a block would read a tiled block output");
        if (p.c1 == C1_PW) LAUNCH(launch_conv_pw(B.c1.desc(true), cur, nullptr, t1, n * H * H, prec, w.rflag, st));
        else if (p.c1 == C1_CONV) LAUNCH(conv(B.c1, cur, H, nullptr, t1, 1, 0));
        const float *s2 = B.c2.scale.as<float>(), *h2 = B.c2.shift.as<float>();
        if (p.c2 == C2_S2P) LAUNCH(launch_conv_s2p(t1, B.c2s2.p, s2, h2, t2, n, p.t2_tiled, prec, w.rflag, st));
        else if (p.c2 == C2_IMG3) LAUNCH(launch_conv_img3(t1, B.c2img.p, s2, h2, t2, n, p.t2_tiled, prec, w.rflag, st));
        else if (p.c2 == C2_PW) LAUNCH(launch_conv_pw_k3(B.c2.desc(true), t1, t2, n, H, prec, w.rflag, st));
        else LAUNCH(conv(B.c2, t1, H, nullptr, t2, 1, p.t2_tiled));
        if (p.end == E_PAIR) {
            const ap_net::Block& Nx = h->blocks[i + 1];
            LAUNCH(launch_conv_pair(t2, B.pair.p, L3.scale.as<float>(), L3.shift.as<float>(), Nx.c1.scale.as<float>(), Nx.c1.shift.as<float>(), cur,
                                    nxt, t1, n * Ho * Ho, Ho, B.has_down ? H : 0, L3.stride2, B.pair_p, B.pair_p2, B.pair_n1,
                                    PairLayout{p.t2_tiled, p.res_tiled, p.out_tiled, p.out_even}, prec, w.rflag, st));
            cur_tiled = p.out_tiled;
        } else if (cur_tiled) {                               // (cannot happen: out_tiled is only set when the next block is a pair block)
            return fail(AP_ESTATE, "trunk: a tiled block output reached a kernel that reads NHWC");
        } else if (p.end == E_FOLD_PW) {
            LAUNCH(launch_conv_pw_ds(L3.desc(true), t2, cur, nxt, n, Ho, H, prec, w.rflag, st));
        } else if (p.end == E_FOLD) {
            LAUNCH(launch_conv(L3.desc(), t2, n, Ho, Ho, nullptr, nxt, 1, 0, cur, H, nullptr, nullptr, prec, mode, w.rflag, st));
        } else if (p.end == E_POOL) {
            // conv3 + bn3 + identity + ReLU AND AvgPool2d(7) + view in one kernel (model_copenet.py:38-47 of layer4.2, then :173-175);
            // the block output is never written
            LAUNCH(launch_conv(B.c3.desc(), t2, n, Ho, Ho, cur, nxt, 1, 0, nullptr, 0, feat, &pooled, prec, mode, w.rflag, st));
        } else if (p.end == E_C3_PW) {
            LAUNCH(launch_conv_pw(B.c3.desc(true), t2, cur, nxt, n * Ho * Ho, prec, w.rflag, st));
        } else {
            if (p.end == E_DS_C3) LAUNCH(conv(B.down, cur, H, nullptr, w.ws_ds.p, 0, 0));
            LAUNCH(conv(B.c3, t2, Ho, p.end == E_DS_C3 ? w.ws_ds.p : cur, nxt, 1, 0));
        }
        std::swap(cur, nxt);
        H = Ho;
    }
#undef LAUNCH
    if (h->tm.on) HIP_TRY(h->tm.rec(st, &e2));
    if (!pooled) HIP_TRY(launch_avgpool(cur, feat, n, 2048, prec, w.rflag, st));
    if (h->tm.on == 1) HIP_TRY(h->tm.rec(st, &e3));
    if (ev_out) {                                            // the caller combines the events of two concurrent passes
        ev_out[0] = e0; ev_out[1] = e1; ev_out[2] = e2; ev_out[3] = e3;
        return AP_OK;
    }
    if (h->tm.on) { h->tm.marks[1].push_back(e1); h->tm.marks[1].push_back(e2); }
    if (h->tm.on == 1) {
        h->tm.marks[0].push_back(e0); h->tm.marks[0].push_back(e1);
        h->tm.marks[2].push_back(e2); h->tm.marks[2].push_back(e3);
    }
    return AP_OK;
}

// trunk over the concatenation [x0 (n0 images) | x1 (n1 images)]; feat rows follow the same order
int trunk_passes(ap_net* h, const float* x0, int n0, const float* x1, int n1, float* feat, hipStream_t st, hipStream_t st_out) {
    const int n_img = n0 + n1;
    h->conv_launches = 0;
    const int chunk = h->chunk > 0 ? h->chunk : 512;
    const size_t IMG_ELEMS = (size_t)3 * 224 * 224;
    if (h->dual_stream && !n1 && n0 >= 128) {                // one list of images (forward_feat_ext, the single-view heads): its two
        n1 = n0 - n0 / 2;                                    // halves as the two concurrent passes (feature rows stay in list order)
        n0 = n0 / 2;
        x1 = x0 + (size_t)n0 * IMG_ELEMS;
    }
    // (measured: +4..5 % at 64 images per view, -4 % at 32, where the launches no longer fill the chip)
    if (h->dual_stream && n0 >= 64 && n1 >= 64 && chunk >= 128) {
        // two views = two concurrent passes: fork from the caller's stream, one pass per internal stream, join.  A view of more
        // than chunk / 2 images goes through its stream in slices of chunk / 2 (same workspace, stream order), so 2 x 256 images
        // are in flight whatever the batch
        if (!h->aux[0]) {
            for (int i = 0; i < 4; ++i) {
                HIP_TRY(hipStreamCreateWithFlags(&h->aux[i], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
            }
            HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&h->ev_skew, hipEventDisableTiming));
        }
        const int ppv = h->passes_per_view == 2 ? 2 : 1, np = 2 * ppv;
        const int per = chunk / 2 / ppv;                     // images of one slice of one pass
        auto part_of = [&](int q, int* lo, int* cnt) {       // pass q's share of its view
            const int v = q / ppv, part = q % ppv, nv = v ? n1 : n0;
            *lo = part * (nv / ppv);
            *cnt = part == ppv - 1 ? nv - *lo : nv / ppv;
        };
        // every pass's workspace is sized BEFORE the fork: a grow inside a pass would synchronise the device and free
        // buffers while the sibling pass is in flight
        int rounds = 1;
        for (int q = 0; q < np; ++q) {
            int lo, cnt;
            part_of(q, &lo, &cnt);
            int rc = reserve_trunk_ws(h, h->tw[q], std::min(cnt, per));
            if (rc) return rc;
            rounds = std::max(rounds, (cnt + per - 1) / per);
        }
        HIP_TRY(hipEventRecord(h->ev_fork, st));
        std::vector<size_t> ev((size_t)np * rounds * 4, 0);
        int rc = AP_OK, forked = 0;
        for (int q = 0; q < np && !rc; ++q) {
            const int v = q / ppv;
            int lo, cnt;
            part_of(q, &lo, &cnt);
            HIP_TRY(hipStreamWaitEvent(h->aux[q], h->ev_fork, 0));
            forked = q + 1;
            if (q == 1 && np == 2 && h->dual_skew) HIP_TRY(hipStreamWaitEvent(h->aux[1], h->ev_skew, 0));
            const int nr = (cnt + per - 1) / per;            // slices of equal size (+-1): 261 images = 131 + 130, not 256 + 5
            for (int r = 0, s0 = 0, c = 0; r < nr && !rc; ++r, s0 += c) {
                c = cnt / nr + (r < cnt % nr ? 1 : 0);
                const float* xv = (v ? x1 : x0) + (size_t)(lo + s0) * IMG_ELEMS;
                rc = trunk_chunk(h, h->tw[q], xv, c, nullptr, 0, feat + ((v ? (size_t)n0 : 0) + lo + s0) * 2048, h->aux[q],
                                 true, &ev[((size_t)q * rounds + r) * 4], (q == 0 && np == 2 && r == 0) ? h->dual_skew : 0);
            }
        }
        // ap_net_range_mark_next: each pass stream snapshots ITS range word behind its last kernel of this call
        const int mslot = h->mark_slot;
        h->mark_slot = -1;
        if (mslot >= 0 && h->range_flag)
            for (int q = 0; q < forked; ++q) HIP_TRY(ap_launch_word_copy(h->range_flag + q, h->range_slots + 4 * mslot + q, h->aux[q]));
        // join every stream that forked, also after a failed launch: later calls reuse tw[q] on the caller's stream order
        for (int q = 0; q < forked; ++q) {
            HIP_TRY(hipEventRecord(h->ev_join[q], h->aux[q]));
            HIP_TRY(hipStreamWaitEvent(st_out, h->ev_join[q], 0));
            if (st_out != st) h->unjoined = true;            // st itself is not behind these passes
        }
        if (rc) return rc;
        if (h->tm.on) {
            // per slice round: span over the first and the last pass issued (two streams: exact); a pass without a slice in this
            // round (views of different sizes) lends the other pass's events
            auto quad = [&](int stage, int a, int b) {
                for (int r = 0; r < rounds; ++r)
                    for (int q : {0, np - 1}) {
                        const size_t* e = &ev[((size_t)q * rounds + r) * 4];
                        if (!e[b]) e = &ev[((size_t)(np - 1 - q) * rounds + r) * 4];
                        h->tm.quads[stage].push_back(e[a]);
                        h->tm.quads[stage].push_back(e[b]);
                        if (q == 0) h->tm.qfree[stage].push_back(st_out != st);
                    }
            };
            quad(1, 1, 2);
            if (h->tm.on == 1) { quad(0, 0, 1); quad(2, 2, 3); }
            h->tm.passes++;
        }
        return AP_OK;
    }
    if (h->unjoined) {                                       // an asynchronous two-pass call came before: its passes may still use tw[0]
        for (int q = 0; q < 4; ++q) HIP_TRY(hipStreamWaitEvent(st_out, h->ev_join[q], 0));
        h->unjoined = false;
    }
    if (st_out != st) {                                      // one pass: it runs on st_out, behind the inputs
        if (!h->ev_in) HIP_TRY(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->ev_in, st));
        HIP_TRY(hipStreamWaitEvent(st_out, h->ev_in, 0));
        st = st_out;
    }
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int i1 = std::min(n_img, i0 + chunk);
        const int a0 = std::min(i0, n0), a1 = std::min(i1, n0);          // part taken from x0
        const int b0 = std::max(i0, n0) - n0, b1 = std::max(i1, n0) - n0; // part taken from x1
        int rc = trunk_chunk(h, h->tw[0], x0 + a0 * IMG_ELEMS, a1 - a0, x1 ? x1 + b0 * IMG_ELEMS : nullptr, b1 - b0,
                             feat + (size_t)i0 * 2048, st, false);
        if (rc) return rc;
    }
    if (h->mark_slot >= 0 && h->range_flag) HIP_TRY(ap_launch_word_copy(h->range_flag, h->range_slots + 4 * h->mark_slot, st));
    h->mark_slot = -1;
    if (h->tm.on) h->tm.passes++;
    return AP_OK;
}

}  // namespace

// st: the stream the inputs are ordered on; st_out (default: st): the stream the features are ordered on.  With two streams
// (ap_trunk_fwd_twoview_async) st is never made to wait for the passes: the next call's passes queue behind this call's on the
// internal streams and the caller's stream stays free
int ap_internal::trunk_fwd(ap_net* h, const float* x0, int n0, const float* x1, int n1, float* feat, hipStream_t st, hipStream_t st_out) {
    if (!st_out) st_out = st;
    if (!h->finalized) return fail(AP_ESTATE, "ap_net_finalize has not been called");
    if (n0 <= 0 || n1 < 0 || !x0 || (n1 && !x1) || !feat) return fail(AP_EINVAL, "ap_trunk_fwd: bad arguments");
    if (h->range_mode && h->range_any())
        return fail(AP_ERANGE, "AP_PREC_F16: an earlier trunk pass of this handle produced non-finite features (a stored activation left "
                               "the fp16 range); clear with ap_net_range_status(h, stream, 1) and use AP_PREC_BF16 for this checkpoint");
    int rc_pass = trunk_passes(h, x0, n0, x1, n1, feat, st, st_out);
    if (rc_pass) return rc_pass;
    if (h->range_flag && h->range_mode == 2) {
        HIP_TRY(hipStreamSynchronize(st_out));
        if (h->range_any())
            return fail(AP_ERANGE, "AP_PREC_F16: non-finite trunk features (a stored activation left the fp16 range); use AP_PREC_BF16 "
                                   "for this checkpoint");
    }
    return AP_OK;
}

extern "C" {

int ap_net_last_conv_launches(const ap_net* h) { return h ? h->conv_launches : AP_EINVAL; }

int ap_trunk_fwd(ap_net* h, const float* x_nchw, int n_img, float* feat, void* stream) {
    if (!h) return fail(AP_EINVAL, "null handle");
    return trunk_fwd(h, x_nchw, n_img, nullptr, 0, feat, (hipStream_t)stream);
}

int ap_trunk_fwd_twoview(ap_net* h, const float* x0, const float* x1, int B, float* feat, void* stream) {
    if (!h || !x0 || !x1 || !feat) return fail(AP_EINVAL, "ap_trunk_fwd_twoview: null argument");
    if (B <= 0) return fail(AP_EINVAL, "ap_trunk_fwd_twoview: bad batch");
    return trunk_fwd(h, x0, B, x1, B, feat, (hipStream_t)stream);
}

int ap_trunk_fwd_twoview_async(ap_net* h, const float* x0, const float* x1, int B, float* feat, void* in_stream, void* out_stream) {
    if (!h || !x0 || !x1 || !feat) return fail(AP_EINVAL, "ap_trunk_fwd_twoview_async: null argument");
    if (B <= 0) return fail(AP_EINVAL, "ap_trunk_fwd_twoview_async: bad batch");
    return trunk_fwd(h, x0, B, x1, B, feat, (hipStream_t)in_stream, (hipStream_t)out_stream);
}

int ap_debug_set_trace(void* device_buf_160_u64) {
    g_conv_dbg = (unsigned long long*)device_buf_160_u64;
    return AP_OK;
}

int ap_debug_set_range_hook(int on) {
    if (!on) {
        g_ops_range.store(nullptr, std::memory_order_relaxed);
        return AP_OK;
    }
    if (!g_ops_word) {
        HIP_TRY(hipHostMalloc((void**)&g_ops_word, sizeof(int), hipHostMallocMapped | hipHostMallocPortable));
    }
    __atomic_store_n(g_ops_word, 0, __ATOMIC_RELAXED);
    g_ops_range.store(g_ops_word, std::memory_order_relaxed);
    return AP_OK;
}

int ap_debug_range_status(int precision, void* stream, int reset) {
    if (!prec_valid(precision)) return fail(AP_EINVAL, "ap_debug_range_status: bad precision");
    int* word = ops_range_word(precision);
    if (!word) return AP_OK;                                 // hook off, or a precision without a range to leave
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const int v = __atomic_load_n(word, __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(word, 0, __ATOMIC_RELAXED);
    return v ? AP_ERANGE : AP_OK;
}

int ap_set_conv_config(int cfg) {
    if (cfg != -1 && cfg != -4 && cfg != -5 && cfg != 100 && (cfg < 0 || cfg > 14) && cfg != 17)
        return fail(AP_EINVAL, "ap_set_conv_config: -1, -4, -5, 0..14, 17 or 100");
    g_conv_mode.store(cfg, std::memory_order_relaxed);
    return AP_OK;
}

}  // extern "C"
