// The trunk schedule of libairpose_hip.so: which kernel runs each convolution (dispatch_conv, run_*), one depth-first pass
// (trunk_chunk), the concurrent passes of a call (trunk_passes, trunk_fwd) and the process-wide tuning knobs.
#include "api_internal.h"

unsigned long long* ap_internal::g_conv_dbg = nullptr;

namespace {
// Tuning knob of ap_set_conv_config, process-wide: ONE atomic word holding the raw value (-1 automatic, -4 automatic
// without the slab / lean kernels, -5 automatic without the lean kernel, 0..14 / 17 / 100 one explicit configuration);
// dispatch_conv reads it once per launch and decodes it (trunk_chunk: once per pass), so handles on different threads never see a
// torn setting.
std::atomic<int> g_conv_mode{-1};
void* g_zero[16] = {nullptr};   // per-device 256-byte zero line
// ap_debug_set_range_hook: one host-mapped word for the process, allocated on first use and kept; g_ops_range is that word while
// the hook is on and NULL while it is off (one atomic pointer: a launch sees the old or the new value)
int* g_ops_word = nullptr;
std::atomic<int*> g_ops_range{nullptr};
}  // namespace

int* ap_internal::ops_range_word(int prec) {
    return prec == AP_PREC_F16 ? g_ops_range.load(std::memory_order_relaxed) : nullptr;
}

hipError_t ap_internal::zero_line(const void** out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    if (!g_zero[dev]) {
        e = hipMalloc(&g_zero[dev], 256);
        if (e != hipSuccess) return e;
        e = hipMemset(g_zero[dev], 0, 256);
        if (e != hipSuccess) return e;
    }
    *out = g_zero[dev];
    return hipSuccess;
}

hipError_t ap_internal::device_cus(int* n) {
    static int cus[AP_MAX_DEVICES] = {};
    int dev = 0;
    hipError_t e = ap_current_device(&dev);
    if (e != hipSuccess) return e;
    if (!cus[dev]) {
        e = hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
    }
    *n = cus[dev];
    return hipSuccess;
}

// choose the tile configuration: large tiles need enough tiles to fill 256 CUs (1 workgroup per CU)
hipError_t ap_internal::dispatch_conv(ConvArgs& a, int prec /* AP_PREC_* */, hipStream_t st) {
    const int is_bf16 = prec_kind(prec);                     // storage kind inside the kernel set: K_F32 / K_BF16 (16-bit) / K_SPLIT
    const int mode = g_conv_mode.load(std::memory_order_relaxed);
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
    // the fragment-tiled output exists in the LDS-staged 16-bit epilogues only (trunk_chunk asks for it in the automatic modes)
    if (a.y_tiled && (is_bf16 != 1 || cfg == 17 || (cfg >= 4 && cfg <= 7) || (a.Cout & 7))) return hipErrorInvalidValue;
    if (cfg == 100) return H16(prec, ap_launch_conv)(a, is_bf16, st);
    hipError_t e = zero_line(&a.zero);
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

// pw: 0 = the generic kernels; 1 / 2 / 3 = conv_pw.hip where the layer has a stream and the shape fits (1: only when its tiles fill
// half the chip, or whole rounds of it to 80 %) -- same bits either way, so the choice may depend on the problem size
// the size rule of conv_pw.hip's automatic choice: its 196-pixel x 256-channel tiles fill half a round of the chip at least, or whole rounds to 80 %
bool pw_fills(long M, int cout, int pw, int* err) {
    int cus = 0;
    if ((*err = device_cus(&cus)) != hipSuccess) return false;
    const int NN = cout >> 8, gmax = k_bf16::ap_conv_pw_grid(1L << 40, cout, cus);
    const long T = ((M / 196 + 7) & ~7L) * NN, rounds = (T + gmax - 1) / gmax;
    return pw == 2 || pw == 3 || (T <= gmax ? T * 2 >= gmax : T * 5 >= rounds * gmax * 4);
}
// the 3 x 3 / stride-2 convolution of a stage's first block (model_copenet.py:32-34, :18) as nine pointwise taps of conv_pw.hip?
bool pw_k3_args(const Layer& L, int N, int H, int W, int prec, PwArgs* p) {
    if (!L.pw.p || !prec_half(prec) || L.k != 3 || L.stride != 2 || L.pad != 1 || (H & 1) || (W & 1)) return false;
    *p = PwArgs{};
    p->k3 = 1; p->Ho = H / 2; p->Wo = W / 2; p->H2 = H; p->W2 = W; p->stride2 = 2;
    p->M = N * p->Ho * p->Wo; p->Cin = L.cin; p->Cout = L.cout; p->relu = 1;
    p->wfrag = L.pw.p; p->scale = L.scale.as<float>(); p->shift = L.shift.as<float>();
    return k_bf16::ap_conv_pw_k3_supported(*p);
}

int run_conv(const Layer& L, const void* x, int N, int H, int W, void* y, const void* res, int relu, int prec,
             hipStream_t st, int* rflag = nullptr, int y_tiled = 0, int pw = 0) {
    if (pw && L.pw.p && prec_half(prec) && relu && !y_tiled && L.k == 1 && L.stride == 1 &&
        g_conv_mode.load(std::memory_order_relaxed) == -1 && k_bf16::ap_conv_pw_supported((long)N * H * W, L.cin, L.cout)) {
        const long M = (long)N * H * W;
        int err = 0;
        const bool fills = pw_fills(M, L.cout, pw, &err);
        HIP_TRY((hipError_t)err);
        if (fills) {
            PwArgs p{};
            p.x = x; p.y = y; p.res = res; p.wfrag = L.pw.p; p.scale = L.scale.as<float>(); p.shift = L.shift.as<float>();
            p.M = (int)M; p.Cin = L.cin; p.Cout = L.cout; p.relu = 1; p.range_flag = rflag;
            HIP_TRY(H16(prec, ap_launch_conv_pw)(p, st));
            return AP_OK;
        }
    }
    PwArgs p3;
    if (pw && relu && !res && !y_tiled && g_conv_mode.load(std::memory_order_relaxed) == -1 && pw_k3_args(L, N, H, W, prec, &p3)) {
        int err = 0;
        const bool fills = pw_fills(p3.M, L.cout, pw, &err);
        HIP_TRY((hipError_t)err);
        if (fills) {
            p3.x = x; p3.y = y; p3.range_flag = rflag;
            HIP_TRY(H16(prec, ap_launch_conv_pw)(p3, st));
            return AP_OK;
        }
    }
    ConvArgs a{};
    a.range_flag = rflag;
    a.y_tiled = y_tiled;
    a.x = x; a.w = L.w.p; a.scale = L.scale.as<float>(); a.shift = L.shift.as<float>(); a.res = res; a.y = y;
    a.N = N; a.H = H; a.W = W; a.Cin = L.cin;
    a.Ho = (H + 2 * L.pad - L.k) / L.stride + 1;
    a.Wo = (W + 2 * L.pad - L.k) / L.stride + 1;
    a.Cout = L.cout;
    a.KH = a.KW = L.k; a.stride = L.stride; a.pad = L.pad;
    a.M = N * a.Ho * a.Wo;
    a.ldx = L.cin; a.ldy = L.cout; a.ldr = L.cout; a.wld = L.wld;
    a.relu = relu;
    HIP_TRY(dispatch_conv(a, prec, st));
    return AP_OK;
}

// fused conv3 + downsample of a stage's first block: t [N][Ho][Ho][cin] (pointwise) and x [N][Hin][Hin][cin2]
// sampled with stride2, concatenated along K
int run_c3_ds(const Layer& L, const void* t, const void* x, int N, int Ho, int Hin, void* y, int prec,
              hipStream_t st, int* rflag = nullptr, int pw = 0) {
    if (pw && L.pw.p && prec_half(prec) && g_conv_mode.load(std::memory_order_relaxed) == -1) {       // conv_pw.hip, as in run_conv
        PwArgs p{};
        p.x = t; p.y = y; p.wfrag = L.pw.p; p.scale = L.scale.as<float>(); p.shift = L.shift.as<float>();
        p.M = N * Ho * Ho; p.Cin = L.cin; p.Cout = L.cout; p.relu = 1; p.range_flag = rflag;
        p.x2 = x; p.Cin2 = L.cin2; p.Ho = p.Wo = Ho; p.H2 = p.W2 = Hin; p.stride2 = L.stride2;
        if (k_bf16::ap_conv_pw_ds_supported(p)) {
            int cus = 0;
            HIP_TRY(device_cus(&cus));
            const int NN = L.cout >> 8, gmax = k_bf16::ap_conv_pw_grid(1L << 40, L.cout, cus);
            const long T = (((long)p.M / 196 + 7) & ~7L) * NN, rounds = (T + gmax - 1) / gmax;
            // (whole rounds only: at half a round -- 64 pairs -- the generic kernel beside the other pass is faster: -0.8 % of that bench)
            if (pw == 2 || pw == 3 || (T >= gmax && T * 5 >= rounds * gmax * 4)) {
                HIP_TRY(H16(prec, ap_launch_conv_pw)(p, st));
                return AP_OK;
            }
        }
    }
    ConvArgs a{};
    a.range_flag = rflag;
    a.x = t; a.w = L.w.p; a.scale = L.scale.as<float>(); a.shift = L.shift.as<float>(); a.res = nullptr; a.y = y;
    a.N = N; a.H = Ho; a.W = Ho; a.Cin = L.cin; a.Ho = Ho; a.Wo = Ho; a.Cout = L.cout;
    a.KH = a.KW = 1; a.stride = 1; a.pad = 0;
    a.M = N * Ho * Ho;
    a.ldx = L.cin; a.ldy = L.cout; a.ldr = L.cout; a.wld = L.wld; a.relu = 1;
    a.x2 = x; a.H2 = Hin; a.W2 = Hin; a.Cin2 = L.cin2; a.stride2 = L.stride2; a.ldx2 = L.cin2;
    HIP_TRY(dispatch_conv(a, prec, st));
    return AP_OK;
}

// fused layer1 bottleneck (bf16): x [N][H][H][c1.cin] -> y [N][H][H][256]
// c1n (or NULL): conv1 of the NEXT block computed on the block output in the same kernel -> t1n [N][H][H][128]; y_even: the block
// output is stored at the even pixels only (its one remaining reader is a stride-2 downsample branch)
int run_bneck64(const Layer& c1, const Layer& c2, const Layer& c3, bool ds, const void* x, int N, int H, void* y,
                int prec, hipStream_t st, int* rflag = nullptr, const Layer* c1n = nullptr, void* t1n = nullptr, int y_even = 0) {
    BneckArgs a{};
    a.range_flag = rflag;
    if (c1n) {
        if (ds || c1n->cin != 256 || c1n->cout != 128 || c1n->k != 1 || c1n->stride != 1 || !t1n)
            return fail(AP_ESHAPE, "fused layer1 bottleneck + next conv1: identity block, 1x1, 256 -> 128");
        a.w1n = c1n->w.p; a.s1n = c1n->scale.as<float>(); a.h1n = c1n->shift.as<float>(); a.t1n = t1n; a.y_even = y_even;
    }
    a.x = x; a.y = y;
    a.w1 = c1.w.p; a.w2 = c2.w.p; a.w3 = c3.w.p;
    a.s1 = c1.scale.as<float>(); a.h1 = c1.shift.as<float>();
    a.s2 = c2.scale.as<float>(); a.h2 = c2.shift.as<float>();
    a.s3 = c3.scale.as<float>(); a.h3 = c3.shift.as<float>();
    a.N = N; a.H = H; a.W = H;
    HIP_TRY(zero_line(&a.zero));
    a.dbg = g_conv_dbg;
    if (!((!ds && c1.cin == 256) || (ds && c1.cin == 64))) return fail(AP_ESHAPE, "fused layer1 bottleneck: C_in 256 (identity) or 64 (first block)");
    HIP_TRY(H16(prec, ap_launch_bneck2)(a, ds ? 1 : 0, st));
    return AP_OK;
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

// one depth-first pass over n = n0 + n1 images: the first n0 from x0, the rest from x1 (two views, one pass)
int trunk_chunk(ap_net* h, ap_net::TrunkWs& w, const float* x0, int n0, const float* x1, int n1, float* feat, hipStream_t st,
                size_t* ev_out = nullptr, int signal_at = 0) {
    const int bf = h->half();                                // gates the fused kernels of the 16-bit throughput modes
    const int prec = h->prec;                                // selects the kernel set (H16) and, as prec_kind, the storage kind
    const int kind = h->kind();
    const size_t es = h->esize();
    const int n = n0 + n1;
    const int conv_mode = g_conv_mode.load(std::memory_order_relaxed);   // ONE schedule for the whole pass, whatever a setter does meanwhile
    { int rc0 = reserve_trunk_ws(h, w, n); if (rc0) return rc0; }
    size_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
    if (h->tm.on == 1) HIP_TRY(h->tm.rec(st, &e0));
    if (bf && h->fuse_stem) {
        HIP_TRY(H16(prec, ap_launch_stem_pool)(x0, x1, n0, h->stem_wpk.p, h->stem_scale.as<float>(), h->stem_shift.as<float>(),
                                               w.ws_a.p, n, w.rflag, h->fuse_stem == 2 ? 1 : 2, st, g_conv_dbg));
    } else if (bf) {
        HIP_TRY(H16(prec, ap_launch_stem_conv_mfma)(x0, x1, n0, h->stem_wpk.p, h->stem_scale.as<float>(),
                                                    h->stem_shift.as<float>(), w.ws_stem.p, n, st));
    } else if (kind == AP_PREC_BF16X2 && h->fuse_stem) {
        HIP_TRY(k_bf16::ap_launch_stem_pool_split(x0, x1, n0, h->stem_wpk.p, h->stem_wpk_lo.p, h->stem_scale.as<float>(),
                                          h->stem_shift.as<float>(), w.ws_a.p, n, st));
    } else if (kind == AP_PREC_BF16X2) {
        HIP_TRY(k_bf16::ap_launch_stem_conv_mfma_split(x0, x1, n0, h->stem_wpk.p, h->stem_wpk_lo.p, h->stem_scale.as<float>(),
                                               h->stem_shift.as<float>(), w.ws_stem.p, n, st));
    } else {
        if (n0)
            HIP_TRY(k_bf16::ap_launch_stem_conv(x0, h->stem_w.as<float>(), h->stem_scale.as<float>(), h->stem_shift.as<float>(),
                                        w.ws_stem.p, n0, kind, st));
        if (n1)
            HIP_TRY(k_bf16::ap_launch_stem_conv(x1, h->stem_w.as<float>(), h->stem_scale.as<float>(), h->stem_shift.as<float>(),
                                        (char*)w.ws_stem.p + (size_t)n0 * 112 * 112 * 64 * es, n1, kind, st));
    }
    if (!(h->fuse_stem && (bf || kind == AP_PREC_BF16X2))) HIP_TRY(H16(prec, ap_launch_maxpool)(w.ws_stem.p, w.ws_a.p, n, kind, w.rflag, st));
    if (h->tm.on) HIP_TRY(h->tm.rec(st, &e1));
    if (signal_at == 1) HIP_TRY(hipEventRecord(h->ev_skew, st));
    void *cur = w.ws_a.p, *nxt = w.ws_b.p;
    int H = 56;
    int rc;
    int blk = 0;
    bool t1_ready = false;                                   // ws_t1 already holds this block's conv1 output (fused pair)
    bool pooled = false;                                     // the last convolution wrote the pooled features itself
    // Fragment-tiled intermediates (ap_common.h: ap_tiled_off): a tensor whose ONLY reader is the fused pair kernel is stored
    // as [M/16][C/8][16 pixels][8 channels], the order the pair kernel's lanes fetch it in -- t2 of every pair block, and a
    // pair block's output when the next block is an identity pair block that also got its conv1 from this kernel.  Same
    // values, same arithmetic: the features are bit-identical with the layout off (ap_net_set_tiled).
    const bool tiling = bf && h->tiled && conv_mode < 0;
    auto is_pair = [&](const ap_net::Block& X) {
        return bf && h->fuse_pair && X.pair_p && &X != &h->blocks.back() && (!X.has_down || h->fuse_ds);
    };
    bool cur_tiled = false;                                  // layout of `cur`
    // conv_pw.hip: automatic rule = conv1 only (layer4 at 512 images: 156 / 70 / 71 -> 136 / 60 / 61 us; whole bench +1.0 % single
    // pass, +0.6 % with two concurrent passes).  conv3 + identity (2: forced) is 3-9 us slower than the lean kernel and, beside a
    // concurrent pass, turns the gain into -0.5 %: a one-wave-per-SIMD kernel keeps the other pass's workgroups off its CUs
    const int pw_conv = h->pw_conv;
    for (auto& B : h->blocks) {
        if (signal_at >= 2 && blk++ == signal_at - 2) HIP_TRY(hipEventRecord(h->ev_skew, st));
        const int Ho = (H + 2 - 3) / B.c2.stride + 1;
        if (bf && h->fuse_block && B.c2.cout == 64 && B.c2.stride == 1 && H % 14 == 0 && (!B.has_down || B.c1.cin == 64)) {
            // layer1: conv1 -> conv2 -> conv3 (+identity | folded downsample) in one kernel, intermediates in LDS
            const Layer& L3 = B.has_down ? B.c3ds : B.c3;
            // last block of layer1: conv1 of layer2.0 (model_copenet.py:29-31) on the block output while it is in registers; what
            // is left to read of that output is layer2.0's stride-2 downsample branch (:41-42, :97-102) -> even pixels only
            const ap_net::Block* Nx = &B != &h->blocks.back() ? &B + 1 : nullptr;
            const bool tail = h->fuse_tail && !B.has_down && Nx && Nx->has_down && Nx->c1.cin == 256 && Nx->c1.cout == 128 &&
                              Nx->c2.stride == 2 && Nx->down.stride == 2 && conv_mode < 0;
            if ((rc = run_bneck64(B.c1, B.c2, L3, B.has_down, cur, n, H, nxt, prec, st, w.rflag, tail ? &Nx->c1 : nullptr,
                                  w.ws_t1.p, tail && h->even_out)))
                return rc;
            ++h->conv_launches;
            t1_ready = tail;
            std::swap(cur, nxt);
            continue;
        }
        bool img_fit = h->img_block == 2;
        if (h->img_block == 1) {                             // an image per CU: 256 (512) images = one (two) full rounds; 300 = two rounds 59 % full
            int cus = 0;
            HIP_TRY(device_cus(&cus));
            const long rounds = (n + cus - 1) / cus;
            img_fit = (long)n * 8 >= rounds * cus * 7;
        }
        if (bf && img_fit && B.imgw.p && H == 14 && !t1_ready && !cur_tiled && conv_mode == -1) {
            // layer3 identity block: conv1 -> conv2 -> conv3 + identity in one kernel, an image per workgroup, t1 / t2 in LDS
            BlkImgArgs a{};
            a.x = cur; a.y = nxt; a.wfrag = B.imgw.p; a.N = n; a.range_flag = w.rflag; a.dbg = g_conv_dbg;
            a.s1 = B.c1.scale.as<float>(); a.h1 = B.c1.shift.as<float>();
            a.s2 = B.c2.scale.as<float>(); a.h2 = B.c2.shift.as<float>();
            a.s3 = B.c3.scale.as<float>(); a.h3 = B.c3.shift.as<float>();
            HIP_TRY(H16(prec, ap_launch_block_img)(a, st));
            ++h->conv_launches;
            std::swap(cur, nxt);
            continue;
        }
        if (!t1_ready && cur_tiled) return fail(AP_ESTATE, "trunk: conv1 of a block would read a tiled block output");
        if (!t1_ready && (rc = run_conv(B.c1, cur, n, H, H, w.ws_t1.p, nullptr, 1, prec, st, w.rflag, 0, pw_conv))) return rc;
        h->conv_launches += (t1_ready ? 0 : 1) + 2 + ((!is_pair(B) && B.has_down && !h->fuse_ds) ? 1 : 0);   // conv1, conv2, conv3 (+ an unfused downsample)
        t1_ready = false;
        const bool pair = is_pair(B);
        // conv2 of a stage's first block on conv_pw.hip (nine taps): it writes NHWC rows, so t2 stays untiled for that block's pair kernel.
        // Automatic rule: only for a pass that has the chip to itself (l4.0.c2 164 -> 149 us, l3.0.c2 168 -> 157: +0.55 % of the whole
        // bench there, -0.45 % beside a concurrent pass, whose workgroups a one-wave-per-SIMD kernel keeps off its CUs; ev_out marks it)
        // conv2 of layer2.0 on the polyphase kernel (conv_s2p.hip; ap_net_set_s2p, off by default): its K order is its own, so when on it
        // takes the layer at EVERY batch size
        const bool c2_s2p = bf && h->s2p && B.c2s2.p && H == 56 && B.c2.stride == 2 && conv_mode == -1;
        bool c2_pw = false;
        if (!c2_s2p && pw_conv && pw_conv != 4 && !(pw_conv == 1 && ev_out) && B.c2.stride == 2 && conv_mode == -1) {
            PwArgs p3;
            int err = 0;
            c2_pw = pw_k3_args(B.c2, n, H, H, prec, &p3) && pw_fills(p3.M, B.c2.cout, pw_conv, &err);
            HIP_TRY((hipError_t)err);
        }
        const int t2_tiled = pair && tiling && !c2_pw;
        bool c2_img = false;
        if (bf && h->img3 && B.c2img.p && H == 28 && B.c2.stride == 1 && conv_mode == -1) {
            c2_img = h->img3 == 2;
            if (h->img3 == 1) {                              // half an image per CU: whole rounds of the chip
                int cus = 0;
                HIP_TRY(device_cus(&cus));
                const long units = 2L * n, rounds = (units + cus - 1) / cus;
                c2_img = units * 8 >= rounds * cus * 7;
            }
        }
        if (c2_s2p) {
            ConvS2pArgs ca{};
            ca.x = w.ws_t1.p; ca.y = w.ws_t2.p; ca.wfrag = B.c2s2.p; ca.scale = B.c2.scale.as<float>(); ca.shift = B.c2.shift.as<float>();
            ca.N = n; ca.y_tiled = t2_tiled; ca.range_flag = w.rflag;
            HIP_TRY(zero_line(&ca.zero));
            HIP_TRY(H16(prec, ap_launch_conv_s2p)(ca, st));
        } else if (c2_img) {
            ConvImg3Args ca{};
            ca.x = w.ws_t1.p; ca.y = w.ws_t2.p; ca.wfrag = B.c2img.p; ca.scale = B.c2.scale.as<float>(); ca.shift = B.c2.shift.as<float>();
            ca.N = n; ca.y_tiled = t2_tiled; ca.range_flag = w.rflag;
            HIP_TRY(zero_line(&ca.zero));
            HIP_TRY(H16(prec, ap_launch_conv_img3)(ca, st));
        } else if ((rc = run_conv(B.c2, w.ws_t1.p, n, H, H, w.ws_t2.p, nullptr, 1, prec, st, w.rflag, t2_tiled, c2_pw ? pw_conv : 0))) return rc;
        if (pair) {
            // conv3 (+ identity | + folded downsample, ReLU) AND -- where the pair carries it -- the next block's conv1 in one
            // kernel: the block output is written once and not read back for conv1 (model_copenet.py:38-45 of this block,
            // :29-31 of the next)
            const ap_net::Block& Nx = *(&B + 1);
            const Layer& L3 = B.has_down ? B.c3ds : B.c3;
            PairArgs a{};
            a.t2 = w.ws_t2.p; a.wstream = B.pair.p;
            a.s3 = L3.scale.as<float>(); a.h3 = L3.shift.as<float>();
            a.s1 = Nx.c1.scale.as<float>(); a.h1 = Nx.c1.shift.as<float>();
            a.out = nxt; a.t1n = w.ws_t1.p; a.M = n * Ho * Ho; a.dbg = g_conv_dbg; a.range_flag = w.rflag;
            a.t2_tiled = t2_tiled; a.res_tiled = cur_tiled;
            a.out_tiled = t2_tiled && B.pair_n1 > 0 && is_pair(Nx) && !Nx.has_down;
            cur_tiled = a.out_tiled != 0;
            a.Ho = a.Wo = Ho;
            if (B.has_down) { a.x2 = cur; a.H2 = a.W2 = H; a.stride2 = L3.stride2; }
            else a.res = cur;
            // the next block is a stage's first one and got its conv1 from this kernel: all that is read of `out` is that block's
            // stride-2 downsample branch (model_copenet.py:41-42, :97-102) -- the even pixels
            a.out_even = h->even_out && !a.out_tiled && B.pair_n1 > 0 && Nx.has_down && Nx.down.stride == 2 && Nx.c2.stride == 2;
            HIP_TRY(H16(prec, ap_launch_conv_pair)(a, B.pair_p, B.pair_p2, B.pair_c3, B.pair_n1, st));
            t1_ready = B.pair_n1 > 0;
        } else if (cur_tiled) {                               // (cannot happen: out_tiled is only set when the next block is a pair block)
            return fail(AP_ESTATE, "trunk: a tiled block output reached a kernel that reads NHWC");
        } else if (B.has_down && h->fuse_ds) {
            if ((rc = run_c3_ds(B.c3ds, w.ws_t2.p, cur, n, Ho, H, nxt, prec, st, w.rflag, pw_conv))) return rc;
        } else if (bf && h->fuse_pool && &B == &h->blocks.back() && !B.has_down && Ho == 7 && conv_mode == -1) {
            // last convolution of the trunk: conv3 + bn3 + identity + ReLU AND AvgPool2d(7) + view in one kernel
            // (model_copenet.py:38-47 of layer4.2, then :173-175); the block output is never written
            ConvArgs a{};
            a.x = w.ws_t2.p; a.w = B.c3.w.p; a.scale = B.c3.scale.as<float>(); a.shift = B.c3.shift.as<float>(); a.res = cur; a.y = nullptr;
            a.N = n; a.H = a.W = a.Ho = a.Wo = Ho; a.Cin = B.c3.cin; a.Cout = B.c3.cout;
            a.KH = a.KW = 1; a.stride = 1; a.pad = 0; a.M = n * Ho * Ho;
            a.ldx = B.c3.cin; a.ldy = B.c3.cout; a.ldr = B.c3.cout; a.wld = B.c3.wld; a.relu = 1;
            a.pool_out = feat; a.range_flag = w.rflag;
            HIP_TRY(zero_line(&a.zero));
            if (k_bf16::ap_conv_lean_supported(a, kind)) {
                HIP_TRY(H16(prec, ap_launch_conv_lean)(a, st));
                pooled = true;
            } else if ((rc = run_conv(B.c3, w.ws_t2.p, n, Ho, Ho, nxt, cur, 1, prec, st, w.rflag))) return rc;
        } else {
            const void* res = cur;
            if (B.has_down) {
                if ((rc = run_conv(B.down, cur, n, H, H, w.ws_ds.p, nullptr, 0, prec, st, w.rflag))) return rc;
                res = w.ws_ds.p;
            }
            if ((rc = run_conv(B.c3, w.ws_t2.p, n, Ho, Ho, nxt, res, 1, prec, st, w.rflag, 0, (B.has_down || pw_conv != 2) ? 0 : pw_conv))) return rc;   // (conv3 + identity: 89-95 us against the lean kernel's 86: only when forced)
        }
        std::swap(cur, nxt);
        H = Ho;
    }
    if (h->tm.on) HIP_TRY(h->tm.rec(st, &e2));
    if (!pooled) HIP_TRY(H16(prec, ap_launch_avgpool)(cur, feat, n, 2048, kind, w.rflag, st));
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
                                 &ev[((size_t)q * rounds + r) * 4], (q == 0 && np == 2 && r == 0) ? h->dual_skew : 0);
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
                             feat + (size_t)i0 * 2048, st);
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
