// What the host translation units of libairpose_hip.so (api_*.hip) share: error reporting, device buffers, the three handle
// structs, the launch functions of the trunk kernels (launch_*: api_ops.hip) and the few other functions that cross files.  No kernel and no exported symbol: everything that crosses a file is in
// namespace ap_internal with hidden visibility; whatever one file alone uses stays in that file's anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <map>
#include <string>
#include <vector>
#include "../../include/airpose_hip.h"
#define AP_API_TU   // kernels.h: declare the launchers of BOTH 16-bit storage flavours (k_bf16:: / k_f16::)
#include "ap_common.h"
#include "kernels.h"

namespace ap_internal __attribute__((visibility("hidden"))) {
extern thread_local std::string g_err;        // what ap_last_error returns (api_net.hip)
int fail(int code, const std::string& msg);   // sets it and returns code
// launcher of the 16-bit kernel set the precision selects: fp16 storage (AP_PREC_F16) or bf16 storage / fp32 / split-bf16
#define H16(prec, fn) ((prec) == AP_PREC_F16 ? k_f16::fn : k_bf16::fn)
inline bool prec_half(int prec) { return prec == AP_PREC_BF16 || prec == AP_PREC_F16; }   // the throughput kernels
inline int prec_kind(int prec) { return prec == AP_PREC_F16 ? K_BF16 : prec; }             // storage kind inside a kernel set
inline bool prec_valid(int prec) { return prec == AP_PREC_FP32 || prec == AP_PREC_BF16 || prec == AP_PREC_BF16X2 || prec == AP_PREC_F16; }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail((int)_e, std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return e;
            (void)hipFree(p);
            p = nullptr;
            bytes = 0;
        }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T* as() const { return (T*)p; }
};

inline hipError_t upload(DevBuf& b, const void* src, size_t n) {
    hipError_t e = b.reserve(n);
    if (e != hipSuccess) return e;
    return hipMemcpy(b.p, src, n, hipMemcpyHostToDevice);
}

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { return data.size(); }
};

// one convolution + folded BatchNorm as the launch functions take it: plain pointers and shapes -- a Layer of the trunk, or the
// arguments of a stand-alone operator entry (w: packed rows, or the fragment stream of the kernel that is launched)
struct ConvDesc {
    const void* w;
    const float *scale, *shift;
    int cin, cout, k, stride, pad, wld;
    int cin2, stride2;              // second K segment (downsample folded into conv3)
};

struct Layer {                  // a conv or linear layer in packed device form
    int cin = 0, cout = 0, k = 1, stride = 1, pad = 0;
    int wld = 0, cout_pad = 0;
    int cin2 = 0, stride2 = 1;      // second K segment (downsample folded into conv3)
    DevBuf w, scale, shift;
    DevBuf pw;                      // pointwise layers of layer3 / layer4: the weights as conv_pw.hip's fragment streams
    ConvDesc desc(bool pw_stream = false) const {
        return ConvDesc{pw_stream ? pw.p : w.p, scale.as<float>(), shift.as<float>(), cin, cout, k, stride, pad, wld, cin2, stride2};
    }
};

struct Timing {
    int on = 0;                     // 0 off, 1 every stage, 2 conv stack only (two events per trunk pass)
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<size_t> marks[4];   // pairs of event indices per stage
    std::vector<char> qfree[4];     // per quad: the two passes ran free of each other (own durations instead of the span)
    std::vector<size_t> quads[4];   // two-stream passes: (start A, end A, start B, end B): the stage's span over both streams
    int64_t passes = 0;
    hipError_t rec(hipStream_t st, size_t* idx) {
        if (used == pool.size()) {
            hipEvent_t e;
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) return r;
            pool.push_back(e);
        }
        *idx = used++;
        return hipEventRecord(pool[*idx], st);
    }
    hipError_t collect(double ms[4], int nstage, int64_t* n, bool reset) {
        for (int s = 0; s < nstage; ++s) {
            ms[s] = 0.0;
            for (size_t i = 0; i + 1 < marks[s].size(); i += 2) {
                hipError_t r = hipEventSynchronize(pool[marks[s][i + 1]]);
                if (r != hipSuccess) return r;
                float t = 0.f;
                r = hipEventElapsedTime(&t, pool[marks[s][i]], pool[marks[s][i + 1]]);
                if (r != hipSuccess) return r;
                ms[s] += t;
            }
            for (size_t i = 0; i + 3 < quads[s].size(); i += 4) {
                float span = 0.f;
                if (i / 4 < qfree[s].size() && qfree[s][i / 4]) {
                    // free-running passes (ap_trunk_fwd_twoview_async): the two streams drift apart by up to a step, so the span from
                    // the first start to the last end also counts time in which one of the two was already / still in a
                    // neighbouring step; every pass shares the chip with exactly one other pass for its whole duration, so the
                    // stage's time is the mean of the two passes' OWN durations (equal to the span when they run in lock step)
                    float own = 0.f;
                    for (int a = 0; a < 2; ++a) {
                        hipError_t r = hipEventSynchronize(pool[quads[s][i + 1 + 2 * a]]);
                        if (r != hipSuccess) return r;
                        float t = 0.f;
                        r = hipEventElapsedTime(&t, pool[quads[s][i + 2 * a]], pool[quads[s][i + 1 + 2 * a]]);
                        if (r != hipSuccess) return r;
                        own += 0.5f * t;
                    }
                    ms[s] += own;
                    continue;
                }
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b) {            // latest end minus earliest start (negative pairs lose)
                        hipError_t r = hipEventSynchronize(pool[quads[s][i + 1 + 2 * b]]);
                        if (r != hipSuccess) return r;
                        float t = 0.f;
                        r = hipEventElapsedTime(&t, pool[quads[s][i + 2 * a]], pool[quads[s][i + 1 + 2 * b]]);
                        if (r != hipSuccess) return r;
                        span = std::max(span, t);
                    }
                ms[s] += span;
            }
        }
        *n = passes;
        if (reset) {
            for (auto& m : marks) m.clear();
            for (auto& q : quads) q.clear();
            for (auto& q : qfree) q.clear();
            used = 0;
            passes = 0;
        }
        return hipSuccess;
    }
    void destroy() {
        for (auto e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

constexpr double BN_EPS = 1e-5;
constexpr int ST = 148, SLD = 288, DLD = 148;

// The stem's weight operands, packed on the host from conv1.weight [64][3][7][7] fp32 -- ONE packing for the trunk (finalize_trunk)
// and for the stand-alone operator (ap_stem_pack), so a test of the operator is a test of the packing the trunk runs on:
//   direct  [k = (r,s,c)][64] fp32 for the direct kernel (fp32 mode)
//   pk      [64][AP_STEM_WLD] 16-bit for the MFMA stems, k' = r*32 + s*4 + c (zero elsewhere: 4th channel slot, 8th tap, row pad):
//           fp16 for AP_PREC_F16 (*f16_overflow set when a weight leaves its range), bf16 otherwise -- for AP_PREC_BF16X2 the high plane
//   pk_lo   AP_PREC_BF16X2 only: the low plane, bf16(w - hi) at the same positions
struct StemPack {
    std::vector<float> direct;
    std::vector<uint16_t> pk, pk_lo;
};
void pack_stem(const float* w, int prec, StemPack& p, bool* f16_overflow);                        // api_net.hip

// api_trunk.hip
extern unsigned long long* g_conv_dbg;   // phase-stamp buffer (ap_debug_set_trace)
// the library's own host-mapped range word while ap_debug_set_range_hook is on and `prec` is AP_PREC_F16, NULL otherwise: what the
// stand-alone operator entries (api_ops.hip) hand their kernels as range_flag
int* ops_range_word(int prec);
int conv_mode();                         // the raw value of ap_set_conv_config, read once: a caller decodes ONE value per launch / per pass
hipError_t dispatch_conv(ConvArgs& a, int prec /* AP_PREC_* */, hipStream_t st, int mode);
const char* conv_refusal(const ConvArgs& a, int prec, int mode);   // why dispatch_conv would not run these arguments (NULL: it runs); no launch
inline hipError_t dispatch_conv(ConvArgs& a, int prec, hipStream_t st) { return dispatch_conv(a, prec, st, conv_mode()); }
int trunk_fwd(ap_net* h, const float* x0, int n0, const float* x1, int n1, float* feat, hipStream_t st, hipStream_t st_out = nullptr);
// api_net.hip
int finalize_trunk(ap_net* h);

// api_ops.hip -- ONE launch function per kernel a trunk pass can run: it fills the kernel's argument struct from plain shapes and
// pointers, takes the zero line, sets the phase-stamp buffer and calls the launcher.  The pass (api_trunk.hip) calls it with its
// Layer fields and workspace, the stand-alone operator entry with its validated arguments: a test of the operator is a test of
// the launch path the trunk runs on.  rflag: the range word of the caller (NULL: none)
// generic kernels via dispatch_conv.  x2: the block input of a folded downsample (second K segment of c.cin2 channels, H2 x H2,
// sampled with c.stride2), or NULL.  pool_out: AvgPool2d(7) into [N][cout] fp32 inside the lean kernel where it takes the shape
// (*pooled = true, y not written); otherwise the plain convolution into y
hipError_t launch_conv(const ConvDesc& c, const void* x, int N, int H, int W, const void* res, void* y, int relu, int y_tiled,
                       const void* x2, int H2, float* pool_out, bool* pooled, int prec, int mode, int* rflag, hipStream_t st);
bool conv_pool_fits(const ConvDesc& c, int N, int prec);     // launch_conv would pool N 7 x 7 images (with an identity and ReLU)
// conv_refusal on the arguments launch_conv would build for a plain / tiled / folded convolution
const char* conv_form_refusal(const ConvDesc& c, int N, int H, int W, int y_tiled, bool fold, int H2, int prec, int mode);
// conv_pw.hip (c.w: its fragment stream): pointwise (+ identity), pointwise + folded downsample, 3 x 3 / stride 2; *_fits: the
// kernel's own predicate on the arguments that launch would build
hipError_t launch_conv_pw(const ConvDesc& c, const void* x, const void* res, void* y, int M, int prec, int* rflag, hipStream_t st);
bool conv_pw_ds_fits(const ConvDesc& c, int N, int Ho, int H2);
hipError_t launch_conv_pw_ds(const ConvDesc& c, const void* t, const void* x2, void* y, int N, int Ho, int H2, int prec, int* rflag, hipStream_t st);
bool conv_pw_k3_fits(const ConvDesc& c, int N, int H);
hipError_t launch_conv_pw_k3(const ConvDesc& c, const void* x, void* y, int N, int H, int prec, int* rflag, hipStream_t st);
// bottleneck2.hip (c1 / c2 / c3, and c1n of the tail variant: w, scale, shift only)
hipError_t launch_bneck2(const ConvDesc& c1, const ConvDesc& c2, const ConvDesc& c3, int ds, const void* x, void* y, int N, int H, int W,
                         const ConvDesc* c1n, void* t1n, int y_even, int prec, int* rflag, hipStream_t st);
hipError_t launch_block_img(const void* x, const void* wfrag, const float* s1, const float* h1, const float* s2, const float* h2,
                            const float* s3, const float* h3, void* y, int N, int prec, int* rflag, hipStream_t st);
hipError_t launch_conv_img3(const void* x, const void* wfrag, const float* scale, const float* shift, void* y, int N, int y_tiled,
                            int prec, int* rflag, hipStream_t st);
hipError_t launch_conv_s2p(const void* x, const void* wfrag, const float* scale, const float* shift, void* y, int N, int y_tiled,
                           int prec, int* rflag, hipStream_t st);
// conv_pair.hip: identity block (in = the residual; H2 = 0) or stage-first block (in = the block input [N][H2][H2][P2], sampled with stride2)
struct PairLayout { int t2_tiled, res_tiled, out_tiled, out_even; };
hipError_t launch_conv_pair(const void* t2, const void* wstream, const float* s3, const float* h3, const float* s1, const float* h1,
                            const void* in, void* out, void* t1n, int M, int Ho, int H2, int stride2, int P, int P2, int N1,
                            PairLayout lay, int prec, int* rflag, hipStream_t st);
// stem.hip: form 0 un-pooled, 1 a workgroup per strip + max-pool, 2 persistent + max-pool (ap_stem_nhwc); x0: the first n0 of n images
hipError_t launch_stem(int prec, int form, const float* x0, const float* x1, int n0, int n, const void* w, const void* w_lo,
                       const float* scale, const float* shift, void* y, int* rflag, hipStream_t st);
hipError_t launch_maxpool(const void* x, void* y, int n, int prec, int* rflag, hipStream_t st);
hipError_t launch_avgpool(const void* x, float* y, int n, int C, int prec, int* rflag, hipStream_t st);

}  // namespace ap_internal
using namespace ap_internal;

struct ap_net {
    int device = 0, prec = AP_PREC_BF16, variant = 0;
    bool finalized = false;
    std::map<std::string, HostTensor> tensors;
    const ap_net* tensors_of = nullptr;                      // the fp32 reference handle of ap_net_parity_probe packs its owner's host tensors
    ap_net* probe_ref = nullptr;                             // ... that handle (trunk only), valid for the current packing
    DevBuf probe_x, probe_bb, probe_pos, probe_feat, probe_out;
    // trunk
    DevBuf stem_w, stem_wpk, stem_wpk_lo, stem_scale, stem_shift;   // stem_wpk_lo: low plane of the split-bf16 stem weights
    struct Block {
        Layer c1, c2, c3, down, c3ds; bool has_down = false;
        DevBuf pair;               // conv3 of this block + conv1 of the next as one weight stream (conv_pair.hip)
        int pair_p = 0, pair_p2 = 0, pair_c3 = 0, pair_n1 = 0;
        DevBuf imgw;               // layer3 identity blocks: the three weight matrices as the fragment streams of block_img.hip
        DevBuf c2img;              // layer2 identity blocks: conv2's weights as the fragment streams of conv_img3.hip
        DevBuf c2s2;               // layer2.0: conv2's weights as the fragment streams of conv_s2p.hip
    };
    std::vector<Block> blocks;
    // regressor (fp32)
    Layer fc1_feat, fc1_state, fc2, dec;
    Layer fold_feat, fold_state;   // dec o fc2 o fc1 folded into one 145 x 2332 map (no activation between them)
    DevBuf foldT_feat, foldT_state, fold_bias;   // the same map k-major ([k][148]) for the fused IEF kernel (copenet head)
    bool fuse_ief = true;          // folded map: one split-K feature kernel + one kernel for all IEF iterations
    bool fold = true;
    double fold_check_err = 0.0;   // ap_net_finalize: folded vs literal chain on the probe batch (max |diff| / max |literal|)
    bool fold_rejected = false;    // ... above fold_bar: fold forced off for this checkpoint
    double fold_bar = 1e-5;        // (ap_net_set_fold_bar: test aid)
    bool fuse_ds = true;           // first block of a stage: downsample conv folded into conv3 as a second K segment
    bool fuse_block = true;        // 16-bit modes: each layer1 bottleneck as one kernel (bottleneck2.hip); off: separate convs
    bool tiled = true;             // 16-bit modes: tensors only the fused pair kernel reads (t2, identity) in its fragment-tiled layout
    bool fuse_pair = true;         // bf16: conv3 of an identity block + conv1 of the next block as one pixel-local kernel (conv_pair.hip)
    bool fuse_tail = true;         // 16-bit modes: conv1 of layer2.0 inside the kernel of layer1's last block (bottleneck2.hip, tail variant);
                                   // the block output is then stored at the even pixels only (layer2.0's stride-2 downsample reads nothing else)
    int pw_conv = 1;               // 16-bit modes: conv1 of the layer3 / layer4 bottlenecks that no fused kernel covers on the one-wave-per-SIMD pointwise
                                   // kernel (conv_pw.hip): 0 never; 1 (default) when its tiles fill half the chip or whole rounds of it; 2 whenever
                                   // supported, and conv3 + identity too; 3 conv1 whenever supported
    int s2p = 0;                   // 16-bit modes: conv2 of layer2.0 (3x3 / stride 2 at 56 x 56) on the polyphase kernel (conv_s2p.hip), at every batch size
                                   // (its K order is its own).  OFF by default: 12-27 % faster than the ring kernel alone, but it owns its CUs (8 waves x 240
                                   // registers) and the two free-running passes of the default lose more concurrency than the layer gains: -1.7 % in the bench
    int img3 = 1;                  // 16-bit modes: conv2 of the layer2 identity blocks on the half-image-resident kernel (conv_img3.hip): 0 never, 1 when the
                                   // pass fills whole rounds of the chip with half images (same bits either way), 2 always
    int img_block = 1;             // 16-bit modes: each layer3 identity bottleneck as ONE image-resident kernel (block_img.hip): 0 never,
                                   // 1 when the pass fills whole rounds of the chip (an image per CU; same bits either way), 2 always
    bool even_out = true;          // 16-bit modes: a pair block whose output is read by a stride-2 downsample branch ONLY stores the even pixels
    int fuse_stem = 1;             // bf16 / bf16x2: conv1+bn1+relu+maxpool in one kernel (bit-identical to the two-kernel path); 16-bit
                                   // modes: 1 = the persistent form of stem.hip (default), 2 = a workgroup per strip (the round-4 form)
    bool fuse_pool = false;        // 16-bit modes: AvgPool2d(7) in the epilogue of layer4.2 conv3 (conv_lean.hip POOL variant; bit-identical).
                                   // Off by default: measured neutral (fp16) to -0.5 % (bf16) in the two-stream trunk (docs/DESIGN_rounds1-4.md, section 5)
    DevBuf mean_pose, mean_shape, mean_cam;
    // workspace
    int chunk = 0;
    struct TrunkWs { DevBuf ws_stem, ws_a, ws_b, ws_t1, ws_t2, ws_ds;
                     int* rflag = nullptr; };   // the range word the kernels of THIS pass stream set (AP_PREC_F16; ap_net::range_flag + q)
    TrunkWs tw[4];                 // [1..]: the other concurrent passes when the views run on several streams
    DevBuf ws_feat;
    // two-view forward: view 0 and view 1 as two concurrent trunk passes on two internal streams (an HBM-bound layer of
    // one pass overlaps an MFMA-bound layer of the other: -4 % trunk time at 2 x 256 images); 0 = one pass over both views
    bool dual_stream = true;
    int dual_skew = 0;             // experiment: the second pass starts after the first has finished its stem (1) / its block k-2 (k >= 2)
    hipEvent_t ev_skew = nullptr;
    hipStream_t aux[4] = {nullptr, nullptr, nullptr, nullptr};
    bool unjoined = false;         // ap_trunk_fwd_twoview_async: the last two-pass call joined into another stream than its inputs'
    hipEvent_t ev_fork = nullptr, ev_in = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    int passes_per_view = 1;       // experiment: 2 = each view as two concurrent half passes (four streams)
    DevBuf ws_H, ws_S, ws_T1, ws_T2, ws_D, ws_state;
    Timing tm;
    bool half() const { return prec_half(prec); }            // the throughput kernels (bf16 or fp16 storage)
    int kind() const { return prec_kind(prec); }
    size_t esize() const { return half() ? 2 : 4; }          // fp32 and split-bf16 pairs: 4 bytes
    // AP_PREC_F16 range sentinel: host-mapped word the pooling stage sets when a trunk feature is not finite (NULL otherwise).
    // range_mode 1 (default): sticky, reported by the NEXT call on the handle and by ap_net_range_status (no sync on the hot path);
    // 2: every trunk-running call synchronises its stream and reports its own pass
    // One word per pass stream (tw[q].rflag = range_flag + q): a snapshot taken on pass stream q behind a batch's last kernel there sees
    // exactly the kernels of this and earlier batches, whatever the sibling stream is already running (ap_net_range_mark_next)
    int* range_flag = nullptr;                               // [4]
    int* range_slots = nullptr;                              // [AP_RANGE_SLOTS][4] host-mapped words: stream-ordered snapshots of the pass words
    int conv_launches = 0;                                   // kernel launches of the conv stack in the most recent trunk call, all passes (ap_net_last_conv_launches)
    int mark_slot = -1;                                      // ap_net_range_mark_next: the next trunk-running call snapshots into this slot
    int range_mode = 1;
    bool range_any() const {
        if (!range_flag) return false;
        int v = 0;
        for (int q = 0; q < 4; ++q) v |= __atomic_load_n(range_flag + q, __ATOMIC_RELAXED);
        return v != 0;
    }
    bool f16_overflow = false;                               // AP_PREC_F16: a packed weight left the fp16 range (ap_net_finalize refuses)
    uint16_t h16(float f) { return prec == AP_PREC_F16 ? host_f32_to_f16(f, &f16_overflow) : host_f32_to_bf16(f); }
};

struct ap_smplx {
    int device = 0;
    SmplxModelDev m{};
    Layer dirs;                 // blend-shape GEMM operand: rows = 3V, K = 512 (fp32: exact fp32 MFMA chain)
    DevBuf dirs_split;          // the same operand as split-bf16 pairs: three-term products (lo lo dropped) on the bf16 matrix pipe (default)
    DevBuf dirs_frag, jv_slot, skin_idx8, skin_w4, skin_idx8b, skin_w4b, jt_pack, ws_side;   // fused contraction + skinning: directions in MFMA fragment order, joint-vertex slots / buffer
    DevBuf ws_cnt;              // ... arrival counters of the body groups (joints by the group's last workgroup); zero between launches
    bool fold_post = true;      // ... and with the post transform composed into those 22 transforms by the prep kernel (A22); ap_smplx_set_fused(h, 7): off (A/B)
    int merge_bones = 1;        // (0: off, 1: on, 2: with 64 bodies per workgroup -- A/B, slower) body-only calls: the fused kernel skins over the 22 posed transforms (merged skin table); ap_smplx_set_fused(h, 6): all 55 (A/B)
    bool fuse_joints = false;   // ap_smplx_set_fused(h, 4): joints / landmarks / projection inside the fused kernel (measured 7 us SLOWER than their own launch)
    bool blend_split = true;
    bool fused = true;          // body-only pose feature, 4 bones per vertex, split-bf16 blend: one kernel for contraction + skinning
    DevBuf j_template, j_shapedirs, parents, depth, skin_idx, skin_w, extra_verts, lmk_tri, lmk_bary;
    DevBuf ws_coef, ws_A, ws_A22, ws_jposed, ws_post, ws_vposed, ws_cc;
    int n_out_joints = 0;
    Timing tm;
    // backward (ap_smplx_bwd): its own tables and workspaces, allocated on the first backward -- never shared with a forward
    bool bw_ready = false;
    int bw_nr = 0;
    DevBuf bw_bone_off, bw_bone_ent, bw_jv_off, bw_jv_ent;                  // bone-major skinning entries per vertex range; joint scatter
    DevBuf bw_coef, bw_A, bw_jposed, bw_vposed, bw_gvp, bw_gA, bw_gt, bw_gcoef;
};

struct ap_fit {                   // AirPose+ fitting loop state (fitting.hip)
    int device = 0;
    const ap_smplx* body = nullptr;
    DevBuf w1t, w2t, w3t, w1, w2, w3, b1, b2, b3;     // VPoser decoder: k-major transposes (forward) / as stored (backward)
    DevBuf H1, H2, O, dO, aa, dphi, dtau, dbeta, loss, adam_m, adam_v, robust;
};
