// Internal helpers shared by the sources of libairpose_grad.so (head_mlp.hip, head_grad.hip, head_local_grad.hip, geom_grad.hip,
// trunk_grad.hip, trunk_grad_bf16.hip, loss_grad.hip, loss_real_grad.hip, optim.hip, eval_metrics.hip, render.hip, eval_align.hip, xview_metrics.hip, seq_fit.hip, seq_batch.hip, synth_batch.hip, augment.hip, roll.hip, guard/grad_guard.hip).  Texts that only some of them share are includes of their own: trunk_elem.inc
// and trunk_walk.inc (the two trunks), loss_common.inc (the losses and geom_grad.hip), metric_common.inc (eval_metrics.hip, eval_align.hip, xview_metrics.hip),
// draws.inc (synth_batch.hip, augment.hip, roll.hip), preprocess_px.inc (synth_batch.hip, roll.hip, and stem.hip of libairpose_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/airpose_grad.h"

// records the thread-local message apg_last_error() returns; returns code
__attribute__((visibility("hidden"))) int apg_fail(int code, const std::string& msg);

// every pointer present and aligned (align a power of two), in list order, or APG_EINVAL naming the first that is not:
// "<f><name> is NULL", "<f><name> is not <align>-byte aligned"
struct ApgPtr { const void* p; const char* name; int align; };
__attribute__((visibility("hidden"))) int apg_check_ptrs(const std::string& f, const ApgPtr* ps, int count);

// returns from the calling entry point with the HIP error code of `expr` and a message naming it
#define APG_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) return apg_fail((int)_e, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// splitmix64 finaliser
__host__ __device__ __forceinline__ uint64_t apg_mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// dropout keep decision of (seed, layer, row, col): u = top 24 bits of the hash / 2^24 (exact in fp32), keep iff u >= p.
// Counter = layer << 56 | row << 24 | col (col < 2^24, row < 2^32).
__host__ __device__ __forceinline__ bool apg_keep(uint64_t seed, int layer, int row, int col, float p) {
    if (p <= 0.f) return true;
    const uint64_t ctr = ((uint64_t)(uint32_t)layer << 56) ^ ((uint64_t)(uint32_t)row << 24) ^ (uint64_t)(uint32_t)col;
    const uint64_t h = apg_mix64(apg_mix64(ctr) ^ seed);
    const float u = (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f);
    return u >= p;
}

// ---------------------------------------------------------------------------------------------
// head_mlp.hip: the library's fp32 product and what the two trainable heads (head_grad.hip, head_local_grad.hip) run on it.
// apg_gemm_kernel: C = A B with one 64 x 64 tile per workgroup, K reduced in index order inside that workgroup (no split, no
// atomics), and one of the epilogues below.
enum {
    APG_EPI_STORE = 0,                   // C[m * ldc + n] = acc
    APG_EPI_HID_FWD = 1,                 // C = dropout(acc + bias[n]) of (seed, layer, row m, column n)
    APG_EPI_DEC_FWD = 2,                 // the two-view decoders: out_v[b * ldo + n] = base[m * ldbase + n] + (acc + bias[n])
    APG_EPI_HID_BWD = 3,                 // C = dropout'(acc)
    APG_EPI_DEC_LOCAL = 4                // packed decoders: column n of decoder d = the one with doff[d] <= n < doff[d + 1], j = n - doff[d]:
                                         // dout[d][m * (doff[d + 1] - doff[d]) + j] = base[m * ldbase + dres[d] + j] + (acc + bias[n])
};

struct ApgGemmArgs {
    const float* A;                      // A(m, k) = A[m * sam + k * sak]
    long long sam, sak;
    const float* B;                      // B(k, n) = B[k * sbk + n * sbn]
    long long sbk, sbn;
    int M, N, K;
    int epi;
    float* C;                            // EPI_STORE / EPI_HID_*: C[m * ldc + n]
    int ldc;
    const float* bias;                   // EPI_HID_FWD / EPI_DEC_*: + bias[n]
    uint64_t seed;                       // EPI_HID_*: dropout of (layer, row m, column n)
    int layer;
    float p, scale;
    int nb;                              // EPI_DEC_FWD: rows per view; out_v[b * ldo + n] = base[m * ldbase + n] + acc + bias[n]
    float* out0;
    float* out1;
    int ldo;
    const float* base;                   // EPI_DEC_*
    int ldbase;
    int ndec;                            // EPI_DEC_LOCAL: decoders, their first packed column (doff[ndec] = N), residual column, output
    int doff[4];
    int dres[3];
    float* dout[3];
};

// A / B given by their two strides (one of each pair is 1); EPI_STORE, no dropout
__attribute__((visibility("hidden"))) ApgGemmArgs apg_gemm_args(const float* A, long long sam, long long sak, const float* B,
                                                                long long sbk, long long sbn, int M, int N, int K);
// epi = APG_EPI_HID_FWD / APG_EPI_HID_BWD with the keep scale of p
__attribute__((visibility("hidden"))) void apg_gemm_set_dropout(ApgGemmArgs& g, int epi, uint64_t seed, int layer, float p);
__attribute__((visibility("hidden"))) hipError_t apg_gemm_launch(const ApgGemmArgs& g, hipStream_t st);
// out[c] = sum over rows of x[r * ld + c] in two fixed-order passes (chunks of APG_CS_ROWS rows in row order, then the chunks in
// order); part: ceil(rows / APG_CS_ROWS) * cols floats
constexpr int APG_CS_ROWS = 32;
__attribute__((visibility("hidden"))) hipError_t apg_colsum(const float* x, int rows, int cols, int ld, float* part, float* out,
                                                            hipStream_t st);

// The heads' network on a packed fc1 input xc (R x K1, K1 = XF + the head's state columns): h1d = drop1(xc W1^T + b1),
// h2d = drop2(h1d W2^T + b2), then ndec decoders packed as N columns (wdec: N x HID).
constexpr int XF = 2048;                 // trunk features, the first columns of xc
constexpr int HID = 1024;
inline size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }

// the fc1 and fc2 launches; -> APG_OK or apg_fail's code
__attribute__((visibility("hidden"))) int apg_head_hidden_fwd(int R, int K1, const float* xc, const float* W1, const float* b1,
                                                              const float* W2, const float* b2, uint64_t seed, float p1, float p2,
                                                              float* h1d, float* h2d, hipStream_t st);

// the backward chain's pieces of a head's workspace, in floats from its start; the head's own pieces go behind total
struct ApgChainLayout {
    size_t gd, gh2, gh1, gxc, part, total;
    int c0;                              // first column of g_xc that is computed: 0, or XF when no feature gradient is wanted
};
__attribute__((visibility("hidden"))) ApgChainLayout apg_chain_layout(size_t R, int K1, int N, int need_gxf);

struct ApgChainBwd {
    int R, K1, N, ndec;
    const int* doff;                     // first packed column of each decoder; doff[ndec] = N
    const float *xc, *h1d, *h2d, *wdec, *W1, *W2;
    uint64_t seed;
    float p1, p2;
    void* const* g_param;                // fc1 W, b, fc2 W, b, then W, b of each decoder; NULL = skipped
    bool want_gxc;                       // g_xc[:, c0:] = g_h1 W1[:, c0:] into the layout's gxc, for the head to scatter
};
// From g_delta (the head has packed it into the layout's gd): per decoder g_W then g_b; g_h2, g_W2, g_b2; g_h1, g_W1, g_b1; g_xc.
__attribute__((visibility("hidden"))) int apg_head_chain_bwd(const ApgChainBwd& c, const ApgChainLayout& l, float* ws,
                                                             hipStream_t st);
