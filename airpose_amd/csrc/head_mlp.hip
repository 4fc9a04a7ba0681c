// What the two trainable regressor heads of libairpose_grad.so share (head_grad.hip: the two-view IEF head; head_local_grad.hip:
// the generic view-local head): the library's fp32 product, the column sums, the dropout mask, and the network both heads run
// on a packed fc1 input xc (R x K1) -- fc1, drop1, fc2, drop2, then decoders packed as N columns.
//   apg_head_hidden_fwd: h1d = drop1(xc W1^T + b1), h2d = drop2(h1d W2^T + b2).  The decoder product stays with each head: its
//             epilogue writes that head's outputs.
//   apg_head_chain_bwd: from g_delta (R x N, packed by the head) the weight gradients g_delta_d^T h2d, g_h2^T h1d, g_h1^T xc, the
//             bias gradients as column sums (two fixed-order passes), g_h2 = drop2'(g_delta wdec), g_h1 = drop1'(g_h2 W2) and
//             g_xc = g_h1 W1 (columns [c0, K1)), which the head scatters into its input gradients.
// apg_gemm_kernel: 64 x 64 tile per workgroup of 4 waves (32 x 32 each), K in stages of 16 through LDS, v_mfma_f32_16x16x4_f32
// (exact fp32).  Every product reduces over K in index order inside ONE workgroup: no split, no atomics, so results are
// bit-reproducible, and a row's result depends only on that row (batch size and position do not change it).
#include "ap_common.h"
#include "grad_internal.h"

namespace {

constexpr int CS_ROWS = APG_CS_ROWS;     // rows per partial of the column sums

enum { EPI_STORE = APG_EPI_STORE, EPI_HID_FWD = APG_EPI_HID_FWD, EPI_DEC_FWD = APG_EPI_DEC_FWD, EPI_HID_BWD = APG_EPI_HID_BWD,
       EPI_DEC_LOCAL = APG_EPI_DEC_LOCAL };

typedef ApgGemmArgs GemmArgs;            // grad_internal.h

// A: AK = K contiguous (sak == 1), else M contiguous (sam == 1).  B: BN = N contiguous (sbn == 1), else K contiguous.
// The tile loaders map consecutive threads to consecutive addresses in either case.
template <bool AK, bool BN>
__global__ void __launch_bounds__(256) apg_gemm_kernel(const GemmArgs g) {
    __shared__ float As[16][80];         // [k][m]; row pitch 80: the 4 k rows an MFMA step reads fall on distinct banks
    __shared__ float Bs[16][80];         // [k][n]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
    const int i = lane & 15, q = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < g.K; k0 += 16) {
        if (AK) {
            const int m = t >> 2, kq = (t & 3) * 4, gm = m0 + m;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gk = k0 + kq + j;
                As[kq + j][m] = (gm < g.M && gk < g.K) ? g.A[(long long)gm * g.sam + gk] : 0.f;
            }
        } else {
            const int k = t >> 4, mq = (t & 15) * 4, gk = k0 + k;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gm = m0 + mq + j;
                As[k][mq + j] = (gm < g.M && gk < g.K) ? g.A[(long long)gk * g.sak + gm] : 0.f;
            }
        }
        if (BN) {
            const int k = t >> 4, nq = (t & 15) * 4, gk = k0 + k;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gn = n0 + nq + j;
                Bs[k][nq + j] = (gn < g.N && gk < g.K) ? g.B[(long long)gk * g.sbk + gn] : 0.f;
            }
        } else {
            const int n = t >> 2, kq = (t & 3) * 4, gn = n0 + n;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gk = k0 + kq + j;
                Bs[kq + j][n] = (gn < g.N && gk < g.K) ? g.B[(long long)gn * g.sbn + gk] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk += 4) {
            // 16x16x4 operand maps: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]
            const float a0 = As[kk + q][wm + i], a1 = As[kk + q][wm + 16 + i];
            const float b0 = Bs[kk + q][wn + i], b1 = Bs[kk + q][wn + 16 + i];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: col = l & 15, row = 4 (l >> 4) + reg
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm + 16 * a + 4 * q + e, col = n0 + wn + 16 * b + i;
                if (row >= g.M || col >= g.N) continue;
                float v = acc[a][b][e];
                if (g.epi == EPI_STORE) {
                    g.C[(long long)row * g.ldc + col] = v;
                } else if (g.epi == EPI_HID_FWD) {
                    v += g.bias[col];
                    g.C[(long long)row * g.ldc + col] = apg_keep(g.seed, g.layer, row, col, g.p) ? v * g.scale : 0.f;
                } else if (g.epi == EPI_HID_BWD) {
                    g.C[(long long)row * g.ldc + col] = apg_keep(g.seed, g.layer, row, col, g.p) ? v * g.scale : 0.f;
                } else if (g.epi == EPI_DEC_LOCAL) {
                    int d = 0;
                    while (d + 1 < g.ndec && col >= g.doff[d + 1]) ++d;
                    const int j = col - g.doff[d], nd = g.doff[d + 1] - g.doff[d];
                    g.dout[d][(long long)row * nd + j] = g.base[(long long)row * g.ldbase + g.dres[d] + j] + (v + g.bias[col]);
                } else {                                         // EPI_DEC_FWD
                    const int vw = row >= g.nb, bi = row - vw * g.nb;
                    float* o = vw ? g.out1 : g.out0;
                    o[(long long)bi * g.ldo + col] = g.base[(long long)row * g.ldbase + col] + (v + g.bias[col]);
                }
            }
}

// column sums, pass 1: part[chunk][c] = sum of rows [chunk * CS_ROWS, +CS_ROWS) in row order
__global__ void __launch_bounds__(256) colsum_part_kernel(const float* __restrict__ x, int rows, int cols, int ld,
                                                          float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    if (c >= cols) return;
    const int r0 = ch * CS_ROWS, r1 = min(r0 + CS_ROWS, rows);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += x[(long long)r * ld + c];
    part[(long long)ch * cols + c] = s;
}

// pass 2: out[c] = sum of the partials in chunk order
__global__ void __launch_bounds__(256) colsum_final_kernel(const float* __restrict__ part, int nch, int cols,
                                                           float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int ch = 0; ch < nch; ++ch) s += part[(long long)ch * cols + c];
    out[c] = s;
}

__global__ void __launch_bounds__(256) dropout_mask_kernel(uint64_t seed, int layer, int rows, int cols, float p,
                                                           uint8_t* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * cols) return;
    out[idx] = apg_keep(seed, layer, (int)(idx / cols), (int)(idx % cols), p) ? 1 : 0;
}

}  // namespace

ApgGemmArgs apg_gemm_args(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, int M,
                          int N, int K) {
    GemmArgs g = {};
    g.A = A; g.sam = sam; g.sak = sak;
    g.B = B; g.sbk = sbk; g.sbn = sbn;
    g.M = M; g.N = N; g.K = K;
    g.epi = EPI_STORE;
    g.p = 0.f; g.scale = 1.f;
    return g;
}

hipError_t apg_gemm_launch(const ApgGemmArgs& g, hipStream_t st) {
    const dim3 grid((g.N + 63) / 64, (g.M + 63) / 64), block(256);
    const bool ak = g.sak == 1, bn = g.sbn == 1;
    if (ak && bn) hipLaunchKernelGGL((apg_gemm_kernel<true, true>), grid, block, 0, st, g);
    else if (ak) hipLaunchKernelGGL((apg_gemm_kernel<true, false>), grid, block, 0, st, g);
    else if (bn) hipLaunchKernelGGL((apg_gemm_kernel<false, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((apg_gemm_kernel<false, false>), grid, block, 0, st, g);
    return hipGetLastError();
}

void apg_gemm_set_dropout(ApgGemmArgs& g, int epi, uint64_t seed, int layer, float p) {
    g.epi = epi;
    g.seed = seed;
    g.layer = layer;
    g.p = p > 0.f ? p : 0.f;
    g.scale = p <= 0.f ? 1.f : (p < 1.f ? 1.f / (1.f - p) : 0.f);
}

hipError_t apg_colsum(const float* x, int rows, int cols, int ld, float* part, float* out, hipStream_t st) {
    const int nch = (rows + CS_ROWS - 1) / CS_ROWS;
    hipLaunchKernelGGL(colsum_part_kernel, dim3((cols + 255) / 256, nch), dim3(256), 0, st, x, rows, cols, ld, part);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, part, nch, cols, out);
    return hipGetLastError();
}

ApgChainLayout apg_chain_layout(size_t R, int K1, int N, int need_gxf) {
    ApgChainLayout l;
    l.c0 = need_gxf ? 0 : XF;
    size_t o = 0;
    l.gd = o;   o += al64(R * N);
    l.gh2 = o;  o += al64(R * HID);
    l.gh1 = o;  o += al64(R * HID);
    l.gxc = o;  o += al64(R * (K1 - l.c0));
    l.part = o; o += al64(((R + CS_ROWS - 1) / CS_ROWS) * HID);
    l.total = o;
    return l;
}

int apg_head_hidden_fwd(int R, int K1, const float* xc, const float* W1, const float* b1, const float* W2, const float* b2,
                        uint64_t seed, float p1, float p2, float* h1d, float* h2d, hipStream_t st) {
    GemmArgs g = apg_gemm_args(xc, K1, 1, W1, 1, K1, R, HID, K1);                // h1 = xc W1^T
    apg_gemm_set_dropout(g, EPI_HID_FWD, seed, 1, p1);
    g.bias = b1; g.C = h1d; g.ldc = HID;
    APG_TRY(apg_gemm_launch(g, st));
    g = apg_gemm_args(h1d, HID, 1, W2, 1, HID, R, HID, HID);                     // h2 = h1d W2^T
    apg_gemm_set_dropout(g, EPI_HID_FWD, seed, 2, p2);
    g.bias = b2; g.C = h2d; g.ldc = HID;
    APG_TRY(apg_gemm_launch(g, st));
    return APG_OK;
}

int apg_head_chain_bwd(const ApgChainBwd& c, const ApgChainLayout& l, float* ws, hipStream_t st) {
    const int R = c.R, K1 = c.K1, N = c.N;
    float *gd = ws + l.gd, *gh2 = ws + l.gh2, *gh1 = ws + l.gh1, *gxc = ws + l.gxc, *part = ws + l.part;
    float* const* gp = (float* const*)c.g_param;
    // decoders: g_W_d = g_delta_d^T h2d, g_b_d = column sums of g_delta_d
    for (int e = 0; e < c.ndec; ++e) {
        const int off = c.doff[e], n = c.doff[e + 1] - off;
        if (gp[4 + 2 * e]) {
            GemmArgs g = apg_gemm_args(gd + off, 1, N, c.h2d, HID, 1, n, HID, R);
            g.C = gp[4 + 2 * e]; g.ldc = HID;
            APG_TRY(apg_gemm_launch(g, st));
        }
        if (gp[5 + 2 * e]) APG_TRY(apg_colsum(gd + off, R, n, N, part, gp[5 + 2 * e], st));
    }
    // g_h2 = drop2'(g_delta wdec)
    GemmArgs g = apg_gemm_args(gd, N, 1, c.wdec, HID, 1, R, HID, N);
    apg_gemm_set_dropout(g, EPI_HID_BWD, c.seed, 2, c.p2);
    g.C = gh2; g.ldc = HID;
    APG_TRY(apg_gemm_launch(g, st));
    if (gp[2]) {
        g = apg_gemm_args(gh2, 1, HID, c.h1d, HID, 1, HID, HID, R);              // g_W2 = g_h2^T h1d
        g.C = gp[2]; g.ldc = HID;
        APG_TRY(apg_gemm_launch(g, st));
    }
    if (gp[3]) APG_TRY(apg_colsum(gh2, R, HID, HID, part, gp[3], st));
    // g_h1 = drop1'(g_h2 W2)
    g = apg_gemm_args(gh2, HID, 1, c.W2, HID, 1, R, HID, HID);
    apg_gemm_set_dropout(g, EPI_HID_BWD, c.seed, 1, c.p1);
    g.C = gh1; g.ldc = HID;
    APG_TRY(apg_gemm_launch(g, st));
    if (gp[0]) {
        g = apg_gemm_args(gh1, 1, HID, c.xc, K1, 1, HID, K1, R);                 // g_W1 = g_h1^T xc
        g.C = gp[0]; g.ldc = K1;
        APG_TRY(apg_gemm_launch(g, st));
    }
    if (gp[1]) APG_TRY(apg_colsum(gh1, R, HID, HID, part, gp[1], st));
    if (c.want_gxc) {
        const int nc = K1 - l.c0;
        g = apg_gemm_args(gh1, HID, 1, c.W1 + l.c0, K1, 1, R, nc, HID);          // g_xc[:, c0:] = g_h1 W1[:, c0:]
        g.C = gxc; g.ldc = nc;
        APG_TRY(apg_gemm_launch(g, st));
    }
    return APG_OK;
}

extern "C" {

int apg_dropout_mask(uint64_t seed, int layer, int rows, int cols, float p, uint8_t* out, void* stream) {
    if (!out || rows <= 0 || cols <= 0) return apg_fail(APG_EINVAL, "apg_dropout_mask: bad argument");
    const long long n = (long long)rows * cols;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, layer,
                       rows, cols, p, out);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
