// IEF regressor head forward / backward for gfx950 (libairpose_grad.so): copenet.forward_reg on live fp32 weights, both views in
// one pass of R = 2B rows, and its adjoint.
//   forward:  head_pack_kernel (the fc1 input xc: features | state | partner's art and shape, a snapshot kept for backward),
//             then three products on apg_gemm_kernel: fc1 (+ bias, drop1), fc2 (+ bias, drop2), decpose / decshape (+ bias
//             and the residual, written straight into the per-view outputs)
//   backward: head_pack_gd_kernel (g_delta from the per-view output gradients), head_pack_wdec_kernel ([Wpose; Wshape]);
//             g_h2 = drop2'(g_delta Wdec), g_h1 = drop1'(g_h2 W2), g_xc = g_h1 W1 (state columns, + features on request);
//             weight gradients g_delta^T h2d, g_h2^T h1d, g_h1^T xc; bias gradients as column sums (two fixed-order passes);
//             head_scatter_kernel adds own columns + partner's fusion columns + residual identity into the input gradients.
// apg_gemm_kernel: 64 x 64 tile per workgroup of 4 waves (32 x 32 each), K in stages of 16 through LDS, v_mfma_f32_16x16x4_f32
// (exact fp32).  Every product reduces over K in index order inside ONE workgroup: no split, no atomics, so results are
// bit-reproducible, and a row's result depends only on that row (batch size and position do not change it).
#include "ap_common.h"
#include "grad_internal.h"

#include <string>

namespace {

constexpr int XC = 2332;                 // fc1 input width
constexpr int XF = 2048;                 // trunk features
constexpr int HID = 1024;
constexpr int NPOSE = 135, NSHAPE = 10, NDEC = NPOSE + NSHAPE;
constexpr int CS_ROWS = APG_CS_ROWS;     // rows per partial of the column sums

// state inputs of one view: bb, pos, orient, art, shape (column offsets inside the 284 state columns)
__constant__ const int k_st_off[5] = {0, 3, 6, 12, 138};
__constant__ const int k_st_w[5] = {3, 3, 6, 126, 10};

struct StatePtrs {
    const float* p[2][5];
    int ld[2][5];
};

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

// xc[r] = [xf_v[b] | bb | pos | orient | art | shape | partner art | partner shape], r = v * B + b
__global__ void __launch_bounds__(256) head_pack_kernel(const float* __restrict__ xf0, const float* __restrict__ xf1,
                                                        const StatePtrs s, int B, float* __restrict__ xc) {
    const int r = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= XC) return;
    const int v = r >= B, b = r - v * B;
    float val;
    if (c < XF) {
        val = (v ? xf1 : xf0)[(long long)b * XF + c];
    } else {
        int sc = c - XF, src = v, idx;
        if (sc >= 274) { src = 1 - v; idx = 4; sc -= 274; }
        else if (sc >= 148) { src = 1 - v; idx = 3; sc -= 148; }
        else { idx = 0; while (idx < 4 && sc >= k_st_off[idx + 1]) ++idx; sc -= k_st_off[idx]; }
        val = s.p[src][idx][(long long)b * s.ld[src][idx] + sc];
    }
    xc[(long long)r * XC + c] = val;
}

// g_delta[r][n] (R x 145) from the per-view output gradients (NULL = zero)
__global__ void __launch_bounds__(256) head_pack_gd_kernel(const float* __restrict__ gp0, const float* __restrict__ gs0,
                                                           const float* __restrict__ gp1, const float* __restrict__ gs1, int B,
                                                           float* __restrict__ gd) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2LL * B * NDEC) return;
    const int r = (int)(idx / NDEC), n = (int)(idx % NDEC);
    const int v = r >= B, b = r - v * B;
    const float* src = n < NPOSE ? (v ? gp1 : gp0) : (v ? gs1 : gs0);
    gd[idx] = src ? (n < NPOSE ? src[(long long)b * NPOSE + n] : src[(long long)b * NSHAPE + n - NPOSE]) : 0.f;
}

__global__ void __launch_bounds__(256) head_pack_wdec_kernel(const float* __restrict__ wp, const float* __restrict__ ws,
                                                             float* __restrict__ wdec) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= NDEC * HID) return;
    wdec[idx] = idx < NPOSE * HID ? wp[idx] : ws[idx - NPOSE * HID];
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

struct GradIn {
    float* g[2][6];                      // xf, bb, pos, orient, art, shape per view
    const float* gpose[2];
    const float* gbetas[2];
};

// input gradients of state column / feature c of row r: own column + (art, shape) the partner row's fusion column + residual.
// gxc holds columns [c0, 2332) of g_xc, row pitch ldg.
__global__ void __launch_bounds__(256) head_scatter_kernel(const float* __restrict__ gxc, int ldg, int c0, int B, const GradIn gi) {
    const int r = blockIdx.x, c = c0 + blockIdx.y * 256 + threadIdx.x;
    if (c >= XF + 148) return;                           // partner columns are gathered by the partner's own row
    const int v = r >= B, b = r - v * B, rp = (1 - v) * B + b;
    const long long own = (long long)r * ldg - c0, par = (long long)rp * ldg - c0;     // + column index >= c0
    if (c < XF) {
        float* o = gi.g[v][0];
        if (o) o[(long long)b * XF + c] = gxc[own + c];
        return;
    }
    const int sc = c - XF;
    int idx = 0;
    while (idx < 4 && sc >= k_st_off[idx + 1]) ++idx;
    float* o = gi.g[v][idx + 1];
    if (!o) return;
    const int j = sc - k_st_off[idx];
    float val = gxc[own + c];
    if (idx == 3) val += gxc[par + XF + 148 + j];
    if (idx == 4) val += gxc[par + XF + 274 + j];
    if (idx >= 1 && idx <= 3 && gi.gpose[v]) val += gi.gpose[v][(long long)b * NPOSE + sc - 3];
    if (idx == 4 && gi.gbetas[v]) val += gi.gbetas[v][(long long)b * NSHAPE + j];
    o[(long long)b * k_st_w[idx] + j] = val;
}

__global__ void __launch_bounds__(256) dropout_mask_kernel(uint64_t seed, int layer, int rows, int cols, float p,
                                                           uint8_t* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * cols) return;
    out[idx] = apg_keep(seed, layer, (int)(idx / cols), (int)(idx % cols), p) ? 1 : 0;
}

GemmArgs gemm_args(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, int M, int N,
                   int K) {
    GemmArgs g = {};
    g.A = A; g.sam = sam; g.sak = sak;
    g.B = B; g.sbk = sbk; g.sbn = sbn;
    g.M = M; g.N = N; g.K = K;
    g.epi = EPI_STORE;
    g.p = 0.f; g.scale = 1.f;
    return g;
}

hipError_t launch_gemm(const GemmArgs& g, hipStream_t st) {
    const dim3 grid((g.N + 63) / 64, (g.M + 63) / 64), block(256);
    const bool ak = g.sak == 1, bn = g.sbn == 1;
    if (ak && bn) hipLaunchKernelGGL((apg_gemm_kernel<true, true>), grid, block, 0, st, g);
    else if (ak) hipLaunchKernelGGL((apg_gemm_kernel<true, false>), grid, block, 0, st, g);
    else if (bn) hipLaunchKernelGGL((apg_gemm_kernel<false, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((apg_gemm_kernel<false, false>), grid, block, 0, st, g);
    return hipGetLastError();
}

void set_dropout(GemmArgs& g, int epi, uint64_t seed, int layer, float p) {
    g.epi = epi;
    g.seed = seed;
    g.layer = layer;
    g.p = p > 0.f ? p : 0.f;
    g.scale = p <= 0.f ? 1.f : (p < 1.f ? 1.f / (1.f - p) : 0.f);
}

hipError_t colsum(const float* x, int rows, int cols, int ld, float* part, float* out, hipStream_t st) {
    const int nch = (rows + CS_ROWS - 1) / CS_ROWS;
    hipLaunchKernelGGL(colsum_part_kernel, dim3((cols + 255) / 256, nch), dim3(256), 0, st, x, rows, cols, ld, part);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, part, nch, cols, out);
    return hipGetLastError();
}

size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

// workspace layout of apg_head_bwd, in floats
struct BwdLayout {
    size_t gd, wdec, gh2, gh1, gxc, part, total;
    int c0;
};

BwdLayout bwd_layout(int B, int need_gxf) {
    const size_t R = 2 * (size_t)B;
    BwdLayout l;
    l.c0 = need_gxf ? 0 : XF;
    size_t o = 0;
    l.gd = o;   o += align64(R * NDEC);
    l.wdec = o; o += align64((size_t)NDEC * HID);
    l.gh2 = o;  o += align64(R * HID);
    l.gh1 = o;  o += align64(R * HID);
    l.gxc = o;  o += align64(R * (XC - l.c0));
    l.part = o; o += align64(((R + CS_ROWS - 1) / CS_ROWS) * HID);
    l.total = o;
    return l;
}

}  // namespace

// the product, its dropout epilogues and the column sums for the library's other sources (grad_internal.h)
ApgGemmArgs apg_gemm_args(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, int M,
                          int N, int K) {
    return gemm_args(A, sam, sak, B, sbk, sbn, M, N, K);
}
void apg_gemm_set_dropout(ApgGemmArgs& g, int epi, uint64_t seed, int layer, float p) { set_dropout(g, epi, seed, layer, p); }
hipError_t apg_gemm_launch(const ApgGemmArgs& g, hipStream_t st) { return launch_gemm(g, st); }
hipError_t apg_colsum(const float* x, int rows, int cols, int ld, float* part, float* out, hipStream_t st) {
    return colsum(x, rows, cols, ld, part, out, st);
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

int apg_head_fwd(int B, const float* xf0, const float* xf1, const void* const* state, const int* state_ld,
                 const float* W1, const float* b1, const float* W2, const float* b2, const float* Wpose, const float* bpose,
                 const float* Wshape, const float* bshape, uint64_t seed, float p1, float p2,
                 float* xc, float* h1d, float* h2d, void* const* pose_out, void* const* betas_out, void* stream) {
    if (B <= 0 || !xf0 || !xf1 || !state || !state_ld || !W1 || !b1 || !W2 || !b2 || !Wpose || !bpose || !Wshape || !bshape ||
        !xc || !h1d || !h2d || !pose_out || !betas_out || !pose_out[0] || !pose_out[1] || !betas_out[0] || !betas_out[1])
        return apg_fail(APG_EINVAL, "apg_head_fwd: bad argument");
    StatePtrs s;
    for (int v = 0; v < 2; ++v)
        for (int k = 0; k < 5; ++k) {
            s.p[v][k] = (const float*)state[v * 5 + k];
            s.ld[v][k] = state_ld[v * 5 + k];
            if (!s.p[v][k] || s.ld[v][k] < 0) return apg_fail(APG_EINVAL, "apg_head_fwd: state input missing");
        }
    hipStream_t st = (hipStream_t)stream;
    const int R = 2 * B;
    hipLaunchKernelGGL(head_pack_kernel, dim3(R, (XC + 255) / 256), dim3(256), 0, st, xf0, xf1, s, B, xc);
    APG_TRY(hipGetLastError());
    GemmArgs g = gemm_args(xc, XC, 1, W1, 1, XC, R, HID, XC);           // h1 = xc W1^T
    set_dropout(g, EPI_HID_FWD, seed, 1, p1);
    g.bias = b1; g.C = h1d; g.ldc = HID;
    APG_TRY(launch_gemm(g, st));
    g = gemm_args(h1d, HID, 1, W2, 1, HID, R, HID, HID);                 // h2 = h1d W2^T
    set_dropout(g, EPI_HID_FWD, seed, 2, p2);
    g.bias = b2; g.C = h2d; g.ldc = HID;
    APG_TRY(launch_gemm(g, st));
    for (int part = 0; part < 2; ++part) {                               // pose = [pos|orient|art] + dec; betas = shape + dec
        g = gemm_args(h2d, HID, 1, part ? Wshape : Wpose, 1, HID, R, part ? NSHAPE : NPOSE, HID);
        g.epi = EPI_DEC_FWD;
        g.bias = part ? bshape : bpose;
        g.nb = B;
        g.out0 = (float*)(part ? betas_out : pose_out)[0];
        g.out1 = (float*)(part ? betas_out : pose_out)[1];
        g.ldo = part ? NSHAPE : NPOSE;
        g.base = xc + XF + (part ? 138 : 3);
        g.ldbase = XC;
        APG_TRY(launch_gemm(g, st));
    }
    return APG_OK;
}

int64_t apg_head_bwd_workspace_bytes(int B, int need_gxf) {
    if (B <= 0) return -1;
    return (int64_t)(bwd_layout(B, need_gxf).total * sizeof(float));
}

int apg_head_bwd(int B, const float* xc, const float* h1d, const float* h2d, const float* W1, const float* W2,
                 const float* Wpose, const float* Wshape, uint64_t seed, float p1, float p2, const void* const* g_out,
                 void* const* g_param, void* const* g_in, void* workspace, int64_t workspace_bytes, void* stream) {
    if (B <= 0 || !xc || !h1d || !h2d || !W1 || !W2 || !Wpose || !Wshape || !g_out || !g_param || !g_in || !workspace)
        return apg_fail(APG_EINVAL, "apg_head_bwd: bad argument");
    const int need_gxf = g_in[0] || g_in[6];
    const BwdLayout l = bwd_layout(B, need_gxf);
    if (workspace_bytes < (int64_t)(l.total * sizeof(float)))
        return apg_fail(APG_ENOMEM, "apg_head_bwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(l.total * sizeof(float)) + " needed");
    hipStream_t st = (hipStream_t)stream;
    const int R = 2 * B;
    float* ws = (float*)workspace;
    float *gd = ws + l.gd, *wdec = ws + l.wdec, *gh2 = ws + l.gh2, *gh1 = ws + l.gh1, *gxc = ws + l.gxc, *part = ws + l.part;
    float* gp[8];
    for (int k = 0; k < 8; ++k) gp[k] = (float*)g_param[k];

    const long long ngd = (long long)R * NDEC;
    hipLaunchKernelGGL(head_pack_gd_kernel, dim3((unsigned)((ngd + 255) / 256)), dim3(256), 0, st, (const float*)g_out[0],
                       (const float*)g_out[1], (const float*)g_out[2], (const float*)g_out[3], B, gd);
    hipLaunchKernelGGL(head_pack_wdec_kernel, dim3((NDEC * HID + 255) / 256), dim3(256), 0, st, Wpose, Wshape, wdec);
    APG_TRY(hipGetLastError());
    // decpose / decshape: g_W = g_delta^T h2d, g_b = column sums of g_delta
    for (int d = 0; d < 2; ++d) {
        const int off = d ? NPOSE : 0, n = d ? NSHAPE : NPOSE;
        if (gp[4 + 2 * d]) {
            GemmArgs g = gemm_args(gd + off, 1, NDEC, h2d, HID, 1, n, HID, R);
            g.C = gp[4 + 2 * d]; g.ldc = HID;
            APG_TRY(launch_gemm(g, st));
        }
        if (gp[5 + 2 * d]) APG_TRY(colsum(gd + off, R, n, NDEC, part, gp[5 + 2 * d], st));
    }
    // g_h2 = drop2'(g_delta Wdec)
    GemmArgs g = gemm_args(gd, NDEC, 1, wdec, HID, 1, R, HID, NDEC);
    set_dropout(g, EPI_HID_BWD, seed, 2, p2);
    g.C = gh2; g.ldc = HID;
    APG_TRY(launch_gemm(g, st));
    if (gp[2]) {
        g = gemm_args(gh2, 1, HID, h1d, HID, 1, HID, HID, R);            // g_W2 = g_h2^T h1d
        g.C = gp[2]; g.ldc = HID;
        APG_TRY(launch_gemm(g, st));
    }
    if (gp[3]) APG_TRY(colsum(gh2, R, HID, HID, part, gp[3], st));
    // g_h1 = drop1'(g_h2 W2)
    g = gemm_args(gh2, HID, 1, W2, HID, 1, R, HID, HID);
    set_dropout(g, EPI_HID_BWD, seed, 1, p1);
    g.C = gh1; g.ldc = HID;
    APG_TRY(launch_gemm(g, st));
    if (gp[0]) {
        g = gemm_args(gh1, 1, HID, xc, XC, 1, HID, XC, R);               // g_W1 = g_h1^T xc
        g.C = gp[0]; g.ldc = XC;
        APG_TRY(launch_gemm(g, st));
    }
    if (gp[1]) APG_TRY(colsum(gh1, R, HID, HID, part, gp[1], st));
    bool any_in = false;
    for (int k = 0; k < 12; ++k) any_in = any_in || g_in[k];
    if (any_in) {
        const int nc = XC - l.c0;
        g = gemm_args(gh1, HID, 1, W1 + l.c0, XC, 1, R, nc, HID);         // g_xc[:, c0:] = g_h1 W1[:, c0:]
        g.C = gxc; g.ldc = nc;
        APG_TRY(launch_gemm(g, st));
        GradIn gi;
        for (int v = 0; v < 2; ++v) {
            for (int k = 0; k < 6; ++k) gi.g[v][k] = (float*)g_in[v * 6 + k];
            gi.gpose[v] = (const float*)g_out[2 * v];
            gi.gbetas[v] = (const float*)g_out[2 * v + 1];
        }
        hipLaunchKernelGGL(head_scatter_kernel, dim3(R, (XF + 148 - l.c0 + 255) / 256), dim3(256), 0, st, gxc, nc, l.c0, B, gi);
        APG_TRY(hipGetLastError());
    }
    return APG_OK;
}

}  // extern "C"
