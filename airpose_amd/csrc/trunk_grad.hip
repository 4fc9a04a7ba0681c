// ResNet-50 trunk forward / backward for gfx950 (libairpose_grad.so): copenet.forward_feat_ext (model_copenet.py:161-176) on live
// fp32 parameters, in train-mode (batch statistics, running-stat update) or eval-mode BatchNorm, and its adjoint.
//   convolution:  apg_conv_kernel, an implicit GEMM on NHWC fp32 activations and the OIHW fp32 weights as they are, 64 x 64 tile
//                 per workgroup of 4 waves, K in stages of 16 through LDS, v_mfma_f32_16x16x4_f32 (exact fp32):
//                   CV_FWD    M = n Ho Wo, N = C_out, K = (r, s, c_in)
//                   CV_DGRAD  M = n H W,   N = C_in,  K = (r, s, c_out), a gather with per-tap validity (stride 2 included)
//                   CV_WGRAD  M = C_out,   N = (r, s, c_in), K = n Ho Wo in fixed split-K chunks; wgrad_combine_kernel
//                             sums the chunks in chunk order straight into the OIHW gradient
// Everything else is trunk_elem.inc, the one source this file shares with trunk_grad_bf16.hip, instantiated on F32Store (fp32
// storage, one channel per thread):
//   BatchNorm:    per-channel statistics over the n H W rows as per-tile centred partials (mean, M2: bn_stats_part_kernel) combined
//                 by Chan's formula in a fixed tree (bn_stats_final_kernel; eval mode: bn_eval_stats_kernel); normalise + affine
//                 (+ residual) (+ ReLU) in one pass (bn_apply_kernel); backward with the ReLU mask and the residual split fused in
//                 (bn_bwd_part_kernel, bn_bwd_final_kernel, bn_bwd_apply_kernel)
//   pools:        max-pool 3 x 3 / s2 / p1 (padding = -inf, the first maximum in row-major window order takes the gradient, as in
//                 torch: maxpool_fwd_kernel, maxpool_bwd_kernel) and avg-pool 7 x 7 (avgpool_fwd_kernel, avgpool_bwd_kernel),
//                 forward and backward as gathers
//   layout:       wgrad_combine_kernel; nhwc_to_nchw_kernel for the crop gradient
// No floating-point atomics anywhere: every reduction runs in a fixed order, so results are bit-reproducible run to run.
#include "ap_common.h"
#include "grad_internal.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

enum { CV_FWD = 0, CV_DGRAD = 1, CV_WGRAD = 2 };

struct ConvArgs {
    const float* x;                      // CV_FWD / CV_WGRAD: input (n, H, W, C)
    const float* w;                      // CV_FWD / CV_DGRAD: weight (K, C, R, S)
    const float* gy;                     // CV_DGRAD / CV_WGRAD: output gradient (n, Ho, Wo, K)
    float* out;                          // CV_FWD: y (n, Ho, Wo, K); CV_DGRAD: gx (n, H, W, C); CV_WGRAD: chunk partials
    const float* add;                    // CV_DGRAD: out = acc + add (same index; may alias out)
    int n, H, W, C, K, R, S, st, pad, Ho, Wo;
    int M, N, KK;                        // GEMM sizes
    int kchunk;                          // CV_WGRAD: pixels per chunk (multiple of 16)
};

// FAST: a stage of 16 k (CV_FWD) or the 64 columns of a tile (CV_WGRAD) lie inside one filter tap, so the channels are contiguous
// and the loaders read float4 (C % 16 == 0 resp. C % 64 == 0).  CV_DGRAD always runs FAST (K % 16 == 0 is an argument check).
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) apg_conv_kernel(const ConvArgs a) {
    __shared__ float As[16][80];         // [k][m]; row pitch 80: the 4 k rows an MFMA step reads fall on distinct banks
    __shared__ float Bs[16][80];         // [k][n]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;      // M tiles on x: n H W / 64 can pass 65535
    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
    const int i = lane & 15, q = lane >> 4;
    int kbeg = 0, kend = a.KK;
    if (MODE == CV_WGRAD) {
        kbeg = blockIdx.z * a.kchunk;
        kend = min(kbeg + a.kchunk, a.KK);
    }
    // CV_FWD / CV_DGRAD: the A loader's row m = m0 + t / 4 is fixed for the whole kernel
    const int am = m0 + (t >> 2);
    const bool am_ok = am < a.M;
    int ab = 0, ah = 0, aw = 0;
    if (MODE == CV_FWD && am_ok) {
        ab = am / (a.Ho * a.Wo);
        const int rem = am - ab * a.Ho * a.Wo;
        ah = rem / a.Wo;
        aw = rem - ah * a.Wo;
    } else if (MODE == CV_DGRAD && am_ok) {
        ab = am / (a.H * a.W);
        const int rem = am - ab * a.H * a.W;
        ah = rem / a.W;
        aw = rem - ah * a.W;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
        if (MODE == CV_FWD) {
            const int kq = (t & 3) * 4;
            if (FAST) {
                const int tap = k0 / a.C, cb = k0 - tap * a.C + kq, r = tap / a.S, s = tap - r * a.S;
                const int h = ah * a.st - a.pad + r, w = aw * a.st - a.pad + s;
                if (am_ok && h >= 0 && h < a.H && w >= 0 && w < a.W) {
                    const float4 f = *(const float4*)(a.x + (((long long)ab * a.H + h) * a.W + w) * a.C + cb);
                    va[0] = f.x; va[1] = f.y; va[2] = f.z; va[3] = f.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int gk = k0 + kq + j;
                    if (!am_ok || gk >= kend) continue;
                    const int tap = gk / a.C, c = gk - tap * a.C, r = tap / a.S, s = tap - r * a.S;
                    const int h = ah * a.st - a.pad + r, w = aw * a.st - a.pad + s;
                    if (h >= 0 && h < a.H && w >= 0 && w < a.W) va[j] = a.x[(((long long)ab * a.H + h) * a.W + w) * a.C + c];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) As[kq + j][t >> 2] = va[j];
            // B(k, co) = w[co][c][r][s]
            const int nl = t >> 2, co = n0 + nl;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gk = k0 + kq + j;
                if (co >= a.N || gk >= kend) continue;
                const int tap = gk / a.C, c = gk - tap * a.C, r = tap / a.S, s = tap - r * a.S;
                vb[j] = a.w[(((long long)co * a.C + c) * a.R + r) * a.S + s];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) Bs[kq + j][nl] = vb[j];
        } else if (MODE == CV_DGRAD) {
            const int kq = (t & 3) * 4;
            const int tap = k0 / a.K, cb = k0 - tap * a.K + kq, r = tap / a.S, s = tap - r * a.S;
            const int th = ah + a.pad - r, tw = aw + a.pad - s;
            if (am_ok && th >= 0 && tw >= 0 && th % a.st == 0 && tw % a.st == 0) {
                const int ho = th / a.st, wo = tw / a.st;
                if (ho < a.Ho && wo < a.Wo) {
                    const float4 f = *(const float4*)(a.gy + (((long long)ab * a.Ho + ho) * a.Wo + wo) * a.K + cb);
                    va[0] = f.x; va[1] = f.y; va[2] = f.z; va[3] = f.w;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) As[kq + j][t >> 2] = va[j];
            // B(k = (r, s, co), c) = w[co][c][r][s]
            const int kk = t >> 4, nq = (t & 15) * 4, gk = k0 + kk;
            const int btap = gk / a.K, co = gk - btap * a.K, br = btap / a.S, bs = btap - br * a.S;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = n0 + nq + j;
                if (c < a.N) vb[j] = a.w[(((long long)co * a.C + c) * a.R + br) * a.S + bs];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) Bs[kk][nq + j] = vb[j];
        } else {                                                 // CV_WGRAD
            const int kk = t >> 4, nq = (t & 15) * 4, pix = k0 + kk;
            const bool pk = pix < kend;
            if (pk && m0 + nq < a.M) {                           // A(co, pix) = gy[pix][co]; K % 4 == 0
                const float4 f = *(const float4*)(a.gy + (long long)pix * a.K + m0 + nq);
                va[0] = f.x; va[1] = f.y; va[2] = f.z; va[3] = f.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) As[kk][nq + j] = va[j];
            if (pk) {                                            // B(pix, (r, s, c)) = x[b][h][w][c]
                const int b = pix / (a.Ho * a.Wo), rem = pix - b * a.Ho * a.Wo, ho = rem / a.Wo, wo = rem - ho * a.Wo;
                if (FAST) {
                    const int tap = n0 / a.C, cb = n0 - tap * a.C + nq, r = tap / a.S, s = tap - r * a.S;
                    const int h = ho * a.st - a.pad + r, w = wo * a.st - a.pad + s;
                    if (h >= 0 && h < a.H && w >= 0 && w < a.W) {
                        const float4 f = *(const float4*)(a.x + (((long long)b * a.H + h) * a.W + w) * a.C + cb);
                        vb[0] = f.x; vb[1] = f.y; vb[2] = f.z; vb[3] = f.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int nn = n0 + nq + j;
                        if (nn >= a.N) continue;
                        const int tap = nn / a.C, c = nn - tap * a.C, r = tap / a.S, s = tap - r * a.S;
                        const int h = ho * a.st - a.pad + r, w = wo * a.st - a.pad + s;
                        if (h >= 0 && h < a.H && w >= 0 && w < a.W) vb[j] = a.x[(((long long)b * a.H + h) * a.W + w) * a.C + c];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) Bs[kk][nq + j] = vb[j];
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
    float* out = a.out;
    if (MODE == CV_WGRAD) out += (long long)blockIdx.z * a.M * a.N;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm + 16 * x + 4 * q + e, col = n0 + wn + 16 * y + i;
                if (row >= a.M || col >= a.N) continue;
                const long long o = (long long)row * a.N + col;
                float v = acc[x][y][e];
                if (MODE == CV_DGRAD && a.add) v = a.add[o] + v;
                out[o] = v;
            }
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm, pools
// fp32 storage for the kernels of trunk_elem.inc: one channel per thread, 4-byte accesses (no alignment demand beyond the float's)
struct F32Store {
    using T = float;
    static constexpr int W = 1;
    struct V {
        float v[1];
    };
    static __device__ __forceinline__ float rd(float x) { return x; }
    static __device__ __forceinline__ V ld(const float* p) { return V{{*p}}; }
    static __device__ __forceinline__ void st(float* p, const V& f) { *p = f.v[0]; }
};
#include "trunk_elem.inc"

// NCHW -> NHWC of the (n, 3, 224, 224) crops
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, int n, int C, int HW, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * C * HW) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int hw = (int)(p % HW), b = (int)(p / HW);
    y[idx] = x[((long long)b * C + c) * HW + hw];
}

// ---------------------------------------------------------------------------------------------------------------- host side
#include "trunk_walk.inc"

// split-K of the weight gradient: enough chunks for ~1024 workgroups, chunks of at least 512 pixels (a multiple of 16)
void wgrad_split(const Geom& g, int* nch, int* chunk) {
    const int M = g.K, N = g.R * g.S * g.C, KK = g.n * g.Ho * g.Wo;
    const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
    int s = std::max(1, std::min((1024 + tiles - 1) / tiles, (KK + 511) / 512));
    int ch = (KK + s - 1) / s;
    ch = (ch + 15) & ~15;
    *chunk = ch;
    *nch = (KK + ch - 1) / ch;
}

hipError_t conv_fwd(const Geom& g, const float* x, const float* w, float* y, hipStream_t st) {
    ConvArgs a = conv_args<ConvArgs>(g);
    a.x = x; a.w = w; a.out = y;
    a.M = g.n * g.Ho * g.Wo; a.N = g.K; a.KK = g.R * g.S * g.C;
    const dim3 grid((a.M + 63) / 64, (a.N + 63) / 64);
    if (g.C % 16 == 0 && al16(x)) hipLaunchKernelGGL((apg_conv_kernel<CV_FWD, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((apg_conv_kernel<CV_FWD, false>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// gx = dgrad(gy) (+ add); needs K % 16 == 0 and gy 16-byte aligned (argument checks)
hipError_t conv_dgrad(const Geom& g, const float* gy, const float* w, const float* add, float* gx, hipStream_t st) {
    ConvArgs a = conv_args<ConvArgs>(g);
    a.gy = gy; a.w = w; a.out = gx; a.add = add;
    a.M = g.n * g.H * g.W; a.N = g.C; a.KK = g.R * g.S * g.K;
    hipLaunchKernelGGL((apg_conv_kernel<CV_DGRAD, true>), dim3((a.M + 63) / 64, (a.N + 63) / 64), dim3(256), 0, st, a);
    return hipGetLastError();
}

// gw (OIHW) = wgrad, through `part` (wgrad_floats(g) floats)
hipError_t conv_wgrad(const Geom& g, const float* x, const float* gy, float* part, float* gw, hipStream_t st) {
    ConvArgs a = conv_args<ConvArgs>(g);
    a.x = x; a.gy = gy; a.out = part;
    a.M = g.K; a.N = g.R * g.S * g.C; a.KK = g.n * g.Ho * g.Wo;
    int nch;
    wgrad_split(g, &nch, &a.kchunk);
    const dim3 grid((a.M + 63) / 64, (a.N + 63) / 64, nch);
    if (g.C % 64 == 0 && al16(x)) hipLaunchKernelGGL((apg_conv_kernel<CV_WGRAD, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((apg_conv_kernel<CV_WGRAD, false>), grid, dim3(256), 0, st, a);
    const long long tot = (long long)g.K * g.C * g.R * g.S;
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(nblk(tot)), dim3(256), 0, st, part, nch, g.K, g.C, g.C, g.R, g.S, gw);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- the trunk walks
// The fp32 backend of trunk_walk.inc: NHWC fp32 activations, the live OIHW parameters as the weights (nothing packed, no padding).
struct F32Ops : ElemOps<F32Store> {
    using L = Layer<float>;
    static constexpr const char *fwd_name = "apg_trunk_fwd", *bwd_name = "apg_trunk_bwd";
    static constexpr bool ws_aligned = false, packed = false;
    static int cpad(int C) { return C; }
    static void pack(const L&, const float*, hipStream_t) {}
    static hipError_t conv_fwd(const L& l, const float* w, hipStream_t st) { return ::conv_fwd(l.g, l.in, w, l.z, st); }
    static hipError_t conv_dgrad(const L& l, const float* gy, const float* w, const float* add, float* gx, hipStream_t st) {
        return ::conv_dgrad(l.g, gy, w, add, gx, st);
    }
    static hipError_t conv_wgrad(const L& l, const float* gz, float* part, float* gw, hipStream_t st) {
        return ::conv_wgrad(l.g, l.in, gz, part, gw, st);
    }
    static void crops_in(const float* x, int n, float* ximg, hipStream_t st) {
        hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(nblk((long long)n * 3 * IMG * IMG)), dim3(256), 0, st, x, n, 3, IMG * IMG, ximg);
    }
    static hipError_t crop_grad(const L& stem, const float* w, const float* g1, float* g2, int n, float* g_x, hipStream_t st) {
        hipError_t e = ::conv_dgrad(stem.g, g1, w, nullptr, g2, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(nblk((long long)n * 3 * IMG * IMG)), dim3(256), 0, st, g2, n, 3, 3, IMG * IMG, g_x);
        return hipGetLastError();
    }
    // the downsample's data gradient goes to gnext and conv1's data gradient adds it in place
    static hipError_t ds_block_dgrad(const L& ds, const float* wds, const float* gres, const L& c1, const float* wc1, const float* g1,
                                     float*, float* gnext, hipStream_t st) {
        hipError_t e = ::conv_dgrad(ds.g, gres, wds, nullptr, gnext, st);
        if (e != hipSuccess) return e;
        return ::conv_dgrad(c1.g, g1, wc1, gnext, gnext, st);
    }
};

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------ primitives
int apg_conv_fwd(const float* x, int n, int H, int W, int C, const float* w, int K, int R, int S, int stride, int pad, float* y,
                 void* stream) {
    const Geom g = make_geom(n, H, W, C, K, R, S, stride, pad);
    if (!x || !w || !y || !geom_ok(g)) return apg_fail(APG_EINVAL, "apg_conv_fwd: bad argument");
    APG_TRY(conv_fwd(g, x, w, y, (hipStream_t)stream));
    return APG_OK;
}

int64_t apg_conv_bwd_workspace_bytes(int n, int H, int W, int C, int K, int R, int S, int stride, int pad) {
    const Geom g = make_geom(n, H, W, C, K, R, S, stride, pad);
    if (!geom_ok(g)) return -1;
    return (int64_t)(wgrad_floats(g) * sizeof(float));
}

int apg_conv_bwd(const float* x, int n, int H, int W, int C, const float* w, int K, int R, int S, int stride, int pad, const float* gy,
                 float* gx, float* gw, void* workspace, int64_t workspace_bytes, void* stream) {
    const Geom g = make_geom(n, H, W, C, K, R, S, stride, pad);
    if (!gy || !geom_ok(g) || (!gx && !gw) || (gx && !w) || (gw && !x) || K % 16 != 0 || !al16(gy))
        return apg_fail(APG_EINVAL, "apg_conv_bwd: bad argument (C_out must be a multiple of 16, gy 16-byte aligned)");
    if (gw && (!workspace || workspace_bytes < (int64_t)(wgrad_floats(g) * sizeof(float))))
        return apg_fail(APG_ENOMEM, "apg_conv_bwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(wgrad_floats(g) * sizeof(float)) + " needed");
    hipStream_t st = (hipStream_t)stream;
    if (gx) APG_TRY(conv_dgrad(g, gy, w, nullptr, gx, st));
    if (gw) APG_TRY(conv_wgrad(g, x, gy, (float*)workspace, gw, st));
    return APG_OK;
}

int64_t apg_bn_workspace_bytes(int M, int C) {
    if (M <= 0 || C <= 0) return -1;
    return (int64_t)(bn_part_floats(M, C) * sizeof(float));
}

int apg_bn_fwd(const float* x, int M, int C, const float* gamma, const float* beta, float* running_mean, float* running_var, int train,
               float momentum, float eps, const float* res, int relu, float* y, float* save_mean, float* save_invstd, void* workspace,
               int64_t workspace_bytes, void* stream) {
    if (!x || M <= 0 || C <= 0 || !gamma || !beta || !y || !save_mean || !save_invstd || !(eps >= 0.f) ||
        (!train && (!running_mean || !running_var)) || (!running_mean != !running_var))
        return apg_fail(APG_EINVAL, "apg_bn_fwd: bad argument");
    if (train && (!workspace || workspace_bytes < apg_bn_workspace_bytes(M, C)))
        return apg_fail(APG_ENOMEM, "apg_bn_fwd: workspace too small");
    APG_TRY(bn_fwd<F32Store>(x, M, C, gamma, beta, running_mean, running_var, train, momentum, eps, res, relu, y, save_mean, save_invstd,
                             (float*)workspace, (hipStream_t)stream));
    return APG_OK;
}

int apg_bn_bwd(const float* gy, const float* y, const float* x, int M, int C, const float* gamma, const float* save_mean,
               const float* save_invstd, int train, float* gx, float* g_res, float* g_gamma, float* g_beta, void* workspace,
               int64_t workspace_bytes, void* stream) {
    if (!gy || !x || M <= 0 || C <= 0 || !gamma || !save_mean || !save_invstd || !gx)
        return apg_fail(APG_EINVAL, "apg_bn_bwd: bad argument");
    if (!workspace || workspace_bytes < apg_bn_workspace_bytes(M, C)) return apg_fail(APG_ENOMEM, "apg_bn_bwd: workspace too small");
    APG_TRY(bn_bwd<F32Store>(gy, y, x, M, C, gamma, save_mean, save_invstd, train, gx, g_res, g_gamma, g_beta, (float*)workspace,
                             (hipStream_t)stream));
    return APG_OK;
}

int apg_maxpool_fwd(const float* x, int n, int H, int W, int C, float* y, void* stream) {
    if (!x || !y || n <= 0 || H <= 0 || W <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_maxpool_fwd: bad argument");
    F32Ops::maxpool_fwd(x, n, H, W, C, y, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_maxpool_bwd(const float* x, int n, int H, int W, int C, const float* gy, float* gx, void* stream) {
    if (!x || !gy || !gx || n <= 0 || H <= 0 || W <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_maxpool_bwd: bad argument");
    F32Ops::maxpool_bwd(x, gy, n, H, W, C, gx, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_avgpool_fwd(const float* x, int n, int C, float* y, void* stream) {
    if (!x || !y || n <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_avgpool_fwd: bad argument");
    F32Ops::avgpool_fwd(x, n, C, y, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_avgpool_bwd(const float* gy, int n, int C, float* gx, void* stream) {
    if (!gy || !gx || n <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_avgpool_bwd: bad argument");
    F32Ops::avgpool_bwd(gy, n, C, gx, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

// ------------------------------------------------------------------------------------------------ the trunk walker
int64_t apg_trunk_workspace_bytes(int n, int save) { return trunk_bytes<F32Ops>(n, save); }

int apg_trunk_fwd(int n, const float* x, const void* const* params, int train, float momentum, float eps, float* xf, int save,
                  void* workspace, int64_t workspace_bytes, void* stream) {
    return trunk_fwd_walk<F32Ops>(n, x, params, train, momentum, eps, xf, save, workspace, workspace_bytes, stream);
}

int apg_trunk_bwd(int n, const void* const* params, int train, const float* g_xf, void* const* g_params, float* g_x, void* workspace,
                  int64_t workspace_bytes, void* stream) {
    return trunk_bwd_walk<F32Ops>(n, params, train, g_xf, g_params, g_x, workspace, workspace_bytes, stream);
}

}  // extern "C"
