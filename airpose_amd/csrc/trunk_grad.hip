// ResNet-50 trunk forward / backward for gfx950 (libairpose_grad.so): copenet.forward_feat_ext (model_copenet.py:161-176) on live
// fp32 parameters, in train-mode (batch statistics, running-stat update) or eval-mode BatchNorm, and its adjoint.
//   convolution:  apg_conv_kernel, an implicit GEMM on NHWC fp32 activations and the OIHW fp32 weights as they are, 64 x 64 tile
//                 per workgroup of 4 waves, K in stages of 16 through LDS, v_mfma_f32_16x16x4_f32 (exact fp32):
//                   CV_FWD    M = n Ho Wo, N = C_out, K = (r, s, c_in)
//                   CV_DGRAD  M = n H W,   N = C_in,  K = (r, s, c_out), a gather with per-tap validity (stride 2 included)
//                   CV_WGRAD  M = C_out,   N = (r, s, c_in), K = n Ho Wo in fixed split-K chunks; conv_wgrad_combine_kernel
//                             sums the chunks in chunk order straight into the OIHW gradient
//   BatchNorm:    per-channel statistics over the n H W rows as per-tile centred partials (mean, M2) combined by Chan's formula in a
//                 fixed tree; normalise + affine (+ residual) (+ ReLU) in one pass; backward with the ReLU mask and the residual
//                 split fused in
//   pools:        max-pool 3 x 3 / s2 / p1 (padding = -inf, the first maximum in row-major window order takes the gradient, as in
//                 torch) and avg-pool 7 x 7, forward and backward as gathers
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

// gW[co][c][r][s] = sum over the chunks, in chunk order, of part[chunk][co][(r S + s) C + c]
__global__ void __launch_bounds__(256) conv_wgrad_combine_kernel(const float* __restrict__ part, int nch, int K, int C, int R, int S,
                                                                 float* __restrict__ gw) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)C * R * S;
    if (idx >= (long long)K * per) return;
    const int co = (int)(idx / per), rem = (int)(idx - co * per);
    const int c = rem / (R * S), rs = rem - c * R * S;
    const long long src = (long long)co * per + (long long)rs * C + c, stride = (long long)K * per;
    float s = 0.f;
    for (int ch = 0; ch < nch; ++ch) s += part[ch * stride + src];
    gw[idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm
// Rows (n H W) are cut into tiles of `tr` rows (tr % 4 == 0, at most 256 tiles); a workgroup takes 64 channels x one tile, its 4
// waves a quarter of the tile each.
#include "bn_common.inc"

// per tile: count, mean, M2 = sum (x - mean)^2 (centred on the tile's own mean)
__global__ void __launch_bounds__(256) bn_stats_part_kernel(const float* __restrict__ x, int M, int C, int tr,
                                                            float* __restrict__ part) {
    __shared__ float sh[4][64];
    __shared__ float smean[64];
    const int t = threadIdx.x, cl = t & 63, g = t >> 6, c = blockIdx.x * 64 + cl, tile = blockIdx.y;
    const int t0 = tile * tr, tcnt = min(tr, M - t0), r0 = t0 + g * (tr / 4), r1 = min(r0 + tr / 4, M);
    float s = 0.f;
    if (c < C)
        for (int r = r0; r < r1; ++r) s += x[(long long)r * C + c];
    sh[g][cl] = s;
    __syncthreads();
    if (g == 0) smean[cl] = (((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl]) / (float)tcnt;
    __syncthreads();
    const float mean = smean[cl];
    float m2 = 0.f;
    if (c < C)
        for (int r = r0; r < r1; ++r) {
            const float d = x[(long long)r * C + c] - mean;
            m2 += d * d;
        }
    sh[g][cl] = m2;
    __syncthreads();
    if (g == 0 && c < C) {
        part[((long long)tile * 3 + 0) * C + c] = (float)tcnt;
        part[((long long)tile * 3 + 1) * C + c] = mean;
        part[((long long)tile * 3 + 2) * C + c] = ((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl];
    }
}

// y = (x - mean) invstd gamma + beta (+ res) (ReLU); y may alias x or res (same index)
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* x, long long total, int C, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* res, int relu, float* y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    float v = (x[idx] - mean[c]) * invstd[c] * gamma[c] + beta[c];
    if (res) v += res[idx];
    if (relu) v = fmaxf(v, 0.f);
    y[idx] = v;
}

// per tile: sum g and sum g xhat, g = gy masked by y > 0 (y NULL: no ReLU)
__global__ void __launch_bounds__(256) bn_bwd_part_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                          const float* __restrict__ x, int M, int C, int tr, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd, float* __restrict__ part) {
    __shared__ float s1[4][64], s2[4][64];
    const int t = threadIdx.x, cl = t & 63, g = t >> 6, c = blockIdx.x * 64 + cl, tile = blockIdx.y;
    const int r0 = tile * tr + g * (tr / 4), r1 = min(r0 + tr / 4, M);
    float a = 0.f, b = 0.f;
    if (c < C) {
        const float mu = mean[c], is = invstd[c];
        for (int r = r0; r < r1; ++r) {
            const long long o = (long long)r * C + c;
            float gv = gy[o];
            if (y && !(y[o] > 0.f)) gv = 0.f;
            a += gv;
            b += gv * ((x[o] - mu) * is);
        }
    }
    s1[g][cl] = a;
    s2[g][cl] = b;
    __syncthreads();
    if (g == 0 && c < C) {
        part[((long long)tile * 2 + 0) * C + c] = ((s1[0][cl] + s1[1][cl]) + s1[2][cl]) + s1[3][cl];
        part[((long long)tile * 2 + 1) * C + c] = ((s2[0][cl] + s2[1][cl]) + s2[2][cl]) + s2[3][cl];
    }
}

// gx = gamma invstd (g - sum g / M - xhat sum(g xhat) / M) (train) or gamma invstd g (eval); g_res = g.  gx may alias gy.
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* gy, const float* __restrict__ y, const float* __restrict__ x,
                                                           long long total, int C, float inv_m, int train, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ sums, float* gx, float* g_res) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    float g = gy[idx];
    if (y && !(y[idx] > 0.f)) g = 0.f;
    const float k = gamma[c] * invstd[c];
    float v;
    if (train) {
        const float xhat = (x[idx] - mean[c]) * invstd[c];
        v = k * ((g - sums[c] * inv_m) - xhat * (sums[C + c] * inv_m));
    } else {
        v = k * g;
    }
    if (g_res) g_res[idx] = g;
    gx[idx] = v;
}

// ---------------------------------------------------------------------------------------------------------------- pools
// max-pool 3 x 3 / s2 / p1, NHWC: padding is -inf; the first maximum in row-major window order is the argmax
__device__ __forceinline__ int maxpool_arg(const float* __restrict__ x, int b, int ho, int wo, int c, int H, int W, int C, float* best) {
    float m = -INFINITY;
    int arg = -1;
    for (int r = 0; r < 3; ++r) {
        const int h = ho * 2 - 1 + r;
        if (h < 0 || h >= H) continue;
        for (int s = 0; s < 3; ++s) {
            const int w = wo * 2 - 1 + s;
            if (w < 0 || w >= W) continue;
            const float v = x[(((long long)b * H + h) * W + w) * C + c];
            if (arg < 0 || v > m || v != v) { m = v; arg = h * W + w; }
        }
    }
    *best = m;
    return arg;
}

__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const float* __restrict__ x, int n, int H, int W, int C, int Ho, int Wo,
                                                          float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * Ho * Wo * C) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int wo = (int)(p % Wo), ho = (int)((p / Wo) % Ho), b = (int)(p / ((long long)Wo * Ho));
    float m;
    maxpool_arg(x, b, ho, wo, c, H, W, C, &m);
    y[idx] = m;
}

// gx[b][h][w][c] = sum, over the windows (ho, wo ascending) whose argmax is (h, w), of gy[b][ho][wo][c]
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, int n, int H, int W,
                                                          int C, int Ho, int Wo, float* __restrict__ gx) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * H * W * C) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int w = (int)(p % W), h = (int)((p / W) % H), b = (int)(p / ((long long)W * H));
    float s = 0.f;
    const int me = h * W + w;
    for (int ho = max(0, h / 2 - 1); ho <= min(Ho - 1, (h + 1) / 2); ++ho) {
        if (h < ho * 2 - 1 || h > ho * 2 + 1) continue;
        for (int wo = max(0, w / 2 - 1); wo <= min(Wo - 1, (w + 1) / 2); ++wo) {
            if (w < wo * 2 - 1 || w > wo * 2 + 1) continue;
            float m;
            if (maxpool_arg(x, b, ho, wo, c, H, W, C, &m) == me) s += gy[(((long long)b * Ho + ho) * Wo + wo) * C + c];
        }
    }
    gx[idx] = s;
}

// avg-pool 7 x 7 over a (n, 7, 7, C) map -> (n, C): the 49 pixels summed in row-major order, / 49
__global__ void __launch_bounds__(256) avgpool_fwd_kernel(const float* __restrict__ x, int n, int C, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * C) return;
    const int c = (int)(idx % C), b = (int)(idx / C);
    float s = 0.f;
    for (int p = 0; p < 49; ++p) s += x[((long long)b * 49 + p) * C + c];
    y[idx] = s / 49.f;
}

__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float* __restrict__ gy, int n, int C, float* __restrict__ gx) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * 49 * C) return;
    const int c = (int)(idx % C), b = (int)(idx / (49LL * C));
    gx[idx] = gy[(long long)b * C + c] / 49.f;
}

// NCHW <-> NHWC of the (n, 3, 224, 224) crops
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, int n, int C, int HW, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * C * HW) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int hw = (int)(p % HW), b = (int)(p / HW);
    y[idx] = x[((long long)b * C + c) * HW + hw];
}

__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const float* __restrict__ x, int n, int C, int HW, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * C * HW) return;
    const int hw = (int)(idx % HW);
    const long long p = idx / HW;
    const int c = (int)(p % C), b = (int)(p / C);
    y[idx] = x[((long long)b * HW + hw) * C + c];
}

// ---------------------------------------------------------------------------------------------------------------- host side
size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }
unsigned nblk(long long total) { return (unsigned)((total + 255) / 256); }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Geom {
    int n, H, W, C, K, R, S, st, pad, Ho, Wo;
};

bool geom_ok(const Geom& g) {
    if (g.n <= 0 || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.K <= 0 || g.R <= 0 || g.S <= 0 || g.st <= 0 || g.pad < 0) return false;
    // the kernel must fit the padded input: make_geom's division truncates toward zero, so at stride >= 2 a too-large kernel
    // would otherwise come out as Ho = 1
    if ((long long)g.H + 2LL * g.pad < g.R || (long long)g.W + 2LL * g.pad < g.S) return false;
    if (g.Ho <= 0 || g.Wo <= 0) return false;
    return (long long)g.n * g.H * g.W * g.C < (1LL << 31) && (long long)g.n * g.Ho * g.Wo * g.K < (1LL << 31) &&
           (long long)g.n * g.Ho * g.Wo < (1LL << 31);
}

Geom make_geom(int n, int H, int W, int C, int K, int R, int S, int st, int pad) {
    Geom g{n, H, W, C, K, R, S, st, pad, 0, 0};
    if (st > 0) {
        g.Ho = (H + 2 * pad - R) / st + 1;
        g.Wo = (W + 2 * pad - S) / st + 1;
    }
    return g;
}

ConvArgs conv_args(const Geom& g) {
    ConvArgs a = {};
    a.n = g.n; a.H = g.H; a.W = g.W; a.C = g.C; a.K = g.K; a.R = g.R; a.S = g.S; a.st = g.st; a.pad = g.pad; a.Ho = g.Ho; a.Wo = g.Wo;
    return a;
}

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

size_t wgrad_floats(const Geom& g) {
    int nch, chunk;
    wgrad_split(g, &nch, &chunk);
    return (size_t)nch * g.K * g.R * g.S * g.C;
}

hipError_t conv_fwd(const Geom& g, const float* x, const float* w, float* y, hipStream_t st) {
    ConvArgs a = conv_args(g);
    a.x = x; a.w = w; a.out = y;
    a.M = g.n * g.Ho * g.Wo; a.N = g.K; a.KK = g.R * g.S * g.C;
    const dim3 grid((a.M + 63) / 64, (a.N + 63) / 64);
    if (g.C % 16 == 0 && al16(x)) hipLaunchKernelGGL((apg_conv_kernel<CV_FWD, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((apg_conv_kernel<CV_FWD, false>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// gx = dgrad(gy) (+ add); needs K % 16 == 0 and gy 16-byte aligned (argument checks)
hipError_t conv_dgrad(const Geom& g, const float* gy, const float* w, const float* add, float* gx, hipStream_t st) {
    ConvArgs a = conv_args(g);
    a.gy = gy; a.w = w; a.out = gx; a.add = add;
    a.M = g.n * g.H * g.W; a.N = g.C; a.KK = g.R * g.S * g.K;
    hipLaunchKernelGGL((apg_conv_kernel<CV_DGRAD, true>), dim3((a.M + 63) / 64, (a.N + 63) / 64), dim3(256), 0, st, a);
    return hipGetLastError();
}

// gw (OIHW) = wgrad, through `part` (wgrad_floats(g) floats)
hipError_t conv_wgrad(const Geom& g, const float* x, const float* gy, float* part, float* gw, hipStream_t st) {
    ConvArgs a = conv_args(g);
    a.x = x; a.gy = gy; a.out = part;
    a.M = g.K; a.N = g.R * g.S * g.C; a.KK = g.n * g.Ho * g.Wo;
    int nch;
    wgrad_split(g, &nch, &a.kchunk);
    const dim3 grid((a.M + 63) / 64, (a.N + 63) / 64, nch);
    if (g.C % 64 == 0 && al16(x)) hipLaunchKernelGGL((apg_conv_kernel<CV_WGRAD, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((apg_conv_kernel<CV_WGRAD, false>), grid, dim3(256), 0, st, a);
    const long long tot = (long long)g.K * g.C * g.R * g.S;
    hipLaunchKernelGGL(conv_wgrad_combine_kernel, dim3(nblk(tot)), dim3(256), 0, st, part, nch, g.K, g.C, g.R, g.S, gw);
    return hipGetLastError();
}

size_t bn_part_floats(int M, int C) { return (size_t)bn_tiles(M) * 3 * C + 2 * (size_t)C; }

// forward BN over (M, C): train -> batch statistics (+ running update when rm / rv given), eval -> running statistics
hipError_t bn_fwd(const float* x, int M, int C, const float* gamma, const float* beta, float* rm, float* rv, int train, float momentum,
                  float eps, const float* res, int relu, float* y, float* mean, float* invstd, float* part, hipStream_t st) {
    if (train) {
        const int tr = bn_tile_rows(M), nt = bn_tiles(M);
        hipLaunchKernelGGL(bn_stats_part_kernel, dim3((C + 63) / 64, nt), dim3(256), 0, st, x, M, C, tr, part);
        hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C), dim3(64), 0, st, part, nt, C, momentum, eps, rm, rv, mean, invstd);
    } else {
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, st, rm, rv, C, eps, mean, invstd);
    }
    const long long tot = (long long)M * C;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(nblk(tot)), dim3(256), 0, st, x, tot, C, mean, invstd, gamma, beta, res, relu, y);
    return hipGetLastError();
}

hipError_t bn_bwd(const float* gy, const float* y, const float* x, int M, int C, const float* gamma, const float* mean,
                  const float* invstd, int train, float* gx, float* g_res, float* g_gamma, float* g_beta, float* part, hipStream_t st) {
    const int tr = bn_tile_rows(M), nt = bn_tiles(M);
    float* sums = part + (size_t)nt * 2 * C;
    hipLaunchKernelGGL(bn_bwd_part_kernel, dim3((C + 63) / 64, nt), dim3(256), 0, st, gy, y, x, M, C, tr, mean, invstd, part);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C), dim3(64), 0, st, part, nt, C, sums, g_gamma, g_beta);
    const long long tot = (long long)M * C;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nblk(tot)), dim3(256), 0, st, gy, y, x, tot, C, 1.f / (float)M, train, mean, invstd,
                       gamma, sums, gx, g_res);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- the trunk plan
constexpr int NLAYER = 53;
constexpr int IMG = 224;

struct Layer {
    int idx;                             // position in state_dict order (conv + BN pair)
    Geom g;
    float *in, *z, *a;                   // conv input, conv output (pre-BN), BN output
    float *mean, *invstd;
};

struct Block {
    Layer c1, c2, c3, ds;
    bool has_ds;
};

struct Plan {
    Layer stem;
    float *ximg, *pool;                  // NHWC copy of the crops; max-pool output
    Block blk[16];
    float* G[6];                         // backward: gradient buffers of the largest activation
    float* part;                         // split-K / BN partials
    size_t total;                        // floats
};

// Walks the fixed [3, 4, 6, 3] graph.  base == nullptr: sizes only.  save = 1: every activation has its own buffer (what backward
// reads) and the backward buffers follow; save = 0: forward only, five rotating buffers, BN in place.
Plan make_plan(int n, int save, float* base) {
    Plan P;
    size_t off = 0;
    auto take = [&](size_t floats) -> float* {
        float* p = base ? base + off : nullptr;
        off += align64(floats);
        return p;
    };
    const size_t big = (size_t)n * 112 * 112 * 64;       // the largest activation (stem output; layer1's 256-channel maps equal it)
    float* slot[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!save)
        for (int k = 0; k < 5; ++k) slot[k] = take(big);
    size_t part = 0;
    auto mk = [&](int idx, float* in, int H, int C, int K, int R, int st, int pad, float* zs) {
        Layer L;
        L.idx = idx;
        L.g = make_geom(n, H, H, C, K, R, R, st, pad);
        L.in = in;
        const size_t sz = (size_t)n * L.g.Ho * L.g.Wo * K;
        L.z = save ? take(sz) : zs;
        L.a = save ? take(sz) : zs;
        L.mean = take(K);
        L.invstd = take(K);
        part = std::max(part, wgrad_floats(L.g));
        part = std::max(part, bn_part_floats(n * L.g.Ho * L.g.Wo, K));
        return L;
    };
    P.ximg = save ? take((size_t)n * IMG * IMG * 3) : slot[0];
    P.stem = mk(0, P.ximg, IMG, 3, 64, 7, 2, 3, slot[1]);
    P.pool = save ? take((size_t)n * 56 * 56 * 64) : slot[2];
    float* x = P.pool;
    int H = 56, C = 64, idx = 1, bi = 0;
    int free_slots[3] = {0, 1, 3};                          // save = 0: the slots not holding the block input (slot 2) ...
    int in_slot = 2, ds_slot = 4;
    const int layers[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < layers[li]; ++b, ++bi) {
            const int p = planes[li], st = (b == 0 && li > 0) ? 2 : 1;
            Block& B = P.blk[bi];
            B.has_ds = b == 0;
            float *s1 = nullptr, *s2 = nullptr, *s3 = nullptr;
            if (!save) { s1 = slot[free_slots[0]]; s2 = slot[free_slots[1]]; s3 = slot[free_slots[2]]; }
            B.c1 = mk(idx++, x, H, C, p, 1, 1, 0, s1);
            B.c2 = mk(idx++, B.c1.a, H, p, p, 3, st, 1, s2);
            const int Ho = B.c2.g.Ho;
            B.c3 = mk(idx++, B.c2.a, Ho, p, 4 * p, 1, 1, 0, s3);
            if (B.has_ds) B.ds = mk(idx++, x, H, C, 4 * p, 1, st, 0, save ? nullptr : slot[ds_slot]);
            x = B.c3.a;
            H = Ho;
            C = 4 * p;
            if (!save) {                                    // the block output (slot free_slots[2]) becomes the next input
                const int o = free_slots[2];
                free_slots[2] = in_slot;
                in_slot = o;
            }
        }
    for (int k = 0; k < 6; ++k) P.G[k] = save ? take(big) : nullptr;
    P.part = take(part);
    P.total = off;
    return P;
}

const float* prm(const void* const* t, int layer, int k) { return (const float*)t[layer * 5 + k]; }

}  // namespace

#define APG_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) return apg_fail((int)_e, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

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
    APG_TRY(bn_fwd(x, M, C, gamma, beta, running_mean, running_var, train, momentum, eps, res, relu, y, save_mean, save_invstd,
                   (float*)workspace, (hipStream_t)stream));
    return APG_OK;
}

int apg_bn_bwd(const float* gy, const float* y, const float* x, int M, int C, const float* gamma, const float* save_mean,
               const float* save_invstd, int train, float* gx, float* g_res, float* g_gamma, float* g_beta, void* workspace,
               int64_t workspace_bytes, void* stream) {
    if (!gy || !x || M <= 0 || C <= 0 || !gamma || !save_mean || !save_invstd || !gx)
        return apg_fail(APG_EINVAL, "apg_bn_bwd: bad argument");
    if (!workspace || workspace_bytes < apg_bn_workspace_bytes(M, C)) return apg_fail(APG_ENOMEM, "apg_bn_bwd: workspace too small");
    APG_TRY(bn_bwd(gy, y, x, M, C, gamma, save_mean, save_invstd, train, gx, g_res, g_gamma, g_beta, (float*)workspace,
                   (hipStream_t)stream));
    return APG_OK;
}

int apg_maxpool_fwd(const float* x, int n, int H, int W, int C, float* y, void* stream) {
    if (!x || !y || n <= 0 || H <= 0 || W <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_maxpool_fwd: bad argument");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(nblk((long long)n * Ho * Wo * C)), dim3(256), 0, (hipStream_t)stream, x, n, H, W, C,
                       Ho, Wo, y);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_maxpool_bwd(const float* x, int n, int H, int W, int C, const float* gy, float* gx, void* stream) {
    if (!x || !gy || !gx || n <= 0 || H <= 0 || W <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_maxpool_bwd: bad argument");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(nblk((long long)n * H * W * C)), dim3(256), 0, (hipStream_t)stream, x, gy, n, H, W, C,
                       Ho, Wo, gx);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_avgpool_fwd(const float* x, int n, int C, float* y, void* stream) {
    if (!x || !y || n <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_avgpool_fwd: bad argument");
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(nblk((long long)n * C)), dim3(256), 0, (hipStream_t)stream, x, n, C, y);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_avgpool_bwd(const float* gy, int n, int C, float* gx, void* stream) {
    if (!gy || !gx || n <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_avgpool_bwd: bad argument");
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(nblk((long long)n * 49 * C)), dim3(256), 0, (hipStream_t)stream, gy, n, C, gx);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

// ------------------------------------------------------------------------------------------------ the trunk walker
int64_t apg_trunk_workspace_bytes(int n, int save) {
    if (n <= 0 || n > 2048) return -1;
    return (int64_t)(make_plan(n, save ? 1 : 0, nullptr).total * sizeof(float));
}

static int check_table(const void* const* params, const char* what) {
    if (!params) return apg_fail(APG_EINVAL, std::string(what) + ": parameter table missing");
    for (int k = 0; k < NLAYER * 5; ++k)
        if (!params[k]) return apg_fail(APG_EINVAL, std::string(what) + ": parameter table entry " + std::to_string(k) + " is NULL");
    return APG_OK;
}

int apg_trunk_fwd(int n, const float* x, const void* const* params, int train, float momentum, float eps, float* xf, int save,
                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (n <= 0 || n > 2048 || !x || !xf || !workspace || !(eps >= 0.f) || (train && !(momentum >= 0.f && momentum <= 1.f)))
        return apg_fail(APG_EINVAL, "apg_trunk_fwd: bad argument");
    if (int rc = check_table(params, "apg_trunk_fwd")) return rc;
    if (workspace_bytes < apg_trunk_workspace_bytes(n, save))
        return apg_fail(APG_ENOMEM, "apg_trunk_fwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(apg_trunk_workspace_bytes(n, save)) + " needed");
    hipStream_t st = (hipStream_t)stream;
    const Plan P = make_plan(n, save ? 1 : 0, (float*)workspace);
    auto run = [&](const Layer& L, const float* res, int relu) -> hipError_t {
        hipError_t e = conv_fwd(L.g, L.in, prm(params, L.idx, 0), L.z, st);
        if (e != hipSuccess) return e;
        return bn_fwd(L.z, n * L.g.Ho * L.g.Wo, L.g.K, prm(params, L.idx, 1), prm(params, L.idx, 2), (float*)prm(params, L.idx, 3),
                      (float*)prm(params, L.idx, 4), train, momentum, eps, res, relu, L.a, L.mean, L.invstd, P.part, st);
    };
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(nblk((long long)n * 3 * IMG * IMG)), dim3(256), 0, st, x, n, 3, IMG * IMG, P.ximg);
    APG_TRY(run(P.stem, nullptr, 1));
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(nblk((long long)n * 56 * 56 * 64)), dim3(256), 0, st, P.stem.a, n, 112, 112, 64, 56,
                       56, P.pool);
    APG_TRY(hipGetLastError());
    for (int b = 0; b < 16; ++b) {
        const Block& B = P.blk[b];
        APG_TRY(run(B.c1, nullptr, 1));
        APG_TRY(run(B.c2, nullptr, 1));
        if (B.has_ds) APG_TRY(run(B.ds, nullptr, 0));
        APG_TRY(run(B.c3, B.has_ds ? B.ds.a : B.c1.in, 1));
    }
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(nblk((long long)n * 2048)), dim3(256), 0, st, P.blk[15].c3.a, n, 2048, xf);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_trunk_bwd(int n, const void* const* params, int train, const float* g_xf, void* const* g_params, float* g_x, void* workspace,
                  int64_t workspace_bytes, void* stream) {
    if (n <= 0 || n > 2048 || !g_xf || !g_params || !workspace) return apg_fail(APG_EINVAL, "apg_trunk_bwd: bad argument");
    if (int rc = check_table(params, "apg_trunk_bwd")) return rc;
    if (workspace_bytes < apg_trunk_workspace_bytes(n, 1))
        return apg_fail(APG_ENOMEM, "apg_trunk_bwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(apg_trunk_workspace_bytes(n, 1)) + " needed (the one apg_trunk_fwd filled, save = 1)");
    hipStream_t st = (hipStream_t)stream;
    const Plan P = make_plan(n, 1, (float*)workspace);
    float *gcur = P.G[0], *gnext = P.G[1], *g3 = P.G[2], *g2 = P.G[3], *g1 = P.G[4], *gres = P.G[5];
    auto gp = [&](const Layer& L, int k) { return (float*)g_params[L.idx * 3 + k]; };
    // BN backward of layer L (gy -> gx, ReLU mask from L.a when relu), then its weight gradient
    auto bnb = [&](const Layer& L, const float* gy, int relu, float* gx, float* g_res) -> hipError_t {
        return bn_bwd(gy, relu ? L.a : nullptr, L.z, n * L.g.Ho * L.g.Wo, L.g.K, prm(params, L.idx, 1), L.mean, L.invstd, train, gx,
                      g_res, gp(L, 1), gp(L, 2), P.part, st);
    };
    auto wg = [&](const Layer& L, const float* gz) -> hipError_t {
        if (!gp(L, 0)) return hipSuccess;
        return conv_wgrad(L.g, L.in, gz, P.part, gp(L, 0), st);
    };
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(nblk((long long)n * 49 * 2048)), dim3(256), 0, st, g_xf, n, 2048, gcur);
    APG_TRY(hipGetLastError());
    for (int b = 15; b >= 0; --b) {
        const Block& B = P.blk[b];
        APG_TRY(bnb(B.c3, gcur, 1, g3, gres));
        APG_TRY(wg(B.c3, g3));
        APG_TRY(conv_dgrad(B.c3.g, g3, prm(params, B.c3.idx, 0), nullptr, g2, st));
        APG_TRY(bnb(B.c2, g2, 1, g2, nullptr));
        APG_TRY(wg(B.c2, g2));
        APG_TRY(conv_dgrad(B.c2.g, g2, prm(params, B.c2.idx, 0), nullptr, g1, st));
        APG_TRY(bnb(B.c1, g1, 1, g1, nullptr));
        APG_TRY(wg(B.c1, g1));
        if (B.has_ds) {
            APG_TRY(bnb(B.ds, gres, 0, gres, nullptr));
            APG_TRY(wg(B.ds, gres));
            APG_TRY(conv_dgrad(B.ds.g, gres, prm(params, B.ds.idx, 0), nullptr, gnext, st));
            APG_TRY(conv_dgrad(B.c1.g, g1, prm(params, B.c1.idx, 0), gnext, gnext, st));
        } else {
            APG_TRY(conv_dgrad(B.c1.g, g1, prm(params, B.c1.idx, 0), gres, gnext, st));
        }
        std::swap(gcur, gnext);
    }
    // stem: max-pool, BN + ReLU, the 7 x 7 convolution
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(nblk((long long)n * 112 * 112 * 64)), dim3(256), 0, st, P.stem.a, gcur, n, 112, 112, 64,
                       56, 56, g1);
    APG_TRY(hipGetLastError());
    APG_TRY(bnb(P.stem, g1, 1, g1, nullptr));
    APG_TRY(wg(P.stem, g1));
    if (g_x) {
        APG_TRY(conv_dgrad(P.stem.g, g1, prm(params, 0, 0), nullptr, g2, st));
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(nblk((long long)n * 3 * IMG * IMG)), dim3(256), 0, st, g2, n, 3, IMG * IMG, g_x);
        APG_TRY(hipGetLastError());
    }
    return APG_OK;
}

}  // extern "C"
