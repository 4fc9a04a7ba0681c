// Mixed-precision (bf16) training mode of the ResNet-50 trunk for gfx950 (libairpose_grad.so): the graph of trunk_grad.hip with bf16
// NHWC activations and activation gradients, bf16 x bf16 products accumulated in fp32 on v_mfma_f32_16x16x32_bf16, fp32 master
// weights (a bf16 copy is packed into the workspace on every forward call), fp32 BatchNorm statistics, fp32 parameter gradients.
// The storage and rounding rules are the table of DESIGN 4.3.4; every rounding is one round-to-nearest-even at a store.
//   convolution:  bconv_kernel<MODE, BM, BN>, an implicit GEMM with both operands k-contiguous in LDS (row pitch 72 bf16, so the
//                 ds_read_b128 fragment reads of 16 rows fall on 16 distinct 16-byte bank slots), K in stages of 64 (two 16x16x32
//                 steps per fragment pair), two LDS stages: the next stage's 16-byte global loads are issued before the current
//                 stage's MFMAs and land in LDS after them, one barrier per stage.  256 threads = 2 x 2 waves; tiles 128 x 128
//                 (16 accumulator fragments per wave, 32 MFMAs between barriers) and 64 x 64.
//                   CV_FWD    M = n Ho Wo, N = C_out, K = (r, s, c_in):  A = x NHWC, B = weights packed [co][r][s][c]
//                   CV_DGRAD  M = n H W,   N = C_in,  K = (r, s, c_out): A = gy NHWC gathered with the per-tap validity test,
//                             B = weights packed [c][r][s][co]
//                   CV_WGRAD  M = C_out,   N = (r, s, c_in), K = n Ho Wo in fixed split-K chunks: neither operand is k-contiguous
//                             in NHWC, so both are transposed on the way into LDS: a thread loads 8 channels of two consecutive
//                             pixels (two 16-byte loads) and writes 8 dwords, each one channel's pixel pair
//   BatchNorm, pools, layout: trunk_elem.inc, the one source this file shares with trunk_grad.hip, instantiated on Bf16Store (bf16
//                 storage, 8 channels = 16 bytes per thread in the element-wise passes, fp32 math, RNE at the store):
//                 bn_stats_part_kernel and bn_bwd_part_kernel (one channel per lane, 2-byte loads: the fp32 path's per-channel
//                 order), bn_stats_final_kernel, bn_eval_stats_kernel, bn_bwd_final_kernel, bn_apply_kernel, bn_bwd_apply_kernel,
//                 maxpool_fwd_kernel / maxpool_bwd_kernel, avgpool_fwd_kernel / avgpool_bwd_kernel, wgrad_combine_kernel, and
//                 nhwc_to_nchw_kernel at a pitch of 8 for the crop gradient.  The crops are cast into an 8-channel NHWC image
//                 (channels 3 .. 7 zero) by this file's nchw_to_nhwc8_kernel
// No floating-point atomics: every reduction runs in a fixed order, so results are bit-reproducible run to run.
#include "ap_common.h"
#include "grad_internal.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

enum { CV_FWD = 0, CV_DGRAD = 1, CV_WGRAD = 2 };
constexpr int LP = 72;                   // LDS row pitch in bf16: 64 k + 8 (144 bytes)

struct BArgs {
    const bf16_t* a;                     // CV_FWD: x (n, H, W, C); CV_DGRAD / CV_WGRAD: gy (n, Ho, Wo, K)
    const bf16_t* b;                     // CV_FWD: wf [K][R S C]; CV_DGRAD: wd [C][R S K]; CV_WGRAD: x (n, H, W, C)
    void* out;                           // CV_FWD: y bf16; CV_DGRAD: gx bf16 (or fp32 when out_f32); CV_WGRAD: fp32 chunk partials
    const void* add;                     // CV_DGRAD: out = acc + add (same index, fp32 add, one rounding; bf16, may alias out;
                                         // fp32 when add_f32)
    int n, H, W, C, K, R, S, st, pad, Ho, Wo;
    int M, N, KK;
    int kchunk;                          // CV_WGRAD: pixels per chunk (a multiple of 64)
    int out_f32, add_f32;
};

__device__ __forceinline__ uint32_t half_of(const u32x4& v, int j) { return (v[j >> 1] >> (16 * (j & 1))) & 0xffffu; }

template <int MODE, int BM, int BN>
__global__ void __launch_bounds__(256) bconv_kernel(const BArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t As[2][BM * LP];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[2][BN * LP];
    constexpr int VA = BM / 32, VB = BN / 32;                   // 16-byte global loads per thread and stage
    constexpr int MI = BM / 32, NI = BN / 32;                   // 16 x 16 fragments per wave
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;       // M tiles on x: n H W / 64 can pass 65535
    const int wm = (wv >> 1) * (BM / 2), wn = (wv & 1) * (BN / 2);
    const int i16 = lane & 15, q = lane >> 4;
    int kbeg = 0, kend = a.KK;
    if (MODE == CV_WGRAD) {
        kbeg = blockIdx.z * a.kchunk;
        kend = min(kbeg + a.kchunk, a.KK);
    }
    // CV_FWD / CV_DGRAD: thread t stages rows t / 8 + 32 i of both tiles, 8 k at 8 (t % 8); the rows' pixels are fixed
    // CV_WGRAD: thread t stages the pixel pair t % 32 of the channel groups (8 channels) t / 32 + 8 i
    const int kv = t & 7, lr = t >> 3, pp = t & 31, cg = t >> 5;
    int pb[VA], ph[VA], pw[VA];                                 // CV_FWD / CV_DGRAD: image (-1: row outside M), h / w base
    int br[VB], bs[VB], bc[VB];                                 // CV_WGRAD: tap and first channel of the B column group (br -1: outside N)
    if (MODE == CV_FWD || MODE == CV_DGRAD) {
        const int hw = MODE == CV_FWD ? a.Ho * a.Wo : a.H * a.W, wd = MODE == CV_FWD ? a.Wo : a.W;
#pragma unroll
        for (int i = 0; i < VA; ++i) {
            const int m = m0 + lr + 32 * i;
            pb[i] = -1; ph[i] = 0; pw[i] = 0;
            if (m < a.M) {
                const int b = m / hw, rem = m - b * hw, y = rem / wd, x = rem - y * wd;
                pb[i] = b;
                ph[i] = MODE == CV_FWD ? y * a.st - a.pad : y + a.pad;
                pw[i] = MODE == CV_FWD ? x * a.st - a.pad : x + a.pad;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < VB / 2; ++i) {
            const int col = n0 + (cg + 8 * i) * 8;
            br[i] = -1; bs[i] = 0; bc[i] = 0;
            if (col < a.N) {
                const int tap = col / a.C;
                bc[i] = col - tap * a.C;
                br[i] = tap / a.S;
                bs[i] = tap - br[i] * a.S;
            }
        }
    }
    u32x4 ra[VA], rb[VB];
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    auto load = [&](int k0) {
        if (MODE == CV_FWD || MODE == CV_DGRAD) {
            const int gk = k0 + kv * 8;
            const bool kok = gk < kend;
            int r = 0, s = 0, c = 0;
            if (kok) {
                const int ch = MODE == CV_FWD ? a.C : a.K, tap = gk / ch;
                c = gk - tap * ch;
                r = tap / a.S;
                s = tap - r * a.S;
            }
#pragma unroll
            for (int i = 0; i < VA; ++i) {
                ra[i] = zero4;
                if (!kok || pb[i] < 0) continue;
                if (MODE == CV_FWD) {
                    const int h = ph[i] + r, w = pw[i] + s;
                    if (h >= 0 && h < a.H && w >= 0 && w < a.W)
                        ra[i] = *(const u32x4*)(a.a + (((long long)pb[i] * a.H + h) * a.W + w) * a.C + c);
                } else {
                    const int th = ph[i] - r, tw = pw[i] - s;
                    if (th >= 0 && tw >= 0 && th % a.st == 0 && tw % a.st == 0) {
                        const int ho = th / a.st, wo = tw / a.st;
                        if (ho < a.Ho && wo < a.Wo)
                            ra[i] = *(const u32x4*)(a.a + (((long long)pb[i] * a.Ho + ho) * a.Wo + wo) * a.K + c);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < VB; ++i) {
                const int nr = n0 + lr + 32 * i;
                rb[i] = zero4;
                if (kok && nr < a.N) rb[i] = *(const u32x4*)(a.b + (long long)nr * a.KK + gk);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int pix = k0 + 2 * pp + e;
                const bool ok = pix < kend;
                int b = 0, h0 = 0, w0 = 0;
                if (ok) {
                    const int hw = a.Ho * a.Wo;
                    b = pix / hw;
                    const int rem = pix - b * hw, ho = rem / a.Wo, wo = rem - ho * a.Wo;
                    h0 = ho * a.st - a.pad;
                    w0 = wo * a.st - a.pad;
                }
#pragma unroll
                for (int i = 0; i < VA / 2; ++i) {               // A(co, pix) = gy[pix][co]
                    const int co = m0 + (cg + 8 * i) * 8;
                    ra[2 * i + e] = zero4;
                    if (ok && co < a.M) ra[2 * i + e] = *(const u32x4*)(a.a + (long long)pix * a.K + co);
                }
#pragma unroll
                for (int i = 0; i < VB / 2; ++i) {               // B((r, s, c), pix) = x[b][ho st - pad + r][wo st - pad + s][c]
                    rb[2 * i + e] = zero4;
                    if (!ok || br[i] < 0) continue;
                    const int h = h0 + br[i], w = w0 + bs[i];
                    if (h >= 0 && h < a.H && w >= 0 && w < a.W)
                        rb[2 * i + e] = *(const u32x4*)(a.b + (((long long)b * a.H + h) * a.W + w) * a.C + bc[i]);
                }
            }
        }
    };
    auto store = [&](int buf) {
        if (MODE == CV_FWD || MODE == CV_DGRAD) {
#pragma unroll
            for (int i = 0; i < VA; ++i) *(u32x4*)&As[buf][(lr + 32 * i) * LP + kv * 8] = ra[i];
#pragma unroll
            for (int i = 0; i < VB; ++i) *(u32x4*)&Bs[buf][(lr + 32 * i) * LP + kv * 8] = rb[i];
        } else {                                                 // the transpose: row = channel, two consecutive pixels per dword
#pragma unroll
            for (int i = 0; i < VA / 2; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    *(uint32_t*)&As[buf][((cg + 8 * i) * 8 + j) * LP + 2 * pp] = half_of(ra[2 * i], j) | (half_of(ra[2 * i + 1], j) << 16);
#pragma unroll
            for (int i = 0; i < VB / 2; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    *(uint32_t*)&Bs[buf][((cg + 8 * i) * 8 + j) * LP + 2 * pp] = half_of(rb[2 * i], j) | (half_of(rb[2 * i + 1], j) << 16);
        }
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int x = 0; x < MI; ++x)
#pragma unroll
        for (int y = 0; y < NI; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kbeg < kend) {
        load(kbeg);
        store(0);
    }
    __syncthreads();
    int buf = 0;
    for (int k0 = kbeg; k0 < kend; k0 += 64, buf ^= 1) {
        const bool more = k0 + 64 < kend;
        if (more) load(k0 + 64);                                 // in flight under this stage's MFMAs
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            // 16x16x32 operand maps: A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15]
            bf16x8 fa[MI], fb[NI];
#pragma unroll
            for (int x = 0; x < MI; ++x) fa[x] = *(const bf16x8*)&As[buf][(wm + 16 * x + i16) * LP + ks * 32 + 8 * q];
#pragma unroll
            for (int y = 0; y < NI; ++y) fb[y] = *(const bf16x8*)&Bs[buf][(wn + 16 * y + i16) * LP + ks * 32 + 8 * q];
#pragma unroll
            for (int x = 0; x < MI; ++x)
#pragma unroll
                for (int y = 0; y < NI; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[x], fb[y], acc[x][y], 0, 0, 0);
        }
        if (more) store(buf ^ 1);                                // the other stage: last read before the previous barrier
        __syncthreads();
    }
    // C/D map: col = l & 15, row = 4 (l >> 4) + reg
#pragma unroll
    for (int x = 0; x < MI; ++x)
#pragma unroll
        for (int y = 0; y < NI; ++y)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm + 16 * x + 4 * q + e, col = n0 + wn + 16 * y + i16;
                if (row >= a.M || col >= a.N) continue;
                const long long o = (long long)row * a.N + col;
                float v = acc[x][y][e];
                if (MODE == CV_WGRAD) {
                    ((float*)a.out)[(long long)blockIdx.z * a.M * a.N + o] = v;
                } else {
                    if (MODE == CV_DGRAD && a.add) v = (a.add_f32 ? ((const float*)a.add)[o] : bf16_to_f32(((const bf16_t*)a.add)[o])) + v;
                    if (MODE == CV_DGRAD && a.out_f32) ((float*)a.out)[o] = v;
                    else ((bf16_t*)a.out)[o] = f32_to_bf16(v);
                }
            }
}

// fp32 OIHW master weights -> bf16 (RNE), channels padded with zeros to Cp: wf[co][r][s][c] and / or wd[c][r][s][co]
__global__ void __launch_bounds__(256) pack_weights_kernel(const float* __restrict__ w, int K, int C, int Cp, int R, int S,
                                                           bf16_t* __restrict__ wf, bf16_t* __restrict__ wd) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)K * R * S * Cp) return;
    const int c = (int)(idx % Cp);
    const long long p = idx / Cp;
    const int rs = (int)(p % (R * S)), co = (int)(p / (R * S));
    const bf16_t v = c < C ? f32_to_bf16(w[((long long)co * C + c) * R * S + rs]) : (bf16_t)0;
    if (wf) wf[idx] = v;
    if (wd) wd[((long long)c * R * S + rs) * K + co] = v;
}

// ---------------------------------------------------------------------------------------------------------------- 8 bf16 at a time
struct F8 {
    float v[8];
};
__device__ __forceinline__ F8 ld8(const bf16_t* p) {
    const u32x4 u = *(const u32x4*)p;
    F8 f;
#pragma unroll
    for (int j = 0; j < 4; ++j) unpack_bf16x2(u[j], f.v[2 * j], f.v[2 * j + 1]);
    return f;
}
__device__ __forceinline__ void st8(bf16_t* p, const F8& f) {
    u32x4 u;
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = pack_bf16x2(f.v[2 * j], f.v[2 * j + 1]);
    *(u32x4*)p = u;
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm, pools
// bf16 storage for the kernels of trunk_elem.inc: 8 channels = one 16-byte access per thread, RNE at the store
struct Bf16Store {
    using T = bf16_t;
    static constexpr int W = 8;
    using V = F8;
    static __device__ __forceinline__ float rd(bf16_t x) { return bf16_to_f32(x); }
    static __device__ __forceinline__ F8 ld(const bf16_t* p) { return ld8(p); }
    static __device__ __forceinline__ void st(bf16_t* p, const F8& f) { st8(p, f); }
};
#include "trunk_elem.inc"

// fp32 NCHW (n, C, HW) -> bf16 NHWC with 8 channels per pixel (C <= 8; channels C .. 7 zero), RNE
__global__ void __launch_bounds__(256) nchw_to_nhwc8_kernel(const float* __restrict__ x, int n, int C, int HW, bf16_t* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * HW) return;
    const int hw = (int)(idx % HW), b = (int)(idx / HW);
    F8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = j < C ? x[((long long)b * C + j) * HW + hw] : 0.f;
    st8(y + idx * 8, o);
}

// ---------------------------------------------------------------------------------------------------------------- host side
#include "trunk_walk.inc"

// the bf16 kernels' geometry: a 16-byte load holds 8 channels of one pixel / tap; packed weights indexed in 32 bits
bool geom_ok8(const Geom& g) {
    return geom_ok(g) && g.C % 8 == 0 && g.K % 8 == 0 && (long long)g.R * g.S * g.C * g.K < (1LL << 31);
}

// the 128 x 128 tile where it fills the part (256 CUs) and both sides reach it, else 64 x 64
bool big_tile(int M, int N) { return N >= 128 && M >= 128 && (long long)((M + 127) / 128) * ((N + 127) / 128) >= 256; }
bool wgrad_big(const Geom& g) { return g.K >= 128 && g.R * g.S * g.C >= 128; }

// split-K of the weight gradient: enough chunks for ~1024 workgroups of 64 x 64 (512 of 128 x 128), chunks of at least 512 pixels
// (a multiple of 64, one K stage)
void wgrad_split(const Geom& g, int* nch, int* chunk) {
    const int M = g.K, N = g.R * g.S * g.C, KK = g.n * g.Ho * g.Wo, T = wgrad_big(g) ? 128 : 64;
    const int tiles = ((M + T - 1) / T) * ((N + T - 1) / T), want = T == 128 ? 512 : 1024;
    const int s = std::max(1, std::min((want + tiles - 1) / tiles, (KK + 511) / 512));
    int ch = (KK + s - 1) / s;
    ch = (ch + 63) & ~63;
    *chunk = ch;
    *nch = (KK + ch - 1) / ch;
}

template <int MODE>
void launch_conv(const BArgs& a, int nz, bool big, hipStream_t st) {
    if (big) hipLaunchKernelGGL((bconv_kernel<MODE, 128, 128>), dim3((a.M + 127) / 128, (a.N + 127) / 128, nz), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((bconv_kernel<MODE, 64, 64>), dim3((a.M + 63) / 64, (a.N + 63) / 64, nz), dim3(256), 0, st, a);
}

hipError_t conv_fwd(const Geom& g, const bf16_t* x, const bf16_t* wf, bf16_t* y, hipStream_t st) {
    BArgs a = conv_args<BArgs>(g);
    a.a = x; a.b = wf; a.out = y;
    a.M = g.n * g.Ho * g.Wo; a.N = g.K; a.KK = g.R * g.S * g.C;
    launch_conv<CV_FWD>(a, 1, big_tile(a.M, a.N), st);
    return hipGetLastError();
}

hipError_t conv_dgrad(const Geom& g, const bf16_t* gy, const bf16_t* wd, const void* add, int add_f32, void* gx, int out_f32,
                      hipStream_t st) {
    BArgs a = conv_args<BArgs>(g);
    a.a = gy; a.b = wd; a.out = gx; a.add = add; a.add_f32 = add_f32; a.out_f32 = out_f32;
    a.M = g.n * g.H * g.W; a.N = g.C; a.KK = g.R * g.S * g.K;
    launch_conv<CV_DGRAD>(a, 1, big_tile(a.M, a.N), st);
    return hipGetLastError();
}

// gw (OIHW fp32, c_real <= C input channels) through `part` (wgrad_floats(g) floats)
hipError_t conv_wgrad(const Geom& g, const bf16_t* x, const bf16_t* gy, float* part, float* gw, int c_real, hipStream_t st) {
    BArgs a = conv_args<BArgs>(g);
    a.a = gy; a.b = x; a.out = part;
    a.M = g.K; a.N = g.R * g.S * g.C; a.KK = g.n * g.Ho * g.Wo;
    int nch;
    wgrad_split(g, &nch, &a.kchunk);
    launch_conv<CV_WGRAD>(a, nch, wgrad_big(g), st);
    const long long tot = (long long)g.K * c_real * g.R * g.S;
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(nblk(tot)), dim3(256), 0, st, part, nch, g.K, c_real, g.C, g.R, g.S, gw);
    return hipGetLastError();
}

void pack_weights(const float* w, int K, int C, int Cp, int R, int S, bf16_t* wf, bf16_t* wd, hipStream_t st) {
    hipLaunchKernelGGL(pack_weights_kernel, dim3(nblk((long long)K * R * S * Cp)), dim3(256), 0, st, w, K, C, Cp, R, S, wf, wd);
}

// ---------------------------------------------------------------------------------------------------------------- the trunk walks
// The bf16 backend of trunk_walk.inc: NHWC bf16 activations and activation gradients on channel counts padded to 8, a bf16 copy of
// the fp32 master weights packed into the workspace in front of every forward convolution (the fp32 parameter `w` goes unused
// after that), element-wise kernels on 8 channels per thread.
struct Bf16Ops : ElemOps<Bf16Store> {
    using L = Layer<bf16_t>;
    static constexpr const char *fwd_name = "apg_trunk_fwd_p", *bwd_name = "apg_trunk_bwd_p";
    static constexpr bool ws_aligned = true, packed = true;
    static int cpad(int C) { return (C + 7) & ~7; }
    static void pack(const L& l, const float* w, hipStream_t st) { pack_weights(w, l.g.K, l.c_real, l.g.C, l.g.R, l.g.S, l.wf, l.wd, st); }
    static hipError_t conv_fwd(const L& l, const float*, hipStream_t st) { return ::conv_fwd(l.g, l.in, l.wf, l.z, st); }
    static hipError_t conv_dgrad(const L& l, const bf16_t* gy, const float*, const bf16_t* add, bf16_t* gx, hipStream_t st) {
        return ::conv_dgrad(l.g, gy, l.wd, add, 0, gx, 0, st);
    }
    static hipError_t conv_wgrad(const L& l, const bf16_t* gz, float* part, float* gw, hipStream_t st) {
        return ::conv_wgrad(l.g, l.in, gz, part, gw, l.c_real, st);
    }
    static void crops_in(const float* x, int n, bf16_t* ximg, hipStream_t st) {
        hipLaunchKernelGGL(nchw_to_nhwc8_kernel, dim3(nblk((long long)n * IMG * IMG)), dim3(256), 0, st, x, n, 3, IMG * IMG, ximg);
    }
    // fp32 crop gradient: 8 channels per pixel in g2 (a bf16 buffer of the largest activation holds exactly that), then NCHW
    static hipError_t crop_grad(const L& stem, const float*, const bf16_t* g1, bf16_t* g2, int n, float* g_x, hipStream_t st) {
        hipError_t e = ::conv_dgrad(stem.g, g1, stem.wd, nullptr, 0, g2, 1, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(nblk((long long)n * 3 * IMG * IMG)), dim3(256), 0, st, (const float*)g2, n, 3, 8,
                           IMG * IMG, g_x);
        return hipGetLastError();
    }
    // the downsample's data gradient stays fp32 (g3 and g2 are free here and adjacent: 2 x big bytes hold the block input in fp32)
    // and conv1's data gradient adds it before the one rounding
    static hipError_t ds_block_dgrad(const L& ds, const float*, const bf16_t* gres, const L& c1, const float*, const bf16_t* g1,
                                     bf16_t* g3, bf16_t* gnext, hipStream_t st) {
        hipError_t e = ::conv_dgrad(ds.g, gres, ds.wd, nullptr, 0, g3, 1, st);
        if (e != hipSuccess) return e;
        return ::conv_dgrad(c1.g, g1, c1.wd, g3, 1, gnext, 0, st);
    }
};

}  // namespace

extern "C" {

int apg_trunk_precisions(void) { return (1 << APG_PREC_FP32) | (1 << APG_PREC_BF16); }

// ------------------------------------------------------------------------------------------------ primitives
int apg_pack_weights_bf16(const float* w, int K, int C, int Cp, int R, int S, void* wf, void* wd, void* stream) {
    if (!w || (!wf && !wd) || K <= 0 || C <= 0 || R <= 0 || S <= 0 || Cp < C || Cp % 8 != 0 || K % 8 != 0 || !al16(wf) || !al16(wd) ||
        (long long)K * R * S * Cp >= (1LL << 31))
        return apg_fail(APG_EINVAL, "apg_pack_weights_bf16: bad argument (Cp >= C and C_out multiples of 8, wf / wd 16-byte aligned)");
    pack_weights(w, K, C, Cp, R, S, (bf16_t*)wf, (bf16_t*)wd, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_conv_fwd_bf16(const void* x, int n, int H, int W, int C, const void* wf, int K, int R, int S, int stride, int pad, void* y,
                      void* stream) {
    const Geom g = make_geom(n, H, W, C, K, R, S, stride, pad);
    if (!x || !wf || !y || !geom_ok8(g) || !al16(x) || !al16(wf) || !al16(y))
        return apg_fail(APG_EINVAL, "apg_conv_fwd_bf16: bad argument (C and C_out multiples of 8, pointers 16-byte aligned)");
    APG_TRY(conv_fwd(g, (const bf16_t*)x, (const bf16_t*)wf, (bf16_t*)y, (hipStream_t)stream));
    return APG_OK;
}

int64_t apg_conv_bwd_bf16_workspace_bytes(int n, int H, int W, int C, int K, int R, int S, int stride, int pad) {
    const Geom g = make_geom(n, H, W, C, K, R, S, stride, pad);
    if (!geom_ok8(g)) return -1;
    return (int64_t)(wgrad_floats(g) * sizeof(float));
}

int apg_conv_bwd_bf16(const void* x, int n, int H, int W, int C, const void* wd, int K, int R, int S, int stride, int pad, const void* gy,
                      const void* add, int add_fp32, void* gx, int gx_fp32, float* gw, int gw_channels, void* workspace, int64_t workspace_bytes,
                      void* stream) {
    const Geom g = make_geom(n, H, W, C, K, R, S, stride, pad);
    if (!gy || !geom_ok8(g) || (!gx && !gw) || (gx && !wd) || (gw && !x) || !al16(gy) || !al16(x) || !al16(wd) || !al16(gx) || !al16(add) ||
        (add && (!gx || gx_fp32)) || (add && add_fp32 && add == gx) || (gw && (gw_channels <= 0 || gw_channels > C)))
        return apg_fail(APG_EINVAL, "apg_conv_bwd_bf16: bad argument (C and C_out multiples of 8, pointers 16-byte aligned, "
                                    "1 <= gw_channels <= C)");
    if (gw && (!workspace || workspace_bytes < (int64_t)(wgrad_floats(g) * sizeof(float))))
        return apg_fail(APG_ENOMEM, "apg_conv_bwd_bf16: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(wgrad_floats(g) * sizeof(float)) + " needed");
    hipStream_t st = (hipStream_t)stream;
    if (gx) APG_TRY(conv_dgrad(g, (const bf16_t*)gy, (const bf16_t*)wd, add, add_fp32 ? 1 : 0, gx, gx_fp32 ? 1 : 0, st));
    if (gw) APG_TRY(conv_wgrad(g, (const bf16_t*)x, (const bf16_t*)gy, (float*)workspace, gw, gw_channels, st));
    return APG_OK;
}

int64_t apg_bn_bf16_workspace_bytes(int M, int C) {
    if (M <= 0 || C <= 0 || C % 8 != 0) return -1;
    return (int64_t)(bn_part_floats(M, C) * sizeof(float));
}

int apg_bn_fwd_bf16(const void* x, int M, int C, const float* gamma, const float* beta, float* running_mean, float* running_var, int train,
                    float momentum, float eps, const void* res, int relu, void* y, float* save_mean, float* save_invstd, void* workspace,
                    int64_t workspace_bytes, void* stream) {
    if (!x || M <= 0 || C <= 0 || C % 8 != 0 || !gamma || !beta || !y || !save_mean || !save_invstd || !(eps >= 0.f) ||
        (!train && (!running_mean || !running_var)) || (!running_mean != !running_var) || !al16(x) || !al16(y) || !al16(res))
        return apg_fail(APG_EINVAL, "apg_bn_fwd_bf16: bad argument (C a multiple of 8, x / y / res 16-byte aligned)");
    if (train && (!workspace || workspace_bytes < apg_bn_bf16_workspace_bytes(M, C)))
        return apg_fail(APG_ENOMEM, "apg_bn_fwd_bf16: workspace too small");
    APG_TRY(bn_fwd<Bf16Store>((const bf16_t*)x, M, C, gamma, beta, running_mean, running_var, train, momentum, eps, (const bf16_t*)res,
                              relu, (bf16_t*)y, save_mean, save_invstd, (float*)workspace, (hipStream_t)stream));
    return APG_OK;
}

int apg_bn_bwd_bf16(const void* gy, const void* y, const void* x, int M, int C, const float* gamma, const float* save_mean,
                    const float* save_invstd, int train, void* gx, void* g_res, float* g_gamma, float* g_beta, void* workspace,
                    int64_t workspace_bytes, void* stream) {
    if (!gy || !x || M <= 0 || C <= 0 || C % 8 != 0 || !gamma || !save_mean || !save_invstd || !gx || !al16(gy) || !al16(y) || !al16(x) ||
        !al16(gx) || !al16(g_res))
        return apg_fail(APG_EINVAL, "apg_bn_bwd_bf16: bad argument (C a multiple of 8, activation pointers 16-byte aligned)");
    if (!workspace || workspace_bytes < apg_bn_bf16_workspace_bytes(M, C))
        return apg_fail(APG_ENOMEM, "apg_bn_bwd_bf16: workspace too small");
    APG_TRY(bn_bwd<Bf16Store>((const bf16_t*)gy, (const bf16_t*)y, (const bf16_t*)x, M, C, gamma, save_mean, save_invstd, train,
                              (bf16_t*)gx, (bf16_t*)g_res, g_gamma, g_beta, (float*)workspace, (hipStream_t)stream));
    return APG_OK;
}

int apg_maxpool_fwd_bf16(const void* x, int n, int H, int W, int C, void* y, void* stream) {
    if (!x || !y || n <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || !al16(x) || !al16(y) ||
        (long long)n * H * W * C >= (1LL << 31))
        return apg_fail(APG_EINVAL, "apg_maxpool_fwd_bf16: bad argument (C a multiple of 8, pointers 16-byte aligned)");
    Bf16Ops::maxpool_fwd((const bf16_t*)x, n, H, W, C, (bf16_t*)y, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_maxpool_bwd_bf16(const void* x, int n, int H, int W, int C, const void* gy, void* gx, void* stream) {
    if (!x || !gy || !gx || n <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || !al16(x) || !al16(gy) || !al16(gx) ||
        (long long)n * H * W * C >= (1LL << 31))
        return apg_fail(APG_EINVAL, "apg_maxpool_bwd_bf16: bad argument (C a multiple of 8, pointers 16-byte aligned)");
    Bf16Ops::maxpool_bwd((const bf16_t*)x, (const bf16_t*)gy, n, H, W, C, (bf16_t*)gx, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_avgpool_fwd_bf16(const void* x, int n, int C, float* y, void* stream) {
    if (!x || !y || n <= 0 || C <= 0) return apg_fail(APG_EINVAL, "apg_avgpool_fwd_bf16: bad argument");
    Bf16Ops::avgpool_fwd((const bf16_t*)x, n, C, y, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_avgpool_bwd_bf16(const float* gy, int n, int C, void* gx, void* stream) {
    if (!gy || !gx || n <= 0 || C <= 0 || C % 8 != 0 || !al16(gx))
        return apg_fail(APG_EINVAL, "apg_avgpool_bwd_bf16: bad argument (C a multiple of 8, gx 16-byte aligned)");
    Bf16Ops::avgpool_bwd(gy, n, C, (bf16_t*)gx, (hipStream_t)stream);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

// ------------------------------------------------------------------------------------------------ the trunk walker
int64_t apg_trunk_workspace_bytes_p(int n, int save, int precision) {
    if (precision == APG_PREC_FP32) return apg_trunk_workspace_bytes(n, save);
    if (precision != APG_PREC_BF16) return -1;
    return trunk_bytes<Bf16Ops>(n, save);
}

int apg_trunk_fwd_p(int precision, int n, const float* x, const void* const* params, int train, float momentum, float eps, float* xf,
                    int save, void* workspace, int64_t workspace_bytes, void* stream) {
    if (precision == APG_PREC_FP32) return apg_trunk_fwd(n, x, params, train, momentum, eps, xf, save, workspace, workspace_bytes, stream);
    if (precision != APG_PREC_BF16) return apg_fail(APG_EINVAL, "apg_trunk_fwd_p: unknown precision " + std::to_string(precision));
    return trunk_fwd_walk<Bf16Ops>(n, x, params, train, momentum, eps, xf, save, workspace, workspace_bytes, stream);
}

int apg_trunk_bwd_p(int precision, int n, const void* const* params, int train, const float* g_xf, void* const* g_params, float* g_x,
                    void* workspace, int64_t workspace_bytes, void* stream) {
    if (precision == APG_PREC_FP32) return apg_trunk_bwd(n, params, train, g_xf, g_params, g_x, workspace, workspace_bytes, stream);
    if (precision != APG_PREC_BF16) return apg_fail(APG_EINVAL, "apg_trunk_bwd_p: unknown precision " + std::to_string(precision));
    return trunk_bwd_walk<Bf16Ops>(n, params, train, g_xf, g_params, g_x, workspace, workspace_bytes, stream);
}

}  // extern "C"
