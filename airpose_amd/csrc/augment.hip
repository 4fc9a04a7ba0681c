// Crop augmentation (libairpose_grad.so): blur, colour, gamma, noise and occluders on the (2, n, 3, 224, 224) crops of apg_synth_crops
// and ap_preprocess_crops.  The contract -- the parameter set, the stages and their order, the draws, the status bits -- is in
// include/airpose_grad.h; the reference only lists its augmentations, commented out (copenet/src/copenet/dsets/aerialpeople.py:72-76).
//
//   augment_draw_kernel    grid = ceil(2 n / 64): one thread per (suffix, sample) writes that image's whole parameter set.  The
//     colour matrix and the blur taps are composed in fp64 and rounded once; every uniform range is lo + u (hi - lo) in fp32.
//   augment_crops_kernel   grid = (49 tiles, n, 2 suffixes), APG_AUG_THREADS threads: one 32 x 32 tile per workgroup, four pixels
//     in a row and all three channels per thread.  An image with nothing to do, and a tile that holds no content pixel, is a copy
//     of the thread's own 16-byte loads.  With a blur of radius r (uniform per image, hence per workgroup) the tile and its halo,
//     (32 + 2 r)^2 x 3 de-normalised values with their coordinates clamped to the content rectangle, are staged in LDS (44 x 45 x 3
//     floats, the row padded by one bank), the horizontal pass goes LDS -> LDS (44 x 33 x 3) and the vertical pass leaves the
//     thread's pixels in registers, where colour, gamma, noise, the occluders and the re-normalisation run: 41 KB of LDS, three
//     workgroups per CU.  The image is read once (plus the halo) and written once.
// Compiled with -ffp-contract=off -fno-slp-vectorize (csrc/Makefile): every stage outside libm is a chain of single fp32 roundings
// in the written order, and there is no packed fp32 math.  No atomic, plain vector stores only.
#include "grad_internal.h"

#include <cmath>
#include <string>

namespace {

constexpr int IMG = 224, TILE = APG_AUG_TILE, NT = APG_AUG_THREADS, RMAX = APG_AUG_MAX_RADIUS, NRECT = APG_AUG_MAX_RECTS;
constexpr int TILES = IMG / TILE, HALO = TILE + 2 * RMAX;
constexpr int MAX_N = 65535;
static_assert(TILES * TILE == IMG && TILE * TILE == NT * 4 && TILE % 4 == 0, "a thread takes four pixels of a row");

struct DrawArgs {
    int n, cam_all;
    uint32_t k0, k1, epoch;
    const int *index, *cam;
    float cfg[APG_AUG_CFG];
    float *taps, *color, *gamma, *nsig, *rgb;
    int *rects, *status;
};

struct CropArgs {
    int n, vec, cam_all;
    uint32_t k0, k1, epoch;
    const int *index, *cam, *crops, *rects;
    const float *im, *taps, *color, *gamma, *nsig, *rgb;
    float* out;
    int* status;
};

#include "draws.inc"

__device__ __forceinline__ float range(uint32_t w, float lo, float hi) { return lo + uni(w) * (hi - lo); }
__device__ __forceinline__ float clamp01(float t) { return fminf(fmaxf(t, 0.f), 1.f); }
__device__ __forceinline__ bool is_fin(float t) { return fabsf(t) < INFINITY; }

// m = a m, 3 x 3 in fp64, row by column
__device__ __forceinline__ void left_mul(const double a[9], double m[9]) {
    double o[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[r * 3 + c] = (a[r * 3] * m[c] + a[r * 3 + 1] * m[3 + c]) + a[r * 3 + 2] * m[6 + c];
#pragma unroll
    for (int e = 0; e < 9; ++e) m[e] = o[e];
}

// t L + u I, L's rows the luma weights
__device__ __forceinline__ void luma_mix(double t, double u, double a[9]) {
    const double L[3] = {0.299, 0.587, 0.114};
#pragma unroll
    for (int e = 0; e < 9; ++e) a[e] = t * L[e % 3] + (e % 4 == 0 ? u : 0.0);
}

__global__ void __launch_bounds__(64) augment_draw_kernel(const DrawArgs a) {
    const int g = blockIdx.x * 64 + threadIdx.x, n = a.n;
    if (g >= 2 * n) return;
    const int s = g / n, i = g - s * n;
    const uint32_t idx = (uint32_t)a.index[i], cam = (uint32_t)(((a.cam ? a.cam[i] : a.cam_all) & 1) ^ s);
    const float* cfg = a.cfg;
    const float p = cfg[0];
    int st = 0;
    U4 d = philox(idx, a.epoch, cam, 1u, a.k0, a.k1);
    // the blur's taps
    {
        float w[RMAX + 1] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float sg = range(d.w[1], cfg[1], cfg[2]);
        if ((cfg[1] != 0.f || cfg[2] != 0.f) && uni(d.w[0]) < p && sg > 0.f) {
            const double sd = (double)sg;
            int r = (int)ceil(3.0 * sd);
            if (r > RMAX) { r = RMAX; st |= APG_AUG_BLUR_CLAMPED; }
            double e[RMAX + 1], sum = 1.0;
#pragma unroll
            for (int k = 1; k <= RMAX; ++k) {
                e[k] = k <= r ? exp(-(double)(k * k) / (2.0 * sd * sd)) : 0.0;
                sum += 2.0 * e[k];
            }
            w[0] = (float)(1.0 / sum);
#pragma unroll
            for (int k = 1; k <= RMAX; ++k) w[k] = (float)(e[k] / sum);
        }
#pragma unroll
        for (int k = 0; k <= RMAX; ++k) a.taps[(size_t)g * (RMAX + 1) + k] = w[k];
    }
    // [M | b]
    {
        double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[9];
        const float beta = cfg[3] != 0.f && uni(d.w[2]) < p ? range(d.w[3], -cfg[3], cfg[3]) : 0.f;
        const U4 d3 = philox(idx, a.epoch, cam, 3u, a.k0, a.k1);
        if ((cfg[7] != 1.f || cfg[8] != 1.f) && uni(d3.w[0]) < p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c * 4] = (double)range(d3.w[1 + c], cfg[7], cfg[8]);
        }
        const U4 d2 = philox(idx, a.epoch, cam, 2u, a.k0, a.k1);
        if (cfg[4] != 0.f && uni(d2.w[0]) < p) {
            const double th = (double)range(d2.w[1], -cfg[4], cfg[4]) * (3.141592653589793 / 180.0);
            const double cs = cos(th), sn = sin(th);
            const double K[9] = {0.168, 0.330, -0.497, -0.328, 0.035, 0.292, 1.25, -1.05, -0.203};
            luma_mix(1.0 - cs, cs, t);                       // L + cos (I - L)
#pragma unroll
            for (int e = 0; e < 9; ++e) t[e] += sn * K[e];
            left_mul(t, m);
        }
        if ((cfg[5] != 1.f || cfg[6] != 1.f) && uni(d2.w[2]) < p) {
            const double sat = (double)range(d2.w[3], cfg[5], cfg[6]);
            luma_mix(1.0 - sat, sat, t);
            left_mul(t, m);
        }
        const U4 d5 = philox(idx, a.epoch, cam, 5u, a.k0, a.k1);
        if ((cfg[11] != 0.f || cfg[12] != 0.f) && uni(d5.w[0]) < p) {
            const double al = (double)range(d5.w[1], cfg[11], cfg[12]);
            luma_mix(al, 1.0 - al, t);
            left_mul(t, m);
        }
        float* o = a.color + (size_t)g * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[r * 4 + c] = (float)m[r * 3 + c];
            o[r * 4 + 3] = beta;
        }
        a.nsig[g] = (cfg[13] != 0.f || cfg[14] != 0.f) && uni(d5.w[2]) < p ? range(d5.w[3], cfg[13], cfg[14]) : 0.f;
    }
    {
        const U4 d4 = philox(idx, a.epoch, cam, 4u, a.k0, a.k1);
        const bool on = (cfg[9] != 1.f || cfg[10] != 1.f) && uni(d4.w[0]) < p;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.gamma[(size_t)g * 3 + c] = on ? range(d4.w[1 + c], cfg[9], cfg[10]) : 1.f;
    }
    {
        const int count = (int)cfg[15];
        const bool on = count > 0 && uni(philox(idx, a.epoch, cam, 6u, a.k0, a.k1).w[0]) < p;
        for (int j = 0; j < NRECT; ++j) {
            int* rc = a.rects + ((size_t)g * NRECT + j) * 4;
            float* col = a.rgb + ((size_t)g * NRECT + j) * 3;
            if (on && j < count) {
                const U4 b = philox(idx, a.epoch, cam, 7u + j, a.k0, a.k1), c = philox(idx, a.epoch, cam, 11u + j, a.k0, a.k1);
                const int hy = (int)(range(b.w[0], cfg[16], cfg[17]) * 224.f), hx = (int)(range(b.w[1], cfg[16], cfg[17]) * 224.f);
                const int cy = (int)(uni(b.w[2]) * 224.f), cx = (int)(uni(b.w[3]) * 224.f);
                rc[0] = cy - hy / 2; rc[1] = rc[0] + hy; rc[2] = cx - hx / 2; rc[3] = rc[2] + hx;
                col[0] = uni(c.w[0]); col[1] = uni(c.w[1]); col[2] = uni(c.w[2]);
            } else {
                rc[0] = rc[1] = rc[2] = rc[3] = 0;
                col[0] = col[1] = col[2] = 0.f;
            }
        }
    }
    a.status[g] = st;
}

__global__ void __launch_bounds__(NT) augment_crops_kernel(const CropArgs a) {
    __shared__ float s_t[3][HALO][HALO + 1];
    __shared__ float s_h[3][HALO][TILE + 1];
    __shared__ float s_w[2 * RMAX + 1];
    const int tid = threadIdx.x, i = blockIdx.y, s = blockIdx.z, n = a.n;
    const int oy = (blockIdx.x / TILES) * TILE, ox = (blockIdx.x % TILES) * TILE;
    const size_t f = (size_t)s * n + i;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    int st = 0;

    // the content rectangle: preprocess_px.inc's expressions (h and w in 64 bits, so that no box overflows them)
    const int* cr = a.crops + f * 4;
    const int by0 = cr[0], by1 = cr[1], bx0 = cr[2], bx1 = cr[3];
    int cy0 = 0, cy1 = 0, cx0 = 0, cx1 = 0;
    if (by1 > by0 && bx1 > bx0) {
        const long long h = (long long)by1 - by0, w = (long long)bx1 - bx0;
        const double scale = 224.0 / (double)(h > w ? h : w);
        const int dw = (int)(scale * (double)w), dh = (int)(scale * (double)h);
        cy0 = (224 - dh) / 2; cy1 = cy0 + dh; cx0 = (224 - dw) / 2; cx1 = cx0 + dw;
    } else {
        st |= APG_AUG_BAD_BOX;
    }
    const bool content = cy1 > cy0 && cx1 > cx0;

    // the parameter set, made safe: the same for every thread of the workgroup
    float taps[RMAX + 1];
    int r = 0;
    {
        bool ok = true;
#pragma unroll
        for (int k = 0; k <= RMAX; ++k) {
            taps[k] = a.taps[f * (RMAX + 1) + k];
            ok = ok && is_fin(taps[k]);
            if (k && taps[k] != 0.f) r = k;
        }
        if (!ok) { r = 0; st |= APG_AUG_NONFINITE; }
    }
    float M[12];
    bool colour = false;
    {
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            M[e] = a.color[f * 12 + e];
            ok = ok && is_fin(M[e]);
            colour = colour || M[e] != (e % 5 == 0 ? 1.f : 0.f);
        }
        if (!ok) { colour = false; st |= APG_AUG_NONFINITE; }
    }
    float gam[3];
    bool any_gamma = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gam[c] = a.gamma[f * 3 + c];
        if (!(gam[c] >= 0.f && gam[c] < INFINITY)) { gam[c] = 1.f; st |= APG_AUG_NONFINITE; }
        any_gamma = any_gamma || gam[c] != 1.f;
    }
    float nsig = a.nsig[f];
    if (!is_fin(nsig)) { nsig = 0.f; st |= APG_AUG_NONFINITE; }
    int ry0[NRECT], ry1[NRECT], rx0[NRECT], rx1[NRECT];
    float rgb[NRECT][3];
    bool any_rect = false;
#pragma unroll
    for (int k = 0; k < NRECT; ++k) {
        const int* q = a.rects + (f * NRECT + k) * 4;
        const int y0 = q[0], y1 = q[1], x0 = q[2], x1 = q[3];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = a.rgb[(f * NRECT + k) * 3 + c];
            ok = ok && is_fin(t);
            rgb[k][c] = clamp01(t);
        }
        const bool filled = y1 > y0 && x1 > x0;
        if (filled && !ok) st |= APG_AUG_NONFINITE;
        ry0[k] = max(y0, cy0); ry1[k] = min(y1, cy1); rx0[k] = max(x0, cx0); rx1[k] = min(x1, cx1);
        if (filled && ok && content && (ry0[k] != y0 || ry1[k] != y1 || rx0[k] != x0 || rx1[k] != x1)) st |= APG_AUG_RECT_CLIPPED;
        if (!filled || !ok) ry1[k] = ry0[k];                 // empty
        any_rect = any_rect || (filled && ok);               // (before the clip: the header's "empty" is y1 <= y0 or x1 <= x0)
    }
    if (blockIdx.x == 0 && tid == 0) a.status[f] = st;

    // the thread's four pixels
    const int py = oy + tid / (TILE / 4), px = ox + (tid % (TILE / 4)) * 4;
    const float* src = a.im + f * 3 * IMG * IMG;
    float* dst = a.out + f * 3 * IMG * IMG;
    float in[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* q = src + ((size_t)c * IMG + py) * IMG + px;
        if (a.vec) {
            const float4 t = *reinterpret_cast<const float4*>(q);
            in[c][0] = t.x; in[c][1] = t.y; in[c][2] = t.z; in[c][3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) in[c][j] = q[j];
        }
    }
    float res[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) res[c][j] = in[c][j];

    const bool work = content && (r > 0 || colour || any_gamma || nsig != 0.f || any_rect);
    const bool here = oy < cy1 && oy + TILE > cy0 && ox < cx1 && ox + TILE > cx0;        // the tile holds a content pixel
    if (work && here) {                                      // (uniform over the workgroup: the barriers below are reached by all)
        float v[3][4];
        if (r > 0) {
            const int side = TILE + 2 * r;                   // <= HALO
            if (tid <= 2 * r) s_w[tid] = a.taps[f * (RMAX + 1) + (tid < r ? r - tid : tid - r)];  // s_w[r + k] = w_|k|
            // staging: a wave takes one row of the halo tile (64 lanes, `side` of them in use), the four waves four rows a step;
            // no division by `side`.  (No loop vectorisation: two iterations at once would de-normalise with v_pk_mul_f32 / v_pk_add_f32)
            const int sx = tid & 63;
            if (sx < side) {
                const int gx = min(max(ox - r + sx, cx0), cx1 - 1);
#pragma clang loop vectorize(disable) interleave(disable)
                for (int sy = tid >> 6; sy < side; sy += NT / 64) {
                    const int gy = min(max(oy - r + sy, cy0), cy1 - 1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) s_t[c][sy][sx] = src[((size_t)c * IMG + gy) * IMG + gx] * stdv[c] + mean[c];
                }
            }
            __syncthreads();
            const int hx = tid & (TILE - 1);                               // the horizontal pass, every staged row: eight rows a step
#pragma clang loop vectorize(disable) interleave(disable)
            for (int hy = tid / TILE; hy < side; hy += NT / TILE) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float t = s_w[0] * s_t[c][hy][hx];
                    for (int k = 1; k <= 2 * r; ++k) t = t + s_w[k] * s_t[c][hy][hx + k];
                    s_h[c][hy][hx] = t;
                }
            }
            __syncthreads();
            const int ly = tid / (TILE / 4), lx = (tid % (TILE / 4)) * 4;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {                              // the vertical pass
                    float t = s_w[0] * s_h[c][ly][lx + j];
                    for (int k = 1; k <= 2 * r; ++k) t = t + s_w[k] * s_h[c][ly + k][lx + j];
                    v[c][j] = t;
                }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[c][j] = in[c][j] * stdv[c] + mean[c];
        }
        const uint32_t idx = (uint32_t)a.index[i], cam = (uint32_t)(((a.cam ? a.cam[i] : a.cam_all) & 1) ^ s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = px + j;
            if (py < cy0 || py >= cy1 || x < cx0 || x >= cx1) continue;    // padding: the copy stands
            float p0 = v[0][j], p1 = v[1][j], p2 = v[2][j];
            if (colour) {
                const float q0 = clamp01(((M[0] * p0 + M[1] * p1) + M[2] * p2) + M[3]);
                const float q1 = clamp01(((M[4] * p0 + M[5] * p1) + M[6] * p2) + M[7]);
                const float q2 = clamp01(((M[8] * p0 + M[9] * p1) + M[10] * p2) + M[11]);
                p0 = q0; p1 = q1; p2 = q2;
            }
            if (gam[0] != 1.f) p0 = powf(clamp01(p0), gam[0]);
            if (gam[1] != 1.f) p1 = powf(clamp01(p1), gam[1]);
            if (gam[2] != 1.f) p2 = powf(clamp01(p2), gam[2]);
            if (nsig != 0.f) {
                const U4 d = philox(idx, a.epoch, cam, 0x80000000u | (uint32_t)(py * IMG + x), a.k0, a.k1);
                const float ra = sqrtf(-2.f * logf((float)((d.w[0] >> 8) + 1u) * (1.0f / 16777216.0f)));
                const float rb = sqrtf(-2.f * logf((float)((d.w[2] >> 8) + 1u) * (1.0f / 16777216.0f)));
                const float pa = 6.2831855f * uni(d.w[1]), pb = 6.2831855f * uni(d.w[3]);
                p0 = clamp01(p0 + nsig * (ra * cosf(pa)));
                p1 = clamp01(p1 + nsig * (ra * sinf(pa)));
                p2 = clamp01(p2 + nsig * (rb * cosf(pb)));
            }
#pragma unroll
            for (int k = 0; k < NRECT; ++k)
                if (py >= ry0[k] && py < ry1[k] && x >= rx0[k] && x < rx1[k]) { p0 = rgb[k][0]; p1 = rgb[k][1]; p2 = rgb[k][2]; }
            res[0][j] = (p0 - mean[0]) / stdv[0];
            res[1][j] = (p1 - mean[1]) / stdv[1];
            res[2][j] = (p2 - mean[2]) / stdv[2];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* q = dst + ((size_t)c * IMG + py) * IMG + px;
        if (a.vec) {
            *reinterpret_cast<float4*>(q) = make_float4(res[c][0], res[c][1], res[c][2], res[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = res[c][j];
        }
    }
}

int check_n_cam(const std::string& f, int n, const int* cam, int cam_all) {
    if (n < 1 || n > MAX_N) return apg_fail(APG_EINVAL, f + "n must be in 1 .. " + std::to_string(MAX_N));
    if ((uintptr_t)cam & 3u) return apg_fail(APG_EINVAL, f + "cam is not 4-byte aligned");
    if (cam_all != 0 && cam_all != 1) return apg_fail(APG_EINVAL, f + "cam_all must be 0 or 1");
    return APG_OK;
}

}  // namespace

extern "C" int apg_augment_draw(int n, uint64_t seed, int epoch, const int* index, const int* cam, int cam_all,
                                const float* cfg, float* blur_taps, float* color, float* gamma, float* noise_sigma, int* rects,
                                float* rect_rgb, int* status, void* stream) {
    const std::string f = "apg_augment_draw: ";
    const ApgPtr ps[] = {{index, "index", 4}, {cfg, "cfg", 4}, {blur_taps, "blur_taps", 4}, {color, "color", 4}, {gamma, "gamma", 4},
                         {noise_sigma, "noise_sigma", 4}, {rects, "rects", 4}, {rect_rgb, "rect_rgb", 4}, {status, "status", 4}};
    if (int rc = apg_check_ptrs(f, ps, 9)) return rc;
    if (int rc = check_n_cam(f, n, cam, cam_all)) return rc;
    DrawArgs k = {n, cam_all, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, index, cam, {}, blur_taps, color, gamma,
                  noise_sigma, rect_rgb, rects, status};
    for (int e = 0; e < APG_AUG_CFG; ++e) {
        if (!std::isfinite(cfg[e])) return apg_fail(APG_EINVAL, f + "cfg[" + std::to_string(e) + "] must be finite");
        k.cfg[e] = cfg[e];
    }
    if (!(cfg[0] >= 0.f && cfg[0] <= 1.f)) return apg_fail(APG_EINVAL, f + "cfg[0] (p) must be in 0 .. 1");
    if (!(cfg[15] >= 0.f && cfg[15] <= (float)NRECT && cfg[15] == (float)(int)cfg[15]))
        return apg_fail(APG_EINVAL, f + "cfg[15] (occluders) must be a whole number in 0 .. " + std::to_string(NRECT));
    if (!(cfg[16] >= 0.f && cfg[17] <= 1.f)) return apg_fail(APG_EINVAL, f + "cfg[16], cfg[17] (occluder side) must be in 0 .. 1");
    hipLaunchKernelGGL(augment_draw_kernel, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

extern "C" int apg_augment_crops(int n, uint64_t seed, int epoch, const int* index, const int* cam, int cam_all,
                                 const float* im, const int* crops, const float* blur_taps, const float* color, const float* gamma,
                                 const float* noise_sigma, const int* rects, const float* rect_rgb, float* out, int* status,
                                 void* stream) {
    const std::string f = "apg_augment_crops: ";
    const ApgPtr ps[] = {{index, "index", 4}, {im, "im", 4}, {crops, "crops", 4}, {blur_taps, "blur_taps", 4}, {color, "color", 4},
                         {gamma, "gamma", 4}, {noise_sigma, "noise_sigma", 4}, {rects, "rects", 4}, {rect_rgb, "rect_rgb", 4},
                         {out, "out", 4}, {status, "status", 4}};
    if (int rc = apg_check_ptrs(f, ps, 11)) return rc;
    if (int rc = check_n_cam(f, n, cam, cam_all)) return rc;
    const uintptr_t bytes = (uintptr_t)2 * n * 3 * IMG * IMG * sizeof(float), i0 = (uintptr_t)im, o0 = (uintptr_t)out;
    if (i0 < o0 + bytes && o0 < i0 + bytes) return apg_fail(APG_EINVAL, f + "out must not overlap im");
    const CropArgs k = {n, ((i0 | o0) & 15u) == 0, cam_all, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, index, cam, crops,
                        rects, im, blur_taps, color, gamma, noise_sigma, rect_rgb, out, status};
    hipLaunchKernelGGL(augment_crops_kernel, dim3(TILES * TILES, (unsigned)n, 2), dim3(NT), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    return APG_OK;
}
