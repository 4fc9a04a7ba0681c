// Real-data batches (libairpose_grad.so): copenet_real.__getitem__ (copenet_real/dsets/copenet_real.py:162-258) and the agreement
// filter of its __init__ (:105-106) between the raw detections and the network's inputs, for n frames of a sequence and both views
// in one launch.  The semantics, the box invariant and the three rules that give it are in include/airpose_grad.h.
//
//   real_batch_kernel   grid = ceil(2 n / WPB), WPB = APG_BATCH_WAVES waves of 64: ONE WAVE per (view, frame); a wave past 2 n leaves
//     as a whole.  Lane j < 24 owns joint j of both detectors: it loads them, filters them (the comparison of seq_init_kernel, see
//     `apart`), and offers its OpenPose position to the box if the filtered confidence is not 0 and the position is finite, clamped
//     to the frame.  min / max of x and y and the two flags meet by xor shuffles over 32 .. 1 with every lane of the wave taking part
//     (lanes 24 .. 63 offer +inf / -inf); every lane ends with the same bits, so the box, bb and scale are computed redundantly per
//     lane and lane j puts its own two keypoints into crop coordinates.  Lane 0 stores the per-frame records.
//
// The box is integer work on a double: min x - border and max x + border are formed in fp64 (exact for fp32 x and an integer
// border, as the reference forms them on its float64 arrays) and compared with 0 and W BEFORE the conversion to int, so no
// conversion is out of range.  bb and j2d_crop are chains of single fp32 operations: this file is compiled with -ffp-contract=off
// (csrc/Makefile), and the one product-sum that seq_init_kernel's build fuses is written as an fmaf here.
// No LDS, no atomic, plain vector stores only.  Latency-bound: 2 n waves, 600 bytes in and 1.3 KB out each.
#include "grad_internal.h"

#include <cmath>
#include <string>

namespace {

constexpr int WPB = APG_BATCH_WAVES;     // waves (= (view, frame) pairs) per workgroup
constexpr int NT = 64 * WPB;
constexpr int NJ2 = 24;
constexpr int MAX_L = 1 << 22, MAX_SIDE = 1 << 20;

struct BatchArgs {
    int L, a, n;
    const float* det;
    float cx[2], cy[2];
    int H[2], W[2];
    float agreement_px;
    int border;
    float *j2d, *bb, *j2d_crop;
    int *crops, *crop_info, *status;
};

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// one axis of the box from the clamped extremes lo <= hi in [0, S]: -> 0 <= p0 < p1 <= S; true if it had to be widened
__device__ __forceinline__ bool box_axis(float lo, float hi, int border, int S, int& p0, int& p1) {
    const double t0 = (double)lo - (double)border, t1 = (double)hi + (double)border;      // t0 <= S, t1 >= 0
    p0 = t0 > 0.0 ? (int)t0 : 0;                                     // int(): towards zero
    p1 = t1 < (double)S ? (int)t1 : S;
    if (p1 > p0) return false;
    p0 = p0 < S - 1 ? p0 : S - 1;
    p1 = p0 + 1;
    return true;
}

__global__ void __launch_bounds__(NT) real_batch_kernel(const BatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (w >= 2 * a.n) return;                                        // the whole wave
    const int v = w / a.n, i = w - v * a.n, l = a.a + i;
    const int H = a.H[v], W = a.W[v];
    const bool live = lane < NJ2;
    const size_t in = (((size_t)v * a.L + l) * 2) * NJ2 * 3 + (size_t)lane * 3;           // detector 0; detector 1 is NJ2 * 3 further
    const size_t out = (((size_t)v * a.n + i) * 2) * NJ2 * 3 + (size_t)lane * 3;
    float x0 = 0.f, y0 = 0.f, c0 = 0.f, x1 = 0.f, y1 = 0.f, c1 = 0.f;
    if (live) {
        const float* p0 = a.det + in;
        const float* p1 = p0 + NJ2 * 3;
        x0 = p0[0]; y0 = p0[1]; c0 = p0[2]; x1 = p1[0]; y1 = p1[1]; c1 = p1[2];
    }
    // seq_init_kernel's comparison, bit for bit: its build contracts dx * dx + dy * dy into fma(dx, dx, dy * dy)
    const float dx = x0 - x1, dy = y0 - y1;
    const bool apart = sqrtf(fmaf(dx, dx, dy * dy)) > a.agreement_px;
    c0 = apart ? 0.f : c0;
    c1 = apart ? 0.f : c1;

    const bool used = live && c0 != 0.f;                             // the reference's opose[..., 2] != 0 (a NaN confidence counts)
    const bool there = used && finite_bits(x0) && finite_bits(y0);   // a non-finite keypoint is absent
    const float fW = (float)W, fH = (float)H;                        // (exact: W, H <= 2^20)
    const float xc = fminf(fmaxf(x0, 0.f), fW), yc = fminf(fmaxf(y0, 0.f), fH);
    const bool moved = used && (!there || xc != x0 || yc != y0);
    const float inf = __uint_as_float(0x7f800000u);
    float xlo = wave_min(there ? xc : inf), xhi = wave_max(there ? xc : -inf);
    float ylo = wave_min(there ? yc : inf), yhi = wave_max(there ? yc : -inf);
    const bool any = __ballot(there) != 0ull, clamped = __ballot(moved) != 0ull;
    if (!any) xlo = xhi = ylo = yhi = 0.f;                           // x = y = np.array([0])

    int bx0, bx1, by0, by1;
    const bool wx = box_axis(xlo, xhi, a.border, W, bx0, bx1);
    const bool wy = box_axis(ylo, yhi, a.border, H, by0, by1);
    const int bh = by1 - by0, bw = bx1 - bx0;
    const float scale = (float)(224.0 / (double)(bh > bw ? bh : bw));                     // preprocess_kernel's expression
    const float cx = a.cx[v], cy = a.cy[v];
    const float bbx = (float)(bx0 + bx1) / 2.f / cx - 1.f;           // (x0 + x1) / 2 is exact; one rounding in / and one in -
    const float bby = (float)(by0 + by1) / 2.f / cy - 1.f;
    const float ox = (bbx + 1.f) * cx, oy = (bby + 1.f) * cy;

    if (live) {
        float* q0 = a.j2d + out;
        float* q1 = q0 + NJ2 * 3;
        q0[0] = x0; q0[1] = y0; q0[2] = c0;
        q1[0] = x1; q1[1] = y1; q1[2] = c1;
        float* r0 = a.j2d_crop + out;
        float* r1 = r0 + NJ2 * 3;
        r0[0] = scale * (x0 - ox); r0[1] = scale * (y0 - oy); r0[2] = c0;
        r1[0] = scale * (x1 - ox); r1[1] = scale * (y1 - oy); r1[2] = c1;
    }
    if (lane == 0) {
        const size_t f = (size_t)v * a.n + i;
        int* c = a.crops + f * 4;
        c[0] = by0; c[1] = by1; c[2] = bx0; c[3] = bx1;
        int* ci = a.crop_info + f * 4;
        ci[0] = by0; ci[1] = bx0; ci[2] = by1; ci[3] = bx1;
        float* b = a.bb + f * 3;
        b[0] = bbx; b[1] = bby; b[2] = scale;
        a.status[f] = (any ? 0 : APG_BATCH_FALLBACK) | (clamped ? APG_BATCH_CLAMPED : 0) | ((wx || wy) ? APG_BATCH_WIDENED : 0);
    }
}

}  // namespace

extern "C" int apg_real_batch(int L, int a, int n, const float* det, const float* principal, const int* size, float agreement_px,
                              int border, float* j2d, int* crops, int* crop_info, float* bb, float* j2d_crop, int* status,
                              void* stream) {
    const std::string f = "apg_real_batch: ";
    const ApgPtr ps[] = {{det, "det", 4}, {principal, "principal", 4}, {size, "size", 4}, {j2d, "j2d", 4}, {crops, "crops", 4},
                         {crop_info, "crop_info", 4}, {bb, "bb", 4}, {j2d_crop, "j2d_crop", 4}, {status, "status", 4}};
    if (int rc = apg_check_ptrs(f, ps, 9)) return rc;
    if (L < 1 || L > MAX_L) return apg_fail(APG_EINVAL, f + "L must be in 1 .. " + std::to_string(MAX_L));
    if (n < 1) return apg_fail(APG_EINVAL, f + "n must be at least 1");
    if (a < 0) return apg_fail(APG_EINVAL, f + "a must not be negative");
    if (a > L - n) return apg_fail(APG_EINVAL, f + "a + n must not exceed L");
    if (!std::isfinite(agreement_px) || agreement_px < 0.f)
        return apg_fail(APG_EINVAL, f + "agreement_px must be finite and not negative");
    if (border < 0 || border > MAX_SIDE) return apg_fail(APG_EINVAL, f + "border must be in 0 .. " + std::to_string(MAX_SIDE));
    if ((const void*)j2d == (const void*)det) return apg_fail(APG_EINVAL, f + "j2d must not be det");
    BatchArgs k = {L, a, n, det, {}, {}, {}, {}, agreement_px, border, j2d, bb, j2d_crop, crops, crop_info, status};
    for (int v = 0; v < 2; ++v) {
        const int H = size[2 * v], W = size[2 * v + 1];
        const float cx = principal[2 * v], cy = principal[2 * v + 1];
        if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE)
            return apg_fail(APG_EINVAL, f + "size of view " + std::to_string(v) + " must be in 1 .. " + std::to_string(MAX_SIDE));
        if (!std::isfinite(cx) || !std::isfinite(cy) || cx <= 0.f || cy <= 0.f)
            return apg_fail(APG_EINVAL, f + "principal point of view " + std::to_string(v) + " must be finite and positive");
        k.H[v] = H; k.W[v] = W; k.cx[v] = cx; k.cy[v] = cy;
    }
    hipLaunchKernelGGL(real_batch_kernel, dim3((unsigned)((2 * n + WPB - 1) / WPB)), dim3(NT), 0, (hipStream_t)stream, k);
    APG_TRY(hipGetLastError());
    return APG_OK;
}
