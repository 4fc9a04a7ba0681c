// Geometry adjoints for gfx950 (libairpose_grad.so), and the library's version / error entry points.
//   rot6d_bwd_kernel       thread = rotation: the Gram-Schmidt map of rot6d_dev (smplx.hip) backwards, F.normalize's
//                          clamp_min(1e-12) included (below the clamp the norm is a constant: g_v = g_b / 1e-12)
//   projection_bwd_kernel  workgroup = body: per-point g_pts, and g_rotation / g_translation / g_center reduced over the
//                          body's points (strided per-thread sums in point order, then a fixed LDS tree)
//   transform_bwd_kernel   workgroup = body: per-point g_pts, g_rt reduced the same way
// No atomics: a body's gradients depend only on that body, bit for bit.
#include "grad_internal.h"

#include <string>

namespace {

thread_local std::string g_err;

#include "loss_common.inc"               // LT (threads per body) and block_reduce; result k in s[k * LT]

__device__ __forceinline__ void normalize_bwd(const float* a, const float* b, float nrm, bool clamped, const float* gb, float* ga) {
    // b = a / max(|a|, eps):  g_a = (g_b - b (b . g_b)) / |a|, or g_b / eps below the clamp
    if (clamped) {
        for (int k = 0; k < 3; ++k) ga[k] = gb[k] / nrm;
    } else {
        const float d = b[0] * gb[0] + b[1] * gb[1] + b[2] * gb[2];
        for (int k = 0; k < 3; ++k) ga[k] = (gb[k] - b[k] * d) / nrm;
    }
    (void)a;
}

__global__ void __launch_bounds__(256) rot6d_bwd_kernel(const float* __restrict__ x6, int n, const float* __restrict__ gR,
                                                        float* __restrict__ gx) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float* x = x6 + (size_t)idx * 6;
    const float a1[3] = {x[0], x[2], x[4]}, a2[3] = {x[1], x[3], x[5]};
    const float r1 = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
    const float n1 = fmaxf(r1, 1e-12f);
    const float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const float d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const float r2 = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const float n2 = fmaxf(r2, 1e-12f);
    const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    // R columns b1 b2 b3: R[k][0] = b1_k, R[k][1] = b2_k, R[k][2] = b3_k
    const float* g = gR + (size_t)idx * 9;
    float gb1[3] = {g[0], g[3], g[6]}, gb2[3] = {g[1], g[4], g[7]};
    const float gb3[3] = {g[2], g[5], g[8]};
    // b3 = b1 x b2:  g_b1 += b2 x g_b3,  g_b2 += g_b3 x b1
    gb1[0] += b2[1] * gb3[2] - b2[2] * gb3[1];
    gb1[1] += b2[2] * gb3[0] - b2[0] * gb3[2];
    gb1[2] += b2[0] * gb3[1] - b2[1] * gb3[0];
    gb2[0] += gb3[1] * b1[2] - gb3[2] * b1[1];
    gb2[1] += gb3[2] * b1[0] - gb3[0] * b1[2];
    gb2[2] += gb3[0] * b1[1] - gb3[1] * b1[0];
    float gu[3];
    normalize_bwd(u, b2, n2, !(r2 > 1e-12f), gb2, gu);
    // u = a2 - d b1, d = b1 . a2
    const float gd = -(gu[0] * b1[0] + gu[1] * b1[1] + gu[2] * b1[2]);
    float ga2[3];
    for (int k = 0; k < 3; ++k) {
        gb1[k] += -d * gu[k] + gd * a2[k];
        ga2[k] = gu[k] + gd * b1[k];
    }
    float ga1[3];
    normalize_bwd(a1, b1, n1, !(r1 > 1e-12f), gb1, ga1);
    float* o = gx + (size_t)idx * 6;
    o[0] = ga1[0]; o[2] = ga1[1]; o[4] = ga1[2];
    o[1] = ga2[0]; o[3] = ga2[1]; o[5] = ga2[2];
}

// out = (fx X / Z + cx, fy Y / Z + cy), [X Y Z] = R p + t
__global__ void __launch_bounds__(LT) projection_bwd_kernel(const float* __restrict__ pts, int P, const float* __restrict__ R,
                                                            const float* __restrict__ tr, float fx, float fy,
                                                            const float* __restrict__ gout, float* __restrict__ gpts,
                                                            float* __restrict__ gR, float* __restrict__ gt,
                                                            float* __restrict__ gc) {
    __shared__ float s[14 * LT];
    const int b = blockIdx.x;
    float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (R)
        for (int k = 0; k < 9; ++k) r[k] = R[(size_t)b * 9 + k];
    float acc[14];                                        // g_R (9) | g_t (3) | g_c (2)
    for (int k = 0; k < 14; ++k) acc[k] = 0.f;
    for (int p = threadIdx.x; p < P; p += LT) {
        const size_t i = (size_t)b * P + p;
        const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
        float X = r[0] * x + r[1] * y + r[2] * z, Y = r[3] * x + r[4] * y + r[5] * z, Z = r[6] * x + r[7] * y + r[8] * z;
        if (tr) { X += tr[b * 3]; Y += tr[b * 3 + 1]; Z += tr[b * 3 + 2]; }
        const float gx = gout[i * 2], gy = gout[i * 2 + 1];
        const float gX = fx * gx / Z, gY = fy * gy / Z, gZ = -(fx * gx * X + fy * gy * Y) / (Z * Z);
        if (gpts) {
            gpts[i * 3] = r[0] * gX + r[3] * gY + r[6] * gZ;
            gpts[i * 3 + 1] = r[1] * gX + r[4] * gY + r[7] * gZ;
            gpts[i * 3 + 2] = r[2] * gX + r[5] * gY + r[8] * gZ;
        }
        const float gv[3] = {gX, gY, gZ}, pv[3] = {x, y, z};
        for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c) acc[a * 3 + c] += gv[a] * pv[c];
            acc[9 + a] += gv[a];
        }
        acc[12] += gx;
        acc[13] += gy;
    }
    block_reduce<14>(s, acc);
    const int t = threadIdx.x;
    if (t < 9 && gR) gR[(size_t)b * 9 + t] = s[t * LT];
    if (t >= 9 && t < 12 && gt) gt[(size_t)b * 3 + t - 9] = s[t * LT];
    if (t >= 12 && t < 14 && gc) gc[(size_t)b * 2 + t - 12] = s[t * LT];
}

// out = M[:, :3] p + M[:, 3]
__global__ void __launch_bounds__(LT) transform_bwd_kernel(const float* __restrict__ rt, const float* __restrict__ pts, int P,
                                                           const float* __restrict__ gout, float* __restrict__ grt,
                                                           float* __restrict__ gpts) {
    __shared__ float s[12 * LT];
    const int b = blockIdx.x;
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = rt[(size_t)b * 12 + k];
    float acc[12];
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    for (int p = threadIdx.x; p < P; p += LT) {
        const size_t i = (size_t)b * P + p;
        const float pv[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
        const float g[3] = {gout[i * 3], gout[i * 3 + 1], gout[i * 3 + 2]};
        if (gpts)
            for (int c = 0; c < 3; ++c) gpts[i * 3 + c] = m[c] * g[0] + m[4 + c] * g[1] + m[8 + c] * g[2];
        for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c) acc[a * 4 + c] += g[a] * pv[c];
            acc[a * 4 + 3] += g[a];
        }
    }
    if (!grt) return;                                     // uniform over the workgroup
    block_reduce<12>(s, acc);
    if (threadIdx.x < 12) grt[(size_t)b * 12 + threadIdx.x] = s[threadIdx.x * LT];
}

}  // namespace

int apg_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int apg_check_ptrs(const std::string& f, const ApgPtr* ps, int count) {
    for (int k = 0; k < count; ++k) {
        if (!ps[k].p) return apg_fail(APG_EINVAL, f + ps[k].name + " is NULL");
        if ((uintptr_t)ps[k].p & (uintptr_t)(ps[k].align - 1))
            return apg_fail(APG_EINVAL, f + ps[k].name + " is not " + std::to_string(ps[k].align) + "-byte aligned");
    }
    return APG_OK;
}

#define APG_CHECK_LAUNCH(what)                                                                      \
    do {                                                                                            \
        hipError_t _e = hipGetLastError();                                                          \
        if (_e != hipSuccess) return apg_fail((int)_e, std::string(what) + ": " + hipGetErrorString(_e)); \
    } while (0)

extern "C" {

const char* apg_version(void) { return "airpose_grad 0.2 (gfx950; abi 2)"; }
int apg_abi_version(void) { return APG_ABI_VERSION; }
const char* apg_last_error(void) { return g_err.c_str(); }

int apg_rot6d_to_rotmat_bwd(const float* x6, int n, const float* g_rotmat, float* g_x6, void* stream) {
    if (!x6 || !g_rotmat || !g_x6 || n <= 0) return apg_fail(APG_EINVAL, "apg_rot6d_to_rotmat_bwd: bad argument");
    hipLaunchKernelGGL(rot6d_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x6, n, g_rotmat, g_x6);
    APG_CHECK_LAUNCH("rot6d_bwd_kernel");
    return APG_OK;
}

int apg_perspective_projection_bwd(const float* pts, int B, int P, const float* rotation, const float* translation, float fx,
                                   float fy, const float* g_out, float* g_pts, float* g_rotation, float* g_translation,
                                   float* g_center, void* stream) {
    if (!pts || !g_out || B <= 0 || P <= 0) return apg_fail(APG_EINVAL, "apg_perspective_projection_bwd: bad argument");
    hipLaunchKernelGGL(projection_bwd_kernel, dim3(B), dim3(LT), 0, (hipStream_t)stream, pts, P, rotation, translation, fx, fy,
                       g_out, g_pts, g_rotation, g_translation, g_center);
    APG_CHECK_LAUNCH("projection_bwd_kernel");
    return APG_OK;
}

int apg_transform_points_bwd(const float* rt, const float* pts, int B, int P, const float* g_out, float* g_rt, float* g_pts,
                             void* stream) {
    if (!rt || !pts || !g_out || B <= 0 || P <= 0) return apg_fail(APG_EINVAL, "apg_transform_points_bwd: bad argument");
    hipLaunchKernelGGL(transform_bwd_kernel, dim3(B), dim3(LT), 0, (hipStream_t)stream, rt, pts, P, g_out, g_rt, g_pts);
    APG_CHECK_LAUNCH("transform_bwd_kernel");
    return APG_OK;
}

}  // extern "C"
