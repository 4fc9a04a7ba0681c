// AirPose+ on a whole sequence (libairpose_grad.so): what stands between the network's per-frame outputs and the fitter
// (copenet_real_data/scripts/bundle_adj.py:176-200, copenet_real/dsets/copenet_real.py:105-106) and between the fitter's result and
// the rest of the package (bundle_adj.py:404-412, 510-516), per frame, fp32.  The semantics are in include/airpose_grad.h.
//
//   seq_init_kernel    grid = ceil(L / SR), 512 threads, SR = APG_SEQ_ROWS frames per workgroup
//     z = Wmu leaky(W1 x + b1) + bmu with x = view 0's 21 body joints: the folded VPoser encoder (loss_real.fold_encoder).  Eight
//       lanes share an output unit for the workgroup's SR frames (layer8: whole cache lines of the unit's weight row per group, the
//       activations from LDS, three xor shuffles), 64 units at a time.
//     phi = the first two rows of pytorch3d 0.3.0's axis_angle_to_matrix of the root joint, tau = the translation, bit for bit.
//     j2d = det with both detectors' confidences zeroed where their positions lie more than agreement_px apart; robust = the
//       filtered AlphaPose confidences of the frame added by ONE thread in the order view 0 joint 0 .. 23, view 1 joint 0 .. 23.
//   seq_export_kernel  the same grid and block
//     thetas = the VPoser decoder (32 -> 512 -> 512 -> 126 on fmaf, layer8 again, the weights in torch's own layout),
//       Gram-Schmidt on the 3 x 2 reshape and tgm 0.1.2's matrot2aa (rot_aa.inc: aa_fwd) -- the formulae of fitting.hip's
//       fit_decode_kernel, so the exported pose is the pose the fit optimised up to the order of the additions.
//     root_rot = rotation_6d_to_matrix(phi) (rows), smpl_wrt_cam = [R | tau; 0 0 0 1], cam1_wrt_cam0 = T0 [R1^T | -R1^T t1].
//
// Latency-bound like the regressor: no MFMA; the weights (1.3 MB for the decoder) stream from L2.  Every sum has a fixed order and
// there is no atomic: two runs give the same bits.  Plain vector stores only.
#include "grad_internal.h"

#include <cmath>
#include <string>

namespace {

constexpr int SR = APG_SEQ_ROWS;         // frames per workgroup
constexpr int NT = 512;                  // one thread per hidden unit
constexpr int NB = 21, NJ2 = 24, NZ = 32, NH = 512, NIN = 63, NOUT = 126;
constexpr int MAX_L = 1 << 22;

#include "rot_aa.inc"                    // V3 and its helpers; aa_fwd (the decoder's matrot2aa)

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : 0.01f * v; }

// Gram-Schmidt of both 6-D conventions (F.normalize's eps): b1 = a1 / |a1|, b2 = (a2 - (b1 . a2) b1) / |..|, b3 = b1 x b2
__device__ __forceinline__ void gram_schmidt(V3 a1, V3 a2, V3& b1, V3& b2, V3& b3) {
    b1 = (1.f / fmaxf(sqrtf(dot(a1, a1)), 1e-12f)) * a1;
    const V3 u = a2 - dot(b1, a2) * b1;
    b2 = (1.f / fmaxf(sqrtf(dot(u, u)), 1e-12f)) * u;
    b3 = cross(b1, b2);
}

// pytorch3d 0.3.0 axis_angle_to_matrix, row-major: axis_angle_to_quaternion (sin(t / 2) / t -> 1/2 - t^2 / 48 below 1e-6) and
// quaternion_to_matrix.  r = 0: q = (1, 0, 0, 0), two_s = 2, the identity exactly
__device__ __forceinline__ void aa_to_matrix_p3d(V3 a, float* R) {
    const float th = sqrtf(dot(a, a)), half = 0.5f * th;
    const float k = th < 1e-6f ? 0.5f - th * th / 48.f : sinf(half) / th;
    const float r = cosf(half), i = a.x * k, j = a.y * k, q = a.z * k;
    const float two_s = 2.0f / (r * r + i * i + j * j + q * q);
    R[0] = 1.f - two_s * (j * j + q * q); R[1] = two_s * (i * j - q * r);       R[2] = two_s * (i * q + j * r);
    R[3] = two_s * (i * j + q * r);       R[4] = 1.f - two_s * (i * i + q * q); R[5] = two_s * (j * q - i * r);
    R[6] = two_s * (i * q - j * r);       R[7] = two_s * (j * q + i * r);       R[8] = 1.f - two_s * (i * i + j * j);
}

// One layer for the workgroup's SR frames: v[r] = sum_k W[o][k] x[r * XLD + k] for every o < nout, W as torch stores it ([out][K]).
// EIGHT lanes share an output: lane s of the group takes the float4 at k = 4 s + 32 i, so a group reads whole 128-byte lines of its
// row and a wave eight rows at once (a thread per row would touch 64 lines per load).  A lane keeps four partial sums per frame (the
// float4's components) in index order, adds them as (p0 + p1) + (p2 + p3), and the eight lanes' sums meet by xor shuffles over 1, 2,
// 4: every lane ends with the same bits.  store(o, v) runs on the group's lane 0.  The trip count is the same for every group of a
// wave (the shuffles need all eight lanes); a group past nout reads row 0 and stores nothing.  K a multiple of 4, W 16-byte aligned.
template <int K, int XLD, class Store>
__device__ __forceinline__ void layer8(const float* __restrict__ W, int nout, const float* x, Store store) {
    const int s = threadIdx.x & 7, g = threadIdx.x >> 3;
    constexpr int NG = NT / 8;
    for (int o = g; o < (nout + NG - 1) / NG * NG; o += NG) {
        const bool live = o < nout;
        const float* w = W + (size_t)(live ? o : 0) * K;
        float p[SR][4] = {};
        for (int k = 4 * s; k < K; k += 32) {
            const float4 wv = *reinterpret_cast<const float4*>(w + k);
#pragma unroll
            for (int r = 0; r < SR; ++r) {
                const float4 xv = *reinterpret_cast<const float4*>(x + r * XLD + k);
                p[r][0] = fmaf(wv.x, xv.x, p[r][0]); p[r][1] = fmaf(wv.y, xv.y, p[r][1]);
                p[r][2] = fmaf(wv.z, xv.z, p[r][2]); p[r][3] = fmaf(wv.w, xv.w, p[r][3]);
            }
        }
        float v[SR];
#pragma unroll
        for (int r = 0; r < SR; ++r) {
            v[r] = (p[r][0] + p[r][1]) + (p[r][2] + p[r][3]);
            v[r] += __shfl_xor(v[r], 1); v[r] += __shfl_xor(v[r], 2); v[r] += __shfl_xor(v[r], 4);
        }
        if (live && s == 0) store(o, v);
    }
}
// the same for rows that are only 4-byte aligned (the encoder's 63 inputs): lane s takes k = s + 8 i < K, one partial sum per frame
template <int K, int XLD, class Store>
__device__ __forceinline__ void layer8_scalar(const float* __restrict__ W, int nout, const float* x, Store store) {
    const int s = threadIdx.x & 7, g = threadIdx.x >> 3;
    constexpr int NG = NT / 8;
    for (int o = g; o < (nout + NG - 1) / NG * NG; o += NG) {
        const bool live = o < nout;
        const float* w = W + (size_t)(live ? o : 0) * K;
        float v[SR] = {};
        for (int k = s; k < K; k += 8) {
            const float wv = w[k];
#pragma unroll
            for (int r = 0; r < SR; ++r) v[r] = fmaf(wv, x[r * XLD + k], v[r]);
        }
#pragma unroll
        for (int r = 0; r < SR; ++r) { v[r] += __shfl_xor(v[r], 1); v[r] += __shfl_xor(v[r], 2); v[r] += __shfl_xor(v[r], 4); }
        if (live && s == 0) store(o, v);
    }
}

struct InitArgs {
    int L;
    const float *angles0, *angles1, *trans0, *trans1, *det, *W1, *b1, *Wmu, *bmu;
    float agreement_px, robust_conf;
    float *z, *phi, *tau, *j2d;
    int* robust;
};

__global__ void __launch_bounds__(NT) seq_init_kernel(const InitArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[SR * 64];       // a frame's 63 inputs (+ one 0)
    __shared__ __attribute__((aligned(16))) float hs[SR * NH];
    __shared__ float cs[SR * 2 * NJ2];                               // the filtered AlphaPose confidences
    const int t = threadIdx.x, L = a.L;
    const int l0 = blockIdx.x * SR;                                  // l0 < L: the grid is ceil(L / SR)
    if (t < SR * 64) {
        const int r = t >> 6, c = t & 63, l = l0 + r;
        xs[t] = (l < L && c < NIN) ? a.angles0[(size_t)l * 66 + 3 + c] : 0.f;
    } else if (t < SR * 64 + SR * 2) {                               // the root rotations: (frame, view)
        const int i = t - SR * 64, r = i >> 1, v = i & 1, l = l0 + r;
        if (l < L) {
            const float* src = (v ? a.angles1 : a.angles0) + (size_t)l * 66;
            float R[9];
            aa_to_matrix_p3d(v3(src[0], src[1], src[2]), R);
            float* dst = a.phi + ((size_t)v * L + l) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) dst[k] = R[k];
            const float* ts = (v ? a.trans1 : a.trans0) + (size_t)l * 3;
            float* td = a.tau + ((size_t)v * L + l) * 3;
            td[0] = ts[0]; td[1] = ts[1]; td[2] = ts[2];
        }
    }
    if (t < SR * 2 * NJ2) {                                          // the agreement filter: (frame, view, joint), both detectors
        const int r = t / (2 * NJ2), vj = t - r * (2 * NJ2), v = vj / NJ2, j = vj - v * NJ2, l = l0 + r;
        float kept = 0.f;
        if (l < L) {
            const size_t base = (((size_t)v * L + l) * 2) * NJ2 * 3 + (size_t)j * 3;      // detector 0; detector 1 is NJ2 * 3 further
            const float* p0 = a.det + base;
            const float* p1 = p0 + NJ2 * 3;
            const float x0 = p0[0], y0 = p0[1], c0 = p0[2], x1 = p1[0], y1 = p1[1], c1 = p1[2];
            const float dx = x0 - x1, dy = y0 - y1;
            const bool apart = sqrtf(dx * dx + dy * dy) > a.agreement_px;
            float* q0 = a.j2d + base;
            float* q1 = q0 + NJ2 * 3;
            q0[0] = x0; q0[1] = y0; q0[2] = apart ? 0.f : c0;
            q1[0] = x1; q1[1] = y1; q1[2] = apart ? 0.f : c1;
            kept = apart ? 0.f : c1;
        }
        cs[t] = kept;
    }
    __syncthreads();
    if (t < SR && l0 + t < L) {
        float s = 0.f;
        for (int k = 0; k < 2 * NJ2; ++k) s += cs[t * 2 * NJ2 + k];
        a.robust[l0 + t] = s > a.robust_conf ? 1 : 0;
    }
    layer8_scalar<NIN, 64>(a.W1, NH, xs, [&](int o, const float (&v)[SR]) {
        const float bias = a.b1[o];
#pragma unroll
        for (int r = 0; r < SR; ++r) hs[r * NH + o] = lrelu(v[r] + bias);
    });
    __syncthreads();
    layer8<NH, NH>(a.Wmu, NZ, hs, [&](int o, const float (&v)[SR]) {
        const float bias = a.bmu[o];
#pragma unroll
        for (int r = 0; r < SR; ++r)
            if (l0 + r < L) a.z[(size_t)(l0 + r) * NZ + o] = v[r] + bias;
    });
}

struct ExportArgs {
    int L;
    const float *z, *phi, *tau, *w1, *b1, *w2, *b2, *w3, *b3;
    float *thetas, *root_rot, *smpl_wrt_cam, *cam1_wrt_cam0;
};

__global__ void __launch_bounds__(NT) seq_export_kernel(const ExportArgs a) {
    __shared__ __attribute__((aligned(16))) float zs[SR * NZ];
    __shared__ __attribute__((aligned(16))) float h1[SR * NH];
    __shared__ __attribute__((aligned(16))) float h2[SR * NH];
    __shared__ float os[SR * 128];
    __shared__ float rt[SR * 2 * 12];                                // per (frame, view): R (9), tau (3)
    const int t = threadIdx.x, L = a.L;
    const int l0 = blockIdx.x * SR;
    if (t < SR * NZ) {
        const int r = t >> 5, l = l0 + r;
        zs[t] = l < L ? a.z[(size_t)l * NZ + (t & 31)] : 0.f;
    } else if (t < SR * NZ + SR * 2) {                               // the rigid poses: (frame, view)
        const int i = t - SR * NZ, r = i >> 1, v = i & 1, l = l0 + r;
        if (l < L) {
            const float* p = a.phi + ((size_t)v * L + l) * 6;
            const float* ts = a.tau + ((size_t)v * L + l) * 3;
            V3 b1, b2, b3;
            gram_schmidt(v3(p[0], p[1], p[2]), v3(p[3], p[4], p[5]), b1, b2, b3);
            const float R[9] = {b1.x, b1.y, b1.z, b2.x, b2.y, b2.z, b3.x, b3.y, b3.z};
            const float tv[3] = {ts[0], ts[1], ts[2]};
            float* rr = a.root_rot + ((size_t)v * L + l) * 9;
            float* T = a.smpl_wrt_cam + ((size_t)v * L + l) * 16;
#pragma unroll
            for (int k = 0; k < 9; ++k) rr[k] = R[k], rt[i * 12 + k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                T[k * 4 + 0] = R[k * 3]; T[k * 4 + 1] = R[k * 3 + 1]; T[k * 4 + 2] = R[k * 3 + 2]; T[k * 4 + 3] = tv[k];
                rt[i * 12 + 9 + k] = tv[k];
            }
            T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
        }
    }
    __syncthreads();
    layer8<NZ, NZ>(a.w1, NH, zs, [&](int o, const float (&v)[SR]) {
        const float bias = a.b1[o];
#pragma unroll
        for (int r = 0; r < SR; ++r) h1[r * NH + o] = lrelu(v[r] + bias);
    });
    __syncthreads();
    layer8<NH, NH>(a.w2, NH, h1, [&](int o, const float (&v)[SR]) {
        const float bias = a.b2[o];
#pragma unroll
        for (int r = 0; r < SR; ++r) h2[r * NH + o] = lrelu(v[r] + bias);
    });
    __syncthreads();
    layer8<NH, NH>(a.w3, NOUT, h2, [&](int o, const float (&v)[SR]) {
        const float bias = a.b3[o];
#pragma unroll
        for (int r = 0; r < SR; ++r) os[r * 128 + o] = v[r] + bias;
    });
    __syncthreads();
    if (t < SR * NB) {                                               // matrot2aa of the Gram-Schmidt rotations
        const int r = t / NB, j = t - r * NB, l = l0 + r;
        if (l < L) {
            const float* o = os + r * 128 + 6 * j;
            V3 b1, b2, b3;
            gram_schmidt(v3(o[0], o[2], o[4]), v3(o[1], o[3], o[5]), b1, b2, b3);
            const float R[9] = {b1.x, b2.x, b3.x, b1.y, b2.y, b3.y, b1.z, b2.z, b3.z};
            const AA aa = aa_fwd(R);
            float* dst = a.thetas + ((size_t)l * NB + j) * 3;
            dst[0] = aa.aa.x; dst[1] = aa.aa.y; dst[2] = aa.aa.z;
        }
    } else if (t >= 128 && t < 128 + SR) {                           // cam1_wrt_cam0 = T0 [R1^T | -R1^T t1]
        const int r = t - 128, l = l0 + r;
        if (l < L) {
            const float* R0 = rt + (r * 2) * 12;
            const float* R1 = rt + (r * 2 + 1) * 12;
            const float* t0 = R0 + 9;
            const float* t1 = R1 + 9;
            float ti[3];                                             // -R1^T t1
#pragma unroll
            for (int c = 0; c < 3; ++c) ti[c] = -(R1[c] * t1[0] + R1[3 + c] * t1[1] + R1[6 + c] * t1[2]);
            float* T = a.cam1_wrt_cam0 + (size_t)l * 16;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c)                          // (R0 R1^T)[i][c] = sum_k R0[i][k] R1[c][k]
                    T[i * 4 + c] = R0[i * 3] * R1[c * 3] + R0[i * 3 + 1] * R1[c * 3 + 1] + R0[i * 3 + 2] * R1[c * 3 + 2];
                T[i * 4 + 3] = (R0[i * 3] * ti[0] + R0[i * 3 + 1] * ti[1] + R0[i * 3 + 2] * ti[2]) + t0[i];
            }
            T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
        }
    }
}

static_assert(SR * 64 + SR * 2 <= NT && SR * 2 * NJ2 <= NT && NT % 64 == 0, "seq_init_kernel's thread roles");
static_assert(SR * NZ + SR * 2 <= NT && SR * NB <= 128 && 128 + SR <= NT && NOUT <= 128, "seq_export_kernel's thread roles");

}  // namespace

extern "C" {

int apg_seq_init(int L, const float* angles0, const float* angles1, const float* trans0, const float* trans1, const float* det,
                 const float* W1, const float* b1, const float* Wmu, const float* bmu, float agreement_px, float robust_conf, float* z,
                 float* phi, float* tau, float* j2d, int* robust, void* stream) {
    const std::string f = "apg_seq_init: ";
    if (L < 1 || L > MAX_L) return apg_fail(APG_EINVAL, f + "L must be in 1 .. " + std::to_string(MAX_L));
    const ApgPtr ps[] = {{angles0, "angles0", 4}, {angles1, "angles1", 4}, {trans0, "trans0", 4}, {trans1, "trans1", 4}, {det, "det", 4},
                      {W1, "W1", 4}, {b1, "b1", 4}, {Wmu, "Wmu", 16}, {bmu, "bmu", 4}, {z, "z", 4}, {phi, "phi", 4}, {tau, "tau", 4},
                      {j2d, "j2d", 4}, {robust, "robust", 4}};
    if (int rc = apg_check_ptrs(f, ps, (int)(sizeof(ps) / sizeof(ps[0])))) return rc;
    if (!std::isfinite(agreement_px) || agreement_px < 0.f)
        return apg_fail(APG_EINVAL, f + "agreement_px must be finite and not negative");
    if (!std::isfinite(robust_conf)) return apg_fail(APG_EINVAL, f + "robust_conf must be finite");
    if ((const void*)j2d == (const void*)det) return apg_fail(APG_EINVAL, f + "j2d must not be det");
    InitArgs a = {L, angles0, angles1, trans0, trans1, det, W1, b1, Wmu, bmu, agreement_px, robust_conf, z, phi, tau, j2d, robust};
    hipLaunchKernelGGL(seq_init_kernel, dim3((unsigned)((L + SR - 1) / SR)), dim3(NT), 0, (hipStream_t)stream, a);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_seq_export(int L, const float* z, const float* phi, const float* tau, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, float* thetas, float* root_rot, float* smpl_wrt_cam,
                   float* cam1_wrt_cam0, void* stream) {
    const std::string f = "apg_seq_export: ";
    if (L < 1 || L > MAX_L) return apg_fail(APG_EINVAL, f + "L must be in 1 .. " + std::to_string(MAX_L));
    const ApgPtr ps[] = {{z, "z", 4}, {phi, "phi", 4}, {tau, "tau", 4}, {w1, "w1", 16}, {b1, "b1", 4}, {w2, "w2", 16}, {b2, "b2", 4},
                      {w3, "w3", 16}, {b3, "b3", 4}, {thetas, "thetas", 4}, {root_rot, "root_rot", 4},
                      {smpl_wrt_cam, "smpl_wrt_cam", 4}, {cam1_wrt_cam0, "cam1_wrt_cam0", 4}};
    if (int rc = apg_check_ptrs(f, ps, (int)(sizeof(ps) / sizeof(ps[0])))) return rc;
    ExportArgs a = {L, z, phi, tau, w1, b1, w2, b2, w3, b3, thetas, root_rot, smpl_wrt_cam, cam1_wrt_cam0};
    hipLaunchKernelGGL(seq_export_kernel, dim3((unsigned)((L + SR - 1) / SR)), dim3(NT), 0, (hipStream_t)stream, a);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
