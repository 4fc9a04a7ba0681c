// Mesh metrics for gfx950 (libairpose_grad.so): the error between two point sets P (prediction) and Q (ground truth), (B, N, 3) fp32
// each, as it stands (abs), after moving a root point of each set onto the other (root), and after the least-squares similarity
// (s, R, t) of P onto Q (pa: Procrustes / Umeyama with det R = +1).  MPJPE, PVE and their aligned forms are these three numbers on the
// joints and on the vertices.  The semantics are in include/airpose_grad.h.
//
//   align_main_kernel<NT>   grid = B * views, one workgroup per (view, sample); NT = 64 threads (one wave) for N <= 64, else 1024
//     phase 1, moments.  With the pivots cp = p_0, cq = q_0 and a = p_i - cp, b = q_i - cq formed in fp64 (the difference of two
//       floats is exact there unless their exponents lie more than 29 apart): sp = sum a, sq = sum b, spp = sum a . a and the nine
//       K[r][c] = sum b_r a_c, 16 fp64 sums.  A thread takes the points tid, tid + NT, ... in that order; its 16 sums are added across
//       the wave by __shfl_down (32, 16, .. 1), the waves' sums in wave order by one thread per sum through LDS.
//     phase 2, solve (thread 0, fp64).  var = spp - sp . sp / N, Kc = K - sq sp^T / N (the centred moments), Horn's symmetric 4 x 4
//       matrix of Kc, SWEEPS cyclic Jacobi sweeps over its six pairs (each rotation: theta = (a_qq - a_pp) / (2 a_pq),
//       t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0;
//       a_pq == 0 selects the identity), the largest diagonal entry lambda and its eigenvector (w, x, y, z), R = the quaternion's matrix divided by |q|^2.  lambda is
//       tr(S D) of the header's formula and a quaternion's matrix has det +1, so the reflection fix is built in and no branch
//       looks at the data.  scale = lambda / var; var <= 0 (all p equal, N = 1) selects scale = 0, R = I.
//       mu_p = cp + sp / N, mu_q = cq + sq / N, t = mu_q - scale R mu_p.  Broadcast through LDS.
//     phase 3, residuals.  The points are read again (they sit in L2: a sample is 2 * 12 N bytes); keeping them in registers over the
//       solve (-DALIGN_KEEP=1) spills at 1024 threads and was measured slower.  Per point, in fp64 and
//       rounded to float once per component: d_abs = p - q, d_root = (p - r_p) - (q - r_q), d_pa = scale (R (p - mu_p)) + (mu_q - q);
//       each norm is sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0))) in fp32, added in fp64 in the order of phase 1.  The sample's three
//       means (sum / N in fp64) go to the workspace, rounded to float to `err`.
//   metric_combine_kernel   (metric_common.inc) one workgroup: the samples' means added in sample order, in fp64, ONE add into the accumulator.
//
// A point is 12 bytes and a sample's base only 4-byte aligned, so a lane loads its point as three dwords (a wave covers 768
// contiguous bytes).  pred == gt bit for bit gives d_abs = 0 and (with equal roots) d_root = 0 exactly.
//
// Determinism.  No atomics and no arrival counter; the partition is a function of N alone.  Plain vector stores only.
#include "grad_internal.h"

#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int NT_SMALL = 64;             // one wave: N <= NT_SMALL (the joints)
#ifndef ALIGN_NT
#define ALIGN_NT 1024
#endif
constexpr int NT_BIG = ALIGN_NT;         // 16 waves (the vertices)
constexpr int NMOM = 16;                 // sp (3), sq (3), spp, K (9)
constexpr int SWEEPS = 6;                // cyclic Jacobi sweeps of the 4 x 4 problem: it converges quadratically, and the host emulation of this
                                         // sequence (tests/align_util.py) holds every fp32 output bar with four
constexpr int ACC = APG_ALIGN_ACC_PER_VIEW;
#ifndef ALIGN_KEEP
#define ALIGN_KEEP 0                     // 1: a 1024-thread workgroup keeps up to KEEP_PTS points per thread in registers over the solve
#endif
constexpr int KEEP_PTS = 11;             // 11 * 1024 >= 10475, SMPL-X's vertex count
constexpr int NBC = 20;                  // broadcast: scale, R (9), mu_p (3), mu_q (3); [16] var, parked over the solve

struct AlignArgs {
    int B, views, N;
    long long sp, sq, srp, srq;                         // sample strides in floats: pred, gt, pred_root, gt_root
    const float *pred[2], *gt[2], *pred_root[2], *gt_root[2];
    float* err;                                          // (views, B, 3) or NULL
    float* transform;                                    // (views, B, 13) or NULL
    double* part;                                        // [view][sample][3]
};

#include "metric_common.inc"

static_assert(2 * (3 + 1) <= COMBINE_NT && 3 + 1 <= ACC, "metric_combine_kernel: a thread per (view, sum) and one per view");

// entry (i, j) of a symmetric 4 x 4 matrix kept as its upper triangle, row by row
__host__ __device__ constexpr int tri(int i, int j) { return i <= j ? 4 * i - i * (i - 1) / 2 + (j - i) : 4 * j - j * (j - 1) / 2 + (i - j); }

// Horn's closed form on the centred moments Kc[r][c] = sum (q - mu_q)_r (p - mu_p)_c: lambda = the largest eigenvalue of his 4 x 4
// matrix = tr(S D), R = the rotation of its eigenvector
__device__ void horn_solve(const double* Kc, double& lambda, double* R) {
    // S_ab = sum p_a q_b = Kc[b][a]
    const double Sxx = Kc[0], Sxy = Kc[3], Sxz = Kc[6], Syx = Kc[1], Syy = Kc[4], Syz = Kc[7], Szx = Kc[2], Szy = Kc[5], Szz = Kc[8];
    // the symmetric matrix as its upper triangle (a full copy would not fit the 128 registers of a 1024-thread workgroup)
    double S[10] = {(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz,
                    (Syy - Sxx) - Szz, Syz + Szy, (Szz - Sxx) - Syy};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = S[tri(p, q)];
                const bool zero = apq == 0.0;
                const double th = (S[tri(q, q)] - S[tri(p, p)]) / (2.0 * (zero ? 1.0 : apq));
                const double t0 = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));   // th = +-inf: t0 = 0
                const double t = zero ? 0.0 : t0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                S[tri(p, p)] -= t * apq, S[tri(q, q)] += t * apq, S[tri(p, q)] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k != p && k != q) {
                        const double x = S[tri(k, p)], y = S[tri(k, q)];
                        S[tri(k, p)] = c * x - s * y, S[tri(k, q)] = s * x + c * y;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double x = V[k][p], y = V[k][q];
                    V[k][p] = c * x - s * y, V[k][q] = s * x + c * y;
                }
            }
        }
    }
    double lam = S[tri(0, 0)], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = S[tri(k, k)] > lam;
        lam = up ? S[tri(k, k)] : lam;
        w = up ? V[0][k] : w, x = up ? V[1][k] : x, y = up ? V[2][k] : y, z = up ? V[3][k] : z;
    }
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double inv = 1.0 / ((ww + xx) + (yy + zz));
    R[0] = (((ww + xx) - yy) - zz) * inv, R[1] = 2.0 * (x * y - w * z) * inv, R[2] = 2.0 * (x * z + w * y) * inv;
    R[3] = 2.0 * (x * y + w * z) * inv, R[4] = (((ww - xx) + yy) - zz) * inv, R[5] = 2.0 * (y * z - w * x) * inv;
    R[6] = 2.0 * (x * z - w * y) * inv, R[7] = 2.0 * (y * z + w * x) * inv, R[8] = (((ww - xx) - yy) + zz) * inv;
    lambda = lam;
}

// one point's share of the 16 moments about the pivots
__device__ __forceinline__ void add_moments(double* m, const float* p, const float* q, double cp0, double cp1, double cp2, double cq0,
                                            double cq1, double cq2) {
    const double a0 = (double)p[0] - cp0, a1 = (double)p[1] - cp1, a2 = (double)p[2] - cp2;
    const double b0 = (double)q[0] - cq0, b1 = (double)q[1] - cq1, b2 = (double)q[2] - cq2;
    m[0] += a0, m[1] += a1, m[2] += a2;
    m[3] += b0, m[4] += b1, m[5] += b2;
    m[6] += (a0 * a0 + a1 * a1) + a2 * a2;
    m[7] += b0 * a0, m[8] += b0 * a1, m[9] += b0 * a2;
    m[10] += b1 * a0, m[11] += b1 * a1, m[12] += b1 * a2;
    m[13] += b2 * a0, m[14] += b2 * a1, m[15] += b2 * a2;
}

// one point's three residual norms
__device__ __forceinline__ void add_errors(double* e, const float* pf, const float* qf, bool has_root, const double* rp, const double* rq,
                                           double scale, const double* R, const double* mup, const double* muq) {
    const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    e[0] += (double)norm3((float)(p[0] - q[0]), (float)(p[1] - q[1]), (float)(p[2] - q[2]));
    if (has_root)
        e[1] += (double)norm3((float)((p[0] - rp[0]) - (q[0] - rq[0])), (float)((p[1] - rp[1]) - (q[1] - rq[1])),
                              (float)((p[2] - rp[2]) - (q[2] - rq[2])));
    const double c[3] = {p[0] - mup[0], p[1] - mup[1], p[2] - mup[2]};
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        d[r] = (float)(scale * ((R[r * 3] * c[0] + R[r * 3 + 1] * c[1]) + R[r * 3 + 2] * c[2]) + (muq[r] - q[r]));
    e[2] += (double)norm3(d[0], d[1], d[2]);
}

template <int NT, int KP>
__global__ void __launch_bounds__(NT) align_main_kernel(const AlignArgs a) {
    __shared__ double red[(NT / 64) * NMOM];
    __shared__ double tot[NMOM];
    __shared__ double bc[NBC];
    const int tid = threadIdx.x;
    const int v = (int)(blockIdx.x / (unsigned)a.B);     // blockIdx.x = v * B + b < views * B
    const int b = (int)(blockIdx.x - (unsigned)v * (unsigned)a.B);
    const float* P = (v ? a.pred[1] : a.pred[0]) + (size_t)b * (size_t)a.sp;
    const float* Q = (v ? a.gt[1] : a.gt[0]) + (size_t)b * (size_t)a.sq;
    const float* rootp = v ? a.pred_root[1] : a.pred_root[0];
    const float* rootq = v ? a.gt_root[1] : a.gt_root[0];
    const int N = a.N;

    // ---- phase 1
    const double cp0 = (double)P[0], cp1 = (double)P[1], cp2 = (double)P[2];
    const double cq0 = (double)Q[0], cq1 = (double)Q[1], cq2 = (double)Q[2];
    double m[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) m[k] = 0.0;
    float kept[KP > 0 ? KP : 1][6];                     // KP > 0: the thread's points stay in registers for phase 3
    const bool keep = KP > 0 && N <= KP * NT;            // (uniform)
    if (keep) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int i = tid + k * NT;
            if (i < N) {
#pragma unroll
                for (int c = 0; c < 3; ++c) kept[k][c] = P[(size_t)i * 3 + c], kept[k][3 + c] = Q[(size_t)i * 3 + c];
                add_moments(m, kept[k], kept[k] + 3, cp0, cp1, cp2, cq0, cq1, cq2);
            }
        }
    } else {
        for (int i = tid; i < N; i += NT) add_moments(m, P + (size_t)i * 3, Q + (size_t)i * 3, cp0, cp1, cp2, cq0, cq1, cq2);
    }
    wg_sum<NT, NMOM>(m, red, tot);

    // ---- phase 2
    if (tid == 0) {
        const double n = (double)N;
        const double sp[3] = {tot[0], tot[1], tot[2]}, sq[3] = {tot[3], tot[4], tot[5]};
        const double var = tot[6] - ((sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]) / n;
        double Kc[9], R[9], lam;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Kc[r * 3 + c] = tot[7 + r * 3 + c] - sq[r] * sp[c] / n;
        // the means go to LDS before the solve and are read back after it: the solve needs the registers
#pragma unroll
        for (int k = 0; k < 3; ++k) bc[10 + k] = (k == 0 ? cp0 : k == 1 ? cp1 : cp2) + sp[k] / n;
#pragma unroll
        for (int k = 0; k < 3; ++k) bc[13 + k] = (k == 0 ? cq0 : k == 1 ? cq1 : cq2) + sq[k] / n;
        bc[16] = var;
        horn_solve(Kc, lam, R);
        const double var1 = bc[16];
        const bool degenerate = !(var1 > 0.0);           // all p equal (N = 1 included): scale = 0, R = I
        const double scale = degenerate ? 0.0 : lam / (degenerate ? 1.0 : var1);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = degenerate ? ((k & 3) == 0 ? 1.0 : 0.0) : R[k];
        const double mup[3] = {bc[10], bc[11], bc[12]}, muq[3] = {bc[13], bc[14], bc[15]};
        bc[0] = scale;
#pragma unroll
        for (int k = 0; k < 9; ++k) bc[1 + k] = R[k];
        if (a.transform) {
            float* T = a.transform + (size_t)blockIdx.x * 13;
            T[0] = (float)scale;
#pragma unroll
            for (int k = 0; k < 9; ++k) T[1 + k] = (float)R[k];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                T[10 + r] = (float)(muq[r] - scale * ((R[r * 3] * mup[0] + R[r * 3 + 1] * mup[1]) + R[r * 3 + 2] * mup[2]));
        }
    }
    __syncthreads();

    // ---- phase 3
    const double scale = bc[0];
    double R[9], mup[3], muq[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = bc[1 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) mup[k] = bc[10 + k], muq[k] = bc[13 + k];
    const bool has_root = rootp != nullptr;              // (a pair: checked on the host)
    double rp[3] = {0.0, 0.0, 0.0}, rq[3] = {0.0, 0.0, 0.0};
    if (has_root) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rp[k] = (double)rootp[(size_t)b * (size_t)a.srp + k];
            rq[k] = (double)rootq[(size_t)b * (size_t)a.srq + k];
        }
    }
    double e[3] = {0.0, 0.0, 0.0};
    if (keep) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (tid + k * NT < N) add_errors(e, kept[k], kept[k] + 3, has_root, rp, rq, scale, R, mup, muq);
    } else {
        for (int i = tid; i < N; i += NT) add_errors(e, P + (size_t)i * 3, Q + (size_t)i * 3, has_root, rp, rq, scale, R, mup, muq);
    }
    wg_sum<NT, 3>(e, red, tot);
    if (tid < 3) {
        const double mean = tot[tid] / (double)N;
        a.part[(size_t)blockIdx.x * 3 + tid] = mean;
        if (a.err) a.err[(size_t)blockIdx.x * 3 + tid] = (float)mean;
    }
}

// accumulator of one view: [0] samples, [1] sum of abs, [2] sum of root, [3] sum of pa, [4] samples that had roots:
// metric_combine_kernel over the samples' means; the root sum of a view without roots is left alone

constexpr int MAX_B = 1 << 22, MAX_N = 1 << 24;

}  // namespace

extern "C" {

int64_t apg_align_acc_doubles(void) { return 2 * ACC; }

int64_t apg_align_workspace_bytes(int B, int views, int N) {
    if (B < 1 || B > MAX_B || N < 1 || N > MAX_N || (views != 1 && views != 2)) return -1;
    return (int64_t)B * views * 3 * (int64_t)sizeof(double);
}

int apg_align_update(int B, int views, int N, int64_t pred_stride, int64_t gt_stride, int64_t pred_root_stride,
                     int64_t gt_root_stride, const void* const* per_view, float* err, float* transform, double* acc, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    const std::string f = "apg_align_update: ";
    static const char* const name[APG_ALIGN_PER_VIEW] = {"pred", "gt", "pred_root", "gt_root"};
    const MetricChecks m = {f, views, per_view, APG_ALIGN_PER_VIEW, 2, name, acc, workspace, workspace_bytes,
                            apg_align_workspace_bytes(B, views, N), "apg_align_workspace_bytes"};
    if (B < 1 || B > MAX_B) return apg_fail(APG_EINVAL, f + "B must be in 1 .. " + std::to_string(MAX_B));
    if (int rc = m.views_ok()) return rc;
    if (N < 1 || N > MAX_N) return apg_fail(APG_EINVAL, f + "N must be in 1 .. " + std::to_string(MAX_N));
    if (pred_stride < 3 * (int64_t)N) return apg_fail(APG_EINVAL, f + "pred_stride must be at least 3 N floats");
    if (gt_stride < 3 * (int64_t)N) return apg_fail(APG_EINVAL, f + "gt_stride must be at least 3 N floats");
    if (int rc = m.table_ok()) return rc;
    if (int rc = m.sinks_ok()) return rc;
    AlignArgs a = {};
    CombineArgs c = {};
    for (int v = 0; v < views; ++v) {
        const void* const* q = per_view + v * APG_ALIGN_PER_VIEW;
        const std::string at = " of view " + std::to_string(v);
        if (int rc = m.view_ok(v)) return rc;
        if (q[2] && !q[3]) return apg_fail(APG_EINVAL, f + "pred_root" + at + " is given without gt_root");
        if (q[3] && !q[2]) return apg_fail(APG_EINVAL, f + "gt_root" + at + " is given without pred_root");
        if (q[2] && pred_root_stride < 3) return apg_fail(APG_EINVAL, f + "pred_root_stride must be at least 3 floats");
        if (q[2] && gt_root_stride < 3) return apg_fail(APG_EINVAL, f + "gt_root_stride must be at least 3 floats");
        a.pred[v] = (const float*)q[0], a.gt[v] = (const float*)q[1];
        a.pred_root[v] = (const float*)q[2], a.gt_root[v] = (const float*)q[3];
        c.count_on[v][0] = 1, c.count_on[v][1] = q[2] != nullptr;
        c.skip[v] = q[2] ? 0u : 1u << 1;                 // sum 1 is the root sum
    }
    if ((uintptr_t)err & 3) return apg_fail(APG_EINVAL, f + "err is not 4-byte aligned");
    if ((uintptr_t)transform & 3) return apg_fail(APG_EINVAL, f + "transform is not 4-byte aligned");
    if (int rc = m.sizes_ok()) return rc;

    a.B = B, a.views = views, a.N = N;
    a.sp = pred_stride, a.sq = gt_stride, a.srp = pred_root_stride, a.srq = gt_root_stride;
    a.err = err, a.transform = transform, a.part = (double*)workspace;
    c.n = B, c.views = views, c.B = B, c.nsum = 3, c.pitch = ACC, c.part = (const double*)workspace, c.acc = acc;
    c.stride = 3, c.view_stride = 3 * (long long)B;      // part[view][sample][3]
    c.count_slot[0] = 0, c.count_slot[1] = 4;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)B * (unsigned)views);
    if (N <= NT_SMALL)
        hipLaunchKernelGGL((align_main_kernel<NT_SMALL, 0>), grid, dim3(NT_SMALL), 0, st, a);
    else
        hipLaunchKernelGGL((align_main_kernel<NT_BIG, ALIGN_KEEP ? KEEP_PTS : 0>), grid, dim3(NT_BIG), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(metric_combine_kernel, dim3(1), dim3(COMBINE_NT), 0, st, c);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
