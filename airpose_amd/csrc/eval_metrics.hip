// Evaluation metrics for gfx950 (libairpose_grad.so): what the reference trainers' test_epoch_end computes from the test_step output
// dicts (copenet_twoview.py:539-601, copenet_singleview.py:394-432, muhmr.py:463-517, hmr.py:365-386) -- MPJPE over the 22 body
// joints, the translation error (MPE) and hmr's angle-axis error -- without the four SMPLX.forward calls per batch it spends on them.
// With betas = 0 the 22 posed joints depend on the 22 rotations and the rest joints J_regressor v_template alone: no vertex is needed.
//
//   eval_main_kernel      grid = ceil(B / SPW), 64 threads (one wave), SPW = 32 / views samples per workgroup
//     A lane owns ONE kinematic chain: lane = 2 * item + kind, item = sample_in_workgroup * views + view, kind 0 = ground truth,
//     1 = prediction.  The 22 joints are walked in index order (fully unrolled); the world transform of joint j (G: 9 floats, p: 3) is
//     kept in LDS as sm[j][component][lane] -- a parent is a run-time index, which a register array could only serve from scratch,
//     and this layout puts the 64 lanes of one read in 64 consecutive words (no bank conflict).  Joint 21 is never a parent
//     (parents[j] < j), so 21 x 12 x 64 floats = 64512 bytes are held.  A lane reads back only what it wrote itself: no barrier in
//     the walk.  The prediction's lane gets the ground truth's position by __shfl_xor(.., 1) and forms the distance.
//     Then the workgroup's 25 sums per view (all joints, each joint, translation, angle) are taken over its samples in index order,
//     in fp64, by one thread each, out of the per-sample values parked in the same LDS, and written to the workspace.
//   metric_combine_kernel (metric_common.inc) one workgroup: each sum's partials added in workgroup order, in fp64, ONE add into the accumulator.
//
// Per chain, with `#pragma clang fp contract(off)` so that every fused product below is an fmaf call and nothing else is fused:
//   angle-axis r = (x, y, z) -> R (torchgeometry 0.1.2, angle_axis_to_rotation_matrix):
//     t2 = fmaf(z, z, fmaf(y, y, x * x))
//     t2 > 1e-6f:  th = sqrtf(t2); d = th + 1e-6f; w = r / d (three divisions); c = cosf(th); s = sinf(th); omc = 1 - c
//                  a_i = w_i * omc; s_i = w_i * s
//                  R00 = fmaf(wx, ax, c)   R01 = fmaf(wx, ay, -sz)  R02 = fmaf(wx, az, sy)
//                  R10 = fmaf(wx, ay, sz)  R11 = fmaf(wy, ay, c)    R12 = fmaf(wy, az, -sx)
//                  R20 = fmaf(wx, az, -sy) R21 = fmaf(wy, az, sx)   R22 = fmaf(wz, az, c)
//     otherwise:   R = I + skew(r), exact
//   chain (lbs.batch_rigid_transform on joints 0 .. 21): G_0 = R_0, p_0 = J_0; for j >= 1 with P = parents[j]:
//     G_j[i][k] = fmaf(G_P[i][2], R_j[2][k], fmaf(G_P[i][1], R_j[1][k], G_P[i][0] * R_j[0][k]))
//     b = J_j - J_P (one rounding per component)
//     p_j[i] = p_P[i] + fmaf(G_P[i][2], b[2], fmaf(G_P[i][1], b[1], G_P[i][0] * b[0]))
//   every error is norm3(d) = sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0))) of a component-wise difference d (one rounding each):
//     joint_err_j = norm3(p_j of the prediction - p_j of the ground truth), trans_err = norm3(t_pred - t_gt),
//     angle_err_j = norm3(a_pred_j - a_gt_j)
// Both chains of an item run the same instructions, so a prediction given as the ground truth's bits has joint_err = 0 exactly.
//
// Determinism.  No atomics and no arrival counter; the partition is a function of (B, views) alone.  Plain vector stores only.
#include "grad_internal.h"

#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int ET = 64;                   // threads per workgroup: one wave
constexpr int NJ = 22;                   // body joints
constexpr int ITEMS = ET / 2;            // (sample, view) pairs per workgroup: two chains each
constexpr int NSUM = 25;                 // sums per view and workgroup: all joints, each joint (22), translation, angle
constexpr int ACC = APG_EVAL_ACC_PER_VIEW;

struct EvalArgs {
    int B, views, matrix;
    int parents[NJ];
    const float* j_rest;
    const float* gt_body;
    // per view (entry 1 unused with one view)
    const float *gt_orient[2], *pred_rot[2], *gt_trans[2], *pred_trans[2], *gt_angles[2];
    float *joint_err, *trans_err, *angle_err;          // optional per-sample outputs
    double* part;                                      // [workgroup][view][NSUM]
};

#include "metric_common.inc"

static_assert(2 * (NSUM + 1) <= COMBINE_NT && NSUM + 1 <= ACC, "metric_combine_kernel: a thread per (view, sum) and one per view");

#include "rot_aa.inc"                    // aa_to_rotmat

__global__ void __launch_bounds__(ET) eval_main_kernel(const EvalArgs a) {
    __shared__ float sm[(NJ - 1) * 12 * ET];             // the walk: sm[(j * 12 + c) * ET + lane]; afterwards the per-sample errors
    const int lane = threadIdx.x;
    const int kind = lane & 1;                           // 0 = ground truth, 1 = prediction
    const int item = lane >> 1;
    const int v = a.views == 2 ? (item & 1) : 0;
    const int sl = a.views == 2 ? (item >> 1) : item;    // sample within the workgroup
    const int spw = ITEMS / a.views;
    const long long s_raw = (long long)blockIdx.x * spw + sl;
    const bool valid = s_raw < a.B;
    const size_t s = (size_t)(valid ? s_raw : a.B - 1);  // lanes past the batch walk the last sample again and contribute nothing
    const bool own = valid && kind == 1;                 // the lane that owns the item's errors

    const float* orient = v ? a.gt_orient[1] : a.gt_orient[0];
    const float* prot = v ? a.pred_rot[1] : a.pred_rot[0];
    const float* gtr = v ? a.gt_trans[1] : a.gt_trans[0];
    const float* ptr = v ? a.pred_trans[1] : a.pred_trans[0];
    const float* gang = v ? a.gt_angles[1] : a.gt_angles[0];

    float je[NJ], ae[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        float R[9];
        float ang[3] = {0.f, 0.f, 0.f};
        if (kind == 0 || a.matrix) {
            const float* src = kind == 0 ? (j == 0 ? orient + s * 9 : a.gt_body + (s * 21 + (j - 1)) * 9) : prot + (s * NJ + j) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = src[k];
        } else {
            const float* src = prot + (s * NJ + j) * 3;
            ang[0] = src[0], ang[1] = src[1], ang[2] = src[2];
            aa_to_rotmat(ang[0], ang[1], ang[2], R);
        }
        float G[9], p[3];
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) G[k] = R[k];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = a.j_rest[i];
        } else {
            const int P = a.parents[j];                  // uniform: 0 <= P < j, checked on the host
            float Gp[9], pp[3], b[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) Gp[k] = sm[(P * 12 + k) * ET + lane];
#pragma unroll
            for (int i = 0; i < 3; ++i) pp[i] = sm[(P * 12 + 9 + i) * ET + lane];
#pragma unroll
            for (int i = 0; i < 3; ++i) b[i] = a.j_rest[j * 3 + i] - a.j_rest[P * 3 + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    G[i * 3 + k] = fmaf(Gp[i * 3 + 2], R[6 + k], fmaf(Gp[i * 3 + 1], R[3 + k], Gp[i * 3] * R[k]));
                p[i] = pp[i] + fmaf(Gp[i * 3 + 2], b[2], fmaf(Gp[i * 3 + 1], b[1], Gp[i * 3] * b[0]));
            }
        }
        if (j < NJ - 1) {
#pragma unroll
            for (int k = 0; k < 9; ++k) sm[(j * 12 + k) * ET + lane] = G[k];
#pragma unroll
            for (int i = 0; i < 3; ++i) sm[(j * 12 + 9 + i) * ET + lane] = p[i];
        }
        // the partner chain's position: lane ^ 1
        const float q0 = __shfl_xor(p[0], 1), q1 = __shfl_xor(p[1], 1), q2 = __shfl_xor(p[2], 1);
        je[j] = norm3(p[0] - q0, p[1] - q1, p[2] - q2);  // meaningful in the prediction's lane (pred - gt); the other lane's is unused
        ae[j] = 0.f;
        if (gang != nullptr && kind == 1) {              // (angle-axis mode only: checked on the host)
            const float* g = gang + (s * NJ + j) * 3;
            ae[j] = norm3(ang[0] - g[0], ang[1] - g[1], ang[2] - g[2]);
        }
    }
    float te = 0.f;
    if (ptr != nullptr && kind == 1) te = norm3(ptr[s * 3] - gtr[s * 3], ptr[s * 3 + 1] - gtr[s * 3 + 1], ptr[s * 3 + 2] - gtr[s * 3 + 2]);

    if (own) {
        const size_t row = (size_t)v * a.B + s;
        if (a.joint_err) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) a.joint_err[row * NJ + j] = je[j];
        }
        if (a.angle_err) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) a.angle_err[row * NJ + j] = ae[j];
        }
        if (a.trans_err) a.trans_err[row] = te;
    }

    // the workgroup's sums: park the per-sample values (zeros for the lanes past the batch), then one thread per sum
    __syncthreads();
    float* rj = sm;                                      // [ITEMS][NJ]
    float* ra = sm + ITEMS * NJ;                         // [ITEMS][NJ]
    float* rt = sm + 2 * ITEMS * NJ;                     // [ITEMS]
    if (kind == 1) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            rj[item * NJ + j] = valid ? je[j] : 0.f;
            ra[item * NJ + j] = valid ? ae[j] : 0.f;
        }
        rt[item] = valid ? te : 0.f;
    }
    __syncthreads();
    if (lane < a.views * NSUM) {
        const int sv = lane / NSUM, q = lane - sv * NSUM;
        double acc = 0.0;
        for (int i = 0; i < spw; ++i) {                  // samples in index order
            const int it = i * a.views + sv;
            if (q == 0) {
                for (int j = 0; j < NJ; ++j) acc += (double)rj[it * NJ + j];
            } else if (q <= NJ) {
                acc += (double)rj[it * NJ + (q - 1)];
            } else if (q == NJ + 1) {
                acc += (double)rt[it];
            } else {
                for (int j = 0; j < NJ; ++j) acc += (double)ra[it * NJ + j];
            }
        }
        a.part[((size_t)blockIdx.x * a.views + sv) * NSUM + q] = acc;
    }
}

// accumulator of one view: [0] samples, [1] sum of joint_err, [2 .. 23] per joint, [24] sum of trans_err, [25] sum of angle_err,
// [26] samples with a translation, [27] samples with gt angles: metric_combine_kernel over the workgroups' partials, no sum skipped

inline int64_t eval_nwg(int B, int views) {
    const int spw = ITEMS / views;
    return ((int64_t)B + spw - 1) / spw;
}

}  // namespace

extern "C" {

int64_t apg_eval_acc_doubles(void) { return 2 * ACC; }

int64_t apg_eval_workspace_bytes(int B, int views) {
    if (B < 0 || (views != 1 && views != 2)) return -1;
    const int64_t nwg = eval_nwg(B, views);
    return (nwg > 0 ? nwg : 1) * views * NSUM * (int64_t)sizeof(double);
}

int apg_eval_update(int B, int views, int flags, const float* j_rest, const int* parents, const void* const* per_view,
                    const float* gt_body, float* joint_err, float* trans_err, float* angle_err, double* acc, void* workspace,
                    int64_t workspace_bytes, void* stream) {
    const std::string f = "apg_eval_update: ";
    static const char* const name[APG_EVAL_PER_VIEW] = {"gt_orient", "pred_rot", "gt_trans", "pred_trans", "gt_angles"};
    const MetricChecks m = {f, views, per_view, APG_EVAL_PER_VIEW, 2, name, acc, workspace, workspace_bytes,
                            apg_eval_workspace_bytes(B, views), "apg_eval_workspace_bytes"};
    if (B < 0) return apg_fail(APG_EINVAL, f + "B must be >= 0");
    if (int rc = m.views_ok()) return rc;
    if (flags != APG_EVAL_ANGLE_AXIS && flags != APG_EVAL_ROTMAT) return apg_fail(APG_EINVAL, f + "flags must be APG_EVAL_ANGLE_AXIS or APG_EVAL_ROTMAT");
    if (!j_rest) return apg_fail(APG_EINVAL, f + "j_rest is NULL");
    if (!parents) return apg_fail(APG_EINVAL, f + "parents is NULL");
    if (int rc = m.table_ok()) return rc;
    if (!gt_body) return apg_fail(APG_EINVAL, f + "gt_body is NULL");
    if (int rc = m.sinks_ok()) return rc;
    if (parents[0] != -1) return apg_fail(APG_EINVAL, f + "parents[0] must be -1");
    for (int j = 1; j < NJ; ++j)
        if (parents[j] < 0 || parents[j] >= j)
            return apg_fail(APG_EINVAL, f + "parents[" + std::to_string(j) + "] must be in 0 .. " + std::to_string(j - 1));
    EvalArgs a = {};
    CombineArgs c = {};
    for (int v = 0; v < views; ++v) {
        const void* const* q = per_view + v * APG_EVAL_PER_VIEW;
        const std::string at = " of view " + std::to_string(v);
        if (int rc = m.view_ok(v)) return rc;
        if (q[3] && !q[2]) return apg_fail(APG_EINVAL, f + "pred_trans" + at + " is given without gt_trans");
        if (q[2] && !q[3]) return apg_fail(APG_EINVAL, f + "gt_trans" + at + " is given without pred_trans");
        if (q[4] && flags != APG_EVAL_ANGLE_AXIS)
            return apg_fail(APG_EINVAL, f + "gt_angles" + at + " needs APG_EVAL_ANGLE_AXIS: the angle error compares angle-axis vectors");
        if (trans_err && !q[3]) return apg_fail(APG_EINVAL, f + "trans_err is asked for but pred_trans" + at + " is NULL");
        if (angle_err && !q[4]) return apg_fail(APG_EINVAL, f + "angle_err is asked for but gt_angles" + at + " is NULL");
        a.gt_orient[v] = (const float*)q[0], a.pred_rot[v] = (const float*)q[1], a.gt_trans[v] = (const float*)q[2];
        a.pred_trans[v] = (const float*)q[3], a.gt_angles[v] = (const float*)q[4];
        c.count_on[v][0] = 1, c.count_on[v][1] = q[3] != nullptr, c.count_on[v][2] = q[4] != nullptr;
    }
    const void* p4[5] = {j_rest, gt_body, joint_err, trans_err, angle_err};
    static const char* const n4[5] = {"j_rest", "gt_body", "joint_err", "trans_err", "angle_err"};
    for (int k = 0; k < 5; ++k)
        if ((uintptr_t)p4[k] & 3) return apg_fail(APG_EINVAL, f + n4[k] + " is not 4-byte aligned");
    if (int rc = m.sizes_ok()) return rc;
    if (B == 0) return APG_OK;                            // nothing to add: no launch, the accumulator stays as it is

    const int64_t nwg = eval_nwg(B, views);
    a.B = B, a.views = views, a.matrix = flags == APG_EVAL_ROTMAT;
    for (int j = 0; j < NJ; ++j) a.parents[j] = parents[j];
    a.j_rest = j_rest, a.gt_body = gt_body;
    a.joint_err = joint_err, a.trans_err = trans_err, a.angle_err = angle_err;
    a.part = (double*)workspace;
    c.n = (int)nwg, c.views = views, c.B = B, c.nsum = NSUM, c.pitch = ACC, c.part = (const double*)workspace, c.acc = acc;
    c.stride = views * NSUM, c.view_stride = NSUM;       // part[workgroup][view][NSUM]
    c.count_slot[0] = 0, c.count_slot[1] = 26, c.count_slot[2] = 27;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_main_kernel, dim3((unsigned)nwg), dim3(ET), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(metric_combine_kernel, dim3(1), dim3(COMBINE_NT), 0, st, c);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
