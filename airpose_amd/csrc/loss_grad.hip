// The training loss of the four reference trainers (get_loss) and its gradient seeds in one pass, for gfx950 (libairpose_grad.so).
//
// The loss is 60 * sum_k w_k * mean((a - b)^2) over a handful of terms, so the seed dL/da = 60 w_k limb_w 2 (a - b) / N_k (plus the
// cross-view share) is known the moment the difference is formed: the forward and the "backward" are the same sweep.
//
//   loss_main_kernel<ALIGNED>   grid = NSB + NVB workgroups of 256 threads
//     workgroups [0, NSB)         the small terms of LOSS_SB bodies each (trans, 2-D joints, 3-D joints, root rotation, pose, betas,
//                                 cam: a few hundred elements per body), their seeds, and the zero rows >= 22 of g_joints / g_j2d;
//                                 13 partial sums per workgroup
//     workgroups [NSB, NSB+NVB)   the vertex term as a flat stream of N = B V 3 floats, LOSS_EPB floats per workgroup: thread t of
//                                 workgroup w owns the float quads at w * LOSS_EPB + (i * 256 + t) * 4, i = 0 .. 3; 3 partial sums
//                                 per workgroup (view 0, view 1, cross)
//   loss_combine_kernel         one workgroup: every partial list summed in index order (thread-strided, then a fixed LDS tree),
//                               the eight terms, the weighted total, terms[9]
//
// Determinism.  No atomics and no arrival counter.  The partition is a function of (B, V, J) alone -- it does not depend on the
// pointers' alignment either: ALIGNED only selects how a thread's quad is moved (one 16-byte access when every vertex pointer is
// 16-byte aligned, four 4-byte accesses otherwise), never which elements a thread owns or the order it adds them in.  The last
// N mod 4 floats of the stream are a partial quad, taken element by element on both paths.
#include "grad_internal.h"

#include <string>

namespace {

#include "loss_common.inc"               // LT, NJ, block_reduce, limb_weight

constexpr int LOSS_EPB = 4096;           // vertex-stream floats per workgroup: 256 threads x 4 quads of 4
constexpr int LOSS_SB = 4;               // bodies per small-term workgroup

// partial sums of a small-term workgroup
enum { S_TRANS0, S_TRANS1, S_KP0, S_KP1, S_KP3D, S_ROOT0, S_ROOT1, S_POSE, S_BET0, S_BET1, S_BETC, S_CAM0, S_CAM1, S_COUNT };
constexpr int V_COUNT = 3;               // partial sums of a vertex workgroup
// weights[]: APG_LOSS_W_* of the header
enum { W_TRANS, W_KP2D, W_KP3D, W_SHAPE, W_ROOT, W_POSE, W_BETA, W_CAM, W_LIMBS3D, W_LIMBSTHETA, W_SCALE };

struct LossArgs {
    int nviews, cross, B, J, Jg;
    long long nv;                        // B V 3
    int nsb;                             // small-term workgroups
    long long nvb;                       // vertex workgroups
    // per view (entry 1 unused with one view)
    const float *trans[2], *rotmat[2], *betas[2], *joints[2], *verts[2], *j2d[2], *cam[2];
    const float *gt_root[2], *gt_j2d[2], *gt_trans[2];
    const float *gt_pose, *gt_joints, *gt_verts;
    float *g_trans[2], *g_rotmat[2], *g_betas[2], *g_joints[2], *g_verts[2], *g_j2d[2], *g_cam[2];
    // seed coefficients scale * w_k * 2 / N_k (cam: scale * w_cam * -20 / B), rounded once from the host's double
    float c_trans, c_kp2d, c_kp3d, c_shape, c_root, c_pose, c_beta, c_cam;
    float limbs3d, limbstheta;
    float* vpart;                        // [nvb][V_COUNT]
    float* spart;                        // [nsb][S_COUNT]
};

struct CombineArgs {
    int nviews, nsb;
    long long nvb;
    const float* vpart;
    const float* spart;
    float w[11];
    float n_trans, n_kp2d, n_kp3d, n_shape, n_root, n_pose, n_beta, n_cam;     // the means' denominators
    int has_trans, has_cam;
    float* terms;
};

template <bool ALIGNED>
__device__ __forceinline__ void load4(const float* p, float* v) {
    if (ALIGNED) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void store4(float* p, const float* v) {
    if (ALIGNED) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
    }
}

// one element of a term with up to two views and a cross-view share: acc3 += (d0^2, d1^2, dc^2); seeds c (d0 + dc), c (d1 - dc)
__device__ __forceinline__ void pair_elem(float a, float b, float g, bool two, bool cross, float c, float* acc, float& ga, float& gb) {
    const float d0 = a - g;
    float d1 = 0.f, dc = 0.f;
    acc[0] = fmaf(d0, d0, acc[0]);
    if (two) {
        d1 = b - g;
        acc[1] = fmaf(d1, d1, acc[1]);
        if (cross) {
            dc = a - b;
            acc[2] = fmaf(dc, dc, acc[2]);
        }
    }
    ga = c * (d0 + dc);
    gb = c * (d1 - dc);
}

template <bool ALIGNED>
__device__ __forceinline__ void verts_block(const LossArgs& a, long long blk, float* s) {
    const bool two = a.nviews == 2, cross = (a.cross & APG_LOSS_CROSS_VERTS) != 0;
    const float* __restrict__ p0 = a.verts[0];
    const float* __restrict__ p1 = a.verts[1];
    const float* __restrict__ gt = a.gt_verts;
    float* __restrict__ g0 = a.g_verts[0];
    float* __restrict__ g1 = a.g_verts[1];
    const float c = a.c_shape;
    float acc[V_COUNT] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < LOSS_EPB / (LT * 4); ++i) {
        const long long e = blk * LOSS_EPB + ((long long)i * LT + threadIdx.x) * 4;
        if (e + 4 <= a.nv) {
            float va[4], vb[4] = {0.f, 0.f, 0.f, 0.f}, vg[4], ga[4], gb[4];
            load4<ALIGNED>(p0 + e, va);
            load4<ALIGNED>(gt + e, vg);
            if (two) load4<ALIGNED>(p1 + e, vb);
#pragma unroll
            for (int k = 0; k < 4; ++k) pair_elem(va[k], vb[k], vg[k], two, cross, c, acc, ga[k], gb[k]);
            if (g0) store4<ALIGNED>(g0 + e, ga);
            if (two && g1) store4<ALIGNED>(g1 + e, gb);
        } else {
            for (long long k = e; k < a.nv; ++k) {                        // the partial quad at the end of the stream
                float ga, gb;
                pair_elem(p0[k], two ? p1[k] : 0.f, gt[k], two, cross, c, acc, ga, gb);
                if (g0) g0[k] = ga;
                if (two && g1) g1[k] = gb;
            }
        }
    }
    block_reduce<V_COUNT>(s, acc);
    if (threadIdx.x < V_COUNT) a.vpart[blk * V_COUNT + threadIdx.x] = s[threadIdx.x * LT];
}

__device__ __forceinline__ void small_block(const LossArgs& a, int blk, float* s) {
    const int t = threadIdx.x;
    const int b0 = blk * LOSS_SB;
    const int nb = min(LOSS_SB, a.B - b0);
    const bool two = a.nviews == 2;
    const int nv = a.nviews;
    float acc[S_COUNT];
#pragma unroll
    for (int k = 0; k < S_COUNT; ++k) acc[k] = 0.f;

    if (a.trans[0])
        for (int i = t; i < nb * 3; i += LT) {
            const size_t o = (size_t)b0 * 3 + i;
            for (int v = 0; v < nv; ++v) {
                const float d = a.trans[v][o] - a.gt_trans[v][o];
                acc[S_TRANS0 + v] = fmaf(d, d, acc[S_TRANS0 + v]);
                if (a.g_trans[v]) a.g_trans[v][o] = a.c_trans * d;
            }
        }

    for (int i = t; i < nb * a.J * 2; i += LT) {                          // 2-D joints; rows >= 22 of the seed are zero
        const int b = b0 + i / (a.J * 2), r = i % (a.J * 2), j = r >> 1, c = r & 1;
        const size_t o = ((size_t)b * a.J + j) * 2 + c;
        if (j < NJ) {
            const size_t og = ((size_t)b * a.Jg + j) * 2 + c;
            for (int v = 0; v < nv; ++v) {
                const float d = a.j2d[v][o] - a.gt_j2d[v][og];
                acc[S_KP0 + v] = fmaf(d, d, acc[S_KP0 + v]);
                if (a.g_j2d[v]) a.g_j2d[v][o] = a.c_kp2d * d;
            }
        } else {
            for (int v = 0; v < nv; ++v)
                if (a.g_j2d[v]) a.g_j2d[v][o] = 0.f;
        }
    }

    {
        const float l = a.limbs3d, l2 = l * l;
        const bool cross = (a.cross & APG_LOSS_CROSS_JOINTS) != 0;
        for (int i = t; i < nb * a.J * 3; i += LT) {                      // 3-D joints
            const int b = b0 + i / (a.J * 3), r = i % (a.J * 3), j = r / 3, c = r % 3;
            const size_t o = ((size_t)b * a.J + j) * 3 + c;
            if (j < NJ) {
                const size_t og = ((size_t)b * a.Jg + j) * 3 + c;
                const float lw = limb_weight(j, l, l2);
                float e[3] = {0.f, 0.f, 0.f}, ga, gb;
                pair_elem(a.joints[0][o], two ? a.joints[1][o] : 0.f, a.gt_joints[og], two, cross, a.c_kp3d * lw, e, ga, gb);
                acc[S_KP3D] += ((e[0] + e[1]) + e[2]) * lw;
                if (a.g_joints[0]) a.g_joints[0][o] = ga;
                if (two && a.g_joints[1]) a.g_joints[1][o] = gb;
            } else {
                for (int v = 0; v < nv; ++v)
                    if (a.g_joints[v]) a.g_joints[v][o] = 0.f;
            }
        }
    }

    {
        const float l = a.limbstheta, l2 = l * l;
        const bool cross = (a.cross & APG_LOSS_CROSS_POSE) != 0;
        for (int i = t; i < nb * NJ * 9; i += LT) {                       // rotations: row 0 = root, rows 1 .. 21 = pose
            const int b = b0 + i / (NJ * 9), r = i % (NJ * 9), j = r / 9, k = r % 9;
            const size_t o = (size_t)b * (NJ * 9) + r;
            if (j == 0) {
                for (int v = 0; v < nv; ++v) {
                    const float d = a.rotmat[v][o] - a.gt_root[v][(size_t)b * 9 + k];
                    acc[S_ROOT0 + v] = fmaf(d, d, acc[S_ROOT0 + v]);
                    if (a.g_rotmat[v]) a.g_rotmat[v][o] = a.c_root * d;
                }
            } else {
                const float lw = limb_weight(j, l, l2);
                float e[3] = {0.f, 0.f, 0.f}, ga, gb;
                pair_elem(a.rotmat[0][o], two ? a.rotmat[1][o] : 0.f, a.gt_pose[((size_t)b * (NJ - 1) + (j - 1)) * 9 + k], two, cross,
                          a.c_pose * lw, e, ga, gb);
                acc[S_POSE] += ((e[0] + e[1]) + e[2]) * lw;
                if (a.g_rotmat[0]) a.g_rotmat[0][o] = ga;
                if (two && a.g_rotmat[1]) a.g_rotmat[1][o] = gb;
            }
        }
    }

    {
        const bool cross = (a.cross & APG_LOSS_CROSS_BETAS) != 0;
        for (int i = t; i < nb * 10; i += LT) {                           // betas against zero, and against each other
            const size_t o = (size_t)b0 * 10 + i;
            float e[3] = {0.f, 0.f, 0.f}, ga, gb;
            pair_elem(a.betas[0][o], two ? a.betas[1][o] : 0.f, 0.f, two, cross, a.c_beta, e, ga, gb);
            acc[S_BET0] += e[0], acc[S_BET1] += e[1], acc[S_BETC] += e[2];
            if (a.g_betas[0]) a.g_betas[0][o] = ga;
            if (two && a.g_betas[1]) a.g_betas[1][o] = gb;
        }
    }

    if (a.cam[0])
        for (int i = t; i < nb * 3; i += LT) {                            // exp(-10 s)^2 of the scale s = cam[:, 0]
            const size_t o = (size_t)b0 * 3 + i;
            for (int v = 0; v < nv; ++v) {
                float g = 0.f;
                if (i % 3 == 0) {
                    const float ex = expf(-10.f * a.cam[v][o]);
                    const float q = ex * ex;
                    acc[S_CAM0 + v] += q;
                    g = a.c_cam * q;
                }
                if (a.g_cam[v]) a.g_cam[v][o] = g;
            }
        }

    block_reduce<S_COUNT>(s, acc);
    if (t < S_COUNT) a.spart[(size_t)blk * S_COUNT + t] = s[t * LT];
}

template <bool ALIGNED>
__global__ void __launch_bounds__(LT) loss_main_kernel(const LossArgs a) {
    __shared__ float s[S_COUNT * LT];
    if ((int)blockIdx.x < a.nsb)                                            // uniform over the workgroup
        small_block(a, (int)blockIdx.x, s);
    else
        verts_block<ALIGNED>(a, (long long)blockIdx.x - a.nsb, s);
}

__global__ void __launch_bounds__(LT) loss_combine_kernel(const CombineArgs a) {
    __shared__ float s[(V_COUNT + S_COUNT) * LT];
    const int t = threadIdx.x;
    float v[V_COUNT + S_COUNT];
#pragma unroll
    for (int k = 0; k < V_COUNT + S_COUNT; ++k) v[k] = 0.f;
    for (long long i = t; i < a.nvb; i += LT)
#pragma unroll
        for (int k = 0; k < V_COUNT; ++k) v[k] += a.vpart[i * V_COUNT + k];
    for (int i = t; i < a.nsb; i += LT)
#pragma unroll
        for (int k = 0; k < S_COUNT; ++k) v[V_COUNT + k] += a.spart[(size_t)i * S_COUNT + k];
    block_reduce<V_COUNT + S_COUNT>(s, v);
    if (t != 0) return;
    const float* sv = s;                                                     // vertex sums: sv[k * LT]
    const float* ss = s + V_COUNT * LT;                                      // small sums: ss[k * LT]
    const bool two = a.nviews == 2;
    auto S = [&](int k) { return ss[k * LT]; };
    float trans = 0.f, cam = 0.f;
    if (a.has_trans) trans = S(S_TRANS0) / a.n_trans + (two ? S(S_TRANS1) / a.n_trans : 0.f);
    const float kp = S(S_KP0) / a.n_kp2d + (two ? S(S_KP1) / a.n_kp2d : 0.f);
    const float kp3d = S(S_KP3D) / a.n_kp3d;
    const float shape = two ? (sv[0] / a.n_shape + sv[LT] / a.n_shape) + sv[2 * LT] / a.n_shape : sv[0] / a.n_shape;
    const float root = S(S_ROOT0) / a.n_root + (two ? S(S_ROOT1) / a.n_root : 0.f);
    const float pose = S(S_POSE) / a.n_pose;
    const float betas = two ? (S(S_BET0) / a.n_beta + S(S_BET1) / a.n_beta) + S(S_BETC) / a.n_beta : S(S_BET0) / a.n_beta;
    if (a.has_cam) cam = S(S_CAM0) / a.n_cam + (two ? S(S_CAM1) / a.n_cam : 0.f);
    float loss = a.w[W_TRANS] * trans;
    loss += a.w[W_KP2D] * kp;
    loss += a.w[W_KP3D] * kp3d;
    loss += a.w[W_SHAPE] * shape;
    loss += a.w[W_ROOT] * root;
    loss += a.w[W_POSE] * pose;
    loss += a.w[W_BETA] * betas;
    loss += a.w[W_CAM] * cam;
    loss *= a.w[W_SCALE];
    a.terms[0] = loss, a.terms[1] = trans, a.terms[2] = kp, a.terms[3] = kp3d, a.terms[4] = shape;
    a.terms[5] = root, a.terms[6] = pose, a.terms[7] = betas, a.terms[8] = cam;
}

inline long long loss_nvb(int B, int V) { return ((long long)B * V * 3 + LOSS_EPB - 1) / LOSS_EPB; }
inline int loss_nsb(int B) { return (B + LOSS_SB - 1) / LOSS_SB; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t apg_loss_workspace_bytes(int B, int V) {
    if (B < 1 || V < 1) return -1;
    // one workgroup per partial: B V 3 / LOSS_EPB + B / LOSS_SB workgroups must fit the grid's 2^31 - 1.  Refused on B * V first
    // (a product of two ints, at most 2^62), so that B V 3 below cannot overflow
    if ((long long)B * V > (0x7fffffffLL - loss_nsb(B)) * (LOSS_EPB / 3)) return -1;
    const long long nvb = loss_nvb(B, V);
    if (nvb + loss_nsb(B) > 0x7fffffffLL) return -1;
    const long long floats = nvb * V_COUNT + (long long)loss_nsb(B) * S_COUNT;
    return (int64_t)((floats * 4 + 255) / 256 * 256);
}

int apg_loss_fwd_bwd(int nviews, int cross, int B, int J, int Jg, int V, const float* weights, const void* const* pred,
                     const void* const* gt, float* terms, void* const* grads, void* workspace, int64_t workspace_bytes, void* stream) {
    if (nviews != 1 && nviews != 2) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: nviews must be 1 or 2");
    if (cross & ~APG_LOSS_CROSS_ALL) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: unknown cross-view bits");
    if (cross && nviews == 1) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: cross-view terms need two views");
    if (B < 1 || V < 1) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: B and V must be >= 1");
    if (J < NJ || Jg < NJ) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: the loss reads joints 0 .. 21, J and Jg must be >= 22");
    if (!weights || !pred || !gt || !terms || !workspace)
        return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: weights, pred, gt, terms and workspace are required");
    const int64_t need = apg_loss_workspace_bytes(B, V);
    if (need < 0) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: B * V is too large");

    LossArgs a = {};
    a.nviews = nviews, a.cross = cross, a.B = B, a.J = J, a.Jg = Jg;
    a.nv = (long long)B * V * 3;
    a.nsb = loss_nsb(B), a.nvb = loss_nvb(B, V);
    static const char* const pname[APG_LOSS_PER_VIEW] = {"trans", "rotmat", "betas", "joints", "verts", "j2d", "cam"};
    for (int v = 0; v < nviews; ++v) {
        const float* const* p = (const float* const*)pred + v * APG_LOSS_PER_VIEW;
        a.trans[v] = p[0], a.rotmat[v] = p[1], a.betas[v] = p[2], a.joints[v] = p[3], a.verts[v] = p[4], a.j2d[v] = p[5], a.cam[v] = p[6];
        for (int k = 1; k <= 5; ++k)
            if (!p[k]) return apg_fail(APG_EINVAL, std::string("apg_loss_fwd_bwd: ") + pname[k] + " of view " + std::to_string(v) + " is NULL");
        const float* const* g = (const float* const*)gt + 3 + v * 3;
        a.gt_root[v] = g[0], a.gt_j2d[v] = g[1], a.gt_trans[v] = g[2];
        if (!g[0] || !g[1]) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: gt_root / gt_j2d of view " + std::to_string(v) + " is NULL");
        if (p[0] && !g[2]) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: trans of view " + std::to_string(v) + " has no gt_trans");
        if (grads) {
            float* const* q = (float* const*)grads + v * APG_LOSS_PER_VIEW;
            a.g_trans[v] = q[0], a.g_rotmat[v] = q[1], a.g_betas[v] = q[2], a.g_joints[v] = q[3], a.g_verts[v] = q[4], a.g_j2d[v] = q[5];
            a.g_cam[v] = q[6];
            if ((q[0] && !p[0]) || (q[6] && !p[6]))
                return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: a gradient of view " + std::to_string(v) + " is asked for an absent trans / cam");
        }
    }
    if (nviews == 2 && ((a.trans[0] == nullptr) != (a.trans[1] == nullptr) || (a.cam[0] == nullptr) != (a.cam[1] == nullptr)))
        return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: trans / cam must be given for both views or for neither");
    a.gt_pose = (const float*)gt[0], a.gt_joints = (const float*)gt[1], a.gt_verts = (const float*)gt[2];
    if (!a.gt_pose || !a.gt_joints || !a.gt_verts) return apg_fail(APG_EINVAL, "apg_loss_fwd_bwd: gt_pose, gt_joints and gt_verts are required");
    if (workspace_bytes < need)
        return apg_fail(APG_ENOMEM, "apg_loss_fwd_bwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) +
                                        " needed");

    const double sc = weights[W_SCALE], Bd = B;
    const double n_trans = Bd * 3, n_kp2d = Bd * NJ * 2, n_kp3d = Bd * NJ * 3, n_shape = Bd * V * 3, n_root = Bd * 9, n_pose = Bd * (NJ - 1) * 9,
                 n_beta = Bd * 10, n_cam = Bd;
    a.c_trans = (float)(sc * weights[W_TRANS] * 2.0 / n_trans);
    a.c_kp2d = (float)(sc * weights[W_KP2D] * 2.0 / n_kp2d);
    a.c_kp3d = (float)(sc * weights[W_KP3D] * 2.0 / n_kp3d);
    a.c_shape = (float)(sc * weights[W_SHAPE] * 2.0 / n_shape);
    a.c_root = (float)(sc * weights[W_ROOT] * 2.0 / n_root);
    a.c_pose = (float)(sc * weights[W_POSE] * 2.0 / n_pose);
    a.c_beta = (float)(sc * weights[W_BETA] * 2.0 / n_beta);
    a.c_cam = (float)(sc * weights[W_CAM] * -20.0 / n_cam);
    a.limbs3d = weights[W_LIMBS3D], a.limbstheta = weights[W_LIMBSTHETA];
    a.vpart = (float*)workspace;
    a.spart = a.vpart + a.nvb * V_COUNT;

    CombineArgs c = {};
    c.nviews = nviews, c.nsb = a.nsb, c.nvb = a.nvb, c.vpart = a.vpart, c.spart = a.spart;
    for (int k = 0; k < 11; ++k) c.w[k] = weights[k];
    c.n_trans = (float)n_trans, c.n_kp2d = (float)n_kp2d, c.n_kp3d = (float)n_kp3d, c.n_shape = (float)n_shape, c.n_root = (float)n_root;
    c.n_pose = (float)n_pose, c.n_beta = (float)n_beta, c.n_cam = (float)n_cam;
    c.has_trans = a.trans[0] != nullptr, c.has_cam = a.cam[0] != nullptr;
    c.terms = terms;

    bool al = aligned16(a.gt_verts);
    for (int v = 0; v < nviews; ++v) al = al && aligned16(a.verts[v]) && aligned16(a.g_verts[v]);
    const dim3 grid((unsigned)(a.nsb + a.nvb));
    hipStream_t st = (hipStream_t)stream;
    if (al)
        hipLaunchKernelGGL(loss_main_kernel<true>, grid, dim3(LT), 0, st, a);
    else
        hipLaunchKernelGGL(loss_main_kernel<false>, grid, dim3(LT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(LT), 0, st, c);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
