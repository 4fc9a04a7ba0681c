// SMPL-X backward kernels for gfx950: the adjoint of ap_smplx_fwd (upstream smplx 0.1.28 lbs.lbs as plain autograd sees it)
// and of lbs.batch_rodrigues.  The driver (api_smplx.hip, ap_smplx_bwd) first recomputes the forward's bone transforms A and v_posed
// into the backward's own workspaces (smplx_prep_kernel + the blend-shape GEMM), then:
//   1. smplx_bwd_lbs_kernel    (vertex range x body): g_v = grad_vertices + the extra-joint / landmark gradients scattered onto
//                              their vertices; g_vposed = T_v[:3,:3]^T g_v; g_A_k = sum_v w_vk g_v (x) [v_posed_v, 1] per range
//   2. smplx_bwd_coef_kernel   (reduction split x body tile x K tile): g_coef = g_vposed . dirs on the fp32 matrix pipe
//                              (v_mfma_f32_16x16x4_f32, exact fp32), one partial per reduction split
//   3. smplx_bwd_chain_kernel  (one wave per body, lane = joint): the kinematic chain backwards -> g_R, g_J; shape / expression
//                              gradient = j_shapedirs^T g_J + g_coef[0..19]; g_R_k += g_coef[pose feature of k]; g_transl
// Every reduction runs in a fixed order (wave butterflies, partials summed in index order): no floating-point atomics, and a
// body's gradients do not depend on how many bodies share the call or where it sits in the batch.
#include "ap_common.h"
#include "kernels.h"

namespace {

constexpr int BW_T = 256;           // threads of the LBS-adjoint workgroup
constexpr int BW_MAXJ = 64;

__device__ __forceinline__ float bw_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------
// grid (vertex ranges of SMPLX_BWD_RV, bodies).  Pass 1 (thread = vertex): the vertex gradient, g_vposed, and the range's
// vertex gradients / rest-posed points in LDS.  Pass 2 (wave = bone): the bone's skinning entries inside the range (bone-major
// table built on the first backward), lanes over entries, one butterfly per bone-transform entry.
__global__ void __launch_bounds__(BW_T) smplx_bwd_lbs_kernel(const SmplxModelDev m, const SmplxBwdArgs a) {
    __shared__ float As[BW_MAXJ * 12];
    __shared__ float sg[SMPLX_BWD_RV * 3], sp[SMPLX_BWD_RV * 3];
    __shared__ float st[BW_T / 64][3];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nj = m.J + m.n_extra + m.n_lmk;
    for (int i = tid; i < m.J * 12; i += BW_T) As[i] = a.A[(size_t)b * m.J * 12 + i];
    __syncthreads();
    const int v0 = r * SMPLX_BWD_RV, nv = min(SMPLX_BWD_RV, m.V - v0);
    float ts[3] = {0.f, 0.f, 0.f};
    for (int i = tid; i < nv; i += BW_T) {
        const int v = v0 + i;
        float g[3] = {0.f, 0.f, 0.f};
        if (a.grad_vertices) {
            const float* s = a.grad_vertices + ((size_t)b * m.V + v) * 3;
            g[0] = s[0]; g[1] = s[1]; g[2] = s[2];
            ts[0] += g[0]; ts[1] += g[1]; ts[2] += g[2];
        }
        if (a.grad_joints) {                                 // vertex picks and landmark corners (fixed order per vertex)
            const int s = m.jv_slot[v];
            if (s >= 0) {
                for (int e = a.jv_off[s]; e < a.jv_off[s + 1]; ++e) {
                    const int2 en = a.jv_ent[e];
                    const float w = __int_as_float(en.y);
                    const float* gj = a.grad_joints + ((size_t)b * nj + en.x) * 3;
                    g[0] = fmaf(w, gj[0], g[0]); g[1] = fmaf(w, gj[1], g[1]); g[2] = fmaf(w, gj[2], g[2]);
                }
            }
        }
        const float* vp = a.vposed + (size_t)b * m.ldv + 3 * (size_t)v;
        float T[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = 0.f;
        for (int k = 0; k < m.K; ++k) {
            const float w = m.skin_w[(size_t)v * m.K + k];
            const float* Ak = As + m.skin_idx[(size_t)v * m.K + k] * 12;
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                for (int c = 0; c < 3; ++c) T[rr * 3 + c] = fmaf(w, Ak[rr * 4 + c], T[rr * 3 + c]);
        }
        float* gq = a.gvp + (size_t)b * m.ldv + 3 * (size_t)v;
#pragma unroll
        for (int c = 0; c < 3; ++c) gq[c] = T[c] * g[0] + T[3 + c] * g[1] + T[6 + c] * g[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) { sg[3 * i + c] = g[c]; sp[3 * i + c] = vp[c]; }
    }
    // the range's share of sum_v grad_vertices (g_transl)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = bw_wave_sum(ts[c]);
        if (lane == 0) st[wave][c] = s;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.f;
        for (int w = 0; w < BW_T / 64; ++w) s += st[w][tid];
        a.gt[((size_t)b * a.nr + r) * 3 + tid] = s;
    }
    for (int j = wave; j < m.J; j += BW_T / 64) {
        const int lo = a.bone_off[j * (a.nr + 1) + r], hi = a.bone_off[j * (a.nr + 1) + r + 1];
        float acc[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[e] = 0.f;
        for (int e = lo + lane; e < hi; e += 64) {
            const int2 en = a.bone_ent[e];
            const int li = en.x - v0;
            const float w = __int_as_float(en.y);
            const float p0 = sp[3 * li], p1 = sp[3 * li + 1], p2 = sp[3 * li + 2];
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                const float gw = w * sg[3 * li + rr];
                acc[rr * 4 + 0] = fmaf(gw, p0, acc[rr * 4 + 0]);
                acc[rr * 4 + 1] = fmaf(gw, p1, acc[rr * 4 + 1]);
                acc[rr * 4 + 2] = fmaf(gw, p2, acc[rr * 4 + 2]);
                acc[rr * 4 + 3] += gw;
            }
        }
        if (lo < hi) {                                       // (wave-uniform)
#pragma unroll
            for (int e = 0; e < 12; ++e) acc[e] = bw_wave_sum(acc[e]);
        }
        if (lane < 12) {
            float o = 0.f;
#pragma unroll
            for (int e = 0; e < 12; ++e) o = lane == e ? acc[e] : o;
            a.gA[(((size_t)b * a.nr + r) * m.J + j) * 12 + lane] = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// g_coef[b][k] = sum_row g_vposed[b][row] dirs[row][k], rows = 3V, on v_mfma_f32_16x16x4_f32.  grid (reduction splits of
// SMPLX_BWD_RC rows, body tiles of 64, K tiles of 256); wave = 16 bodies x NBK column blocks of 16.  MFMA step s of a 16-row
// slice: lane (i, q) feeds A = g_vposed[body i][row r + 4q + s] and B = dirs[row r + 4q + s][col i] (the A / B maps of the
// 16x16x4 form: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]); C/D: col = l & 15, row = 4 (l >> 4) + reg.
template <int NBK>
__global__ void __launch_bounds__(256) smplx_bwd_coef_kernel(const SmplxModelDev m, const SmplxBwdArgs a) {
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.y * 64 + wave * 16;
    if (b0 >= a.n) return;
    const int k0 = blockIdx.z * 256;
    const int i = lane & 15, q = lane >> 4;
    const int rows = 3 * m.V, r16 = (rows + 15) & ~15;
    const int rbeg = c * SMPLX_BWD_RC, rend = min(rbeg + SMPLX_BWD_RC, r16);
    const float* ap = a.gvp + (size_t)min(b0 + i, a.n - 1) * m.ldv + 4 * q;   // (rows past the last body: clamped, never stored)
    const float* bp = a.dirs + (size_t)(4 * q) * m.ncoef + k0 + i;
    f32x4 acc[NBK];
#pragma unroll
    for (int k = 0; k < NBK; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = rbeg; r < rend; r += 16) {
        const float4 av = *(const float4*)(ap + r);          // 16-byte aligned: ldv and r are multiples of 16
        const int rq = r + 4 * q;
        const float as[4] = {rq < rows ? av.x : 0.f, rq + 1 < rows ? av.y : 0.f, rq + 2 < rows ? av.z : 0.f,
                             rq + 3 < rows ? av.w : 0.f};   // the pad rows of g_vposed are never written
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float* brow = bp + (size_t)(r + s) * m.ncoef;
            float bv[NBK];
#pragma unroll
            for (int k = 0; k < NBK; ++k) bv[k] = brow[k * 16];
#pragma unroll
            for (int k = 0; k < NBK; ++k) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[s], bv[k], acc[k], 0, 0, 0);
        }
    }
#pragma unroll
    for (int k = 0; k < NBK; ++k) {
        const int col = k0 + k * 16 + i;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int body = b0 + 4 * q + e;
            if (body < a.n && col < a.kp) a.gcoef[((size_t)c * a.n + body) * a.kp + col] = acc[k][e];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// One wave per body, lane = joint (smplx_prep_kernel's chain, then its adjoint level by level from the leaves).  Forward:
// G_k = G_p [R_k | J_k - J_p], A_k = [G_k.R | G_k.t - G_k.R J_k], posed joint = G_k.t.  Adjoint, with g_A from the LBS kernel
// and the chain joints' own gradients: g_GR = g_AR - g_At J^T, g_Gt = g_At + g_joint, g_J = -G_R^T g_At; a child pushes
// g_GR R^T + g_Gt rel^T, g_Gt and -G_pR^T g_Gt to its parent (the parent pulls them in ascending child order) and keeps
// g_R = G_pR^T g_GR, g_J += G_pR^T g_Gt.
__global__ void __launch_bounds__(64) smplx_bwd_chain_kernel(const SmplxModelDev m, const SmplxBwdArgs a) {
    __shared__ float G[BW_MAXJ][12];
    __shared__ float Jr[BW_MAXJ][3];
    __shared__ float cf[20];
    __shared__ float cGR[BW_MAXJ][9], cGt[BW_MAXJ][3], cJ[BW_MAXJ][3], gJs[BW_MAXJ][3];
    __shared__ int par_s[BW_MAXJ];
    const int b = blockIdx.x, j = threadIdx.x;
    const bool live = j < m.J;
    const int nj = m.J + m.n_extra + m.n_lmk;
    if (j < 20) cf[j] = j < 10 ? a.betas[(size_t)b * 10 + j] : (a.expression ? a.expression[(size_t)b * 10 + j - 10] : 0.f);
    par_s[j] = live ? (j == 0 ? -1 : m.parents[j]) : -2;
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (live) {
        const float* src = j == 0 ? a.global_orient ? a.global_orient + (size_t)b * 9 : nullptr
                         : j < 22 ? a.body_pose + ((size_t)b * 21 + (j - 1)) * 9
                         : a.extra_pose ? a.extra_pose + ((size_t)b * (m.J - 22) + (j - 22)) * 9 : nullptr;
        if (src)
            for (int e = 0; e < 9; ++e) R[e] = src[e];
    }
    const int dep = live ? m.depth[j] : -1;
    __syncthreads();
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = 0.f;
#pragma unroll
            for (int l = 0; l < 20; ++l) acc = fmaf(m.j_shapedirs[((size_t)j * 3 + c) * 20 + l], cf[l], acc);
            Jr[j][c] = m.j_template[j * 3 + c] + acc;
        }
    }
    __syncthreads();
    const int par = (live && j > 0) ? par_s[j] : 0;
    float rel[3] = {0.f, 0.f, 0.f};
    if (live) {
        for (int c = 0; c < 3; ++c) rel[c] = j == 0 ? Jr[0][c] : Jr[j][c] - Jr[par][c];
        if (j == 0)
            for (int rr = 0; rr < 3; ++rr) {
                G[0][rr * 4 + 0] = R[rr * 3 + 0]; G[0][rr * 4 + 1] = R[rr * 3 + 1]; G[0][rr * 4 + 2] = R[rr * 3 + 2];
                G[0][rr * 4 + 3] = rel[rr];
            }
    }
    __syncthreads();
    for (int d = 1; d <= m.max_depth; ++d) {
        if (dep == d) {
            float P[12];
            for (int e = 0; e < 12; ++e) P[e] = G[par][e];
            for (int rr = 0; rr < 3; ++rr) {
                const float p0 = P[rr * 4 + 0], p1 = P[rr * 4 + 1], p2 = P[rr * 4 + 2], p3 = P[rr * 4 + 3];
                G[j][rr * 4 + 0] = p0 * R[0] + p1 * R[3] + p2 * R[6];
                G[j][rr * 4 + 1] = p0 * R[1] + p1 * R[4] + p2 * R[7];
                G[j][rr * 4 + 2] = p0 * R[2] + p1 * R[5] + p2 * R[8];
                G[j][rr * 4 + 3] = p0 * rel[0] + p1 * rel[1] + p2 * rel[2] + p3;
            }
        }
        __syncthreads();
    }
    // ---- adjoint
    float gA[12], gGR[9], gGt[3], gJ[3], gR[9];
#pragma unroll
    for (int e = 0; e < 12; ++e) gA[e] = 0.f;
    if (live)
        for (int r = 0; r < a.nr; ++r) {
            const float* s = a.gA + (((size_t)b * a.nr + r) * m.J + j) * 12;
#pragma unroll
            for (int e = 0; e < 12; ++e) gA[e] += s[e];
        }
    float gjp[3] = {0.f, 0.f, 0.f};
    if (live && a.grad_joints)
        for (int c = 0; c < 3; ++c) gjp[c] = a.grad_joints[((size_t)b * nj + j) * 3 + c];
    const float Jj[3] = {live ? Jr[j][0] : 0.f, live ? Jr[j][1] : 0.f, live ? Jr[j][2] : 0.f};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) gGR[rr * 3 + cc] = gA[rr * 4 + cc] - gA[rr * 4 + 3] * Jj[cc];
        gGt[rr] = gA[rr * 4 + 3] + gjp[rr];
    }
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        float s = 0.f;
        if (live)
            for (int rr = 0; rr < 3; ++rr) s += G[j][rr * 4 + cc] * gA[rr * 4 + 3];
        gJ[cc] = -s;
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) gR[e] = 0.f;
    for (int d = m.max_depth; d >= 1; --d) {
        if (dep == d) {
            float P[12];
            for (int e = 0; e < 12; ++e) P[e] = G[par][e];
            for (int x = 0; x < 3; ++x)
                for (int y = 0; y < 3; ++y)
                    gR[x * 3 + y] = P[0 * 4 + x] * gGR[0 * 3 + y] + P[1 * 4 + x] * gGR[1 * 3 + y] + P[2 * 4 + x] * gGR[2 * 3 + y];
            float grel[3];
            for (int cc = 0; cc < 3; ++cc) grel[cc] = P[0 * 4 + cc] * gGt[0] + P[1 * 4 + cc] * gGt[1] + P[2 * 4 + cc] * gGt[2];
            for (int rr = 0; rr < 3; ++rr) {
                for (int cc = 0; cc < 3; ++cc)
                    cGR[j][rr * 3 + cc] = gGR[rr * 3 + 0] * R[cc * 3 + 0] + gGR[rr * 3 + 1] * R[cc * 3 + 1] +
                                          gGR[rr * 3 + 2] * R[cc * 3 + 2] + gGt[rr] * rel[cc];
                cGt[j][rr] = gGt[rr];
                cJ[j][rr] = -grel[rr];
                gJ[rr] += grel[rr];
            }
        }
        __syncthreads();
        if (dep == d - 1) {
            for (int c2 = 1; c2 < m.J; ++c2) {
                if (par_s[c2] != j) continue;
                for (int e = 0; e < 9; ++e) gGR[e] += cGR[c2][e];
                for (int e = 0; e < 3; ++e) { gGt[e] += cGt[c2][e]; gJ[e] += cJ[c2][e]; }
            }
        }
        __syncthreads();
    }
    if (j == 0) {                                            // G_0 = [R_0 | J_0]
        for (int e = 0; e < 9; ++e) gR[e] = gGR[e];
        for (int e = 0; e < 3; ++e) gJ[e] += gGt[e];
    }
    // pose feature (R_k - I, k >= 1): the blend-shape part of g_R
    if (live && j >= 1 && a.nsplit > 0) {
        for (int e = 0; e < 9; ++e) {
            const int k = 20 + (j - 1) * 9 + e;
            if (k >= a.kp) break;
            float s = 0.f;
            for (int c = 0; c < a.nsplit; ++c) s += a.gcoef[((size_t)c * a.n + b) * a.kp + k];
            gR[e] += s;
        }
    }
    for (int c = 0; c < 3; ++c) gJs[j][c] = live ? gJ[c] : 0.f;
    __syncthreads();
    if (j < 20 && ((j < 10 && a.grad_betas) || (j >= 10 && a.grad_expression))) {
        float s = 0.f;
        for (int c = 0; c < a.nsplit; ++c) s += a.gcoef[((size_t)c * a.n + b) * a.kp + j];
        for (int jj = 0; jj < m.J; ++jj)
            for (int c = 0; c < 3; ++c) s = fmaf(m.j_shapedirs[((size_t)jj * 3 + c) * 20 + j], gJs[jj][c], s);
        if (j < 10) a.grad_betas[(size_t)b * 10 + j] = s;
        else a.grad_expression[(size_t)b * 10 + j - 10] = s;
    }
    if (live) {
        float* dst = j == 0 ? a.grad_global_orient ? a.grad_global_orient + (size_t)b * 9 : nullptr
                   : j < 22 ? a.grad_body_pose ? a.grad_body_pose + ((size_t)b * 21 + (j - 1)) * 9 : nullptr
                   : a.grad_extra_pose ? a.grad_extra_pose + ((size_t)b * (m.J - 22) + (j - 22)) * 9 : nullptr;
        if (dst)
            for (int e = 0; e < 9; ++e) dst[e] = gR[e];
    }
    if (j < 3 && a.grad_transl) {                            // transl is added to every vertex and every output joint
        float s = 0.f;
        for (int r = 0; r < a.nr; ++r) s += a.gt[((size_t)b * a.nr + r) * 3 + j];
        if (a.grad_joints)
            for (int t = 0; t < nj; ++t) s += a.grad_joints[((size_t)b * nj + t) * 3 + j];
        a.grad_transl[(size_t)b * 3 + j] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// adjoint of batch_rodrigues_kernel variant 0 (lbs.batch_rodrigues, angle = |r + 1e-8|, d = r / angle,
// R = I + sin K + (1 - cos) K K with K = skew(d), K K = d d^T - |d|^2 I):
//   g_sin = <g_R, K>, g_c1 = <g_R, K K>, g_angle = cos g_sin + sin g_c1, g_K = sin g_R + c1 (g_R K^T + K^T g_R),
//   g_d = (g_K[2,1] - g_K[1,2], g_K[0,2] - g_K[2,0], g_K[1,0] - g_K[0,1]), g_r = g_d / angle + (g_angle - <g_d, r> / angle) (r + eps) / angle
__global__ void batch_rodrigues_bwd_kernel(const float* __restrict__ aa, int n, const float* __restrict__ gR,
                                           float* __restrict__ gaa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float rx = aa[(size_t)i * 3], ry = aa[(size_t)i * 3 + 1], rz = aa[(size_t)i * 3 + 2];
    const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
    const float th = sqrtf(ex * ex + ey * ey + ez * ez);
    const float x = rx / th, y = ry / th, z = rz / th;
    const float sn = sinf(th), cs = cosf(th), c1 = 1.f - cs, dd = x * x + y * y + z * z;
    const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
    const float K2[9] = {x * x - dd, x * y, x * z, x * y, y * y - dd, y * z, x * z, y * z, z * z - dd};
    float g[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) g[e] = gR[(size_t)i * 9 + e];
    float gs = 0.f, gc = 0.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) { gs += g[e] * K[e]; gc += g[e] * K2[e]; }
    float gth = cs * gs + sn * gc;
    float gK[9];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < 3; ++t) acc += g[p * 3 + t] * K[q * 3 + t] + K[t * 3 + p] * g[t * 3 + q];
            gK[p * 3 + q] = sn * g[p * 3 + q] + c1 * acc;
        }
    // (K2 is K K written out; its derivative with respect to K is the product rule above, as autograd takes it upstream)
    const float gx = gK[7] - gK[5], gy = gK[2] - gK[6], gz = gK[3] - gK[1];
    gth -= (gx * rx + gy * ry + gz * rz) / (th * th);
    const float it = 1.f / th, s = gth / th;
    gaa[(size_t)i * 3 + 0] = gx * it + s * ex;
    gaa[(size_t)i * 3 + 1] = gy * it + s * ey;
    gaa[(size_t)i * 3 + 2] = gz * it + s * ez;
}

}  // namespace

hipError_t ap_launch_smplx_bwd_lbs(const SmplxModelDev& m, const SmplxBwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(smplx_bwd_lbs_kernel, dim3(a.nr, a.n), dim3(BW_T), 0, st, m, a);
    return hipGetLastError();
}

hipError_t ap_launch_smplx_bwd_coef(const SmplxModelDev& m, const SmplxBwdArgs& a, hipStream_t st) {
    const dim3 grid(a.nsplit, (a.n + 63) / 64, (a.kp + 255) / 256);
    if (a.kp <= 224) hipLaunchKernelGGL(smplx_bwd_coef_kernel<14>, grid, dim3(256), 0, st, m, a);
    else hipLaunchKernelGGL(smplx_bwd_coef_kernel<16>, grid, dim3(256), 0, st, m, a);
    return hipGetLastError();
}

hipError_t ap_launch_smplx_bwd_chain(const SmplxModelDev& m, const SmplxBwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(smplx_bwd_chain_kernel, dim3(a.n), dim3(64), 0, st, m, a);
    return hipGetLastError();
}

hipError_t ap_launch_batch_rodrigues_bwd(const float* aa, int n, const float* gR, float* gaa, hipStream_t st) {
    hipLaunchKernelGGL(batch_rodrigues_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, aa, n, gR, gaa);
    return hipGetLastError();
}
