// The real-data fine-tuning loss of the reference's copenet_real trainers (get_loss) and its gradient seeds in one pass, for gfx950
// (libairpose_grad.so).  See include/airpose_grad.h for the terms.
//
//   real_pack_kernel            the folded encoder (W1 512 x 63, b1, W2 64 x 512, b2) into the packed table: each matrix in both
//                               orientations, so that every GEMV below reads consecutive floats in consecutive lanes
//   real_main_kernel            grid = nviews * B workgroups of 256 threads, ONE (view, body) row each:
//     threads 0 .. 20             rotation j + 1 -> axis-angle (aa_fwd), kept in registers for the adjoint
//     all                         h = W1 aa + b1 (two outputs per thread, 63 fmaf in index order), a = leaky(h), both in LDS
//     all                         [mu | s] = W2 a + b2: output t & 63, k segment t >> 6 of 128 (fmaf in index order), the four segments
//                                 added in order, then b2
//     threads 0 .. 31             z = mu + softplus(s) eps, z^2, the seeds d mu = c z, d s = c z eps sigmoid(s)
//     all                         the way back: da = W2^T d[mu | s] (64 fmaf), dh = da leaky'(h), daa = W1^T dh (four segments of 128)
//     threads 0 .. 20             aa_bwd, + the pose term's share, rows 1 .. 21 of g_rotmat; threads 21 .. 29 the zero row 0
//     all                         the keypoint term and its seeds (fixed tree), betas (threads 0 .. 9), depth (thread 0)
//     thread 0                    the row's six partial sums, each list added in index order
//   real_combine_kernel         one workgroup: the rows' partials per view, thread-strided in index order, then a fixed tree; the six terms
//
// Determinism.  No atomics.  One row per workgroup whatever B is, so the only partition that moves with the shape is the combine's
// stride of 256 rows per view.  Every access is a 4-byte one: alignment cannot change a bit.  Which gradients are asked for decides
// what is stored (and whether a row's way back runs at all), never what another output's arithmetic is.
//
// Built with -fno-slp-vectorize (Makefile: FLAGS_loss_real_grad), as smplx.hip and smplx_bwd.hip are: with SLP vectorisation hipcc jams
// the two-output h loop into v_pk_fma_f32 on LDS-read operands (65 of them), the family of code that gave wrong lanes in
// smplx_prep_kernel while another kernel's waves shared the SIMD.  With the flag the device code holds no packed fp32 math.
//
// aa_fwd / aa_bwd are the fitter's, shared with fitting.hip (libairpose_hip.so) through rot_aa.inc; the tree, limb_weight, LT and NJ
// are shared with loss_grad.hip and geom_grad.hip through loss_common.inc.  The hidden vector stays in LDS between the two halves.
#include "grad_internal.h"

#include <string>

namespace {

#include "loss_common.inc"
#include "rot_aa.inc"

constexpr int NR = 21;                   // body rotations behind the prior
constexpr int NIN = 63, NH = 512, NO = 64, NZ = 32;
constexpr int SEG = NH / 4;              // k segment of the two long dot products
// the packed table, in floats
constexpr int P_W1T = 0;                 // [63][512]   W1T[j * 512 + k] = W1[k][j]
constexpr int P_B1 = P_W1T + NIN * NH;   // [512]
constexpr int P_W1B = P_B1 + NH;         // [512][64]   W1B[k * 64 + j] = W1[k][j], column 63 zero
constexpr int P_W2F = P_W1B + NH * 64;   // [512][64]   W2F[k * 64 + o] = W2[o][k]
constexpr int P_B2 = P_W2F + NH * NO;    // [64]
constexpr int P_W2B = P_B2 + NO;         // [64][512]   W2B[o * 512 + k] = W2[o][k]
constexpr int P_FLOATS = P_W2B + NO * NH;
// partial sums of a row
enum { R_KP, R_VP, R_POSE, R_BET, R_BETC, R_DEPTH, R_COUNT };
enum { W_KP, W_BETA, W_VPOSER, W_POSE, W_LIMBS2D, W_SCALE, W_COUNT };

struct RealArgs {
    int nviews, cross, B, J, Jg, col;
    float gain;
    const float* enc;
    const float *rotmat[2], *betas[2], *j2d[2], *depth[2], *gt[2], *eps[2];
    float *g_rotmat[2], *g_betas[2], *g_j2d[2], *g_depth[2];
    float c_kp, c_vp, c_pose, c_beta, c_depth;               // seed coefficients, rounded once from the host's double
    float limbs2d;
    float* part;                                             // [nviews * B][R_COUNT]
};

struct RealCombineArgs {
    int nviews, cross, B;
    const float* part;
    float w[W_COUNT];
    float n_kp, n_vp, n_pose, n_beta, n_depth;               // the means' denominators
    float* terms;
};

// the four k segments of thread t's output, in order
__device__ __forceinline__ float seg_sum(const float* sp, int o) { return ((sp[o] + sp[64 + o]) + sp[128 + o]) + sp[192 + o]; }

__global__ void __launch_bounds__(LT) real_main_kernel(const RealArgs a) {
    __shared__ float sx[64];             // aa (63), later d loss / d aa
    __shared__ float sh[NH];             // h, before the LeakyReLU
    __shared__ float sa[NH];             // leaky(h), later d loss / d h
    __shared__ float sp[LT];             // segment partials
    __shared__ float so[NO];             // [mu | s], later their seeds
    __shared__ float sz[NZ];             // z^2
    __shared__ float sred[LT];           // the keypoint tree
    __shared__ float spose[NR];
    __shared__ float sbet[20];
    __shared__ float sdepth;
    const int t = threadIdx.x;
    const int row = (int)blockIdx.x, v = row / a.B, b = row - v * a.B;
    const bool two = a.nviews == 2;
    const bool xpose = two && (a.cross & APG_LOSS_CROSS_POSE), xbeta = two && (a.cross & APG_LOSS_CROSS_BETAS);
    const float* __restrict__ E = a.enc;
    const float* R = a.rotmat[v] + (size_t)b * (NJ * 9);
    float* gR = a.g_rotmat[v] ? a.g_rotmat[v] + (size_t)b * (NJ * 9) : nullptr;

    AA st;
    if (t < NR) {
        st = aa_fwd(R + 9 * (t + 1));
        sx[3 * t] = st.aa.x, sx[3 * t + 1] = st.aa.y, sx[3 * t + 2] = st.aa.z;
    }
    if (t == 63) sx[63] = 0.f;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NH / LT; ++q) {
        const int k = t + q * LT;
        float acc = E[P_B1 + k];
        for (int j = 0; j < NIN; ++j) acc = fmaf(E[P_W1T + j * NH + k], sx[j], acc);
        sh[k] = acc;
        sa[k] = acc > 0.f ? acc : 0.01f * acc;
    }
    __syncthreads();
    {
        const int o = t & 63, k0 = (t >> 6) * SEG;
        float acc = 0.f;
        for (int i = 0; i < SEG; ++i) acc = fmaf(E[P_W2F + (k0 + i) * NO + o], sa[k0 + i], acc);
        sp[t] = acc;
    }
    __syncthreads();
    if (t < NO) so[t] = seg_sum(sp, t) + E[P_B2 + t];
    __syncthreads();
    float d_mu = 0.f, d_s = 0.f;
    if (t < NZ) {
        const float mu = so[t], s = so[NZ + t], e = a.eps[v][(size_t)b * NZ + t];
        const float sg = s > 20.f ? s : log1pf(expf(s));                   // torch's softplus
        const float z = fmaf(sg, e, mu);
        sz[t] = z * z;
        const float dz = a.c_vp * z;
        d_mu = dz;
        d_s = (dz * e) * (s > 20.f ? 1.f : 1.f / (1.f + expf(-s)));
    }
    __syncthreads();                                                        // every read of so is done
    if (t < NZ) so[t] = d_mu, so[NZ + t] = d_s;
    __syncthreads();

    if (gR) {                                                               // uniform over the workgroup
#pragma unroll
        for (int q = 0; q < NH / LT; ++q) {
            const int k = t + q * LT;
            float acc = 0.f;
            for (int o = 0; o < NO; ++o) acc = fmaf(E[P_W2B + o * NH + k], so[o], acc);
            sa[k] = sh[k] > 0.f ? acc : 0.01f * acc;
        }
        __syncthreads();
        {
            const int j = t & 63, k0 = (t >> 6) * SEG;
            float acc = 0.f;
            for (int i = 0; i < SEG; ++i) acc = fmaf(E[P_W1B + (k0 + i) * 64 + j], sa[k0 + i], acc);
            sp[t] = acc;
        }
        __syncthreads();
        if (t < 64) sx[t] = seg_sum(sp, t);
        __syncthreads();
    }

    // rotations: the pose term (counted once, on view 0's row) and rows 0 .. 21 of g_rotmat
    if (t < NR) {
        float dr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (gR) aa_bwd(st, v3(sx[3 * t], sx[3 * t + 1], sx[3 * t + 2]), dr);
        const float* R0 = a.rotmat[0] + (size_t)b * (NJ * 9) + 9 * (t + 1);
        const float* R1 = two ? a.rotmat[1] + (size_t)b * (NJ * 9) + 9 * (t + 1) : R0;
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            float share = 0.f;
            if (xpose) {
                const float dc = R0[e] - R1[e];
                if (v == 0) ps = fmaf(dc, dc, ps);                          // the term is counted once, on view 0's row
                share = a.c_pose * dc;
                if (v == 1) share = -share;
            }
            if (gR) gR[9 * (t + 1) + e] = share + dr[e];
        }
        spose[t] = ps;
    } else if (t < NR + 9) {
        if (gR) gR[t - NR] = 0.f;
    }

    // 2-D keypoints
    {
        const float l = a.limbs2d, l2 = l * l;
        const float* P = a.j2d[v] + (size_t)b * a.J * 2;
        const float* G = a.gt[v] + (size_t)b * a.Jg * 3;
        float* gP = a.g_j2d[v] ? a.g_j2d[v] + (size_t)b * a.J * 2 : nullptr;
        float acc = 0.f;
        for (int i = t; i < a.J * 2; i += LT) {
            const int j = i >> 1, c = i & 1;
            float g = 0.f;
            if (j < NJ) {
                const float d = P[i] - G[j * 3 + c];
                const float wgt = G[j * 3 + 2] * limb_weight(j, l, l2);
                acc = fmaf(d * d, wgt, acc);
                g = (a.c_kp * wgt) * d;
            }
            if (gP) gP[i] = g;
        }
        sred[t] = acc;
    }
    if (t < 10) {                                                           // betas against zero, and against each other
        const size_t o = (size_t)b * 10 + t;
        const float x = a.betas[v][o];
        float dc = 0.f;
        if (xbeta) dc = a.betas[0][o] - a.betas[1][o];
        sbet[t] = x * x;
        sbet[10 + t] = dc * dc;
        if (a.g_betas[v]) a.g_betas[v][o] = a.c_beta * (v == 0 ? x + dc : x - dc);
    }
    if (t < 3) {                                                            // exp(-gain d)^2 of column col
        const size_t o = (size_t)b * 3 + t;
        float g = 0.f;
        if (t == a.col) {
            const float ex = expf(-a.gain * a.depth[v][o]);
            const float q = ex * ex;
            sdepth = q;
            g = a.c_depth * q;
        }
        if (a.g_depth[v]) a.g_depth[v][o] = g;
    }
    // the keypoint tree: block_reduce<1>'s order, written out because sred[t] is stored above, ahead of the betas and depth work,
    // and moving that store down to the call changes the kernel's code
    __syncthreads();
    for (int h = LT / 2; h > 0; h >>= 1) {
        if (t < h) sred[t] += sred[t + h];
        __syncthreads();
    }
    if (t == 0) {
        float vp = 0.f, pose = 0.f, bs = 0.f, bc = 0.f;
        for (int i = 0; i < NZ; ++i) vp += sz[i];
        if (xpose && v == 0)
            for (int i = 0; i < NR; ++i) pose += spose[i];
        for (int i = 0; i < 10; ++i) bs += sbet[i];
        if (xbeta && v == 0)
            for (int i = 0; i < 10; ++i) bc += sbet[10 + i];
        float* p = a.part + (size_t)row * R_COUNT;
        p[R_KP] = sred[0], p[R_VP] = vp, p[R_POSE] = pose, p[R_BET] = bs, p[R_BETC] = bc, p[R_DEPTH] = sdepth;
    }
}

__global__ void __launch_bounds__(LT) real_combine_kernel(const RealCombineArgs a) {
    constexpr int NV = 2 * R_COUNT;
    __shared__ float s[NV * LT];
    const int t = threadIdx.x;
    float acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.f;
    for (int v = 0; v < a.nviews; ++v)
        for (int b = t; b < a.B; b += LT)
#pragma unroll
            for (int k = 0; k < R_COUNT; ++k) {
                const float x = a.part[((size_t)v * a.B + b) * R_COUNT + k];
                if (v == 0) acc[k] += x; else acc[R_COUNT + k] += x;
            }
    block_reduce<NV>(s, acc);
    if (t != 0) return;
    const bool two = a.nviews == 2;
    auto S = [&](int v, int k) { return s[(v * R_COUNT + k) * LT]; };
    const float kp = S(0, R_KP) / a.n_kp + (two ? S(1, R_KP) / a.n_kp : 0.f);
    const float vp = S(0, R_VP) / a.n_vp + (two ? S(1, R_VP) / a.n_vp : 0.f);
    const float pose = S(0, R_POSE) / a.n_pose;
    const float betas = two ? (S(0, R_BET) / a.n_beta + S(1, R_BET) / a.n_beta) + S(0, R_BETC) / a.n_beta : S(0, R_BET) / a.n_beta;
    const float depth = S(0, R_DEPTH) / a.n_depth + (two ? S(1, R_DEPTH) / a.n_depth : 0.f);
    float loss = a.w[W_KP] * kp;
    loss += a.w[W_BETA] * betas;
    loss += a.w[W_VPOSER] * vp;
    loss += a.w[W_POSE] * pose;
    loss += depth;
    loss *= a.w[W_SCALE];
    a.terms[0] = loss, a.terms[1] = vp, a.terms[2] = pose, a.terms[3] = kp, a.terms[4] = betas, a.terms[5] = depth;
}

__global__ void __launch_bounds__(LT) real_pack_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                                       const float* __restrict__ W2, const float* __restrict__ b2,
                                                       float* __restrict__ out) {
    const int i = (int)(blockIdx.x * LT + threadIdx.x);
    if (i >= P_FLOATS) return;
    float x;
    if (i < P_B1) {
        const int j = i / NH, k = i % NH;
        x = W1[k * NIN + j];
    } else if (i < P_W1B) {
        x = b1[i - P_B1];
    } else if (i < P_W2F) {
        const int k = (i - P_W1B) / 64, j = (i - P_W1B) % 64;
        x = j < NIN ? W1[k * NIN + j] : 0.f;
    } else if (i < P_B2) {
        const int k = (i - P_W2F) / NO, o = (i - P_W2F) % NO;
        x = W2[o * NH + k];
    } else if (i < P_W2B) {
        x = b2[i - P_B2];
    } else {
        x = W2[i - P_W2B];
    }
    out[i] = x;
}

struct Range { const char* lo; const char* hi; };
inline Range range_of(const void* p, long long floats) { return {(const char*)p, (const char*)p + floats * 4}; }
inline bool overlaps(Range a, Range b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

int64_t apg_real_loss_workspace_bytes(int B) {
    if (B < 1 || B > (1 << 30)) return -1;
    const long long floats = 2LL * B * R_COUNT;
    return (int64_t)((floats * 4 + 255) / 256 * 256);
}

int64_t apg_real_loss_encoder_bytes(void) { return (int64_t)P_FLOATS * 4; }

int apg_real_loss_pack_encoder(const float* W1, const float* b1, const float* W2, const float* b2, void* packed, int64_t bytes,
                               void* stream) {
    if (!W1) return apg_fail(APG_EINVAL, "apg_real_loss_pack_encoder: W1 is NULL");
    if (!b1) return apg_fail(APG_EINVAL, "apg_real_loss_pack_encoder: b1 is NULL");
    if (!W2) return apg_fail(APG_EINVAL, "apg_real_loss_pack_encoder: W2 is NULL");
    if (!b2) return apg_fail(APG_EINVAL, "apg_real_loss_pack_encoder: b2 is NULL");
    if (!packed) return apg_fail(APG_EINVAL, "apg_real_loss_pack_encoder: packed is NULL");
    if (bytes < apg_real_loss_encoder_bytes())
        return apg_fail(APG_ENOMEM, "apg_real_loss_pack_encoder: packed of " + std::to_string(bytes) + " bytes, " +
                                        std::to_string(apg_real_loss_encoder_bytes()) + " needed");
    hipLaunchKernelGGL(real_pack_kernel, dim3((P_FLOATS + LT - 1) / LT), dim3(LT), 0, (hipStream_t)stream, W1, b1, W2, b2, (float*)packed);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_real_loss_fwd_bwd(int nviews, int cross, int B, int J, int Jg, int depth_col, float depth_gain, const float* weights,
                          const void* encoder, const void* const* pred, const void* const* gt, float* terms, void* const* grads,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    const std::string me = "apg_real_loss_fwd_bwd: ";
    if (nviews != 1 && nviews != 2) return apg_fail(APG_EINVAL, me + "nviews must be 1 or 2");
    if (cross & ~(APG_LOSS_CROSS_POSE | APG_LOSS_CROSS_BETAS)) return apg_fail(APG_EINVAL, me + "cross has bits other than POSE | BETAS");
    if (cross && nviews == 1) return apg_fail(APG_EINVAL, me + "cross-view terms need two views (nviews = 1)");
    if (B < 1) return apg_fail(APG_EINVAL, me + "B must be >= 1");
    if (J < NJ) return apg_fail(APG_EINVAL, me + "the loss reads joints 0 .. 21, J must be >= 22");
    if (Jg < NJ) return apg_fail(APG_EINVAL, me + "the loss reads joints 0 .. 21, Jg must be >= 22");
    if (depth_col < 0 || depth_col > 2) return apg_fail(APG_EINVAL, me + "depth_col must be 0, 1 or 2");
    if (!weights) return apg_fail(APG_EINVAL, me + "weights is NULL");
    if (!encoder) return apg_fail(APG_EINVAL, me + "encoder is NULL");
    if (!pred) return apg_fail(APG_EINVAL, me + "pred is NULL");
    if (!gt) return apg_fail(APG_EINVAL, me + "gt is NULL");
    if (!terms) return apg_fail(APG_EINVAL, me + "terms is NULL");
    if (!workspace) return apg_fail(APG_EINVAL, me + "workspace is NULL");
    const int64_t need = apg_real_loss_workspace_bytes(B);
    if (need < 0) return apg_fail(APG_EINVAL, me + "B is too large");

    RealArgs a = {};
    a.nviews = nviews, a.cross = cross, a.B = B, a.J = J, a.Jg = Jg, a.col = depth_col, a.gain = depth_gain;
    a.enc = (const float*)encoder;
    static const char* const pname[APG_REAL_LOSS_PER_VIEW] = {"rotmat", "betas", "j2d", "depth"};
    const long long pn[APG_REAL_LOSS_PER_VIEW] = {(long long)B * NJ * 9, (long long)B * 10, (long long)B * J * 2, (long long)B * 3};
    Range in[1 + 2 * (APG_REAL_LOSS_PER_VIEW + 2)], out[2 + 2 * APG_REAL_LOSS_PER_VIEW];
    const char* out_name[2 + 2 * APG_REAL_LOSS_PER_VIEW];
    int nin = 0, nout = 0;
    in[nin++] = range_of(encoder, P_FLOATS);
    out[nout] = range_of(terms, APG_REAL_LOSS_NTERMS), out_name[nout++] = "terms";
    out[nout] = {(const char*)workspace, (const char*)workspace + need}, out_name[nout++] = "workspace";
    for (int v = 0; v < nviews; ++v) {
        const float* const* p = (const float* const*)pred + v * APG_REAL_LOSS_PER_VIEW;
        for (int k = 0; k < APG_REAL_LOSS_PER_VIEW; ++k) {
            if (!p[k]) return apg_fail(APG_EINVAL, me + pname[k] + " of view " + std::to_string(v) + " is NULL");
            in[nin++] = range_of(p[k], pn[k]);
        }
        a.rotmat[v] = p[0], a.betas[v] = p[1], a.j2d[v] = p[2], a.depth[v] = p[3];
        const float* const* g = (const float* const*)gt + v * 2;
        if (!g[0]) return apg_fail(APG_EINVAL, me + "gt of view " + std::to_string(v) + " is NULL");
        if (!g[1]) return apg_fail(APG_EINVAL, me + "eps of view " + std::to_string(v) + " is NULL");
        a.gt[v] = g[0], a.eps[v] = g[1];
        in[nin++] = range_of(g[0], (long long)B * Jg * 3);
        in[nin++] = range_of(g[1], (long long)B * NZ);
        if (grads) {
            float* const* q = (float* const*)grads + v * APG_REAL_LOSS_PER_VIEW;
            a.g_rotmat[v] = q[0], a.g_betas[v] = q[1], a.g_j2d[v] = q[2], a.g_depth[v] = q[3];
            for (int k = 0; k < APG_REAL_LOSS_PER_VIEW; ++k)
                if (q[k]) out[nout] = range_of(q[k], pn[k]), out_name[nout++] = pname[k];
        }
    }
    if (workspace_bytes < need)
        return apg_fail(APG_ENOMEM, me + "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed");
    for (int o = 0; o < nout; ++o)
        for (int i = 0; i < nin; ++i)
            if (overlaps(out[o], in[i]))
                return apg_fail(APG_EINVAL, me + "the output " + out_name[o] + (o >= 2 ? " (a gradient)" : "") + " overlaps an input");

    const double sc = weights[W_SCALE], Bd = B;
    const double n_kp = Bd * NJ * 2, n_vp = Bd * NZ, n_pose = Bd * NR * 9, n_beta = Bd * 10, n_depth = Bd;
    a.c_kp = (float)(sc * weights[W_KP] * 2.0 / n_kp);
    a.c_vp = (float)(sc * weights[W_VPOSER] * 2.0 / n_vp);
    a.c_pose = (float)(sc * weights[W_POSE] * 2.0 / n_pose);
    a.c_beta = (float)(sc * weights[W_BETA] * 2.0 / n_beta);
    a.c_depth = (float)(sc * -2.0 * (double)depth_gain / n_depth);
    a.limbs2d = weights[W_LIMBS2D];
    a.part = (float*)workspace;

    RealCombineArgs c = {};
    c.nviews = nviews, c.cross = cross, c.B = B, c.part = a.part;
    for (int k = 0; k < W_COUNT; ++k) c.w[k] = weights[k];
    c.n_kp = (float)n_kp, c.n_vp = (float)n_vp, c.n_pose = (float)n_pose, c.n_beta = (float)n_beta, c.n_depth = (float)n_depth;
    c.terms = terms;

    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(real_main_kernel, dim3((unsigned)(nviews * B)), dim3(LT), 0, st, a);
    APG_TRY(hipGetLastError());
    hipLaunchKernelGGL(real_combine_kernel, dim3(1), dim3(LT), 0, st, c);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // extern "C"
