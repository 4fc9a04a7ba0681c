// IEF regressor head forward / backward for gfx950 (libairpose_grad.so): copenet.forward_reg on live fp32 weights, both views in
// one pass of R = 2B rows, and its adjoint.  The network itself -- fc1, drop1, fc2, drop2 and the backward chain through them -- is
// head_mlp.hip's, shared with the generic head (head_local_grad.hip); here is what the two-view layout needs:
//   forward:  head_pack_kernel (the fc1 input xc: features | state | partner's art and shape, a snapshot kept for backward),
//             apg_head_hidden_fwd, then decpose and decshape, one apg_gemm_args product each (APG_EPI_DEC_FWD: + bias and the
//             residual, written straight into the per-view outputs)
//   backward: head_pack_gd_kernel (g_delta from the per-view output gradients), head_pack_wdec_kernel ([Wpose; Wshape]),
//             apg_head_chain_bwd (parameter gradients and g_xc: state columns, + features on request), then
//             head_scatter_kernel adds own columns + partner's fusion columns + residual identity into the input gradients.
#include "ap_common.h"
#include "grad_internal.h"

#include <string>

namespace {

constexpr int XC = 2332;                 // fc1 input width
constexpr int NPOSE = 135, NSHAPE = 10, NDEC = NPOSE + NSHAPE;

// state inputs of one view: bb, pos, orient, art, shape (column offsets inside the 284 state columns)
__constant__ const int k_st_off[5] = {0, 3, 6, 12, 138};
__constant__ const int k_st_w[5] = {3, 3, 6, 126, 10};

struct StatePtrs {
    const float* p[2][5];
    int ld[2][5];
};

// xc[r] = [xf_v[b] | bb | pos | orient | art | shape | partner art | partner shape], r = v * B + b
__global__ void __launch_bounds__(256) head_pack_kernel(const float* __restrict__ xf0, const float* __restrict__ xf1,
                                                        const StatePtrs s, int B, float* __restrict__ xc) {
    const int r = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= XC) return;
    const int v = r >= B, b = r - v * B;
    float val;
    if (c < XF) {
        val = (v ? xf1 : xf0)[(long long)b * XF + c];
    } else {
        int sc = c - XF, src = v, idx;
        if (sc >= 274) { src = 1 - v; idx = 4; sc -= 274; }
        else if (sc >= 148) { src = 1 - v; idx = 3; sc -= 148; }
        else { idx = 0; while (idx < 4 && sc >= k_st_off[idx + 1]) ++idx; sc -= k_st_off[idx]; }
        val = s.p[src][idx][(long long)b * s.ld[src][idx] + sc];
    }
    xc[(long long)r * XC + c] = val;
}

// g_delta[r][n] (R x 145) from the per-view output gradients (NULL = zero)
__global__ void __launch_bounds__(256) head_pack_gd_kernel(const float* __restrict__ gp0, const float* __restrict__ gs0,
                                                           const float* __restrict__ gp1, const float* __restrict__ gs1, int B,
                                                           float* __restrict__ gd) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2LL * B * NDEC) return;
    const int r = (int)(idx / NDEC), n = (int)(idx % NDEC);
    const int v = r >= B, b = r - v * B;
    const float* src = n < NPOSE ? (v ? gp1 : gp0) : (v ? gs1 : gs0);
    gd[idx] = src ? (n < NPOSE ? src[(long long)b * NPOSE + n] : src[(long long)b * NSHAPE + n - NPOSE]) : 0.f;
}

__global__ void __launch_bounds__(256) head_pack_wdec_kernel(const float* __restrict__ wp, const float* __restrict__ ws,
                                                             float* __restrict__ wdec) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= NDEC * HID) return;
    wdec[idx] = idx < NPOSE * HID ? wp[idx] : ws[idx - NPOSE * HID];
}

struct GradIn {
    float* g[2][6];                      // xf, bb, pos, orient, art, shape per view
    const float* gpose[2];
    const float* gbetas[2];
};

// input gradients of state column / feature c of row r: own column + (art, shape) the partner row's fusion column + residual.
// gxc holds columns [c0, 2332) of g_xc, row pitch ldg.
__global__ void __launch_bounds__(256) head_scatter_kernel(const float* __restrict__ gxc, int ldg, int c0, int B, const GradIn gi) {
    const int r = blockIdx.x, c = c0 + blockIdx.y * 256 + threadIdx.x;
    if (c >= XF + 148) return;                           // partner columns are gathered by the partner's own row
    const int v = r >= B, b = r - v * B, rp = (1 - v) * B + b;
    const long long own = (long long)r * ldg - c0, par = (long long)rp * ldg - c0;     // + column index >= c0
    if (c < XF) {
        float* o = gi.g[v][0];
        if (o) o[(long long)b * XF + c] = gxc[own + c];
        return;
    }
    const int sc = c - XF;
    int idx = 0;
    while (idx < 4 && sc >= k_st_off[idx + 1]) ++idx;
    float* o = gi.g[v][idx + 1];
    if (!o) return;
    const int j = sc - k_st_off[idx];
    float val = gxc[own + c];
    if (idx == 3) val += gxc[par + XF + 148 + j];
    if (idx == 4) val += gxc[par + XF + 274 + j];
    if (idx >= 1 && idx <= 3 && gi.gpose[v]) val += gi.gpose[v][(long long)b * NPOSE + sc - 3];
    if (idx == 4 && gi.gbetas[v]) val += gi.gbetas[v][(long long)b * NSHAPE + j];
    o[(long long)b * k_st_w[idx] + j] = val;
}

// workspace of apg_head_bwd, in floats: the chain's pieces, then wdec
size_t bwd_floats(const ApgChainLayout& l) { return l.total + al64((size_t)NDEC * HID); }

}  // namespace

extern "C" {

int apg_head_fwd(int B, const float* xf0, const float* xf1, const void* const* state, const int* state_ld,
                 const float* W1, const float* b1, const float* W2, const float* b2, const float* Wpose, const float* bpose,
                 const float* Wshape, const float* bshape, uint64_t seed, float p1, float p2,
                 float* xc, float* h1d, float* h2d, void* const* pose_out, void* const* betas_out, void* stream) {
    if (B <= 0 || !xf0 || !xf1 || !state || !state_ld || !W1 || !b1 || !W2 || !b2 || !Wpose || !bpose || !Wshape || !bshape ||
        !xc || !h1d || !h2d || !pose_out || !betas_out || !pose_out[0] || !pose_out[1] || !betas_out[0] || !betas_out[1])
        return apg_fail(APG_EINVAL, "apg_head_fwd: bad argument");
    StatePtrs s;
    for (int v = 0; v < 2; ++v)
        for (int k = 0; k < 5; ++k) {
            s.p[v][k] = (const float*)state[v * 5 + k];
            s.ld[v][k] = state_ld[v * 5 + k];
            if (!s.p[v][k] || s.ld[v][k] < 0) return apg_fail(APG_EINVAL, "apg_head_fwd: state input missing");
        }
    hipStream_t st = (hipStream_t)stream;
    const int R = 2 * B;
    hipLaunchKernelGGL(head_pack_kernel, dim3(R, (XC + 255) / 256), dim3(256), 0, st, xf0, xf1, s, B, xc);
    APG_TRY(hipGetLastError());
    if (int rc = apg_head_hidden_fwd(R, XC, xc, W1, b1, W2, b2, seed, p1, p2, h1d, h2d, st)) return rc;
    for (int part = 0; part < 2; ++part) {                               // pose = [pos|orient|art] + dec; betas = shape + dec
        ApgGemmArgs g = apg_gemm_args(h2d, HID, 1, part ? Wshape : Wpose, 1, HID, R, part ? NSHAPE : NPOSE, HID);
        g.epi = APG_EPI_DEC_FWD;
        g.bias = part ? bshape : bpose;
        g.nb = B;
        g.out0 = (float*)(part ? betas_out : pose_out)[0];
        g.out1 = (float*)(part ? betas_out : pose_out)[1];
        g.ldo = part ? NSHAPE : NPOSE;
        g.base = xc + XF + (part ? 138 : 3);
        g.ldbase = XC;
        APG_TRY(apg_gemm_launch(g, st));
    }
    return APG_OK;
}

int64_t apg_head_bwd_workspace_bytes(int B, int need_gxf) {
    if (B <= 0) return -1;
    return (int64_t)(bwd_floats(apg_chain_layout(2 * (size_t)B, XC, NDEC, need_gxf)) * sizeof(float));
}

int apg_head_bwd(int B, const float* xc, const float* h1d, const float* h2d, const float* W1, const float* W2,
                 const float* Wpose, const float* Wshape, uint64_t seed, float p1, float p2, const void* const* g_out,
                 void* const* g_param, void* const* g_in, void* workspace, int64_t workspace_bytes, void* stream) {
    if (B <= 0 || !xc || !h1d || !h2d || !W1 || !W2 || !Wpose || !Wshape || !g_out || !g_param || !g_in || !workspace)
        return apg_fail(APG_EINVAL, "apg_head_bwd: bad argument");
    const int need_gxf = g_in[0] || g_in[6];
    const int R = 2 * B;
    const ApgChainLayout l = apg_chain_layout(R, XC, NDEC, need_gxf);
    if (workspace_bytes < (int64_t)(bwd_floats(l) * sizeof(float)))
        return apg_fail(APG_ENOMEM, "apg_head_bwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(bwd_floats(l) * sizeof(float)) + " needed");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float *gd = ws + l.gd, *gxc = ws + l.gxc, *wdec = ws + l.total;

    const long long ngd = (long long)R * NDEC;
    hipLaunchKernelGGL(head_pack_gd_kernel, dim3((unsigned)((ngd + 255) / 256)), dim3(256), 0, st, (const float*)g_out[0],
                       (const float*)g_out[1], (const float*)g_out[2], (const float*)g_out[3], B, gd);
    hipLaunchKernelGGL(head_pack_wdec_kernel, dim3((NDEC * HID + 255) / 256), dim3(256), 0, st, Wpose, Wshape, wdec);
    APG_TRY(hipGetLastError());
    bool any_in = false;
    for (int k = 0; k < 12; ++k) any_in = any_in || g_in[k];
    const int doff[3] = {0, NPOSE, NDEC};
    const ApgChainBwd c = {R, XC, NDEC, 2, doff, xc, h1d, h2d, wdec, W1, W2, seed, p1, p2, g_param, any_in};
    if (int rc = apg_head_chain_bwd(c, l, ws, st)) return rc;
    if (any_in) {
        GradIn gi;
        for (int v = 0; v < 2; ++v) {
            for (int k = 0; k < 6; ++k) gi.g[v][k] = (float*)g_in[v * 6 + k];
            gi.gpose[v] = (const float*)g_out[2 * v];
            gi.gbetas[v] = (const float*)g_out[2 * v + 1];
        }
        hipLaunchKernelGGL(head_scatter_kernel, dim3(R, (XF + 148 - l.c0 + 255) / 256), dim3(256), 0, st, gxc, XC - l.c0, l.c0, B, gi);
        APG_TRY(hipGetLastError());
    }
    return APG_OK;
}

}  // extern "C"
