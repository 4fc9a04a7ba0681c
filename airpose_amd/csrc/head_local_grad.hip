// Generic view-local regressor head for gfx950 (libairpose_grad.so): ONE weight set over R rows with the layout given by the
// caller.  It serves copenet.regressor_step (and copenet_sep, which is built from it), model_hmr, model_muhmr and
// model_copenet_singleview:
//   xc = [xf (2048) | segment 0 | ... | segment nseg-1]            K1 = 2048 + S columns, S = sum of the segment widths
//   h1d = drop1(xc W1^T + b1), h2d = drop2(h1d W2^T + b2)
//   out_d = xc[:, 2048 + res_d : 2048 + res_d + n_d] + h2d W_d^T + b_d        for each of the ndec decoders
// The network itself -- fc1, drop1, fc2, drop2 and the backward chain through them -- is head_mlp.hip's, shared with the two-view
// head (head_grad.hip); here is what the caller-given layout needs:
//   forward:  head_local_pack_kernel (xc, a snapshot of the inputs, and wdec = [W_0; W_1; W_2 | b_0; b_1; b_2] in one launch),
//             apg_head_hidden_fwd, then ALL decoders as one product of N = sum n_d columns on apg_gemm_kernel whose epilogue
//             (APG_EPI_DEC_LOCAL) adds bias and residual and writes every decoder's own output
//   backward: head_local_pack_gd_kernel (g_delta, R x N, from the per-decoder output gradients), apg_head_chain_bwd (parameter
//             gradients and g_xc: segment columns, + features on request); head_local_scatter_kernel adds the residual identity
//             and writes the per-segment gradients; a broadcast (stride-0) segment's rows go to the workspace and are summed by
//             the column sums' two fixed-order passes.
// Every product reduces over K in index order inside one workgroup, no float atomics anywhere: results are bit-reproducible and
// a row's outputs and input gradients depend only on that row.  Rows are numbered [0, R) for the dropout hash.
#include "ap_common.h"
#include "grad_internal.h"

#include <string>

namespace {

constexpr int MAX_SEG = APG_HEAD_LOCAL_MAX_SEG, MAX_DEC = APG_HEAD_LOCAL_MAX_DEC;

struct Segs {
    const float* p[MAX_SEG];
    int ld[MAX_SEG];
    int off[MAX_SEG + 1];                // first column of the segment inside the S segment columns; off[nseg] = S
    int nseg;
};

struct Decs {
    const float* W[MAX_DEC];
    const float* b[MAX_DEC];
    int off[MAX_DEC + 1];                // first packed column; off[ndec] = N
    int res[MAX_DEC];
    int ndec;
};

// blocks [0, R * cb): xc[r][c], cb = ceil(K1 / 256) blocks per row; the blocks behind them: wdec (N x 1024 weights, then N biases)
__global__ void __launch_bounds__(256) head_local_pack_kernel(const float* __restrict__ xf, const Segs s, const Decs d, int R, int K1,
                                                              int cb, float* __restrict__ xc, float* __restrict__ wdec) {
    const long long blk = blockIdx.x;
    if (blk < (long long)R * cb) {
        const int r = (int)(blk / cb), c = (int)(blk % cb) * 256 + threadIdx.x;
        if (c >= K1) return;
        float val;
        if (c < XF) {
            val = xf[(long long)r * XF + c];
        } else {
            const int sc = c - XF;
            int k = 0;
            while (k + 1 < s.nseg && sc >= s.off[k + 1]) ++k;
            val = s.p[k][(long long)r * s.ld[k] + sc - s.off[k]];
        }
        xc[(long long)r * K1 + c] = val;
        return;
    }
    const int N = d.off[d.ndec];
    const long long idx = (blk - (long long)R * cb) * 256 + threadIdx.x;
    if (idx >= (long long)N * (HID + 1)) return;
    if (idx < (long long)N * HID) {
        const int n = (int)(idx / HID), k = (int)(idx % HID);
        int e = 0;
        while (e + 1 < d.ndec && n >= d.off[e + 1]) ++e;
        wdec[idx] = d.W[e][(long long)(n - d.off[e]) * HID + k];
    } else {
        const int n = (int)(idx - (long long)N * HID);
        int e = 0;
        while (e + 1 < d.ndec && n >= d.off[e + 1]) ++e;
        wdec[idx] = d.b[e][n - d.off[e]];
    }
}

struct GOut {
    const float* g[MAX_DEC];             // NULL = zero
    int off[MAX_DEC + 1];
    int res[MAX_DEC];
    int ndec;
};

// g_delta[r][n] (R x N) from the per-decoder output gradients
__global__ void __launch_bounds__(256) head_local_pack_gd_kernel(const GOut go, int R, float* __restrict__ gd) {
    const int N = go.off[go.ndec];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)R * N) return;
    const int r = (int)(idx / N), n = (int)(idx % N);
    int e = 0;
    while (e + 1 < go.ndec && n >= go.off[e + 1]) ++e;
    const int nd = go.off[e + 1] - go.off[e];
    gd[idx] = go.g[e] ? go.g[e][(long long)r * nd + n - go.off[e]] : 0.f;
}

struct GSeg {
    float* g[MAX_SEG];                   // per segment: the caller's (R x width), or for a broadcast segment the workspace (R x S, at the
    int ld[MAX_SEG];                     // segment's column); NULL = not needed
    int off[MAX_SEG + 1];
    int nseg;
};

// gradient of segment column sc of row r: its fc1 column + the output gradient of every decoder whose residual range holds it, in
// decoder order.  gxc holds columns [c0, K1) of g_xc, row pitch ldg.  The feature columns go to gxf (when asked for).
__global__ void __launch_bounds__(256) head_local_scatter_kernel(const float* __restrict__ gxc, int ldg, int c0, int K1,
                                                                 float* __restrict__ gxf, const GSeg gs, const GOut go) {
    const int r = blockIdx.x, c = c0 + blockIdx.y * 256 + threadIdx.x;
    if (c >= K1) return;
    const long long own = (long long)r * ldg - c0;
    if (c < XF) {
        if (gxf) gxf[(long long)r * XF + c] = gxc[own + c];
        return;
    }
    const int sc = c - XF;
    int k = 0;
    while (k + 1 < gs.nseg && sc >= gs.off[k + 1]) ++k;
    float* o = gs.g[k];
    if (!o) return;
    float val = gxc[own + c];
    for (int e = 0; e < go.ndec; ++e) {
        const int j = sc - go.res[e];
        if (go.g[e] && j >= 0 && j < go.off[e + 1] - go.off[e]) val += go.g[e][(long long)r * (go.off[e + 1] - go.off[e]) + j];
    }
    o[(long long)r * gs.ld[k] + sc - gs.off[k]] = val;
}

// workspace of apg_head_local_bwd, in floats: the chain's pieces, then the per-row gradients of the broadcast segments (R x S)
size_t bwd_floats(const ApgChainLayout& l, int R, int K1) { return l.total + al64((size_t)R * (K1 - XF)); }

// the shared checks of the layout: -> "" or what is wrong; fills off / N / S
std::string check_layout(int R, int nseg, const int* seg_w, int ndec, const int* dec_n, const int* dec_res, int* seg_off, int* dec_off) {
    if (R < 1) return "R < 1";
    if (nseg < 1 || nseg > MAX_SEG) return "1 .. " + std::to_string(MAX_SEG) + " segments, got " + std::to_string(nseg);
    if (ndec < 1 || ndec > MAX_DEC) return "1 .. " + std::to_string(MAX_DEC) + " decoders, got " + std::to_string(ndec);
    if (!seg_w || !dec_n || !dec_res) return "a layout array is NULL";
    seg_off[0] = 0;
    for (int k = 0; k < nseg; ++k) {
        if (seg_w[k] < 1 || seg_w[k] > HID) return "segment " + std::to_string(k) + ": width outside 1 .. 1024";
        seg_off[k + 1] = seg_off[k] + seg_w[k];
    }
    dec_off[0] = 0;
    for (int e = 0; e < ndec; ++e) {
        if (dec_n[e] < 1 || dec_n[e] > HID) return "decoder " + std::to_string(e) + ": width outside 1 .. 1024";
        if (dec_res[e] < 0 || dec_res[e] + dec_n[e] > seg_off[nseg])
            return "decoder " + std::to_string(e) + ": residual columns [" + std::to_string(dec_res[e]) + ", " +
                   std::to_string(dec_res[e] + dec_n[e]) + ") outside the " + std::to_string(seg_off[nseg]) + " segment columns";
        dec_off[e + 1] = dec_off[e] + dec_n[e];
    }
    return "";
}

}  // namespace

extern "C" {

int apg_head_local_fwd(int R, const float* xf, int nseg, const void* const* seg, const int* seg_ld, const int* seg_w,
                       const float* W1, const float* b1, const float* W2, const float* b2, int ndec, const void* const* dec_W,
                       const void* const* dec_b, const int* dec_n, const int* dec_res, uint64_t seed, float p1, float p2,
                       float* xc, float* h1d, float* h2d, float* wdec, void* const* out, void* stream) {
    Segs s = {};
    Decs d = {};
    const std::string bad = check_layout(R, nseg, seg_w, ndec, dec_n, dec_res, s.off, d.off);
    if (!bad.empty()) return apg_fail(APG_EINVAL, "apg_head_local_fwd: " + bad);
    if (!xf || !seg || !seg_ld || !W1 || !b1 || !W2 || !b2 || !dec_W || !dec_b || !xc || !h1d || !h2d || !wdec || !out)
        return apg_fail(APG_EINVAL, "apg_head_local_fwd: bad argument");
    s.nseg = nseg;
    for (int k = 0; k < nseg; ++k) {
        s.p[k] = (const float*)seg[k];
        s.ld[k] = seg_ld[k];
        if (!s.p[k] || (s.ld[k] != 0 && s.ld[k] < seg_w[k])) return apg_fail(APG_EINVAL, "apg_head_local_fwd: segment input missing or row stride below its width");
    }
    d.ndec = ndec;
    for (int e = 0; e < ndec; ++e) {
        d.W[e] = (const float*)dec_W[e];
        d.b[e] = (const float*)dec_b[e];
        d.res[e] = dec_res[e];
        if (!d.W[e] || !d.b[e] || !out[e]) return apg_fail(APG_EINVAL, "apg_head_local_fwd: decoder weight, bias or output missing");
    }
    hipStream_t st = (hipStream_t)stream;
    const int K1 = XF + s.off[nseg], N = d.off[ndec];
    const int cb = (K1 + 255) / 256;
    const long long blocks = (long long)R * cb + ((long long)N * (HID + 1) + 255) / 256;
    if (blocks > 0x7fffffffLL) return apg_fail(APG_EINVAL, "apg_head_local_fwd: too many rows");
    hipLaunchKernelGGL(head_local_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, xf, s, d, R, K1, cb, xc, wdec);
    APG_TRY(hipGetLastError());
    if (int rc = apg_head_hidden_fwd(R, K1, xc, W1, b1, W2, b2, seed, p1, p2, h1d, h2d, st)) return rc;
    ApgGemmArgs g = apg_gemm_args(h2d, HID, 1, wdec, 1, HID, R, N, HID);         // every decoder: delta = h2d wdec^T
    g.epi = APG_EPI_DEC_LOCAL;
    g.bias = wdec + (size_t)N * HID;
    g.base = xc + XF;
    g.ldbase = K1;
    g.ndec = ndec;
    for (int e = 0; e < ndec; ++e) {
        g.doff[e] = d.off[e];
        g.dres[e] = d.res[e];
        g.dout[e] = (float*)out[e];
    }
    g.doff[ndec] = N;
    APG_TRY(apg_gemm_launch(g, st));
    return APG_OK;
}

int64_t apg_head_local_bwd_workspace_bytes(int R, int K1, int N, int need_gxf) {
    if (R < 1 || K1 <= XF || K1 > XF + MAX_SEG * HID || N < 1 || N > MAX_DEC * HID) return -1;
    return (int64_t)(bwd_floats(apg_chain_layout(R, K1, N, need_gxf), R, K1) * sizeof(float));
}

int apg_head_local_bwd(int R, int nseg, const int* seg_w, const int* seg_bcast, int ndec, const int* dec_n, const int* dec_res,
                       const float* xc, const float* h1d, const float* h2d, const float* wdec, const float* W1, const float* W2,
                       uint64_t seed, float p1, float p2, const void* const* g_out, void* const* g_param, float* g_xf,
                       void* const* g_seg, void* workspace, int64_t workspace_bytes, void* stream) {
    GSeg gs = {};
    GOut go = {};
    const std::string bad = check_layout(R, nseg, seg_w, ndec, dec_n, dec_res, gs.off, go.off);
    if (!bad.empty()) return apg_fail(APG_EINVAL, "apg_head_local_bwd: " + bad);
    if (!seg_bcast || !xc || !h1d || !h2d || !wdec || !W1 || !W2 || !g_out || !g_param || !g_seg || !workspace)
        return apg_fail(APG_EINVAL, "apg_head_local_bwd: bad argument");
    const int S = gs.off[nseg], K1 = XF + S, N = go.off[ndec];
    const int need_gxf = g_xf != nullptr;
    const ApgChainLayout l = apg_chain_layout(R, K1, N, need_gxf);
    if (workspace_bytes < (int64_t)(bwd_floats(l, R, K1) * sizeof(float)))
        return apg_fail(APG_ENOMEM, "apg_head_local_bwd: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(bwd_floats(l, R, K1) * sizeof(float)) + " needed");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float *gd = ws + l.gd, *gxc = ws + l.gxc, *part = ws + l.part, *gseg = ws + l.total;
    go.ndec = ndec;
    for (int e = 0; e < ndec; ++e) {
        go.g[e] = (const float*)g_out[e];
        go.res[e] = dec_res[e];
    }
    const long long ngd = (long long)R * N;
    hipLaunchKernelGGL(head_local_pack_gd_kernel, dim3((unsigned)((ngd + 255) / 256)), dim3(256), 0, st, go, R, gd);
    APG_TRY(hipGetLastError());
    bool any_in = need_gxf;
    gs.nseg = nseg;
    for (int k = 0; k < nseg; ++k) {
        if (!g_seg[k]) continue;
        any_in = true;
        if (seg_bcast[k]) { gs.g[k] = gseg + gs.off[k]; gs.ld[k] = S; }          // per-row values, summed below
        else { gs.g[k] = (float*)g_seg[k]; gs.ld[k] = seg_w[k]; }
    }
    const ApgChainBwd c = {R, K1, N, ndec, go.off, xc, h1d, h2d, wdec, W1, W2, seed, p1, p2, g_param, any_in};
    if (int rc = apg_head_chain_bwd(c, l, ws, st)) return rc;
    if (any_in) {
        const int nc = K1 - l.c0;
        hipLaunchKernelGGL(head_local_scatter_kernel, dim3(R, (nc + 255) / 256), dim3(256), 0, st, gxc, nc, l.c0, K1, g_xf, gs, go);
        APG_TRY(hipGetLastError());
        for (int k = 0; k < nseg; ++k)
            if (g_seg[k] && seg_bcast[k]) APG_TRY(apg_colsum(gseg + gs.off[k], R, seg_w[k], S, part, (float*)g_seg[k], st));
    }
    return APG_OK;
}

}  // extern "C"
