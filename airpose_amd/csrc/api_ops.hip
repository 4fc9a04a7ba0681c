// The launch functions of the trunk kernels (ap_internal::launch_*, declared in api_internal.h): each fills ONE kernel's argument
// struct and calls its launcher, for the trunk pass (api_trunk.hip) and for the stand-alone operator entry alike.  Below them
// the operator entry points: every kernel a trunk pass can launch on caller-owned tensors -- validate the arguments, then the
// shared launch (the element-wise tests go through these; the forms a pass selects with y_tiled, x2, pool_out and PairLayout have
// entries of their own: ap_conv2d_tiled_nhwc, _fold_nhwc, _pool_nhwc, ap_conv_pair_layout_nhwc) -- and the geometry operators.
#include "api_internal.h"

namespace {
const char g_any = 0;   // the shape predicates only ask that an operand exists
// the generic kernels' argument struct from plain shapes and pointers (x2: second K segment of c.cin2 channels, or NULL)
ConvArgs conv_args(const ConvDesc& c, const void* x, int N, int H, int W, const void* res, void* y, int relu, int y_tiled, const void* x2,
                   int H2, int* rflag) {
    ConvArgs a{};
    a.x = x; a.w = c.w; a.scale = c.scale; a.shift = c.shift; a.res = res; a.y = y;
    a.N = N; a.H = H; a.W = W; a.Cin = c.cin; a.Cout = c.cout;
    a.Ho = (H + 2 * c.pad - c.k) / c.stride + 1;
    a.Wo = (W + 2 * c.pad - c.k) / c.stride + 1;
    a.KH = a.KW = c.k; a.stride = c.stride; a.pad = c.pad;
    a.M = N * a.Ho * a.Wo;
    a.ldx = c.cin; a.ldy = c.cout; a.ldr = c.cout; a.wld = c.wld;
    a.relu = relu; a.y_tiled = y_tiled; a.range_flag = rflag;
    if (x2) { a.x2 = x2; a.H2 = a.W2 = H2; a.Cin2 = a.ldx2 = c.cin2; a.stride2 = c.stride2; }
    return a;
}
}  // namespace

hipError_t ap_internal::launch_conv(const ConvDesc& c, const void* x, int N, int H, int W, const void* res, void* y, int relu, int y_tiled,
                                    const void* x2, int H2, float* pool_out, bool* pooled, int prec, int mode, int* rflag, hipStream_t st) {
    ConvArgs a = conv_args(c, x, N, H, W, res, y, relu, y_tiled, x2, H2, rflag);
    if (pool_out && k_bf16::ap_conv_lean_supported(a, prec_kind(prec))) {
        a.y = nullptr; a.pool_out = pool_out; a.dbg = g_conv_dbg;
        hipError_t e = ap_zero_line(&a.zero);
        if (e != hipSuccess) return e;
        *pooled = true;
        return H16(prec, ap_launch_conv_lean)(a, st);
    }
    return dispatch_conv(a, prec, st, mode);
}
// launch_conv's own condition for the pooling branch, on the arguments it would build (7 x 7 images, identity, ReLU)
bool ap_internal::conv_pool_fits(const ConvDesc& c, int N, int prec) {
    return k_bf16::ap_conv_lean_supported(conv_args(c, &g_any, N, 7, 7, &g_any, nullptr, 1, 0, nullptr, 0, nullptr), prec_kind(prec));
}
const char* ap_internal::conv_form_refusal(const ConvDesc& c, int N, int H, int W, int y_tiled, bool fold, int H2, int prec, int mode) {
    return conv_refusal(conv_args(c, &g_any, N, H, W, nullptr, nullptr, 1, y_tiled, fold ? &g_any : nullptr, H2, nullptr), prec, mode);
}

namespace {
// conv_pw.hip's three forms
PwArgs pw_args(const ConvDesc& c, const void* x, const void* res, void* y, int M, int* rflag) {
    PwArgs p{};
    p.x = x; p.y = y; p.res = res; p.wfrag = c.w; p.scale = c.scale; p.shift = c.shift;
    p.M = M; p.Cin = c.cin; p.Cout = c.cout; p.relu = 1; p.range_flag = rflag;
    return p;
}
PwArgs pw_ds_args(const ConvDesc& c, const void* t, const void* x2, void* y, int N, int Ho, int H2, int* rflag) {
    PwArgs p = pw_args(c, t, nullptr, y, N * Ho * Ho, rflag);
    p.x2 = x2; p.Cin2 = c.cin2; p.Ho = p.Wo = Ho; p.H2 = p.W2 = H2; p.stride2 = c.stride2;
    return p;
}
PwArgs pw_k3_args(const ConvDesc& c, const void* x, void* y, int N, int H, int* rflag) {
    PwArgs p = pw_args(c, x, nullptr, y, N * (H / 2) * (H / 2), rflag);
    p.k3 = 1; p.Ho = p.Wo = H / 2; p.H2 = p.W2 = H; p.stride2 = 2;
    return p;
}
}  // namespace

hipError_t ap_internal::launch_conv_pw(const ConvDesc& c, const void* x, const void* res, void* y, int M, int prec, int* rflag, hipStream_t st) {
    return H16(prec, ap_launch_conv_pw)(pw_args(c, x, res, y, M, rflag), st);
}
bool ap_internal::conv_pw_ds_fits(const ConvDesc& c, int N, int Ho, int H2) {
    return k_bf16::ap_conv_pw_ds_supported(pw_ds_args(c, &g_any, &g_any, nullptr, N, Ho, H2, nullptr));
}
hipError_t ap_internal::launch_conv_pw_ds(const ConvDesc& c, const void* t, const void* x2, void* y, int N, int Ho, int H2, int prec,
                                          int* rflag, hipStream_t st) {
    return H16(prec, ap_launch_conv_pw)(pw_ds_args(c, t, x2, y, N, Ho, H2, rflag), st);
}
bool ap_internal::conv_pw_k3_fits(const ConvDesc& c, int N, int H) {
    return !(H & 1) && k_bf16::ap_conv_pw_k3_supported(pw_k3_args(c, &g_any, nullptr, N, H, nullptr));
}
hipError_t ap_internal::launch_conv_pw_k3(const ConvDesc& c, const void* x, void* y, int N, int H, int prec, int* rflag, hipStream_t st) {
    return H16(prec, ap_launch_conv_pw)(pw_k3_args(c, x, y, N, H, rflag), st);
}

hipError_t ap_internal::launch_bneck2(const ConvDesc& c1, const ConvDesc& c2, const ConvDesc& c3, int ds, const void* x, void* y, int N,
                                      int H, int W, const ConvDesc* c1n, void* t1n, int y_even, int prec, int* rflag, hipStream_t st) {
    BneckArgs a{};
    a.x = x; a.y = y; a.w1 = c1.w; a.w2 = c2.w; a.w3 = c3.w;
    a.s1 = c1.scale; a.h1 = c1.shift; a.s2 = c2.scale; a.h2 = c2.shift; a.s3 = c3.scale; a.h3 = c3.shift;
    a.N = N; a.H = H; a.W = W; a.range_flag = rflag; a.dbg = g_conv_dbg;
    if (c1n) { a.w1n = c1n->w; a.s1n = c1n->scale; a.h1n = c1n->shift; a.t1n = t1n; a.y_even = y_even; }
    hipError_t e = ap_zero_line(&a.zero);
    if (e != hipSuccess) return e;
    return H16(prec, ap_launch_bneck2)(a, ds, st);
}

hipError_t ap_internal::launch_block_img(const void* x, const void* wfrag, const float* s1, const float* h1, const float* s2, const float* h2,
                                         const float* s3, const float* h3, void* y, int N, int prec, int* rflag, hipStream_t st) {
    BlkImgArgs a{};
    a.x = x; a.y = y; a.wfrag = wfrag; a.s1 = s1; a.h1 = h1; a.s2 = s2; a.h2 = h2; a.s3 = s3; a.h3 = h3; a.N = N;
    a.range_flag = rflag; a.dbg = g_conv_dbg;
    return H16(prec, ap_launch_block_img)(a, st);
}

hipError_t ap_internal::launch_conv_img3(const void* x, const void* wfrag, const float* scale, const float* shift, void* y, int N, int y_tiled,
                                         int prec, int* rflag, hipStream_t st) {
    ConvImg3Args a{};
    a.x = x; a.y = y; a.wfrag = wfrag; a.scale = scale; a.shift = shift; a.N = N; a.y_tiled = y_tiled; a.range_flag = rflag;
    hipError_t e = ap_zero_line(&a.zero);
    if (e != hipSuccess) return e;
    return H16(prec, ap_launch_conv_img3)(a, st);
}

hipError_t ap_internal::launch_conv_s2p(const void* x, const void* wfrag, const float* scale, const float* shift, void* y, int N, int y_tiled,
                                        int prec, int* rflag, hipStream_t st) {
    ConvS2pArgs a{};
    a.x = x; a.y = y; a.wfrag = wfrag; a.scale = scale; a.shift = shift; a.N = N; a.y_tiled = y_tiled; a.range_flag = rflag;
    hipError_t e = ap_zero_line(&a.zero);
    if (e != hipSuccess) return e;
    return H16(prec, ap_launch_conv_s2p)(a, st);
}

hipError_t ap_internal::launch_conv_pair(const void* t2, const void* wstream, const float* s3, const float* h3, const float* s1, const float* h1,
                                         const void* in, void* out, void* t1n, int M, int Ho, int H2, int stride2, int P, int P2, int N1,
                                         PairLayout lay, int prec, int* rflag, hipStream_t st) {
    PairArgs a{};
    a.t2 = t2; a.wstream = wstream; a.s3 = s3; a.h3 = h3; a.s1 = s1; a.h1 = h1; a.out = out; a.t1n = t1n; a.M = M;
    a.Ho = a.Wo = Ho;
    if (H2) { a.x2 = in; a.H2 = a.W2 = H2; a.stride2 = stride2; }
    else a.res = in;
    a.t2_tiled = lay.t2_tiled; a.res_tiled = lay.res_tiled; a.out_tiled = lay.out_tiled; a.out_even = lay.out_even;
    a.dbg = g_conv_dbg; a.range_flag = rflag;
    return H16(prec, ap_launch_conv_pair)(a, P, P2, 4 * P, N1, st);
}

hipError_t ap_internal::launch_stem(int prec, int form, const float* x0, const float* x1, int n0, int n, const void* w, const void* w_lo,
                                    const float* scale, const float* shift, void* y, int* rflag, hipStream_t st) {
    if (prec_half(prec)) {
        if (form == 0) return H16(prec, ap_launch_stem_conv_mfma)(x0, x1, n0, w, scale, shift, y, n, st);
        return H16(prec, ap_launch_stem_pool)(x0, x1, n0, w, scale, shift, y, n, rflag, form, st, g_conv_dbg);
    }
    if (prec == AP_PREC_BF16X2) {
        if (form == 0) return k_bf16::ap_launch_stem_conv_mfma_split(x0, x1, n0, w, w_lo, scale, shift, y, n, st);
        return k_bf16::ap_launch_stem_pool_split(x0, x1, n0, w, w_lo, scale, shift, y, n, st);
    }
    hipError_t e = n0 ? k_bf16::ap_launch_stem_conv(x0, (const float*)w, scale, shift, y, n0, K_F32, st) : hipSuccess;
    if (e == hipSuccess && n > n0)
        e = k_bf16::ap_launch_stem_conv(x1, (const float*)w, scale, shift, (char*)y + (size_t)n0 * 112 * 112 * 64 * 4, n - n0, K_F32, st);
    return e;
}

hipError_t ap_internal::launch_maxpool(const void* x, void* y, int n, int prec, int* rflag, hipStream_t st) {
    return H16(prec, ap_launch_maxpool)(x, y, n, prec_kind(prec), rflag, st);
}
hipError_t ap_internal::launch_avgpool(const void* x, float* y, int n, int C, int prec, int* rflag, hipStream_t st) {
    return H16(prec, ap_launch_avgpool)(x, y, n, C, prec_kind(prec), rflag, st);
}

extern "C" {

int ap_conv2d_nhwc(int precision, const void* x, const void* w, const float* scale, const float* shift,
                   const void* res, void* y, int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad,
                   int relu, void* stream) {
    const int bf = prec_half(precision);
    if (!prec_valid(precision) || !x || !w || !scale ||
        !shift || !y || N <= 0 ||
        H <= 0 || W <= 0 || ksize <= 0 || stride <= 0 || pad < 0)
        return fail(AP_EINVAL, "ap_conv2d_nhwc: bad argument");
    if (Cin % (bf ? 64 : 32) || Cout % (precision == AP_PREC_FP32 ? 4 : 8) || Cin <= 0 || Cout <= 0)
        return fail(AP_ESHAPE, "ap_conv2d_nhwc: Cin must be a multiple of 64 (bf16) / 32 (fp32), Cout of 8 / 4");
    if ((H + 2 * pad - ksize) / stride + 1 <= 0 || (W + 2 * pad - ksize) / stride + 1 <= 0) return fail(AP_ESHAPE, "ap_conv2d_nhwc: empty output");
    const ConvDesc c{w, scale, shift, Cin, Cout, ksize, stride, pad, ksize * ksize * Cin, 0, 1};
    HIP_TRY(launch_conv(c, x, N, H, W, res, y, relu, 0, nullptr, 0, nullptr, nullptr, precision, conv_mode(), ops_range_word(precision),
                        (hipStream_t)stream));
    return AP_OK;
}

int ap_conv2d_tiled_nhwc(int precision, const void* x, const void* w, const float* scale, const float* shift,
                         const void* res, void* y, int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad,
                         int relu, void* stream) {
    const int bf = prec_half(precision);
    if (!prec_valid(precision) || !x || !w || !scale || !shift || !y || N <= 0 || H <= 0 || W <= 0 || ksize <= 0 || stride <= 0 || pad < 0)
        return fail(AP_EINVAL, "ap_conv2d_tiled_nhwc: bad argument");
    if (Cin % (bf ? 64 : 32) || Cout % (precision == AP_PREC_FP32 ? 4 : 8) || Cin <= 0 || Cout <= 0)
        return fail(AP_ESHAPE, "ap_conv2d_tiled_nhwc: Cin must be a multiple of 64 (bf16) / 32 (fp32), Cout of 8 / 4");
    if ((H + 2 * pad - ksize) / stride + 1 <= 0 || (W + 2 * pad - ksize) / stride + 1 <= 0)
        return fail(AP_ESHAPE, "ap_conv2d_tiled_nhwc: empty output");
    const ConvDesc c{w, scale, shift, Cin, Cout, ksize, stride, pad, ksize * ksize * Cin, 0, 1};
    const int mode = conv_mode();                            // ONE value for the check and for the launch
    if (const char* why = conv_form_refusal(c, N, H, W, 1, false, 0, precision, mode)) return fail(AP_ESHAPE, std::string("ap_conv2d_tiled_nhwc: ") + why);
    HIP_TRY(launch_conv(c, x, N, H, W, res, y, relu, 1, nullptr, 0, nullptr, nullptr, precision, mode, ops_range_word(precision),
                        (hipStream_t)stream));
    return AP_OK;
}

int ap_conv2d_fold_nhwc(int precision, const void* t, const void* x2, const void* w, const float* scale, const float* shift,
                        const void* res, void* y, int N, int Ho, int H2, int Cin, int Cin2, int Cout, int stride2, int relu,
                        void* stream) {
    const int bf = prec_half(precision);
    if (!prec_valid(precision) || !t || !x2 || !w || !scale || !shift || !y || N <= 0 || Ho <= 0 || H2 <= 0 || stride2 < 1 || stride2 > 2)
        return fail(AP_EINVAL, "ap_conv2d_fold_nhwc: bad argument (stride2 1 or 2)");
    if (Cin % (bf ? 64 : 32) || Cin2 % (bf ? 64 : 32) || Cout % (precision == AP_PREC_FP32 ? 4 : 8) || Cin <= 0 || Cin2 <= 0 || Cout <= 0)
        return fail(AP_ESHAPE, "ap_conv2d_fold_nhwc: Cin and Cin2 must be multiples of 64 (bf16) / 32 (fp32), Cout of 8 / 4");
    if (Ho != (H2 - 1) / stride2 + 1) return fail(AP_ESHAPE, "ap_conv2d_fold_nhwc: Ho must be (H2 - 1) / stride2 + 1");
    const ConvDesc c{w, scale, shift, Cin, Cout, 1, 1, 0, Cin + Cin2, Cin2, stride2};
    const int mode = conv_mode();                            // ONE value for the check and for the launch
    if (const char* why = conv_form_refusal(c, N, Ho, Ho, 0, true, H2, precision, mode)) return fail(AP_ESHAPE, std::string("ap_conv2d_fold_nhwc: ") + why);
    HIP_TRY(launch_conv(c, t, N, Ho, Ho, res, y, relu, 0, x2, H2, nullptr, nullptr, precision, mode, ops_range_word(precision),
                        (hipStream_t)stream));
    return AP_OK;
}

int ap_conv2d_pool_nhwc(int precision, const void* x, const void* w, const float* scale, const float* shift, const void* res,
                        float* pool_out, int N, int Cin, int Cout, void* stream) {
    if (!prec_valid(precision) || !x || !w || !scale || !shift || !res || !pool_out || N <= 0)
        return fail(AP_EINVAL, "ap_conv2d_pool_nhwc: bad argument (the identity is part of the operator)");
    const ConvDesc c{w, scale, shift, Cin, Cout, 1, 1, 0, Cin, 0, 1};
    if (Cin <= 0 || Cout <= 0 || Cin % 64 || Cout % 8 || !conv_pool_fits(c, N, precision))
        return fail(AP_ESHAPE, "ap_conv2d_pool_nhwc: 16-bit precision, Cin a multiple of 64, Cout of 8, tensors below 4 GiB");
    bool pooled = false;                                     // (true after the call: conv_pool_fits IS launch_conv's condition for the pooling branch)
    HIP_TRY(launch_conv(c, x, N, 7, 7, res, nullptr, 1, 0, nullptr, 0, pool_out, &pooled, precision, conv_mode(), ops_range_word(precision),
                        (hipStream_t)stream));
    return AP_OK;
}

int ap_bottleneck64_nhwc(int precision, const void* x, const void* w1, const float* s1, const float* h1, const void* w2,
                         const float* s2, const float* h2, const void* w3, const float* s3, const float* h3, void* y,
                         int N, int H, int W, int Cin, int downsample, void* stream) {
    if (!prec_half(precision) || !x || !w1 || !s1 || !h1 || !w2 || !s2 || !h2 || !w3 || !s3 || !h3 || !y || N <= 0)
        return fail(AP_EINVAL, "ap_bottleneck64_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (H <= 0 || W <= 0 || H % 14 || W % 14 || !((Cin == 256 && !downsample) || (Cin == 64 && downsample)))
        return fail(AP_ESHAPE, "ap_bottleneck64_nhwc: H, W multiples of 14; Cin 256 (identity) or 64 (downsample)");
    HIP_TRY(launch_bneck2(ConvDesc{w1, s1, h1}, ConvDesc{w2, s2, h2}, ConvDesc{w3, s3, h3}, downsample ? 1 : 0, x, y, N, H, W, nullptr, nullptr, 0,
                          precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_bottleneck64_tail_nhwc(int precision, const void* x, const void* w1, const float* s1, const float* h1, const void* w2,
                              const float* s2, const float* h2, const void* w3, const float* s3, const float* h3, void* y,
                              const void* w1n, const float* s1n, const float* h1n, void* t1n, int y_even, int N, int H, int W,
                              void* stream) {
    if (!prec_half(precision) || !x || !w1 || !s1 || !h1 || !w2 || !s2 || !h2 || !w3 || !s3 || !h3 || !y || !w1n || !s1n || !h1n ||
        !t1n || N <= 0)
        return fail(AP_EINVAL, "ap_bottleneck64_tail_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (H <= 0 || W <= 0 || H % 14 || W % 14) return fail(AP_ESHAPE, "ap_bottleneck64_tail_nhwc: H, W multiples of 14");
    const ConvDesc c1n{w1n, s1n, h1n};
    HIP_TRY(launch_bneck2(ConvDesc{w1, s1, h1}, ConvDesc{w2, s2, h2}, ConvDesc{w3, s3, h3}, 0, x, y, N, H, W, &c1n, t1n, y_even != 0, precision,
                          ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int64_t ap_conv_pw_stream_bytes(int Cin, int Cout) {
    return (Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 256 == 0) ? (int64_t)k_bf16::ap_conv_pw_stream_bytes(Cin, Cout) : -1;
}

int ap_conv_pw_pack(int precision, const void* w, int Cin, int Cout, void* wstream, void* stream) {
    if (!prec_half(precision) || !w || !wstream || Cin <= 0 || Cout <= 0 || Cin % 32 || Cout % 256)
        return fail(AP_EINVAL, "ap_conv_pw_pack: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16; Cin % 32 == 0, Cout % 256 == 0)");
    HIP_TRY(H16(precision, ap_launch_conv_pw_pack)(w, wstream, Cin, Cout, Cin, (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_pw_nhwc(int precision, const void* x, const void* wstream, const float* scale, const float* shift, const void* res,
                    void* y, int M, int Cin, int Cout, void* stream) {
    if (!prec_half(precision) || !x || !wstream || !scale || !shift || !y)
        return fail(AP_EINVAL, "ap_conv_pw_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (!k_bf16::ap_conv_pw_supported(M, Cin, Cout))
        return fail(AP_ESHAPE, "ap_conv_pw_nhwc: M must be a multiple of 196, Cin of 128 (>= 256), Cout of 256");
    HIP_TRY(launch_conv_pw(ConvDesc{wstream, scale, shift, Cin, Cout}, x, res, y, M, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_pw_ds_nhwc(int precision, const void* t2, const void* x, const void* wstream, const float* scale, const float* shift,
                       void* y, int N, int Ho, int Cin, int Cin2, int Cout, int stride, void* stream) {
    if (!prec_half(precision) || !t2 || !x || !wstream || !scale || !shift || !y || N <= 0 || Ho <= 0 || stride < 1 || stride > 2)
        return fail(AP_EINVAL, "ap_conv_pw_ds_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16; stride 1 or 2)");
    const ConvDesc c{wstream, scale, shift, Cin, Cout, 1, 1, 0, Cin + Cin2, Cin2, stride};
    if (!conv_pw_ds_fits(c, N, Ho, Ho * stride))
        return fail(AP_ESHAPE, "ap_conv_pw_ds_nhwc: N Ho Ho a multiple of 196 with Ho Ho | 196, Cin and Cin2 multiples of 64 (sum: of 128), Cout of 256");
    HIP_TRY(launch_conv_pw_ds(c, t2, x, y, N, Ho, Ho * stride, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_pw_k3s2_nhwc(int precision, const void* x, const void* wstream, const float* scale, const float* shift, void* y, int N,
                         int H, int Cin, int Cout, void* stream) {
    if (!prec_half(precision) || !x || !wstream || !scale || !shift || !y || N <= 0 || H <= 0)
        return fail(AP_EINVAL, "ap_conv_pw_k3s2_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    const ConvDesc c{wstream, scale, shift, Cin, Cout, 3, 2, 1};
    if (!conv_pw_k3_fits(c, N, H))
        return fail(AP_ESHAPE, "ap_conv_pw_k3s2_nhwc: H even with (H / 2)^2 | 196 (14 or 28), N (H / 2)^2 a multiple of 196, Cin / 64 a power of two >= 2, Cout a multiple of 256");
    HIP_TRY(launch_conv_pw_k3(c, x, y, N, H, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int64_t ap_block_img_stream_bytes(void) { return (int64_t)k_bf16::ap_block_img_stream_bytes(); }

int ap_block_img_pack(int precision, const void* w1, const void* w2, const void* w3, void* wstream, void* stream) {
    if (!prec_half(precision) || !w1 || !w2 || !w3 || !wstream)
        return fail(AP_EINVAL, "ap_block_img_pack: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    HIP_TRY(H16(precision, ap_launch_block_img_pack)(w1, w2, w3, wstream, (hipStream_t)stream));
    return AP_OK;
}

int ap_block_img_nhwc(int precision, const void* x, const void* wstream, const float* s1, const float* h1, const float* s2,
                      const float* h2, const float* s3, const float* h3, void* y, int N, void* stream) {
    if (!prec_half(precision) || !x || !wstream || !s1 || !h1 || !s2 || !h2 || !s3 || !h3 || !y || N <= 0)
        return fail(AP_EINVAL, "ap_block_img_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    HIP_TRY(launch_block_img(x, wstream, s1, h1, s2, h2, s3, h3, y, N, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int64_t ap_conv_img3_stream_bytes(void) { return (int64_t)k_bf16::ap_conv_img3_stream_bytes(); }

int64_t ap_conv_s2p_stream_bytes(void) { return (int64_t)k_bf16::ap_conv_s2p_stream_bytes(); }

int ap_conv_s2p_pack(int precision, const void* w2, void* wstream, void* stream) {
    if (!prec_half(precision) || !w2 || !wstream) return fail(AP_EINVAL, "ap_conv_s2p_pack: 16-bit precision, w2 [128][3][3][128], stream buffer");
    HIP_TRY(H16(precision, ap_launch_conv_s2p_pack)(w2, wstream, (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_s2p_nhwc(int precision, const void* x, const void* wstream, const float* scale, const float* shift, void* y, int N,
                     int y_tiled, void* stream) {
    if (!prec_half(precision) || !x || !wstream || !scale || !shift || !y || N <= 0)
        return fail(AP_EINVAL, "ap_conv_s2p_nhwc: bad argument");
    HIP_TRY(launch_conv_s2p(x, wstream, scale, shift, y, N, y_tiled != 0, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_img3_pack(int precision, const void* w2, void* wstream, void* stream) {
    if (!prec_half(precision) || !w2 || !wstream) return fail(AP_EINVAL, "ap_conv_img3_pack: 16-bit precision, w2 [128][3][3][128], stream buffer");
    HIP_TRY(H16(precision, ap_launch_conv_img3_pack)(w2, wstream, (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_img3_nhwc(int precision, const void* x, const void* wstream, const float* scale, const float* shift, void* y, int N,
                      int y_tiled, void* stream) {
    if (!prec_half(precision) || !x || !wstream || !scale || !shift || !y || N <= 0)
        return fail(AP_EINVAL, "ap_conv_img3_nhwc: bad argument");
    HIP_TRY(launch_conv_img3(x, wstream, scale, shift, y, N, y_tiled != 0, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

// ---- stem and pooling operators: every kernel of stem.hip a trunk pass can launch, through the launch calls the pass makes
int64_t ap_stem_pack_bytes(int precision) {
    if (!prec_valid(precision)) return AP_EINVAL;
    return precision == AP_PREC_FP32 ? 147 * 64 * 4 : (precision == AP_PREC_BF16X2 ? 2 : 1) * 64 * AP_STEM_WLD * 2;
}

int ap_stem_pack(int precision, const float* w, void* wpacked, void* stream) {
    if (!prec_valid(precision) || !w || !wpacked) return fail(AP_EINVAL, "ap_stem_pack: precision, w [64][3][7][7] fp32, packed buffer");
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> hw(64 * 3 * 49);
    HIP_TRY(hipMemcpyAsync(hw.data(), w, hw.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    StemPack sp;
    bool ovf = false;
    pack_stem(hw.data(), precision, sp, &ovf);
    if (ovf) return fail(AP_ERANGE, "ap_stem_pack: a weight leaves the fp16 range");
    if (precision == AP_PREC_FP32) {
        HIP_TRY(hipMemcpyAsync(wpacked, sp.direct.data(), sp.direct.size() * 4, hipMemcpyHostToDevice, st));
    } else {
        const size_t plane = sp.pk.size() * 2;
        HIP_TRY(hipMemcpyAsync(wpacked, sp.pk.data(), plane, hipMemcpyHostToDevice, st));
        if (precision == AP_PREC_BF16X2)
            HIP_TRY(hipMemcpyAsync((char*)wpacked + plane, sp.pk_lo.data(), plane, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                       // (the host vectors go out of scope)
    return AP_OK;
}

int ap_stem_nhwc(int precision, int form, const float* x0, const float* x1, int n_split, const void* wpacked, const float* scale,
                 const float* shift, void* y, int N, void* stream) {
    if (!prec_valid(precision) || !wpacked || !scale || !shift || !y || N <= 0 || n_split < 0 || n_split > N || (n_split > 0 && !x0) ||
        (n_split < N && !x1))
        return fail(AP_EINVAL, "ap_stem_nhwc: bad argument (x0: the first n_split images, x1: the other N - n_split)");
    const bool half = prec_half(precision);
    if (form < 0 || form > (half ? 2 : precision == AP_PREC_BF16X2 ? 1 : 0))
        return fail(AP_EINVAL, "ap_stem_nhwc: form 0 (un-pooled; every precision), 1 (strip kernel; 16-bit, bf16x2), 2 (persistent kernel; 16-bit)");
    const void* wlo = (const char*)wpacked + (size_t)64 * AP_STEM_WLD * 2;   // (AP_PREC_BF16X2: the low plane follows the high one)
    HIP_TRY(launch_stem(precision, form, x0, x1, n_split, N, wpacked, wlo, scale, shift, y, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_maxpool_nhwc(int precision, const void* x, void* y, int N, void* stream) {
    if (!prec_valid(precision) || !x || !y || N <= 0) return fail(AP_EINVAL, "ap_maxpool_nhwc: bad argument");
    HIP_TRY(launch_maxpool(x, y, N, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_avgpool_nhwc(int precision, const void* x, float* y, int N, int C, void* stream) {
    if (!prec_valid(precision) || !x || !y || N <= 0) return fail(AP_EINVAL, "ap_avgpool_nhwc: bad argument");
    if (C <= 0 || C % (precision == AP_PREC_FP32 ? 128 : 256)) return fail(AP_ESHAPE, "ap_avgpool_nhwc: C a multiple of 256 (fp32: 128)");
    HIP_TRY(launch_avgpool(x, y, N, C, precision, ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

// The fused pair kernel consumes its two weight matrices as ONE stream of 16-KiB tiles in consumption order.  The stream is
// CALLER-OWNED: packed once by ap_conv_pair_pack into a buffer of ap_conv_pair_stream_bytes, handed to every launch -- the
// library keeps no hidden copy keyed by weight addresses (an allocator may reuse an address for new contents).
int64_t ap_conv_pair_stream_bytes(int P, int P2, int N1) {
    if (!k_bf16::ap_conv_pair_supported(P, P2, 4 * P, N1)) return AP_ESHAPE;
    return (int64_t)k_bf16::ap_conv_pair_stream_bytes(P, P2, 4 * P, N1);
}

int ap_conv_pair_pack(int precision, const void* w3, const void* w1, int P, int P2, int N1, void* wstream, void* stream) {
    if (!prec_half(precision) || !w3 || !wstream || (N1 > 0 && !w1))
        return fail(AP_EINVAL, "ap_conv_pair_pack: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (!k_bf16::ap_conv_pair_supported(P, P2, 4 * P, N1))
        return fail(AP_ESHAPE, "ap_conv_pair_pack: (P, P2, N1) must be (128,0,128), (128,0,256), (256,0,256), (128,256,128) or (256,512,0)");
    HIP_TRY(H16(precision, ap_launch_pair_pack)(w3, N1 ? w1 : nullptr, wstream, P, P2, 4 * P, N1, (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_pair_nhwc(int precision, const void* t2, const void* wstream, const float* s3, const float* h3, const void* res,
                      const float* s1, const float* h1, void* out, void* t1n, int M, int P, int N1, void* stream) {
    if (!prec_half(precision) || !t2 || !wstream || !s3 || !h3 || !res || !s1 || !h1 || !out || !t1n || M <= 0)
        return fail(AP_EINVAL, "ap_conv_pair_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (!k_bf16::ap_conv_pair_supported(P, 0, 4 * P, N1)) return fail(AP_ESHAPE, "ap_conv_pair_nhwc: (P, N1) must be (128,128), (128,256) or (256,256)");
    HIP_TRY(launch_conv_pair(t2, wstream, s3, h3, s1, h1, res, out, t1n, M, 0, 0, 0, P, 0, N1, PairLayout{}, precision, ops_range_word(precision),
                             (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_pair_ds_nhwc(int precision, const void* t2, const void* x, const void* wstream, const float* s3, const float* h3,
                         const float* s1, const float* h1, void* out, void* t1n, int N, int Ho, int P, int P2, int stride, int N1,
                         void* stream) {
    if (!prec_half(precision) || !t2 || !x || !wstream || !s3 || !h3 || !out || N <= 0 || Ho <= 0 || (N1 > 0 && (!s1 || !h1 || !t1n)))
        return fail(AP_EINVAL, "ap_conv_pair_ds_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (!k_bf16::ap_conv_pair_supported(P, P2, 4 * P, N1) || stride < 1 || stride > 2)
        return fail(AP_ESHAPE, "ap_conv_pair_ds_nhwc: (P, P2, N1) must be (128,256,128) or (256,512,0); stride 1 or 2");
    HIP_TRY(launch_conv_pair(t2, wstream, s3, h3, s1, h1, x, out, t1n, N * Ho * Ho, Ho, Ho * stride, stride, P, P2, N1, PairLayout{}, precision,
                             ops_range_word(precision), (hipStream_t)stream));
    return AP_OK;
}

int ap_conv_pair_layout_nhwc(int precision, const void* t2, const void* in, const void* wstream, const float* s3, const float* h3,
                             const float* s1, const float* h1, void* out, void* t1n, int N, int Ho, int P, int P2, int stride, int N1,
                             int t2_tiled, int res_tiled, int out_tiled, int out_even, void* stream) {
    if (!prec_half(precision) || !t2 || !in || !wstream || !s3 || !h3 || !out || N <= 0 || Ho <= 0 || (N1 > 0 && (!s1 || !h1 || !t1n)))
        return fail(AP_EINVAL, "ap_conv_pair_layout_nhwc: bad argument (precision: AP_PREC_BF16 or AP_PREC_F16)");
    if (!k_bf16::ap_conv_pair_supported(P, P2, 4 * P, N1) || (P2 > 0 && (stride < 1 || stride > 2)))
        return fail(AP_ESHAPE, "ap_conv_pair_layout_nhwc: (P, P2, N1) must be (128,0,128), (128,0,256), (256,0,256), (128,256,128) or (256,512,0); stride 1 or 2");
    if ((res_tiled && P2 > 0) || (out_even && out_tiled) || (out_even && N1 == 0))
        return fail(AP_ESHAPE, "ap_conv_pair_layout_nhwc: res_tiled needs an identity block, out_even an untiled out and a next conv1");
    HIP_TRY(launch_conv_pair(t2, wstream, s3, h3, s1, h1, in, out, t1n, N * Ho * Ho, Ho, P2 > 0 ? Ho * stride : 0, P2 > 0 ? stride : 0, P, P2, N1,
                             PairLayout{t2_tiled != 0, res_tiled != 0, out_tiled != 0, out_even != 0}, precision, ops_range_word(precision),
                             (hipStream_t)stream));
    return AP_OK;
}

int ap_rotmat_to_angle_axis(const float* rotmat, int n, int cols, float* angle_axis, void* stream) {
    if (!rotmat || !angle_axis || n <= 0 || (cols != 3 && cols != 4))
        return fail(AP_EINVAL, "ap_rotmat_to_angle_axis: bad argument (cols must be 3 or 4)");
    HIP_TRY(ap_launch_rotmat_to_angle_axis(rotmat, n, cols, angle_axis, (hipStream_t)stream));
    return AP_OK;
}

int ap_batch_rodrigues(const float* angle_axis, int n, int variant, float* rotmat, void* stream) {
    if (!angle_axis || !rotmat || n <= 0 || (variant != 0 && variant != 1))
        return fail(AP_EINVAL, "ap_batch_rodrigues: bad argument (variant 0 = smplx lbs, 1 = copenet geometry)");
    HIP_TRY(ap_launch_batch_rodrigues(angle_axis, n, variant, rotmat, (hipStream_t)stream));
    return AP_OK;
}

int ap_batch_rodrigues_bwd(const float* angle_axis, int n, const float* grad_rotmat, float* grad_angle_axis, void* stream) {
    if (!angle_axis || !grad_rotmat || !grad_angle_axis || n <= 0) return fail(AP_EINVAL, "ap_batch_rodrigues_bwd: bad argument");
    HIP_TRY(ap_launch_batch_rodrigues_bwd(angle_axis, n, grad_rotmat, grad_angle_axis, (hipStream_t)stream));
    return AP_OK;
}

int ap_rot6d_to_rotmat(const float* x6, int n, float* rotmat, void* stream) {
    if (!x6 || !rotmat || n <= 0) return fail(AP_EINVAL, "ap_rot6d_to_rotmat: bad argument");
    HIP_TRY(ap_launch_rot6d(x6, n, rotmat, (hipStream_t)stream));
    return AP_OK;
}

int ap_transform_points(const float* rt, const float* pts, int B, int P, float* out, void* stream) {
    if (!rt || !pts || !out || B <= 0 || P <= 0) return fail(AP_EINVAL, "ap_transform_points: bad argument");
    HIP_TRY(ap_launch_transform_points(rt, pts, B, P, out, (hipStream_t)stream));
    return AP_OK;
}

int ap_preprocess_crops(const unsigned char* frames, int64_t frame_stride_bytes, int n, int H, int W, int bgr,
                        const int* crop_y0y1x0x1, float* out_nchw, float* scale_out, int* pad_left_top_out, void* stream) {
    if (!frames || !crop_y0y1x0x1 || !out_nchw || !scale_out || !pad_left_top_out || n <= 0 || H <= 0 || W <= 0 ||
        frame_stride_bytes < 0)
        return fail(AP_EINVAL, "ap_preprocess_crops: bad argument");
    HIP_TRY(k_bf16::ap_launch_preprocess(frames, (size_t)frame_stride_bytes, n, H, W, bgr, crop_y0y1x0x1, out_nchw, scale_out,
                                 pad_left_top_out, (hipStream_t)stream));
    return AP_OK;
}

int ap_perspective_projection(const float* pts, int B, int P, const float* rotation, const float* translation,
                              float fx, float fy, const float* center, float* out, void* stream) {
    if (!pts || !center || !out || B <= 0 || P <= 0) return fail(AP_EINVAL, "ap_perspective_projection: bad argument");
    HIP_TRY(ap_launch_projection(pts, B, P, rotation, translation, fx, fy, center, out, (hipStream_t)stream));
    return AP_OK;
}

}  // extern "C"
