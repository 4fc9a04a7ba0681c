// The regressor heads of libairpose_hip.so: IEF from trunk features (copenet, single-view, muhmr, hmr), the whole-model entry
// points that run the trunk first, and the precision probe of a checkpoint.
#include "api_internal.h"

namespace {

// y[M][ldy] = x[M][ldx(:K)] * W^T * scale + shift (+ res)
int run_gemm(const Layer& L, const float* x, int ldx, int K, int M, float* y, int ldy, const float* res, int ldr,
             hipStream_t st) {
    ConvArgs a{};
    a.x = x; a.w = L.w.p; a.scale = L.scale.as<float>(); a.shift = L.shift.as<float>(); a.res = res; a.y = y;
    a.N = M; a.H = a.W = a.Ho = a.Wo = 1;
    a.Cin = K; a.Cout = L.cout;
    a.KH = a.KW = 1; a.stride = 1; a.pad = 0;
    a.M = M;
    a.ldx = ldx; a.ldy = ldy; a.ldr = ldr; a.wld = L.wld;
    a.relu = 0;
    HIP_TRY(dispatch_conv(a, 0, st));
    return AP_OK;
}

struct RegInputs {
    const float *xf0, *xf1, *bb0, *bb1, *pos0, *pos1, *th0, *th1, *sh0, *sh1;
    int th0_bs, th1_bs, sh0_bs, sh1_bs;
};

// initial state of the IEF iterations, everything but `state` (where the kernel leaves it: the caller's choice)
RegInitArgs reg_init_args(const ap_net* h, const RegInputs& in, int pos_bs, int rows, int B) {
    RegInitArgs ia{};
    ia.pos0 = in.pos0; ia.pos1 = in.pos1; ia.theta0 = in.th0; ia.theta1 = in.th1; ia.shape0 = in.sh0; ia.shape1 = in.sh1;
    ia.theta0_bs = in.th0_bs; ia.theta1_bs = in.th1_bs; ia.shape0_bs = in.sh0_bs; ia.shape1_bs = in.sh1_bs;
    ia.pos_bs = pos_bs; ia.rows = rows; ia.B = B;
    ia.mean_pose = h->mean_pose.as<float>(); ia.mean_shape = h->mean_shape.as<float>();
    return ia;
}

// xf rows: view 0 then view 1 (two_view) laid out by the caller as two pointers; H rows follow the same order
int regressor_run(ap_net* h, const RegInputs& in, int B, int iters, int two_view, const float* partner,
                  int partner_ld, int pos_bs, float* pose0, float* betas0, float* pose1, float* betas1,
                  hipStream_t st) {
    if (!h->finalized) return fail(AP_ESTATE, "ap_net_finalize has not been called");
    if (h->variant == 1)
        return fail(AP_ESTATE, "regressor entry points need a copenet-layout handle (variants 0, 2, 3), not hmr");
    if (h->variant == 2 && (two_view || partner))
        return fail(AP_ESTATE, "a copenet_singleview handle has no cross-view inputs");
    if (h->variant != 2 && !two_view && !partner) return fail(AP_EINVAL, "regressor step: partner state missing");
    if (B <= 0 || iters < 1) return fail(AP_EINVAL, "regressor: bad B / iters");
    const int rows = two_view ? 2 * B : B;
    HIP_TRY(h->ws_H.reserve((size_t)rows * 1024 * 4));
    HIP_TRY(h->ws_T1.reserve((size_t)rows * 1024 * 4));
    HIP_TRY(h->ws_T2.reserve((size_t)rows * 1024 * 4));
    HIP_TRY(h->ws_S.reserve((size_t)rows * SLD * 4));
    HIP_TRY(h->ws_D.reserve((size_t)rows * DLD * 4));
    HIP_TRY(h->ws_state.reserve((size_t)rows * ST * 4));
    size_t e0 = 0, e1 = 0;
    if (h->tm.on == 1) HIP_TRY(h->tm.rec(st, &e0));
    if (h->fold && h->fuse_ief) {
        HIP_TRY(h->ws_H.reserve((size_t)ap_reg_fold_part_floats(rows) * 4));
        RegInitArgs ia = reg_init_args(h, in, pos_bs, rows, B);
        ia.state = nullptr;
        HIP_TRY(ap_launch_reg_fold_ief(ia, in.xf0, two_view ? in.xf1 : in.xf0, in.bb0, in.bb1, partner, partner_ld,
                                       h->foldT_feat.as<float>(), h->foldT_state.as<float>(), h->fold_bias.as<float>(),
                                       h->ws_H.as<float>(), iters, two_view, pose0, betas0, pose1, betas1, st));
        if (h->tm.on == 1) {
            HIP_TRY(h->tm.rec(st, &e1));
            h->tm.marks[3].push_back(e0); h->tm.marks[3].push_back(e1);
        }
        return AP_OK;
    }
    float *Hb = h->ws_H.as<float>(), *T1 = h->ws_T1.as<float>(), *T2 = h->ws_T2.as<float>(), *S = h->ws_S.as<float>(),
          *D = h->ws_D.as<float>(), *state = h->ws_state.as<float>();
    int rc;
    // trunk-feature part (+ bias), constant over the iterations: of fc1 (literal chain) or of the folded map
    const Layer& Lf = h->fold ? h->fold_feat : h->fc1_feat;
    const int hld = h->fold ? DLD : 1024;
    if (two_view && in.xf1 == in.xf0 + (size_t)B * 2048) {          // both views contiguous: one launch
        if ((rc = run_gemm(Lf, in.xf0, 2048, 2048, 2 * B, Hb, hld, nullptr, 0, st))) return rc;
    } else {
        if ((rc = run_gemm(Lf, in.xf0, 2048, 2048, B, Hb, hld, nullptr, 0, st))) return rc;
        if (two_view)
            if ((rc = run_gemm(Lf, in.xf1, 2048, 2048, B, Hb + (size_t)B * hld, hld, nullptr, 0, st))) return rc;
    }
    RegInitArgs ia = reg_init_args(h, in, pos_bs, rows, B);
    ia.state = state;
    HIP_TRY(ap_launch_reg_init(ia, st));
    for (int it = 0; it < iters; ++it) {
        HIP_TRY(ap_launch_reg_update_assemble(state, it ? D : nullptr, DLD, in.bb0, in.bb1, partner, partner_ld, S, B,
                                              two_view, st));
        if (h->fold) {
            if ((rc = run_gemm(h->fold_state, S, SLD, SLD, rows, D, DLD, Hb, DLD, st))) return rc;
        } else {
            if ((rc = run_gemm(h->fc1_state, S, SLD, SLD, rows, T1, 1024, Hb, 1024, st))) return rc;
            if ((rc = run_gemm(h->fc2, T1, 1024, 1024, rows, T2, 1024, nullptr, 0, st))) return rc;
            if ((rc = run_gemm(h->dec, T2, 1024, 1024, rows, D, DLD, nullptr, 0, st))) return rc;
        }
    }
    // fold the last delta into the state and emit
    HIP_TRY(ap_launch_reg_update_assemble(state, D, DLD, in.bb0, in.bb1, partner, partner_ld, S, B, two_view, st));
    HIP_TRY(ap_launch_reg_output(state, pose0, betas0, pose1, betas1, B, two_view, st));
    if (h->tm.on == 1) {
        HIP_TRY(h->tm.rec(st, &e1));
        h->tm.marks[3].push_back(e0); h->tm.marks[3].push_back(e1);
    }
    return AP_OK;
}

// IEF of the HMR head from trunk features: state rows of 160 floats = pose132 | shape10 | cam3 | pad, left in ws_state
int hmr_ief(ap_net* h, const float* feat, int B, int iters, const float* init_theta, int theta_bs, const float* init_shape,
            int shape_bs, const float* init_cam, int cam_bs, hipStream_t st) {
    HIP_TRY(h->ws_H.reserve((size_t)B * DLD * 4));
    HIP_TRY(h->ws_D.reserve((size_t)B * DLD * 4));
    HIP_TRY(h->ws_state.reserve((size_t)B * 160 * 4));
    float *Hb = h->ws_H.as<float>(), *D = h->ws_D.as<float>(), *state = h->ws_state.as<float>();
    int rc;
    if ((rc = run_gemm(h->fold_feat, feat, 2048, 2048, B, Hb, DLD, nullptr, 0, st))) return rc;
    HIP_TRY(ap_launch_hmr_init(init_theta, theta_bs, init_shape, shape_bs, init_cam, cam_bs, h->mean_pose.as<float>(),
                               h->mean_shape.as<float>(), h->mean_cam.as<float>(), state, B, st));
    for (int it = 0; it < iters; ++it) {
        if ((rc = run_gemm(h->fold_state, state, 160, 160, B, D, DLD, Hb, DLD, st))) return rc;
        HIP_TRY(ap_launch_hmr_update(state, D, DLD, B, st));
    }
    return AP_OK;
}

}  // namespace

extern "C" {

int ap_regressor_fwd(ap_net* h, const float* xf0, const float* xf1, const float* bb0, const float* bb1,
                     const float* pos0, const float* pos1, const float* init_theta0, int theta0_bs,
                     const float* init_theta1, int theta1_bs, const float* init_shape0, int shape0_bs,
                     const float* init_shape1, int shape1_bs, int B, int iters, float* pose0, float* betas0,
                     float* pose1, float* betas1, void* stream) {
    if (!h || !xf0 || !xf1 || !bb0 || !bb1 || !pos0 || !pos1 || !pose0 || !betas0 || !pose1 || !betas1)
        return fail(AP_EINVAL, "ap_regressor_fwd: null argument");
    RegInputs in{xf0, xf1, bb0, bb1, pos0, pos1, init_theta0, init_theta1, init_shape0, init_shape1,
                 theta0_bs, theta1_bs, shape0_bs, shape1_bs};
    return regressor_run(h, in, B, iters, 1, nullptr, 0, 3, pose0, betas0, pose1, betas1, (hipStream_t)stream);
}

int ap_regressor_step(ap_net* h, const float* xf, const float* bb, const float* pose_in, const float* betas_in,
                      const float* partner, int partner_ld, int B, float* pose_out, float* betas_out, void* stream) {
    if (!h || !xf || !bb || !pose_in || !betas_in || !partner || !pose_out || !betas_out || partner_ld < 136)
        return fail(AP_EINVAL, "ap_regressor_step: bad argument");
    RegInputs in{xf, nullptr, bb, nullptr, pose_in, nullptr, pose_in + 3, nullptr, betas_in, nullptr, 135, 0, 10, 0};
    return regressor_run(h, in, B, 1, 0, partner, partner_ld, 135, pose_out, betas_out, nullptr, nullptr,
                         (hipStream_t)stream);
}

int ap_regressor_feat_part(ap_net* h, const float* xf, int B, float* hfeat, void* stream) {
    if (!h || !xf || !hfeat || B <= 0) return fail(AP_EINVAL, "ap_regressor_feat_part: bad argument");
    if (!h->finalized) return fail(AP_ESTATE, "ap_net_finalize has not been called");
    if (h->variant != 0 || !h->fold)
        return fail(AP_ESTATE, "ap_regressor_feat_part / _step_local / _step_finish evaluate the folded two-view map (ap_net_fold_status == 1); "
                               "this handle runs the literal chain: use ap_regressor_step");
    HIP_TRY(h->ws_H.reserve((size_t)ap_reg_fold_part_floats(B) * 4));
    HIP_TRY(ap_launch_reg_feat_part(xf, B, h->foldT_feat.as<float>(), h->fold_bias.as<float>(), h->ws_H.as<float>(), hfeat, (hipStream_t)stream));
    return AP_OK;
}

int ap_regressor_step_local(ap_net* h, const float* hfeat, const float* bb, const float* pose_in, const float* betas_in, int B,
                            float* partial, void* stream) {
    if (!h || !hfeat || !bb || !pose_in || !betas_in || !partial || B <= 0) return fail(AP_EINVAL, "ap_regressor_step_local: bad argument");
    if (!h->finalized) return fail(AP_ESTATE, "ap_net_finalize has not been called");
    if (h->variant != 0 || !h->fold) return fail(AP_ESTATE, "ap_regressor_step_local needs the folded two-view map (ap_net_fold_status == 1)");
    HIP_TRY(ap_launch_reg_step_local(hfeat, bb, pose_in, betas_in, B, h->foldT_state.as<float>(), partial, (hipStream_t)stream));
    return AP_OK;
}

int ap_regressor_step_finish(ap_net* h, const float* partial, const float* pose_in, const float* betas_in, const float* partner,
                             int partner_ld, int B, float* pose_out, float* betas_out, void* stream) {
    if (!h || !partial || !pose_in || !betas_in || !partner || !pose_out || !betas_out || partner_ld < 136 || B <= 0)
        return fail(AP_EINVAL, "ap_regressor_step_finish: bad argument");
    if (!h->finalized) return fail(AP_ESTATE, "ap_net_finalize has not been called");
    if (h->variant != 0 || !h->fold) return fail(AP_ESTATE, "ap_regressor_step_finish needs the folded two-view map (ap_net_fold_status == 1)");
    HIP_TRY(ap_launch_reg_step_finish(partial, pose_in, betas_in, partner, partner_ld, B, h->foldT_state.as<float>(), pose_out, betas_out,
                                      (hipStream_t)stream));
    return AP_OK;
}

// The handle's arithmetic against the exact-fp32 mode of the SAME weights on a seeded probe batch, on the GPU: what the 1e-4 claim of a
// 16-bit mode is worth on THIS checkpoint.  Only the trunk differs between the modes (the regressor is fp32 everywhere), so the
// reference is an fp32 trunk packed from the handle's own host tensors (kept until the next ap_net_finalize) and both feature sets
// go through the handle's regressor.
int ap_net_parity_probe(ap_net* h, int n_pairs, uint64_t seed, double* err8, void* stream) {
    if (!h || !err8 || n_pairs < 1 || n_pairs > 64) return fail(AP_EINVAL, "ap_net_parity_probe: handle, 1 <= n_pairs <= 64, err8");
    if (!h->finalized) return fail(AP_ESTATE, "ap_net_finalize has not been called");
    if (h->variant != 0) return fail(AP_ESTATE, "ap_net_parity_probe: two-view copenet handles only");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(h->device));
    for (int i = 0; i < 8; ++i) err8[i] = 0.0;
    if (h->prec == AP_PREC_FP32) return AP_OK;               // the reference itself
    if (!h->probe_ref) {
        ap_net* r = new ap_net();
        r->device = h->device; r->prec = AP_PREC_FP32; r->variant = h->variant; r->tensors_of = h;
        const int rc = finalize_trunk(r);
        if (rc) { ap_net_destroy(r); return rc; }
        r->finalized = true;                                 // (trunk only: its regressor is never called)
        h->probe_ref = r;
    }
    const int B = n_pairs;
    const size_t IMG = (size_t)3 * 224 * 224;
    HIP_TRY(h->probe_x.reserve(2 * B * IMG * 4));
    HIP_TRY(h->probe_bb.reserve((size_t)2 * B * 3 * 4));
    HIP_TRY(h->probe_pos.reserve((size_t)B * 3 * 4));
    HIP_TRY(h->probe_feat.reserve((size_t)2 * 2 * B * 2048 * 4));
    HIP_TRY(h->probe_out.reserve((size_t)2 * 2 * B * 145 * 4));
    float *x = h->probe_x.as<float>(), *bb = h->probe_bb.as<float>(), *pos = h->probe_pos.as<float>();
    HIP_TRY(ap_launch_probe_inputs(x, 2 * B * IMG, bb, 2 * B, seed, st));
    std::vector<float> hp((size_t)B * 3);
    for (int b = 0; b < B; ++b) { hp[3 * b] = 0.f; hp[3 * b + 1] = 0.f; hp[3 * b + 2] = 10.f * 0.05f; }   // copenet_twoview.py:184,201-203
    HIP_TRY(hipMemcpyAsync(pos, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                       // (hp is a local)
    std::vector<float> out[2];
    for (int m = 0; m < 2; ++m) {
        ap_net* net = m ? h->probe_ref : h;
        float* feat = h->probe_feat.as<float>() + (size_t)m * 2 * B * 2048;
        float* o = h->probe_out.as<float>() + (size_t)m * 2 * B * 145;
        int rc = trunk_fwd(net, x, B, x + B * IMG, B, feat, st);
        if (rc) return rc;
        RegInputs in{feat, feat + (size_t)B * 2048, bb, bb + (size_t)B * 3, pos, pos, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
        float *p0 = o, *p1 = o + (size_t)B * 135, *b0 = o + (size_t)2 * B * 135, *b1 = b0 + (size_t)B * 10;
        if ((rc = regressor_run(h, in, B, 3, 1, nullptr, 0, 3, p0, b0, p1, b1, st))) return rc;
        out[m].resize((size_t)2 * B * 145);
        HIP_TRY(hipMemcpyAsync(out[m].data(), o, out[m].size() * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (h->range_any())
        return fail(AP_ERANGE, "ap_net_parity_probe: the probe batch left the fp16 range");
    // slices: translation (3), 6-D rotations (132), betas (10), projected root u = f tx / tz + cx, v likewise (the 2-D error is the
    // translation error seen through the camera: f = 1475, centre (960, 540), constants.py:7-11); norm-wise max|a-b| / max|b| in
    // err8[0..3], element-wise max |a-b| / (1e-2 + |b|) in err8[4..7]
    double num[4] = {0, 0, 0, 0}, den[4] = {0, 0, 0, 0}, el[4] = {0, 0, 0, 0};
    auto acc = [&](int sl, double a, double b) {
        num[sl] = std::max(num[sl], std::fabs(a - b));
        den[sl] = std::max(den[sl], std::fabs(b));
        el[sl] = std::max(el[sl], std::fabs(a - b) / (1e-2 + std::fabs(b)));
    };
    for (int r = 0; r < 2 * B; ++r) {
        const float *pa = &out[0][(size_t)r * 135], *pb = &out[1][(size_t)r * 135];
        for (int e = 0; e < 135; ++e) acc(e < 3 ? 0 : 1, pa[e], pb[e]);
        const float *ba = &out[0][(size_t)2 * B * 135 + (size_t)r * 10], *bbv = &out[1][(size_t)2 * B * 135 + (size_t)r * 10];
        for (int e = 0; e < 10; ++e) acc(2, ba[e], bbv[e]);
        if (std::fabs(pb[2]) > 1e-6 && std::fabs(pa[2]) > 1e-6) {
            acc(3, 1475.0 * pa[0] / pa[2] + 960.0, 1475.0 * pb[0] / pb[2] + 960.0);
            acc(3, 1475.0 * pa[1] / pa[2] + 540.0, 1475.0 * pb[1] / pb[2] + 540.0);
        }
    }
    for (int sl = 0; sl < 4; ++sl) { err8[sl] = den[sl] > 0 ? num[sl] / den[sl] : 0.0; err8[4 + sl] = el[sl]; }
    return AP_OK;
}

int ap_singleview_fwd(ap_net* h, const float* x, const float* bb, const float* pos, const float* init_theta,
                      int theta_bs, const float* init_shape, int shape_bs, int B, int iters, float* pose, float* betas,
                      void* stream) {
    if (!h || !x || !bb || !pos || !pose || !betas) return fail(AP_EINVAL, "ap_singleview_fwd: null argument");
    if (h->variant != 2) return fail(AP_ESTATE, "ap_singleview_fwd needs a copenet_singleview (variant 2) handle");
    if (B <= 0) return fail(AP_EINVAL, "ap_singleview_fwd: bad batch");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->ws_feat.reserve((size_t)B * 2048 * 4));
    float* f = h->ws_feat.as<float>();
    int rc = trunk_fwd(h, x, B, nullptr, 0, f, st);
    if (rc) return rc;
    RegInputs in{f, nullptr, bb, nullptr, pos, nullptr, init_theta, nullptr, init_shape, nullptr, theta_bs, 0, shape_bs, 0};
    return regressor_run(h, in, B, iters, 0, nullptr, 0, 3, pose, betas, nullptr, nullptr, st);
}

// feature-level evaluation of the single-view head: `iters` regressor evaluations from pre-computed trunk features
// (model_copenet_singleview.py:159-170 for iters = 1)
int ap_singleview_reg(ap_net* h, const float* xf, const float* bb, const float* pos, const float* init_theta, int theta_bs,
                      const float* init_shape, int shape_bs, int B, int iters, float* pose, float* betas, void* stream) {
    if (!h || !xf || !bb || !pos || !pose || !betas) return fail(AP_EINVAL, "ap_singleview_reg: null argument");
    if (h->variant != 2) return fail(AP_ESTATE, "ap_singleview_reg needs a copenet_singleview (variant 2) handle");
    if (B <= 0) return fail(AP_EINVAL, "ap_singleview_reg: bad batch");
    RegInputs in{xf, nullptr, bb, nullptr, pos, nullptr, init_theta, nullptr, init_shape, nullptr, theta_bs, 0, shape_bs, 0};
    return regressor_run(h, in, B, iters, 0, nullptr, 0, 3, pose, betas, nullptr, nullptr, (hipStream_t)stream);
}

int ap_muhmr_fwd(ap_net* h, const float* x0, const float* x1, const float* init_cam0, int cam0_bs, const float* init_cam1,
                 int cam1_bs, const float* init_theta0, int theta0_bs, const float* init_theta1, int theta1_bs,
                 const float* init_shape0, int shape0_bs, const float* init_shape1, int shape1_bs, int B, int iters,
                 float* campose0, float* betas0, float* campose1, float* betas1, void* stream) {
    if (!h || !x0 || !x1 || !campose0 || !betas0 || !campose1 || !betas1) return fail(AP_EINVAL, "ap_muhmr_fwd: null argument");
    if (h->variant != 3) return fail(AP_ESTATE, "ap_muhmr_fwd needs a muhmr (variant 3) handle");
    if (B <= 0) return fail(AP_EINVAL, "ap_muhmr_fwd: bad batch");
    if (cam0_bs != cam1_bs) return fail(AP_EINVAL, "ap_muhmr_fwd: init_cam0 / init_cam1 must share their batch stride");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->ws_feat.reserve((size_t)2 * B * 2048 * 4));
    float* f0 = h->ws_feat.as<float>();
    float* f1 = f0 + (size_t)B * 2048;
    int rc = trunk_fwd(h, x0, B, x1, B, f0, st);
    if (rc) return rc;
    const float* c0 = init_cam0 ? init_cam0 : h->mean_cam.as<float>();
    const float* c1 = init_cam1 ? init_cam1 : h->mean_cam.as<float>();
    const int cbs = init_cam0 ? cam0_bs : 0;
    if (!!init_cam0 != !!init_cam1) return fail(AP_EINVAL, "ap_muhmr_fwd: give both initial cameras or neither");
    // bb has zero weight in the re-mapped fc1: any finite [B][3] floats do (the head of the feature rows is at hand)
    RegInputs in{f0, f1, f0, f1, c0, c1, init_theta0, init_theta1, init_shape0, init_shape1, theta0_bs, theta1_bs, shape0_bs, shape1_bs};
    return regressor_run(h, in, B, iters, 1, nullptr, 0, cbs, campose0, betas0, campose1, betas1, st);
}

int ap_copenet_fwd(ap_net* h, const float* x0, const float* x1, const float* bb0, const float* bb1,
                   const float* pos0, const float* pos1, const float* init_theta0, int theta0_bs,
                   const float* init_theta1, int theta1_bs, const float* init_shape0, int shape0_bs,
                   const float* init_shape1, int shape1_bs, int B, int iters, float* pose0, float* betas0,
                   float* pose1, float* betas1, void* stream) {
    if (!h || !x0 || !x1) return fail(AP_EINVAL, "ap_copenet_fwd: null argument");
    if (B <= 0) return fail(AP_EINVAL, "ap_copenet_fwd: bad batch");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->ws_feat.reserve((size_t)2 * B * 2048 * 4));
    float* f0 = h->ws_feat.as<float>();
    float* f1 = f0 + (size_t)B * 2048;
    int rc = trunk_fwd(h, x0, B, x1, B, f0, st);      // both views in one pass (shared weights)
    if (rc) return rc;
    return ap_regressor_fwd(h, f0, f1, bb0, bb1, pos0, pos1, init_theta0, theta0_bs, init_theta1, theta1_bs,
                            init_shape0, shape0_bs, init_shape1, shape1_bs, B, iters, pose0, betas0, pose1, betas1,
                            stream);
}

// model_hmr.copenet.forward_reg (:160-172) from pre-computed features: `iters` evaluations, the raw 6-D pose / shape /
// camera state out (no rot6d conversion)
int ap_hmr_reg(ap_net* h, const float* xf, int B, int iters, const float* pose_in, int pose_bs, const float* shape_in,
               int shape_bs, const float* cam_in, int cam_bs, float* pose_out, float* shape_out, float* cam_out,
               void* stream) {
    if (!h || !xf || B <= 0 || iters < 1 || !pose_out || !shape_out || !cam_out)
        return fail(AP_EINVAL, "ap_hmr_reg: bad argument");
    if (h->variant != 1) return fail(AP_ESTATE, "ap_hmr_reg needs an hmr (variant 1) handle");
    hipStream_t st = (hipStream_t)stream;
    int rc = hmr_ief(h, xf, B, iters, pose_in, pose_bs, shape_in, shape_bs, cam_in, cam_bs, st);
    if (rc) return rc;
    const float* state = h->ws_state.as<float>();
    HIP_TRY(hipMemcpy2DAsync(pose_out, 132 * 4, state, 160 * 4, 132 * 4, B, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpy2DAsync(shape_out, 10 * 4, state + 132, 160 * 4, 10 * 4, B, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpy2DAsync(cam_out, 3 * 4, state + 142, 160 * 4, 3 * 4, B, hipMemcpyDeviceToDevice, st));
    return AP_OK;
}

int ap_hmr_fwd(ap_net* h, const float* x, int B, int iters, const float* init_theta, int theta_bs,
               const float* init_shape, int shape_bs, const float* init_cam, int cam_bs, float* rotmat, float* betas,
               float* cam, void* stream) {
    if (!h || !x || B <= 0 || iters < 1 || !rotmat || !betas || !cam) return fail(AP_EINVAL, "ap_hmr_fwd: bad argument");
    if (h->variant != 1) return fail(AP_ESTATE, "ap_hmr_fwd needs an hmr (variant 1) handle");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->ws_feat.reserve((size_t)B * 2048 * 4));
    float* feat = h->ws_feat.as<float>();
    int rc = trunk_fwd(h, x, B, nullptr, 0, feat, st);
    if (rc) return rc;
    if ((rc = hmr_ief(h, feat, B, iters, init_theta, theta_bs, init_shape, shape_bs, init_cam, cam_bs, st))) return rc;
    float* state = h->ws_state.as<float>();
    HIP_TRY(ap_launch_hmr_output(state, rotmat, betas, cam, B, st));
    return AP_OK;
}

}  // extern "C"
