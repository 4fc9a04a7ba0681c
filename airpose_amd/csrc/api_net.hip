// ap_net handle of libairpose_hip.so: life cycle, weight folding / packing (ap_net_finalize), knobs, range check, timing.
// Declarations and the reference interfaces each entry point replaces: include/airpose_hip.h.
#include "api_internal.h"

thread_local std::string ap_internal::g_err;
int ap_internal::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {

// ---------------------------------------------------------------------------------- packing
const HostTensor* find(const ap_net* h, const std::string& name) {
    const ap_net* src = h->tensors_of ? h->tensors_of : h;
    auto it = src->tensors.find(name);
    return it == src->tensors.end() ? nullptr : &it->second;
}

int bn_fold(const ap_net* h, const std::string& p, int c, std::vector<float>& scale, std::vector<float>& shift) {
    const HostTensor *g = find(h, p + ".weight"), *b = find(h, p + ".bias"), *m = find(h, p + ".running_mean"),
                     *v = find(h, p + ".running_var");
    if (!g || !b || !m || !v) return fail(AP_ESTATE, "missing BatchNorm tensors for " + p);
    if ((int)g->numel() != c || (int)b->numel() != c || (int)m->numel() != c || (int)v->numel() != c)
        return fail(AP_ESHAPE, "BatchNorm size mismatch for " + p);
    const int cp = ((c + 127) / 128) * 128;
    scale.assign(cp, 1.f);
    shift.assign(cp, 0.f);
    for (int i = 0; i < c; ++i) {
        const double s = (double)g->data[i] / std::sqrt((double)v->data[i] + BN_EPS);
        scale[i] = (float)s;
        shift[i] = (float)((double)b->data[i] - (double)m->data[i] * s);
    }
    return AP_OK;
}

// OIHW fp32 -> [cout_pad][kh][kw][cin] in the handle's storage type
int pack_conv(ap_net* h, const std::string& wname, const std::string& bnname, int cin, int cout, int k, int stride,
              int pad, Layer& L) {
    const HostTensor* w = find(h, wname);
    if (!w) return fail(AP_ESTATE, "missing tensor " + wname);
    if (w->shape.size() != 4 || w->shape[0] != cout || w->shape[1] != cin || w->shape[2] != k || w->shape[3] != k)
        return fail(AP_ESHAPE, "shape mismatch for " + wname);
    L.cin = cin; L.cout = cout; L.k = k; L.stride = stride; L.pad = pad;
    L.wld = k * k * cin;
    L.cout_pad = ((cout + 127) / 128) * 128;
    std::vector<float> scale, shift;
    int rc = bn_fold(h, bnname, cout, scale, shift);
    if (rc) return rc;
    const size_t n = (size_t)L.cout_pad * L.wld;
    if (h->half()) {
        std::vector<uint16_t> pk(n, 0);
        for (int o = 0; o < cout; ++o)
            for (int c = 0; c < cin; ++c)
                for (int r = 0; r < k; ++r)
                    for (int s = 0; s < k; ++s)
                        pk[(size_t)o * L.wld + (r * k + s) * cin + c] =
                            h->h16(w->data[(((size_t)o * cin + c) * k + r) * k + s]);
        HIP_TRY(upload(L.w, pk.data(), n * 2));
    } else {
        std::vector<float> pk(n, 0.f);
        for (int o = 0; o < cout; ++o)
            for (int c = 0; c < cin; ++c)
                for (int r = 0; r < k; ++r)
                    for (int s = 0; s < k; ++s)
                        pk[(size_t)o * L.wld + (r * k + s) * cin + c] = w->data[(((size_t)o * cin + c) * k + r) * k + s];
        if (h->prec == AP_PREC_BF16X2) {                    // rows of k*k*cin elements, cin a multiple of 8: planar groups of 8
            std::vector<uint16_t> ps(2 * n);
            host_split_pack_planar(pk.data(), n, ps.data());
            HIP_TRY(upload(L.w, ps.data(), n * 4));
        } else {
            HIP_TRY(upload(L.w, pk.data(), n * 4));
        }
    }
    HIP_TRY(upload(L.scale, scale.data(), scale.size() * 4));
    HIP_TRY(upload(L.shift, shift.data(), shift.size() * 4));
    return AP_OK;
}

// conv3 (1x1, planes -> cout) and the downsample conv (1x1 stride s, inplanes -> cout) of a stage's first block
// share the output: relu(bn3(conv3(t)) + bn_ds(conv_ds(x))).  Fold each BN scale into its weights (fp64) and
// concatenate along K: one GEMM over [t | x(strided)] with shift = shift3 + shift_ds, no residual tensor.
int pack_c3_ds(ap_net* h, const std::string& P, int planes, int inplanes, int stride, Layer& L) {
    const HostTensor *w3 = find(h, P + ".conv3.weight"), *wd = find(h, P + ".downsample.0.weight");
    if (!w3 || !wd) return fail(AP_ESTATE, "missing conv3/downsample weights for " + P);
    const int cout = planes * 4, K1 = planes, K2 = inplanes;
    if ((int)w3->numel() != cout * K1 || (int)wd->numel() != cout * K2) return fail(AP_ESHAPE, "shape mismatch in " + P);
    std::vector<float> s3, h3, sd, hd;
    int rc = bn_fold(h, P + ".bn3", cout, s3, h3);
    if (rc) return rc;
    if ((rc = bn_fold(h, P + ".downsample.1", cout, sd, hd))) return rc;
    L.cin = K1; L.cout = cout; L.k = 1; L.stride = 1; L.pad = 0;
    L.cin2 = K2; L.stride2 = stride;
    L.wld = K1 + K2;
    L.cout_pad = ((cout + 127) / 128) * 128;
    const size_t n = (size_t)L.cout_pad * L.wld;
    std::vector<float> pk(n, 0.f), scale(L.cout_pad, 1.f), shift(L.cout_pad, 0.f);
    for (int o = 0; o < cout; ++o) {
        for (int c = 0; c < K1; ++c) pk[(size_t)o * L.wld + c] = (float)((double)w3->data[(size_t)o * K1 + c] * (double)s3[o]);
        for (int c = 0; c < K2; ++c) pk[(size_t)o * L.wld + K1 + c] = (float)((double)wd->data[(size_t)o * K2 + c] * (double)sd[o]);
        shift[o] = h3[o] + hd[o];
    }
    if (h->half()) {
        std::vector<uint16_t> pb(n);
        for (size_t i = 0; i < n; ++i) pb[i] = h->h16(pk[i]);
        HIP_TRY(upload(L.w, pb.data(), n * 2));
    } else if (h->prec == AP_PREC_BF16X2) {
        std::vector<uint16_t> ps(2 * n);
        host_split_pack_planar(pk.data(), n, ps.data());
        HIP_TRY(upload(L.w, ps.data(), n * 4));
    } else {
        HIP_TRY(upload(L.w, pk.data(), n * 4));
    }
    HIP_TRY(upload(L.scale, scale.data(), scale.size() * 4));
    HIP_TRY(upload(L.shift, shift.data(), shift.size() * 4));
    return AP_OK;
}

// fp32 GEMM operand from rows [out][ld_src] taking columns [col0, col0+ncols); K padded to 32
int pack_linear(const float* W, int ld_src, int col0, int ncols, int nout, const float* bias, Layer& L) {
    L.cin = ((ncols + 31) / 32) * 32;
    L.cout = ((nout + 3) / 4) * 4;
    L.k = 1; L.stride = 1; L.pad = 0;
    L.wld = L.cin;
    L.cout_pad = ((nout + 127) / 128) * 128;
    std::vector<float> pk((size_t)L.cout_pad * L.wld, 0.f), scale(L.cout_pad, 1.f), shift(L.cout_pad, 0.f);
    for (int o = 0; o < nout; ++o) {
        memcpy(&pk[(size_t)o * L.wld], W + (size_t)o * ld_src + col0, (size_t)ncols * 4);
        if (bias) shift[o] = bias[o];
    }
    HIP_TRY(upload(L.w, pk.data(), pk.size() * 4));
    HIP_TRY(upload(L.scale, scale.data(), scale.size() * 4));
    HIP_TRY(upload(L.shift, shift.data(), shift.size() * 4));
    return AP_OK;
}

// every device buffer a trunk block owns (packed rows, BatchNorm vectors, the weight streams of conv_pair / block_img / conv_pw):
// DevBuf has no destructor, so whoever drops a Block releases it first (re-finalize and ap_net_destroy)
void release_layer(Layer& L) { L.w.release(); L.scale.release(); L.shift.release(); L.pw.release(); }
void release_blocks(ap_net* h) {
    for (auto& B : h->blocks) {
        for (Layer* L : {&B.c1, &B.c2, &B.c3, &B.down, &B.c3ds}) release_layer(*L);
        B.pair.release();
        B.imgw.release();
        B.c2img.release();
        B.c2s2.release();
    }
    h->blocks.clear();
}

int finalize_regressor(ap_net* h) {
    const HostTensor *w1 = find(h, "fc1.weight"), *b1 = find(h, "fc1.bias"), *w2 = find(h, "fc2.weight"),
                     *b2 = find(h, "fc2.bias"), *wp = find(h, "decpose.weight"), *bp = find(h, "decpose.bias"),
                     *wsh = find(h, "decshape.weight"), *bsh = find(h, "decshape.bias"), *ip = find(h, "init_pose"),
                     *is = find(h, "init_shape");
    if (!w1 || !b1 || !w2 || !b2 || !wp || !bp || !wsh || !bsh || !ip || !is)
        return fail(AP_ESTATE, "missing regressor tensors (fc1/fc2/decpose/decshape/init_pose/init_shape)");
    if (h->variant == 1) {
        // single-view HMR head (model_hmr.py:160-172): xc = [xf | pose132 | shape10 | cam3] -> fc1 -> fc2 ->
        // decpose/decshape/deccam, all affine: folded like the copenet head into Wf (145 x 2193), bf
        const HostTensor *wc = find(h, "deccam.weight"), *bc = find(h, "deccam.bias"), *ic = find(h, "init_cam");
        if (!wc || !bc || !ic) return fail(AP_ESTATE, "missing deccam / init_cam tensors");
        if (w1->numel() != (size_t)1024 * 2193 || w2->numel() != (size_t)1024 * 1024 || wp->numel() != (size_t)132 * 1024 ||
            wsh->numel() != (size_t)10 * 1024 || wc->numel() != (size_t)3 * 1024 || ip->numel() < 132 || is->numel() != 10)
            return fail(AP_ESHAPE, "hmr regressor tensor shape mismatch");
        std::vector<float> wd((size_t)145 * 1024), bd(145);
        memcpy(wd.data(), wp->data.data(), (size_t)132 * 1024 * 4);
        memcpy(wd.data() + (size_t)132 * 1024, wsh->data.data(), (size_t)10 * 1024 * 4);
        memcpy(wd.data() + (size_t)142 * 1024, wc->data.data(), (size_t)3 * 1024 * 4);
        memcpy(bd.data(), bp->data.data(), 132 * 4);
        memcpy(bd.data() + 132, bsh->data.data(), 10 * 4);
        memcpy(bd.data() + 142, bc->data.data(), 3 * 4);
        std::vector<double> A((size_t)145 * 1024, 0.0);
        for (int o = 0; o < 145; ++o)
            for (int k = 0; k < 1024; ++k) {
                const double wv = wd[(size_t)o * 1024 + k];
                const float* w2r = &w2->data[(size_t)k * 1024];
                double* ar = &A[(size_t)o * 1024];
                for (int j = 0; j < 1024; ++j) ar[j] += wv * w2r[j];
            }
        std::vector<float> wf((size_t)145 * 2193), bfv(145);
        std::vector<double> row(2193);
        for (int o = 0; o < 145; ++o) {
            std::fill(row.begin(), row.end(), 0.0);
            double bacc = bd[o];
            for (int k = 0; k < 1024; ++k) {
                const double av = A[(size_t)o * 1024 + k];
                const float* w1r = &w1->data[(size_t)k * 2193];
                for (int j = 0; j < 2193; ++j) row[j] += av * w1r[j];
                bacc += av * b1->data[k] + (double)wd[(size_t)o * 1024 + k] * b2->data[k];
            }
            for (int j = 0; j < 2193; ++j) wf[(size_t)o * 2193 + j] = (float)row[j];
            bfv[o] = (float)bacc;
        }
        int rc2;
        if ((rc2 = pack_linear(wf.data(), 2193, 0, 2048, 145, bfv.data(), h->fold_feat))) return rc2;
        if ((rc2 = pack_linear(wf.data(), 2193, 2048, 145, 145, nullptr, h->fold_state))) return rc2;
        std::vector<float> mp(144, 0.f);
        memcpy(mp.data(), ip->data.data(), std::min<size_t>(144, ip->numel()) * 4);
        HIP_TRY(upload(h->mean_pose, mp.data(), 144 * 4));
        HIP_TRY(upload(h->mean_shape, is->data.data(), 10 * 4));
        HIP_TRY(upload(h->mean_cam, ic->data.data(), 3 * 4));
        return AP_OK;
    }
    // copenet_singleview (model_copenet_singleview.py:67,156-168): xc = [xf | bb | pose135 | shape10], i.e. the two-view
    // layout without the partner's 136 columns -> the same code with those fc1 columns zero
    HostTensor w1_padded;
    if (h->variant == 2) {
        if (w1->numel() != (size_t)1024 * 2196) return fail(AP_ESHAPE, "copenet_singleview: fc1.weight must be 1024 x 2196");
        w1_padded.shape = {1024, 2332};
        w1_padded.data.assign((size_t)1024 * 2332, 0.f);
        for (int o = 0; o < 1024; ++o)
            memcpy(&w1_padded.data[(size_t)o * 2332], &w1->data[(size_t)o * 2196], (size_t)2196 * 4);
        w1 = &w1_padded;
    }
    // muhmr (model_muhmr.py:67-72,163-197): xc = [xf | cam3 | orient6 | art126 | shape10 | partner 136], decoders
    // decpose (132) / decshape / deccam.  The weak-perspective camera takes the place of the two-view model's
    // translation: cam goes into the `pos` slot (fc1 columns of bb are zero) and deccam's rows are stacked in front of
    // decpose's, so the state row is [cam3 | pose132 | shape10] and the two-view code runs unchanged
    HostTensor wp_stacked, bp_stacked;
    if (h->variant == 3) {
        const HostTensor *wc = find(h, "deccam.weight"), *bc = find(h, "deccam.bias");
        if (!wc || !bc) return fail(AP_ESTATE, "muhmr: missing deccam tensors");
        if (w1->numel() != (size_t)1024 * 2329 || wp->numel() != (size_t)132 * 1024 || wc->numel() != (size_t)3 * 1024 ||
            bp->numel() != 132 || bc->numel() != 3)
            return fail(AP_ESHAPE, "muhmr: fc1.weight must be 1024 x 2329, decpose 132 x 1024, deccam 3 x 1024");
        w1_padded.shape = {1024, 2332};
        w1_padded.data.assign((size_t)1024 * 2332, 0.f);
        for (int o = 0; o < 1024; ++o) {
            const float* src = &w1->data[(size_t)o * 2329];
            float* dst = &w1_padded.data[(size_t)o * 2332];
            memcpy(dst, src, (size_t)2048 * 4);                       // trunk features
            memcpy(dst + 2051, src + 2048, (size_t)(2329 - 2048) * 4);   // cam -> pos slot, then orient .. partner
        }
        w1 = &w1_padded;
        wp_stacked.shape = {135, 1024};
        wp_stacked.data.resize((size_t)135 * 1024);
        memcpy(wp_stacked.data.data(), wc->data.data(), (size_t)3 * 1024 * 4);
        memcpy(wp_stacked.data.data() + (size_t)3 * 1024, wp->data.data(), (size_t)132 * 1024 * 4);
        bp_stacked.shape = {135};
        bp_stacked.data.resize(135);
        memcpy(bp_stacked.data.data(), bc->data.data(), 3 * 4);
        memcpy(bp_stacked.data.data() + 3, bp->data.data(), 132 * 4);
        wp = &wp_stacked;
        bp = &bp_stacked;
    }
    if (w1->numel() != (size_t)1024 * 2332 || w2->numel() != (size_t)1024 * 1024 || wp->numel() != (size_t)135 * 1024 ||
        wsh->numel() != (size_t)10 * 1024 || ip->numel() < 132 || is->numel() != 10)
        return fail(AP_ESHAPE, "regressor tensor shape mismatch");
    int rc;
    if ((rc = pack_linear(w1->data.data(), 2332, 0, 2048, 1024, b1->data.data(), h->fc1_feat))) return rc;
    if ((rc = pack_linear(w1->data.data(), 2332, 2048, 284, 1024, nullptr, h->fc1_state))) return rc;
    if ((rc = pack_linear(w2->data.data(), 1024, 0, 1024, 1024, b2->data.data(), h->fc2))) return rc;
    std::vector<float> wd((size_t)145 * 1024), bd(145);
    memcpy(wd.data(), wp->data.data(), (size_t)135 * 1024 * 4);
    memcpy(wd.data() + (size_t)135 * 1024, wsh->data.data(), (size_t)10 * 1024 * 4);
    memcpy(bd.data(), bp->data.data(), 135 * 4);
    memcpy(bd.data() + 135, bsh->data.data(), 10 * 4);
    if ((rc = pack_linear(wd.data(), 1024, 0, 1024, 145, bd.data(), h->dec))) return rc;
    {
        // forward_reg is fc1 -> dropout(identity in eval) -> fc2 -> dropout -> decpose/decshape with NO activation
        // (model_copenet.py:186-202), i.e. one affine map.  Fold it once in fp64:
        //   Wf = Wd W2 W1 (145 x 2332),  bf = Wd (W2 b1 + b2) + bd
        std::vector<double> A((size_t)145 * 1024, 0.0);                       // Wd W2
        for (int o = 0; o < 145; ++o)
            for (int k = 0; k < 1024; ++k) {
                const double wv = wd[(size_t)o * 1024 + k];
                const float* w2r = &w2->data[(size_t)k * 1024];
                double* ar = &A[(size_t)o * 1024];
                for (int j = 0; j < 1024; ++j) ar[j] += wv * w2r[j];
            }
        std::vector<float> wf((size_t)145 * 2332), bfv(145);
        std::vector<double> row(2332);
        for (int o = 0; o < 145; ++o) {
            std::fill(row.begin(), row.end(), 0.0);
            double bacc = bd[o];
            for (int k = 0; k < 1024; ++k) {
                const double av = A[(size_t)o * 1024 + k];
                const float* w1r = &w1->data[(size_t)k * 2332];
                for (int j = 0; j < 2332; ++j) row[j] += av * w1r[j];
                bacc += av * b1->data[k] + (double)wd[(size_t)o * 1024 + k] * b2->data[k];
            }
            for (int j = 0; j < 2332; ++j) wf[(size_t)o * 2332 + j] = (float)row[j];
            bfv[o] = (float)bacc;
        }
        if ((rc = pack_linear(wf.data(), 2332, 0, 2048, 145, bfv.data(), h->fold_feat))) return rc;
        if ((rc = pack_linear(wf.data(), 2332, 2048, 284, 145, nullptr, h->fold_state))) return rc;
        {   // Guard of the fold on THIS checkpoint: the fp32-rounded folded map against the literal fc1 -> fc2 -> dec chain, both
            // evaluated in fp64 on a fixed probe batch (post-pooling-like features, states around the mean parameters).  The
            // fold is exact algebra; what can go wrong is cancellation -- folded rows whose fp32 rounding error, summed over the
            // 2332 inputs, is visible in the small decoder outputs.  Above 1e-5 of the output scale the handle evaluates the
            // literal chain instead (ap_net_fold_status reports which and why).
            const int NP = 8;
            uint64_t lcg = 0x9E3779B97F4A7C15ull;
            auto unif = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) * (1.0 / 9007199254740992.0); };
            auto gauss = [&]() { const double u = std::max(unif(), 1e-300), v = unif(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); };
            double worst = 0.0, scale = 0.0;
            std::vector<double> x(2332), t1(1024), t2(1024);
            std::vector<double> ylit((size_t)NP * 145), yfold((size_t)NP * 145);
            for (int r = 0; r < NP; ++r) {
                for (int j = 0; j < 2048; ++j) x[j] = std::fabs(gauss()) * 0.8;               // pooled post-ReLU features
                for (int j = 2048; j < 2332; ++j) x[j] = 0.3 * gauss();                        // bb / position / 6-D pose / shape
                for (int j = 0; j < 132 && 2054 + j < 2332; ++j) x[2054 + j] += ip->data[j];  // around the mean pose
                for (int o = 0; o < 1024; ++o) {
                    double acc = b1->data[o];
                    const float* wr = &w1->data[(size_t)o * 2332];
                    for (int j = 0; j < 2332; ++j) acc += (double)wr[j] * x[j];
                    t1[o] = acc;
                }
                for (int o = 0; o < 1024; ++o) {
                    double acc = b2->data[o];
                    const float* wr = &w2->data[(size_t)o * 1024];
                    for (int j = 0; j < 1024; ++j) acc += (double)wr[j] * t1[j];
                    t2[o] = acc;
                }
                for (int o = 0; o < 145; ++o) {
                    double acc = bd[o], accf = bfv[o];
                    const float* wr = &wd[(size_t)o * 1024];
                    for (int j = 0; j < 1024; ++j) acc += (double)wr[j] * t2[j];
                    const float* fr = &wf[(size_t)o * 2332];
                    for (int j = 0; j < 2332; ++j) accf += (double)fr[j] * x[j];
                    ylit[(size_t)r * 145 + o] = acc;
                    yfold[(size_t)r * 145 + o] = accf;
                    scale = std::max(scale, std::fabs(acc));
                    worst = std::max(worst, std::fabs(acc - accf));
                }
            }
            h->fold_check_err = scale > 0.0 ? worst / scale : 0.0;
            const bool was_rejected = h->fold_rejected;
            h->fold_rejected = !(h->fold_check_err <= h->fold_bar);
            if (was_rejected && !h->fold_rejected) h->fold = true;      // re-packed weights pass: back to the default
            if (h->fold_rejected) {
                h->fold = false;
                fprintf(stderr, "airpose_hip: the folded regressor map differs from the literal fc1 -> fc2 -> dec chain by %.3e of the "
                                "output scale on the probe batch (bar %.1e): this handle evaluates the literal chain\n", h->fold_check_err, h->fold_bar);
            }
        }
        {   // k-major copies for the fused IEF kernel
            std::vector<float> tf((size_t)2048 * 148, 0.f), ts((size_t)288 * 148, 0.f), tb(148, 0.f);   // (k padded to 288 with zero rows)
            for (int o = 0; o < 145; ++o) {
                for (int k = 0; k < 2048; ++k) tf[(size_t)k * 148 + o] = wf[(size_t)o * 2332 + k];
                for (int k = 0; k < 284; ++k) ts[(size_t)k * 148 + o] = wf[(size_t)o * 2332 + 2048 + k];
                tb[o] = bfv[o];
            }
            HIP_TRY(upload(h->foldT_feat, tf.data(), tf.size() * 4));
            HIP_TRY(upload(h->foldT_state, ts.data(), ts.size() * 4));
            HIP_TRY(upload(h->fold_bias, tb.data(), tb.size() * 4));
        }
    }
    std::vector<float> mp(144, 0.f);
    memcpy(mp.data(), ip->data.data(), std::min<size_t>(144, ip->numel()) * 4);
    HIP_TRY(upload(h->mean_pose, mp.data(), 144 * 4));
    HIP_TRY(upload(h->mean_shape, is->data.data(), 10 * 4));
    if (h->variant == 3) {
        const HostTensor* ic = find(h, "init_cam");
        if (!ic || ic->numel() != 3) return fail(AP_ESTATE, "muhmr: missing init_cam");
        HIP_TRY(upload(h->mean_cam, ic->data.data(), 3 * 4));
    }
    return AP_OK;
}
}  // namespace

void ap_internal::pack_stem(const float* w, int prec, StemPack& p, bool* f16_overflow) {
    p.direct.assign(147 * 64, 0.f);
    p.pk.assign(64 * AP_STEM_WLD, 0);
    p.pk_lo.clear();
    if (prec == AP_PREC_BF16X2) p.pk_lo.assign(64 * AP_STEM_WLD, 0);
    for (int o = 0; o < 64; ++o)
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 7; ++r)
                for (int s = 0; s < 7; ++s) {
                    const float wv = w[((o * 3 + c) * 7 + r) * 7 + s];
                    p.direct[((r * 7 + s) * 3 + c) * 64 + o] = wv;
                    const int k = o * AP_STEM_WLD + r * 32 + s * 4 + c;
                    p.pk[k] = prec == AP_PREC_F16 ? host_f32_to_f16(wv, f16_overflow) : host_f32_to_bf16(wv);
                    if (prec == AP_PREC_BF16X2) {
                        uint16_t hi;
                        host_split_parts(wv, &hi, &p.pk_lo[k]);
                    }
                }
}

int ap_internal::finalize_trunk(ap_net* h) {
    const HostTensor* w = find(h, "conv1.weight");
    if (!w) return fail(AP_ESTATE, "missing tensor conv1.weight");
    if (w->numel() != 64 * 3 * 49) return fail(AP_ESHAPE, "shape mismatch for conv1.weight");
    {
        StemPack sp;
        pack_stem(w->data.data(), h->prec, sp, &h->f16_overflow);
        HIP_TRY(upload(h->stem_w, sp.direct.data(), sp.direct.size() * 4));
        HIP_TRY(upload(h->stem_wpk, sp.pk.data(), sp.pk.size() * 2));
        if (h->prec == AP_PREC_BF16X2) HIP_TRY(upload(h->stem_wpk_lo, sp.pk_lo.data(), sp.pk_lo.size() * 2));
    }
    std::vector<float> sc, sh;
    int rc = bn_fold(h, "bn1", 64, sc, sh);
    if (rc) return rc;
    HIP_TRY(upload(h->stem_scale, sc.data(), sc.size() * 4));
    HIP_TRY(upload(h->stem_shift, sh.data(), sh.size() * 4));

    static const int layers[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
    HIP_TRY(hipDeviceSynchronize());                        // (a re-finalize: no pass of the previous packing may still be in flight)
    release_blocks(h);
    h->blocks.resize(16);
    int inpl = 64, bi_all = 0;
    for (int li = 0; li < 4; ++li)
        for (int bi = 0; bi < layers[li]; ++bi, ++bi_all) {
            char p[64];
            snprintf(p, sizeof p, "layer%d.%d", li + 1, bi);
            const std::string P(p);
            const int pl = planes[li], stride = (bi == 0 && li > 0) ? 2 : 1;
            ap_net::Block& B = h->blocks[bi_all];
            if ((rc = pack_conv(h, P + ".conv1.weight", P + ".bn1", inpl, pl, 1, 1, 0, B.c1))) return rc;
            if ((rc = pack_conv(h, P + ".conv2.weight", P + ".bn2", pl, pl, 3, stride, 1, B.c2))) return rc;
            if ((rc = pack_conv(h, P + ".conv3.weight", P + ".bn3", pl, pl * 4, 1, 1, 0, B.c3))) return rc;
            B.has_down = bi == 0;
            if (B.has_down) {
                if ((rc = pack_conv(h, P + ".downsample.0.weight", P + ".downsample.1", inpl, pl * 4, 1, stride, 0,
                                    B.down)))
                    return rc;
                if ((rc = pack_c3_ds(h, P, pl, inpl, stride, B.c3ds))) return rc;
            }
            inpl = pl * 4;
        }
    // conv3 of a block + conv1 of the next block (conv_pair.hip): the two weight matrices as one stream of 16-KiB tiles in
    // the order the fused kernel consumes them, built on the device from the rows packed above.  Identity blocks: conv3 +
    // identity; stage-first blocks: conv3 with the downsample branch folded in as a second K segment (pack_c3_ds), with the
    // next conv1 where the registers allow, alone otherwise
    if (h->half())
        for (size_t b = 0; b + 1 < h->blocks.size(); ++b) {
            ap_net::Block &A = h->blocks[b], &N = h->blocks[b + 1];
            const Layer& L3 = A.has_down ? A.c3ds : A.c3;
            const int P = L3.cin, P2 = A.has_down ? L3.cin2 : 0, C3 = L3.cout;
            int N1 = N.c1.cout;
            if (N.c1.cin != C3) continue;
            if (!k_bf16::ap_conv_pair_supported(P, P2, C3, N1)) N1 = 0;
            if (!k_bf16::ap_conv_pair_supported(P, P2, C3, N1)) continue;
            HIP_TRY(A.pair.reserve(k_bf16::ap_conv_pair_stream_bytes(P, P2, C3, N1)));
            HIP_TRY(H16(h->prec, ap_launch_pair_pack)(L3.w.p, N1 ? N.c1.w.p : nullptr, A.pair.p, P, P2, C3, N1, nullptr));
            A.pair_p = P; A.pair_p2 = P2; A.pair_c3 = C3; A.pair_n1 = N1;
        }
    // layer3 identity blocks (1024 -> 256 -> 256 -> 1024 at 14 x 14): weight streams of the image-resident kernel
    if (h->half())
        for (auto& B : h->blocks) {
            if (B.has_down || B.c1.cin != 1024 || B.c1.cout != 256 || B.c2.cout != 256 || B.c2.stride != 1 || B.c3.cout != 1024) continue;
            HIP_TRY(B.imgw.reserve(k_bf16::ap_block_img_stream_bytes()));
            HIP_TRY(H16(h->prec, ap_launch_block_img_pack)(B.c1.w.p, B.c2.w.p, B.c3.w.p, B.imgw.p, nullptr));
        }
    // stride-1 3 x 3 of the 28 x 28 stage (layer2.1 - 2.3 conv2): weight streams of the half-image-resident kernel
    if (h->half())
        for (auto& B : h->blocks) {
            const Layer& L = B.c2;
            if (!k_bf16::ap_conv_img3_supported(28, 28, L.cin, L.cout, L.k, L.stride, L.pad) || L.wld != 9 * L.cin) continue;
            HIP_TRY(B.c2img.reserve(k_bf16::ap_conv_img3_stream_bytes()));
            HIP_TRY(H16(h->prec, ap_launch_conv_img3_pack)(L.w.p, B.c2img.p, nullptr));
        }
    // stride-2 3 x 3 of layer2.0 (56 x 56 -> 28 x 28, 128 channels): weight streams of the polyphase kernel
    if (h->half())
        for (auto& B : h->blocks) {
            const Layer& L = B.c2;
            if (!k_bf16::ap_conv_s2p_supported(56, 56, L.cin, L.cout, L.k, L.stride, L.pad) || L.wld != 9 * L.cin) continue;
            HIP_TRY(B.c2s2.reserve(k_bf16::ap_conv_s2p_stream_bytes()));
            HIP_TRY(H16(h->prec, ap_launch_conv_s2p_pack)(L.w.p, B.c2s2.p, nullptr));
        }
    // pointwise layers of the 14 x 14 and 7 x 7 stages: weight streams of conv_pw.hip (conv1, and conv3 of the identity blocks)
    if (h->half())
        for (auto& B : h->blocks)
            for (Layer* L : {&B.c1, &B.c3}) {
                if (L->k != 1 || L->stride != 1 || L->cin2 || L->cin < 256 || L->cin % 128 || L->cout % 256 || (L == &B.c3 && B.has_down)) continue;
                if (L->cin * L->cout < 1024 * 256) continue;             // (layer1 / layer2: HBM-bound, and covered by the fused kernels)
                HIP_TRY(L->pw.reserve(k_bf16::ap_conv_pw_stream_bytes(L->cin, L->cout)));
                HIP_TRY(H16(h->prec, ap_launch_conv_pw_pack)(L->w.p, L->pw.p, L->cin, L->cout, L->wld, nullptr));
            }
    // ... conv2 of layer3.0 / layer4.0 (3 x 3, stride 2: K = [tap][Cin], consumed as nine pointwise taps)
    if (h->half())
        for (auto& B : h->blocks) {
            Layer& L = B.c2;
            const int cc = L.cin >> 6;
            if (L.k != 3 || L.stride != 2 || L.pad != 1 || L.cin % 64 || cc < 2 || (cc & (cc - 1)) || L.cout % 256) continue;
            HIP_TRY(L.pw.reserve(k_bf16::ap_conv_pw_stream_bytes(9 * L.cin, L.cout)));
            HIP_TRY(H16(h->prec, ap_launch_conv_pw_pack)(L.w.p, L.pw.p, 9 * L.cin, L.cout, L.wld, nullptr));
        }
    // ... and conv3 + folded downsample of layer4.0 (K = [t2: 512 | x sampled with stride 2: 1024]; layer3.0's rides in a pair kernel)
    if (h->half() && h->fuse_ds)
        for (auto& B : h->blocks) {
            Layer& L = B.c3ds;
            if (!B.has_down || B.pair_p || !L.w.p || L.cin % 64 || L.cin2 % 64 || (L.cin + L.cin2) % 128 || L.cout % 256 || L.cin + L.cin2 < 1024) continue;
            HIP_TRY(L.pw.reserve(k_bf16::ap_conv_pw_stream_bytes(L.cin + L.cin2, L.cout)));
            HIP_TRY(H16(h->prec, ap_launch_conv_pw_pack)(L.w.p, L.pw.p, L.cin + L.cin2, L.cout, L.wld, nullptr));
        }
    HIP_TRY(hipDeviceSynchronize());
    return AP_OK;
}

extern "C" {

const char* ap_version(void) { return "airpose_hip 0.7 (gfx950; abi 13)"; }
int ap_abi_version(void) { return AP_ABI_VERSION; }
const char* ap_last_error(void) { return g_err.c_str(); }

int ap_net_create(ap_net** out, int device, int precision, int variant) {
    if (!out || !prec_valid(precision) || (variant < 0 || variant > 3))
        return fail(AP_EINVAL, "ap_net_create: bad arguments");
    HIP_TRY(hipSetDevice(device));
    ap_net* h = new ap_net();
    h->device = device; h->prec = precision; h->variant = variant;
    if (precision == AP_PREC_F16) {
        hipError_t e = hipHostMalloc((void**)&h->range_flag, 4 * sizeof(int), hipHostMallocMapped);
        if (e != hipSuccess) { delete h; return fail((int)e, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
        for (int q = 0; q < 4; ++q) h->range_flag[q] = 0;
        e = hipHostMalloc((void**)&h->range_slots, AP_RANGE_SLOTS * 4 * sizeof(int), hipHostMallocMapped);
        if (e != hipSuccess) { (void)hipHostFree(h->range_flag); delete h; return fail((int)e, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
        for (int i = 0; i < AP_RANGE_SLOTS * 4; ++i) h->range_slots[i] = 0;
        for (int q = 0; q < 4; ++q) h->tw[q].rflag = h->range_flag + q;
    }
    *out = h;
    return AP_OK;
}

void ap_net_destroy(ap_net* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (DevBuf* b : {&h->stem_w, &h->stem_wpk, &h->stem_wpk_lo, &h->stem_scale, &h->stem_shift, &h->mean_pose, &h->mean_shape, &h->mean_cam, &h->tw[0].ws_stem, &h->tw[0].ws_a,
                      &h->tw[0].ws_b, &h->tw[0].ws_t1, &h->tw[0].ws_t2, &h->tw[0].ws_ds, &h->tw[1].ws_stem, &h->tw[1].ws_a, &h->tw[1].ws_b,
                      &h->tw[1].ws_t1, &h->tw[1].ws_t2, &h->tw[1].ws_ds, &h->tw[2].ws_stem, &h->tw[2].ws_a, &h->tw[2].ws_b, &h->tw[2].ws_t1,
                      &h->tw[2].ws_t2, &h->tw[2].ws_ds, &h->tw[3].ws_stem, &h->tw[3].ws_a, &h->tw[3].ws_b, &h->tw[3].ws_t1, &h->tw[3].ws_t2,
                      &h->tw[3].ws_ds, &h->ws_feat, &h->ws_H, &h->ws_S, &h->ws_T1, &h->ws_T2,
                      &h->ws_D, &h->ws_state})
        b->release();
    auto rel = [](Layer& L) { release_layer(L); };
    release_blocks(h);
    rel(h->fc1_feat); rel(h->fc1_state); rel(h->fc2); rel(h->dec); rel(h->fold_feat); rel(h->fold_state);
    h->foldT_feat.release(); h->foldT_state.release(); h->fold_bias.release();
    h->tm.destroy();
    for (int i = 0; i < 4; ++i) {
        if (h->aux[i]) (void)hipStreamDestroy(h->aux[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_skew) (void)hipEventDestroy(h->ev_skew);
    if (h->range_flag) (void)hipHostFree(h->range_flag);
    if (h->range_slots) (void)hipHostFree(h->range_slots);
    if (h->probe_ref) { ap_net* r = h->probe_ref; h->probe_ref = nullptr; ap_net_destroy(r); }
    for (DevBuf* b : {&h->probe_x, &h->probe_bb, &h->probe_pos, &h->probe_feat, &h->probe_out}) b->release();
    delete h;
}

int ap_net_set_tensor(ap_net* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    if (!h || !name || !host_data || ndim < 0 || ndim > 8) return fail(AP_EINVAL, "ap_net_set_tensor: bad arguments");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return fail(AP_ESHAPE, "negative dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(host_data, host_data + n);
    h->tensors[name] = std::move(t);
    h->finalized = false;
    return AP_OK;
}

int ap_net_finalize(ap_net* h) {
    if (!h) return fail(AP_EINVAL, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    h->f16_overflow = false;
    if (h->probe_ref) { ap_net* r = h->probe_ref; h->probe_ref = nullptr; ap_net_destroy(r); }   // (packed from the previous tensors)
    int rc = finalize_trunk(h);
    if (rc) return rc;
    if ((rc = finalize_regressor(h))) return rc;
    // fp16 storage: a BatchNorm-folded weight above 65 504 would become inf on the device
    if (h->f16_overflow)
        return fail(AP_ESHAPE, "ap_net_finalize: a (BatchNorm-folded) weight exceeds the fp16 range of AP_PREC_F16; "
                               "use AP_PREC_BF16 (precision='bf16': fp32's exponent range)");
    h->finalized = true;
    return AP_OK;
}

int ap_net_precision(const ap_net* h) { return h ? h->prec : AP_EINVAL; }

int ap_net_set_range_check(ap_net* h, int mode) {
    if (!h || mode < 0 || mode > 2) return fail(AP_EINVAL, "ap_net_set_range_check: handle, mode in {0, 1, 2}");
    h->range_mode = mode;
    return AP_OK;
}

int ap_net_range_status(ap_net* h, void* stream, int reset) {
    if (!h) return fail(AP_EINVAL, "null handle");
    if (!h->range_flag) return AP_OK;                        // only fp16 storage has a range to leave
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const int bad = h->range_any();
    if (reset) for (int q = 0; q < 4; ++q) __atomic_store_n(h->range_flag + q, 0, __ATOMIC_RELAXED);
    if (bad) return fail(AP_ERANGE, "AP_PREC_F16: a trunk pass produced non-finite features (a stored activation left the fp16 range)");
    return AP_OK;
}

int ap_net_range_peek(const ap_net* h) {
    if (!h) return fail(AP_EINVAL, "null handle");
    if (h->range_any())
        return fail(AP_ERANGE, "AP_PREC_F16: a trunk pass of this handle left the fp16 range (flag read without a stream sync)");
    return AP_OK;
}

int ap_net_range_mark_next(ap_net* h, int slot) {
    if (!h || slot < -1 || slot >= AP_RANGE_SLOTS) return fail(AP_EINVAL, "ap_net_range_mark_next: handle, slot in [-1, AP_RANGE_SLOTS)");
    h->mark_slot = h->range_flag ? slot : -1;
    // (the slot's previous batch is done -- the caller waited for it before reusing the slot -- so the host may clear its words)
    if (h->mark_slot >= 0) for (int q = 0; q < 4; ++q) __atomic_store_n(h->range_slots + 4 * slot + q, 0, __ATOMIC_RELAXED);
    return AP_OK;
}

int ap_net_range_slot(const ap_net* h, int slot) {
    if (!h || slot < 0 || slot >= AP_RANGE_SLOTS) return fail(AP_EINVAL, "ap_net_range_slot: handle, slot in [0, AP_RANGE_SLOTS)");
    int v = 0;
    if (h->range_slots) for (int q = 0; q < 4; ++q) v |= __atomic_load_n(h->range_slots + 4 * slot + q, __ATOMIC_RELAXED);
    if (v)
        return fail(AP_ERANGE, "AP_PREC_F16: a stored activation of this batch's trunk passes (or of an earlier batch's) left the fp16 "
                               "range; use precision bf16 / bf16x2 for this checkpoint");
    return AP_OK;
}

int ap_net_enable_timing(ap_net* h, int on) {
    if (!h || on < 0 || on > 2) return fail(AP_EINVAL, "ap_net_enable_timing: handle, on in {0, 1, 2}");
    h->tm.on = on;
    return AP_OK;
}

int ap_net_timing(ap_net* h, double ms[4], int64_t* passes, int reset) {
    if (!h || !ms || !passes) return fail(AP_EINVAL, "ap_net_timing: null argument");
    HIP_TRY(h->tm.collect(ms, 4, passes, reset != 0));
    return AP_OK;
}

// Knob setters that only store their argument: a null handle is AP_EINVAL, `value` is what the knob keeps of `on`
#define AP_NET_SETTER(knob, value) \
    int ap_net_set_##knob(ap_net* h, int on) { if (!h) return fail(AP_EINVAL, "null handle"); h->knob = (value); return AP_OK; }
#define AP_NET_FLAG(knob) AP_NET_SETTER(knob, on != 0)
#define AP_NET_LEVEL(knob, top) AP_NET_SETTER(knob, on < 0 ? 0 : (on > (top) ? (top) : on))
AP_NET_FLAG(fuse_ds)
AP_NET_FLAG(fuse_block)
AP_NET_FLAG(fuse_pair)
AP_NET_FLAG(fuse_tail)
AP_NET_LEVEL(pw_conv, 4)                                     // (3: 1 without the size rule; 4: 1 without the 3 x 3 / stride-2 layers -- A/B aids)
AP_NET_FLAG(s2p)
AP_NET_LEVEL(img3, 2)
AP_NET_LEVEL(img_block, 2)
AP_NET_FLAG(even_out)
AP_NET_FLAG(fuse_ief)
AP_NET_FLAG(fuse_pool)
AP_NET_FLAG(tiled)
AP_NET_SETTER(fuse_stem, on == 2 ? 2 : on != 0)

int ap_net_set_fold(ap_net* h, int on) {
    if (!h) return fail(AP_EINVAL, "null handle");
    if (on && h->fold_rejected) {
        // a remembered knob re-applied to a checkpoint the probe rejects (copenet._set_knob) must not turn every later call
        // into an error: the literal chain stays, ap_net_fold_status says why
        fprintf(stderr, "airpose_hip: ap_net_set_fold(1) ignored -- ap_net_finalize rejected the fold for this checkpoint "
                        "(ap_net_fold_status); the handle keeps evaluating the literal fc1 -> fc2 -> dec chain\n");
        return AP_OK;
    }
    h->fold = on != 0;
    return AP_OK;
}

int ap_net_set_fold_bar(ap_net* h, double bar) {
    if (!h || !(bar >= 0.0)) return fail(AP_EINVAL, "ap_net_set_fold_bar: handle, bar >= 0");
    h->fold_bar = bar;
    // the bar is applied by the regressor's finalize step (the fold probe): re-run THAT step when the handle holds a packed
    // checkpoint -- behind a device sync (passes in flight read the maps it rebuilds), and with the handle marked un-finalized
    // while it runs, so a failure leaves it in a state every later call reports
    if (h->finalized) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipDeviceSynchronize());
        h->finalized = false;
        const int rc = finalize_regressor(h);
        if (rc) return rc;
        h->finalized = true;
    }
    return AP_OK;
}

int ap_net_fold_status(const ap_net* h, double* probe_rel_err) {
    if (!h) return fail(AP_EINVAL, "null handle");
    if (probe_rel_err) *probe_rel_err = h->fold_check_err;
    return h->fold_rejected ? 0 : (h->fold ? 1 : 2);
}

int ap_net_set_dual_stream(ap_net* h, int on) {
    if (!h) return fail(AP_EINVAL, "null handle");
    h->dual_stream = on != 0;
    h->passes_per_view = on == 100 ? 2 : 1;                  // (tuning: 100 = four half passes)
    h->dual_skew = (on > 1 && on < 100) ? on - 1 : 0;        // (tuning: on = 1 + skew point)
    return AP_OK;
}

int ap_net_set_chunk(ap_net* h, int images_per_chunk) {
    if (!h || images_per_chunk < 0) return fail(AP_EINVAL, "ap_net_set_chunk: bad argument");
    // kernels address an activation tensor of one chunk with 32-bit byte offsets in places (folded downsample segment,
    // fused layer1 bottleneck): 1024 images keep every tensor of the pass below 4 GiB in both storage types
    if (images_per_chunk > 1024) return fail(AP_EINVAL, "ap_net_set_chunk: at most 1024 images per chunk");
    h->chunk = images_per_chunk;
    return AP_OK;
}

}  // extern "C"
