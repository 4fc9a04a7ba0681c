// ap_smplx handle of libairpose_hip.so: model packing, the forward driver (smplx_run) and the backward driver.
#include "api_internal.h"


namespace {

int smplx_run(ap_smplx* h, SmplxFwdArgs a, bool body_only, hipStream_t st) {
    h->m.coef_split = h->blend_split ? 1 : 0;
    const SmplxModelDev& m = h->m;
    const int n = a.n;
    HIP_TRY(h->ws_coef.reserve((size_t)n * m.ncoef * 4));
    HIP_TRY(h->ws_A.reserve((size_t)n * m.J * 12 * 4));
    HIP_TRY(h->ws_jposed.reserve((size_t)n * m.J * 3 * 4));
    HIP_TRY(h->ws_post.reserve((size_t)n * 12 * 4));
    // body-only pose feature, 4 bones per vertex, split-bf16 coefficients: contraction + skinning in ONE kernel (v_posed stays
    // on the chip); anything else (hand / face poses: K = 512, more bones per vertex, the fp32 contraction) takes the two kernels
    const bool fused = h->fused && h->blend_split && body_only && ap_smplx_lbs_fused_supported(m);
    if (fused) HIP_TRY(h->ws_side.reserve((size_t)n * m.n_jv * 3 * 4));
    else HIP_TRY(h->ws_vposed.reserve((size_t)n * m.ldv * 4));
    a.dbg = g_conv_dbg;
    a.grp_cnt = nullptr;
    if (fused && h->fuse_joints) {
        const size_t need = (size_t)((n + 31) / 32) * 4;
        if (need > h->ws_cnt.bytes) {                        // (re)allocated: zero once; every launch leaves the counters at zero
            HIP_TRY(h->ws_cnt.reserve(need < 4096 ? 4096 : need));
            HIP_TRY(hipMemsetAsync(h->ws_cnt.p, 0, h->ws_cnt.bytes, st));
        }
        a.grp_cnt = h->ws_cnt.as<int>();
    }
    a.coef = h->ws_coef.as<float>(); a.A = h->ws_A.as<float>(); a.jposed = h->ws_jposed.as<float>();
    a.post = (a.pose6d || a.post_rt) ? h->ws_post.as<float>() : nullptr;
    a.A22 = nullptr;
    if (fused && h->fold_post && h->merge_bones && a.post && !a.transl && !a.grp_cnt && m.nb == 22) {
        HIP_TRY(h->ws_A22.reserve((size_t)n * 22 * 12 * 4));
        a.A22 = h->ws_A22.as<float>();
    }
    a.vposed = h->ws_vposed.as<float>();
    a.vp_side = fused ? h->ws_side.as<float>() : nullptr;
    if (a.n_main > 0 && a.intr0) {                           // camera centres resolved by the prep kernel
        HIP_TRY(h->ws_cc.reserve((size_t)a.n_main * 2 * 4));
        a.cc_ws = h->ws_cc.as<float>();
        a.cam_center = a.cc_ws;
    }
    size_t ev[5] = {0, 0, 0, 0, 0};
    // tm.on == 1: an event between every two kernels (per-stage times; each record costs a bubble of several microseconds on the
    // stream); 2: one event in front of the first kernel and one behind the last (the tail's span, no bubbles inside: reported in slot 0)
    const bool stages = h->tm.on == 1;
    if (h->tm.on) HIP_TRY(h->tm.rec(st, &ev[0]));
    HIP_TRY(ap_launch_smplx_prep(m, a, st));
    if (stages) HIP_TRY(h->tm.rec(st, &ev[1]));
    if (fused) {
        int dev = 0, n_cu = 0;
        HIP_TRY(ap_device(&dev, &n_cu));
        HIP_TRY(ap_launch_smplx_lbs_fused(m, a, n_cu, h->merge_bones, st));
        if (stages) { HIP_TRY(h->tm.rec(st, &ev[2])); ev[3] = ev[2]; }        // stage 1 = the fused kernel, stage 2 empty
    } else {
        // v_posed = v_template + [betas | expr | pose_feature] . dirs^T; hand/face rows of the pose feature are
        // identically zero when no extra pose is supplied, so the contraction stops after the 21 body joints
        int K = body_only ? 20 + 21 * 9 : 20 + (m.J - 1) * 9;
        K = ((K + 31) / 32) * 32;
        ConvArgs g{};
        g.x = a.coef; g.w = h->blend_split ? h->dirs_split.p : h->dirs.w.p;
        g.scale = h->dirs.scale.as<float>(); g.shift = h->dirs.shift.as<float>();
        g.out_f32 = 1;                                       // v_posed stays fp32 (only the split kind reads the flag)
        g.res = nullptr; g.y = h->ws_vposed.p;
        g.N = n; g.H = g.W = g.Ho = g.Wo = 1; g.Cin = K; g.Cout = h->dirs.cout; g.KH = g.KW = 1; g.stride = 1; g.pad = 0;
        g.M = n; g.ldx = m.ncoef; g.ldy = m.ldv; g.ldr = 0; g.wld = h->dirs.wld; g.relu = 0;
        HIP_TRY(dispatch_conv(g, h->blend_split ? AP_PREC_BF16X2 : AP_PREC_FP32, st));
        if (stages) HIP_TRY(h->tm.rec(st, &ev[2]));
        HIP_TRY(ap_launch_smplx_skin(m, a, st));
        if (stages) HIP_TRY(h->tm.rec(st, &ev[3]));
    }
    if (!a.grp_cnt) HIP_TRY(ap_launch_smplx_joints(m, a, st));
    if (h->tm.on) {
        HIP_TRY(h->tm.rec(st, &ev[4]));
        if (stages) for (int s = 0; s < 4; ++s) { h->tm.marks[s].push_back(ev[s]); h->tm.marks[s].push_back(ev[s + 1]); }
        else { h->tm.marks[0].push_back(ev[0]); h->tm.marks[0].push_back(ev[4]); }
        h->tm.passes++;
    }
    return AP_OK;
}

// ---- backward
template <typename T> hipError_t download(std::vector<T>& dst, const DevBuf& src, size_t count) {
    dst.resize(std::max<size_t>(count, 1));
    return hipMemcpy(dst.data(), src.p, count * sizeof(T), hipMemcpyDeviceToHost);
}

// tables of the first backward, built from what the handle already holds on the device: the skinning entries bone-major
// (ascending vertex, zero weights dropped) with each bone's start per vertex range, and per joint-vertex slot the output joints
// it feeds (vertex picks: weight 1; landmarks: barycentric weight) in output-joint order
hipError_t smplx_bwd_tables(ap_smplx* h) {
    if (h->bw_ready) return hipSuccess;
    const SmplxModelDev& m = h->m;
    const int V = m.V, J = m.J, K = m.K, nr = (V + SMPLX_BWD_RV - 1) / SMPLX_BWD_RV;
    std::vector<int> sidx, slot, ev, tri;
    std::vector<float> sw, bary;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = download(sidx, h->skin_idx, (size_t)V * K);
    if (e == hipSuccess) e = download(sw, h->skin_w, (size_t)V * K);
    if (e == hipSuccess) e = download(slot, h->jv_slot, V);
    if (e == hipSuccess) e = download(ev, h->extra_verts, m.n_extra);
    if (e == hipSuccess) e = download(tri, h->lmk_tri, (size_t)m.n_lmk * 3);
    if (e == hipSuccess) e = download(bary, h->lmk_bary, (size_t)m.n_lmk * 3);
    if (e != hipSuccess) return e;
    std::vector<std::vector<int2>> per_bone(J);
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < K; ++k) {
            const float w = sw[(size_t)v * K + k];
            if (w == 0.f) continue;
            int wb;
            memcpy(&wb, &w, 4);
            per_bone[sidx[(size_t)v * K + k]].push_back(make_int2(v, wb));
        }
    std::vector<int2> ent;
    std::vector<int> off((size_t)J * (nr + 1));
    for (int j = 0; j < J; ++j) {
        size_t i = 0;
        for (int r = 0; r <= nr; ++r) {
            while (i < per_bone[j].size() && per_bone[j][i].x < r * SMPLX_BWD_RV) ++i;
            off[(size_t)j * (nr + 1) + r] = (int)(ent.size() + i);
        }
        ent.insert(ent.end(), per_bone[j].begin(), per_bone[j].end());
    }
    std::vector<std::vector<int2>> per_slot(m.n_jv);
    auto add = [&](int v, int t, float w) {
        int wb;
        memcpy(&wb, &w, 4);
        per_slot[slot[v]].push_back(make_int2(t, wb));
    };
    for (int t = 0; t < m.n_extra; ++t) add(ev[t], J + t, 1.f);
    for (int l = 0; l < m.n_lmk; ++l)
        for (int f = 0; f < 3; ++f) add(tri[l * 3 + f], J + m.n_extra + l, bary[l * 3 + f]);
    std::vector<int2> jent;
    std::vector<int> joff(m.n_jv + 1);
    for (int s = 0; s < m.n_jv; ++s) {
        joff[s] = (int)jent.size();
        jent.insert(jent.end(), per_slot[s].begin(), per_slot[s].end());
    }
    joff[m.n_jv] = (int)jent.size();
    if (ent.empty()) ent.push_back(make_int2(0, 0));
    if (jent.empty()) jent.push_back(make_int2(0, 0));
    e = upload(h->bw_bone_off, off.data(), off.size() * 4);
    if (e == hipSuccess) e = upload(h->bw_bone_ent, ent.data(), ent.size() * sizeof(int2));
    if (e == hipSuccess) e = upload(h->bw_jv_off, joff.data(), joff.size() * 4);
    if (e == hipSuccess) e = upload(h->bw_jv_ent, jent.data(), jent.size() * sizeof(int2));
    if (e != hipSuccess) return e;
    h->bw_nr = nr;
    h->bw_ready = true;
    return hipSuccess;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------- SMPL-X
int ap_smplx_create(ap_smplx** out, const ap_smplx_model* md, int device) {
    if (!out || !md) return fail(AP_EINVAL, "ap_smplx_create: null argument");
    const int V = md->num_verts, J = md->num_joints, NS = md->num_shape_coeffs;
    if (V <= 0 || J <= 1 || J > 64 || NS != 20 || md->num_extra < 0 || md->num_landmarks < 0 ||
        J + md->num_extra + md->num_landmarks > 128)
        return fail(AP_ESHAPE, "ap_smplx_create: unsupported model dimensions");
    if (!md->v_template || !md->shapedirs || !md->posedirs || !md->J_regressor || !md->parents || !md->lbs_weights ||
        (md->num_landmarks && (!md->faces || !md->lmk_faces_idx || !md->lmk_bary_coords)) ||
        (md->num_extra && !md->extra_joint_verts))
        return fail(AP_EINVAL, "ap_smplx_create: null model array");
    HIP_TRY(hipSetDevice(device));
    ap_smplx* h = new ap_smplx();
    h->device = device;
    SmplxModelDev& m = h->m;
    m.V = V; m.J = J; m.ncoef = 512;
    const int NP = (J - 1) * 9;
    if (20 + NP > m.ncoef) { delete h; return fail(AP_ESHAPE, "too many pose features"); }
    // rest joints as an affine function of the shape coefficients (exact algebra, done in fp64):
    //   J = J_regressor (v_template + shapedirs c) = J_template + J_shapedirs c
    std::vector<float> jt((size_t)J * 3), jsd((size_t)J * 3 * 20);
    for (int j = 0; j < J; ++j) {
        double t[3] = {0, 0, 0};
        std::vector<double> sd(60, 0.0);
        for (int v = 0; v < V; ++v) {
            const double r = md->J_regressor[(size_t)j * V + v];
            if (r == 0.0) continue;
            for (int c = 0; c < 3; ++c) {
                t[c] += r * md->v_template[(size_t)v * 3 + c];
                for (int l = 0; l < 20; ++l) sd[c * 20 + l] += r * md->shapedirs[((size_t)v * 3 + c) * 20 + l];
            }
        }
        for (int c = 0; c < 3; ++c) {
            jt[j * 3 + c] = (float)t[c];
            for (int l = 0; l < 20; ++l) jsd[((size_t)j * 3 + c) * 20 + l] = (float)sd[c * 20 + l];
        }
    }
    // kinematic tree
    std::vector<int> par(J), dep(J, 0);
    int maxd = 0;
    for (int j = 0; j < J; ++j) {
        par[j] = j == 0 ? -1 : (int)md->parents[j];
        if (j > 0 && (par[j] < 0 || par[j] >= j)) { delete h; return fail(AP_ESHAPE, "parents must satisfy 0 <= parent < child"); }
        dep[j] = j == 0 ? 0 : dep[par[j]] + 1;
        maxd = std::max(maxd, dep[j]);
    }
    m.max_depth = maxd;
    // sparse skinning weights, ascending bone index, K = max non-zeros per vertex (4 / 8 / exact)
    int K = 1;
    for (int v = 0; v < V; ++v) {
        int nz = 0;
        for (int j = 0; j < J; ++j) nz += md->lbs_weights[(size_t)v * J + j] != 0.f;
        K = std::max(K, nz);
    }
    K = K <= 4 ? 4 : (K <= 8 ? 8 : K);
    m.K = K;
    std::vector<int> sidx((size_t)V * K, 0);
    std::vector<float> sw((size_t)V * K, 0.f);
    for (int v = 0; v < V; ++v) {
        int k = 0;
        for (int j = 0; j < J; ++j) {
            const float w = md->lbs_weights[(size_t)v * J + j];
            if (w != 0.f) { sidx[(size_t)v * K + k] = j; sw[(size_t)v * K + k] = w; ++k; }
        }
    }
    // blend-shape operand: row n = 3v+c, columns [20 shape/expr | (J-1)*9 pose | 0 pad]; shift = v_template
    Layer& L = h->dirs;
    const int rows = 3 * V;
    L.cin = m.ncoef; L.k = 1; L.stride = 1; L.pad = 0; L.wld = m.ncoef;
    L.cout = ((rows + 3) / 4) * 4;
    L.cout_pad = ((rows + 127) / 128) * 128;
    m.ldv = L.cout_pad;
    {
        std::vector<float> pk((size_t)L.cout_pad * L.wld, 0.f), scale(L.cout_pad, 1.f), shift(L.cout_pad, 0.f);
        for (int n = 0; n < rows; ++n) {
            float* dst = &pk[(size_t)n * L.wld];
            memcpy(dst, md->shapedirs + (size_t)n * 20, 20 * 4);
            shift[n] = md->v_template[n];
        }
        for (int p = 0; p < NP; ++p) {
            const float* src = md->posedirs + (size_t)p * rows;
            for (int n = 0; n < rows; ++n) pk[(size_t)n * L.wld + 20 + p] = src[n];
        }
        hipError_t e = upload(L.w, pk.data(), pk.size() * 4);
        if (e == hipSuccess) {
            std::vector<uint16_t> ps(2 * pk.size());          // rows of 512 coefficients: planar groups of 8
            host_split_pack_planar(pk.data(), pk.size(), ps.data());
            e = upload(h->dirs_split, ps.data(), pk.size() * 4);
        }
        if (e == hipSuccess) {
            // the same directions for the fused kernel: split-bf16 MFMA A fragments in register order, K = 224 (20 shape /
            // expression + the 21 body joints' 189 pose features; the 8th K step holds jaw / eye features, zero on that path):
            // block ((g*8 + ks)*3 + c)*2 + plane = 64 lanes x 8 bf16, lane (lr, g4) = row 3*(16 g + lr) + c,
            // coefficients 32 ks + 8 g4 .. + 7
            const int ng = (V + 15) / 16;
            std::vector<uint16_t> fr(ap_smplx_dirs_frag_bytes(V) / 2, 0);
            for (int g = 0; g < ng; ++g)
                for (int ks = 0; ks < 8; ++ks)
                    for (int c = 0; c < 3; ++c)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int v = g * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
                            if (v >= V) continue;
                            uint16_t* hi = &fr[((((size_t)g * 8 + ks) * 3 + c) * 2) * 512 + lane * 8];
                            uint16_t* lo = hi + 512;
                            for (int i = 0; i < 8; ++i) host_split_parts(pk[(size_t)(3 * v + c) * L.wld + k0 + i], &hi[i], &lo[i]);
                        }
            e = upload(h->dirs_frag, fr.data(), fr.size() * 2);
        }
        if (e == hipSuccess) e = upload(L.scale, scale.data(), scale.size() * 4);
        if (e == hipSuccess) e = upload(L.shift, shift.data(), shift.size() * 4);
        if (e != hipSuccess) { ap_smplx_destroy(h); return fail((int)e, std::string("upload: ") + hipGetErrorString(e)); }
    }
    std::vector<int> ev(std::max(1, md->num_extra)), tri(std::max(1, md->num_landmarks * 3));
    for (int i = 0; i < md->num_extra; ++i) {
        ev[i] = (int)md->extra_joint_verts[i];
        if (ev[i] < 0 || ev[i] >= V) { ap_smplx_destroy(h); return fail(AP_ESHAPE, "extra joint vertex id out of range"); }
    }
    for (int l = 0; l < md->num_landmarks; ++l) {
        const int64_t f = md->lmk_faces_idx[l];
        if (f < 0 || f >= md->num_faces) { ap_smplx_destroy(h); return fail(AP_ESHAPE, "landmark face id out of range"); }
        for (int c = 0; c < 3; ++c) {
            tri[l * 3 + c] = (int)md->faces[f * 3 + c];
            if (tri[l * 3 + c] < 0 || tri[l * 3 + c] >= V) { ap_smplx_destroy(h); return fail(AP_ESHAPE, "face vertex id out of range"); }
        }
    }
    // distinct vertices the joints kernel skins (vertex picks + landmark corners): their v_posed goes to a compact side buffer
    std::vector<int> slot(V, -1);
    int n_jv = 0;
    for (int i = 0; i < md->num_extra; ++i) if (slot[ev[i]] < 0) slot[ev[i]] = n_jv++;
    for (int i = 0; i < md->num_landmarks * 3; ++i) if (slot[tri[i]] < 0) slot[tri[i]] = n_jv++;
    m.n_jv = std::max(n_jv, 1);
    hipError_t e = upload(h->j_template, jt.data(), jt.size() * 4);
    if (e == hipSuccess) e = upload(h->jv_slot, slot.data(), slot.size() * 4);
    if (e == hipSuccess && K == 4 && n_jv < 255) {           // fused kernel: bone indices as 6-bit fields + joint-vertex slot, weights padded to whole groups
        const int vp = (V + 15) / 16 * 16;
        std::vector<uint32_t> i8(vp, 0);
        std::vector<float> w4((size_t)vp * 4, 0.f);
        for (int v = 0; v < V; ++v) {
            for (int k = 0; k < 4; ++k) i8[v] |= (uint32_t)(sidx[(size_t)v * 4 + k] & 0x3f) << (6 * k);
            if (slot[v] >= 0 && slot[v] < 255) i8[v] |= (uint32_t)(slot[v] + 1) << 24;
            memcpy(&w4[(size_t)v * 4], &sw[(size_t)v * 4], 16);
        }
        e = upload(h->skin_idx8, i8.data(), i8.size() * 4);
        if (e == hipSuccess) e = upload(h->skin_w4, w4.data(), w4.size() * 4);
        if (e == hipSuccess) {
            // the joints kernel's record per output joint beyond the chain (21 vertex picks, 51 landmarks): its three corner
            // vertices' side-buffer slots, packed bone ids, weights and barycentric weights in 6 x 16 bytes -- one load level
            const int nj2 = md->num_extra + md->num_landmarks;
            std::vector<float> pk((size_t)std::max(nj2, 1) * 24, 0.f);
            for (int t = 0; t < nj2; ++t) {
                float* r = &pk[(size_t)t * 24];
                for (int f = 0; f < 3; ++f) {
                    const bool lm = t >= md->num_extra;
                    const int v = lm ? tri[(t - md->num_extra) * 3 + f] : ev[t];
                    const int sl = slot[v];
                    const uint32_t id = i8[v] & 0x00ffffffu;
                    memcpy(&r[f], &sl, 4);
                    memcpy(&r[4 + f], &id, 4);
                    memcpy(&r[8 + 4 * f], &w4[(size_t)v * 4], 16);
                    r[20 + f] = lm ? md->lmk_bary_coords[(t - md->num_extra) * 3 + f] : (f == 0 ? 1.f : 0.f);
                }
            }
            e = upload(h->jt_pack, pk.data(), pk.size() * 4);
        }
        // body-only table: every joint >= 22 (jaw, eyes, fingers: identity rotation without a hand / face pose) skins exactly like its
        // nearest ancestor < 22, so a vertex needs at most as many DISTINCT transforms as it has bones -- usually fewer (a finger
        // vertex: one).  Bones merged by representative, weights summed in double, heaviest first; unused slots repeat slot 0's bone
        // with weight 0 (the kernel skips zero weights).
        const int NBODY = 22;
        if (e == hipSuccess && J >= NBODY) {
            std::vector<int> rep(J);
            for (int j = 0; j < J; ++j) { int r = j; while (r >= NBODY) r = par[r]; rep[j] = r; }
            std::vector<uint32_t> i8b(vp, 0);
            std::vector<float> w4b((size_t)vp * 4, 0.f);
            for (int v = 0; v < V; ++v) {
                int bj[4]; double bw[4]; int nbn = 0;
                for (int k = 0; k < 4; ++k) {
                    const float w = sw[(size_t)v * 4 + k];
                    if (w == 0.f) continue;
                    const int r = rep[sidx[(size_t)v * 4 + k]];
                    int q = 0;
                    while (q < nbn && bj[q] != r) ++q;
                    if (q == nbn) { bj[nbn] = r; bw[nbn] = 0.0; ++nbn; }
                    bw[q] += (double)w;
                }
                for (int a2 = 0; a2 < nbn; ++a2)             // heaviest first (stable)
                    for (int b2 = a2 + 1; b2 < nbn; ++b2)
                        if (bw[b2] > bw[a2]) { std::swap(bw[a2], bw[b2]); std::swap(bj[a2], bj[b2]); }
                if (nbn == 0) { bj[0] = 0; bw[0] = 0.0; nbn = 1; }
                for (int k = 0; k < 4; ++k) {
                    i8b[v] |= (uint32_t)((k < nbn ? bj[k] : bj[0]) & 0x3f) << (6 * k);
                    w4b[(size_t)v * 4 + k] = k < nbn ? (float)bw[k] : 0.f;
                }
                i8b[v] |= i8[v] & 0xff000000u;
            }
            e = upload(h->skin_idx8b, i8b.data(), i8b.size() * 4);
            if (e == hipSuccess) e = upload(h->skin_w4b, w4b.data(), w4b.size() * 4);
            if (e == hipSuccess) m.nb = NBODY;
        }
    }
    if (e == hipSuccess) e = upload(h->j_shapedirs, jsd.data(), jsd.size() * 4);
    if (e == hipSuccess) e = upload(h->parents, par.data(), par.size() * 4);
    if (e == hipSuccess) e = upload(h->depth, dep.data(), dep.size() * 4);
    if (e == hipSuccess) e = upload(h->skin_idx, sidx.data(), sidx.size() * 4);
    if (e == hipSuccess) e = upload(h->skin_w, sw.data(), sw.size() * 4);
    if (e == hipSuccess) e = upload(h->extra_verts, ev.data(), ev.size() * 4);
    if (e == hipSuccess) e = upload(h->lmk_tri, tri.data(), tri.size() * 4);
    if (e == hipSuccess)
        e = upload(h->lmk_bary, md->num_landmarks ? (const void*)md->lmk_bary_coords : (const void*)tri.data(),
                   std::max(1, md->num_landmarks * 3) * 4);
    if (e != hipSuccess) { ap_smplx_destroy(h); return fail((int)e, std::string("upload: ") + hipGetErrorString(e)); }
    m.j_template = h->j_template.as<float>(); m.j_shapedirs = h->j_shapedirs.as<float>();
    m.parents = h->parents.as<int>(); m.depth = h->depth.as<int>();
    m.skin_idx = h->skin_idx.as<int>(); m.skin_w = h->skin_w.as<float>();
    m.extra_verts = h->extra_verts.as<int>(); m.lmk_tri = h->lmk_tri.as<int>(); m.lmk_bary = h->lmk_bary.as<float>();
    m.n_extra = md->num_extra; m.n_lmk = md->num_landmarks;
    m.dirs_frag = h->dirs_frag.p; m.v_template = h->dirs.shift.as<float>(); m.jv_slot = h->jv_slot.as<int>();
    m.skin_idx8 = h->skin_idx8.as<uint32_t>(); m.skin_w4 = h->skin_w4.as<float>();
    m.skin_idx8b = h->skin_idx8b.as<uint32_t>(); m.skin_w4b = h->skin_w4b.as<float>();
    m.jt_pack = h->jt_pack.as<float4>();
    h->n_out_joints = J + md->num_extra + md->num_landmarks;
    *out = h;
    return AP_OK;
}

void ap_smplx_destroy(ap_smplx* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (DevBuf* b : {&h->dirs.w, &h->dirs_split, &h->dirs.scale, &h->dirs.shift, &h->j_template, &h->j_shapedirs, &h->parents, &h->depth,
                      &h->skin_idx, &h->skin_w, &h->extra_verts, &h->lmk_tri, &h->lmk_bary, &h->ws_coef, &h->ws_A, &h->ws_A22, &h->dirs_frag, &h->jv_slot, &h->skin_idx8, &h->skin_w4, &h->skin_idx8b, &h->skin_w4b, &h->jt_pack, &h->ws_side,
                      &h->ws_jposed, &h->ws_post, &h->ws_vposed, &h->ws_cc, &h->ws_cnt, &h->bw_bone_off, &h->bw_bone_ent, &h->bw_jv_off,
                      &h->bw_jv_ent, &h->bw_coef, &h->bw_A, &h->bw_jposed, &h->bw_vposed, &h->bw_gvp, &h->bw_gA, &h->bw_gt, &h->bw_gcoef})
        b->release();
    h->tm.destroy();
    delete h;
}

int ap_smplx_num_joints_out(const ap_smplx* h) { return h ? h->n_out_joints : AP_EINVAL; }

int ap_smplx_fwd(ap_smplx* h, int n, const float* betas, const float* expression, const float* global_orient,
                 const float* body_pose, const float* extra_pose, const float* transl, float* vertices,
                 float* joints, void* stream) {
    if (!h || n <= 0 || !betas || !body_pose || !vertices || !joints) return fail(AP_EINVAL, "ap_smplx_fwd: bad argument");
    SmplxFwdArgs a{};
    a.n = n; a.betas = betas; a.expression = expression; a.global_orient = global_orient; a.body_pose = body_pose;
    a.extra_pose = extra_pose; a.transl = transl; a.vertices = vertices; a.joints = joints;
    return smplx_run(h, a, extra_pose == nullptr, (hipStream_t)stream);
}

int ap_smplx_fwd_fused(ap_smplx* h, int n, const float* pred_pose, int pose_ld, const float* betas,
                       const float* cam_center, float fx, float fy, float* vertices_cam, float* joints_cam,
                       float* joints2d, float* rotmat, void* stream) {
    if (!h || n <= 0 || !pred_pose || pose_ld < 135 || !betas || !vertices_cam || !joints_cam)
        return fail(AP_EINVAL, "ap_smplx_fwd_fused: bad argument");
    SmplxFwdArgs a{};
    a.n = n; a.betas = betas;
    a.pose6d = pred_pose + 3; a.pose6d_ld = pose_ld;
    a.post_t = pred_pose; a.post_t_ld = pose_ld;
    a.cam_center = cam_center; a.fx = fx; a.fy = fy;
    a.vertices = vertices_cam; a.joints = joints_cam; a.joints2d = cam_center ? joints2d : nullptr;
    a.rotmat_out = rotmat;
    return smplx_run(h, a, true, (hipStream_t)stream);
}

int ap_smplx_fwd_twoview(ap_smplx* h, int B, float* pred_pose, int pose_ld, float trans_scale, const float* betas,
                         const float* intr0, const float* intr1, float fx, float fy, const float* in_smpltrans,
                         float* vertices, float* joints_cam, float* joints2d, float* rotmat, void* stream) {
    if (!h || B <= 0 || !pred_pose || pose_ld < 135 || !betas || !vertices || !joints_cam || (!intr0) != (!intr1) ||
        trans_scale < 0.f)
        return fail(AP_EINVAL, "ap_smplx_fwd_twoview: bad argument");
    SmplxFwdArgs a{};
    a.n_main = 2 * B;
    a.n = in_smpltrans ? 4 * B : 2 * B;
    a.in_trans = in_smpltrans;
    a.betas = betas;
    a.pose6d = pred_pose + 3; a.pose6d_ld = pose_ld;
    a.post_t = pred_pose; a.post_t_ld = pose_ld;
    if (trans_scale > 0.f) { a.pose_rw = pred_pose; a.trans_scale = trans_scale; }
    a.intr0 = intr0; a.intr1 = intr1; a.fx = fx; a.fy = fy;
    a.vertices = vertices; a.joints = joints_cam; a.joints2d = intr0 ? joints2d : nullptr;
    a.rotmat_out = rotmat;
    return smplx_run(h, a, true, (hipStream_t)stream);
}

int ap_smplx_bwd(ap_smplx* h, int n, const float* betas, const float* expression, const float* global_orient,
                 const float* body_pose, const float* extra_pose, const float* transl, const float* grad_vertices,
                 const float* grad_joints, float* grad_betas, float* grad_expression, float* grad_global_orient,
                 float* grad_body_pose, float* grad_extra_pose, float* grad_transl, void* stream) {
    (void)transl;                                            // the gradients do not depend on the translation
    if (!h || n <= 0 || !betas || !body_pose) return fail(AP_EINVAL, "ap_smplx_bwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const bool want_rest = grad_betas || grad_expression || grad_global_orient || grad_body_pose || grad_extra_pose;
    if (!want_rest && !grad_transl) return AP_OK;
    if (!grad_vertices && !grad_joints) {                    // zero upstream gradient
        const std::pair<float*, size_t> outs[6] = {{grad_betas, 10}, {grad_expression, 10}, {grad_global_orient, 9},
                                                   {grad_body_pose, 21 * 9}, {grad_extra_pose, (size_t)(h->m.J - 22) * 9}, {grad_transl, 3}};
        for (const auto& o : outs)
            if (o.first) HIP_TRY(hipMemsetAsync(o.first, 0, (size_t)n * o.second * 4, st));
        return AP_OK;
    }
    HIP_TRY(smplx_bwd_tables(h));
    SmplxModelDev m = h->m;                                  // (a copy: the forward's handle state is not touched)
    m.coef_split = h->blend_split ? 1 : 0;
    // hand / face poses (or their gradient): the K = 512 contraction; body-only: 224
    const bool body_only = !extra_pose && !grad_extra_pose;
    int K = body_only ? 20 + 21 * 9 : 20 + (m.J - 1) * 9;
    K = ((K + 31) / 32) * 32;
    const int rows16 = (3 * m.V + 15) & ~15;
    const bool want_coef = grad_betas || grad_expression || grad_body_pose || grad_extra_pose;   // global_orient alone: no pose feature
    const int nsplit = want_coef ? (rows16 + SMPLX_BWD_RC - 1) / SMPLX_BWD_RC : 0;
    const int nr = h->bw_nr;
    HIP_TRY(h->bw_coef.reserve((size_t)n * m.ncoef * 4));
    HIP_TRY(h->bw_A.reserve((size_t)n * m.J * 12 * 4));
    HIP_TRY(h->bw_jposed.reserve((size_t)n * m.J * 3 * 4));
    HIP_TRY(h->bw_vposed.reserve((size_t)n * m.ldv * 4));
    HIP_TRY(h->bw_gvp.reserve((size_t)n * m.ldv * 4));
    HIP_TRY(h->bw_gA.reserve((size_t)n * nr * m.J * 12 * 4));
    HIP_TRY(h->bw_gt.reserve((size_t)n * nr * 3 * 4));
    if (nsplit) HIP_TRY(h->bw_gcoef.reserve((size_t)nsplit * n * K * 4));
    // recompute: coefficient rows and bone transforms (smplx_prep_kernel), v_posed (the forward's two-kernel blend GEMM)
    SmplxFwdArgs f{};
    f.n = n; f.betas = betas; f.expression = expression; f.global_orient = global_orient; f.body_pose = body_pose;
    f.extra_pose = extra_pose;
    f.coef = h->bw_coef.as<float>(); f.A = h->bw_A.as<float>(); f.jposed = h->bw_jposed.as<float>();
    HIP_TRY(ap_launch_smplx_prep(m, f, st));
    {
        ConvArgs g{};
        g.x = f.coef; g.w = h->blend_split ? h->dirs_split.p : h->dirs.w.p;
        g.scale = h->dirs.scale.as<float>(); g.shift = h->dirs.shift.as<float>();
        g.out_f32 = 1;
        g.res = nullptr; g.y = h->bw_vposed.p;
        g.N = n; g.H = g.W = g.Ho = g.Wo = 1; g.Cin = K; g.Cout = h->dirs.cout; g.KH = g.KW = 1; g.stride = 1; g.pad = 0;
        g.M = n; g.ldx = m.ncoef; g.ldy = m.ldv; g.ldr = 0; g.wld = h->dirs.wld; g.relu = 0;
        HIP_TRY(dispatch_conv(g, h->blend_split ? AP_PREC_BF16X2 : AP_PREC_FP32, st));
    }
    SmplxBwdArgs a{};
    a.n = n; a.betas = betas; a.expression = expression; a.global_orient = global_orient; a.body_pose = body_pose;
    a.extra_pose = extra_pose; a.grad_vertices = grad_vertices; a.grad_joints = grad_joints;
    a.grad_betas = grad_betas; a.grad_expression = grad_expression; a.grad_global_orient = grad_global_orient;
    a.grad_body_pose = grad_body_pose; a.grad_extra_pose = grad_extra_pose; a.grad_transl = grad_transl;
    a.A = f.A; a.vposed = h->bw_vposed.as<float>(); a.gvp = h->bw_gvp.as<float>(); a.gA = h->bw_gA.as<float>();
    a.gt = h->bw_gt.as<float>(); a.gcoef = h->bw_gcoef.as<float>();
    a.nr = nr; a.nsplit = nsplit; a.kp = K;
    a.dirs = h->dirs.w.as<float>();
    a.bone_off = h->bw_bone_off.as<int>(); a.bone_ent = h->bw_bone_ent.as<int2>();
    a.jv_off = h->bw_jv_off.as<int>(); a.jv_ent = h->bw_jv_ent.as<int2>();
    HIP_TRY(ap_launch_smplx_bwd_lbs(m, a, st));
    if (nsplit) HIP_TRY(ap_launch_smplx_bwd_coef(m, a, st));
    HIP_TRY(ap_launch_smplx_bwd_chain(m, a, st));
    return AP_OK;
}

int ap_smplx_set_blend_precision(ap_smplx* h, int precision) {
    if (!h || (precision != AP_PREC_FP32 && precision != AP_PREC_BF16X2))
        return fail(AP_EINVAL, "ap_smplx_set_blend_precision: AP_PREC_FP32 or AP_PREC_BF16X2");
    h->blend_split = precision == AP_PREC_BF16X2;
    return AP_OK;
}

int ap_smplx_debug_poison_workspace(ap_smplx* h, int n) {
    if (!h || n <= 0) return fail(AP_EINVAL, "ap_smplx_debug_poison_workspace: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->ws_coef.reserve((size_t)n * h->m.ncoef * 4));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(h->ws_coef.p, 0xFF, h->ws_coef.bytes));           // NaN bit patterns in both storage forms
    return AP_OK;
}

int ap_smplx_set_fused(ap_smplx* h, int on) {
    if (!h) return fail(AP_EINVAL, "null handle");
    h->fused = on != 0;
    h->fuse_joints = on == 4;                                // 4: joints stage inside the kernel, done by each group's last workgroup (A/B: slower)
    h->merge_bones = on == 6 ? 0 : (on == 8 ? 2 : 1);        // 6: every joint's transform in LDS (round 5's form); 8: merged table, 64 bodies per workgroup (A/B: slower)
    h->fold_post = on != 7;                                  // 7: merged table, post transform applied per vertex instead of composed into the bones (A/B)
    return AP_OK;
}

int ap_smplx_enable_timing(ap_smplx* h, int on) {
    if (!h) return fail(AP_EINVAL, "null handle");
    h->tm.on = on < 0 ? 0 : (on > 2 ? 2 : on);               // 1: per-stage events; 2: the span of the whole tail (two events)
    return AP_OK;
}

int ap_smplx_timing(ap_smplx* h, double ms[4], int64_t* passes, int reset) {
    if (!h || !ms || !passes) return fail(AP_EINVAL, "ap_smplx_timing: null argument");
    HIP_TRY(h->tm.collect(ms, 4, passes, reset != 0));
    return AP_OK;
}

}  // extern "C"
