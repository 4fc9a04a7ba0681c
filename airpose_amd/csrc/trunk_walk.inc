// The precision-agnostic host side of the trainable ResNet-50 trunk, shared by trunk_grad.hip (F32Ops) and trunk_grad_bf16.hip
// (Bf16Ops): convolution geometry, the workspace plan of the fixed [3, 4, 6, 3] graph, and the forward and backward walks over it.
// Included inside each file's unnamed namespace, after its kernels (and trunk_elem.inc) and in front of its launch helpers, which use
// Geom; nothing here is exported.  A backend is a struct `Ops` of static functions over that file's launchers (no virtual calls);
// what only depends on the file's storage trait S (trunk_elem.inc) it inherits from ElemOps<S>:
//   act                        activation / activation-gradient storage type (ElemOps)
//   fwd_name, bwd_name         the entry points' names, the prefix of every message
//   ws_aligned                 refuse a workspace that is not 256-byte aligned
//   packed, cpad(C)            a bf16 copy of the weights lives in the workspace (Layer::wf / wd); channels of x as stored
//   pack                       fill wf / wd in front of a forward convolution
//   conv_fwd, conv_dgrad, conv_wgrad
//   bn_fwd, bn_bwd, maxpool_fwd / _bwd, avgpool_fwd / _bwd   (ElemOps)
//   crops_in, crop_grad        NCHW fp32 crops -> Plan::ximg; stem data gradient (through g2) -> NCHW fp32 g_x
//   ds_block_dgrad             the input gradient of a block with a downsample branch

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
unsigned nblk(long long total) { return (unsigned)((total + 255) / 256); }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Geom {
    int n, H, W, C, K, R, S, st, pad, Ho, Wo;                   // C: the channel count of x as stored
};

// the checks every backend needs; a backend with stricter rules adds its own on top
bool geom_ok(const Geom& g) {
    if (g.n <= 0 || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.K <= 0 || g.R <= 0 || g.S <= 0 || g.st <= 0 || g.pad < 0) return false;
    // the kernel must fit the padded input: make_geom's division truncates toward zero, so at stride >= 2 a too-large kernel
    // would otherwise come out as Ho = 1
    if ((long long)g.H + 2LL * g.pad < g.R || (long long)g.W + 2LL * g.pad < g.S) return false;
    if (g.Ho <= 0 || g.Wo <= 0) return false;
    return (long long)g.n * g.H * g.W * g.C < (1LL << 31) && (long long)g.n * g.Ho * g.Wo * g.K < (1LL << 31) &&
           (long long)g.n * g.Ho * g.Wo < (1LL << 31);
}

Geom make_geom(int n, int H, int W, int C, int K, int R, int S, int st, int pad) {
    Geom g{n, H, W, C, K, R, S, st, pad, 0, 0};
    if (st > 0) {
        g.Ho = (H + 2 * pad - R) / st + 1;
        g.Wo = (W + 2 * pad - S) / st + 1;
    }
    return g;
}

template <class Args>
Args conv_args(const Geom& g) {
    Args a = {};
    a.n = g.n; a.H = g.H; a.W = g.W; a.C = g.C; a.K = g.K; a.R = g.R; a.S = g.S; a.st = g.st; a.pad = g.pad; a.Ho = g.Ho; a.Wo = g.Wo;
    return a;
}

void wgrad_split(const Geom& g, int* nch, int* chunk);          // the backend's split-K rule

size_t wgrad_floats(const Geom& g) {
    int nch, chunk;
    wgrad_split(g, &nch, &chunk);
    return (size_t)nch * g.K * g.R * g.S * g.C;
}

size_t bn_part_floats(int M, int C) { return (size_t)bn_tiles(M) * 3 * C + 2 * (size_t)C; }

// ---------------------------------------------------------------------------------------------------------------- BatchNorm, pools
// forward BN over (M, C): train -> batch statistics (+ running update when rm / rv given), eval -> running statistics
template <class S>
hipError_t bn_fwd(const typename S::T* x, int M, int C, const float* gamma, const float* beta, float* rm, float* rv, int train,
                  float momentum, float eps, const typename S::T* res, int relu, typename S::T* y, float* mean, float* invstd, float* part,
                  hipStream_t st) {
    if (train) {
        const int tr = bn_tile_rows(M), nt = bn_tiles(M);
        hipLaunchKernelGGL(bn_stats_part_kernel<S>, dim3((C + 63) / 64, nt), dim3(256), 0, st, x, M, C, tr, part);
        hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C), dim3(64), 0, st, part, nt, C, momentum, eps, rm, rv, mean, invstd);
    } else {
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, st, rm, rv, C, eps, mean, invstd);
    }
    const long long groups = (long long)M * C / S::W;
    hipLaunchKernelGGL(bn_apply_kernel<S>, dim3(nblk(groups)), dim3(256), 0, st, x, groups, C, mean, invstd, gamma, beta, res, relu, y);
    return hipGetLastError();
}

template <class S>
hipError_t bn_bwd(const typename S::T* gy, const typename S::T* y, const typename S::T* x, int M, int C, const float* gamma,
                  const float* mean, const float* invstd, int train, typename S::T* gx, typename S::T* g_res, float* g_gamma,
                  float* g_beta, float* part, hipStream_t st) {
    const int tr = bn_tile_rows(M), nt = bn_tiles(M);
    float* sums = part + (size_t)nt * 2 * C;
    hipLaunchKernelGGL(bn_bwd_part_kernel<S>, dim3((C + 63) / 64, nt), dim3(256), 0, st, gy, y, x, M, C, tr, mean, invstd, part);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C), dim3(64), 0, st, part, nt, C, sums, g_gamma, g_beta);
    const long long groups = (long long)M * C / S::W;
    hipLaunchKernelGGL(bn_bwd_apply_kernel<S>, dim3(nblk(groups)), dim3(256), 0, st, gy, y, x, groups, C, 1.f / (float)M, train, mean,
                       invstd, gamma, sums, gx, g_res);
    return hipGetLastError();
}

// the launchers a backend's Ops inherits: one thread per S::W channels in the element-wise kernels
template <class S>
struct ElemOps {
    using act = typename S::T;
    static constexpr auto bn_fwd = &::bn_fwd<S>;
    static constexpr auto bn_bwd = &::bn_bwd<S>;
    static void maxpool_fwd(const act* x, int n, int H, int W, int C, act* y, hipStream_t st) {
        const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
        hipLaunchKernelGGL(maxpool_fwd_kernel<S>, dim3(nblk((long long)n * Ho * Wo * C / S::W)), dim3(256), 0, st, x, n, H, W, C, Ho, Wo,
                           y);
    }
    static void maxpool_bwd(const act* x, const act* gy, int n, int H, int W, int C, act* gx, hipStream_t st) {
        const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
        hipLaunchKernelGGL(maxpool_bwd_kernel<S>, dim3(nblk((long long)n * H * W * C / S::W)), dim3(256), 0, st, x, gy, n, H, W, C, Ho, Wo,
                           gx);
    }
    static void avgpool_fwd(const act* x, int n, int C, float* y, hipStream_t st) {
        hipLaunchKernelGGL(avgpool_fwd_kernel<S>, dim3(nblk((long long)n * C)), dim3(256), 0, st, x, n, C, y);
    }
    static void avgpool_bwd(const float* gy, int n, int C, act* gx, hipStream_t st) {
        hipLaunchKernelGGL(avgpool_bwd_kernel<S>, dim3(nblk((long long)n * 49 * C / S::W)), dim3(256), 0, st, gy, n, C, gx);
    }
};

// ---------------------------------------------------------------------------------------------------------------- the trunk plan
constexpr int NLAYER = 53;
constexpr int IMG = 224;

template <class T>
struct Layer {
    int idx, c_real;                     // position in state_dict order (conv + BN pair); input channels of the fp32 weight
    Geom g;
    T *in, *z, *a;                       // conv input, conv output (pre-BN), BN output
    T *wf, *wd;                          // Ops::packed: this call's packed weights (forward; data gradient, save = 1 only)
    float *mean, *invstd;
};

template <class T>
struct Block {
    Layer<T> c1, c2, c3, ds;
    bool has_ds;
};

template <class T>
struct Plan {
    Layer<T> stem;
    T *ximg, *pool;                      // NHWC copy of the crops (Ops::cpad(3) channels); max-pool output
    Block<T> blk[16];
    T* G[6];                             // backward: gradient buffers of the largest activation
    float* part;                         // split-K / BN partials
    size_t total;                        // bytes
};

// Walks the fixed [3, 4, 6, 3] graph.  base == nullptr: sizes only.  Every buffer starts on a 256-byte boundary.  save = 1: every
// activation has its own buffer (what backward reads) and the backward buffers follow; save = 0: forward only, five rotating
// buffers, BN in place.  Per layer: packed weights (Ops::packed: wf, and wd when save = 1), z, a (save = 1), mean, invstd.
template <class Ops>
Plan<typename Ops::act> make_plan(int n, int save, void* base) {
    using T = typename Ops::act;
    Plan<T> P;
    size_t off = 0;
    auto take = [&](size_t bytes) -> void* {
        void* p = base ? (char*)base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    auto acts = [&](size_t count) { return (T*)take(count * sizeof(T)); };
    const size_t big = (size_t)n * 112 * 112 * 64;       // the largest activation (stem output; layer1's 256-channel maps equal it)
    T* slot[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!save)
        for (int k = 0; k < 5; ++k) slot[k] = acts(big);
    size_t part = 0;
    auto mk = [&](Layer<T>& L, int idx, T* in, int H, int C, int K, int R, int st, int pad, T* zs) {
        L.idx = idx;
        L.c_real = C;
        L.g = make_geom(n, H, H, Ops::cpad(C), K, R, R, st, pad);
        L.in = in;
        const size_t wsz = (size_t)K * R * R * L.g.C;
        L.wf = Ops::packed ? acts(wsz) : nullptr;
        L.wd = Ops::packed && save ? acts(wsz) : nullptr;       // the data gradient's packing: backward only
        const size_t sz = (size_t)n * L.g.Ho * L.g.Wo * K;
        L.z = save ? acts(sz) : zs;
        L.a = save ? acts(sz) : zs;
        L.mean = (float*)take((size_t)K * sizeof(float));
        L.invstd = (float*)take((size_t)K * sizeof(float));
        part = std::max(part, wgrad_floats(L.g));
        part = std::max(part, bn_part_floats(n * L.g.Ho * L.g.Wo, K));
    };
    P.ximg = save ? acts((size_t)n * IMG * IMG * Ops::cpad(3)) : slot[0];
    mk(P.stem, 0, P.ximg, IMG, 3, 64, 7, 2, 3, slot[1]);
    P.pool = save ? acts((size_t)n * 56 * 56 * 64) : slot[2];
    T* x = P.pool;
    int H = 56, C = 64, idx = 1, bi = 0;
    int free_slots[3] = {0, 1, 3};                          // save = 0: the slots not holding the block input (slot 2) ...
    int in_slot = 2, ds_slot = 4;
    const int layers[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < layers[li]; ++b, ++bi) {
            const int p = planes[li], st = (b == 0 && li > 0) ? 2 : 1;
            Block<T>& B = P.blk[bi];
            B.has_ds = b == 0;
            T *s1 = nullptr, *s2 = nullptr, *s3 = nullptr;
            if (!save) { s1 = slot[free_slots[0]]; s2 = slot[free_slots[1]]; s3 = slot[free_slots[2]]; }
            mk(B.c1, idx++, x, H, C, p, 1, 1, 0, s1);
            mk(B.c2, idx++, B.c1.a, H, p, p, 3, st, 1, s2);
            const int Ho = B.c2.g.Ho;
            mk(B.c3, idx++, B.c2.a, Ho, p, 4 * p, 1, 1, 0, s3);
            if (B.has_ds) mk(B.ds, idx++, x, H, C, 4 * p, 1, st, 0, save ? nullptr : slot[ds_slot]);
            x = B.c3.a;
            H = Ho;
            C = 4 * p;
            if (!save) {                                    // the block output (slot free_slots[2]) becomes the next input
                const int o = free_slots[2];
                free_slots[2] = in_slot;
                in_slot = o;
            }
        }
    for (int k = 0; k < 6; ++k) P.G[k] = save ? acts(big) : nullptr;
    P.part = (float*)take(part * sizeof(float));
    P.total = off;
    return P;
}

template <class Ops>
int64_t trunk_bytes(int n, int save) {
    if (n <= 0 || n > 2048) return -1;
    return (int64_t)make_plan<Ops>(n, save ? 1 : 0, nullptr).total;
}

const float* prm(const void* const* t, int layer, int k) { return (const float*)t[layer * 5 + k]; }

int check_table(const void* const* params, const char* what) {
    if (!params) return apg_fail(APG_EINVAL, std::string(what) + ": parameter table missing");
    for (int k = 0; k < NLAYER * 5; ++k)
        if (!params[k]) return apg_fail(APG_EINVAL, std::string(what) + ": parameter table entry " + std::to_string(k) + " is NULL");
    return APG_OK;
}

// the checks both walks share behind their own argument test: workspace alignment, the parameter table, the workspace size
template <class Ops>
int check_walk(const char* what, const char* filled_by, int n, int save, const void* const* params, const void* workspace,
               int64_t workspace_bytes) {
    if (Ops::ws_aligned && ((uintptr_t)workspace & 255) != 0)
        return apg_fail(APG_EINVAL, std::string(what) + ": the workspace must be 256-byte aligned");
    if (int rc = check_table(params, what)) return rc;
    const int64_t needed = trunk_bytes<Ops>(n, save);
    if (workspace_bytes < needed)
        return apg_fail(APG_ENOMEM, std::string(what) + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                        std::to_string(needed) + " needed" +
                                        (filled_by ? " (the one " + std::string(filled_by) + " filled, save = 1)" : std::string()));
    return APG_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the walks
template <class Ops>
int trunk_fwd_walk(int n, const float* x, const void* const* params, int train, float momentum, float eps, float* xf, int save,
                   void* workspace, int64_t workspace_bytes, void* stream) {
    using T = typename Ops::act;
    if (n <= 0 || n > 2048 || !x || !xf || !workspace || !(eps >= 0.f) || (train && !(momentum >= 0.f && momentum <= 1.f)))
        return apg_fail(APG_EINVAL, std::string(Ops::fwd_name) + ": bad argument");
    if (int rc = check_walk<Ops>(Ops::fwd_name, nullptr, n, save, params, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Plan<T> P = make_plan<Ops>(n, save ? 1 : 0, workspace);
    auto run = [&](const Layer<T>& L, const T* res, int relu) -> hipError_t {
        const float* w = prm(params, L.idx, 0);
        Ops::pack(L, w, st);
        hipError_t e = Ops::conv_fwd(L, w, st);
        if (e != hipSuccess) return e;
        return Ops::bn_fwd(L.z, n * L.g.Ho * L.g.Wo, L.g.K, prm(params, L.idx, 1), prm(params, L.idx, 2), (float*)prm(params, L.idx, 3),
                           (float*)prm(params, L.idx, 4), train, momentum, eps, res, relu, L.a, L.mean, L.invstd, P.part, st);
    };
    Ops::crops_in(x, n, P.ximg, st);
    APG_TRY(run(P.stem, nullptr, 1));
    Ops::maxpool_fwd(P.stem.a, n, 112, 112, 64, P.pool, st);
    APG_TRY(hipGetLastError());
    for (int b = 0; b < 16; ++b) {
        const Block<T>& B = P.blk[b];
        APG_TRY(run(B.c1, nullptr, 1));
        APG_TRY(run(B.c2, nullptr, 1));
        if (B.has_ds) APG_TRY(run(B.ds, nullptr, 0));
        APG_TRY(run(B.c3, B.has_ds ? B.ds.a : B.c1.in, 1));
    }
    Ops::avgpool_fwd(P.blk[15].c3.a, n, 2048, xf, st);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

template <class Ops>
int trunk_bwd_walk(int n, const void* const* params, int train, const float* g_xf, void* const* g_params, float* g_x, void* workspace,
                   int64_t workspace_bytes, void* stream) {
    using T = typename Ops::act;
    if (n <= 0 || n > 2048 || !g_xf || !g_params || !workspace) return apg_fail(APG_EINVAL, std::string(Ops::bwd_name) + ": bad argument");
    if (int rc = check_walk<Ops>(Ops::bwd_name, Ops::fwd_name, n, 1, params, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Plan<T> P = make_plan<Ops>(n, 1, workspace);
    T *gcur = P.G[0], *gnext = P.G[1], *g3 = P.G[2], *g2 = P.G[3], *g1 = P.G[4], *gres = P.G[5];
    auto gp = [&](const Layer<T>& L, int k) { return (float*)g_params[L.idx * 3 + k]; };
    // BN backward of layer L (gy -> gx, ReLU mask from L.a when relu), then its weight gradient
    auto bnb = [&](const Layer<T>& L, const T* gy, int relu, T* gx, T* g_res) -> hipError_t {
        return Ops::bn_bwd(gy, relu ? L.a : nullptr, L.z, n * L.g.Ho * L.g.Wo, L.g.K, prm(params, L.idx, 1), L.mean, L.invstd, train, gx,
                           g_res, gp(L, 1), gp(L, 2), P.part, st);
    };
    auto wg = [&](const Layer<T>& L, const T* gz) -> hipError_t {
        if (!gp(L, 0)) return hipSuccess;
        return Ops::conv_wgrad(L, gz, P.part, gp(L, 0), st);
    };
    // gx = dgrad of layer L (gy) (+ add)
    auto dg = [&](const Layer<T>& L, const T* gy, const T* add, T* gx) -> hipError_t {
        return Ops::conv_dgrad(L, gy, prm(params, L.idx, 0), add, gx, st);
    };
    Ops::avgpool_bwd(g_xf, n, 2048, gcur, st);
    APG_TRY(hipGetLastError());
    for (int b = 15; b >= 0; --b) {
        const Block<T>& B = P.blk[b];
        APG_TRY(bnb(B.c3, gcur, 1, g3, gres));
        APG_TRY(wg(B.c3, g3));
        APG_TRY(dg(B.c3, g3, nullptr, g2));
        APG_TRY(bnb(B.c2, g2, 1, g2, nullptr));
        APG_TRY(wg(B.c2, g2));
        APG_TRY(dg(B.c2, g2, nullptr, g1));
        APG_TRY(bnb(B.c1, g1, 1, g1, nullptr));
        APG_TRY(wg(B.c1, g1));
        if (B.has_ds) {
            APG_TRY(bnb(B.ds, gres, 0, gres, nullptr));
            APG_TRY(wg(B.ds, gres));
            // gnext = dgrad of the downsample (gres) + dgrad of conv1 (g1); g3 and the adjacent g2 are free here
            APG_TRY(Ops::ds_block_dgrad(B.ds, prm(params, B.ds.idx, 0), gres, B.c1, prm(params, B.c1.idx, 0), g1, g3, gnext, st));
        } else {
            APG_TRY(dg(B.c1, g1, gres, gnext));
        }
        std::swap(gcur, gnext);
    }
    // stem: max-pool, BN + ReLU, the 7 x 7 convolution
    Ops::maxpool_bwd(P.stem.a, gcur, n, 112, 112, 64, g1, st);
    APG_TRY(hipGetLastError());
    APG_TRY(bnb(P.stem, g1, 1, g1, nullptr));
    APG_TRY(wg(P.stem, g1));
    if (g_x) APG_TRY(Ops::crop_grad(P.stem, prm(params, 0, 0), g1, g2, n, g_x, st));
    return APG_OK;
}
