// Every trunk kernel that is not a convolution, once, for trunk_grad.hip and trunk_grad_bf16.hip: BatchNorm (the tiling rule, the
// reduction passes, the combination of their partials, the element-wise passes), the two pools, the split-K combine and the crop
// gradient's layout kernel.  Included inside each file's unnamed namespace, so there is one source of the rule, of the per-channel
// summation order and of the reduction trees.  A kernel that touches activations is a template over the file's storage trait S:
//   S::T, S::W         storage type; channels a thread moves in the element-wise passes (C % W == 0)
//   S::V               W floats
//   S::rd(T)           one stored value as fp32
//   S::ld(const T*)    W stored values as fp32, one access
//   S::st(T*, V)       W fp32 values to storage, one access (any rounding happens here)
// All math is fp32 on the values rd / ld return, whatever the storage.

// ---------------------------------------------------------------------------------------------------------------- split-K, layout
// gW[co][c][r][s] (c < C) = sum over the chunks, in chunk order, of part[chunk][co][(r S + s) Cp + c]; Cp: the channels of x as stored
__global__ void __launch_bounds__(256) wgrad_combine_kernel(const float* __restrict__ part, int nch, int K, int C, int Cp, int R, int S,
                                                            float* __restrict__ gw) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)C * R * S, perp = (long long)Cp * R * S;
    if (idx >= (long long)K * per) return;
    const int co = (int)(idx / per), rem = (int)(idx - co * per);
    const int c = rem / (R * S), rs = rem - c * R * S;
    const long long src = (long long)co * perp + (long long)rs * Cp + c, stride = (long long)K * perp;
    float s = 0.f;
    for (int ch = 0; ch < nch; ++ch) s += part[ch * stride + src];
    gw[idx] = s;
}

// fp32 NHWC with `pitch` channels per pixel -> fp32 NCHW (n, C, HW), the first C channels
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const float* __restrict__ x, int n, int C, int pitch, int HW,
                                                           float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * C * HW) return;
    const int hw = (int)(idx % HW);
    const long long p = idx / HW;
    const int c = (int)(p % C), b = (int)(p / C);
    y[idx] = x[((long long)b * HW + hw) * pitch + c];
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm
// Rows (n H W) are cut into tiles of `tr` rows (tr % 4 == 0, at most 256 tiles); a workgroup of the reduction passes takes 64
// channels x one tile, its 4 waves a quarter of the tile each.
int bn_tile_rows(int M) { return std::max(256, (((M + 255) / 256) + 3) & ~3); }
int bn_tiles(int M) { return (M + bn_tile_rows(M) - 1) / bn_tile_rows(M); }

// per tile: count, mean, M2 = sum (x - mean)^2 (centred on the tile's own mean).  One channel per lane and scalar reads whatever
// S::W is: the per-channel summation order is the contract
template <class S>
__global__ void __launch_bounds__(256) bn_stats_part_kernel(const typename S::T* __restrict__ x, int M, int C, int tr,
                                                            float* __restrict__ part) {
    __shared__ float sh[4][64];
    __shared__ float smean[64];
    const int t = threadIdx.x, cl = t & 63, g = t >> 6, c = blockIdx.x * 64 + cl, tile = blockIdx.y;
    const int t0 = tile * tr, tcnt = min(tr, M - t0), r0 = t0 + g * (tr / 4), r1 = min(r0 + tr / 4, M);
    float s = 0.f;
    if (c < C)
        for (int r = r0; r < r1; ++r) s += S::rd(x[(long long)r * C + c]);
    sh[g][cl] = s;
    __syncthreads();
    if (g == 0) smean[cl] = (((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl]) / (float)tcnt;
    __syncthreads();
    const float mean = smean[cl];
    float m2 = 0.f;
    if (c < C)
        for (int r = r0; r < r1; ++r) {
            const float d = S::rd(x[(long long)r * C + c]) - mean;
            m2 += d * d;
        }
    sh[g][cl] = m2;
    __syncthreads();
    if (g == 0 && c < C) {
        part[((long long)tile * 3 + 0) * C + c] = (float)tcnt;
        part[((long long)tile * 3 + 1) * C + c] = mean;
        part[((long long)tile * 3 + 2) * C + c] = ((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl];
    }
}

// Chan's combination of (na, ma, qa) with (nb, mb, qb)
__device__ __forceinline__ void chan(float& na, float& ma, float& qa, float nb, float mb, float qb) {
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; qa = qb; return; }
    const float n = na + nb, d = mb - ma, f = nb / n;
    ma = ma + d * f;
    qa = qa + qb + d * d * na * f;
    na = n;
}

// one workgroup of 64 lanes per channel: lane l combines tiles l, l + 64, ... in order, then a fixed tree over the lanes.
// Writes the batch mean and 1 / sqrt(var + eps) (biased var); running_mean / running_var updated as nn.BatchNorm2d does
// (unbiased var), when given.
__global__ void __launch_bounds__(64) bn_stats_final_kernel(const float* __restrict__ part, int nt, int C, float momentum, float eps,
                                                            float* running_mean, float* running_var, float* __restrict__ mean_out,
                                                            float* __restrict__ invstd_out) {
    __shared__ float sn[64], sm[64], sq[64];
    const int l = threadIdx.x, c = blockIdx.x;
    float n = 0.f, m = 0.f, q = 0.f;
    for (int tl = l; tl < nt; tl += 64)
        chan(n, m, q, part[((long long)tl * 3 + 0) * C + c], part[((long long)tl * 3 + 1) * C + c], part[((long long)tl * 3 + 2) * C + c]);
    sn[l] = n; sm[l] = m; sq[l] = q;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (l < off) {
            float a = sn[l], b = sm[l], d = sq[l];
            chan(a, b, d, sn[l + off], sm[l + off], sq[l + off]);
            sn[l] = a; sm[l] = b; sq[l] = d;
        }
        __syncthreads();
    }
    if (l == 0) {
        const float cnt = sn[0], mean = sm[0], var = sq[0] / cnt;
        mean_out[c] = mean;
        invstd_out[c] = 1.f / sqrtf(var + eps);
        if (running_mean) {
            const float unb = cnt > 1.f ? sq[0] / (cnt - 1.f) : var;
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
        }
    }
}

__global__ void __launch_bounds__(256) bn_eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int C, float eps,
                                                            float* __restrict__ mean_out, float* __restrict__ invstd_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    mean_out[c] = rm[c];
    invstd_out[c] = 1.f / sqrtf(rv[c] + eps);
}

// y = (x - mean) invstd gamma + beta (+ res) (ReLU) on W channels per thread; y may alias x or res (same index)
template <class S>
__global__ void __launch_bounds__(256) bn_apply_kernel(const typename S::T* x, long long groups, int C, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const typename S::T* res, int relu,
                                                       typename S::T* y) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= groups) return;
    const long long idx = gi * S::W;
    const int c = (int)(idx % C);
    typename S::V v = S::ld(x + idx), r;
    if (res) r = S::ld(res + idx);
#pragma unroll
    for (int j = 0; j < S::W; ++j) {
        float f = (v.v[j] - mean[c + j]) * invstd[c + j] * gamma[c + j] + beta[c + j];
        if (res) f += r.v[j];
        if (relu) f = fmaxf(f, 0.f);
        v.v[j] = f;
    }
    S::st(y + idx, v);
}

// per tile: sum g and sum g xhat, g = gy masked by y > 0 (y NULL: no ReLU).  One channel per lane, scalar reads, as the statistics
template <class S>
__global__ void __launch_bounds__(256) bn_bwd_part_kernel(const typename S::T* __restrict__ gy, const typename S::T* __restrict__ y,
                                                          const typename S::T* __restrict__ x, int M, int C, int tr,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          float* __restrict__ part) {
    __shared__ float s1[4][64], s2[4][64];
    const int t = threadIdx.x, cl = t & 63, g = t >> 6, c = blockIdx.x * 64 + cl, tile = blockIdx.y;
    const int r0 = tile * tr + g * (tr / 4), r1 = min(r0 + tr / 4, M);
    float a = 0.f, b = 0.f;
    if (c < C) {
        const float mu = mean[c], is = invstd[c];
        for (int r = r0; r < r1; ++r) {
            const long long o = (long long)r * C + c;
            float gv = S::rd(gy[o]);
            if (y && !(S::rd(y[o]) > 0.f)) gv = 0.f;
            a += gv;
            b += gv * ((S::rd(x[o]) - mu) * is);
        }
    }
    s1[g][cl] = a;
    s2[g][cl] = b;
    __syncthreads();
    if (g == 0 && c < C) {
        part[((long long)tile * 2 + 0) * C + c] = ((s1[0][cl] + s1[1][cl]) + s1[2][cl]) + s1[3][cl];
        part[((long long)tile * 2 + 1) * C + c] = ((s2[0][cl] + s2[1][cl]) + s2[2][cl]) + s2[3][cl];
    }
}

// sums[0][c] = sum g, sums[1][c] = sum g xhat: lane l sums tiles l, l + 64, ... in order, then a fixed tree; g_beta / g_gamma copies
__global__ void __launch_bounds__(64) bn_bwd_final_kernel(const float* __restrict__ part, int nt, int C, float* __restrict__ sums,
                                                          float* __restrict__ g_gamma, float* __restrict__ g_beta) {
    __shared__ float sa[64], sb[64];
    const int l = threadIdx.x, c = blockIdx.x;
    float a = 0.f, b = 0.f;
    for (int tl = l; tl < nt; tl += 64) {
        a += part[((long long)tl * 2 + 0) * C + c];
        b += part[((long long)tl * 2 + 1) * C + c];
    }
    sa[l] = a; sb[l] = b;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (l < off) { sa[l] += sa[l + off]; sb[l] += sb[l + off]; }
        __syncthreads();
    }
    if (l == 0) {
        sums[c] = sa[0];
        sums[C + c] = sb[0];
        if (g_beta) g_beta[c] = sa[0];
        if (g_gamma) g_gamma[c] = sb[0];
    }
}

// gx = gamma invstd (g - sum g / M - xhat sum(g xhat) / M) (train) or gamma invstd g (eval); g_res = g.  gx may alias gy.
template <class S>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const typename S::T* gy, const typename S::T* __restrict__ y,
                                                           const typename S::T* __restrict__ x, long long groups, int C, float inv_m,
                                                           int train, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ sums,
                                                           typename S::T* gx, typename S::T* g_res) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= groups) return;
    const long long idx = gi * S::W;
    const int c = (int)(idx % C);
    typename S::V g = S::ld(gy + idx), xv = S::ld(x + idx), o;
    if (y) {
        const typename S::V yv = S::ld(y + idx);
#pragma unroll
        for (int j = 0; j < S::W; ++j)
            if (!(yv.v[j] > 0.f)) g.v[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < S::W; ++j) {
        const float k = gamma[c + j] * invstd[c + j];
        if (train) {
            const float xhat = (xv.v[j] - mean[c + j]) * invstd[c + j];
            o.v[j] = k * ((g.v[j] - sums[c + j] * inv_m) - xhat * (sums[C + c + j] * inv_m));
        } else {
            o.v[j] = k * g.v[j];
        }
    }
    if (g_res) S::st(g_res + idx, g);                            // exact: g is gy or 0
    S::st(gx + idx, o);
}

// ---------------------------------------------------------------------------------------------------------------- pools
// max-pool 3 x 3 / s2 / p1, NHWC, on W channels per thread: padding is -inf; the first maximum in row-major window order is the
// argmax, as in torch
template <class S>
__device__ __forceinline__ void maxpool_arg(const typename S::T* __restrict__ x, int b, int ho, int wo, int c, int H, int W, int C,
                                            float* best, int* arg) {
#pragma unroll
    for (int j = 0; j < S::W; ++j) { best[j] = -INFINITY; arg[j] = -1; }
    for (int r = 0; r < 3; ++r) {
        const int h = ho * 2 - 1 + r;
        if (h < 0 || h >= H) continue;
        for (int s = 0; s < 3; ++s) {
            const int w = wo * 2 - 1 + s;
            if (w < 0 || w >= W) continue;
            const typename S::V v = S::ld(x + (((long long)b * H + h) * W + w) * C + c);
#pragma unroll
            for (int j = 0; j < S::W; ++j)
                if (arg[j] < 0 || v.v[j] > best[j] || v.v[j] != v.v[j]) { best[j] = v.v[j]; arg[j] = h * W + w; }
        }
    }
}

template <class S>
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const typename S::T* __restrict__ x, int n, int H, int W, int C, int Ho, int Wo,
                                                          typename S::T* __restrict__ y) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x, idx = gi * S::W;
    if (idx >= (long long)n * Ho * Wo * C) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int wo = (int)(p % Wo), ho = (int)((p / Wo) % Ho), b = (int)(p / ((long long)Wo * Ho));
    typename S::V m;
    int arg[S::W];
    maxpool_arg<S>(x, b, ho, wo, c, H, W, C, m.v, arg);
    S::st(y + idx, m);                                           // a selection: exact
}

// gx[b][h][w][c] = sum, over the windows (ho, wo ascending) whose argmax is (h, w), of gy[b][ho][wo][c]
template <class S>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const typename S::T* __restrict__ x, const typename S::T* __restrict__ gy, int n,
                                                          int H, int W, int C, int Ho, int Wo, typename S::T* __restrict__ gx) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x, idx = gi * S::W;
    if (idx >= (long long)n * H * W * C) return;
    const int c = (int)(idx % C);
    const long long p = idx / C;
    const int w = (int)(p % W), h = (int)((p / W) % H), b = (int)(p / ((long long)W * H));
    typename S::V s;
#pragma unroll
    for (int j = 0; j < S::W; ++j) s.v[j] = 0.f;
    const int me = h * W + w;
    for (int ho = max(0, h / 2 - 1); ho <= min(Ho - 1, (h + 1) / 2); ++ho) {
        if (h < ho * 2 - 1 || h > ho * 2 + 1) continue;
        for (int wo = max(0, w / 2 - 1); wo <= min(Wo - 1, (w + 1) / 2); ++wo) {
            if (w < wo * 2 - 1 || w > wo * 2 + 1) continue;
            float m[S::W];
            int arg[S::W];
            maxpool_arg<S>(x, b, ho, wo, c, H, W, C, m, arg);
            const typename S::V g = S::ld(gy + (((long long)b * Ho + ho) * Wo + wo) * C + c);
#pragma unroll
            for (int j = 0; j < S::W; ++j)
                if (arg[j] == me) s.v[j] += g.v[j];
        }
    }
    S::st(gx + idx, s);
}

// avg-pool 7 x 7 over a (n, 7, 7, C) map -> fp32 (n, C): the 49 pixels summed in row-major order in fp32, / 49
template <class S>
__global__ void __launch_bounds__(256) avgpool_fwd_kernel(const typename S::T* __restrict__ x, int n, int C, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * C) return;
    const int c = (int)(idx % C), b = (int)(idx / C);
    float s = 0.f;
    for (int p = 0; p < 49; ++p) s += S::rd(x[((long long)b * 49 + p) * C + c]);
    y[idx] = s / 49.f;
}

template <class S>
__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float* __restrict__ gy, int n, int C, typename S::T* __restrict__ gx) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x, idx = gi * S::W;
    if (idx >= (long long)n * 49 * C) return;
    const int c = (int)(idx % C), b = (int)(idx / (49LL * C));
    typename S::V o;
#pragma unroll
    for (int j = 0; j < S::W; ++j) o.v[j] = gy[(long long)b * C + c + j] / 49.f;
    S::st(gx + idx, o);
}
