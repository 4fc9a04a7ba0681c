// BatchNorm pieces shared by trunk_grad.hip and trunk_grad_bf16.hip: the tiling rule and the kernels that touch fp32 data only
// (the combination of the per-tile partials, the eval-mode statistics, the backward sums).  Included inside each file's unnamed
// namespace, so there is one source of the rule and of the reduction trees.
// Rows (n H W) are cut into tiles of `tr` rows (tr % 4 == 0, at most 256 tiles).
int bn_tile_rows(int M) { return std::max(256, (((M + 255) / 256) + 3) & ~3); }
int bn_tiles(int M) { return (M + bn_tile_rows(M) - 1) / bn_tile_rows(M); }

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
