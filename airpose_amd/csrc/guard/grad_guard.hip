// Gradient clipping and the non-finite guard for gfx950 (libairpose_grad.so).
// The guard (apg_grad_norm, apg_grad_scale, apg_adam_step_guarded): the global L2 norm of a gradient list, torch's clip coefficient
// and a non-finite flag, computed on the device in one read of the gradients and consumed by adam_guarded_kernel<AMSGRAD> in the same
// step -- no host copy, no synchronisation, no second pass over the gradients.
//
//   grad_norm_chunk_kernel   grid = the batch's chunk count, 256 threads
//     adam_kernel's partition: GRAD_BATCH = 192 tensors per launch in the argument block (GradBatch: 3880 bytes), 4096-element
//     chunks, the same owner thread per quad.  A thread squares its (up to) 16 elements in fp64 -- (double) g * (double) g is exact --
//     and adds them in element order into ONE fp64 accumulator from the first add: S cannot overflow for any fp32 gradients, tiny
//     ones do not flush, and S is non-finite exactly when an element is.  Then a fixed tree: lane l += lane l + 32, 16, 8, 4, 2, 1 inside
//     each wave, the four wave sums through LDS as ((w0 + w1) + w2) + w3.  The chunk's partial goes to the workspace.
//   grad_norm_tensor_kernel  grid = the batch's tensor count, 64 threads
//     S_i = the tensor's chunk partials added in chunk order by ONE thread (staged through LDS 64 at a time so that the loads are
//     coalesced); writes S_i to the workspace and per_tensor[i] = (float) sqrt(S_i).  A tensor without elements has S_i = 0.
//   grad_norm_final_kernel   one workgroup of 64 threads
//     S = the S_i added in tensor order by one thread, then the guard record (GuardRecord below) and the two counters.
// so an apg_grad_norm call is 2 ceil(ntensors / 192) + 1 launches.  No atomics and no arrival counter: every sum has one order, which
// depends on the sizes alone -- not on pointers, alignment or timing.  The 16-byte and 4-byte paths differ only in how a quad is moved.
//   grad_scale_kernel        the same partition; g = __fmul_rn(g, coef); a workgroup returns without a store when coef == 1.
//   adam_guarded_kernel<AMSGRAD>   optim.hip's step (adam_seq.inc: adam_body<AMSGRAD, true>): every workgroup loads skip and coef; with
//     skip set it returns before its first store, otherwise g2 = __fmul_rn(coef, g) and the sequence runs on g2.
// This source sits in a directory of its own and is linked through GUARD_UNITS (../Makefile says why); tests/test_gradnorm_abi.py
// scans it for packed fp32 math as tests/test_packed_math_scan.py scans the sources of the committed list.
#include "../grad_internal.h"

#include "../adam_seq.inc"

namespace {

template <bool AMSGRAD>
__global__ void __launch_bounds__(AT) adam_guarded_kernel(const AdamBatch a) {
    adam_body<AMSGRAD, true>(a);
}

// ------------------------------------------------------------------------------------------------ the guard
constexpr int GRAD_BATCH = APG_GRAD_NORM_BATCH;                           // tensors per launch: as many as the argument block holds
constexpr int GT = 64;                                                    // threads of the two combining kernels: one wave

struct GradBatch {
    float* g[GRAD_BATCH];
    long long numel[GRAD_BATCH];
    unsigned prefix[GRAD_BATCH + 1];     // as AdamBatch's; a tensor without elements takes a slot here and owns no chunk
    int count;                           // tensors of this batch
    double* partial;                     // workspace: the partial of this batch's chunk 0
    double* tsum;                        // workspace: S_i of this batch's tensor 0
    float* per_tensor;                   // this batch's tensor 0 of the caller's array, or nullptr
    const GuardRecord* guard;            // grad_scale_kernel only
};
static_assert(sizeof(GradBatch) <= 4096, "one batch must fit the kernel-argument block");

// the tensor of workgroup w: the last i with prefix[i] <= w (adam_kernel's search)
__device__ __forceinline__ int grad_find(const GradBatch& a, unsigned w) {
    int lo = 0, hi = GRAD_BATCH;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.prefix[mid] <= w)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// this thread's share of sum g^2 over one chunk, in fp64 from the first add, in element order
template <bool ALIGNED>
__device__ __forceinline__ double sumsq_chunk(const float* __restrict__ G, long long base, long long n) {
    constexpr int Q = ADAM_CHUNK / (AT * 4);
    float g[Q][4];
    bool full[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const long long e = base + ((long long)i * AT + threadIdx.x) * 4;
        full[i] = e + 4 <= n;
        if (full[i]) load4<ALIGNED>(G + e, g[i]);
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const long long e = base + ((long long)i * AT + threadIdx.x) * 4;
        if (full[i]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)g[i][k];
                acc = fma(d, d, acc);                                     // d * d is exact in fp64: the fma rounds what the sum would
            }
        } else {
            for (long long k = e; k < n; ++k) {                           // the partial quad at the end of the tensor
                const double d = (double)G[k];
                acc = fma(d, d, acc);
            }
        }
    }
    return acc;
}

__global__ void __launch_bounds__(AT) grad_norm_chunk_kernel(const GradBatch a) {
    __shared__ double wsum[AT / 64];
    const unsigned w = blockIdx.x;
    const int i = grad_find(a, w);
    const long long n = a.numel[i];
    const long long base = (long long)(w - a.prefix[i]) * ADAM_CHUNK;
    const float* G = a.g[i];
    double acc = (((uintptr_t)G & 15) == 0) ? sumsq_chunk<true>(G, base, n) : sumsq_chunk<false>(G, base, n);   // uniform
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off, 64);  // lane 0 of each wave: the wave's fixed tree
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[w] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// src[0] + src[1] + .. + src[n - 1] in that order, by thread 0 (the value it returns; the other threads' is meaningless).  GT values
// at a time are loaded by the whole workgroup into LDS, so the loads are coalesced and the one thread's chain is LDS reads and adds.
__device__ __forceinline__ double ordered_sum(const double* __restrict__ src, long long n, double* lds) {
    double acc = 0.0;
    for (long long b = 0; b < n; b += GT) {
        const long long k = b + threadIdx.x;
        if (k < n) lds[threadIdx.x] = src[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - b < GT ? (int)(n - b) : GT;
            for (int j = 0; j < m; ++j) acc += lds[j];
        }
        __syncthreads();
    }
    return acc;
}

__global__ void __launch_bounds__(GT) grad_norm_tensor_kernel(const GradBatch a) {
    __shared__ double lds[GT];
    const int i = blockIdx.x;                                             // < a.count
    const double S = ordered_sum(a.partial + a.prefix[i], (long long)(a.prefix[i + 1] - a.prefix[i]), lds);
    if (threadIdx.x == 0) {
        a.tsum[i] = S;
        if (a.per_tensor) a.per_tensor[i] = (float)sqrt(S);
    }
}

__global__ void __launch_bounds__(GT) grad_norm_final_kernel(const double* __restrict__ tsum, int ntensors, double max_norm, int skip_nonfinite,
                                                             int empty, GuardRecord* __restrict__ guard, long long* __restrict__ counters) {
    __shared__ double lds[GT];
    const double S = ordered_sum(tsum, ntensors, lds);
    if (threadIdx.x != 0) return;
    const double nrm = sqrt(S);
    const bool bad = !(S - S == 0.0);                                     // NaN or +Inf: some element was NaN or +-Inf
    const double c = max_norm / (nrm + 1e-6);                             // torch's clip_coef, then its clamp at 1
    float coef = (float)(c < 1.0 ? c : 1.0);
    if (bad) coef = __builtin_nanf("");
    const int skip = bad && skip_nonfinite;
    if (skip || empty) coef = 1.f;
    guard->coef = coef;
    guard->norm = (float)nrm;
    guard->skip = skip;
    guard->reserved = 0;
    if (counters) {
        counters[0] += 1;
        if (skip) counters[1] += 1;
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void scale_chunk(float coef, float* __restrict__ G, long long base, long long n) {
    constexpr int Q = ADAM_CHUNK / (AT * 4);
    float g[Q][4];
    bool full[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const long long e = base + ((long long)i * AT + threadIdx.x) * 4;
        full[i] = e + 4 <= n;
        if (full[i]) load4<ALIGNED>(G + e, g[i]);
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const long long e = base + ((long long)i * AT + threadIdx.x) * 4;
        if (full[i]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) g[i][k] = __fmul_rn(g[i][k], coef);
            store4<ALIGNED>(G + e, g[i]);
        } else {
            for (long long k = e; k < n; ++k) G[k] = __fmul_rn(G[k], coef);
        }
    }
}

__global__ void __launch_bounds__(AT) grad_scale_kernel(const GradBatch a) {
    const float coef = a.guard->coef;                                     // uniform
    if (coef == 1.f) return;                                              // nothing to clip (or a skipped step): no store at all
    const unsigned w = blockIdx.x;
    const int i = grad_find(a, w);
    const long long n = a.numel[i];
    const long long base = (long long)(w - a.prefix[i]) * ADAM_CHUNK;
    float* G = a.g[i];
    if (((uintptr_t)G & 15) == 0)
        scale_chunk<true>(coef, G, base, n);
    else
        scale_chunk<false>(coef, G, base, n);
}

// the argument checks apg_grad_norm and apg_grad_scale share; chunks: the list's chunk count
int grad_check(const std::string& f, int ntensors, const void* const* g, const int64_t* numel, const void* guard, int64_t* chunks) {
    if (ntensors < 0) return apg_fail(APG_EINVAL, f + "ntensors must be >= 0");
    if (!g) return apg_fail(APG_EINVAL, f + "the g table is NULL");
    if (!numel) return apg_fail(APG_EINVAL, f + "the numel array is NULL");
    if (!guard) return apg_fail(APG_EINVAL, f + "the guard record is NULL");
    if ((uintptr_t)guard & 3) return apg_fail(APG_EINVAL, f + "the guard record is not 4-byte aligned");
    *chunks = 0;
    for (int i = 0; i < ntensors; ++i) {
        const std::string at = " of tensor " + std::to_string(i);
        if (numel[i] < 0) return apg_fail(APG_EINVAL, f + "numel" + at + " is negative");
        if (numel[i] > (int64_t)0x7fffffff * ADAM_CHUNK) return apg_fail(APG_EINVAL, f + "numel" + at + " is too large");
        if (numel[i] > 0 && !g[i]) return apg_fail(APG_EINVAL, f + "g" + at + " is NULL");
        if ((uintptr_t)g[i] & 3) return apg_fail(APG_EINVAL, f + "g" + at + " is not 4-byte aligned");
        *chunks += (numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    }
    return APG_OK;
}

// walks the list GRAD_BATCH tensors at a time (fewer where a grid would pass 2^31 - 1 chunks) and calls launch(b, chunks) for each
// batch, with b.partial / b.tsum / b.per_tensor moved to the batch's first chunk / tensor
template <class F>
int grad_batches(int ntensors, const void* const* g, const int64_t* numel, GradBatch& b, F&& launch) {
    double* const partial = b.partial;
    double* const tsum = b.tsum;
    float* const per_tensor = b.per_tensor;
    int64_t chunk0 = 0;
    int first = 0, count = 0;
    unsigned chunks = 0;
    auto flush = [&]() -> int {
        for (int i = count; i < GRAD_BATCH; ++i) b.g[i] = nullptr, b.numel[i] = 0;
        for (int i = count; i <= GRAD_BATCH; ++i) b.prefix[i] = chunks;
        b.count = count;
        b.partial = partial ? partial + chunk0 : nullptr;
        b.tsum = tsum ? tsum + first : nullptr;
        b.per_tensor = per_tensor ? per_tensor + first : nullptr;
        return count ? launch(b, chunks) : APG_OK;
    };
    for (int i = 0; i < ntensors; ++i) {
        const unsigned nc = (unsigned)((numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK);
        if (count == GRAD_BATCH || nc > 0x7fffffffu - chunks) {
            const int rc = flush();
            if (rc != APG_OK) return rc;
            chunk0 += chunks, first = i, count = 0, chunks = 0;
        }
        b.g[count] = (float*)g[i], b.numel[count] = numel[i], b.prefix[count] = chunks;
        chunks += nc;
        ++count;
    }
    return flush();
}

}  // namespace

extern "C" {

int apg_adam_step_guarded(int ntensors, const void* const* p, const void* const* g, const void* const* m, const void* const* v,
                          const void* const* vmax, const int64_t* numel, const int64_t* step, double lr, double beta1, double beta2,
                          double eps, double weight_decay, const void* guard, void* stream) {
    return adam_step("apg_adam_step_guarded: ", true, ntensors, p, g, m, v, vmax, numel, step, lr, beta1, beta2, eps, weight_decay, guard,
                     stream, [](const AdamBatch& b, unsigned chunks, bool amsgrad, hipStream_t st) {
                         if (amsgrad)
                             hipLaunchKernelGGL(adam_guarded_kernel<true>, dim3(chunks), dim3(AT), 0, st, b);
                         else
                             hipLaunchKernelGGL(adam_guarded_kernel<false>, dim3(chunks), dim3(AT), 0, st, b);
                     });
}

int64_t apg_grad_norm_workspace_bytes(int ntensors, const int64_t* numel) {
    if (ntensors < 0 || (ntensors > 0 && !numel)) return -1;
    int64_t chunks = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (numel[i] < 0 || numel[i] > (int64_t)0x7fffffff * ADAM_CHUNK) return -1;
        chunks += (numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    }
    return (chunks + ntensors) * (int64_t)sizeof(double);
}

int apg_grad_norm(int ntensors, const void* const* g, const int64_t* numel, double max_norm, int skip_nonfinite, void* workspace,
                  int64_t workspace_bytes, void* guard, float* per_tensor, int64_t* counters, void* stream) {
    const std::string f = "apg_grad_norm: ";
    int64_t chunks = 0;
    const int rc = grad_check(f, ntensors, g, numel, guard, &chunks);
    if (rc != APG_OK) return rc;
    if (!(max_norm >= 0.0)) return apg_fail(APG_EINVAL, f + "max_norm must be >= 0 (+inf: guard only)");
    const int64_t need = (chunks + ntensors) * (int64_t)sizeof(double);
    if (workspace_bytes < need || (need > 0 && !workspace))
        return apg_fail(APG_EINVAL, f + "the workspace holds " + std::to_string(workspace ? workspace_bytes : 0) + " bytes, apg_grad_norm_workspace_bytes asks for " +
                                        std::to_string(need));
    if ((uintptr_t)workspace & 7) return apg_fail(APG_EINVAL, f + "the workspace is not 8-byte aligned");
    if ((uintptr_t)per_tensor & 3) return apg_fail(APG_EINVAL, f + "per_tensor is not 4-byte aligned");
    if ((uintptr_t)counters & 7) return apg_fail(APG_EINVAL, f + "the counters are not 8-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    GradBatch b;
    b.partial = (double*)workspace;
    b.tsum = (double*)workspace + chunks;
    b.per_tensor = per_tensor;
    b.guard = nullptr;
    const int rb = grad_batches(ntensors, g, numel, b, [st](const GradBatch& a, unsigned nchunks) -> int {
        if (nchunks) hipLaunchKernelGGL(grad_norm_chunk_kernel, dim3(nchunks), dim3(AT), 0, st, a);
        hipLaunchKernelGGL(grad_norm_tensor_kernel, dim3(a.count), dim3(GT), 0, st, a);
        APG_TRY(hipGetLastError());
        return APG_OK;
    });
    if (rb != APG_OK) return rb;
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(GT), 0, st, (const double*)workspace + chunks, ntensors, max_norm,
                       skip_nonfinite ? 1 : 0, chunks == 0 ? 1 : 0, (GuardRecord*)guard, (long long*)counters);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

int apg_grad_scale(int ntensors, const void* const* g, const int64_t* numel, const void* guard, void* stream) {
    int64_t chunks = 0;
    const int rc = grad_check("apg_grad_scale: ", ntensors, g, numel, guard, &chunks);
    if (rc != APG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    GradBatch b;
    b.partial = nullptr, b.tsum = nullptr, b.per_tensor = nullptr;
    b.guard = (const GuardRecord*)guard;
    return grad_batches(ntensors, g, numel, b, [st](const GradBatch& a, unsigned nchunks) -> int {
        if (!nchunks) return APG_OK;
        hipLaunchKernelGGL(grad_scale_kernel, dim3(nchunks), dim3(AT), 0, st, a);
        APG_TRY(hipGetLastError());
        return APG_OK;
    });
}

}  // extern "C"
