// Multi-tensor Adam / AMSGrad step for gfx950 (libairpose_grad.so): torch.optim.Adam's _single_tensor_adam (maximize = False, L2
// weight decay) over a whole list of fp32 tensors in one pass -- 5 floats read (p, g, m, v, vmax) and 4 written per parameter.
//
//   adam_kernel<AMSGRAD>   grid = the batch's chunk count, 256 threads
//     The tensors travel in the kernel-argument block, ADAM_BATCH = 64 at a time (AdamBatch below: 3880 bytes of the 4096 a launch
//     may carry), one launch per batch.  A chunk is ADAM_CHUNK = 4096 consecutive elements of ONE tensor; a tensor of n elements owns
//     ceil(n / 4096) consecutive workgroups and prefix[] holds the running count, so a workgroup finds its tensor by a binary search
//     of prefix[] with its own index (uniform over the workgroup: scalar loads from the argument block).  Thread t owns the float
//     quads at chunk * 4096 + (i * 256 + t) * 4, i = 0 .. 3.
//
// Per element, with the host's double-precision scalars each rounded to float ONCE (wd, 1 - beta1, beta2, 1 - beta2, eps, and per
// tensor ss = lr / (1 - beta1^step), rb = 1 / sqrt(1 - beta2^step)):
//     g'   = fmaf(wd, p, g)                              fused            (wd = 0: g' = g exactly)
//     d    = g' - m                                      one rounding
//     m    = fmaf(1 - beta1, d, m)                       fused            torch's lerp
//     t    = g' * g'                                     NOT fused        (__fmul_rn)
//     w    = beta2 * v                                   NOT fused        (__fmul_rn)
//     v    = fmaf(1 - beta2, t, w)                       fused
//     vmax = fmaxf(vmax, v)                              exact            (AMSGRAD only; the maximum is taken AFTER v is updated)
//     den  = fmaf(sqrtf(vmax or v), rb, eps)             sqrt correctly rounded, then fused
//     q    = m / den                                     correctly rounded division
//     p    = fmaf(-ss, q, p)                             fused
// `#pragma clang fp contract(off)` below leaves no other fusion to the compiler: every fma of the sequence is an fmaf call, every
// plain product and sum stays one (with the pragma's default, `fast`, __fmul_rn is an ordinary product that may be contracted).
//
// Alignment only selects how a thread's quad is moved: one 16-byte access per array when all of the tensor's pointers are 16-byte
// aligned, four 4-byte accesses otherwise (a per-tensor bit computed on the host).  It changes neither the elements a thread owns
// nor the arithmetic, so it cannot change a bit of any result.  The last numel mod 4 elements of a tensor are a partial quad, taken
// one by one on both paths.  Plain vector stores only: no atomics, no inline assembly, no reduction, nothing carried between calls.
#include "grad_internal.h"

#include <cmath>
#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int AT = 256;                  // threads per workgroup
constexpr int ADAM_CHUNK = 4096;         // elements per workgroup: 256 threads x 4 quads of 4
constexpr int ADAM_BATCH = 64;           // tensors per launch

struct AdamBatch {
    float* p[ADAM_BATCH];
    const float* g[ADAM_BATCH];
    float* m[ADAM_BATCH];
    float* v[ADAM_BATCH];
    float* vmax[ADAM_BATCH];
    long long numel[ADAM_BATCH];
    float ss[ADAM_BATCH];                // lr / (1 - beta1^step)
    float rb[ADAM_BATCH];                // 1 / sqrt(1 - beta2^step)
    unsigned prefix[ADAM_BATCH + 1];     // prefix[i] = chunks of the tensors before i; prefix[n ..] = the batch's chunk count
    unsigned long long aligned;          // bit i: every pointer of tensor i is 16-byte aligned
    float wd, omb1, b2, omb2, eps;
};
static_assert(sizeof(AdamBatch) <= 4096, "one batch must fit the kernel-argument block");

struct AdamScalars {
    float wd, omb1, b2, omb2, eps, ss, rb;
};

template <bool AMSGRAD>
__device__ __forceinline__ void adam_elem(const AdamScalars& s, float& p, float g, float& m, float& v, float& vmax) {
    const float g1 = fmaf(s.wd, p, g);
    const float d = g1 - m;
    m = fmaf(s.omb1, d, m);
    const float t = __fmul_rn(g1, g1);
    const float w = __fmul_rn(s.b2, v);
    v = fmaf(s.omb2, t, w);
    float vh = v;
    if (AMSGRAD) {
        vmax = fmaxf(vmax, v);
        vh = vmax;
    }
    const float den = fmaf(sqrtf(vh), s.rb, s.eps);
    const float q = m / den;
    p = fmaf(-s.ss, q, p);
}

template <bool ALIGNED>
__device__ __forceinline__ void load4(const float* p, float* x) {
    if (ALIGNED) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
        x[0] = p[0], x[1] = p[1], x[2] = p[2], x[3] = p[3];
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void store4(float* p, const float* x) {
    if (ALIGNED) {
        *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
        p[0] = x[0], p[1] = x[1], p[2] = x[2], p[3] = x[3];
    }
}

// one chunk of one tensor: elements [base, min(base + ADAM_CHUNK, n))
template <bool ALIGNED, bool AMSGRAD>
__device__ __forceinline__ void adam_chunk(const AdamScalars& s, float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M,
                                           float* __restrict__ V, float* __restrict__ X, long long base, long long n) {
    constexpr int Q = ADAM_CHUNK / (AT * 4);
    float p[Q][4], g[Q][4], m[Q][4], v[Q][4], x[Q][4];
    bool full[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {                                         // every load of the chunk first: 5 Q independent loads in flight
        const long long e = base + ((long long)i * AT + threadIdx.x) * 4;
        full[i] = e + 4 <= n;
        if (full[i]) {
            load4<ALIGNED>(P + e, p[i]);
            load4<ALIGNED>(G + e, g[i]);
            load4<ALIGNED>(M + e, m[i]);
            load4<ALIGNED>(V + e, v[i]);
            if (AMSGRAD) load4<ALIGNED>(X + e, x[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const long long e = base + ((long long)i * AT + threadIdx.x) * 4;
        if (full[i]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) adam_elem<AMSGRAD>(s, p[i][k], g[i][k], m[i][k], v[i][k], x[i][k]);
            store4<ALIGNED>(P + e, p[i]);
            store4<ALIGNED>(M + e, m[i]);
            store4<ALIGNED>(V + e, v[i]);
            if (AMSGRAD) store4<ALIGNED>(X + e, x[i]);
        } else {
            for (long long k = e; k < n; ++k) {                           // the partial quad at the end of the tensor (no trip when e >= n)
                float pk = P[k], mk = M[k], vk = V[k], xk = AMSGRAD ? X[k] : 0.f;
                adam_elem<AMSGRAD>(s, pk, G[k], mk, vk, xk);
                P[k] = pk, M[k] = mk, V[k] = vk;
                if (AMSGRAD) X[k] = xk;
            }
        }
    }
}

template <bool AMSGRAD>
__global__ void __launch_bounds__(AT) adam_kernel(const AdamBatch a) {
    // the tensor of this workgroup: the last i with prefix[i] <= blockIdx.x (a tensor without elements owns no chunk and is never
    // found: its prefix equals its successor's).  prefix[ADAM_BATCH] > blockIdx.x always, so i <= ADAM_BATCH - 1.
    const unsigned w = blockIdx.x;
    int lo = 0, hi = ADAM_BATCH;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.prefix[mid] <= w)
            lo = mid;
        else
            hi = mid;
    }
    const int i = lo;
    const long long n = a.numel[i];
    const long long base = (long long)(w - a.prefix[i]) * ADAM_CHUNK;
    const AdamScalars s = {a.wd, a.omb1, a.b2, a.omb2, a.eps, a.ss[i], a.rb[i]};
    if ((a.aligned >> i) & 1ull)                                           // uniform over the workgroup
        adam_chunk<true, AMSGRAD>(s, a.p[i], a.g[i], a.m[i], a.v[i], a.vmax[i], base, n);
    else
        adam_chunk<false, AMSGRAD>(s, a.p[i], a.g[i], a.m[i], a.v[i], a.vmax[i], base, n);
}

inline int adam_launch(AdamBatch& b, int count, unsigned chunks, bool amsgrad, hipStream_t st) {
    for (int i = count; i < ADAM_BATCH; ++i) {                            // unused slots: no chunk, never found by the search
        b.p[i] = b.m[i] = b.v[i] = b.vmax[i] = nullptr, b.g[i] = nullptr;
        b.numel[i] = 0, b.ss[i] = b.rb[i] = 0.f;
    }
    for (int i = count; i <= ADAM_BATCH; ++i) b.prefix[i] = chunks;
    if (chunks == 0) return APG_OK;
    if (amsgrad)
        hipLaunchKernelGGL(adam_kernel<true>, dim3(chunks), dim3(AT), 0, st, b);
    else
        hipLaunchKernelGGL(adam_kernel<false>, dim3(chunks), dim3(AT), 0, st, b);
    APG_TRY(hipGetLastError());
    return APG_OK;
}

}  // namespace

extern "C" {

int apg_adam_step(int ntensors, const void* const* p, const void* const* g, const void* const* m, const void* const* v,
                  const void* const* vmax, const int64_t* numel, const int64_t* step, double lr, double beta1, double beta2, double eps,
                  double weight_decay, void* stream) {
    if (ntensors < 0) return apg_fail(APG_EINVAL, "apg_adam_step: ntensors must be >= 0");
    if (!(lr >= 0.0)) return apg_fail(APG_EINVAL, "apg_adam_step: lr must be >= 0");
    if (!(eps >= 0.0)) return apg_fail(APG_EINVAL, "apg_adam_step: eps must be >= 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return apg_fail(APG_EINVAL, "apg_adam_step: beta1 must be in [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return apg_fail(APG_EINVAL, "apg_adam_step: beta2 must be in [0, 1)");
    if (!(weight_decay >= 0.0)) return apg_fail(APG_EINVAL, "apg_adam_step: weight_decay must be >= 0");
    if (!p) return apg_fail(APG_EINVAL, "apg_adam_step: the p table is NULL");
    if (!g) return apg_fail(APG_EINVAL, "apg_adam_step: the g table is NULL");
    if (!m) return apg_fail(APG_EINVAL, "apg_adam_step: the m table is NULL");
    if (!v) return apg_fail(APG_EINVAL, "apg_adam_step: the v table is NULL");
    if (!numel) return apg_fail(APG_EINVAL, "apg_adam_step: the numel array is NULL");
    if (!step) return apg_fail(APG_EINVAL, "apg_adam_step: the step array is NULL");
    const bool amsgrad = vmax != nullptr;
    // every tensor is checked before the first launch: a refused call has changed nothing
    for (int i = 0; i < ntensors; ++i) {
        const std::string at = " of tensor " + std::to_string(i);
        if (numel[i] < 0) return apg_fail(APG_EINVAL, "apg_adam_step: numel" + at + " is negative");
        if (step[i] < 1) return apg_fail(APG_EINVAL, "apg_adam_step: step" + at + " must be >= 1 (the count after this update)");
        // a launch's grid holds at most 2^31 - 1 chunks
        if (numel[i] > (int64_t)0x7fffffff * ADAM_CHUNK) return apg_fail(APG_EINVAL, "apg_adam_step: numel" + at + " is too large");
        const void* q[5] = {p[i], g[i], m[i], v[i], amsgrad ? vmax[i] : nullptr};
        static const char* const name[5] = {"p", "g", "m", "v", "vmax"};
        for (int k = 0; k < (amsgrad ? 5 : 4); ++k) {
            if (numel[i] > 0 && !q[k]) return apg_fail(APG_EINVAL, std::string("apg_adam_step: ") + name[k] + at + " is NULL");
            if ((uintptr_t)q[k] & 3) return apg_fail(APG_EINVAL, std::string("apg_adam_step: ") + name[k] + at + " is not 4-byte aligned");
        }
    }

    AdamBatch b;
    b.wd = (float)weight_decay, b.omb1 = (float)(1.0 - beta1), b.b2 = (float)beta2, b.omb2 = (float)(1.0 - beta2), b.eps = (float)eps;
    b.aligned = 0;
    int count = 0;
    unsigned chunks = 0;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < ntensors; ++i) {
        if (numel[i] == 0) continue;
        const unsigned nc = (unsigned)((numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK);
        if (count == ADAM_BATCH || nc > 0x7fffffffu - chunks) {           // the batch is full, or its grid would be
            const int rc = adam_launch(b, count, chunks, amsgrad, st);
            if (rc != APG_OK) return rc;
            count = 0, chunks = 0, b.aligned = 0;
        }
        const uintptr_t bits = (uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i] | (amsgrad ? (uintptr_t)vmax[i] : 0);
        b.p[count] = (float*)p[i], b.g[count] = (const float*)g[i], b.m[count] = (float*)m[i], b.v[count] = (float*)v[i];
        b.vmax[count] = amsgrad ? (float*)vmax[i] : nullptr;
        b.numel[count] = numel[i];
        const double t = (double)step[i];
        b.ss[count] = (float)(lr / (1.0 - std::pow(beta1, t)));
        b.rb[count] = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, t)));
        b.prefix[count] = chunks;
        if ((bits & 15) == 0) b.aligned |= 1ull << count;
        chunks += nc;
        ++count;
    }
    return adam_launch(b, count, chunks, amsgrad, st);
}

}  // extern "C"
