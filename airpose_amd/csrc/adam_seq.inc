// The Adam / AMSGrad sequence and its host side, ONE text for the two sources that launch it: optim.hip (apg_adam_step:
// adam_kernel<AMSGRAD> = adam_body<AMSGRAD, false>) and guard/grad_guard.hip (apg_adam_step_guarded: adam_guarded_kernel<AMSGRAD> =
// adam_body<AMSGRAD, true>, which reads the guard record first).  optim.hip's header comment states the partition and the sequence.
// Include after grad_internal.h; everything here is in the including source's anonymous namespace, and the pragma holds to its end.
#include <cmath>
#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int AT = 256;                  // threads per workgroup
constexpr int ADAM_CHUNK = 4096;         // elements per workgroup: 256 threads x 4 quads of 4
constexpr int ADAM_BATCH = 64;           // tensors per launch

// include/airpose_grad.h: the guard record, 16 bytes
struct GuardRecord {
    float coef;                          // (float) min(1, max_norm / (sqrt(S) + 1e-6)); 1 when skip is set
    float norm;                          // (float) sqrt(S)
    int skip;                            // 1: S is non-finite and skip_nonfinite was asked for
    int reserved;                        // written as 0
};
static_assert(sizeof(GuardRecord) == APG_GUARD_BYTES, "the header states the record's size");

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
    const struct GuardRecord* guard;     // adam_body<.., true> only: what apg_grad_norm wrote
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
template <bool ALIGNED, bool AMSGRAD, bool GUARDED>
__device__ __forceinline__ void adam_chunk(const AdamScalars& s, float coef, float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M,
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
            for (int k = 0; k < 4; ++k) {
                if (GUARDED) g[i][k] = __fmul_rn(coef, g[i][k]);          // the clipped gradient: one rounded product, then the sequence
                adam_elem<AMSGRAD>(s, p[i][k], g[i][k], m[i][k], v[i][k], x[i][k]);
            }
            store4<ALIGNED>(P + e, p[i]);
            store4<ALIGNED>(M + e, m[i]);
            store4<ALIGNED>(V + e, v[i]);
            if (AMSGRAD) store4<ALIGNED>(X + e, x[i]);
        } else {
            for (long long k = e; k < n; ++k) {                           // the partial quad at the end of the tensor (no trip when e >= n)
                float pk = P[k], mk = M[k], vk = V[k], xk = AMSGRAD ? X[k] : 0.f;
                adam_elem<AMSGRAD>(s, pk, GUARDED ? __fmul_rn(coef, G[k]) : G[k], mk, vk, xk);
                P[k] = pk, M[k] = mk, V[k] = vk;
                if (AMSGRAD) X[k] = xk;
            }
        }
    }
}

// one workgroup of the step: what adam_kernel and adam_guarded_kernel run
template <bool AMSGRAD, bool GUARDED>
__device__ __forceinline__ void adam_body(const AdamBatch& a) {
    float coef = 1.f;
    if (GUARDED) {                                                        // uniform: with skip set the workgroup stores nothing
        if (a.guard->skip) return;
        coef = a.guard->coef;
    }
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
        adam_chunk<true, AMSGRAD, GUARDED>(s, coef, a.p[i], a.g[i], a.m[i], a.v[i], a.vmax[i], base, n);
    else
        adam_chunk<false, AMSGRAD, GUARDED>(s, coef, a.p[i], a.g[i], a.m[i], a.v[i], a.vmax[i], base, n);
}

template <class Launch>
inline int adam_launch(AdamBatch& b, int count, unsigned chunks, bool amsgrad, hipStream_t st, Launch&& launch) {
    for (int i = count; i < ADAM_BATCH; ++i) {                            // unused slots: no chunk, never found by the search
        b.p[i] = b.m[i] = b.v[i] = b.vmax[i] = nullptr, b.g[i] = nullptr;
        b.numel[i] = 0, b.ss[i] = b.rb[i] = 0.f;
    }
    for (int i = count; i <= ADAM_BATCH; ++i) b.prefix[i] = chunks;
    if (chunks == 0) return APG_OK;
    launch(b, chunks, amsgrad, st);                                       // the including source's kernel: plain or guarded
    APG_TRY(hipGetLastError());
    return APG_OK;
}

// apg_adam_step (guard = nullptr, its check skipped) and apg_adam_step_guarded; f = the entry's name for the messages
template <class Launch>
int adam_step(const std::string& f, bool guarded, int ntensors, const void* const* p, const void* const* g, const void* const* m,
              const void* const* v, const void* const* vmax, const int64_t* numel, const int64_t* step, double lr, double beta1, double beta2,
              double eps, double weight_decay, const void* guard, void* stream, Launch&& launch) {
    if (ntensors < 0) return apg_fail(APG_EINVAL, f + "ntensors must be >= 0");
    if (!(lr >= 0.0)) return apg_fail(APG_EINVAL, f + "lr must be >= 0");
    if (!(eps >= 0.0)) return apg_fail(APG_EINVAL, f + "eps must be >= 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return apg_fail(APG_EINVAL, f + "beta1 must be in [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return apg_fail(APG_EINVAL, f + "beta2 must be in [0, 1)");
    if (!(weight_decay >= 0.0)) return apg_fail(APG_EINVAL, f + "weight_decay must be >= 0");
    if (!p) return apg_fail(APG_EINVAL, f + "the p table is NULL");
    if (!g) return apg_fail(APG_EINVAL, f + "the g table is NULL");
    if (!m) return apg_fail(APG_EINVAL, f + "the m table is NULL");
    if (!v) return apg_fail(APG_EINVAL, f + "the v table is NULL");
    if (!numel) return apg_fail(APG_EINVAL, f + "the numel array is NULL");
    if (!step) return apg_fail(APG_EINVAL, f + "the step array is NULL");
    if (guarded && !guard) return apg_fail(APG_EINVAL, f + "the guard record is NULL");
    if ((uintptr_t)guard & 3) return apg_fail(APG_EINVAL, f + "the guard record is not 4-byte aligned");
    const bool amsgrad = vmax != nullptr;
    // every tensor is checked before the first launch: a refused call has changed nothing
    for (int i = 0; i < ntensors; ++i) {
        const std::string at = " of tensor " + std::to_string(i);
        if (numel[i] < 0) return apg_fail(APG_EINVAL, f + "numel" + at + " is negative");
        if (step[i] < 1) return apg_fail(APG_EINVAL, f + "step" + at + " must be >= 1 (the count after this update)");
        // a launch's grid holds at most 2^31 - 1 chunks
        if (numel[i] > (int64_t)0x7fffffff * ADAM_CHUNK) return apg_fail(APG_EINVAL, f + "numel" + at + " is too large");
        const void* q[5] = {p[i], g[i], m[i], v[i], amsgrad ? vmax[i] : nullptr};
        static const char* const name[5] = {"p", "g", "m", "v", "vmax"};
        for (int k = 0; k < (amsgrad ? 5 : 4); ++k) {
            if (numel[i] > 0 && !q[k]) return apg_fail(APG_EINVAL, f + name[k] + at + " is NULL");
            if ((uintptr_t)q[k] & 3) return apg_fail(APG_EINVAL, f + name[k] + at + " is not 4-byte aligned");
        }
    }

    AdamBatch b;
    b.wd = (float)weight_decay, b.omb1 = (float)(1.0 - beta1), b.b2 = (float)beta2, b.omb2 = (float)(1.0 - beta2), b.eps = (float)eps;
    b.aligned = 0;
    b.guard = (const GuardRecord*)guard;
    int count = 0;
    unsigned chunks = 0;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < ntensors; ++i) {
        if (numel[i] == 0) continue;
        const unsigned nc = (unsigned)((numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK);
        if (count == ADAM_BATCH || nc > 0x7fffffffu - chunks) {           // the batch is full, or its grid would be
            const int rc = adam_launch(b, count, chunks, amsgrad, st, launch);
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
    return adam_launch(b, count, chunks, amsgrad, st, launch);
}

}  // namespace
