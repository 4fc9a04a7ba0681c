// What the metric sources of libairpose_grad.so share, once, for eval_metrics.hip, eval_align.hip and xview_metrics.hip: the fp32 norm
// every error is, the workgroup's fixed-order fp64 sum, the combine kernel that makes the metrics bit-reproducible, and the host checks
// of the arguments the entry points have in common.  Included inside each file's unnamed namespace, after its `#pragma clang fp contract(off)`.

__device__ __forceinline__ float norm3(float d0, float d1, float d2) { return sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0))); }

// v[k] summed over the workgroup in a fixed order; every thread returns with the totals in tot[0 .. NV)
template <int NT, int NV>
__device__ __forceinline__ void wg_sum(double (&v)[NV], double* red, double* tot) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_down(v[k], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = red[threadIdx.x];
        for (int w = 1; w < NW; ++w) s += red[w * NV + threadIdx.x];      // waves in index order
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

constexpr int COMBINE_NT = 64;           // one workgroup of one wave: a thread per (view, sum), then one per view for the counts
constexpr int COMBINE_COUNTS = 3;

struct CombineArgs {
    int n, views, B;                                     // n partials of each sum, left by the main kernel
    int nsum, pitch;                                     // sums per view; the accumulator of view v starts at acc[v * pitch]
    long long stride, view_stride;                       // partial i of sum q of view v: part[i * stride + v * view_stride + q]
    unsigned skip[2];                                    // per view: bit q set = sum q is left alone
    int count_slot[COMBINE_COUNTS];                      // acc[v * pitch + count_slot[k]] += B where count_on[v][k]
    int count_on[2][COMBINE_COUNTS];
    const double* part;
    double* acc;
};

// each sum's partials added in index order, in fp64, from 0.0, then ONE add into acc[v * pitch + 1 + q]; view 1 untouched with one view
__global__ void __launch_bounds__(COMBINE_NT) metric_combine_kernel(const CombineArgs c) {
    const int t = threadIdx.x;
    if (t < c.views * c.nsum) {
        const int v = t / c.nsum, q = t - v * c.nsum;
        if (((v ? c.skip[1] : c.skip[0]) >> q) & 1) return;
        const double* p = c.part + (size_t)v * (size_t)c.view_stride + q;
        double sum = 0.0;
        for (int i = 0; i < c.n; ++i) sum += p[(size_t)i * (size_t)c.stride];
        c.acc[v * c.pitch + 1 + q] += sum;
    } else if (t < c.views * c.nsum + c.views) {
        const int v = t - c.views * c.nsum;
#pragma unroll
        for (int k = 0; k < COMBINE_COUNTS; ++k)
            if (v ? c.count_on[1][k] : c.count_on[0][k]) c.acc[v * c.pitch + c.count_slot[k]] += (double)c.B;
    }
}

// the host checks, under the entry point's names; in steps, because each entry point has checks of its own between them and a call
// with two mistakes is told of the same one as ever
struct MetricChecks {
    std::string f;                                       // "apg_..._update: "
    int views;
    const void* const* per_view;                         // [views][per] device pointers
    int per, required;                                   // entries per view; the first `required` must not be NULL
    const char* const* name;                             // [per]
    const void *acc, *workspace;
    int64_t workspace_bytes, need;
    const char* query;                                   // the size query that gave `need`

    int bad(const std::string& what) const { return apg_fail(APG_EINVAL, f + what); }
    int views_ok() const { return views != 1 && views != 2 ? bad("views must be 1 or 2") : APG_OK; }
    int table_ok() const { return !per_view ? bad("the per_view table is NULL") : APG_OK; }
    int sinks_ok() const { return !acc ? bad("acc is NULL") : !workspace ? bad("workspace is NULL") : APG_OK; }
    int view_ok(int v) const {
        const void* const* q = per_view + v * per;
        const std::string at = " of view " + std::to_string(v);
        for (int k = 0; k < per; ++k) {
            if (k < required && !q[k]) return bad(name[k] + at + " is NULL");
            if ((uintptr_t)q[k] & 3) return bad(name[k] + at + " is not 4-byte aligned");
        }
        return APG_OK;
    }
    int sizes_ok() const {
        if ((uintptr_t)acc & 7) return bad("acc is not 8-byte aligned");
        if ((uintptr_t)workspace & 7) return bad("workspace is not 8-byte aligned");
        if (workspace_bytes < need)
            return apg_fail(APG_ENOMEM, f + "workspace of " + std::to_string(workspace_bytes) + " bytes, " + query + " asks for " +
                                            std::to_string(need));
        return APG_OK;
    }
};
