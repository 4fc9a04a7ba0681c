// What the workgroup-per-row reductions of libairpose_grad.so share, once, for loss_grad.hip, loss_real_grad.hip and geom_grad.hip:
// the workgroup size, the fixed-order LDS tree, and the two losses' joint count and limb weights.  Included inside each file's
// unnamed namespace.

constexpr int LT = 256;                  // threads per workgroup
constexpr int NJ = 22;                   // joints the losses read

// fixed-order tree over the LT threads of NV values each (s: LT * NV floats of LDS); result k in s[k * LT]
template <int NV>
__device__ __forceinline__ void block_reduce(float* s, const float* v) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k * LT + t] = v[k];
    __syncthreads();
    for (int h = LT / 2; h > 0; h >>= 1) {
        if (t < h)
#pragma unroll
            for (int k = 0; k < NV; ++k) s[k * LT + t] += s[k * LT + t + h];
        __syncthreads();
    }
}

// limb weight of joint j: {4, 5, 18, 19} -> l, {7, 8, 20, 21} -> l^2.  The training loss's pose term asks with j = its own index + 1
// (the root is not among its 21 rotations), which gives the reference's {3, 4, 17, 18} and {6, 7, 19, 20}.
__device__ __forceinline__ float limb_weight(int j, float l, float l2) {
    if (j == 4 || j == 5 || j == 18 || j == 19) return l;
    if (j == 7 || j == 8 || j == 20 || j == 21) return l2;
    return 1.f;
}
