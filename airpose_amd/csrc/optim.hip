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
// The sequence itself, AdamBatch and the host side are adam_seq.inc, shared with guard/grad_guard.hip (apg_adam_step_guarded), so that
// the guarded step has no second copy of them; this source's two kernels are adam_body<AMSGRAD, false>.
#include "grad_internal.h"

#include "adam_seq.inc"

namespace {

template <bool AMSGRAD>
__global__ void __launch_bounds__(AT) adam_kernel(const AdamBatch a) {
    adam_body<AMSGRAD, false>(a);
}

}  // namespace

extern "C" {

int apg_adam_step(int ntensors, const void* const* p, const void* const* g, const void* const* m, const void* const* v,
                  const void* const* vmax, const int64_t* numel, const int64_t* step, double lr, double beta1, double beta2, double eps,
                  double weight_decay, void* stream) {
    return adam_step("apg_adam_step: ", false, ntensors, p, g, m, v, vmax, numel, step, lr, beta1, beta2, eps, weight_decay, nullptr, stream,
                     [](const AdamBatch& b, unsigned chunks, bool amsgrad, hipStream_t st) {
                         if (amsgrad)
                             hipLaunchKernelGGL(adam_kernel<true>, dim3(chunks), dim3(AT), 0, st, b);
                         else
                             hipLaunchKernelGGL(adam_kernel<false>, dim3(chunks), dim3(AT), 0, st, b);
                     });
}

}  // extern "C"
