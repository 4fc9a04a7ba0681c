// The hand-placed primitives of the 16-bit forward conv kernels (the H16SRCS of the Makefile): how this library places a load, a
// wait and an MFMA.  Included inside AP_NS_BEGIN / an anonymous namespace by each kernel source, so the 16-bit storage type stays
// a property of the compilation (bf16 or, with -DAP_F16, fp16: ap_common.h).  ONE definition per emitted form; where two kernels
// need different instructions both forms are here, named by their difference, with the reason beside them.  The packed
// conversion and the packed ReLU (pack_bf16x2, ap_relu_pk) are in ap_common.h.
//
// The rules behind all of it.  Left to hipcc (first cut of block_img.hip, bit-identical results, 3x slower) every operand
// fragment was read right in front of its four MFMAs behind an s_waitcnt lgkmcnt(0), every weight prefetch was sunk to its use
// behind vmcnt(0), and the accumulators wandered between the two register halves.  So: loads are asm statements the compiler
// cannot move and does not count, a destination is valid only behind the counted wait that covers it, and an MFMA updates its
// accumulator in place.  vmcnt / lgkmcnt retire in order per type, so a wait for "at most N younger operations" is exact when N
// operations are known to follow the target and merely conservative when more do.
//
// Not here: mma_issue ("N MFMAs with NP callbacks spread between them") stays a copy each in conv_slab.hip and conv_pipe.hip --
// conv_pipe.hip's is a template on the element type with an fp32 branch, the RP_PIECES placements and the builtin MFMA behind
// RP_ABLATE, conv_slab.hip's issues the tied asm MFMA on fixed FM x FN; one function would carry the first one's branches into
// the second.
#pragma once
template <int I, int N, typename F> __device__ __forceinline__ void sfor(F&& f) {      // compile-time loop: f(integral_constant<I>) .. <N - 1>
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sfor<I + 1, N>(f);
    }
}
typedef __attribute__((ext_vector_type(2))) float f32x2;

// ---- waits.  -DAP_SAFE=1 turns every counted vmcnt into vmcnt(0), 2 every counted lgkmcnt as well: cross-check builds (a
// result that changes under them names a miscounted wait); `make variant SRC=... DEF=-DAP_SAFE=2`
#ifndef AP_SAFE
#define AP_SAFE 0
#endif
// vmcnt, fenced: nothing is scheduled across it (register-only instructions ignore the "memory" clobber, and a wait is followed
// by uses of registers an asm load wrote).  bottleneck2, conv_pair, block_img, conv_pw, conv_img3, conv_s2p
template <int N> __device__ __forceinline__ void ap_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AP_SAFE ? 0 : N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// vmcnt, bare: the wait alone.  Enough where it covers LDS-DMA pieces only (no register destination; the s_barrier behind it
// and the volatile asm reads behind that keep their order), and the compiler stays free to move address arithmetic across it.
// Not interchangeable with the fenced form: the fence changes these kernels' schedules.  conv_pipe, conv_slab, conv_lean
template <int N> __device__ __forceinline__ void ap_wait_vm_bare() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AP_SAFE ? 0 : N) : "memory"); }
// lgkmcnt: always fenced -- keeps register-only MFMAs below the wait (they ignore "memory")
template <int N> __device__ __forceinline__ void ap_wait_lgkm() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(AP_SAFE > 1 ? 0 : N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- LDS.  A fragment read the compiler does not count: hipcc answers a ds_read pending across the loop back-edge with
// lgkmcnt(0), which serialises the fragment double-buffering; the waits are placed by hand instead.
// return-value form: the destination register is the compiler's choice per call
template <int OFF> __device__ __forceinline__ u32x4 ap_lds_read(uint32_t addr) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
// out-parameter form: reads INTO a named register of a fragment ring (ap_frag_pipe: the register is free again when the read LA
// groups ahead is issued)
template <int OFF> __device__ __forceinline__ void ap_lds_read_to(u32x4& r, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
}
// fp32 table rows (BatchNorm scale / shift) are read as f32x4 AT ONCE: __builtin_bit_cast applied to ONE ELEMENT of an integer
// vector mis-compiles with this hipcc -- every element but the first comes out wrong (conv_pipe.hip's epilogue carries the same
// note); the whole-vector cast is a register rename
template <int OFF> __device__ __forceinline__ f32x4 ap_lds_read_f32x4(uint32_t addr) { return __builtin_bit_cast(f32x4, ap_lds_read<OFF>(addr)); }
// asm write (its wait is a counted lgkmcnt as well).  bottleneck2: t1 to LDS
template <int OFF> __device__ __forceinline__ void ap_lds_write(uint32_t addr, const u32x4& v) {
    asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
// plain C++ assignment, counted and ordered by the compiler (zeroing, staging behind a __syncthreads)
__device__ __forceinline__ void ap_lds_assign(unsigned char* smem, uint32_t off, const u32x4& v) {
    *(u32x4*)__builtin_assume_aligned(smem + off, 16) = v;
}
// LDS-DMA of 16 bytes per lane with the LDS base written to m0 by hand, from a computed 32-bit LDS address (a wave-uniform value:
// an "s" operand).  s_nop 0: a wait state between the scalar write of m0 and the load that takes its LDS base from it.
// conv_img3, conv_s2p: the feeding loops of the image-resident 3x3 kernels
__device__ __forceinline__ void ap_dma_lds_m0(uint32_t m0v, const unsigned char* src) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(m0v), "v"(src) : "memory", "m0");
}

// ---- global loads into registers.  A register load the compiler does not count (a load it counts is answered with vmcnt(0)
// beside LDS-DMA and would drain the weight ring): the destination is valid only behind the hand-placed wait that names it
// 64-bit VGPR address, default cache policy
template <int OFF> __device__ __forceinline__ u32x4 ap_gld(const unsigned char* p) {
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
    return r;
}
// ... streaming (nt): activations that are read once (conv_pair: t2 / identity / x2, +0.3 % on the whole bench)
template <int OFF> __device__ __forceinline__ u32x4 ap_gld_nt(const unsigned char* p) {
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
    return r;
}
// uniform base (SGPR pair) + 32-bit lane offset: one VGPR per address instead of two (the launchers keep every tensor below 4 GB).
// Two forms, and the difference is a hardware hazard: a VALU write of an SGPR (v_readlane / v_readfirstlane) followed by a VMEM
// read of that SGPR needs 5 wait states, and hipcc pads nothing in front of an asm statement.
// PADDED (block_img, conv_pw, conv_img3, conv_s2p): the base may come straight out of a v_readlane / v_readfirstlane (an SGPR the
// compiler had spilled to a VGPR lane, or the readfirstlane below).  Without the s_nop 4 the load now and then used the PREVIOUS
// value of the pair (seen: the identity of image row 5 added to row 6)
template <int OFF> __device__ __forceinline__ void ap_gld_sbase_pad(u32x4& r, uint32_t voff, const unsigned char* sbase) {
    // (the bases are uniform by construction; readfirstlane makes that provable where hipcc lost track: folded away otherwise)
    const uint64_t u = (uint64_t)sbase;
    const uint64_t su = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(su), "n"(OFF) : "memory");
}
// UNPADDED (bottleneck2: x fragments).  Sound only while the last write of the base pair in front of the load is a scalar one
// (s_load of a kernel argument behind its s_waitcnt, s_mov, s_add: the scalar unit interlocks those) or a VALU write at least
// 5 wait states earlier: i.e. while the pair is never a v_readfirstlane result or reloaded from a spill lane (v_readlane) right
// in front of the load.  bottleneck2's one call site passes the kernel argument x, brought into SGPRs by the empty asm behind
// the argument loads.  Read in the assembly of this build, all six kernels (three variants x bf16 / fp16): the pair (s[12:13];
// s[24:25] in the first-block variant) is written ONCE, by the s_load of the kernel arguments at the kernel's entry; the kernels
// have no SGPR spill (.sgpr_spill_count 0, no v_readlane / v_writelane), and their v_readfirstlane results go to other
// registers.  The condition holds.  It is a property of the register allocation: re-read it when that kernel's SGPR pressure
// changes, or use the padded form
template <int OFF> __device__ __forceinline__ u32x4 ap_gld_sbase(uint32_t voff, const unsigned char* sbase) {
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
    return r;
}

// ---- MFMA on u32x4 fragments (w: 16 rows x 8 K values of the weight tile, x: 16 pixels x 8 K values, per lane group)
// through the builtin: the compiler schedules it, pads its hazards and may move the accumulator (d != c).  bottleneck2,
// conv_pair, conv_pipe, whose accumulators are few enough to stay put
__device__ __forceinline__ f32x4 ap_mfma_frag(const u32x4& w, const u32x4& x, const f32x4& c) {
    return ap_mfma16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), c);
}
// as asm with the accumulator tied in place.  With the nine taps of conv_slab unrolled the register allocator otherwise lets the
// eight accumulators migrate (v_mfma d, a, b, c with d != c), which costs ~25 registers and spills; spill reloads sit behind
// s_waitcnt vmcnt(0) and would drain the DMA queue every K step.  Hazards the compiler no longer sees: consecutive MFMAs never
// share an accumulator back to back with different operands, and the first VALU read of an accumulator is fenced by a settle
// pad (below).
// "+v": accumulators in the architectural VGPRs (conv_slab, conv_lean: 8 accumulators, <= 128 registers, two / three workgroups per CU)
__device__ __forceinline__ void ap_mfma_acc_v(f32x4& c, const u32x4& w, const u32x4& x) {
    asm volatile(AP_MFMA16_ASM " %0, %1, %2, %0" : "+v"(c) : "v"(w), "v"(x));
}
// "+a": accumulators in the AGPR half (the one-wave-per-SIMD kernels: up to 56 accumulators, the VGPR half holds operands and rings)
__device__ __forceinline__ void ap_mfma_acc_a(f32x4& c, const u32x4& w, const u32x4& x) {
    asm volatile(AP_MFMA16_ASM " %0, %1, %2, %0" : "+a"(c) : "v"(w), "v"(x));
}
__device__ __forceinline__ void ap_mfma_zero_a(f32x4& c, const u32x4& w, const u32x4& x) {      // first K step: C = 0
    asm volatile(AP_MFMA16_ASM " %0, %1, %2, 0" : "=a"(c) : "v"(w), "v"(x));
}
// The last MFMAs' results must settle before a VALU instruction reads them, and hipcc pads nothing around an asm MFMA.
// Operand form: the nops name the accumulators (two arrays of N) as operands, or the compiler hoists its v_accvgpr_read above
// them (it did: register-only instructions ignore a "memory" clobber).  N = 14: block_img, conv_pw, conv_img3; N = 7: conv_s2p
template <int N> __device__ __forceinline__ void ap_settle(f32x4 (&p)[N], f32x4 (&q)[N]) {
    static_assert(N == 7 || N == 14, "an asm statement's operands are written out");
    if constexpr (N == 14)
        asm volatile("s_nop 15\n\ts_nop 15"
                     : "+a"(p[0]), "+a"(p[1]), "+a"(p[2]), "+a"(p[3]), "+a"(p[4]), "+a"(p[5]), "+a"(p[6]), "+a"(p[7]), "+a"(p[8]), "+a"(p[9]),
                       "+a"(p[10]), "+a"(p[11]), "+a"(p[12]), "+a"(p[13]), "+a"(q[0]), "+a"(q[1]), "+a"(q[2]), "+a"(q[3]), "+a"(q[4]),
                       "+a"(q[5]), "+a"(q[6]), "+a"(q[7]), "+a"(q[8]), "+a"(q[9]), "+a"(q[10]), "+a"(q[11]), "+a"(q[12]), "+a"(q[13]));
    else
        asm volatile("s_nop 15\n\ts_nop 15"
                     : "+a"(p[0]), "+a"(p[1]), "+a"(p[2]), "+a"(p[3]), "+a"(p[4]), "+a"(p[5]), "+a"(p[6]), "+a"(q[0]), "+a"(q[1]), "+a"(q[2]),
                       "+a"(q[3]), "+a"(q[4]), "+a"(q[5]), "+a"(q[6]));
    __builtin_amdgcn_sched_barrier(0);
}
// Bare form: a "memory" clobber only -- nothing ties the accumulators to the pad, so by the note above the compiler COULD hoist a
// read of them over it.  It does not in conv_slab and conv_lean (a branch or a barrier follows the pad, the epilogue's reads
// come behind that); new code takes the operand form
__device__ __forceinline__ void ap_settle_bare() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }

// ---- the register epilogue.  Row rho of a wave's weight tile holds channel ap_row_channel(rho) of the tile: fragment
// f = rho >> 4, row i of it; lane group g4 of fragment PAIR q = f >> 1 owns channels q*32 + g4*8 .. + 7 (fragment f = 2q + e
// holds e*4 .. e*4 + 3 of them).  A lane's accumulator elements of a fragment pair are then 8 CONSECUTIVE channels = one 16-byte
// piece of a B fragment / of an NHWC row.  The pack kernels and in-kernel weight loads permute by it
__host__ __device__ __forceinline__ int ap_row_channel(int rho) {
    const int f = rho >> 4, i = rho & 15;
    return (f >> 1) * 32 + (i >> 2) * 8 + (f & 1) * 4 + (i & 3);
}
// BN (+ identity) + ReLU + 16-bit of the 8 consecutive channels a lane holds in fragments (2q, 2q+1) = lo, hi; s0 s1 / h0 h1:
// their scale / shift rows; res: the identity's 16 bytes or nullptr; rng: the fp16 range sentinel's running maximum
// (ap_common.h).  The expression of the stand-alone kernels' epilogue (fma, add, max, round), two values per instruction
// (v_pk_fma_f32 / v_pk_add_f32: the same IEEE fma / add per component), one v_cvt_pk + one packed integer max per pair.
// (conv_pair.hip carries the same text as a lambda of its own and says why: keep the two alike)
__device__ __forceinline__ u32x4 ap_bn8(const f32x4& lo, const f32x4& hi, const f32x4& s0, const f32x4& s1, const f32x4& h0,
                                        const f32x4& h1, const u32x4* res, uint32_t& rng) {
    f32x2 v0 = __builtin_elementwise_fma(lo.xy, s0.xy, h0.xy), v1 = __builtin_elementwise_fma(lo.zw, s0.zw, h0.zw);
    f32x2 v2 = __builtin_elementwise_fma(hi.xy, s1.xy, h1.xy), v3 = __builtin_elementwise_fma(hi.zw, s1.zw, h1.zw);
    if (res) {
        const uint32_t r0 = (*res).x, r1 = (*res).y, r2 = (*res).z, r3 = (*res).w;
#ifdef AP_F16
        { float a_ = v0.x, b_ = v0.y; ap_res_add2(a_, b_, r0); v0 = f32x2{a_, b_}; }
        { float a_ = v1.x, b_ = v1.y; ap_res_add2(a_, b_, r1); v1 = f32x2{a_, b_}; }
        { float a_ = v2.x, b_ = v2.y; ap_res_add2(a_, b_, r2); v2 = f32x2{a_, b_}; }
        { float a_ = v3.x, b_ = v3.y; ap_res_add2(a_, b_, r3); v3 = f32x2{a_, b_}; }
#else
        { float a_, b_; unpack_bf16x2(r0, a_, b_); v0 += f32x2{a_, b_}; }
        { float a_, b_; unpack_bf16x2(r1, a_, b_); v1 += f32x2{a_, b_}; }
        { float a_, b_; unpack_bf16x2(r2, a_, b_); v2 += f32x2{a_, b_}; }
        { float a_, b_; unpack_bf16x2(r3, a_, b_); v3 += f32x2{a_, b_}; }
#endif
    }
    u32x4 o;
    o.x = ap_relu_pk(pack_bf16x2(v0.x, v0.y)); o.y = ap_relu_pk(pack_bf16x2(v1.x, v1.y));
    o.z = ap_relu_pk(pack_bf16x2(v2.x, v2.y)); o.w = ap_relu_pk(pack_bf16x2(v3.x, v3.y));
    ap_rng_note2(rng, o.x, o.y); ap_rng_note2(rng, o.z, o.w);
    return o;
}

// B-fragment pipeline of one segment of NR 16-pixel groups: LA reads in flight ahead of the MFMAs (LA fragment registers in use)
// (NB fragment registers: a register is free again when the read LA groups ahead is issued, so NB > LA)
template <int NR, int LA, int NB = 16, typename RD, typename USE> __device__ __forceinline__ void ap_frag_pipe(u32x4 (&b)[NB], RD&& rd, USE&& use) {
    static_assert(LA >= 1 && LA <= 15, "lgkmcnt is 4 bits");
    static_assert((NB == 8 || NB == 16) && LA < NB, "fragment registers");
    sfor<0, (NR < LA ? NR : LA)>([&](auto I) __attribute__((always_inline)) { rd(I, b[decltype(I)::value & (NB - 1)]); });
    sfor<0, NR>([&](auto I) __attribute__((always_inline)) {
        constexpr int n = decltype(I)::value, rem = NR - 1 - n;
        ap_wait_lgkm<(rem < LA - 1 ? rem : LA - 1)>();
        use(I, b[n & (NB - 1)]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (n + LA < NR) rd(std::integral_constant<int, n + LA>{}, b[(n + LA) & (NB - 1)]);
    });
}
