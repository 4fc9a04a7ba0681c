// The data path's random draws, once, for synth_batch.hip, augment.hip and roll.hip (libairpose_grad.so).  Included inside each file's unnamed
// namespace.
//
// Philox4x32-10 of Random123: ten rounds, the key bumped by the Weyl constants between them.  Key = (seed's low word, seed's high
// word).  The counter layout of include/airpose_grad.h, the one thing that keeps the streams of one seed apart:
//   (c0, c1, c2, c3) = (index[i], epoch, camera, block)
//     block 0, camera 0 / 1      apg_synth_batch's jitter: words 0 .. 3 the ymin, ymax, xmin, xmax side offsets
//     block 0, camera 2          apg_synth_batch's flip: bit 31 of word 0
//     block 1 .. 14, camera 0 / 1   apg_augment_draw's parameter set (block k, word w as the header lists them)
//     block 15, camera 0 / 1        apg_roll_draw's gate (word 0) and angle (word 1)
//     block 0x80000000 | pixel   apg_augment_crops' noise of pixel row * 224 + column
// A new stream takes a block (or a camera value) none of these uses.
struct U4 { uint32_t w[4]; };
__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{{c0, c1, c2, c3}};
}

// the 24-bit uniform in [0, 1): (word >> 8) * 2^-24, exact in fp32
__device__ __forceinline__ float uni(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
