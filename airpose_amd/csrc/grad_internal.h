// Internal helpers shared by the sources of libairpose_grad.so (head_grad.hip, geom_grad.hip, trunk_grad.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/airpose_grad.h"

// records the thread-local message apg_last_error() returns; returns code
__attribute__((visibility("hidden"))) int apg_fail(int code, const std::string& msg);

// splitmix64 finaliser
__host__ __device__ __forceinline__ uint64_t apg_mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// dropout keep decision of (seed, layer, row, col): u = top 24 bits of the hash / 2^24 (exact in fp32), keep iff u >= p.
// Counter = layer << 56 | row << 24 | col (col < 2^24, row < 2^32).
__host__ __device__ __forceinline__ bool apg_keep(uint64_t seed, int layer, int row, int col, float p) {
    if (p <= 0.f) return true;
    const uint64_t ctr = ((uint64_t)(uint32_t)layer << 56) ^ ((uint64_t)(uint32_t)row << 24) ^ (uint64_t)(uint32_t)col;
    const uint64_t h = apg_mix64(apg_mix64(ctr) ^ seed);
    const float u = (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f);
    return u >= p;
}
