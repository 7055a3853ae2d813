// philox.hpp — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the one
// state-free generator of the library: drop-out's keep flags (dropout.hip) and the grey-value noise (grey.hip) are words of it.
// Each caller states its own counter and key layout; tests/philox_ref.py restates the function and is pinned to the published
// known answers.
#pragma once
#include "common.hpp"

namespace unet {

struct u32x4 { unsigned v[4]; };

// the four output words of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ u32x4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{{c0, c1, c2, c3}};
}

}  // namespace unet
