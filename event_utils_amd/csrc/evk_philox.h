// Counter-based random numbers for the augmentation kernels: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random
// numbers: as easy as 1, 2, 3", SC 2011; the Random123 constants).  A draw is a pure function of (key, counter), so every event
// draws its own numbers independently of the launch shape, and a call repeats exactly under the same seed.
// Convention of this library: key = the call's 64-bit seed (low word, high word), counter = (event index low word, event index
// high word, purpose id, 0); one purpose id per kind of draw (EVK_PHILOX_* in evk.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace evk {

struct Philox4 {
    uint32_t v[4];
};

__host__ __device__ __forceinline__ constexpr Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// Random123's known-answer vectors (kat_vectors, philox4x32_10), checked at compile time on the function the kernels call
constexpr bool philox_kat(Philox4 r, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return r.v[0] == a && r.v[1] == b && r.v[2] == c && r.v[3] == d;
}
static_assert(philox_kat(philox4x32_10(0, 0, 0, 0, 0, 0), 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u), "Philox KAT 1");
static_assert(philox_kat(philox4x32_10(~0u, ~0u, ~0u, ~0u, ~0u, ~0u), 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu),
              "Philox KAT 2");
static_assert(philox_kat(philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u),
                         0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u),
              "Philox KAT 3");

// the four words of (seed, purpose) at event index i
__host__ __device__ __forceinline__ Philox4 philox_at(uint64_t seed, uint32_t purpose, uint64_t i) {
    return philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), purpose, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__host__ __device__ __forceinline__ uint64_t words64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// uniform double in [0, 1) from 53 bits (numpy's random_standard_uniform: (r >> 11) * 2^-53)
__host__ __device__ __forceinline__ double unit53(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }

// uniform integer in [0, range) by a 64-bit multiply-shift: floor(r * range / 2^64).  No rejection: an outcome's probability
// differs from 1 / range by at most range / 2^64 relative, i.e. the bias is below 2^-32 for every range below 2^32
__device__ __forceinline__ uint64_t uniform_below(uint64_t r, uint64_t range) { return __umul64hi(r, range); }

}  // namespace evk
