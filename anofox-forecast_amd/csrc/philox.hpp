// philox.hpp -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011), the counter-based generator of the sample-path kernels (paths.hip,
// ets_paths.hip): four 32-bit output words per (counter, key), no state and no draw order.  tests/paths_ref.py philox4x32_10 is the
// same statement in Python integers and is held to the published known answers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anofox {

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10: ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

} // namespace

} // namespace anofox
