// wave_sort.hpp -- the one-wavefront sorting network on total-order keys, shared by the selections of stats.hip, the residual
// quantiles of conformal.hip and the quartiles of quality.hip.  An fp64 value becomes a 64-bit key whose unsigned order is the order of the values (negatives: all
// bits flipped, others: sign bit flipped; -0.0 sorts below +0.0, a NaN beyond the infinity of its sign); the buffer -- LDS or a
// slice of a global workspace -- is sorted in place by a bitonic network, every stage closed by st_sync.  The largest key ~0 pads
// the buffer to a power of two.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_math.hpp"

namespace anofox {

namespace {

constexpr uint64_t ST_SIGN = 0x8000000000000000ull;

// what one lane wrote to the buffer becomes visible to the other lanes of its wave
__device__ __forceinline__ void st_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint64_t st_key(uint64_t bits) { return (bits >> 63) ? ~bits : (bits | ST_SIGN); }
__device__ __forceinline__ double st_unkey(uint64_t k) { return dm_from_bits((k >> 63) ? (k ^ ST_SIGN) : ~k); }

// ascending bitonic network over buf[0 .. p2), p2 a power of two, one wave
template <class B>
__device__ __forceinline__ void st_sort(B buf, int p2, int lane)
{
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = lane; p < (p2 >> 1); p += 64) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int hi = lo | j;
                const bool up = (lo & k) == 0;
                const uint64_t x = buf[lo], y = buf[hi];
                if ((x > y) == up) { buf[lo] = y; buf[hi] = x; }
            }
            st_sync();
        }
    }
}

} // namespace

} // namespace anofox
