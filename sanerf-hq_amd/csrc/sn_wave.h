// sn_wave.h — wave-wide primitives of the mesh files (gfx950, 64 lanes): ranking by ballot + mbcnt, 64-bit shuffles, the inclusive sum.
#pragma once

#include "sn_common.h"

namespace sn {

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Exclusive prefix and total of a small per-lane count over the wave: one ballot per bit of the count.  Every lane of the wave calls it.
template <int BITS>
__device__ __forceinline__ void wave_rank(uint32_t cnt, uint32_t &prefix, uint32_t &total) {
    prefix = 0u; total = 0u;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const uint64_t m = __ballot((cnt >> b) & 1u);
        prefix += lanes_below(m) << b;
        total += (uint32_t)__popcll(m) << b;
    }
}

// The shuffles of a 64-bit value, T = uint64_t or int64_t, as two 32-bit halves.
template <class T>
__device__ __forceinline__ T shfl64(T x, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)(uint64_t)x, src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)x >> 32), src);
    return (T)(((uint64_t)hi << 32) | lo);
}

template <class T>
__device__ __forceinline__ T shfl_up64(T x, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)(uint64_t)x, d), hi = (uint32_t)__shfl_up((int)(uint32_t)((uint64_t)x >> 32), d);
    return (T)(((uint64_t)hi << 32) | lo);
}

template <class T>
__device__ __forceinline__ T shfl_xor64(T x, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)x, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)x >> 32), m);
    return (T)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint32_t shfl_up(uint32_t x, int d) { return (uint32_t)__shfl_up((int)x, d); }
__device__ __forceinline__ uint64_t shfl_up(uint64_t x, int d) { return shfl_up64(x, d); }

// Inclusive sum over the wave (uint32_t or uint64_t), by doubling.  Every lane of the wave calls it: all lanes shuffle, the add is guarded.
template <class T>
__device__ __forceinline__ T wave_inclusive_sum(T s) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = shfl_up(s, d);
        if (lane >= (uint32_t)d) s += u;
    }
    return s;
}

}  // namespace sn
