// sn_wave.h — wave-wide ranking by ballot + mbcnt, shared by mesh.hip and mesh_clean.hip (gfx950, 64 lanes).
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

}  // namespace sn
