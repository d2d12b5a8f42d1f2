// mesh_common.h — what the mesh files (mesh.hip, mesh_clean.hip, mesh_simplify.hip, mesh_smooth.hip, mesh_raster.hip) share: the segment
// pattern, a triangle's corners, and the host checks of a workspace (gfx950).
//
// The segment pattern.  A list whose output size depends on the data is compacted in three steps, none of which places anything by an atomic
// or makes a workgroup wait on another: one wave per SEGMENT of MESH_SEG consecutive elements writes every element's rank inside the segment
// (for a kept / dropped list: [keep << 31 | rank], segment_flag_rank) and the segment's total; ONE workgroup scans the totals in place
// (workgroup_exclusive_scan) and has the grand total; the emit finds an element's place as base[i >> MESH_SEG_LOG2] + rank (segment_index).
#pragma once

#include "sn_common.h"
#include "sn_wave.h"

namespace sn {

constexpr uint32_t MESH_SEG = 1024u;       // elements per wave = the unit of the scan
constexpr uint32_t MESH_SEG_LOG2 = 10u;
constexpr uint32_t MESH_WAVES = 4u;        // waves (segments) per workgroup of 256
constexpr uint32_t MESH_KEEP = 0x80000000u;
static_assert(MESH_SEG == 1u << MESH_SEG_LOG2, "MESH_SEG_LOG2 is the logarithm of MESH_SEG");

static inline size_t align16(size_t n) { return (n + 15u) & ~(size_t)15u; }

// N values of one element of the scan, loaded and stored as one.
template <class T, int N>
struct alignas(N * sizeof(T)) ScanItem { T c[N]; };

// Exclusive scan in place of n elements of N interleaved components each (element i's component k at totals[i N + k]; T = uint32_t or
// uint64_t) by ONE workgroup of 1024, every lane of which calls it.  Whole tiles of 1024, so that every lane reaches every shuffle and both
// barriers; the carry from tile to tile has 64 bits, a stored value is its low sizeof(T) bytes; total[k] = the grand total of component k.
// lds: 16 words per component.
template <int N, class T>
__device__ __forceinline__ void workgroup_exclusive_scan(T *__restrict__ totals, uint32_t n, T *lds, uint64_t (&total)[N]) {
    using Item = ScanItem<T, N>;
    Item *items = reinterpret_cast<Item *>(totals);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry[N];
#pragma unroll
    for (int k = 0; k < N; ++k) carry[k] = 0u;
    for (uint32_t s0 = 0; s0 < n; s0 += 1024u) {       // whole tiles
        const uint32_t i = s0 + tid;
        Item c;
#pragma unroll
        for (int k = 0; k < N; ++k) c.c[k] = 0u;
        if (i < n) c = items[i];
        T s[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            s[k] = wave_inclusive_sum(c.c[k]);
            if (lane == 63u) lds[k * 16 + wave] = s[k];
        }
        __syncthreads();
        Item out;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            T before = 0u, all = 0u;
#pragma unroll
            for (uint32_t w = 0; w < 16u; ++w) {
                const T a = lds[k * 16 + w];
                if (w < wave) before += a;
                all += a;
            }
            out.c[k] = (T)(carry[k] + before + (s[k] - c.c[k]));
            carry[k] += all;
        }
        if (i < n) items[i] = out;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < N; ++k) total[k] = carry[k];
}

template <class T>
__device__ __forceinline__ uint64_t workgroup_exclusive_scan(T *__restrict__ totals, uint32_t n, T *lds) {
    uint64_t total[1];
    workgroup_exclusive_scan<1>(totals, n, lds, total);
    return total[0];
}

// A kernel of 256 lanes, one wave per segment of the n elements: rank[i] = keep(i) << 31 | the kept elements before i in its segment;
// totals[seg] = the segment's kept elements.  keep: bool(uint32_t i), called for i < n only.  The kernel has no barrier.
template <class Keep>
__device__ __forceinline__ void segment_flag_rank(uint32_t n, uint32_t nseg, uint32_t *__restrict__ rank, uint32_t *__restrict__ totals,
                                                  const Keep &keep_of) {
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform
    uint32_t base = 0u;
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t i = seg * MESH_SEG + it * 64u + lane;
        const bool keep = i < n && keep_of(i);
        const uint64_t m = __ballot(keep);
        if (i < n) rank[i] = (keep ? MESH_KEEP : 0u) | (base + lanes_below(m));
        base += (uint32_t)__popcll(m);
    }
    if (lane == 0u) totals[seg] = base;
}

// Where the emit puts element i: its segment's scanned total + its rank (word = rank[i], with or without the keep bit).
__device__ __forceinline__ uint32_t segment_index(const uint32_t *__restrict__ base, uint32_t word, uint32_t i) {
    return base[i >> MESH_SEG_LOG2] + (word & ~MESH_KEEP);
}

// c = the three indices of triangle t, as they are; true iff all lie in [0, V).  c is filled either way, so a caller that tests the
// corners one by one (the emit loops: -1 per bad corner) or has tested them already (k_raster_resolve) ignores the result.
__device__ __forceinline__ bool triangle_corners(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, uint32_t c[3]) {
    const int32_t *tri = triangles + (size_t)t * 3u;
    c[0] = (uint32_t)tri[0]; c[1] = (uint32_t)tri[1]; c[2] = (uint32_t)tri[2];
    return c[0] < V && c[1] < V && c[2] < V;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static inline bool mesh_sizes_ok(uint32_t V, uint32_t T) { return V < (1u << 31) && T < (1u << 31); }

#define MESH_SIZES_MSG "%s: V = %u, T = %u is not supported (both below 2^31)"

// The size and the alignment of a workspace that is not NULL.
static inline int workspace_check(const char *who, const void *workspace, size_t bytes, size_t need) {
    if (bytes < need) { set_error("%s: workspace too small (%zu bytes, need %zu)", who, bytes, need); return SN_ERR_WORKSPACE; }
    SN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);
    return SN_OK;
}

}  // namespace sn
