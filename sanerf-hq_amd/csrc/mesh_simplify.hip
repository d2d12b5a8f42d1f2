// mesh_simplify.hip — uniform vertex clustering of an indexed triangle mesh on the device (sn_rm_mesh_simplify_count / _emit), for gfx950:
// one output vertex per occupied cell of a coarse lattice, triangles that collapse or repeat dropped.
//
// Definition: include/sanerf_hip.h states it in full; tests/mesh_simplify_ref.py restates it in numpy.  In short: a vertex has the cell
// floor((p - origin) / cell) (fp32, no clamping; outside the lattice or non-finite: no cell); a triangle is invalid (an index out of range
// or a corner without a cell), degenerate (two corners in one cell), a duplicate (a lower-indexed valid, non-degenerate triangle has the
// same set of three cells) or kept; a cell is used iff it is a corner of a kept triangle; output vertex j is the j-th used cell in key
// order, at the mean of ALL input vertices of the cell (integer sums of 16-bit offsets, one fp64 evaluation), with the normalised integer
// sum of their normals.
//
// The count entry, six launches behind two memsets; no workgroup waits on, spins on or retries against another:
//   k_simp_keys        one lane per vertex: vkey[v] = the cell key, or -1.
//   k_simp_insert      one lane per triangle: the valid, non-degenerate ones enter an insert-only open-addressing table of triangle indices
//                      (capacity a power of two >= 2T, linear probing from a hash of the sorted key triple).  At a slot the lane does
//                      atomicCAS(slot, EMPTY, t); if the slot was occupied it compares the occupant's key set with its own (the occupant's
//                      three vertex keys, read-only in this launch) and on equality does atomicMin(slot, t), else moves on.  tslot[t] = the
//                      slot where it stopped.
//                      Why that is race-free.  A slot is claimed once and never emptied, and every value stored in it later comes from a
//                      triangle that compared equal to its occupant: a claimed slot's key set never changes.  Two triangles of one set S walk
//                      the same probe sequence, and each stops at the first slot that is empty or holds S.  Let s be the first slot of that
//                      sequence that ever holds S: every slot before s is passed by S's triangles only while it holds another set (an empty
//                      one would have been claimed for S), so it holds that set for ever and nobody of S stops there; and s, once S's, is
//                      where every later arrival stops.  So all of S's triangles end at s, and what s holds after the launch is the minimum
//                      of their indices: atomicMin commutes, the CAS winner is just the first operand.  The probe loop is bounded by the
//                      capacity and cannot be exhausted (the load is at most 1/2).
//   k_simp_keep        one wave per 1024 triangles: kept = valid, non-degenerate and table[tslot[t]] == t; the corners of the kept ones set
//                      their cells' bits (atomicOr: idempotent); trank[t] = kept << 31 | rank inside the segment; the segment's total.
//   k_simp_rank_cells  one wave per 1024 words of the cell bitmap (32 cells a word): the number of used cells before each word inside its
//                      segment, and the segment's total.
//   k_simp_scan        one workgroup: exclusive scan of both lists of totals; counts = {V', T'} (and a copy in the workspace for the emit).
//   k_simp_accumulate  one lane per vertex with a used cell: n, sum q (3 x u64) and sum Q (3 x i64) of its OUTPUT row, by 64-bit integer
//                      atomicAdd -- order-independent, so exact and deterministic -- after a segmented sum over the wave: consecutive lanes
//                      of one row (marching tetrahedra emits a cell's vertices close together) add once.  The row's key is stored beside
//                      the sums by a plain store (every writer stores the same value).
// The emit entry reads the workspace and `triangles`: one lane per output row evaluates position and normal; one lane per triangle and one
// per input vertex remap.  Nothing is placed by an atomic; every store is guarded by cap_v / cap_t / V and every index and key is
// range-tested before it addresses anything.  Plain vector loads, plain vector stores and integer atomics only.
#include "mesh_common.h"

#include <cmath>

namespace sn {

constexpr uint32_t SIMP_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t SIMP_ROW = 8u;          // u64 words per output row: key, n, sum q[3], sum Q[3]

struct SimpLattice { float origin[3], cell[3]; uint32_t dims[3]; };

// Parts in order, each rounded up to 16 bytes.  `head` holds {V', T'} for the emit; bits .. acc is one range that the count zeroes.
struct SimpLayout { size_t head, vkey, tslot, trank, ttot, table, cwrank, ctot, bits, acc, bytes; uint32_t nsegt, nwords, nsegc; uint64_t cap; };

static inline uint64_t simp_table_capacity(uint32_t T) {
    uint64_t cap = 1u;
    while (cap < 2u * (uint64_t)T) cap <<= 1;
    return cap;
}

static inline SimpLayout simp_layout(uint32_t V, uint32_t T, uint32_t cells) {
    SimpLayout l;
    l.nsegt = div_up(T, MESH_SEG);
    l.nwords = div_up(cells, 32u);
    l.nsegc = div_up(l.nwords, MESH_SEG);
    l.cap = simp_table_capacity(T);
    l.head = 0;
    l.vkey = l.head + 16u;
    l.tslot = l.vkey + align16((size_t)V * 4u);
    l.trank = l.tslot + align16((size_t)T * 4u);
    l.ttot = l.trank + align16((size_t)T * 4u);
    l.table = l.ttot + align16((size_t)l.nsegt * 4u);
    l.cwrank = l.table + align16((size_t)l.cap * 4u);
    l.ctot = l.cwrank + align16((size_t)l.nwords * 4u);
    l.bits = l.ctot + align16((size_t)l.nsegc * 4u);
    l.acc = l.bits + align16((size_t)l.nwords * 4u);
    l.bytes = l.acc + (size_t)V * (SIMP_ROW * 8u);
    return l;
}

// Cell of a position: per axis u = p - origin, s = u / cell (two fp32 roundings, IEEE division), i = floor(s); false when some i is outside
// [0, dims) -- which every NaN and infinity is.  q = rint((s - i) 65536) in [0, 65536]: the subtraction and the product are exact.
__device__ __forceinline__ bool simp_cell(const float *__restrict__ p, const SimpLattice &lat, uint32_t i[3], uint32_t q[3]) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = p[a] - lat.origin[a];
        const float s = u / lat.cell[a];
        const float f = floorf(s);
        const bool in = f >= 0.0f && f < 2147483648.0f;
        const uint32_t ia = in ? (uint32_t)(int32_t)f : 0u;
        ok = ok && in && ia < lat.dims[a];
        i[a] = ia;
        q[a] = in ? (uint32_t)(int32_t)rintf((s - f) * 65536.0f) : 0u;
    }
    return ok;
}

__device__ __forceinline__ uint32_t simp_key(const SimpLattice &lat, const uint32_t i[3]) {
    return (i[0] * lat.dims[1] + i[1]) * lat.dims[2] + i[2];         // below the product of dims, which is below 2^31
}

__global__ __launch_bounds__(256) void k_simp_keys(const float *__restrict__ vertices, uint32_t V, SimpLattice lat, int32_t *__restrict__ vkey) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    uint32_t i[3], q[3];
    vkey[v] = simp_cell(vertices + (size_t)v * 3u, lat, i, q) ? (int32_t)simp_key(lat, i) : -1;
}

// The three cell keys of triangle t, sorted; false for an invalid or a degenerate triangle.  Every index is range-tested before it addresses
// vkey, every key before it is believed.
__device__ __forceinline__ bool simp_triangle_keys(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, uint32_t cells,
                                                   const int32_t *__restrict__ vkey, uint32_t k[3], uint32_t sorted[3]) {
    uint32_t c[3];
    if (!triangle_corners(triangles, t, V, c)) return false;
    k[0] = (uint32_t)vkey[c[0]]; k[1] = (uint32_t)vkey[c[1]]; k[2] = (uint32_t)vkey[c[2]];
    const uint32_t lo = umin(k[0], umin(k[1], k[2])), hi = ~umin(~k[0], umin(~k[1], ~k[2]));
    if (hi >= cells) return false;                                              // -1 reads as 2^32 - 1; the largest key is tested, so the three loads fly together
    if (k[0] == k[1] || k[1] == k[2] || k[0] == k[2]) return false;
    sorted[0] = lo; sorted[2] = hi; sorted[1] = (k[0] ^ k[1] ^ k[2]) ^ lo ^ hi;
    return true;
}

__device__ __forceinline__ uint32_t simp_mix(uint32_t h) {          // the 32-bit finaliser of MurmurHash3 (public domain)
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

__global__ __launch_bounds__(256) void k_simp_insert(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, uint32_t cells,
                                                     const int32_t *__restrict__ vkey, uint32_t *table, uint32_t mask,
                                                     uint32_t *__restrict__ tslot) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    uint32_t k[3], mine[3];
    if (!simp_triangle_keys(triangles, t, V, cells, vkey, k, mine)) return;     // tslot[t] is not read for such a triangle
    uint32_t slot = simp_mix(simp_mix(simp_mix(mine[0] + 0x9E3779B9u) ^ mine[1]) ^ mine[2]) & mask;
    for (uint64_t probes = 0; probes <= (uint64_t)mask; ++probes, slot = (slot + 1u) & mask) {
        const uint32_t seen = atomicCAS(&table[slot], SIMP_EMPTY, t);
        if (seen == SIMP_EMPTY) break;                                          // claimed
        uint32_t ko[3], theirs[3];
        if (seen < T && simp_triangle_keys(triangles, seen, V, cells, vkey, ko, theirs) && theirs[0] == mine[0] && theirs[1] == mine[1] &&
            theirs[2] == mine[2]) {
            atomicMin(&table[slot], t);
            break;
        }
    }
    tslot[t] = slot;
}

// One wave per segment of 1024 triangles: kept iff it holds its set's slot; marks the cells of the kept ones; rank inside the segment.
__global__ __launch_bounds__(256) void k_simp_keep(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, uint32_t cells,
                                                   const int32_t *__restrict__ vkey, const uint32_t *__restrict__ table, uint32_t mask,
                                                   const uint32_t *__restrict__ tslot, uint32_t *bits, uint32_t *__restrict__ rank,
                                                   uint32_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    segment_flag_rank(T, nseg, rank, totals, [&](uint32_t t) {
        uint32_t k[3], sorted[3];
        bool keep = false;
        if (simp_triangle_keys(triangles, t, V, cells, vkey, k, sorted)) keep = table[tslot[t] & mask] == t;
        if (keep) {
#pragma unroll
            for (int c = 0; c < 3; ++c) atomicOr(&bits[k[c] >> 5], 1u << (k[c] & 31u));
        }
        return keep;
    });
}

// One wave per segment of 1024 bitmap words: wrank[w] = used cells before word w inside the segment; totals[seg].
__global__ __launch_bounds__(256) void k_simp_rank_cells(const uint32_t *__restrict__ bits, uint32_t nwords, uint32_t *__restrict__ wrank,
                                                         uint32_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform; the kernel has no barrier
    uint32_t base = 0u;
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t w = seg * MESH_SEG + it * 64u + lane;
        const uint32_t cnt = w < nwords ? (uint32_t)__popc(bits[w]) : 0u;      // 0 .. 32: six bits
        uint32_t prefix, total;
        wave_rank<6>(cnt, prefix, total);
        if (w < nwords) wrank[w] = base + prefix;
        base += total;
    }
    if (lane == 0u) totals[seg] = base;
}

__global__ __launch_bounds__(1024) void k_simp_scan(uint32_t *__restrict__ ctot, uint32_t nsegc, uint32_t *__restrict__ ttot, uint32_t nsegt,
                                                    uint32_t *__restrict__ head, uint32_t *__restrict__ counts) {
    SN_POISON_ALL();
    __shared__ uint32_t ws[16];
    const uint32_t nv = (uint32_t)workgroup_exclusive_scan(ctot, nsegc, ws);       // both below 2^31
    const uint32_t nt = (uint32_t)workgroup_exclusive_scan(ttot, nsegt, ws);
    if (threadIdx.x == 0u) { counts[0] = nv; counts[1] = nt; head[0] = nv; head[1] = nt; }
}

// The output index of a USED cell; key < cells.
__device__ __forceinline__ uint32_t simp_cell_rank(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ wrank,
                                                   const uint32_t *__restrict__ cbase, uint32_t key) {
    const uint32_t w = key >> 5;
    return cbase[w >> MESH_SEG_LOG2] + wrank[w] + (uint32_t)__popc(bits[w] & ((1u << (key & 31u)) - 1u));
}

__device__ __forceinline__ bool simp_cell_used(const uint32_t *__restrict__ bits, uint32_t key, uint32_t cells) {
    return key < cells && ((bits[key >> 5] >> (key & 31u)) & 1u) != 0u;
}

// Q of one normal component: rint(n 2^20) where that is finite and below 2^31 in magnitude, else 0 (so that no sum of < 2^31 of them overflows).
__device__ __forceinline__ int64_t simp_normal_q(float n) {
    const float p = n * 1048576.0f;
    return fabsf(p) < 2147483648.0f ? (int64_t)rintf(p) : 0;                   // NaN compares false
}

template <bool NORMALS>
__global__ __launch_bounds__(256) void k_simp_accumulate(const float *__restrict__ vertices, const float *__restrict__ normals, uint32_t V,
                                                         SimpLattice lat, uint32_t cells, const uint32_t *__restrict__ bits,
                                                         const uint32_t *__restrict__ wrank, const uint32_t *__restrict__ cbase,
                                                         unsigned long long *acc) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t row = SIMP_EMPTY, key = 0u, n = 0u, q[3] = {0u, 0u, 0u};
    int64_t Q[3] = {0, 0, 0};
    if (v < V) {
        uint32_t i[3];
        if (simp_cell(vertices + (size_t)v * 3u, lat, i, q)) {
            key = simp_key(lat, i);
            if (simp_cell_used(bits, key, cells)) {
                row = simp_cell_rank(bits, wrank, cbase, key);
                n = 1u;
                if (NORMALS) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) Q[a] = simp_normal_q(normals[(size_t)v * 3u + a]);
                }
            }
        }
        if (row == SIMP_EMPTY || row >= V) { row = SIMP_EMPTY; n = 0u; q[0] = q[1] = q[2] = 0u; }     // at most V rows exist
    }
    // Segmented inclusive sum over runs of consecutive lanes with one row (wave-uniform control flow; lanes without a row are runs of their own).
    const uint32_t prev = (uint32_t)__shfl_up((int)row, 1), next = (uint32_t)__shfl_down((int)row, 1);
    const bool head = lane == 0u || prev != row || row == SIMP_EMPTY;
    const bool tail = lane == 63u || next != row;
    const uint32_t run = lanes_below(__ballot(head)) + (head ? 1u : 0u);        // the same on every lane of a run, increasing along the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t urun = (uint32_t)__shfl_up((int)run, d);                 // every lane shuffles: never behind a short-circuit
        const bool take = lane >= (uint32_t)d && urun == run;
        const uint32_t un = (uint32_t)__shfl_up((int)n, d);
        const uint32_t u0 = (uint32_t)__shfl_up((int)q[0], d), u1 = (uint32_t)__shfl_up((int)q[1], d), u2 = (uint32_t)__shfl_up((int)q[2], d);
        if (take) { n += un; q[0] += u0; q[1] += u1; q[2] += u2; }             // at most 64 x 65536: 32 bits hold it
        if (NORMALS) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int64_t uq = shfl_up64(Q[a], d);
                if (take) Q[a] += uq;
            }
        }
    }
    if (row != SIMP_EMPTY && tail) {
        unsigned long long *r = acc + (size_t)row * SIMP_ROW;
        r[0] = (unsigned long long)key;                                        // every writer of the row stores the same key
        atomicAdd(&r[1], (unsigned long long)n);
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd(&r[2 + a], (unsigned long long)q[a]);
        if (NORMALS) {
#pragma unroll
            for (int a = 0; a < 3; ++a) atomicAdd(&r[5 + a], (unsigned long long)Q[a]);      // two's complement: the signed sum
        }
    }
}

// One lane per output row: the position and the normal, each quantity one fp64 evaluation rounded once to fp32.
__global__ __launch_bounds__(256) void k_simp_emit_vertices(const unsigned long long *__restrict__ acc, const uint32_t *__restrict__ head, uint32_t V,
                                                            SimpLattice lat, uint32_t cells, float *__restrict__ out_vertices,
                                                            float *__restrict__ out_normals, uint32_t cap_v) {
    SN_POISON_ALL();
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= cap_v || j >= V || j >= head[0]) return;
    const unsigned long long *r = acc + (size_t)j * SIMP_ROW;
    const uint32_t key = (uint32_t)r[0] < cells ? (uint32_t)r[0] : 0u;
    const uint32_t i[3] = {key / (lat.dims[1] * lat.dims[2]), (key / lat.dims[2]) % lat.dims[1], key % lat.dims[2]};
    const double n = (double)r[1];
    float *p = out_vertices + (size_t)j * 3u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mean = ((double)r[2 + a] / n) / 65536.0;
        p[a] = (float)((double)lat.origin[a] + (double)lat.cell[a] * ((double)i[a] + mean));
    }
    if (out_normals) {
        const double sx = (double)(long long)r[5], sy = (double)(long long)r[6], sz = (double)(long long)r[7];
        const double len = sqrt((sx * sx + sy * sy) + sz * sz);
        float *q = out_normals + (size_t)j * 3u;
        const bool zero = r[5] == 0ull && r[6] == 0ull && r[7] == 0ull;
        q[0] = zero ? 0.0f : (float)(sx / len);
        q[1] = zero ? 0.0f : (float)(sy / len);
        q[2] = zero ? 0.0f : (float)(sz / len);
    }
}

__global__ __launch_bounds__(256) void k_simp_emit_triangles(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, uint32_t cells,
                                                             const int32_t *__restrict__ vkey, const uint32_t *__restrict__ bits,
                                                             const uint32_t *__restrict__ wrank, const uint32_t *__restrict__ cbase,
                                                             const uint32_t *__restrict__ trank, const uint32_t *__restrict__ tbase,
                                                             int32_t *__restrict__ out_triangles, uint32_t cap_t) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    const uint32_t w = trank[t];
    if (!(w & MESH_KEEP)) return;
    const uint32_t id = segment_index(tbase, w, t);
    if (id >= cap_t) return;
    uint32_t x[3];
    triangle_corners(triangles, t, V, x);
    int32_t *out = out_triangles + (size_t)id * 3u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                      // range-tested again, corner by corner: `triangles` may have changed since the count
        const uint32_t key = x[c] < V ? (uint32_t)vkey[x[c]] : SIMP_EMPTY;
        out[c] = simp_cell_used(bits, key, cells) ? (int32_t)simp_cell_rank(bits, wrank, cbase, key) : -1;
    }
}

__global__ __launch_bounds__(256) void k_simp_emit_cluster(uint32_t V, uint32_t cells, const int32_t *__restrict__ vkey,
                                                           const uint32_t *__restrict__ bits, const uint32_t *__restrict__ wrank,
                                                           const uint32_t *__restrict__ cbase, int32_t *__restrict__ vertex_cluster) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    const uint32_t key = (uint32_t)vkey[v];
    vertex_cluster[v] = simp_cell_used(bits, key, cells) ? (int32_t)simp_cell_rank(bits, wrank, cbase, key) : -1;
}

}  // namespace sn

using namespace sn;

extern "C" size_t sn_rm_mesh_simplify_workspace_bytes(uint32_t V, uint32_t T, uint32_t cells) {
    if (!(mesh_sizes_ok(V, T) && cells < (1u << 31))) {
        set_error("mesh_simplify: V = %u, T = %u, cells = %u is not supported (all below 2^31)", V, T, cells);
        return 0;
    }
    return simp_layout(V, T, cells).bytes;
}

// The checks the two entries share; fills the lattice, the cell count and the layout.
static int simp_check(const char *who, uint32_t V, uint32_t T, const float *origin, const float *cell, const uint32_t *dims, const void *workspace,
                      size_t bytes, SimpLattice *lat, uint32_t *cells, SimpLayout *l) {
    SN_REQUIRE(origin && cell && dims && workspace, "%s: NULL pointer", who);
    uint64_t n = 1u;
    for (int a = 0; a < 3; ++a) {
        SN_REQUIRE(std::isfinite(origin[a]), "%s: origin[%d] = %g is not finite", who, a, (double)origin[a]);
        SN_REQUIRE(std::isfinite(cell[a]) && cell[a] > 0.0f, "%s: cell[%d] = %g must be positive and finite", who, a, (double)cell[a]);
        SN_REQUIRE(dims[a] >= 1u, "%s: dims[%d] must be at least 1", who, a);
        SN_UNSUPPORTED(dims[a] < (1u << 31), "%s: dims[%d] = %u is not supported (the product below 2^31)", who, a, dims[a]);
        n *= dims[a];
        SN_UNSUPPORTED(n < (1ull << 31), "%s: %u x %u x %u cells is not supported (the product below 2^31)", who, dims[0], dims[1], dims[2]);
        lat->origin[a] = origin[a]; lat->cell[a] = cell[a]; lat->dims[a] = dims[a];
    }
    SN_UNSUPPORTED(mesh_sizes_ok(V, T), MESH_SIZES_MSG, who, V, T);
    *cells = (uint32_t)n;                  // below 2^31: the loop tested it
    *l = simp_layout(V, T, *cells);
    return workspace_check(who, workspace, bytes, l->bytes);
}

extern "C" int sn_rm_mesh_simplify_count(const float *vertices, const float *normals, const int32_t *triangles, uint32_t V, uint32_t T,
                                         const float *origin, const float *cell, const uint32_t *dims, void *workspace, size_t workspace_bytes,
                                         uint32_t *counts, sn_stream_t stream) {
    if (V == 0) return SN_OK;              // the empty mesh: nothing is stored, counts included
    SN_REQUIRE(vertices && counts && (triangles || T == 0), "mesh_simplify_count: NULL pointer");
    SimpLattice lat;
    SimpLayout l;
    uint32_t cells = 0;
    const int rc = simp_check("mesh_simplify_count", V, T, origin, cell, dims, workspace, workspace_bytes, &lat, &cells, &l);
    if (rc != SN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *head = (uint32_t *)(ws + l.head), *tslot = (uint32_t *)(ws + l.tslot), *trank = (uint32_t *)(ws + l.trank);
    uint32_t *ttot = (uint32_t *)(ws + l.ttot), *table = (uint32_t *)(ws + l.table), *cwrank = (uint32_t *)(ws + l.cwrank);
    uint32_t *ctot = (uint32_t *)(ws + l.ctot), *bits = (uint32_t *)(ws + l.bits);
    int32_t *vkey = (int32_t *)(ws + l.vkey);
    unsigned long long *acc = (unsigned long long *)(ws + l.acc);
    const uint32_t mask = (uint32_t)(l.cap - 1u);
    SN_HIP_OK(hipMemsetAsync(bits, 0, l.bytes - l.bits, st));                  // the bitmap and the rows
    if (T) SN_HIP_OK(hipMemsetAsync(table, 0xFF, (size_t)l.cap * 4u, st));     // SIMP_EMPTY
    hipLaunchKernelGGL(k_simp_keys, dim3(div_up(V, 256)), dim3(256), 0, st, vertices, V, lat, vkey);
    if (T) {
        hipLaunchKernelGGL(k_simp_insert, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, cells, vkey, table, mask, tslot);
        hipLaunchKernelGGL(k_simp_keep, dim3(div_up(l.nsegt, MESH_WAVES)), dim3(256), 0, st, triangles, T, V, cells, vkey, table, mask, tslot, bits,
                           trank, ttot, l.nsegt);
    }
    hipLaunchKernelGGL(k_simp_rank_cells, dim3(div_up(l.nsegc, MESH_WAVES)), dim3(256), 0, st, bits, l.nwords, cwrank, ctot, l.nsegc);
    hipLaunchKernelGGL(k_simp_scan, dim3(1), dim3(1024), 0, st, ctot, l.nsegc, ttot, l.nsegt, head, counts);
    if (T) {                               // without a triangle no cell is used and no row exists
        if (normals) hipLaunchKernelGGL(k_simp_accumulate<true>, dim3(div_up(V, 256)), dim3(256), 0, st, vertices, normals, V, lat, cells, bits, cwrank, ctot, acc);
        else hipLaunchKernelGGL(k_simp_accumulate<false>, dim3(div_up(V, 256)), dim3(256), 0, st, vertices, normals, V, lat, cells, bits, cwrank, ctot, acc);
    }
    SN_LAUNCH_CHECK("k_simp_keys .. k_simp_accumulate");
    return SN_OK;
}

extern "C" int sn_rm_mesh_simplify_emit(const float *vertices, const float *normals, const int32_t *triangles, uint32_t V, uint32_t T,
                                        const float *origin, const float *cell, const uint32_t *dims, const void *workspace,
                                        size_t workspace_bytes, float *out_vertices, float *out_normals, int32_t *out_triangles,
                                        int32_t *vertex_cluster, uint32_t cap_v, uint32_t cap_t, sn_stream_t stream) {
    (void)vertices;                        // the positions come from the sums of the count
    if (V == 0 || (cap_v == 0 && cap_t == 0 && !vertex_cluster)) return SN_OK;  // nothing can be stored
    SN_REQUIRE(triangles || T == 0 || cap_t == 0, "mesh_simplify_emit: NULL pointer");
    SN_REQUIRE((out_vertices || cap_v == 0) && (out_triangles || cap_t == 0 || T == 0) && (out_normals || !normals || cap_v == 0),
               "mesh_simplify_emit: NULL output with a non-zero capacity");
    SN_REQUIRE(cap_v <= 0x7fffffffu, "mesh_simplify_emit: cap_v beyond the int32 vertex ids of the triangles");
    SimpLattice lat;
    SimpLayout l;
    uint32_t cells = 0;
    const int rc = simp_check("mesh_simplify_emit", V, T, origin, cell, dims, workspace, workspace_bytes, &lat, &cells, &l);
    if (rc != SN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *ws = (const uint8_t *)workspace;
    const uint32_t *head = (const uint32_t *)(ws + l.head), *trank = (const uint32_t *)(ws + l.trank), *ttot = (const uint32_t *)(ws + l.ttot);
    const uint32_t *cwrank = (const uint32_t *)(ws + l.cwrank), *ctot = (const uint32_t *)(ws + l.ctot), *bits = (const uint32_t *)(ws + l.bits);
    const int32_t *vkey = (const int32_t *)(ws + l.vkey);
    const unsigned long long *acc = (const unsigned long long *)(ws + l.acc);
    const uint32_t rows = cap_v < V ? cap_v : V;
    if (rows) hipLaunchKernelGGL(k_simp_emit_vertices, dim3(div_up(rows, 256)), dim3(256), 0, st, acc, head, V, lat, cells, out_vertices,
                                 normals ? out_normals : (float *)nullptr, cap_v);
    if (cap_t && T) hipLaunchKernelGGL(k_simp_emit_triangles, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, cells, vkey, bits, cwrank, ctot,
                                       trank, ttot, out_triangles, cap_t);
    if (vertex_cluster) hipLaunchKernelGGL(k_simp_emit_cluster, dim3(div_up(V, 256)), dim3(256), 0, st, V, cells, vkey, bits, cwrank, ctot, vertex_cluster);
    SN_LAUNCH_CHECK("k_simp_emit");
    return SN_OK;
}
