// mesh_split.hip — an indexed triangle mesh with a label on every vertex, taken apart into one mesh per label on the device
// (sn_rm_mesh_split_count / _emit), for gfx950.
//
// Definition: include/sanerf_hip.h states it in full; tests/mesh_split_ref.py restates it in numpy.  In short: part(label) = min(label, 32);
// a triangle is valid iff its three indices are in [0, V) and goes to the part that two of its corners have, or to the lowest of three
// different ones; a vertex belongs to every part that has a valid triangle with it as a corner (a seam vertex is duplicated); the output is
// packed in part order, triangles in their input order, vertices in increasing input index, indices local to the part.
//
// A stable partition into P = 33 buckets with the segment pattern of mesh_common.h.  Per vertex one 64-bit MEMBERSHIP word, bit p = "in
// part p"; a triangle counts as a word with one bit.  One wave walks a segment of MESH_SEG elements 64 at a time and, for every part that
// is present in the 64 words, takes the ballot of the part's bit; lane p of the wave keeps the running count of part p (wave_parts).
// The segment's P totals go into a table PART-MAJOR, totals[p nseg + seg], so that ONE exclusive scan over the P nseg words (one workgroup,
// workgroup_exclusive_scan) gives base[p][seg] with the parts contiguous and in order, and base[p][0] is the part's offset.
//   k_split_rank_triangles   the vote, atomicOr of the part's bit into the three corners' words (integer, order-independent: the only atomic
//                            of the file, and it places nothing), trank[t] = part << 16 | rank in the segment (SPLIT_NONE: invalid), totals
//   k_split_rank_vertices    over the finished words: group_count[group][p] (uint16) = the members of part p before the group of 64 inside
//                            its segment, totals
//   k_split_scan             one workgroup: both tables, the two offset arrays, counts
//   k_split_emit_vertices    lane = input vertex; for each bit p of its word, row = vbase[p][seg] + group_count[group][p] + the lanes
//                            below it in the ballot of p.  It also leaves first_row[v] = the row in the vertex's LOWEST part.
//   k_split_emit_triangles   lane = input triangle; row = tbase[part][seg] + rank; a corner's row in that part is first_row[c] when the part
//                            is the corner's lowest -- every vertex with one bit, nearly all -- and is otherwise recomputed from the words of
//                            the <= 63 vertices before it in its group.
// No workgroup waits on another: every hand-off is a launch boundary.  Every store of the emit is guarded by cap_v / cap_t, and every
// index, part included, is range-tested before it addresses anything: a workspace that does not belong to `triangles` misplaces rows (an
// index that cannot be resolved is emitted as -1) and never writes out of bounds.  Plain vector loads and stores and one integer atomic.
#include "mesh_common.h"

namespace sn {

constexpr uint32_t SPLIT_P = SN_MESH_SPLIT_PARTS;
constexpr uint64_t SPLIT_BITS = (1ull << SPLIT_P) - 1u;
constexpr uint32_t SPLIT_NONE = 0xFFFFFFFFu;
static_assert(SPLIT_P <= 64u && MESH_SEG <= (1u << 16), "one lane and one membership bit per part; a rank inside a segment has 16 bits");

struct SplitLayout { size_t ttot, vtot, member, first_row, group_count, trank, bytes; uint32_t nsegv, nsegt, ngroups; };

static inline SplitLayout split_layout(uint32_t V, uint32_t T) {
    SplitLayout l;
    l.nsegv = div_up(V, MESH_SEG);
    l.nsegt = div_up(T, MESH_SEG);
    l.ngroups = div_up(V, 64u);
    l.ttot = 0;
    l.vtot = l.ttot + align16((size_t)SPLIT_P * l.nsegt * 4u);
    l.member = l.vtot + align16((size_t)SPLIT_P * l.nsegv * 4u);
    l.first_row = l.member + align16((size_t)V * 8u);
    l.group_count = l.first_row + align16((size_t)V * 4u);
    l.trank = l.group_count + align16((size_t)SPLIT_P * l.ngroups * 2u);
    l.bytes = l.trank + align16((size_t)T * 4u);
    return l;
}

__device__ __forceinline__ uint32_t part_of(uint8_t label) { return umin((uint32_t)label, SPLIT_P - 1u); }

// The part of a triangle from its corners' parts: the one that two corners share, else the lowest.  Symmetric in the three.
__device__ __forceinline__ uint32_t vote(uint32_t a, uint32_t b, uint32_t c) {
    if (a == b || a == c) return a;
    if (b == c) return b;
    return umin(a, umin(b, c));
}

// The 64 membership words w of the wave, part by part.  For every part p with a bit in some lane, once and in no particular order:
// visit(p, m, before) with m = the ballot of bit p and before = the running count of p; then lane p's `running` grows by popcount(m).
// Every lane of the wave calls it; p, m and before are wave-uniform.  At most 64 turns, whatever the words hold.
template <class Visit>
__device__ __forceinline__ void wave_parts(uint64_t w, uint32_t &running, const Visit &visit) {
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        const uint64_t todo = __ballot(w != 0u);
        if (!todo) break;                              // wave-uniform
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const uint32_t p = (uint32_t)__shfl(w ? __ffsll((unsigned long long)w) - 1 : 0, lead);
        const uint64_t m = __ballot((w >> p) & 1u);
        const uint32_t before = (uint32_t)__shfl((int)running, (int)p);
        visit(p, m, before);
        if (lane == p) running += (uint32_t)__popcll(m);
        w &= ~(1ull << p);
    }
}

// One wave per segment of 1024 triangles: the vote, the corners' membership bits, the rank inside the segment, the segment's P totals.
__global__ __launch_bounds__(256) void k_split_rank_triangles(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                              const uint8_t *__restrict__ labels, unsigned long long *member,
                                                              uint32_t *__restrict__ trank, uint32_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform
    uint32_t running = 0u;
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t t = seg * MESH_SEG + it * 64u + lane;
        uint32_t c[3], part = 0u;
        const bool valid = t < T && triangle_corners(triangles, t, V, c);
        if (valid) {
            part = vote(part_of(labels[c[0]]), part_of(labels[c[1]]), part_of(labels[c[2]]));
#pragma unroll
            for (int q = 0; q < 3; ++q) atomicOr(&member[c[q]], 1ull << part);
        }
        uint32_t word = SPLIT_NONE;
        wave_parts(valid ? 1ull << part : 0ull, running, [&](uint32_t p, uint64_t m, uint32_t before) {
            if (valid && part == p) word = (p << 16) | (before + lanes_below(m));
        });
        if (t < T) trank[t] = word;
    }
    if (lane < SPLIT_P) totals[lane * nseg + seg] = running;
}

// One wave per segment of 1024 vertices over the finished membership words: the count of every part before each group of 64, the totals.
__global__ __launch_bounds__(256) void k_split_rank_vertices(uint32_t V, const unsigned long long *__restrict__ member,
                                                             uint16_t *__restrict__ group_count, uint32_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform
    uint32_t running = 0u;
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t v0 = seg * MESH_SEG + it * 64u;
        if (v0 >= V) break;                // wave-uniform
        if (lane < SPLIT_P) group_count[(size_t)(v0 >> 6) * SPLIT_P + lane] = (uint16_t)running;      // at most 1024 - 64
        const uint32_t v = v0 + lane;
        wave_parts(v < V ? member[v] & SPLIT_BITS : 0ull, running, [](uint32_t, uint64_t, uint32_t) {});
    }
    if (lane < SPLIT_P) totals[lane * nseg + seg] = running;
}

__global__ __launch_bounds__(1024) void k_split_scan(uint32_t *__restrict__ ttot, uint32_t nsegt, uint32_t *__restrict__ vtot, uint32_t nsegv,
                                                     uint32_t *__restrict__ part_triangle_offsets, uint32_t *__restrict__ part_vertex_offsets,
                                                     uint32_t *__restrict__ counts) {
    SN_POISON_ALL();
    __shared__ uint32_t ws[16];
    const uint32_t nt = (uint32_t)workgroup_exclusive_scan(ttot, SPLIT_P * nsegt, ws);
    const uint32_t nv = (uint32_t)workgroup_exclusive_scan(vtot, SPLIT_P * nsegv, ws);
    // (the scan ends in a barrier: the tables below are this workgroup's own finished stores)
    const uint32_t p = threadIdx.x;
    if (p <= SPLIT_P) {
        part_triangle_offsets[p] = p < SPLIT_P ? ttot[p * nsegt] : nt;
        part_vertex_offsets[p] = p < SPLIT_P ? vtot[p * nsegv] : nv;
    }
    if (p == 0u) { counts[0] = nv; counts[1] = nt; }
}

// Whole waves, one per group of 64 vertices: every lane reaches every ballot, the stores are guarded.
__global__ __launch_bounds__(256) void k_split_emit_vertices(uint32_t V, const uint32_t *__restrict__ vertices, const uint32_t *__restrict__ normals,
                                                             const unsigned long long *__restrict__ member, const uint16_t *__restrict__ group_count,
                                                             const uint32_t *__restrict__ vbase, uint32_t nseg, uint32_t *__restrict__ first_row,
                                                             uint32_t *__restrict__ out_vertices, uint32_t *__restrict__ out_normals,
                                                             int32_t *__restrict__ source_vertex, uint32_t cap_v) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, group = v >> 6;
    if ((v & ~63u) >= V) return;           // wave-uniform
    const bool live = v < V;
    const uint64_t w = live ? member[v] & SPLIT_BITS : 0ull;
    const uint32_t lowest = w ? (uint32_t)__ffsll((unsigned long long)w) - 1u : SPLIT_P;
    uint32_t x[3] = {0u, 0u, 0u}, n[3] = {0u, 0u, 0u};
    if (w && cap_v) {                      // (cap_v = 0: only first_row is wanted, and `vertices` may be NULL)
        const uint32_t *p = vertices + (size_t)v * 3u;
        x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
        if (normals) {
            const uint32_t *pn = normals + (size_t)v * 3u;
            n[0] = pn[0]; n[1] = pn[1]; n[2] = pn[2];
        }
    }
    uint32_t unused = 0u;
    wave_parts(w, unused, [&](uint32_t p, uint64_t m, uint32_t) {
        const uint32_t row = vbase[p * nseg + (v >> MESH_SEG_LOG2)] + group_count[(size_t)group * SPLIT_P + p] + lanes_below(m);
        if (!((w >> p) & 1u)) return;
        if (p == lowest) first_row[v] = row;
        if (row >= cap_v) return;
        uint32_t *q = out_vertices + (size_t)row * 3u;
        q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
        if (normals) {
            uint32_t *qn = out_normals + (size_t)row * 3u;
            qn[0] = n[0]; qn[1] = n[1]; qn[2] = n[2];
        }
        if (source_vertex) source_vertex[row] = (int32_t)v;
    });
}

__global__ __launch_bounds__(256) void k_split_emit_triangles(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                              const unsigned long long *__restrict__ member, const uint16_t *__restrict__ group_count,
                                                              const uint32_t *__restrict__ vbase, uint32_t nsegv, const uint32_t *__restrict__ first_row,
                                                              const uint32_t *__restrict__ trank, const uint32_t *__restrict__ tbase, uint32_t nsegt,
                                                              int32_t *__restrict__ out_triangles, int32_t *__restrict__ source_triangle, uint32_t cap_t) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    const uint32_t word = trank[t], part = word >> 16;
    if (word == SPLIT_NONE || part >= SPLIT_P) return;
    const uint32_t id = tbase[part * nsegt + (t >> MESH_SEG_LOG2)] + (word & 0xFFFFu);
    if (id >= cap_t) return;
    const uint32_t first = vbase[part * nsegv];        // = part_vertex_offsets[part]
    uint32_t c[3];
    triangle_corners(triangles, t, V, c);
    int32_t *out = out_triangles + (size_t)id * 3u;
#pragma unroll
    for (int q = 0; q < 3; ++q) {          // range-tested again, corner by corner: `triangles` may have changed since the count
        int32_t local = -1;
        const uint64_t w = c[q] < V ? member[c[q]] & SPLIT_BITS : 0ull;
        if ((w >> part) & 1u) {
            uint32_t row;
            if ((w & ((1ull << part) - 1u)) == 0u) row = first_row[c[q]];      // the corner's lowest part
            else {                                     // a seam vertex in one of its higher parts: the emit's row, once more
                const uint32_t g0 = c[q] & ~63u;
                row = vbase[part * nsegv + (c[q] >> MESH_SEG_LOG2)] + group_count[(size_t)(c[q] >> 6) * SPLIT_P + part];
                for (uint32_t u = g0; u < c[q]; ++u) row += (uint32_t)((member[u] >> part) & 1u);
            }
            local = (int32_t)(row - first);
        }
        out[q] = local;
    }
    if (source_triangle) source_triangle[id] = (int32_t)t;
}

}  // namespace sn

using namespace sn;

#define SPLIT_SIZES(who) SN_UNSUPPORTED(mesh_sizes_ok(V, T), MESH_SIZES_MSG, who, V, T)

extern "C" size_t sn_rm_mesh_split_workspace_bytes(uint32_t V, uint32_t T) {
    if (!mesh_sizes_ok(V, T)) {
        set_error(MESH_SIZES_MSG, "mesh_split", V, T);
        return 0;
    }
    return split_layout(V, T).bytes;
}

static int split_check(const char *who, uint32_t V, uint32_t T, const void *workspace, size_t bytes, SplitLayout *l) {
    SN_REQUIRE(workspace, "%s: NULL pointer", who);
    SPLIT_SIZES(who);
    *l = split_layout(V, T);
    return workspace_check(who, workspace, bytes, l->bytes);
}

extern "C" int sn_rm_mesh_split_count(const int32_t *triangles, uint32_t T, uint32_t V, const uint8_t *vertex_labels, void *workspace,
                                      size_t workspace_bytes, int32_t *part_triangle_offsets, int32_t *part_vertex_offsets, uint32_t *counts,
                                      sn_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (V == 0 || T == 0) {                // no triangle, no member: every part is empty
        if (part_triangle_offsets) SN_HIP_OK(hipMemsetAsync(part_triangle_offsets, 0, (SPLIT_P + 1u) * sizeof(int32_t), st));
        if (part_vertex_offsets) SN_HIP_OK(hipMemsetAsync(part_vertex_offsets, 0, (SPLIT_P + 1u) * sizeof(int32_t), st));
        if (counts) SN_HIP_OK(hipMemsetAsync(counts, 0, 2u * sizeof(uint32_t), st));
        return SN_OK;
    }
    SN_REQUIRE(triangles && vertex_labels && part_triangle_offsets && part_vertex_offsets && counts, "mesh_split_count: NULL pointer");
    SplitLayout l;
    const int rc = split_check("mesh_split_count", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *ttot = (uint32_t *)(ws + l.ttot), *vtot = (uint32_t *)(ws + l.vtot), *trank = (uint32_t *)(ws + l.trank);
    unsigned long long *member = (unsigned long long *)(ws + l.member);
    SN_HIP_OK(hipMemsetAsync(member, 0, (size_t)V * 8u, st));
    hipLaunchKernelGGL(k_split_rank_triangles, dim3(div_up(l.nsegt, MESH_WAVES)), dim3(256), 0, st, triangles, T, V, vertex_labels, member, trank,
                       ttot, l.nsegt);
    hipLaunchKernelGGL(k_split_rank_vertices, dim3(div_up(l.nsegv, MESH_WAVES)), dim3(256), 0, st, V, member, (uint16_t *)(ws + l.group_count), vtot,
                       l.nsegv);
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, st, ttot, l.nsegt, vtot, l.nsegv, (uint32_t *)part_triangle_offsets,
                       (uint32_t *)part_vertex_offsets, counts);
    SN_LAUNCH_CHECK("k_split_rank / k_split_scan");
    return SN_OK;
}

extern "C" int sn_rm_mesh_split_emit(const int32_t *triangles, uint32_t T, uint32_t V, const float *vertices, const float *normals, void *workspace,
                                     size_t workspace_bytes, float *out_vertices, float *out_normals, int32_t *out_triangles,
                                     int32_t *source_vertex, int32_t *source_triangle, uint32_t cap_v, uint32_t cap_t, sn_stream_t stream) {
    if (V == 0 || T == 0 || (cap_v == 0 && cap_t == 0)) return SN_OK;          // nothing can be stored
    SN_REQUIRE((triangles || cap_t == 0) && (vertices || cap_v == 0), "mesh_split_emit: NULL pointer");
    SN_REQUIRE((out_vertices || cap_v == 0) && (out_triangles || cap_t == 0) && (out_normals || !normals || cap_v == 0),
               "mesh_split_emit: NULL output with a non-zero capacity");
    SN_REQUIRE(cap_v <= 0x7fffffffu, "mesh_split_emit: cap_v beyond the int32 vertex ids of the triangles");
    SplitLayout l;
    const int rc = split_check("mesh_split_emit", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    uint8_t *ws = (uint8_t *)workspace;
    const uint32_t *ttot = (const uint32_t *)(ws + l.ttot), *vtot = (const uint32_t *)(ws + l.vtot), *trank = (const uint32_t *)(ws + l.trank);
    const unsigned long long *member = (const unsigned long long *)(ws + l.member);
    const uint16_t *group_count = (const uint16_t *)(ws + l.group_count);
    uint32_t *first_row = (uint32_t *)(ws + l.first_row);
    hipStream_t st = (hipStream_t)stream;
    // the vertices also with cap_v = 0: the triangles read first_row
    hipLaunchKernelGGL(k_split_emit_vertices, dim3(div_up(V, 256)), dim3(256), 0, st, V, (const uint32_t *)vertices, (const uint32_t *)normals, member,
                       group_count, vtot, l.nsegv, first_row, (uint32_t *)out_vertices, (uint32_t *)out_normals, source_vertex, cap_v);
    if (cap_t) hipLaunchKernelGGL(k_split_emit_triangles, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, member, group_count, vtot, l.nsegv,
                                  first_row, trank, ttot, l.nsegt, out_triangles, source_triangle, cap_t);
    SN_LAUNCH_CHECK("k_split_emit");
    return SN_OK;
}
