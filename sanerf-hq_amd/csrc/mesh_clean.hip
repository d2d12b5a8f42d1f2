// mesh_clean.hip — clean-up of an indexed triangle mesh on the device: connected components (sn_rm_mesh_components_init / _sweep),
// their statistics (sn_rm_mesh_component_stats) and the removal of small components (sn_rm_mesh_filter_count / _emit), for gfx950.
//
// Definition: include/sanerf_hip.h states it in full; tests/mesh_clean_ref.py restates it in numpy.  In short: a triangle is valid iff its
// three indices are in [0, V); two vertices are connected iff a valid triangle holds both, closed transitively; label[v] is the smallest
// vertex index of v's component; a component is kept by its triangle count and by its key (count << 32 | ~root); the filtered mesh keeps
// the relative order of the kept vertices and triangles.
//
// Components.  No workgroup waits on, spins on or retries against another's data, and nothing depends on one workgroup seeing another's
// stores inside a launch (the per-XCD L2s are not coherent, a CU's L1 is never refreshed).  One ROUND is two launches:
//   k_cc_hook   one lane per triangle.  It range-tests a, b, c, reads la, lb, lc, takes m = min and, for every corner x whose label lx is
//               above m, issues atomicMin(&labels[x], m) and atomicMin(&labels[lx], m).  The second hooks the label's label: it is what
//               makes the number of rounds logarithmic instead of the graph's diameter.
//   k_cc_jump   one lane per vertex follows l = labels[l] until labels[l] == l and stores that (atomicMin again).
// Why that is safe.  Invariant of the labels: labels[v] <= v, labels[v] is a vertex of v's component, and a value never increases -- every
// store is an integer atomicMin (device scope) of a value that is itself a label of the same component, and its result does not depend on
// the order of arrival.  A stale read is harmless: inside a launch a read returns a value no older than the launch's start and no smaller
// than the true minimum, so it is still a vertex of the component, above or at the final label; it can only delay convergence.  The chain
// the jump follows strictly decreases (it stops at the first l with labels[l] >= l), so it ends whatever it reads.  A label that is read
// is clamped to its own index before it is used as an address, so even labels that were never initialised address nothing out of range.
// Round flag.  changed[i] becomes nonzero iff round i lowered a label (the atomicMin returned more than it stored): a wave __any, then one
// lane's atomicOr.  A round that lowers nothing stored nothing, so every value it read was the one in memory at its launch boundary -- the
// final one -- and it saw la == lb == lc on every valid triangle: the labels are constant on every component, and since labels[r] <= r
// for the component's smallest vertex r, that constant is r.  So an unchanged round proves the fixed point, which is unique: the labels
// depend on neither the algorithm, the launch shape nor the run.
//
// Statistics.  Integer atomicAdd at the root (order-independent, so deterministic), aggregated per wave: on a real mesh nearly every lane
// of a wave has the same root, so the wave's lanes are grouped by root and one lane per group adds the group's size.
//
// Filter.  The segment pattern of mesh_common.h, once over the vertices (keep = the root of labels[v] is selected) and once over the
// triangles (valid, and its first corner is kept); one workgroup scans both lists of totals and writes counts = {V', T'} (both below
// 2^31).  The emit reads the keep flags, the ranks
// and the scanned totals from the workspace, and `triangles`; never `labels`.  Nothing is placed by an atomic; every store of the emit is
// guarded by cap_v / cap_t and every index is range-tested before it addresses anything.
// Plain vector loads, plain vector stores and integer atomics only.
#include "mesh_common.h"

namespace sn {

constexpr uint32_t CLEAN_MAX_ROUNDS = 4096u;

struct CleanLayout { size_t vtot, ttot, vrank, trank, bytes; uint32_t nsegv, nsegt; };

static inline CleanLayout clean_layout(uint32_t V, uint32_t T) {
    CleanLayout l;
    l.nsegv = div_up(V, MESH_SEG);
    l.nsegt = div_up(T, MESH_SEG);
    l.vtot = 0;
    l.ttot = l.vtot + align16((size_t)l.nsegv * 4u);
    l.vrank = l.ttot + align16((size_t)l.nsegt * 4u);
    l.trank = l.vrank + align16((size_t)V * 4u);
    l.bytes = l.trank + align16((size_t)T * 4u);
    return l;
}

// The label of vertex v as an address: a value outside [0, v] (labels that were never initialised) reads as v itself.
__device__ __forceinline__ uint32_t label_of(const int32_t *labels, uint32_t v) {
    const uint32_t l = (uint32_t)labels[v];
    return l < v ? l : v;
}

__global__ __launch_bounds__(256) void k_cc_init(int32_t *__restrict__ labels, uint32_t V) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < V) labels[v] = (int32_t)v;
}

__global__ __launch_bounds__(256) void k_cc_hook(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, int32_t *labels,
                                                 uint32_t *changed) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool lowered = false;
    if (t < T) {
        uint32_t x[3];
        if (triangle_corners(triangles, t, V, x)) {
            const uint32_t l[3] = {label_of(labels, x[0]), label_of(labels, x[1]), label_of(labels, x[2])};
            const uint32_t m = umin(l[0], umin(l[1], l[2]));
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (l[q] > m) {
                    lowered |= atomicMin(&labels[x[q]], (int32_t)m) > (int32_t)m;
                    lowered |= atomicMin(&labels[l[q]], (int32_t)m) > (int32_t)m;
                }
            }
        }
    }
    if (__any(lowered) && (threadIdx.x & 63u) == 0u) atomicOr(changed, 1u);
}

__global__ __launch_bounds__(256) void k_cc_jump(uint32_t V, int32_t *labels, uint32_t *changed) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    bool lowered = false;
    if (v < V) {
        const uint32_t l0 = label_of(labels, v);
        uint32_t l = l0;
        for (;;) {                                     // strictly decreasing: at most l0 steps, whatever the loads return
            const uint32_t n = (uint32_t)labels[l];
            if (n >= l) break;
            l = n;
        }
        if (l < l0) lowered = atomicMin(&labels[v], (int32_t)l) > (int32_t)l;
    }
    if (__any(lowered) && (threadIdx.x & 63u) == 0u) atomicOr(changed, 1u);
}

// arr[key] += the number of lanes of the wave that are active with that key: the lanes are grouped by key, one lane per group adds.
// Every lane of the wave calls it; key < the array's length wherever active.
__device__ __forceinline__ void wave_add_by_key(int32_t *arr, uint32_t key, bool active) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t todo = __ballot(active);
    while (todo) {                                     // wave-uniform
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t k0 = (uint32_t)__shfl((int)key, (int)lead);
        const uint64_t same = __ballot(active && key == k0);
        if (lane == lead) atomicAdd(&arr[k0], (int32_t)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void k_cc_zero(int32_t *__restrict__ a, int32_t *__restrict__ b, uint32_t V, uint32_t *__restrict__ counts) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < V) { a[v] = 0; b[v] = 0; }
    if (v < 2u) counts[v] = 0u;
}

__global__ __launch_bounds__(256) void k_cc_triangle_counts(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                            const int32_t *__restrict__ labels, int32_t *triangle_counts) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool valid = false;
    uint32_t root = 0u;
    if (t < T) {
        uint32_t c[3];
        valid = triangle_corners(triangles, t, V, c);
        if (valid) root = label_of(labels, c[0]);
    }
    wave_add_by_key(triangle_counts, root, valid);
}

__global__ __launch_bounds__(256) void k_cc_vertex_counts(uint32_t V, const int32_t *__restrict__ labels, const int32_t *__restrict__ triangle_counts,
                                                          int32_t *vertex_counts, uint32_t *counts) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < V;
    const uint32_t root = live ? label_of(labels, v) : 0u;
    const bool is_root = live && root == v;
    const bool has_triangles = is_root && triangle_counts[v] > 0;
    wave_add_by_key(vertex_counts, root, live);
    const uint64_t mr = __ballot(is_root), mt = __ballot(has_triangles);
    if ((threadIdx.x & 63u) == 0u) {
        if (mr) atomicAdd(&counts[0], (uint32_t)__popcll(mr));
        if (mt) atomicAdd(&counts[1], (uint32_t)__popcll(mt));
    }
}

// One wave per segment of 1024 vertices: rank[v] = keep << 31 | number of kept vertices before v in the segment; totals[seg].
__global__ __launch_bounds__(256) void k_clean_rank_vertices(uint32_t V, const int32_t *__restrict__ labels, const int32_t *__restrict__ triangle_counts,
                                                             uint32_t min_triangles, const uint64_t *__restrict__ min_key,
                                                             uint32_t *__restrict__ rank, uint32_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    const uint64_t mk = *min_key;
    const uint32_t mt = min_triangles > 1u ? min_triangles : 1u;
    segment_flag_rank(V, nseg, rank, totals, [&](uint32_t v) {
        const uint32_t r = label_of(labels, v);
        const int32_t tc = triangle_counts[r];
        return tc > 0 && (uint32_t)tc >= mt && (((uint64_t)(uint32_t)tc << 32) | (uint64_t)(0xFFFFFFFFu - r)) >= mk;
    });
}

// The same over the triangles: kept iff valid and its first corner is kept (vrank is the finished output of the launch before).
__global__ __launch_bounds__(256) void k_clean_rank_triangles(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                              const uint32_t *__restrict__ vrank, uint32_t *__restrict__ rank,
                                                              uint32_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    segment_flag_rank(T, nseg, rank, totals, [&](uint32_t t) {
        uint32_t c[3];
        return triangle_corners(triangles, t, V, c) && (vrank[c[0]] & MESH_KEEP) != 0u;
    });
}

__global__ __launch_bounds__(1024) void k_clean_scan(uint32_t *__restrict__ vtot, uint32_t nsegv, uint32_t *__restrict__ ttot, uint32_t nsegt,
                                                     uint32_t *__restrict__ counts) {
    SN_POISON_ALL();
    __shared__ uint32_t ws[16];
    const uint32_t nv = (uint32_t)workgroup_exclusive_scan(vtot, nsegv, ws);
    const uint32_t nt = (uint32_t)workgroup_exclusive_scan(ttot, nsegt, ws);
    if (threadIdx.x == 0u) { counts[0] = nv; counts[1] = nt; }
}

__global__ __launch_bounds__(256) void k_clean_emit_vertices(uint32_t V, const uint32_t *__restrict__ vertices, const uint32_t *__restrict__ normals,
                                                             const uint32_t *__restrict__ vrank, const uint32_t *__restrict__ vbase,
                                                             uint32_t *__restrict__ out_vertices, uint32_t *__restrict__ out_normals,
                                                             int32_t *__restrict__ source_vertex, uint32_t cap_v) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= V) return;
    const uint32_t w = vrank[v];
    if (!(w & MESH_KEEP)) return;
    const uint32_t id = segment_index(vbase, w, v);
    if (id >= cap_v) return;
    const uint32_t *p = vertices + (size_t)v * 3u;
    uint32_t *q = out_vertices + (size_t)id * 3u;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    if (normals) {
        const uint32_t *pn = normals + (size_t)v * 3u;
        uint32_t *qn = out_normals + (size_t)id * 3u;
        qn[0] = pn[0]; qn[1] = pn[1]; qn[2] = pn[2];
    }
    if (source_vertex) source_vertex[id] = (int32_t)v;
}

__global__ __launch_bounds__(256) void k_clean_emit_triangles(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                              const uint32_t *__restrict__ vrank, const uint32_t *__restrict__ vbase,
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
    for (int q = 0; q < 3; ++q)                        // range-tested again, corner by corner: `triangles` may have changed since the count
        out[q] = x[q] < V ? (int32_t)segment_index(vbase, vrank[x[q]], x[q]) : -1;
}

}  // namespace sn

using namespace sn;

#define CLEAN_SIZES(who) SN_UNSUPPORTED(mesh_sizes_ok(V, T), MESH_SIZES_MSG, who, V, T)

extern "C" size_t sn_rm_mesh_clean_workspace_bytes(uint32_t V, uint32_t T) {
    if (!mesh_sizes_ok(V, T)) {
        set_error(MESH_SIZES_MSG, "mesh_clean", V, T);
        return 0;
    }
    return clean_layout(V, T).bytes;
}

extern "C" int sn_rm_mesh_components_init(uint32_t V, int32_t *labels, sn_stream_t stream) {
    if (V == 0) return SN_OK;
    SN_REQUIRE(labels, "mesh_components_init: NULL pointer");
    SN_UNSUPPORTED(V < (1u << 31), "mesh_components_init: V = %u is not supported (below 2^31)", V);
    hipLaunchKernelGGL(k_cc_init, dim3(div_up(V, 256)), dim3(256), 0, (hipStream_t)stream, labels, V);
    SN_LAUNCH_CHECK("k_cc_init");
    return SN_OK;
}

extern "C" int sn_rm_mesh_components_sweep(const int32_t *triangles, uint32_t T, uint32_t V, int32_t *labels, uint32_t rounds, uint32_t *changed,
                                           sn_stream_t stream) {
    if (V == 0 || rounds == 0) return SN_OK;
    SN_REQUIRE(labels && changed && (triangles || T == 0), "mesh_components_sweep: NULL pointer");
    SN_REQUIRE(rounds <= CLEAN_MAX_ROUNDS, "mesh_components_sweep: at most %u rounds per call, got %u", CLEAN_MAX_ROUNDS, rounds);
    CLEAN_SIZES("mesh_components_sweep");
    hipStream_t st = (hipStream_t)stream;
    SN_HIP_OK(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(uint32_t), st));
    for (uint32_t i = 0; i < rounds; ++i) {
        if (T) hipLaunchKernelGGL(k_cc_hook, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, labels, changed + i);
        hipLaunchKernelGGL(k_cc_jump, dim3(div_up(V, 256)), dim3(256), 0, st, V, labels, changed + i);
    }
    SN_LAUNCH_CHECK("k_cc_hook / k_cc_jump");
    return SN_OK;
}

extern "C" int sn_rm_mesh_component_stats(const int32_t *triangles, uint32_t T, uint32_t V, const int32_t *labels, int32_t *triangle_counts,
                                          int32_t *vertex_counts, uint32_t *counts, sn_stream_t stream) {
    if (V == 0) return SN_OK;              // no vertex, no root: nothing is stored, counts included
    SN_REQUIRE(labels && triangle_counts && vertex_counts && counts && (triangles || T == 0), "mesh_component_stats: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    CLEAN_SIZES("mesh_component_stats");
    hipLaunchKernelGGL(k_cc_zero, dim3(div_up(V, 256)), dim3(256), 0, st, triangle_counts, vertex_counts, V, counts);
    if (T) hipLaunchKernelGGL(k_cc_triangle_counts, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, labels, triangle_counts);
    hipLaunchKernelGGL(k_cc_vertex_counts, dim3(div_up(V, 256)), dim3(256), 0, st, V, labels, triangle_counts, vertex_counts, counts);
    SN_LAUNCH_CHECK("k_cc_triangle_counts / k_cc_vertex_counts");
    return SN_OK;
}

static int clean_check(const char *who, uint32_t V, uint32_t T, const void *workspace, size_t bytes, CleanLayout *l) {
    SN_REQUIRE(workspace, "%s: NULL pointer", who);
    CLEAN_SIZES(who);
    *l = clean_layout(V, T);
    return workspace_check(who, workspace, bytes, l->bytes);
}

extern "C" int sn_rm_mesh_filter_count(const int32_t *triangles, uint32_t T, uint32_t V, const int32_t *labels, const int32_t *triangle_counts,
                                       uint32_t min_triangles, const uint64_t *min_key, void *workspace, size_t workspace_bytes,
                                       uint32_t *counts, sn_stream_t stream) {
    if (V == 0) return SN_OK;              // the empty mesh: nothing is stored, counts included
    SN_REQUIRE(labels && triangle_counts && min_key && counts && (triangles || T == 0), "mesh_filter_count: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    CleanLayout l;
    const int rc = clean_check("mesh_filter_count", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *vtot = (uint32_t *)(ws + l.vtot), *ttot = (uint32_t *)(ws + l.ttot), *vrank = (uint32_t *)(ws + l.vrank), *trank = (uint32_t *)(ws + l.trank);
    hipLaunchKernelGGL(k_clean_rank_vertices, dim3(div_up(l.nsegv, MESH_WAVES)), dim3(256), 0, st, V, labels, triangle_counts, min_triangles,
                       min_key, vrank, vtot, l.nsegv);
    if (T) hipLaunchKernelGGL(k_clean_rank_triangles, dim3(div_up(l.nsegt, MESH_WAVES)), dim3(256), 0, st, triangles, T, V, vrank, trank, ttot,
                              l.nsegt);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(1024), 0, st, vtot, l.nsegv, ttot, l.nsegt, counts);
    SN_LAUNCH_CHECK("k_clean_rank / k_clean_scan");
    return SN_OK;
}

extern "C" int sn_rm_mesh_filter_emit(const int32_t *triangles, uint32_t T, uint32_t V, const float *vertices, const float *normals,
                                      const void *workspace, size_t workspace_bytes, float *out_vertices, float *out_normals,
                                      int32_t *out_triangles, int32_t *source_vertex, uint32_t cap_v, uint32_t cap_t, sn_stream_t stream) {
    if (V == 0 || (cap_v == 0 && cap_t == 0)) return SN_OK;          // nothing can be stored
    SN_REQUIRE((triangles || T == 0 || cap_t == 0) && (vertices || cap_v == 0), "mesh_filter_emit: NULL pointer");
    SN_REQUIRE((out_vertices || cap_v == 0) && (out_triangles || cap_t == 0 || T == 0) && (out_normals || !normals || cap_v == 0),
               "mesh_filter_emit: NULL output with a non-zero capacity");
    SN_REQUIRE(cap_v <= 0x7fffffffu, "mesh_filter_emit: cap_v beyond the int32 vertex ids of the triangles");
    CleanLayout l;
    const int rc = clean_check("mesh_filter_emit", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    const uint8_t *ws = (const uint8_t *)workspace;
    const uint32_t *vtot = (const uint32_t *)(ws + l.vtot), *ttot = (const uint32_t *)(ws + l.ttot);
    const uint32_t *vrank = (const uint32_t *)(ws + l.vrank), *trank = (const uint32_t *)(ws + l.trank);
    hipStream_t st = (hipStream_t)stream;
    if (cap_v) hipLaunchKernelGGL(k_clean_emit_vertices, dim3(div_up(V, 256)), dim3(256), 0, st, V, (const uint32_t *)vertices,
                                  (const uint32_t *)normals, vrank, vtot, (uint32_t *)out_vertices, (uint32_t *)out_normals, source_vertex, cap_v);
    if (cap_t && T) hipLaunchKernelGGL(k_clean_emit_triangles, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, vrank, vtot, trank, ttot,
                                       out_triangles, cap_t);
    SN_LAUNCH_CHECK("k_clean_emit");
    return SN_OK;
}
