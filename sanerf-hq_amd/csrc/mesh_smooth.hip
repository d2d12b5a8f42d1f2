// mesh_smooth.hip — Taubin / Laplacian smoothing of an indexed triangle mesh in fixed point, and the geometric normals of the result
// (sn_rm_mesh_smooth_build / _steps / _emit), for gfx950.
//
// Definition: include/sanerf_hip.h states it in full; tests/mesh_smooth_ref.py restates it in numpy.  In short: a vertex is quantised to
// Q = rint((p - origin) / quantum) (fp32; placed iff every component is in [0, 2^22)); a valid triangle (a, b, c) -- indices in range and
// pairwise distinct -- gives a the pair (next = b, prev = c), b the pair (c, a), c the pair (a, b); a vertex is open iff the sums of
// mix(next) and of mix(prev) over its pairs differ; a half-step with factor f moves every free vertex by rint(f (S / n - Q)), S and n the
// integer sum and the count of the placed next and prev of its pairs, all vertices at once; the emit turns the integers that moved back
// into fp32, leaves the others their input bits, and sums (Q_next - Q_v) x (Q_prev - Q_v) over each vertex's pairs for the normal.
//
// The topology does not change over the iterations, so the build inverts it ONCE and every later pass gathers:
//   k_smooth_degree   one lane per triangle: the valid ones count one pair at each corner (integer atomicAdd).
//   k_smooth_rank     one wave per 1024 vertices: the exclusive prefix of the degrees inside the segment (64-bit), the segment's total.
//   k_smooth_scan     one workgroup: exclusive scan of the totals.  A vertex's row of pairs starts at base[v >> 10] + rank[v].
//   k_smooth_fill     one lane per triangle: each corner takes the slot atomicAdd(cursor[v], 1) of its vertex's row and stores (next, prev).
//                     The order of the pairs INSIDE a row therefore depends on the run.  No output can see it: every consumer of a row
//                     -- the open test, the half-step, the normal -- is a sum of integers modulo 2^64 over the row, and such a sum does
//                     not depend on the order of its terms.  The row itself (its start, its length) is fixed by the scan.
//   k_smooth_init     one lane per vertex: quantises, reads the row for the open test, stores Q[v] = {x, y, z, placed | open << 1}.
// A half-step is ONE launch, one lane per vertex: the row, Q[next] and Q[prev] from one buffer (16 bytes a neighbour), the new Q into the
// other.  Plain vector loads and stores only; no atomics; no workgroup waits on another.  Which of the two buffers is current is a word in
// the workspace (a Laplacian iteration is one half-step, so calls must compose across an odd number): every launch gets the number of
// half-steps issued before it in its call, and the call flips the word at its end if it issued an odd number.
// The emit gathers over the same rows: no triangle pass, no atomics.
// A row longer than SMOOTH_LONG pairs (a fan's apex) is summed by the whole wave of its owner, lanes striding the row, and the partial
// sums added across the wave -- integers again, so the result equals the one-lane sum.
// Integer atomics appear in the build only (degree counts and cursors).  Every index read from `triangles` or from a row is range-tested
// before it is an address, and a row is read only if it lies inside the 3T pairs of the workspace.
#include "mesh_common.h"

#include <cmath>

namespace sn {

#ifndef SN_SMOOTH_LONG
#define SN_SMOOTH_LONG 128u                    // (tools/mesh_smooth_bench.py --fan times a build with another value)
#endif
constexpr uint32_t SMOOTH_LONG = SN_SMOOTH_LONG;       // pairs: a longer row is summed by the wave
constexpr int32_t SMOOTH_RANGE = 1 << 22;      // Q in [0, 2^22)
constexpr int32_t SMOOTH_PLACED = 1, SMOOTH_OPEN = 2, SMOOTH_MOVED = 4;

struct SmoothQuant { float origin[3], quantum; };

// Parts in order, each rounded up to 16 bytes.  head[0] = which of qa / qb is current.
struct SmoothLayout { size_t head, qa, qb, rank, deg, cursor, base, pairs, bytes; uint32_t nseg; };

static inline SmoothLayout smooth_layout(uint32_t V, uint32_t T) {
    SmoothLayout l;
    l.nseg = div_up(V, MESH_SEG);
    l.head = 0;
    l.qa = l.head + 16u;
    l.qb = l.qa + (size_t)V * 16u;
    l.rank = l.qb + (size_t)V * 16u;
    l.deg = l.rank + align16((size_t)V * 8u);
    l.cursor = l.deg + align16((size_t)V * 4u);
    l.base = l.cursor + align16((size_t)V * 4u);
    l.pairs = l.base + align16((size_t)l.nseg * 8u);
    l.bytes = l.pairs + align16((size_t)T * 24u);
    return l;
}

// Q of a position: per axis u = p - origin, s = u / quantum (two fp32 roundings, IEEE division), r = rintf(s); placed iff every r is in
// [0, 2^22) -- which no NaN and no infinity is.  An unplaced vertex gets {0, 0, 0, 0}.
__device__ __forceinline__ int4 smooth_quantise(const float *__restrict__ p, const SmoothQuant &qt) {
    int4 q = make_int4(0, 0, 0, SMOOTH_PLACED);
    int32_t r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = p[a] - qt.origin[a];
        const float s = u / qt.quantum;
        const float f = rintf(s);
        const bool in = f >= 0.0f && f < 4194304.0f;
        r[a] = in ? (int32_t)f : 0;
        if (!in) q.w = 0;
    }
    if (q.w) { q.x = r[0]; q.y = r[1]; q.z = r[2]; }
    return q;
}

__device__ __forceinline__ uint64_t smooth_mix(uint32_t i) {       // the finaliser of splitmix64 (public domain) of i + 1
    uint64_t x = (uint64_t)i + 1u;
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The three indices of triangle t; false unless all lie in [0, V) and are pairwise distinct.
__device__ __forceinline__ bool smooth_triangle(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, uint32_t c[3]) {
    return triangle_corners(triangles, t, V, c) && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

__global__ __launch_bounds__(256) void k_smooth_degree(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, uint32_t *deg) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t c[3];
    if (t >= T || !smooth_triangle(triangles, t, V, c)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&deg[c[k]], 1u);
}

// One wave per segment of 1024 vertices: rank[v] = the pairs of the segment's vertices before v; totals[seg].  64 bits: 3T passes 2^32.
__global__ __launch_bounds__(256) void k_smooth_rank(const uint32_t *__restrict__ deg, uint32_t V, uint64_t *__restrict__ rank,
                                                     uint64_t *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform; the kernel has no barrier
    uint64_t base = 0u;
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t v = seg * MESH_SEG + it * 64u + lane;
        const uint64_t c = v < V ? (uint64_t)deg[v] : 0u;
        const uint64_t s = wave_inclusive_sum(c);
        if (v < V) rank[v] = base + (s - c);
        base += shfl64(s, 63);
    }
    if (lane == 0u) totals[seg] = base;
}

// Exclusive scan of the n segment totals in place by one workgroup of 1024.
__global__ __launch_bounds__(1024) void k_smooth_scan(uint64_t *__restrict__ totals, uint32_t n) {
    SN_POISON_ALL();
    __shared__ uint64_t ws[16];
    workgroup_exclusive_scan(totals, n, ws);
}

__global__ __launch_bounds__(256) void k_smooth_fill(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                     const uint64_t *__restrict__ rank, const uint64_t *__restrict__ base, uint32_t *cursor,
                                                     int2 *__restrict__ pairs) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t c[3];
    if (t >= T || !smooth_triangle(triangles, t, V, c)) return;
    const uint64_t cap = 3u * (uint64_t)T;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = c[k];
        const uint64_t slot = base[v >> MESH_SEG_LOG2] + rank[v] + atomicAdd(&cursor[v], 1u);
        if (slot < cap) pairs[slot] = make_int2((int32_t)c[(k + 1) % 3], (int32_t)c[(k + 2) % 3]);      // (`triangles` may have changed since the count)
    }
}

// The row of vertex v: where it starts and how many pairs it has; none if it does not lie inside the cap pairs of the workspace.
struct SmoothRows {
    const uint64_t *rank, *base;
    const uint32_t *deg;
    const int2 *pairs;
    uint64_t cap;
};

__device__ __forceinline__ void smooth_row(const SmoothRows &rows, uint32_t v, uint64_t &begin, uint32_t &d) {
    begin = rows.base[v >> MESH_SEG_LOG2] + rows.rank[v];
    d = rows.deg[v];
    if (begin > rows.cap || (uint64_t)d > rows.cap - begin) { begin = 0u; d = 0u; }
}

// acc[0 .. K) += the sum over the d pairs from `begin` of what f adds for a pair (64-bit words, modulo 2^64).  EVERY lane of the wave calls
// it (d = 0 for a lane without a vertex).  A row of at most SMOOTH_LONG pairs is summed by its lane; the longer ones one after the other by
// the whole wave, with f's context broadcast from the owner.  F: void operator()(int2, uint64_t *) const; F from_lane(int) const.
template <int K, class F>
__device__ __forceinline__ void smooth_row_sum(const int2 *__restrict__ pairs, uint64_t begin, uint32_t d, const F &f, uint64_t acc[K]) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool wide = d > SMOOTH_LONG;
    if (!wide) {
#pragma unroll 4
        for (uint32_t i = 0; i < d; ++i) f(pairs[begin + i], acc);
    }
    uint64_t todo = __ballot(wide);
    while (todo) {                         // wave-uniform
        const int owner = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1u;
        const uint64_t b = shfl64(begin, owner);
        const uint32_t n = (uint32_t)__shfl((int)d, owner);
        const F g = f.from_lane(owner);
        uint64_t part[K];
#pragma unroll
        for (int k = 0; k < K; ++k) part[k] = 0u;
        for (uint32_t i = lane; i < n; i += 64u) g(pairs[b + i], part);
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) part[k] += shfl_xor64(part[k], m);
            if (lane == (uint32_t)owner) acc[k] += part[k];
        }
    }
}

struct SmoothOpenSum {                     // acc = {sum mix(next), sum mix(prev)}
    uint32_t V;
    __device__ __forceinline__ void operator()(int2 pr, uint64_t *acc) const {
        if ((uint32_t)pr.x < V && (uint32_t)pr.y < V) { acc[0] += smooth_mix((uint32_t)pr.x); acc[1] += smooth_mix((uint32_t)pr.y); }
    }
    __device__ __forceinline__ SmoothOpenSum from_lane(int) const { return *this; }
};

__global__ __launch_bounds__(256) void k_smooth_init(const float *__restrict__ vertices, uint32_t V, SmoothQuant qt, SmoothRows rows,
                                                     int4 *__restrict__ qa, uint32_t *__restrict__ head) {
    SN_POISON_ALL();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < V;
    uint64_t begin = 0u;
    uint32_t d = 0u;
    if (live) smooth_row(rows, v, begin, d);
    uint64_t acc[2] = {0u, 0u};
    smooth_row_sum<2>(rows.pairs, begin, d, SmoothOpenSum{V}, acc);
    if (!live) return;
    int4 q = smooth_quantise(vertices + (size_t)v * 3u, qt);
    if (acc[0] != acc[1]) q.w |= SMOOTH_OPEN;
    qa[v] = q;
    if (v == 0u) head[0] = 0u;             // qa is current
}

struct SmoothNeighbourSum {                // acc = {Sx, Sy, Sz, n} over the placed next and prev
    const int4 *q;
    uint32_t V;
    __device__ __forceinline__ void add(int32_t i, uint64_t *acc) const {
        if ((uint32_t)i >= V) return;
        const int4 p = q[(uint32_t)i];
        if (p.w & SMOOTH_PLACED) {
            acc[0] += (uint64_t)(int64_t)p.x; acc[1] += (uint64_t)(int64_t)p.y; acc[2] += (uint64_t)(int64_t)p.z;
            acc[3] += 1u;
        }
    }
    __device__ __forceinline__ void operator()(int2 pr, uint64_t *acc) const { add(pr.x, acc); add(pr.y, acc); }
    __device__ __forceinline__ SmoothNeighbourSum from_lane(int) const { return *this; }
};

// One half-step: reads the buffer that is current after `done` half-steps of this call, writes the other.
__global__ __launch_bounds__(256) void k_smooth_step(int4 *qa, int4 *qb, const uint32_t *__restrict__ head, uint32_t done, uint32_t V,
                                                     SmoothRows rows, double f, int pin_open) {
    SN_POISON_ALL();
    const bool swapped = ((head[0] + done) & 1u) != 0u;
    const int4 *src = swapped ? qb : qa;
    int4 *dst = swapped ? qa : qb;
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < V;
    uint64_t begin = 0u;
    uint32_t d = 0u;
    if (live) smooth_row(rows, v, begin, d);
    uint64_t acc[4] = {0u, 0u, 0u, 0u};
    smooth_row_sum<4>(rows.pairs, begin, d, SmoothNeighbourSum{src, V}, acc);
    if (!live) return;
    int4 q = src[v];
    const bool is_free = (q.w & SMOOTH_PLACED) && acc[3] != 0u && !((q.w & SMOOTH_OPEN) && pin_open);
    if (is_free) {
        const double n = (double)acc[3];
        int32_t *c = &q.x;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double dlt = (double)(int64_t)acc[a] / n - (double)c[a];
            const int64_t moved = (int64_t)c[a] + (int64_t)rint(f * dlt);
            c[a] = (int32_t)(moved < 0 ? 0 : (moved > SMOOTH_RANGE - 1 ? SMOOTH_RANGE - 1 : moved));
        }
    }
    dst[v] = q;
}

__global__ void k_smooth_flip(uint32_t *head) {
    SN_POISON_ALL();
    if (blockIdx.x == 0u && threadIdx.x == 0u) head[0] = (head[0] + 1u) & 1u;
}

struct SmoothNormalSum {                   // acc = the sum of (Q_next - Q_v) x (Q_prev - Q_v) over the pairs with three placed corners
    const int4 *q;
    uint32_t V;
    int4 own;
    __device__ __forceinline__ void operator()(int2 pr, uint64_t *acc) const {
        if ((uint32_t)pr.x >= V || (uint32_t)pr.y >= V) return;
        const int4 n = q[(uint32_t)pr.x], p = q[(uint32_t)pr.y];
        if (!((n.w & p.w & own.w) & SMOOTH_PLACED)) return;
        const int64_t ax = (int64_t)n.x - own.x, ay = (int64_t)n.y - own.y, az = (int64_t)n.z - own.z;
        const int64_t bx = (int64_t)p.x - own.x, by = (int64_t)p.y - own.y, bz = (int64_t)p.z - own.z;
        acc[0] += (uint64_t)(ay * bz - az * by);
        acc[1] += (uint64_t)(az * bx - ax * bz);
        acc[2] += (uint64_t)(ax * by - ay * bx);
    }
    __device__ __forceinline__ SmoothNormalSum from_lane(int lane) const {
        return SmoothNormalSum{q, V, make_int4(__shfl(own.x, lane), __shfl(own.y, lane), __shfl(own.z, lane), __shfl(own.w, lane))};
    }
};

template <bool NORMALS>
__global__ __launch_bounds__(256) void k_smooth_emit(const float *__restrict__ vertices, uint32_t V, SmoothQuant qt, const int4 *qa, const int4 *qb,
                                                     const uint32_t *__restrict__ head, SmoothRows rows, float *__restrict__ out_vertices,
                                                     float *__restrict__ out_normals, uint8_t *__restrict__ vertex_flags) {
    SN_POISON_ALL();
    const int4 *cur = (head[0] & 1u) ? qb : qa;
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < V;
    int4 q = make_int4(0, 0, 0, 0);
    if (live) q = cur[v];
    if (NORMALS) {
        uint64_t begin = 0u;
        uint32_t d = 0u;
        if (live) smooth_row(rows, v, begin, d);
        uint64_t acc[3] = {0u, 0u, 0u};
        smooth_row_sum<3>(rows.pairs, begin, d, SmoothNormalSum{cur, V, q}, acc);
        if (live) {
            const double sx = (double)(int64_t)acc[0], sy = (double)(int64_t)acc[1], sz = (double)(int64_t)acc[2];
            const double len = sqrt((sx * sx + sy * sy) + sz * sz);
            const bool zero = acc[0] == 0u && acc[1] == 0u && acc[2] == 0u;
            float *n = out_normals + (size_t)v * 3u;
            n[0] = zero ? 0.0f : (float)(sx / len);
            n[1] = zero ? 0.0f : (float)(sy / len);
            n[2] = zero ? 0.0f : (float)(sz / len);
        }
    }
    if (!live) return;
    const float *p = vertices + (size_t)v * 3u;
    const int4 q0 = smooth_quantise(p, qt);
    const bool placed = (q.w & SMOOTH_PLACED) != 0;
    const bool moved = placed && (q.x != q0.x || q.y != q0.y || q.z != q0.z);
    const int32_t *c = &q.x;
    float *o = out_vertices + (size_t)v * 3u;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = moved ? (float)((double)qt.origin[a] + (double)qt.quantum * (double)c[a]) : p[a];
    if (vertex_flags) vertex_flags[v] = (uint8_t)((q.w & (SMOOTH_PLACED | SMOOTH_OPEN)) | (moved ? SMOOTH_MOVED : 0));
}

}  // namespace sn

using namespace sn;

extern "C" size_t sn_rm_mesh_smooth_workspace_bytes(uint32_t V, uint32_t T) {
    if (!mesh_sizes_ok(V, T)) {
        set_error(MESH_SIZES_MSG, "mesh_smooth", V, T);
        return 0;
    }
    return smooth_layout(V, T).bytes;
}

// The checks the three entries share; fills the layout.
static int smooth_check(const char *who, uint32_t V, uint32_t T, const void *workspace, size_t bytes, SmoothLayout *l) {
    SN_REQUIRE(workspace, "%s: NULL pointer", who);
    SN_UNSUPPORTED(mesh_sizes_ok(V, T), MESH_SIZES_MSG, who, V, T);
    *l = smooth_layout(V, T);
    return workspace_check(who, workspace, bytes, l->bytes);
}

static int smooth_quant(const char *who, const float *origin, float quantum, SmoothQuant *qt) {
    SN_REQUIRE(origin, "%s: NULL pointer", who);
    for (int a = 0; a < 3; ++a) {
        SN_REQUIRE(std::isfinite(origin[a]), "%s: origin[%d] = %g is not finite", who, a, (double)origin[a]);
        qt->origin[a] = origin[a];
    }
    SN_REQUIRE(std::isfinite(quantum) && quantum > 0.0f, "%s: quantum = %g must be positive and finite", who, (double)quantum);
    qt->quantum = quantum;
    return SN_OK;
}

static SmoothRows smooth_rows(const uint8_t *ws, const SmoothLayout &l, uint32_t T) {
    return SmoothRows{(const uint64_t *)(ws + l.rank), (const uint64_t *)(ws + l.base), (const uint32_t *)(ws + l.deg), (const int2 *)(ws + l.pairs),
                      3u * (uint64_t)T};
}

extern "C" int sn_rm_mesh_smooth_build(const float *vertices, const int32_t *triangles, uint32_t V, uint32_t T, const float *origin, float quantum,
                                       void *workspace, size_t workspace_bytes, sn_stream_t stream) {
    if (V == 0) return SN_OK;              // the empty mesh: nothing is stored
    SN_REQUIRE(vertices && (triangles || T == 0), "mesh_smooth_build: NULL pointer");
    SmoothQuant qt;
    SmoothLayout l;
    int rc = smooth_quant("mesh_smooth_build", origin, quantum, &qt);
    if (rc != SN_OK) return rc;
    rc = smooth_check("mesh_smooth_build", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint64_t *rank = (uint64_t *)(ws + l.rank), *base = (uint64_t *)(ws + l.base);
    uint32_t *deg = (uint32_t *)(ws + l.deg), *cursor = (uint32_t *)(ws + l.cursor);
    SN_HIP_OK(hipMemsetAsync(deg, 0, l.base - l.deg, st));                     // the degrees and the cursors
    if (T) hipLaunchKernelGGL(k_smooth_degree, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, deg);
    hipLaunchKernelGGL(k_smooth_rank, dim3(div_up(l.nseg, MESH_WAVES)), dim3(256), 0, st, deg, V, rank, base, l.nseg);
    hipLaunchKernelGGL(k_smooth_scan, dim3(1), dim3(1024), 0, st, base, l.nseg);
    if (T) hipLaunchKernelGGL(k_smooth_fill, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, rank, base, cursor, (int2 *)(ws + l.pairs));
    hipLaunchKernelGGL(k_smooth_init, dim3(div_up(V, 256)), dim3(256), 0, st, vertices, V, qt, smooth_rows(ws, l, T), (int4 *)(ws + l.qa),
                       (uint32_t *)(ws + l.head));
    SN_LAUNCH_CHECK("k_smooth_degree .. k_smooth_init");
    return SN_OK;
}

extern "C" int sn_rm_mesh_smooth_steps(uint32_t V, uint32_t T, uint32_t iterations, float lambda, float mu, int pin_open, void *workspace,
                                       size_t workspace_bytes, sn_stream_t stream) {
    if (V == 0) return SN_OK;
    SN_REQUIRE(lambda > 0.0f && lambda <= 1.0f, "mesh_smooth_steps: lambda = %g must be in (0, 1]", (double)lambda);
    SN_REQUIRE(mu == 0.0f || (mu >= -1.0f && mu < -lambda), "mesh_smooth_steps: mu = %g must be 0 or in [-1, -lambda)", (double)mu);
    SmoothLayout l;
    const int rc = smooth_check("mesh_smooth_steps", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *head = (uint32_t *)(ws + l.head);
    const SmoothRows rows = smooth_rows(ws, l, T);
    const bool taubin = mu != 0.0f;
    uint32_t done = 0;                     // half-steps issued; only its parity is used
    for (uint32_t it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_smooth_step, dim3(div_up(V, 256)), dim3(256), 0, st, (int4 *)(ws + l.qa), (int4 *)(ws + l.qb), head, done++ & 1u, V, rows,
                           (double)lambda, pin_open ? 1 : 0);
        if (taubin) hipLaunchKernelGGL(k_smooth_step, dim3(div_up(V, 256)), dim3(256), 0, st, (int4 *)(ws + l.qa), (int4 *)(ws + l.qb), head, done++ & 1u, V,
                                       rows, (double)mu, pin_open ? 1 : 0);
    }
    if (done & 1u) hipLaunchKernelGGL(k_smooth_flip, dim3(1), dim3(64), 0, st, head);
    SN_LAUNCH_CHECK("k_smooth_step");
    return SN_OK;
}

extern "C" int sn_rm_mesh_smooth_emit(const float *vertices, uint32_t V, uint32_t T, const float *origin, float quantum, const void *workspace,
                                      size_t workspace_bytes, float *out_vertices, float *out_normals, uint8_t *vertex_flags, sn_stream_t stream) {
    if (V == 0) return SN_OK;
    SN_REQUIRE(vertices && out_vertices, "mesh_smooth_emit: NULL pointer");
    SmoothQuant qt;
    SmoothLayout l;
    int rc = smooth_quant("mesh_smooth_emit", origin, quantum, &qt);
    if (rc != SN_OK) return rc;
    rc = smooth_check("mesh_smooth_emit", V, T, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *ws = (const uint8_t *)workspace;
    const int4 *qa = (const int4 *)(ws + l.qa), *qb = (const int4 *)(ws + l.qb);
    const uint32_t *head = (const uint32_t *)(ws + l.head);
    const SmoothRows rows = smooth_rows(ws, l, T);
    if (out_normals) hipLaunchKernelGGL(k_smooth_emit<true>, dim3(div_up(V, 256)), dim3(256), 0, st, vertices, V, qt, qa, qb, head, rows, out_vertices, out_normals, vertex_flags);
    else hipLaunchKernelGGL(k_smooth_emit<false>, dim3(div_up(V, 256)), dim3(256), 0, st, vertices, V, qt, qa, qb, head, rows, out_vertices, out_normals, vertex_flags);
    SN_LAUNCH_CHECK("k_smooth_emit");
    return SN_OK;
}
