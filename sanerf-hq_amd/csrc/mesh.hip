// mesh.hip — geometry export: lattice positions (sn_rm_lattice_points) and marching tetrahedra on a density lattice
// (sn_rm_isosurface_count / sn_rm_isosurface_emit), for gfx950.
//
// Definition: include/sanerf_hip.h states it in full; tests/mesh_ref.py restates it in numpy, operation for operation.  In short: a lattice
// vertex is inside iff f > iso; each lattice vertex owns the up-to-7 edges to its +x, +y, +z, +xy, +xz, +yz, +xyz neighbours; an edge whose
// ends differ carries a mesh vertex at t = (iso - f_a) / (f_b - f_a); a cell splits into the six Kuhn tetrahedra; the triangles of a
// tetrahedron and their orientation come from a 6 x 16 table generated at compile time (mesh_table.h).  Mesh vertices are numbered by owning
// lattice vertex then slot, triangles by cell then tetrahedron then triangle.
//
// Launch plan: the segment pattern of mesh_common.h with two totals a segment (two launches for the count, one for the emit; no workgroup
// waits on another, nothing is placed by an atomic):
//   k_iso_classify  one wave per SEGMENT of 1024 consecutive lattice vertices (z fastest: coalesced rows), 16 steps of 64.  A lane loads the
//                   column of its vertex -- f at (x,y), (x,y+1), (x+1,y), (x+1,y+1), same z -- and takes the z+1 column's inside bits from the
//                   next lane (lane 63: from lane 0 of the next step, whose loads were issued two steps earlier): 4 loads per lattice
//                   vertex, issued before the ranking of an earlier step.  It writes the byte [inside | 7 edge bits] and the vertex's
//                   rank inside the segment (ballots of the count's bits + mbcnt above a running base), and the segment's two totals.
//   k_iso_scan      one workgroup: exclusive scan of the segment totals in place (64-bit carry), the two grand totals to counts[2].
//   k_iso_emit      the same segments.  Everything structural is re-derived from the BYTES -- the inside bits of a cell's 8 corners are its
//                   lowest corner's byte -- so the emit agrees with the count whatever the volume holds by then; the volume is read only on
//                   crossing edges (f_a, f_b; the gradients).  id(v, e) = segment base + rank[v] + popcount(byte[v] & ((1 << e) - 1)).
// Every store of the emit is guarded by cap_v / cap_t; every load stays inside the lattice by the kernel's own range tests.
// Workspace: 8 bytes per segment, 4 bytes + 1 byte per lattice vertex.  Plain vector loads and stores.
#include "mesh_common.h"
#include "mesh_table.h"

namespace sn {

constexpr TetTable H_TET = make_tet_table();
static_assert(!H_TET.bad, "a triangle of the marching-tetrahedra table has no orientation (zero dot product)");
__constant__ TetTable c_tet = H_TET;

struct IsoDims { uint32_t nx, ny, nz, sx, V; };      // sx = ny * nz (the x stride); V = nx * ny * nz < 2^31

struct IsoLayout { size_t totals, base, mask, bytes; uint32_t nseg; };

static inline bool iso_dims(uint32_t nx, uint32_t ny, uint32_t nz, IsoDims *d) {
    if (nx < 2u || ny < 2u || nz < 2u) return false;
    const uint64_t yz = (uint64_t)ny * nz;
    if (yz >= (1ull << 31) || yz * nx >= (1ull << 31)) return false;
    d->nx = nx; d->ny = ny; d->nz = nz; d->sx = (uint32_t)yz; d->V = (uint32_t)(yz * nx);
    return true;
}

static inline IsoLayout iso_layout(const IsoDims &d) {
    IsoLayout l;
    l.nseg = div_up(d.V, MESH_SEG);
    l.totals = 0;
    l.base = align16((size_t)l.nseg * 8u);
    l.mask = l.base + (size_t)d.V * 4u;
    l.bytes = l.mask + align16(d.V);
    return l;
}

__device__ __forceinline__ bool inside_of(float f, float iso) { return f > iso; }      // NaN outside, +inf inside, f == iso outside

// Inside bits of the 8 corners of the cell whose lowest corner has byte m; corner code bit 0 = +x, bit 1 = +y, bit 2 = +z.
__device__ __forceinline__ uint32_t cell_config(uint32_t m) {
    const uint32_t diff = ((m & 1u) << 1) | (((m >> 1) & 1u) << 2) | (((m >> 3) & 1u) << 3) | (((m >> 2) & 1u) << 4) | (((m >> 4) & 1u) << 5)
                          | (((m >> 5) & 1u) << 6) | (((m >> 6) & 1u) << 7);
    return (m & 0x80u) ? (~diff & 0xffu) : diff;
}

__device__ __forceinline__ uint32_t tet_case(uint32_t cfg, int k) {
    return (cfg & 1u) | (((cfg >> tet_corner(k, 1)) & 1u) << 1) | (((cfg >> tet_corner(k, 2)) & 1u) << 2) | (((cfg >> 7) & 1u) << 3);
}

__device__ __forceinline__ uint32_t tet_triangles(uint32_t lm) {
    const uint32_t pc = (uint32_t)__popc(lm);
    return pc == 2u ? 2u : (pc & 1u);
}

__device__ __forceinline__ uint32_t cell_triangles(uint32_t cfg) {
    uint32_t n = 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) n += tet_triangles(tet_case(cfg, k));
    return n;
}

__device__ __forceinline__ void lattice_coords(uint32_t v, const IsoDims &d, uint32_t &x, uint32_t &y, uint32_t &z) {
    const uint32_t xy = v / d.nz;
    z = v - xy * d.nz;
    x = xy / d.ny;
    y = xy - x * d.ny;
}

// One block of 64 consecutive lattice vertices, in two steps so that the loads of a block fly while an earlier block is ranked.
// block_issue: the four values of the lane's column -- (x,y), (x,y+1), (x+1,y), (x+1,y+1) at the vertex's z -- from addresses that are
// always inside the lattice (an out-of-range neighbour, or a vertex past the end, reads its own vertex again: the flags say so), and the
// flags: bit 4 x+1 in range, bit 5 y+1, bit 6 z+1, bit 7 the vertex exists.  block_state: flags | the four inside bits; 0 past the end.
struct BlockLoads { float a, b, c, e; uint32_t flags; };

__device__ __forceinline__ BlockLoads block_issue(const float *__restrict__ f, uint32_t v, const IsoDims &d) {
    const bool live = v < d.V;
    const uint32_t vc = live ? v : d.V - 1u;
    uint32_t x, y, z;
    lattice_coords(vc, d, x, y, z);
    const bool rx = x + 1u < d.nx, ry = y + 1u < d.ny, rz = z + 1u < d.nz;
    const uint32_t ox = rx ? d.sx : 0u, oy = ry ? d.nz : 0u;
    BlockLoads l;
    l.a = f[vc]; l.b = f[vc + oy]; l.c = f[vc + ox]; l.e = f[vc + ox + oy];
    l.flags = live ? ((rx ? 16u : 0u) | (ry ? 32u : 0u) | (rz ? 64u : 0u) | 128u) : 0u;
    return l;
}

__device__ __forceinline__ uint32_t block_state(const BlockLoads &l, float iso) {
    const uint32_t bits = (inside_of(l.a, iso) ? 1u : 0u) | (inside_of(l.b, iso) ? 2u : 0u) | (inside_of(l.c, iso) ? 4u : 0u)
                          | (inside_of(l.e, iso) ? 8u : 0u);
    return l.flags ? (l.flags | bits) : 0u;
}

__global__ __launch_bounds__(256) void k_iso_classify(const float *__restrict__ f, IsoDims d, float iso, uint8_t *__restrict__ mask,
                                                      uint32_t *__restrict__ rank, uint2 *__restrict__ totals, uint32_t nseg) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform; the kernel has no barrier
    const uint32_t v0 = seg * MESH_SEG + lane;
    uint32_t vb = 0u, tb = 0u;
    uint32_t cur = block_state(block_issue(f, v0, d), iso), nxt = block_state(block_issue(f, v0 + 64u, d), iso);
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t v = v0 + it * 64u;
        const BlockLoads ahead = block_issue(f, v + 128u, d);              // two blocks ahead (past the segment's end: the next segment's, unused)
        // the z+1 column: the next lane's, and for lane 63 the next block's lane 0 (same x, y wherever z+1 is in range)
        uint32_t ncode = (uint32_t)__shfl_down((int)cur, 1);
        const uint32_t first_of_next = (uint32_t)__shfl((int)nxt, 0);
        if (lane == 63u) ncode = first_of_next;
        const bool live = (cur & 128u) != 0u, rx = (cur & 16u) != 0u, ry = (cur & 32u) != 0u, rz = (cur & 64u) != 0u;
        const uint32_t code = cur & 15u, in0 = code & 1u;
        uint32_t m = 0u;
        if (rx && ((code >> 2) & 1u) != in0) m |= 1u;
        if (ry && ((code >> 1) & 1u) != in0) m |= 2u;
        if (rz && (ncode & 1u) != in0) m |= 4u;
        if (rx && ry && ((code >> 3) & 1u) != in0) m |= 8u;
        if (rx && rz && ((ncode >> 2) & 1u) != in0) m |= 16u;
        if (ry && rz && ((ncode >> 1) & 1u) != in0) m |= 32u;
        if (rx && ry && rz && ((ncode >> 3) & 1u) != in0) m |= 64u;
        const uint32_t byte = m | (in0 << 7);
        const uint32_t nv = (uint32_t)__popc(m);
        const uint32_t nt = (m != 0u && rx && ry && rz) ? cell_triangles(cell_config(byte)) : 0u;
        uint32_t pv, tv, pt, tt;
        wave_rank<3>(nv, pv, tv);
        wave_rank<4>(nt, pt, tt);
        if (live) { mask[v] = (uint8_t)byte; rank[v] = vb + pv; }
        vb += tv; tb += tt;
        cur = nxt;
        nxt = block_state(ahead, iso);
    }
    if (lane == 0u) totals[seg] = make_uint2(vb, tb);
}

// Exclusive scan of the segment totals, in place; one workgroup of 1024.  counts[0..1] = the grand totals, saturated at 2^32 - 1.
__global__ __launch_bounds__(1024) void k_iso_scan(uint2 *__restrict__ totals, uint32_t nseg, uint32_t *__restrict__ counts) {
    SN_POISON_ALL();
    __shared__ uint32_t ws[2 * 16];
    uint64_t total[2];
    workgroup_exclusive_scan<2>(&totals->x, nseg, ws, total);
    if (threadIdx.x == 0u) {
        counts[0] = total[0] > 0xffffffffull ? 0xffffffffu : (uint32_t)total[0];
        counts[1] = total[1] > 0xffffffffull ? 0xffffffffu : (uint32_t)total[1];
    }
}

// Lattice gradient at (x,y,z): central differences (f[i+1] - f[i-1]) / (2 step), one-sided at the faces.
__device__ __forceinline__ void lattice_gradient(const float *__restrict__ f, const IsoDims &d, uint32_t x, uint32_t y, uint32_t z,
                                                 float sx, float sy, float sz, float &gx, float &gy, float &gz) {
    const uint32_t v = (x * d.ny + y) * d.nz + z;
    const uint32_t xh = x + 1u < d.nx ? 1u : 0u, xl = x ? 1u : 0u, yh = y + 1u < d.ny ? 1u : 0u, yl = y ? 1u : 0u;
    const uint32_t zh = z + 1u < d.nz ? 1u : 0u, zl = z ? 1u : 0u;
    gx = (f[v + xh * d.sx] - f[v - xl * d.sx]) / ((xh + xl == 2u) ? 2.0f * sx : sx);
    gy = (f[v + yh * d.nz] - f[v - yl * d.nz]) / ((yh + yl == 2u) ? 2.0f * sy : sy);
    gz = (f[v + zh] - f[v - zl]) / ((zh + zl == 2u) ? 2.0f * sz : sz);
}

__global__ __launch_bounds__(256) void k_iso_emit(const float *__restrict__ f, IsoDims d, float iso, float ox, float oy, float oz, float sx,
                                                  float sy, float sz, const uint8_t *__restrict__ mask, const uint32_t *__restrict__ rank,
                                                  const uint2 *__restrict__ segbase, uint32_t nseg, float *__restrict__ vertices,
                                                  float *__restrict__ normals, int32_t *__restrict__ triangles, uint32_t cap_v, uint32_t cap_t) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6);
    if (seg >= nseg) return;               // wave-uniform; the kernel has no barrier
    const uint2 sb = segbase[seg];
    uint32_t tb = sb.y;
    const uint32_t v0 = seg * MESH_SEG + lane;
    uint32_t byte_next = v0 < d.V ? (uint32_t)mask[v0] : 0u;
    for (uint32_t it = 0; it < MESH_SEG / 64u; ++it) {
        const uint32_t v = v0 + it * 64u;
        const uint32_t byte = byte_next;
        byte_next = (it + 1u < MESH_SEG / 64u && v + 64u < d.V) ? (uint32_t)mask[v + 64u] : 0u;      // one block ahead of the ballots
        const uint32_t m = byte & 0x7fu;
        uint32_t x = 0u, y = 0u, z = 0u;
        bool rx = false, ry = false, rz = false;
        if (m) {
            lattice_coords(v, d, x, y, z);
            rx = x + 1u < d.nx; ry = y + 1u < d.ny; rz = z + 1u < d.nz;
        }
        const uint32_t cfg = cell_config(byte);
        const uint32_t nt = (m != 0u && rx && ry && rz) ? cell_triangles(cfg) : 0u;
        uint32_t pt, tt;
        wave_rank<4>(nt, pt, tt);
        uint32_t my_t = tb + pt;
        tb += tt;
        if (!m) continue;                  // (the ballots are behind us)
        // ---- the mesh vertices this lattice vertex owns, in slot order
        uint32_t id = sb.x + rank[v];
        const float fa = f[v];
        float gax = 0.0f, gay = 0.0f, gaz = 0.0f;
        if (normals) lattice_gradient(f, d, x, y, z, sx, sy, sz, gax, gay, gaz);
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            const uint32_t ec = slot_corner(e), dx = ec & 1u, dy = (ec >> 1) & 1u, dz = (ec >> 2) & 1u;
            if (!((m >> e) & 1u) || (dx && !rx) || (dy && !ry) || (dz && !rz)) continue;
            const float fb = f[v + dx * d.sx + dy * d.nz + dz];
            float t = (iso - fa) / (fb - fa);
            if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
            if (id < cap_v) {
                float *p = vertices + (size_t)id * 3u;
                p[0] = ox + ((float)x + t * (float)dx) * sx;
                p[1] = oy + ((float)y + t * (float)dy) * sy;
                p[2] = oz + ((float)z + t * (float)dz) * sz;
                if (normals) {
                    float gbx, gby, gbz;
                    lattice_gradient(f, d, x + dx, y + dy, z + dz, sx, sy, sz, gbx, gby, gbz);
                    const float gx = gax + t * (gbx - gax), gy = gay + t * (gby - gay), gz = gaz + t * (gbz - gaz);
                    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
                    const bool good = len > 0.0f && len < __builtin_inff();          // false for NaN
                    float *q = normals + (size_t)id * 3u;
                    q[0] = good ? -gx / len : 0.0f;
                    q[1] = good ? -gy / len : 0.0f;
                    q[2] = good ? -gz / len : 0.0f;
                }
            }
            ++id;
        }
        // ---- the triangles of the cell whose lowest corner this is
        if (!(rx && ry && rz)) continue;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t lm = tet_case(cfg, k), n = tet_triangles(lm);
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t w = c_tet.tri[k][lm][j];
                if (my_t < cap_t) {
                    int32_t *tri = triangles + (size_t)my_t * 3u;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const uint32_t ed = (w >> (6 * q)) & 63u, oc = ed & 7u, sl = ed >> 3;
                        const uint32_t o = v + (oc & 1u) * d.sx + ((oc >> 1) & 1u) * d.nz + ((oc >> 2) & 1u);
                        tri[q] = (int32_t)(segbase[o >> MESH_SEG_LOG2].x + rank[o] + (uint32_t)__popc((uint32_t)mask[o] & ((1u << sl) - 1u)));
                    }
                }
                ++my_t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_lattice_points(float ox, float oy, float oz, float sx, float sy, float sz, uint32_t ny, uint32_t nz,
                                                        uint32_t first, uint32_t count, int contract, float *__restrict__ xyz) {
    SN_POISON_ALL();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = first + i, xy = v / nz, iz = v - xy * nz, ix = xy / ny, iy = xy - ix * ny;
    float x = ox + (float)ix * sx, y = oy + (float)iy * sy, z = oz + (float)iz * sz;
    if (contract) contract3(x, y, z);
    float *p = xyz + (size_t)i * 3u;
    p[0] = x; p[1] = y; p[2] = z;
}

}  // namespace sn

using namespace sn;

extern "C" int sn_rm_lattice_points(const float *origin, const float *step, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t first, uint32_t count,
                                    int32_t contract, float *xyz, sn_stream_t stream) {
    if (count == 0) return SN_OK;
    SN_REQUIRE(origin && step && xyz, "lattice_points: NULL pointer");
    SN_REQUIRE(nx >= 1u && ny >= 1u && nz >= 1u, "lattice_points: empty lattice %u x %u x %u", nx, ny, nz);
    const uint64_t V = (uint64_t)nx * ny * nz;
    SN_UNSUPPORTED((uint64_t)ny * nz < (1ull << 31) && V < (1ull << 31), "lattice_points: at most 2^31 - 1 lattice vertices (%u x %u x %u)", nx, ny, nz);
    SN_REQUIRE((uint64_t)first + count <= V, "lattice_points: vertices %u .. %llu outside the lattice of %llu", first,
               (unsigned long long)first + count - 1u, (unsigned long long)V);
    hipLaunchKernelGGL(k_lattice_points, dim3(div_up(count, 256)), dim3(256), 0, (hipStream_t)stream, origin[0], origin[1], origin[2], step[0],
                       step[1], step[2], ny, nz, first, count, (int)contract, xyz);
    SN_LAUNCH_CHECK("k_lattice_points");
    return SN_OK;
}

extern "C" size_t sn_rm_isosurface_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    IsoDims d;
    if (!iso_dims(nx, ny, nz, &d)) {
        set_error("isosurface: a lattice of %u x %u x %u is not supported (every dimension >= 2, fewer than 2^31 vertices)", nx, ny, nz);
        return 0;
    }
    return iso_layout(d).bytes;
}

static int iso_check(const char *who, const void *volume, uint32_t nx, uint32_t ny, uint32_t nz, const void *workspace, size_t bytes, IsoDims *d,
                     IsoLayout *l) {
    SN_REQUIRE(volume && workspace, "%s: NULL pointer", who);
    SN_UNSUPPORTED(iso_dims(nx, ny, nz, d), "%s: a lattice of %u x %u x %u is not supported (every dimension >= 2, fewer than 2^31 vertices)", who,
                   nx, ny, nz);
    *l = iso_layout(*d);
    return workspace_check(who, workspace, bytes, l->bytes);
}

extern "C" int sn_rm_isosurface_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *workspace, size_t workspace_bytes,
                                      uint32_t *counts, sn_stream_t stream) {
    IsoDims d;
    IsoLayout l;
    SN_REQUIRE(counts, "isosurface_count: NULL pointer");
    const int rc = iso_check("isosurface_count", volume, nx, ny, nz, workspace, workspace_bytes, &d, &l);
    if (rc != SN_OK) return rc;
    uint8_t *ws = (uint8_t *)workspace;
    uint2 *totals = (uint2 *)(ws + l.totals);
    hipLaunchKernelGGL(k_iso_classify, dim3(div_up(l.nseg, MESH_WAVES)), dim3(256), 0, (hipStream_t)stream, volume, d, iso, ws + l.mask,
                       (uint32_t *)(ws + l.base), totals, l.nseg);
    SN_LAUNCH_CHECK("k_iso_classify");
    hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, totals, l.nseg, counts);
    SN_LAUNCH_CHECK("k_iso_scan");
    return SN_OK;
}

extern "C" int sn_rm_isosurface_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const float *origin, const float *step,
                                     const void *workspace, size_t workspace_bytes, float *vertices, float *normals, int32_t *triangles,
                                     uint32_t cap_v, uint32_t cap_t, sn_stream_t stream) {
    if (cap_v == 0 && cap_t == 0) return SN_OK;          // nothing can be stored
    IsoDims d;
    IsoLayout l;
    SN_REQUIRE(origin && step, "isosurface_emit: NULL pointer");
    SN_REQUIRE((vertices || cap_v == 0) && (triangles || cap_t == 0), "isosurface_emit: NULL output with a non-zero capacity");
    SN_REQUIRE(cap_v <= 0x7fffffffu, "isosurface_emit: cap_v beyond the int32 vertex ids of the triangles");
    const int rc = iso_check("isosurface_emit", volume, nx, ny, nz, workspace, workspace_bytes, &d, &l);
    if (rc != SN_OK) return rc;
    const uint8_t *ws = (const uint8_t *)workspace;
    hipLaunchKernelGGL(k_iso_emit, dim3(div_up(l.nseg, MESH_WAVES)), dim3(256), 0, (hipStream_t)stream, volume, d, iso, origin[0], origin[1],
                       origin[2], step[0], step[1], step[2], ws + l.mask, (const uint32_t *)(ws + l.base), (const uint2 *)(ws + l.totals), l.nseg,
                       vertices, cap_v ? normals : nullptr, triangles, cap_v, cap_t);
    SN_LAUNCH_CHECK("k_iso_emit");
    return SN_OK;
}
