// mesh_raster.hip — a depth-buffered rasteriser of an indexed triangle mesh for one pinhole camera, exact to the bit
// (sn_rm_mesh_raster_project / _draw / _resolve), for gfx950.
//
// Definition: include/sanerf_hip.h states it in full; tests/mesh_raster_ref.py restates it in numpy.  In short: a vertex is taken into the
// camera frame in fp32 (c = R^T (v - o), z = -c.z), projected with the IEEE division and snapped to integers with 8 sub-pixel bits
// (X, Y in [-2^22, 2^22]); r = 1 / z.  A triangle with three placed corners and a doubled area A != 0 is drawn: its three edge functions
// at a pixel centre are exact int64, the top-left rule decides the pixels on an edge, rho = (w0 r0 + w1 r1 + w2 r2) / A in fp64 is the
// interpolated inverse depth, and a pixel keeps the largest (bits(fp32 rho) << 32 | ~t) -- ONE 64-bit unsigned atomic maximum, whose result
// does not depend on the order in which the triangles arrive.  The resolve recomputes rho and the perspective-correct weights of the
// winner from its vertex rows and interpolates the attributes in fp64.
//
//   k_raster_project  one lane per vertex: the 16-byte row {X, Y, bits(r), placed}; the same launch clears the 64-bit depth buffer, the
//                     queue length and the four counters.
//   k_raster_small    one lane per triangle: classifies it (drawn / dropped / degenerate / culled; one atomic add per wave and counter),
//                     clips its bounding box to the screen, and scans it if it holds at most small_max_pixels pixel centres.  The others
//                     are appended to a queue: ballot + mbcnt rank, one atomic add of the wave's count.  The queue's order depends on the
//                     run; nothing can see it, because the depth buffer is a maximum.
//   k_raster_large    a fixed grid; its waves stride over the queue, whose length is read on the device.  The 64 lanes of a wave share
//                     one triangle and walk its clipped bounding box in steps of 64 / sw rows of sw = min(64, pow2 >= columns) columns:
//                     the atomics of one wave instruction fall into at most 64 / sw runs of contiguous pixels.
//   k_raster_resolve  one lane per pixel.
// The atomics: the 64-bit maximum (global_atomic_umax_x2; no return value is used, no compare-and-swap loop) and integer adds on the
// counters.  Every index read from `triangles`, from the queue or from the depth buffer is range-tested before it is an address.
#include "mesh_common.h"

#include <cmath>

namespace sn {

constexpr uint32_t RASTER_MAX_SIDE = 8192u;    // H, W
constexpr int32_t RASTER_GUARD = 1 << 22;      // |X|, |Y| <= 2^22 (8 sub-pixel bits: 2^14 pixels)
constexpr uint32_t RASTER_LARGE_BLOCKS = 1024u;        // x 4 waves: the fixed grid of k_raster_large

// Parts in order, each rounded up to 16 bytes.  head[0] = the queue's length.
struct RasterLayout { size_t head, rows, zbuf, queue, bytes; };

static inline RasterLayout raster_layout(uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    RasterLayout l;
    l.head = 0;
    l.rows = l.head + 16u;
    l.zbuf = l.rows + (size_t)V * 16u;
    l.queue = l.zbuf + (size_t)H * W * 8u;
    l.bytes = l.queue + align16((size_t)T * 4u);
    return l;
}

// ---- project ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_raster_project(const float *__restrict__ vertices, uint32_t V, const float *__restrict__ pose,
                                                        const float *__restrict__ intr, float near_plane, int4 *__restrict__ rows,
                                                        uint64_t *__restrict__ zbuf, uint32_t npix, uint32_t *__restrict__ head,
                                                        int32_t *__restrict__ counts) {
    SN_POISON_ALL();
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n < npix) zbuf[n] = 0ull;
    if (n < 4u) { counts[n] = 0; head[n] = 0u; }
    if (n >= V) return;
    const float *p = vertices + (size_t)n * 3u;
    const float v[3] = {p[0], p[1], p[2]};
    bool placed = fabsf(v[0]) < __builtin_inff() && fabsf(v[1]) < __builtin_inff() && fabsf(v[2]) < __builtin_inff();
    const float d0 = v[0] - pose[3], d1 = v[1] - pose[7], d2 = v[2] - pose[11];
    float c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float a = pose[j] * d0, b = pose[4 + j] * d1, e = pose[8 + j] * d2;
        c[j] = (a + b) + e;
    }
    const float z = -c[2];
    placed = placed && z >= near_plane;
    const float r = 1.0f / z;
    placed = placed && fabsf(r) < __builtin_inff();
    const float qx = (intr[0] * c[0]) / z, qy = (intr[1] * c[1]) / z;
    const float x = qx + intr[2], y = -qy + intr[3];
    const float fx = rintf(256.0f * x), fy = rintf(256.0f * y);
    placed = placed && fabsf(fx) <= (float)RASTER_GUARD && fabsf(fy) <= (float)RASTER_GUARD;    // no NaN passes
    rows[n] = placed ? make_int4((int32_t)fx, (int32_t)fy, (int32_t)__float_as_uint(r), 1) : make_int4(0, 0, 0, 0);
}

// ---- the triangle -------------------------------------------------------------------------------------------------------------------------
enum { RASTER_DRAWN = 0, RASTER_DROPPED = 1, RASTER_DEGENERATE = 2, RASTER_CULLED = 3 };

// Edge k runs from corner k + 1 to corner k + 2 and is opposite corner k; oriented so that A > 0 and the inside has w_k > 0.
// w_k at the centre of pixel (i, j) = w00[k] + i sx[k] + j sy[k]; covered iff every w_k + bias[k] >= 0 (bias 0 on a top or left edge, else -1).
struct RasterTri {
    int64_t A, w00[3], sx[3], sy[3];
    int32_t bias[3];
    float r[3];
    int32_t i0, j0, nx, ny;            // the pixel centres inside the bounding box, clipped to the screen: nx x ny of them from (i0, j0)
};

__device__ __forceinline__ int raster_setup(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, const int4 *__restrict__ rows,
                                            int cull, uint32_t H, uint32_t W, RasterTri &s) {
    uint32_t c[3];
    if (!triangle_corners(triangles, t, V, c)) return RASTER_DROPPED;
    const int4 q[3] = {rows[c[0]], rows[c[1]], rows[c[2]]};
    if (!(q[0].w & q[1].w & q[2].w & 1)) return RASTER_DROPPED;
    const int64_t A = (int64_t)(q[1].x - q[0].x) * (int64_t)(q[2].y - q[0].y) - (int64_t)(q[1].y - q[0].y) * (int64_t)(q[2].x - q[0].x);
    if (A == 0) return RASTER_DEGENERATE;
    if (cull && A > 0) return RASTER_CULLED;           // front faces have A < 0 on a screen whose y points down
    const int64_t sg = A < 0 ? -1 : 1;
    s.A = sg * A;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int4 &p = q[(k + 1) % 3], &n = q[(k + 2) % 3];
        const int64_t dx = sg * (int64_t)(n.x - p.x), dy = sg * (int64_t)(n.y - p.y);
        s.w00[k] = dx * (int64_t)(128 - p.y) - dy * (int64_t)(128 - p.x);
        s.sx[k] = -256 * dy;
        s.sy[k] = 256 * dx;
        s.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
        s.r[k] = __uint_as_float((uint32_t)q[k].z);
    }
    const int32_t xmin = min(q[0].x, min(q[1].x, q[2].x)), xmax = max(q[0].x, max(q[1].x, q[2].x));
    const int32_t ymin = min(q[0].y, min(q[1].y, q[2].y)), ymax = max(q[0].y, max(q[1].y, q[2].y));
    // centres 256 i + 128 in [min, max]: i from ceil((min - 128) / 256) to floor((max - 128) / 256); >> is the floor
    const int32_t i0 = max((xmin + 127) >> 8, 0), i1 = min((xmax - 128) >> 8, (int32_t)W - 1);
    const int32_t j0 = max((ymin + 127) >> 8, 0), j1 = min((ymax - 128) >> 8, (int32_t)H - 1);
    s.i0 = i0; s.j0 = j0;
    s.nx = i1 >= i0 ? i1 - i0 + 1 : 0;
    s.ny = j1 >= j0 ? j1 - j0 + 1 : 0;
    return RASTER_DRAWN;
}

__device__ __forceinline__ double raster_rho(const RasterTri &s, int64_t w0, int64_t w1, int64_t w2) {
    const double p0 = (double)w0 * (double)s.r[0], p1 = (double)w1 * (double)s.r[1], p2 = (double)w2 * (double)s.r[2];
    return ((p0 + p1) + p2) / (double)s.A;
}

__device__ __forceinline__ void raster_sample(const RasterTri &s, int64_t w0, int64_t w1, int64_t w2, uint32_t t, uint64_t *__restrict__ zbuf,
                                              uint32_t pixel, uint32_t npix) {
    if ((w0 + s.bias[0]) < 0 || (w1 + s.bias[1]) < 0 || (w2 + s.bias[2]) < 0) return;
    const float key = (float)raster_rho(s, w0, w1, w2);
    if (pixel < npix) atomicMax((unsigned long long *)(zbuf + pixel), ((unsigned long long)__float_as_uint(key) << 32) | (0xFFFFFFFFu - t));
}

// ---- draw -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_raster_small(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, const int4 *__restrict__ rows,
                                                      int cull, uint32_t H, uint32_t W, uint32_t small_max, uint64_t *__restrict__ zbuf,
                                                      uint32_t *__restrict__ queue, uint32_t *__restrict__ head, int32_t *__restrict__ counts) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = t < T;
    RasterTri s;
    int status = -1;
    if (live) status = raster_setup(triangles, t, V, rows, cull, H, W, s);
#pragma unroll
    for (int k = 0; k < 4; ++k) {          // every lane of the wave reaches the ballots
        const uint32_t n = (uint32_t)__popcll(__ballot(status == k));
        if (lane == 0u && n) atomicAdd(&counts[k], (int32_t)n);
    }
    const uint32_t area = status == RASTER_DRAWN ? (uint32_t)s.nx * (uint32_t)s.ny : 0u;       // <= 2^26
    const bool queued = area > small_max;
    const uint64_t m = __ballot(queued);
    if (m) {                               // wave-uniform
        uint32_t base = 0u;
        if (lane == 0u) base = atomicAdd(&head[0], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0);
        const uint32_t slot = base + lanes_below(m);
        if (queued && slot < T) queue[slot] = t;
    }
    if (area == 0u || queued) return;
    const uint32_t npix = H * W;
    int64_t r0 = s.w00[0] + s.i0 * s.sx[0] + s.j0 * s.sy[0];
    int64_t r1 = s.w00[1] + s.i0 * s.sx[1] + s.j0 * s.sy[1];
    int64_t r2 = s.w00[2] + s.i0 * s.sx[2] + s.j0 * s.sy[2];
    for (int32_t j = 0; j < s.ny; ++j) {
        int64_t w0 = r0, w1 = r1, w2 = r2;
        const uint32_t row = (uint32_t)(s.j0 + j) * W + (uint32_t)s.i0;
        for (int32_t i = 0; i < s.nx; ++i) {
            raster_sample(s, w0, w1, w2, t, zbuf, row + (uint32_t)i, npix);
            w0 += s.sx[0]; w1 += s.sx[1]; w2 += s.sx[2];
        }
        r0 += s.sy[0]; r1 += s.sy[1]; r2 += s.sy[2];
    }
}

__global__ __launch_bounds__(256) void k_raster_large(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, const int4 *__restrict__ rows,
                                                      int cull, uint32_t H, uint32_t W, uint64_t *__restrict__ zbuf,
                                                      const uint32_t *__restrict__ queue, const uint32_t *__restrict__ head) {
    SN_POISON_ALL();
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    const uint32_t qlen = umin(head[0], T), npix = H * W;
    for (uint32_t q = wave; q < qlen; q += nwaves) {           // wave-uniform
        const uint32_t t = queue[q];
        RasterTri s;
        if (t >= T || raster_setup(triangles, t, V, rows, cull, H, W, s) != RASTER_DRAWN) continue;
        if (s.nx == 0 || s.ny == 0) continue;
        // sw columns x 64 / sw rows per step
        uint32_t lg = 0u;
        while (lg < 6u && (1u << lg) < (uint32_t)s.nx) ++lg;
        const int32_t sw = 1 << lg, sh = 64 >> lg;
        const int32_t li = (int32_t)(lane & (uint32_t)(sw - 1)), lj = (int32_t)(lane >> lg);
        for (int32_t jb = 0; jb < s.ny; jb += sh) {
            const int32_t j = jb + lj;
            for (int32_t ib = 0; ib < s.nx; ib += sw) {
                const int32_t i = ib + li;
                if (i >= s.nx || j >= s.ny) continue;
                const int64_t pi = s.i0 + i, pj = s.j0 + j;
                raster_sample(s, s.w00[0] + pi * s.sx[0] + pj * s.sy[0], s.w00[1] + pi * s.sx[1] + pj * s.sy[1],
                              s.w00[2] + pi * s.sx[2] + pj * s.sy[2], t, zbuf, (uint32_t)pj * W + (uint32_t)pi, npix);
            }
        }
    }
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------------------
struct RasterOut {
    int32_t *triangle_id;
    float *depth;
    uint8_t *mask;
    const float *colors, *normals;
    const uint8_t *labels;
    float *image, *normal;
    uint8_t *label;
    float bg;
};

__device__ __forceinline__ void raster_blend(const float *__restrict__ attr, const uint32_t (&c)[3], const double (&mu)[3], float *__restrict__ out) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double t0 = mu[0] * (double)attr[(size_t)c[0] * 3u + ch], t1 = mu[1] * (double)attr[(size_t)c[1] * 3u + ch],
                     t2 = mu[2] * (double)attr[(size_t)c[2] * 3u + ch];
        out[ch] = (float)((t0 + t1) + t2);
    }
}

__global__ __launch_bounds__(256) void k_raster_resolve(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, const int4 *__restrict__ rows,
                                                        uint32_t H, uint32_t W, const uint64_t *__restrict__ zbuf, RasterOut o) {
    SN_POISON_ALL();
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= H * W) return;
    const uint64_t key = zbuf[n];
    const uint32_t t = 0xFFFFFFFFu - (uint32_t)key;
    RasterTri s;
    const bool hit = key != 0ull && t < T && raster_setup(triangles, t, V, rows, 0, H, W, s) == RASTER_DRAWN;
    if (!hit) {
        o.triangle_id[n] = -1; o.depth[n] = 0.0f; o.mask[n] = 0u;
        if (o.image) { o.image[(size_t)n * 3u] = o.bg; o.image[(size_t)n * 3u + 1u] = o.bg; o.image[(size_t)n * 3u + 2u] = o.bg; }
        if (o.normal) { o.normal[(size_t)n * 3u] = 0.0f; o.normal[(size_t)n * 3u + 1u] = 0.0f; o.normal[(size_t)n * 3u + 2u] = 0.0f; }
        if (o.label) o.label[n] = 255u;
        return;
    }
    const int64_t pj = n / W, pi = n - (uint32_t)pj * W;
    const int64_t w[3] = {s.w00[0] + pi * s.sx[0] + pj * s.sy[0], s.w00[1] + pi * s.sx[1] + pj * s.sy[1], s.w00[2] + pi * s.sx[2] + pj * s.sy[2]};
    const double p[3] = {(double)w[0] * (double)s.r[0], (double)w[1] * (double)s.r[1], (double)w[2] * (double)s.r[2]};
    const double sum = (p[0] + p[1]) + p[2];
    const double rho = sum / (double)s.A;
    o.triangle_id[n] = (int32_t)t;
    o.depth[n] = (float)(1.0 / rho);
    o.mask[n] = 1u;
    if (!(o.image || o.normal || o.label)) return;
    const double mu[3] = {p[0] / sum, p[1] / sum, p[2] / sum};
    uint32_t c[3];
    triangle_corners(triangles, t, V, c);              // in [0, V): the setup tested them
    if (o.image) raster_blend(o.colors, c, mu, o.image + (size_t)n * 3u);
    if (o.normal) raster_blend(o.normals, c, mu, o.normal + (size_t)n * 3u);
    if (o.label) {
        int best = 0;
        if (mu[1] > mu[best]) best = 1;
        if (mu[2] > mu[best]) best = 2;
        o.label[n] = o.labels[c[best]];
    }
}

}  // namespace sn

using namespace sn;

static bool raster_sizes_ok(uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    return mesh_sizes_ok(V, T) && H >= 1u && H <= RASTER_MAX_SIDE && W >= 1u && W <= RASTER_MAX_SIDE;
}

#define RASTER_SIZES_MSG "%s: V = %u, T = %u, H = %u, W = %u is not supported (V, T below 2^31; H, W in [1, 8192])"

extern "C" size_t sn_rm_mesh_raster_workspace_bytes(uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    if (!raster_sizes_ok(V, T, H, W)) {
        set_error(RASTER_SIZES_MSG, "mesh_raster", V, T, H, W);
        return 0;
    }
    return raster_layout(V, T, H, W).bytes;
}

// The checks the three entries share; fills the layout.
static int raster_check(const char *who, uint32_t V, uint32_t T, uint32_t H, uint32_t W, const void *workspace, size_t bytes, RasterLayout *l) {
    SN_REQUIRE(workspace, "%s: NULL pointer", who);
    SN_UNSUPPORTED(raster_sizes_ok(V, T, H, W), RASTER_SIZES_MSG, who, V, T, H, W);
    *l = raster_layout(V, T, H, W);
    return workspace_check(who, workspace, bytes, l->bytes);
}

extern "C" int sn_rm_mesh_raster_project(const float *vertices, uint32_t V, uint32_t T, const float *pose, const float *intrinsics, uint32_t H,
                                         uint32_t W, float near_plane, void *workspace, size_t workspace_bytes, int32_t *counts,
                                         sn_stream_t stream) {
    SN_REQUIRE((vertices || V == 0) && pose && intrinsics && counts, "mesh_raster_project: NULL pointer");
    SN_REQUIRE(std::isfinite(near_plane) && near_plane > 0.0f, "mesh_raster_project: near = %g must be positive and finite", (double)near_plane);
    RasterLayout l;
    const int rc = raster_check("mesh_raster_project", V, T, H, W, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    uint8_t *ws = (uint8_t *)workspace;
    const uint32_t npix = H * W, n = V > npix ? V : npix;      // npix >= 1: the counters and the head are cleared by lanes 0 .. 3 of workgroup 0
    hipLaunchKernelGGL(k_raster_project, dim3(div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, vertices, V, pose, intrinsics, near_plane,
                       (int4 *)(ws + l.rows), (uint64_t *)(ws + l.zbuf), npix, (uint32_t *)(ws + l.head), counts);
    SN_LAUNCH_CHECK("k_raster_project");
    return SN_OK;
}

extern "C" int sn_rm_mesh_raster_draw(const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, int cull,
                                      uint32_t small_max_pixels, void *workspace, size_t workspace_bytes, int32_t *counts, sn_stream_t stream) {
    SN_REQUIRE((triangles || T == 0) && counts, "mesh_raster_draw: NULL pointer");
    SN_REQUIRE(small_max_pixels < (1u << 31), "mesh_raster_draw: small_max_pixels = %u must be below 2^31", small_max_pixels);
    RasterLayout l;
    const int rc = raster_check("mesh_raster_draw", V, T, H, W, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    if (T == 0) return SN_OK;
    uint8_t *ws = (uint8_t *)workspace;
    const int4 *rows = (const int4 *)(ws + l.rows);
    uint64_t *zbuf = (uint64_t *)(ws + l.zbuf);
    uint32_t *queue = (uint32_t *)(ws + l.queue), *head = (uint32_t *)(ws + l.head);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_raster_small, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, rows, cull ? 1 : 0, H, W, small_max_pixels, zbuf, queue,
                       head, counts);
    const uint32_t blocks = div_up(T, 4) < RASTER_LARGE_BLOCKS ? div_up(T, 4) : RASTER_LARGE_BLOCKS;      // a function of T only: capturable
    hipLaunchKernelGGL(k_raster_large, dim3(blocks), dim3(256), 0, st, triangles, T, V, rows, cull ? 1 : 0, H, W, zbuf, queue, head);
    SN_LAUNCH_CHECK("k_raster_small, k_raster_large");
    return SN_OK;
}

extern "C" int sn_rm_mesh_raster_resolve(const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, const float *colors,
                                         const float *normals, const uint8_t *labels, float bg_color, const void *workspace,
                                         size_t workspace_bytes, int32_t *triangle_id, float *depth, uint8_t *mask, float *image, float *normal,
                                         uint8_t *label, sn_stream_t stream) {
    SN_REQUIRE((triangles || T == 0) && triangle_id && depth && mask, "mesh_raster_resolve: NULL pointer");
    // (an attribute of an empty mesh may be NULL: its image is what asks for it)
    SN_REQUIRE((image ? colors || V == 0 : !colors) && (normal ? normals || V == 0 : !normals) && (label ? labels || V == 0 : !labels),
               "mesh_raster_resolve: an attribute and its output image come together (colors/image, normals/normal, labels/label)");
    RasterLayout l;
    const int rc = raster_check("mesh_raster_resolve", V, T, H, W, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    const uint8_t *ws = (const uint8_t *)workspace;
    RasterOut o{triangle_id, depth, mask, colors, normals, labels, image, normal, label, bg_color};
    hipLaunchKernelGGL(k_raster_resolve, dim3(div_up((uint64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, triangles, T, V,
                       (const int4 *)(ws + l.rows), H, W, (const uint64_t *)(ws + l.zbuf), o);
    SN_LAUNCH_CHECK("k_raster_resolve");
    return SN_OK;
}
