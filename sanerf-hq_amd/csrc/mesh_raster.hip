// mesh_raster.hip — a depth-buffered rasteriser of an indexed triangle mesh for one pinhole camera, exact to the bit
// (sn_rm_mesh_raster_project / _draw / _resolve and _draw_clip / _resolve_clip), for gfx950.
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
// Near-plane clipping (sn_rm_mesh_raster_draw_clip / _resolve_clip) is the CLIP = true instantiation of the last three: a triangle with one
// or two corners behind the plane z = near becomes a polygon of three or four points -- its front corners and the fp64 crossing points of
// the cut edges, whose roles come from the vertices so that a shared edge gives shared bits -- and one or two pieces, each set up as a
// triangle is and keyed by the PARENT's index.  The setup is a function of (triangle, piece) that the three kernels share; the unclipped
// entries launch the CLIP = false instantiations, which take no clip argument and read nothing more than an unclipped rasteriser needs.
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
// c = R^T (v - o) in fp32, every product and sum rounded on its own: the camera frame of the definition.  The projection and the clipped
// kernels call this one function, so a crossing point starts from the bits the vertex's row was made from.
__device__ __forceinline__ void raster_camera(const float (&v)[3], const float *__restrict__ pose, float (&c)[3]) {
    const float d0 = v[0] - pose[3], d1 = v[1] - pose[7], d2 = v[2] - pose[11];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float a = pose[j] * d0, b = pose[4 + j] * d1, e = pose[8 + j] * d2;
        c[j] = (a + b) + e;
    }
}

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
    float c[3];
    raster_camera(v, pose, c);
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

// The setup of three placed points {X, Y, bits(r), .}: a triangle's three rows, or one piece of a clipped triangle.
__device__ __forceinline__ int raster_setup_points(const int4 (&q)[3], int cull, uint32_t H, uint32_t W, RasterTri &s) {
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

__device__ __forceinline__ int raster_setup(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, const int4 *__restrict__ rows,
                                            int cull, uint32_t H, uint32_t W, RasterTri &s) {
    uint32_t c[3];
    if (!triangle_corners(triangles, t, V, c)) return RASTER_DROPPED;
    const int4 q[3] = {rows[c[0]], rows[c[1]], rows[c[2]]};
    if (!(q[0].w & q[1].w & q[2].w & 1)) return RASTER_DROPPED;
    return raster_setup_points(q, cull, H, W, s);
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

// ---- near-plane clipping ----------------------------------------------------------------------------------------------------------------
// What the clipped instantiations read beside the rows: the mesh and the camera, on the device.
struct RasterClip { const float *vertices, *pose, *intr; float near_plane; };
// The same as a kernel argument: nothing at all for the unclipped instantiations.
template <bool CLIP> struct RasterClipArg { __device__ __forceinline__ RasterClip get() const { return RasterClip{nullptr, nullptr, nullptr, 0.0f}; } };
template <> struct RasterClipArg<true> { RasterClip cl; __device__ __forceinline__ RasterClip get() const { return cl; } };

// A point of a clipped triangle's polygon: {X, Y, bits(r)} and where it lies on the parent -- the parent's corner kp itself (kq < 0), or
// the crossing point of the edge from the front corner kp to the behind corner kq, with the weights 1 - s at kp and s at kq.
struct RasterPoint { int32_t x, y, r, kp, kq; double s; };

// What a lane knows of its triangle: the setup and the status of each piece.  Without clipping the triangle is its only piece.
template <bool CLIP> struct RasterParent;
template <> struct RasterParent<false> { RasterTri s[1]; int status[1]; };
template <> struct RasterParent<true> { RasterTri s[2]; int status[2]; RasterPoint pts[4]; bool clipped; };

enum { RASTER_WHOLE = 0, RASTER_GONE = 1, RASTER_CLIPPED = 2 };

// The corner roles and the polygon of triangle t: RASTER_WHOLE (three front corners: the unclipped triangle), RASTER_GONE (a bad index, a bad
// corner, no front corner, or a crossing point outside the guard band) or RASTER_CLIPPED with pts[0 .. 2] or pts[0 .. 3] in the
// triangle's winding (pts[3].kp < 0: three points).  Every array below is indexed by constants once the loops are unrolled.
__device__ __forceinline__ int raster_clip(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, const int4 *__restrict__ rows,
                                           const RasterClip &cl, RasterPoint (&pts)[4]) {
    uint32_t c[3];
    if (!triangle_corners(triangles, t, V, c)) return RASTER_GONE;
    const int4 q[3] = {rows[c[0]], rows[c[1]], rows[c[2]]};
    const bool front[3] = {(q[0].w & 1) != 0, (q[1].w & 1) != 0, (q[2].w & 1) != 0};
    if (front[0] && front[1] && front[2]) return RASTER_WHOLE;
    if (!(front[0] || front[1] || front[2])) return RASTER_GONE;
    const float near_plane = cl.near_plane;
    float cam[3][3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = cl.vertices + (size_t)c[k] * 3u;          // c[k] < V
        const float v[3] = {p[0], p[1], p[2]};
        raster_camera(v, cl.pose, cam[k]);
        const bool finite = fabsf(v[0]) < __builtin_inff() && fabsf(v[1]) < __builtin_inff() && fabsf(v[2]) < __builtin_inff();
        ok = ok && (front[k] || (finite && -cam[k][2] < near_plane));         // front or behind; no NaN is behind
    }
    if (!ok) return RASTER_GONE;
    const double near64 = (double)near_plane, fx = (double)cl.intr[0], fy = (double)cl.intr[1], cx = (double)cl.intr[2], cy = (double)cl.intr[3];
    const int32_t r_near = (int32_t)__float_as_uint(1.0f / near_plane);
    RasterPoint cand[6];
    bool present[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int n = (k + 1) % 3;
        cand[2 * k] = RasterPoint{q[k].x, q[k].y, q[k].z, k, -1, 0.0};
        present[2 * k] = front[k];
        present[2 * k + 1] = front[k] != front[n];
        cand[2 * k + 1] = RasterPoint{0, 0, r_near, 0, 0, 0.0};
        if (present[2 * k + 1]) {
            // the roles come from the vertices, not from the order in the triangle: P is the front end, Q the behind one
            const bool kf = front[k];
            const double xp = (double)(kf ? cam[k][0] : cam[n][0]), yp = (double)(kf ? cam[k][1] : cam[n][1]), zp = (double)-(kf ? cam[k][2] : cam[n][2]);
            const double xq = (double)(kf ? cam[n][0] : cam[k][0]), yq = (double)(kf ? cam[n][1] : cam[k][1]), zq = (double)-(kf ? cam[n][2] : cam[k][2]);
            const double sp = (zp - near64) / (zp - zq);
            const double x = xp + sp * (xq - xp), y = yp + sp * (yq - yp);
            const double px = (fx * x) / near64 + cx, py = -((fy * y) / near64) + cy;
            const double X = rint(256.0 * px), Y = rint(256.0 * py);
            const bool in = fabs(X) <= (double)RASTER_GUARD && fabs(Y) <= (double)RASTER_GUARD;        // no NaN passes
            ok = ok && in;
            cand[2 * k + 1] = RasterPoint{in ? (int32_t)X : 0, in ? (int32_t)Y : 0, r_near, kf ? k : n, kf ? n : k, sp};
        }
    }
    if (!ok) return RASTER_GONE;
    pts[3].kp = -1;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (present[i] && n == j) pts[j] = cand[i];
        n += present[i] ? 1 : 0;
    }
    return RASTER_CLIPPED;
}

// Piece 0 is (p0, p1, p2), piece 1 of a polygon of four points (p0, p2, p3): set up exactly as a triangle is.
__device__ __forceinline__ int raster_setup_piece(const RasterPoint (&pts)[4], int piece, int cull, uint32_t H, uint32_t W, RasterTri &s) {
    const RasterPoint &b = piece ? pts[2] : pts[1], &c = piece ? pts[3] : pts[2];
    const int4 q[3] = {make_int4(pts[0].x, pts[0].y, pts[0].r, 1), make_int4(b.x, b.y, b.r, 1), make_int4(c.x, c.y, c.r, 1)};
    return raster_setup_points(q, cull, H, W, s);
}

// The setup as a function of (triangle, piece), shared by the small, the large and the resolve kernels.  Returns the triangle's status:
// drawn if a piece is drawn, else culled if a piece was culled, else degenerate.  A piece that does not exist has the status -1.
template <bool CLIP>
__device__ __forceinline__ int raster_parent(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, const int4 *__restrict__ rows, int cull,
                                             uint32_t H, uint32_t W, const RasterClip &cl, RasterParent<CLIP> &p) {
    if constexpr (!CLIP) {
        return p.status[0] = raster_setup(triangles, t, V, rows, cull, H, W, p.s[0]);
    } else {
        p.clipped = false;
        p.status[0] = p.status[1] = -1;
        const int kind = raster_clip(triangles, t, V, rows, cl, p.pts);
        if (kind == RASTER_GONE) return RASTER_DROPPED;
        if (kind == RASTER_WHOLE) return p.status[0] = raster_setup(triangles, t, V, rows, cull, H, W, p.s[0]);
        p.clipped = true;
        p.status[0] = raster_setup_piece(p.pts, 0, cull, H, W, p.s[0]);
        if (p.pts[3].kp >= 0) p.status[1] = raster_setup_piece(p.pts, 1, cull, H, W, p.s[1]);
        const bool drawn = p.status[0] == RASTER_DRAWN || p.status[1] == RASTER_DRAWN;
        const bool culled = p.status[0] == RASTER_CULLED || p.status[1] == RASTER_CULLED;
        return drawn ? RASTER_DRAWN : (culled ? RASTER_CULLED : RASTER_DEGENERATE);
    }
}

// ---- draw -----------------------------------------------------------------------------------------------------------------------------------
// One lane walks the clipped bounding box of one piece.
__device__ __forceinline__ void raster_scan_lane(const RasterTri &s, uint32_t t, uint64_t *__restrict__ zbuf, uint32_t W, uint32_t npix) {
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

// The 64 lanes of a wave walk the clipped bounding box of one piece: sw columns x 64 / sw rows per step.
__device__ __forceinline__ void raster_scan_wave(const RasterTri &s, uint32_t t, uint32_t lane, uint64_t *__restrict__ zbuf, uint32_t W, uint32_t npix) {
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

// CLIP: a lane scans its own pieces one after the other; a clipped triangle is queued ONCE if either piece's box exceeds small_max, and
// clip_counts gains the clipped triangles and their drawn pieces.  Without CLIP neither cl nor clip_counts is read.
template <bool CLIP>
__global__ __launch_bounds__(256) void k_raster_small(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, const int4 *__restrict__ rows,
                                                      int cull, uint32_t H, uint32_t W, uint32_t small_max, uint64_t *__restrict__ zbuf,
                                                      uint32_t *__restrict__ queue, uint32_t *__restrict__ head, int32_t *__restrict__ counts,
                                                      RasterClipArg<CLIP> clip, int32_t *__restrict__ clip_counts) {
    SN_POISON_ALL();
    const RasterClip cl = clip.get();
    constexpr int NP = CLIP ? 2 : 1;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = t < T;
    RasterParent<CLIP> p;
    int status = -1;
    if constexpr (CLIP) p.clipped = false;
#pragma unroll
    for (int k = 0; k < NP; ++k) p.status[k] = -1;
    if (live) status = raster_parent<CLIP>(triangles, t, V, rows, cull, H, W, cl, p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {          // every lane of the wave reaches the ballots
        const uint32_t n = (uint32_t)__popcll(__ballot(status == k));
        if (lane == 0u && n) atomicAdd(&counts[k], (int32_t)n);
    }
    if constexpr (CLIP) {
        const uint32_t parents = (uint32_t)__popcll(__ballot(p.clipped));
        const uint32_t pieces = (uint32_t)__popcll(__ballot(p.clipped && p.status[0] == RASTER_DRAWN)) +
                                (uint32_t)__popcll(__ballot(p.clipped && p.status[1] == RASTER_DRAWN));
        if (lane == 0u && parents) { atomicAdd(&clip_counts[0], (int32_t)parents); atomicAdd(&clip_counts[1], (int32_t)pieces); }
    }
    uint32_t area[NP], largest = 0u;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        area[k] = p.status[k] == RASTER_DRAWN ? (uint32_t)p.s[k].nx * (uint32_t)p.s[k].ny : 0u;       // <= 2^26
        largest = area[k] > largest ? area[k] : largest;
    }
    const bool queued = largest > small_max;
    const uint64_t m = __ballot(queued);
    if (m) {                               // wave-uniform
        uint32_t base = 0u;
        if (lane == 0u) base = atomicAdd(&head[0], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0);
        const uint32_t slot = base + lanes_below(m);
        if (queued && slot < T) queue[slot] = t;
    }
    if (largest == 0u || queued) return;
    const uint32_t npix = H * W;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        if (area[k]) raster_scan_lane(p.s[k], t, zbuf, W, npix);
}

template <bool CLIP>
__global__ __launch_bounds__(256) void k_raster_large(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, const int4 *__restrict__ rows,
                                                      int cull, uint32_t H, uint32_t W, uint64_t *__restrict__ zbuf,
                                                      const uint32_t *__restrict__ queue, const uint32_t *__restrict__ head, RasterClipArg<CLIP> clip) {
    SN_POISON_ALL();
    const RasterClip cl = clip.get();
    constexpr int NP = CLIP ? 2 : 1;
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    const uint32_t qlen = umin(head[0], T), npix = H * W;
    for (uint32_t q = wave; q < qlen; q += nwaves) {           // wave-uniform
        const uint32_t t = queue[q];
        RasterParent<CLIP> p;
        if (t >= T || raster_parent<CLIP>(triangles, t, V, rows, cull, H, W, cl, p) != RASTER_DRAWN) continue;
#pragma unroll
        for (int k = 0; k < NP; ++k) {     // the wave walks both pieces of a clipped triangle
            if (p.status[k] != RASTER_DRAWN || p.s[k].nx == 0 || p.s[k].ny == 0) continue;
            raster_scan_wave(p.s[k], t, lane, zbuf, W, npix);
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

__device__ __forceinline__ void raster_empty(const RasterOut &o, uint32_t n) {
    o.triangle_id[n] = -1; o.depth[n] = 0.0f; o.mask[n] = 0u;
    if (o.image) { o.image[(size_t)n * 3u] = o.bg; o.image[(size_t)n * 3u + 1u] = o.bg; o.image[(size_t)n * 3u + 2u] = o.bg; }
    if (o.normal) { o.normal[(size_t)n * 3u] = 0.0f; o.normal[(size_t)n * 3u + 1u] = 0.0f; o.normal[(size_t)n * 3u + 2u] = 0.0f; }
    if (o.label) o.label[n] = 255u;
}

// The weight of the parent's corner i at a point of the polygon.
__device__ __forceinline__ double raster_corner_weight(const RasterPoint &pt, int i) {
    if (pt.kq < 0) return i == pt.kp ? 1.0 : 0.0;
    return i == pt.kp ? 1.0 - pt.s : (i == pt.kq ? pt.s : 0.0);
}

// The attributes of a pixel of triangle t from lambda, the weights of the triangle's own corners.
__device__ __forceinline__ void raster_attributes(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, uint32_t n, const double (&lambda)[3],
                                                  const RasterOut &o) {
    uint32_t c[3];
    triangle_corners(triangles, t, V, c);              // in [0, V): the setup tested them
    if (o.image) raster_blend(o.colors, c, lambda, o.image + (size_t)n * 3u);
    if (o.normal) raster_blend(o.normals, c, lambda, o.normal + (size_t)n * 3u);
    if (o.label) {
        int best = 0;
        if (lambda[1] > lambda[best]) best = 1;
        if (lambda[2] > lambda[best]) best = 2;
        o.label[n] = o.labels[c[best]];
    }
}

template <bool CLIP>
__global__ __launch_bounds__(256) void k_raster_resolve(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V, const int4 *__restrict__ rows,
                                                        uint32_t H, uint32_t W, const uint64_t *__restrict__ zbuf, RasterOut o, RasterClipArg<CLIP> clip) {
    SN_POISON_ALL();
    const RasterClip cl = clip.get();
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= H * W) return;
    const uint64_t key = zbuf[n];
    const uint32_t t = 0xFFFFFFFFu - (uint32_t)key;
    if constexpr (!CLIP) {                 // written out, not through the clipped branch's helpers: with them the compiler lays this path out differently
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
    } else {
        RasterParent<CLIP> p;
        const bool hit = key != 0ull && t < T && raster_parent<CLIP>(triangles, t, V, rows, 0, H, W, cl, p) == RASTER_DRAWN;
        if (!hit) { raster_empty(o, n); return; }
        const int64_t pj = n / W, pi = n - (uint32_t)pj * W;
        // the piece that covers the pixel centre; of two, the one with the larger fp32 rho bits, then the first
        int sel = -1;
        uint32_t best = 0u;
        double pk[3] = {0.0, 0.0, 0.0}, sum = 0.0, rho = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (p.status[k] != RASTER_DRAWN) continue;
            const RasterTri &s = p.s[k];
            const int64_t w[3] = {s.w00[0] + pi * s.sx[0] + pj * s.sy[0], s.w00[1] + pi * s.sx[1] + pj * s.sy[1], s.w00[2] + pi * s.sx[2] + pj * s.sy[2]};
            const bool inside = !p.clipped || ((w[0] + s.bias[0]) >= 0 && (w[1] + s.bias[1]) >= 0 && (w[2] + s.bias[2]) >= 0);
            const double q[3] = {(double)w[0] * (double)s.r[0], (double)w[1] * (double)s.r[1], (double)w[2] * (double)s.r[2]};
            const double qsum = (q[0] + q[1]) + q[2], qrho = qsum / (double)s.A;
            const uint32_t bits = __float_as_uint((float)qrho);
            if (inside && (sel < 0 || bits > best)) { sel = k; best = bits; pk[0] = q[0]; pk[1] = q[1]; pk[2] = q[2]; sum = qsum; rho = qrho; }
        }
        if (sel < 0) { raster_empty(o, n); return; }           // (a depth buffer that no draw of this mesh and camera filled)
        o.triangle_id[n] = (int32_t)t;
        o.depth[n] = (float)(1.0 / rho);
        o.mask[n] = 1u;
        if (!(o.image || o.normal || o.label)) return;
        const double mu[3] = {pk[0] / sum, pk[1] / sum, pk[2] / sum};
        if (!p.clipped) { raster_attributes(triangles, t, V, n, mu, o); return; }
        const RasterPoint pt[3] = {p.pts[0], sel ? p.pts[2] : p.pts[1], sel ? p.pts[3] : p.pts[2]};
        double lambda[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc = acc + mu[k] * raster_corner_weight(pt[k], i);
            lambda[i] = acc;
        }
        raster_attributes(triangles, t, V, n, lambda, o);
    }
}

}  // namespace sn

using namespace sn;

static bool raster_sizes_ok(uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    return mesh_sizes_ok(V, T) && H >= 1u && H <= RASTER_MAX_SIDE && W >= 1u && W <= RASTER_MAX_SIDE;
}

#define RASTER_SIZES_MSG "%s: V = %u, T = %u, H = %u, W = %u is not supported (V, T below 2^31; H, W in [1, 8192])"
#define RASTER_NEAR_OK(who, near_plane) \
    SN_REQUIRE(std::isfinite(near_plane) && near_plane > 0.0f, who ": near = %g must be positive and finite", (double)near_plane)

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
    RASTER_NEAR_OK("mesh_raster_project", near_plane);
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

// The draw and the resolve behind their entries: without clip the launches are the unclipped instantiations, which read nothing of cl.
template <bool CLIP>
static int raster_draw(const char *who, const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, int cull, uint32_t small_max_pixels,
                       void *workspace, size_t workspace_bytes, int32_t *counts, const RasterClipArg<CLIP> &cl, int32_t *clip_counts, sn_stream_t stream) {
    SN_REQUIRE(small_max_pixels < (1u << 31), "%s: small_max_pixels = %u must be below 2^31", who, small_max_pixels);
    RasterLayout l;
    const int rc = raster_check(who, V, T, H, W, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (CLIP) SN_HIP_OK(hipMemsetAsync(clip_counts, 0, 2 * sizeof(int32_t), st));
    if (T == 0) return SN_OK;
    uint8_t *ws = (uint8_t *)workspace;
    const int4 *rows = (const int4 *)(ws + l.rows);
    uint64_t *zbuf = (uint64_t *)(ws + l.zbuf);
    uint32_t *queue = (uint32_t *)(ws + l.queue), *head = (uint32_t *)(ws + l.head);
    hipLaunchKernelGGL(k_raster_small<CLIP>, dim3(div_up(T, 256)), dim3(256), 0, st, triangles, T, V, rows, cull ? 1 : 0, H, W, small_max_pixels, zbuf,
                       queue, head, counts, cl, clip_counts);
    const uint32_t blocks = div_up(T, 4) < RASTER_LARGE_BLOCKS ? div_up(T, 4) : RASTER_LARGE_BLOCKS;      // a function of T only: capturable
    hipLaunchKernelGGL(k_raster_large<CLIP>, dim3(blocks), dim3(256), 0, st, triangles, T, V, rows, cull ? 1 : 0, H, W, zbuf, queue, head, cl);
    SN_LAUNCH_CHECK("k_raster_small, k_raster_large");
    return SN_OK;
}

template <bool CLIP>
static int raster_resolve(const char *who, const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, const float *colors,
                          const float *normals, const uint8_t *labels, float bg_color, const void *workspace, size_t workspace_bytes,
                          int32_t *triangle_id, float *depth, uint8_t *mask, float *image, float *normal, uint8_t *label, const RasterClipArg<CLIP> &cl,
                          sn_stream_t stream) {
    // (an attribute of an empty mesh may be NULL: its image is what asks for it)
    SN_REQUIRE((image ? colors || V == 0 : !colors) && (normal ? normals || V == 0 : !normals) && (label ? labels || V == 0 : !labels),
               "%s: an attribute and its output image come together (colors/image, normals/normal, labels/label)", who);
    RasterLayout l;
    const int rc = raster_check(who, V, T, H, W, workspace, workspace_bytes, &l);
    if (rc != SN_OK) return rc;
    const uint8_t *ws = (const uint8_t *)workspace;
    RasterOut o{triangle_id, depth, mask, colors, normals, labels, image, normal, label, bg_color};
    hipLaunchKernelGGL(k_raster_resolve<CLIP>, dim3(div_up((uint64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, triangles, T, V,
                       (const int4 *)(ws + l.rows), H, W, (const uint64_t *)(ws + l.zbuf), o, cl);
    SN_LAUNCH_CHECK("k_raster_resolve");
    return SN_OK;
}

extern "C" int sn_rm_mesh_raster_draw(const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, int cull,
                                      uint32_t small_max_pixels, void *workspace, size_t workspace_bytes, int32_t *counts, sn_stream_t stream) {
    SN_REQUIRE((triangles || T == 0) && counts, "mesh_raster_draw: NULL pointer");
    return raster_draw<false>("mesh_raster_draw", triangles, V, T, H, W, cull, small_max_pixels, workspace, workspace_bytes, counts, RasterClipArg<false>{}, nullptr,
                              stream);
}

extern "C" int sn_rm_mesh_raster_draw_clip(const float *vertices, const int32_t *triangles, uint32_t V, uint32_t T, const float *pose,
                                           const float *intrinsics, uint32_t H, uint32_t W, float near_plane, int cull, uint32_t small_max_pixels,
                                           void *workspace, size_t workspace_bytes, int32_t *counts, int32_t *clip_counts, sn_stream_t stream) {
    SN_REQUIRE((vertices || V == 0) && (triangles || T == 0) && pose && intrinsics && counts && clip_counts, "mesh_raster_draw_clip: NULL pointer");
    RASTER_NEAR_OK("mesh_raster_draw_clip", near_plane);
    return raster_draw<true>("mesh_raster_draw_clip", triangles, V, T, H, W, cull, small_max_pixels, workspace, workspace_bytes, counts,
                             RasterClipArg<true>{{vertices, pose, intrinsics, near_plane}}, clip_counts, stream);
}

extern "C" int sn_rm_mesh_raster_resolve(const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, const float *colors,
                                         const float *normals, const uint8_t *labels, float bg_color, const void *workspace,
                                         size_t workspace_bytes, int32_t *triangle_id, float *depth, uint8_t *mask, float *image, float *normal,
                                         uint8_t *label, sn_stream_t stream) {
    SN_REQUIRE((triangles || T == 0) && triangle_id && depth && mask, "mesh_raster_resolve: NULL pointer");
    return raster_resolve<false>("mesh_raster_resolve", triangles, V, T, H, W, colors, normals, labels, bg_color, workspace, workspace_bytes, triangle_id,
                                 depth, mask, image, normal, label, RasterClipArg<false>{}, stream);
}

extern "C" int sn_rm_mesh_raster_resolve_clip(const float *vertices, const int32_t *triangles, uint32_t V, uint32_t T, const float *pose,
                                              const float *intrinsics, uint32_t H, uint32_t W, float near_plane, const float *colors,
                                              const float *normals, const uint8_t *labels, float bg_color, const void *workspace,
                                              size_t workspace_bytes, int32_t *triangle_id, float *depth, uint8_t *mask, float *image,
                                              float *normal, uint8_t *label, sn_stream_t stream) {
    SN_REQUIRE((vertices || V == 0) && (triangles || T == 0) && pose && intrinsics && triangle_id && depth && mask,
               "mesh_raster_resolve_clip: NULL pointer");
    RASTER_NEAR_OK("mesh_raster_resolve_clip", near_plane);
    return raster_resolve<true>("mesh_raster_resolve_clip", triangles, V, T, H, W, colors, normals, labels, bg_color, workspace, workspace_bytes,
                                triangle_id, depth, mask, image, normal, label, RasterClipArg<true>{{vertices, pose, intrinsics, near_plane}}, stream);
}
