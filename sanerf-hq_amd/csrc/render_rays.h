// render_rays.h -- fused renderer: the rays of a launch.  Tile orders (workgroup -> wave tile -> pixel), ray set-up, bins -> sample position.
#ifndef SN_RENDER_RAYS_H
#define SN_RENDER_RAYS_H
#include "sn_common.h"
#include <type_traits>

namespace sn {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct RayCommon {
    const float *rays_o, *rays_d, *cnf;
    uint32_t N;        // rays in this launch
    uint32_t W;        // image width (tile mode) or 0
    uint32_t rows;     // image rows in this launch (tile mode)
    uint32_t Npad;     // scratch row stride = gridDim.x * 256
    float aabb[6];
    float min_near, bound;
    int contract, last_opaque;
    float bg;
    int xcd_swizzle;
    uint32_t st_w, st_h;   // wave tiles walked in super-tiles of st_w units x st_h row pairs (wave_tile_of); st_w = 0: in whole row pairs
    uint32_t tlw;      // log2 of the wave tile's width in pixels (3: 8x8; sn_render_tuning.wave_tile)
    float inv_den;     // 1 / (2*bound) when that is a power of two (exact scaling), else 0
};

// Workgroup id -> tile id.  The dispatcher places workgroup b on XCD b % 8 (observed, not contractual: used
// for speed only).  Remapping so that each XCD owns a contiguous range of tile ids keeps neighbouring image
// tiles -- which share fine-level table lines -- behind the same private L2.  Bijective for any grid size.
__host__ __device__ __forceinline__ uint32_t xcd_tile_id(uint32_t b, uint32_t nwg) {
    const uint32_t xcd = b & 7u, q = nwg >> 3, r = nwg & 7u;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (b >> 3);
}
// The eight tile queues of the persistent launch of the last stage (k_final_stage_pt).  Queue x holds the WAVE tiles of the workgroup-tile
// range xcd_tile_id() gives XCD x in a launch of `units` workgroup tiles -- the same contiguous ranges x 4, in the same order: ids
// [begin, end).  xcd = 0 (tile orders without the remap): one queue, number 0, over all ids.  The ranges partition [0, 4 * units).
__host__ __device__ __forceinline__ void tile_queue_range(uint32_t x, uint32_t units, int xcd, uint32_t &begin, uint32_t &end) {
    if (!xcd) { begin = 0u; end = x == 0u ? 4u * units : 0u; return; }
    const uint32_t q = units >> 3, r = units & 7u;
    const uint32_t first = x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q;      // = xcd_tile_id(x, units)
    begin = 4u * first;
    end = 4u * (first + q + (x < r ? 1u : 0u));
}
__device__ __forceinline__ uint32_t tile_id_x(const RayCommon &rc, uint32_t b, uint32_t nwg) { return rc.xcd_swizzle ? xcd_tile_id(b, nwg) : b; }
__device__ __forceinline__ uint32_t tile_id(const RayCommon &rc) { return tile_id_x(rc, blockIdx.x, gridDim.x); }

// Wave-tile id -> wave tile (wx, wy) of an image of tx8 x ty8 wave tiles.  Wave-tile rows go in pairs; a "unit" is one column of a pair
// (two wave tiles, one above the other), so that the four consecutive ids of a workgroup are a 2x2 block wherever the image has one.  An
// odd last wave-tile row comes after all pairs, left to right.
//   sw = 0: the units of a row pair left to right, pair after pair: 64 consecutive workgroups are a strip the width of the image.
//   sw > 0: the units in super-tiles sw units wide and up to sh row pairs high (the row pairs are dealt evenly to ceil(P / sh)
//           super-tile rows).  Super-tile rows alternate direction (odd ones are walked mirrored), a super-tile is row-major inside, edge
//           super-tiles are narrower: a contiguous range of ids -- what one XCD has in flight, xcd_tile_id -- is a connected region a few
//           super-tiles long.  Closed form, evaluated once per lane before the march.  Bijective on the units for every shape.
__host__ __device__ __forceinline__ void wave_tile_of(uint32_t g, uint32_t tx8, uint32_t ty8, uint32_t sw, uint32_t sh, uint32_t &wx, uint32_t &wy) {
    const uint32_t P = ty8 >> 1, pair = 2u * tx8, paired = P * pair;
    if (g >= paired) { wx = g - paired; wy = ty8 & ~1u; return; }          // the odd last row
    if (sw == 0u) { const uint32_t p = g / pair, i = g - p * pair; wx = i >> 1; wy = 2u * p + (i & 1u); return; }
    const uint32_t u = g >> 1;
    const uint32_t nsy = (P + sh - 1u) / sh, base = P / nsy, extra = P - base * nsy;    // the first `extra` super-tile rows are base + 1 high
    const uint32_t big = (base + 1u) * tx8;                                                         // units of such a row
    uint32_t sy, r0, h, y0;
    if (u < extra * big) { sy = u / big; r0 = u - sy * big; h = base + 1u; y0 = sy * h; }
    else { const uint32_t v = u - extra * big, row = base * tx8, s = v / row; r0 = v - s * row; sy = extra + s; h = base; y0 = extra * (base + 1u) + s * base; }
    const uint32_t full = sw * h, sx = r0 / full, r1 = r0 - sx * full;
    const uint32_t left = tx8 - sx * sw, w = left < sw ? left : sw;
    const uint32_t ry = r1 / w, rx = r1 - ry * w;
    const uint32_t x = sx * sw + rx;
    wx = (sy & 1u) ? tx8 - 1u - x : x;
    wy = 2u * (y0 + ry) + (g & 1u);
}

// lane -> ray.  Tile mode: wave = 8x8 pixels; a workgroup takes four CONSECUTIVE wave tiles of this order: wave-tile rows go in
// pairs, column-major inside a pair ((0,0) (0,1) (1,0) (1,1) (2,0) ...; wave_tile_of, which also states the super-tile order), so that a workgroup is a 16x16-pixel block wherever the
// image has one, and an odd last wave-tile row is walked left to right (32x8 pixels per workgroup).  The launch has
// ceil(wave tiles / 4) workgroups whatever the shape -- a 200-row band of a 1600-wide image (BASELINE configs[3] on 8 GPUs) is 1250
// workgroups, not the 1300 of whole 16x16 tiles: tools/staircase.py shows the stages' time stepping at multiples of 256 workgroups
// (one per CU), 1300 is just past the step at 1280 (profiles/r04/staircase_1600.txt).  Host twin: blocks_for().
// (g: the wave tile id, wave-uniform -- four consecutive ones per workgroup of the ordinary launch, one per fetch of the persistent one;
//  linear order: rays g * 64 .. g * 64 + 63)
__device__ __forceinline__ bool ray_of_wave_tile(const RayCommon &rc, uint32_t g, uint32_t lane, uint32_t &n) {
    if (rc.W) {
        // wave tile = 2^tlw x 2^(6 - tlw) pixels (8x8 unless sn_render_tuning.wave_tile says otherwise; tx8 / ty8 keep their round-1 names)
        const uint32_t tlw = rc.tlw, tlh = 6u - tlw, tw = 1u << tlw, th = 1u << tlh;
        const uint32_t tx8 = (rc.W + tw - 1u) >> tlw, ty8 = (rc.rows + th - 1u) >> tlh;
        uint32_t wx, wy;
        wave_tile_of(g, tx8, ty8, rc.st_w, rc.st_h, wx, wy);   // (wx >= tx8: padding of the last workgroup)
        const uint32_t py = (wy << tlh) + (lane >> tlw);
        const uint32_t px = (wx << tlw) + (lane & (tw - 1u));
        const bool ok = wx < tx8 && px < rc.W && py < rc.rows;
        n = ok ? py * rc.W + px : 0u;
        return ok;
    }
    n = g * 64u + lane;
    const bool ok = n < rc.N;
    if (!ok) n = 0;
    return ok;
}
__device__ __forceinline__ bool ray_of_lane(const RayCommon &rc, uint32_t wg, uint32_t &n) {
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (the wave tile is the same for all lanes: scalar arithmetic)
    return ray_of_wave_tile(rc, wg * 4u + wave, tid & 63u, n);
}

struct RaySetup {
    float o[3], d[3];
    float s_near, s_far;
};

__device__ __forceinline__ void setup_ray(const RayCommon &rc, uint32_t n, RaySetup &rs) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { rs.o[k] = rc.rays_o[(size_t)n * 3 + k]; rs.d[k] = rc.rays_d[(size_t)n * 3 + k]; }
    float near, far;
    near_far_one(rs.o, rs.d, rc.aabb, rc.min_near, near, far);
    if (rc.cnf) {  // renderer.py:233-235
        const float cn = rc.cnf[(size_t)n * 2], cf = rc.cnf[(size_t)n * 2 + 1];
        near = cn > near ? cn : near;
        far = cf < far ? cf : far;
    }
    rs.s_near = spacing_fn(near);
    rs.s_far = spacing_fn(far);
}

// renderer.py:277 — normalised bin -> distance along the ray
__device__ __forceinline__ float real_bin(const RaySetup &rs, float b) {
    const float a = rs.s_near * (1.0f - b);
    const float c = rs.s_far * b;
    return spacing_inv(a + c);
}

// renderer.py:279-285 + grid.py:156: sample position -> table coordinate in [0,1]
__device__ __forceinline__ void sample_x01(const RayCommon &rc, const RaySetup &rs, float tmid, float (&p)[3], float (&x01)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float m = rs.d[k] * tmid; p[k] = rs.o[k] + m; }
    if (rc.contract) contract3(p[0], p[1], p[2]);
    const float den = 2.0f * rc.bound;
    if (rc.inv_den != 0.0f) {   // 2*bound is a power of two (bound = 2 when contracted): x / den == x * (1/den) exactly
#pragma unroll
        for (int k = 0; k < 3; ++k) x01[k] = (p[k] + rc.bound) * rc.inv_den;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) x01[k] = (p[k] + rc.bound) / den;
    }
}

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

}  // namespace sn

#endif  // SN_RENDER_RAYS_H
