// prompts.hip — the propagation of 3D point prompts across views and the decode overlays, for gfx950: what the reference does between a
// click and the SAM decoder's prompt, and between the decoder's masks and the picture a user sees.
//   sn_rm_points_lift          test_step's "remember new point_3d" (nerf/trainer.py:803-809): clicked pixel -> o + d * depth
//   sn_rm_point_store_update   the add-or-remove rule of the remembered points (trainer.py:812-834) on a fixed-capacity device store
//   sn_rm_points_project       world -> camera -> pixel, screen test, depth test, the two boolean compactions, the SAM-frame round trip
//                              of the coordinates and decode_step's validity rule (trainer.py:838-875, 931-976) -- one wave per view
//   sn_rm_prompt_overlay       decode_step's score selection, overlay_mask and overlay_point (trainer.py:979-991, 881-884,
//                              nerf/utils.py:23-29, 80-98) and the 8-bit image -- one launch over the image
//
// Conventions of mask_output.hip: division is IEEE-rounded, nothing is contracted into an fma, no atomics, every output has one writer:
// two runs give the same bits.  Counts, labels, flags and coordinates are int32 on the device; nothing is read on the host.
//
// Compaction (sn_rm_points_project): a wave owns a view and walks the points in chunks of 64, one point per lane.  The lanes that keep
// their point are ranked by the prefix count of the wave's ballot (mbcnt) above a running base, the slot dealing of render.hip: the kept
// points leave in their original order, without LDS and without atomics.  The view's 3 x 4 inverse is wave-uniform fp64 arithmetic.
// Overlay: a workgroup owns 256 consecutive pixels.  It stages the count's points as clipped rectangles in LDS (two dwords a point) and
// every pixel scans them from the last to the first: the reads are wave-uniform (one address: a broadcast, no bank conflict), the first
// hit is the reference's last writer.  The colours leave through LDS as whole dwords like sn_rm_mask_output's.
#include "sn_common.h"

namespace sn {

constexpr uint32_t PP_MAX = SN_PROMPT_MAX_POINTS;
constexpr uint32_t PP_TILE = 256;
constexpr uint32_t PP_MAX_EXTENT = 32767;           // overlay: a rectangle bound fits 15 bits

// ---- lift ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_points_lift(const int32_t *__restrict__ pixels, uint32_t M, const float *__restrict__ rays_o,
                                                    const float *__restrict__ rays_d, const float *__restrict__ depth, uint32_t depth_stride,
                                                    uint32_t H, uint32_t W, float *__restrict__ point_3d) {
    const uint32_t m = blockIdx.x * 64u + threadIdx.x;
    if (m >= M) return;
    const int32_t x = pixels[2 * m], y = pixels[2 * m + 1];
    float p[3];
    if (x < 0 || y < 0 || (uint32_t)x >= W || (uint32_t)y >= H) {
        p[0] = p[1] = p[2] = __builtin_nanf("");     // a click outside the image: nothing is read
    } else {
        const size_t n = (size_t)y * W + (uint32_t)x;
        const float t = depth[n * depth_stride];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float s = rays_d[n * 3 + j] * t;
            p[j] = rays_o[n * 3 + j] + s;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) point_3d[3 * m + j] = p[j];
}

// ---- store update -------------------------------------------------------------------------------------------------------------------
// One workgroup of cap <= 1024 threads rounded up to whole waves, one stored point per thread.
__global__ __launch_bounds__(1024) void k_point_store_update(float *__restrict__ xyz, int32_t *__restrict__ labels, int32_t *__restrict__ crucial,
                                                             int32_t *__restrict__ count, uint32_t cap, const float *__restrict__ point,
                                                             const int32_t *__restrict__ label, float dist_thresh, int32_t *__restrict__ status) {
    SN_POISON_ALL();
    __shared__ uint32_t s_wave[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = blockDim.x >> 6;
    const int32_t c0 = *count;
    const uint32_t n = c0 < 0 ? 0u : umin((uint32_t)c0, cap);
    const float q[3] = {point[0], point[1], point[2]};
    const bool mine = tid < n;
    float v[3] = {0.0f, 0.0f, 0.0f};
    int32_t lb = 0, cr = 0;
    bool far = false;
    if (mine) {
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            v[j] = xyz[3 * tid + j];
            const float d = v[j] - q[j];
            s = s + d * d;
        }
        lb = labels[tid]; cr = crucial[tid];
        far = sqrtf(s) > dist_thresh;                // a NaN distance is not far: the point is removed, as the reference's mask does
    }
    const uint64_t kept = __ballot(mine && far);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(kept);
    __syncthreads();                                 // every thread has read its entry: the store may be rewritten
    uint32_t base = 0, total = 0;
    for (uint32_t w = 0; w < waves; ++w) {
        const uint32_t c = s_wave[w];
        base += w < wave ? c : 0u;
        total += c;
    }
    if (total == n) {                                // no stored point within the threshold (or an empty store): append
        if (n == cap) {
            if (tid == 0) { status[0] = 3; status[1] = (int32_t)n; status[2] = (int32_t)n; status[3] = 1; }
            return;
        }
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) xyz[3 * n + j] = q[j];
            labels[n] = *label; crucial[n] = 0;
            *count = (int32_t)(n + 1u);
            status[0] = n == 0u ? 0 : 1; status[1] = (int32_t)n; status[2] = (int32_t)(n + 1u);
        }
        return;
    }
    if (mine && far) {                               // remove every point within the threshold, the others keep their order
        const uint32_t dst = base + rank;
#pragma unroll
        for (int j = 0; j < 3; ++j) xyz[3 * dst + j] = v[j];
        labels[dst] = lb; crucial[dst] = cr;
    }
    if (tid == 0) { *count = (int32_t)total; status[0] = 2; status[1] = (int32_t)n; status[2] = (int32_t)total; }
}

// ---- project ------------------------------------------------------------------------------------------------------------------------
struct ProjectArgs {
    const float *points; const int32_t *labels, *crucial, *n_points;
    const float *poses, *intrinsics, *depth;
    uint32_t N, V, n_intr, depth_stride, H, W;
    float depth_tol, ratio_f;
    double ratio;
    int32_t crucial_count, valid_threshold;
    int32_t *coords, *labels_out, *kept_index, *sam_coords, *overlay_coords;
    float *cam, *uv;
    int32_t *state, *counts;
};

__global__ __launch_bounds__(64) void k_points_project(const ProjectArgs a) {
    const uint32_t v = blockIdx.x, lane = threadIdx.x;
    const int32_t np = a.n_points ? *a.n_points : (int32_t)a.N;
    const uint32_t n = np < 0 ? 0u : umin((uint32_t)np, a.N);
    // world -> camera: the inverse of the affine cam2world [R t] is [R^-1, -R^-1 t], R^-1 = adj(R) / det(R), in fp64 (wave-uniform)
    const float *P = a.poses + (size_t)v * 16;
    double R[3][3], t[3], Wm[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = (double)P[4 * i + j];
        t[i] = (double)P[4 * i + 3];
    }
    const double c00 = R[1][1] * R[2][2] - R[1][2] * R[2][1], c01 = R[1][2] * R[2][0] - R[1][0] * R[2][2], c02 = R[1][0] * R[2][1] - R[1][1] * R[2][0];
    const double det = R[0][0] * c00 + R[0][1] * c01 + R[0][2] * c02;
    const double adj[3][3] = {{c00, R[0][2] * R[2][1] - R[0][1] * R[2][2], R[0][1] * R[1][2] - R[0][2] * R[1][1]},
                              {c01, R[0][0] * R[2][2] - R[0][2] * R[2][0], R[0][2] * R[1][0] - R[0][0] * R[1][2]},
                              {c02, R[0][1] * R[2][0] - R[0][0] * R[2][1], R[0][0] * R[1][1] - R[0][1] * R[1][0]}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Wm[i][j] = adj[i][j] / det;
        Wm[i][3] = -(Wm[i][0] * t[0] + Wm[i][1] * t[1] + Wm[i][2] * t[2]);
    }
    const float *K = a.intrinsics + (a.n_intr > 1u ? (size_t)v * 4 : 0);
    const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const float Wf = (float)a.W, Hf = (float)a.H;
    const float *dimg = a.depth + (size_t)v * a.H * a.W * a.depth_stride;
    const size_t row = (size_t)v * a.N;

    uint32_t base = 0, n_on = 0, n_crucial = 0;
    for (uint32_t i0 = 0; i0 < a.N; i0 += 64u) {      // whole chunks: every lane reaches the ballots
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        float cam[3] = {0.0f, 0.0f, 0.0f}, px = 0.0f, py = 0.0f;
        int32_t ix = 0, iy = 0, st = 0;
        if (live) {
            const double x = (double)a.points[3 * i], y = (double)a.points[3 * i + 1], z = (double)a.points[3 * i + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k) cam[k] = (float)(Wm[k][0] * x + Wm[k][1] * y + Wm[k][2] * z + Wm[k][3]);
            // trainer.py:846-849 in the reference's order: W - (fx * x / z + cx), fy * y / z + cy
            const float qx = (fx * cam[0]) / cam[2], qy = (fy * cam[1]) / cam[2];
            px = Wf - (qx + cx);
            py = qy + cy;
            // .long() truncates toward zero: (-1, 0) lands on pixel 0.  Tested in float: no integer overflow, a NaN fails every comparison
            const bool on = px > -1.0f && px < Wf && py > -1.0f && py < Hf;
            if (on) {
                ix = (int32_t)px; iy = (int32_t)py;
                const float seen = dimg[((size_t)iy * a.W + (uint32_t)ix) * a.depth_stride];
                st = fabsf((-cam[2]) - seen) <= a.depth_tol ? 2 : 1;
            }
        }
        const bool keep = st == 2;
        const uint64_t m_keep = __ballot(keep);
        n_on += (uint32_t)__popcll(__ballot(st >= 1));
        n_crucial += (uint32_t)__popcll(__ballot(keep && a.crucial && a.crucial[i] != 0));
        if (keep) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m_keep >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_keep, 0u));
            const size_t dst = row + base + rank;
            a.coords[2 * dst] = ix; a.coords[2 * dst + 1] = iy;
            a.labels_out[dst] = a.labels[i];
            a.kept_index[dst] = (int32_t)i;
            if (a.sam_coords) {
                // (c.astype(float32) * r).astype(int32), then (pc / r).astype(int32): an fp32 product, an fp64 quotient, both truncated
                const int32_t sx = (int32_t)((float)ix * a.ratio_f), sy = (int32_t)((float)iy * a.ratio_f);
                a.sam_coords[2 * dst] = sx; a.sam_coords[2 * dst + 1] = sy;
                a.overlay_coords[2 * dst] = (int32_t)((double)sx / a.ratio); a.overlay_coords[2 * dst + 1] = (int32_t)((double)sy / a.ratio);
            }
        }
        base += (uint32_t)__popcll(m_keep);
        if (i < a.N) {
            if (a.cam) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.cam[3 * (row + i) + k] = cam[k];
            }
            if (a.uv) { a.uv[2 * (row + i)] = px; a.uv[2 * (row + i) + 1] = py; }
            if (a.state) a.state[row + i] = st;
        }
    }
    for (uint32_t j = base + lane; j < a.N; j += 64u) {      // the tail: SAM's padding label, a fixed-shape prompt needs no count
        const size_t dst = row + j;
        a.coords[2 * dst] = 0; a.coords[2 * dst + 1] = 0;
        a.labels_out[dst] = -1;
        a.kept_index[dst] = -1;
        if (a.sam_coords) {
            a.sam_coords[2 * dst] = 0; a.sam_coords[2 * dst + 1] = 0;
            a.overlay_coords[2 * dst] = 0; a.overlay_coords[2 * dst + 1] = 0;
        }
    }
    if (lane < 4u) {
        const bool valid = base > 0u && (int64_t)n_crucial >= (int64_t)a.crucial_count && (int64_t)base >= (int64_t)a.valid_threshold;   // trainer.py:969-971
        a.counts[4 * v + lane] = lane == 0u ? (int32_t)n_on : lane == 1u ? (int32_t)base : lane == 2u ? (int32_t)n_crucial : (int32_t)valid;
    }
}

// ---- overlay ------------------------------------------------------------------------------------------------------------------------
// Python's slice [c - r : c + r] on an axis of `len` entries: a negative bound counts from the end, then both are clamped to [0, len].
__device__ __forceinline__ void py_slice(int32_t c, int32_t r, int32_t len, uint32_t &start, uint32_t &stop) {
    long long s = (long long)c - r, e = (long long)c + r;
    if (s < 0) s += len;
    if (e < 0) e += len;
    s = s < 0 ? 0 : s > len ? len : s;
    e = e < 0 ? 0 : e > len ? len : e;
    start = (uint32_t)s; stop = (uint32_t)e;
}

struct OverlayArgs {
    const float *image; const uint8_t *masks; const float *scores;
    const int32_t *coords, *labels, *count;
    uint32_t image_stride, H, W, M, N;
    int32_t mask_index, radius;
    float a, b;
    float *rgb; uint8_t *rgb8, *pred_mask; int32_t *selected;
};

__global__ __launch_bounds__(256) void k_prompt_overlay(const OverlayArgs a) {
    SN_POISON_ALL();
    __shared__ uint32_t s_rx[PP_MAX], s_ry[PP_MAX];              // x0 | x1 << 16;  y0 | y1 << 16 | (label != 0) << 31
    __shared__ float s_rgb[PP_TILE * 3];
    __shared__ uint32_t s_rgb8[PP_TILE * 3 / 4];
    __shared__ int32_t s_sel;
    const uint32_t tid = threadIdx.x, P = a.H * a.W, n0 = blockIdx.x * PP_TILE, cnt = umin(PP_TILE, P - n0), n = n0 + tid;
    const bool active = tid < cnt;
    const int32_t c0 = a.count ? *a.count : (int32_t)a.N;
    const uint32_t np = c0 < 0 ? 0u : umin((uint32_t)c0, a.N);
    for (uint32_t i = tid; i < np; i += PP_TILE) {
        uint32_t x0, x1, y0, y1;
        py_slice(a.coords[2 * i], a.radius, (int32_t)a.W, x0, x1);
        py_slice(a.coords[2 * i + 1], a.radius, (int32_t)a.H, y0, y1);
        if (x0 >= x1 || y0 >= y1) x0 = x1 = y0 = y1 = 0u;
        s_rx[i] = x0 | (x1 << 16);
        s_ry[i] = y0 | (y1 << 16) | (a.labels[i] != 0 ? 0x80000000u : 0u);
    }
    if (tid == 0) {
        int32_t sel = a.mask_index;
        if (a.masks && a.scores) {                   // trainer.py:979-984: the first score above the running maximum, which starts at 0
            float best = 0.0f;
            sel = 0;
            for (uint32_t j = 0; j < a.M; ++j) {
                const float s = a.scores[j];
                if (s > best) { best = s; sel = (int32_t)j; }
            }
        }
        s_sel = np == 0u || !a.masks ? -1 : sel;
        if (blockIdx.x == 0) *a.selected = np == 0u ? -1 : a.masks ? sel : -1;
    }
    __syncthreads();
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (active) {
        const uint32_t y = n / a.W, x = n - y * a.W;
        float img[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) img[j] = a.image[(size_t)n * a.image_stride + j];
        const int32_t sel = s_sel;
        const bool under = sel >= 0 && a.masks[(size_t)sel * P + n] != 0;
        if (a.pred_mask) a.pred_mask[n] = under ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = img[j];   // no point (decode_step's else branch): the render as it is
        if (np != 0u) {
            if (a.masks) {                           // overlay_mask; without a decoder (trainer.py:884) the points go on the plain render
                const float red[3] = {1.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float over = under ? red[j] : img[j];
                    const float u = img[j] * a.a, w = over * a.b;
                    c[j] = u + w;
                }
            }
            for (uint32_t i = np; i-- > 0u;) {       // the last point that covers the pixel wins
                const uint32_t rx = s_rx[i], ry = s_ry[i];
                if (x >= (rx & 0xffffu) && x < ((rx >> 16) & 0x7fffu) && y >= (ry & 0xffffu) && y < ((ry >> 16) & 0x7fffu)) {
                    const bool pos = (ry >> 31) != 0u;                   // utils.py:96: green for label 0, red otherwise
                    c[0] = pos ? 1.0f : 0.0f; c[1] = pos ? 0.0f : 1.0f; c[2] = 0.0f;
                    break;
                }
            }
        }
    }
    if (!a.rgb && !a.rgb8) return;                   // uniform over the workgroup
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(s_rgb8);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s_rgb[tid * 3 + j] = c[j];
        s_bytes[tid * 3 + j] = rgb8_of(c[j]);
    }
    __syncthreads();
    if (a.rgb) {
        float *dst = a.rgb + (size_t)n0 * 3;
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            const uint32_t i = tid + j * PP_TILE;
            if (i < cnt * 3u) dst[i] = s_rgb[i];
        }
    }
    if (a.rgb8 && tid < PP_TILE * 3 / 4) {
        uint8_t *dst = a.rgb8 + (size_t)n0 * 3;      // n0 * 3 = blockIdx.x * 768: a dword boundary (the base is 4-byte aligned)
        const uint32_t bytes = cnt * 3u, b0 = tid * 4u;
        if (b0 + 4u <= bytes) {
            reinterpret_cast<uint32_t *>(dst)[tid] = s_rgb8[tid];
        } else {
            for (uint32_t b = b0; b < bytes; ++b) dst[b] = s_bytes[b];    // the image's last <= 3 bytes
        }
    }
}

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_points_lift(const int32_t *pixels, uint32_t M, const float *rays_o, const float *rays_d, const float *depth, uint32_t depth_stride,
                      uint32_t H, uint32_t W, float *point_3d, sn_stream_t stream) {
    if (M == 0) return SN_OK;
    SN_REQUIRE(pixels && rays_o && rays_d && depth && point_3d, "points_lift: NULL pointer");
    SN_REQUIRE(H >= 1 && W >= 1, "points_lift: an image of %u x %u pixels", H, W);
    SN_REQUIRE(depth_stride >= 1, "points_lift: depth pixel stride 0 (1: a plain [H,W] image, 5: the depth column of the render buffer)");
    SN_UNSUPPORTED((uint64_t)H * W < (1ull << 31), "points_lift: H * W must stay below 2^31 (got %u x %u)", H, W);
    SN_UNSUPPORTED(M < (1u << 30), "points_lift: M must stay below 2^30 (got %u)", M);
    hipLaunchKernelGGL(k_points_lift, dim3(div_up(M, 64)), dim3(64), 0, (hipStream_t)stream, pixels, M, rays_o, rays_d, depth, depth_stride, H, W, point_3d);
    SN_LAUNCH_CHECK("k_points_lift");
    return SN_OK;
}

int sn_rm_point_store_update(float *xyz, int32_t *labels, int32_t *crucial, int32_t *count, uint32_t cap, const float *point, const int32_t *label,
                             float dist_thresh, int32_t *status, sn_stream_t stream) {
    SN_REQUIRE(cap >= 1, "point_store_update: a store of capacity 0");
    SN_UNSUPPORTED(cap <= PP_MAX, "point_store_update: at most %u stored points (got cap=%u)", PP_MAX, cap);
    SN_REQUIRE(xyz && labels && crucial && count && point && label && status, "point_store_update: NULL pointer");
    SN_REQUIRE(dist_thresh >= 0.0f, "point_store_update: dist_thresh must be a number >= 0");
    hipLaunchKernelGGL(k_point_store_update, dim3(1), dim3(div_up(cap, 64) * 64), 0, (hipStream_t)stream, xyz, labels, crucial, count, cap, point, label,
                       dist_thresh, status);
    SN_LAUNCH_CHECK("k_point_store_update");
    return SN_OK;
}

int sn_rm_points_project(const float *points, const int32_t *labels, const int32_t *crucial, uint32_t N, const int32_t *n_points, const float *poses,
                         uint32_t V, const float *intrinsics, uint32_t n_intr, const float *depth, uint32_t depth_stride, uint32_t H, uint32_t W,
                         float depth_tol, int32_t crucial_count, int32_t valid_threshold, double resize_ratio, int32_t *coords, int32_t *labels_out,
                         int32_t *kept_index, int32_t *sam_coords, int32_t *overlay_coords, float *cam, float *uv, int32_t *state, int32_t *counts,
                         sn_stream_t stream) {
    if (N == 0 || V == 0) return SN_OK;
    SN_REQUIRE(points && labels && poses && intrinsics && depth, "points_project: NULL input pointer");
    SN_REQUIRE(coords && labels_out && kept_index && counts, "points_project: NULL output pointer (coords, labels_out, kept_index and counts are always written)");
    SN_REQUIRE(n_intr == 1 || n_intr == V, "points_project: %u intrinsics for %u views (1 or V)", n_intr, V);
    SN_REQUIRE(H >= 1 && W >= 1, "points_project: an image of %u x %u pixels", H, W);
    SN_REQUIRE(depth_stride >= 1, "points_project: depth pixel stride 0 (1: a plain [V,H,W] stack, 5: the depth column of the render buffer)");
    SN_REQUIRE(resize_ratio >= 0.0 && resize_ratio < 1e300, "points_project: resize_ratio must be a finite number >= 0 (0: no SAM-frame coordinates)");
    if (resize_ratio > 0.0) SN_REQUIRE(sam_coords && overlay_coords, "points_project: NULL sam_coords / overlay_coords with a resize_ratio");
    SN_UNSUPPORTED(H < (1u << 24) && W < (1u << 24) && (uint64_t)H * W < (1ull << 31), "points_project: H * W must stay below 2^31 (got %u x %u)", H, W);
    SN_UNSUPPORTED((uint64_t)N * V < (1ull << 30), "points_project: N * V must stay below 2^30 (got %u x %u)", N, V);
    ProjectArgs a;
    a.points = points; a.labels = labels; a.crucial = crucial; a.n_points = n_points; a.poses = poses; a.intrinsics = intrinsics; a.depth = depth;
    a.N = N; a.V = V; a.n_intr = n_intr; a.depth_stride = depth_stride; a.H = H; a.W = W;
    a.depth_tol = depth_tol; a.ratio = resize_ratio; a.ratio_f = (float)resize_ratio;
    a.crucial_count = crucial_count; a.valid_threshold = valid_threshold;
    a.coords = coords; a.labels_out = labels_out; a.kept_index = kept_index;
    a.sam_coords = resize_ratio > 0.0 ? sam_coords : nullptr; a.overlay_coords = resize_ratio > 0.0 ? overlay_coords : nullptr;
    a.cam = cam; a.uv = uv; a.state = state; a.counts = counts;
    hipLaunchKernelGGL(k_points_project, dim3(V), dim3(64), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_points_project");
    return SN_OK;
}

int sn_rm_prompt_overlay(const float *image, uint32_t image_stride, uint32_t H, uint32_t W, const uint8_t *masks, uint32_t M, const float *scores,
                         int32_t mask_index, const int32_t *coords, const int32_t *labels, uint32_t N, const int32_t *count, int32_t radius, double alpha,
                         float *rgb, uint8_t *rgb8, uint8_t *pred_mask, int32_t *selected, sn_stream_t stream) {
    if (H == 0 || W == 0) return SN_OK;
    SN_REQUIRE(image, "prompt_overlay: NULL image");
    SN_REQUIRE(image_stride >= 3, "prompt_overlay: image row stride %u floats, at least 3", image_stride);
    SN_UNSUPPORTED(H <= PP_MAX_EXTENT && W <= PP_MAX_EXTENT, "prompt_overlay: H and W at most %u (got %u x %u)", PP_MAX_EXTENT, H, W);
    SN_UNSUPPORTED(N <= PP_MAX, "prompt_overlay: at most %u points (got N=%u)", PP_MAX, N);
    SN_REQUIRE(N == 0 || (coords && labels), "prompt_overlay: NULL coords / labels for N=%u points", N);
    SN_REQUIRE(radius >= 0 && radius <= (int32_t)PP_MAX_EXTENT, "prompt_overlay: radius %d outside 0..%u", radius, PP_MAX_EXTENT);
    SN_REQUIRE(selected, "prompt_overlay: NULL selected (one int32 on the device)");
    SN_REQUIRE(rgb || rgb8 || pred_mask, "prompt_overlay: no output given");
    if (masks) {
        SN_REQUIRE(M >= 1, "prompt_overlay: masks without a mask (M = 0)");
        if (!scores) SN_REQUIRE(mask_index >= 0 && (uint32_t)mask_index < M, "prompt_overlay: mask_index %d outside the %u masks", mask_index, M);
        SN_UNSUPPORTED((uint64_t)M * H * W < (1ull << 32), "prompt_overlay: M * H * W must stay below 2^32");
    }
    SN_REQUIRE((reinterpret_cast<uintptr_t>(rgb8) & 3u) == 0, "prompt_overlay: rgb8 must be 4-byte aligned (it is stored as dwords)");
    OverlayArgs a;
    a.image = image; a.masks = masks; a.scores = scores; a.coords = coords; a.labels = labels; a.count = count;
    a.image_stride = image_stride; a.H = H; a.W = W; a.M = M; a.N = N; a.mask_index = mask_index; a.radius = radius;
    a.a = (float)alpha; a.b = (float)(1.0 - alpha);
    a.rgb = rgb; a.rgb8 = rgb8; a.pred_mask = pred_mask; a.selected = selected;
    hipLaunchKernelGGL(k_prompt_overlay, dim3(div_up((uint64_t)H * W, PP_TILE)), dim3(PP_TILE), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_prompt_overlay");
    return SN_OK;
}

}  // extern "C"
