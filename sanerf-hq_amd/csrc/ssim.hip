// ssim.hip — the reference's SSIMMeter.update (nerf/metrics.py:124-131: torchmetrics' structural_similarity_index_measure at its defaults)
// for one image pair on the device, for gfx950:
//   sn_rm_image_ssim_accumulate   [k_image_range +] k_image_ssim -- one launch per image (two when data_range is derived), no host read
//
// The quantity (include/sanerf_hip.h states it in full): g = the normalised 11-tap Gaussian of sigma 1.5, window g (x) g; per channel and
// per interior pixel (5 <= y < H - 5, 5 <= x < W - 5) the five window means mu_p, mu_t, E[pp], E[tt], E[pt], the two clamped variances,
// the covariance, and ((2 mu_p mu_t + c1)(2 s_pt + c2)) / ((mu_p^2 + mu_t^2 + c1)(s_p^2 + s_t^2 + c2)); the image's value is the mean over
// channels and interior pixels.  The package's reflect padding never reaches a kept pixel, so this is a valid-window evaluation.
//
// Conventions of mask_output.hip: IEEE division, nothing contracted (every fma below is an explicit fmaf), no float atomics, nothing
// synchronises with the host, every floating-point sum has a fixed order: two runs give the same bits, the record included.
//
// Layout.  A workgroup of 256 lanes owns tiles of 32 x 16 interior pixels and walks its tiles in ascending order; the grid depends on H
// and W only.  Per tile:
//   stage      the (32 + 10) x (16 + 10) halo of both images into LDS, a plane per channel.  A halo row is one contiguous range of
//              42 * stride floats of the image (stride 3: a packed image; 5: the [N,5] render buffer read in place), and the 26 ranges
//              laid end to end are read as consecutive dwords, lane i + 256 k the dword i + 256 k (a wave instruction reads 256
//              contiguous bytes, broken only where a halo row ends); dwords of the columns 3.. of a wider row are not loaded.
//              What is stored is p - a, t - b: the CENTRED values, a / b = the tile's first interior pixel per image and channel.
//   horizontal the 11-tap pass of the five maps q, u, qq, uu, qu (q = p - a, u = t - b) from the planes into LDS rows of 32 floats,
//              a 32-lane group a halo row, a lane a column;
//   vertical   the 11-tap pass in registers: a lane owns a column and two output rows and slides over 12 rows of each map;
//   evaluate   in fp32, the pivots added back to the means only; the valid pixels' values are added to the lane's double.
// The three channels go through horizontal / vertical one after the other and share the LDS of the maps.
//
// Centred moments.  E[pp] - mu_p^2 on raw fp32 values cancels catastrophically when the image varies little around a large mean (a
// derived data_range of 1e-3 makes c2 = 9e-10 while ulp(1) = 6e-8: the uncentred fp32 statement gives -1.84 where fp64 gives 0.8895).
// Variance and covariance do not change under a shift, so they are formed from the centred maps, whose values are of the size of the
// tile's own variation; only the means get the pivots back.
//
// LDS banks (ds_read_b32 / ds_write_b32: 32 banks, serviced per group of 32 lanes).  In both passes the 32 lanes of a group address 32
// consecutive dwords of one row -- every bank once, whatever the row stride (42 floats in the planes, 32 in the maps).  The staging
// stores of a group go to <= 11 consecutive pixels of each of the three planes; the plane stride is 11 mod 32, so the three runs lie in
// disjoint banks (a group that straddles two halo rows can meet a bank twice, which a ds_write_b32 absorbs at no cost).
// LDS per workgroup: 6 planes * 1099 + 5 maps * 26 * 32 floats = 43 016 bytes, three workgroups per CU.
//
// Reduction: the ticket reduction of sn_reduce.h.  A lane adds its pixels in ascending (tile, channel, row) order in double; the workgroup
// that draws the last ticket sums the partials (out of the maps' LDS), divides, adds to the record and returns the workspace to zero.
//
// k_image_range (only when data_range is derived): min and max of both images in one launch, consecutive dwords as above; a wave's
// results enter the workspace through integer atomic maxima on an order-preserving key (of x for the maximum, of -x for the minimum; key 0
// = nothing seen yet, so the workspace is zero at rest), a NaN through an atomic OR.  k_image_ssim decodes them on the same stream.
#include "sn_reduce.h"

namespace sn {

constexpr uint32_t SS_TAPS = 11, SS_R = SS_TAPS / 2;
constexpr uint32_t SS_TW = 32, SS_TH = 16;                              // interior pixels of a tile
constexpr uint32_t SS_HW = SS_TW + 2 * SS_R, SS_HH = SS_TH + 2 * SS_R;  // its halo: 42 x 26
constexpr uint32_t SS_THREADS = SN_REDUCE_THREADS;
constexpr uint32_t SS_PLANE = 1099;                                     // floats per channel plane: 26 * 42 = 1092, padded to 11 mod 32
constexpr uint32_t SS_MAX_PARTIALS = 512;                               // workgroups of k_image_ssim (a workgroup loops over tiles beyond)
constexpr uint32_t SS_MAX_RANGE_BLOCKS = 1024;
constexpr uint32_t SS_MAX_STRIDE = 64;                                  // floats between rows: the halo is read as whole rows
static_assert(SS_PLANE >= SS_HH * SS_HW && SS_PLANE % 32 == 11, "plane stride");
static_assert(SS_THREADS == 8 * SS_TW && SS_TH == 2 * 8, "8 groups of 32 lanes: a halo row each in the horizontal pass, two output rows each in the vertical");

// workspace (SN_SSIM_WORKSPACE_BYTES, zero at rest)
struct SsimWorkspace {
    uint32_t ticket, nan_seen;
    uint32_t key[4];                              // order_key of: max pred | max -pred | max truth | max -truth; 0: nothing seen
    uint32_t pad[2];
    double part_sum[SS_MAX_PARTIALS];
};
static_assert(sizeof(SsimWorkspace) <= SN_SSIM_WORKSPACE_BYTES, "the workspace constant of the header is too small");

// a uint32 that orders as the floats do (-inf lowest; no NaN comes here); never 0
__device__ __forceinline__ uint32_t order_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// One image's dwords [0, (N - 1) stride + 3) -- its first pixel's red to its last pixel's blue -- grid-strided; the column of a lane's
// dword advances by a constant per step, so no element pays a division.
__device__ __forceinline__ void scan_range(const float *__restrict__ img, uint32_t stride, uint32_t N, float &lo, float &hi, bool &nan) {
    const uint64_t total = (uint64_t)(N - 1u) * stride + 3u;
    const uint32_t step = gridDim.x * SS_THREADS, step_c = step % stride, first = blockIdx.x * SS_THREADS + threadIdx.x;
    uint32_t c = first % stride;
    for (uint64_t i = first; i < total; i += step) {
        if (c < 3u) {
            const float v = img[i];
            lo = fminf(lo, v); hi = fmaxf(hi, v); nan = nan || v != v;
        }
        c += step_c;
        if (c >= stride) c -= stride;
    }
}

__global__ __launch_bounds__(256) void k_image_range(const float *__restrict__ pred, uint32_t pred_stride, const float *__restrict__ truth,
                                                     uint32_t truth_stride, uint32_t N, SsimWorkspace *__restrict__ ws) {
    const float inf = __builtin_inff();
    float lo_p = inf, hi_p = -inf, lo_t = inf, hi_t = -inf;
    bool nan = false;
    scan_range(pred, pred_stride, N, lo_p, hi_p, nan);
    scan_range(truth, truth_stride, N, lo_t, hi_t, nan);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo_p = fminf(lo_p, __shfl_xor(lo_p, off, 64)); hi_p = fmaxf(hi_p, __shfl_xor(hi_p, off, 64));
        lo_t = fminf(lo_t, __shfl_xor(lo_t, off, 64)); hi_t = fmaxf(hi_t, __shfl_xor(hi_t, off, 64));
    }
    const bool any_nan = __any(nan ? 1 : 0) != 0;
    if ((threadIdx.x & 63u) == 0) {               // integer maxima: the result does not depend on the order of arrival
        if (hi_p >= lo_p) { atomicMax(&ws->key[0], order_key(hi_p)); atomicMax(&ws->key[1], order_key(-lo_p)); }
        if (hi_t >= lo_t) { atomicMax(&ws->key[2], order_key(hi_t)); atomicMax(&ws->key[3], order_key(-lo_t)); }
        if (any_nan) atomicOr(&ws->nan_seen, 1u);
    }
}

struct SsimArgs {
    const float *pred, *truth;
    uint32_t pred_stride, truth_stride, H, W, tiles_x, tiles;
    float data_range;                             // used when derive == 0
    int derive;
    float g[SS_TAPS];
    sn_ssim_record *rec;
    SsimWorkspace *ws;
};

// The halo of the tile whose first interior pixel is (y0, x0) -- image rows y0 .. y0 + 25, columns x0 .. x0 + 41 -- minus the pivots, into
// the image's three planes; positions outside the image (a ragged last tile) hold 0 and feed no valid pixel.  Every lane calls it.
__device__ __forceinline__ void stage_halo(const float *__restrict__ img, uint32_t stride, uint32_t H, uint32_t W, uint32_t y0, uint32_t x0,
                                           float piv0, float piv1, float piv2, float *__restrict__ planes) {
    const uint32_t span = SS_HW * stride, total = SS_HH * span;          // stride <= SS_MAX_STRIDE: no overflow
    // the dword i = tid + 256 k of the 26 rows laid end to end is (row r, pixel px, column c); a step of 256 moves all three by constants
    const uint32_t rem = SS_THREADS % span, d_r = SS_THREADS / span, d_px = rem / stride, d_c = rem % stride;
    const uint32_t tid = threadIdx.x, j = tid % span;
    uint32_t r = tid / span, px = j / stride, c = j % stride;
    for (uint32_t i = tid; i < total; i += SS_THREADS) {
        if (c < 3u) {
            const uint32_t y = y0 + r, x = x0 + px;
            float v = 0.0f;
            if (y < H && x < W) v = img[((size_t)y * W + x) * stride + c] - (c == 0u ? piv0 : (c == 1u ? piv1 : piv2));
            planes[c * SS_PLANE + r * SS_HW + px] = v;
        }
        c += d_c;
        if (c >= stride) { c -= stride; ++px; }
        px += d_px;
        if (px >= SS_HW) { px -= SS_HW; ++r; }
        r += d_r;
    }
}

__global__ __launch_bounds__(256) void k_image_ssim(const SsimArgs a) {
    SN_POISON_ALL();
    __shared__ float s_img[2 * 3 * SS_PLANE];                            // centred pred | truth, a plane per channel, rows of SS_HW floats
    __shared__ __align__(8) float s_h[5 * SS_HH * SS_TW];                // the five maps after the horizontal pass; at the end: the partials
    __shared__ double s_wave[4];
    __shared__ uint32_t s_flag;
    static_assert(sizeof(s_h) >= SS_MAX_PARTIALS * sizeof(double), "the partials are summed out of the maps' LDS");
    const uint32_t tid = threadIdx.x, x = tid & (SS_TW - 1u), grp = tid / SS_TW;
    const uint32_t Hi = a.H - 2u * SS_R, Wi = a.W - 2u * SS_R;

    float dr = a.data_range;
    if (a.derive) {                                                      // what k_image_range left: max(pred.max - pred.min, truth.max - truth.min)
        uint32_t k[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) k[i] = __hip_atomic_load(&a.ws->key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t nan_seen = __hip_atomic_load(&a.ws->nan_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float rp = key_value(k[0]) + key_value(k[1]), rt = key_value(k[2]) + key_value(k[3]);      // max + (-min)
        dr = (nan_seen != 0u || rp != rp || rt != rt) ? __builtin_nanf("") : fmaxf(rp, rt);
    }
    const float k1 = 0.01f * dr, k2 = 0.03f * dr, c1 = k1 * k1, c2 = k2 * k2;

    double sum = 0.0;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x, y0 = ty * SS_TH, x0 = tx * SS_TW;
        // pivots: the tile's first interior pixel (always inside the image), uniform over the workgroup
        const size_t pv = (size_t)(y0 + SS_R) * a.W + (x0 + SS_R);
        const float *pp = a.pred + pv * a.pred_stride, *tp = a.truth + pv * a.truth_stride;
        const float pa[3] = {pp[0], pp[1], pp[2]}, tb[3] = {tp[0], tp[1], tp[2]};
        // (the planes were last read by the previous tile's third horizontal pass, which a barrier follows)
        stage_halo(a.pred, a.pred_stride, a.H, a.W, y0, x0, pa[0], pa[1], pa[2], s_img);
        stage_halo(a.truth, a.truth_stride, a.H, a.W, y0, x0, tb[0], tb[1], tb[2], s_img + 3 * SS_PLANE);
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            __syncthreads();                                             // the planes are staged / the maps of the previous channel have been read
            for (uint32_t r = grp; r < SS_HH; r += SS_THREADS / SS_TW) {
                const float *q_row = s_img + c * SS_PLANE + r * SS_HW + x, *u_row = q_row + 3 * SS_PLANE;
                float mq = 0.0f, mu = 0.0f, qq = 0.0f, uu = 0.0f, qu = 0.0f;
#pragma unroll
                for (uint32_t k = 0; k < SS_TAPS; ++k) {
                    const float q = q_row[k], u = u_row[k], gq = a.g[k] * q, gu = a.g[k] * u;
                    mq += gq; mu += gu;
                    qq = __builtin_fmaf(gq, q, qq); uu = __builtin_fmaf(gu, u, uu); qu = __builtin_fmaf(gq, u, qu);
                }
                float *h = s_h + r * SS_TW + x;
                h[0 * SS_HH * SS_TW] = mq; h[1 * SS_HH * SS_TW] = mu; h[2 * SS_HH * SS_TW] = qq; h[3 * SS_HH * SS_TW] = uu; h[4 * SS_HH * SS_TW] = qu;
            }
            __syncthreads();
            const uint32_t oy = 2u * grp;                                // this lane's output rows oy, oy + 1 of column x
            float acc[2][5];
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[0][m] = acc[1][m] = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < SS_TAPS + 1; ++k) {
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    const float v = s_h[m * SS_HH * SS_TW + (oy + k) * SS_TW + x];
                    if (k < SS_TAPS) acc[0][m] = __builtin_fmaf(a.g[k < SS_TAPS ? k : 0], v, acc[0][m]);
                    if (k >= 1) acc[1][m] = __builtin_fmaf(a.g[k >= 1 ? k - 1 : 0], v, acc[1][m]);
                }
            }
#pragma unroll
            for (uint32_t o = 0; o < 2; ++o) {
                const float mq = acc[o][0], mu = acc[o][1];
                const float mp = pa[c] + mq, mt = tb[c] + mu;            // the pivots go back into the means only
                const float var_p = relu_ieee(acc[o][2] - mq * mq), var_t = relu_ieee(acc[o][3] - mu * mu), cov = acc[o][4] - mq * mu;
                const float num = (2.0f * mp * mt + c1) * (2.0f * cov + c2);
                const float den = (mp * mp + mt * mt + c1) * (var_p + var_t + c2);
                const float s = num / den;
                if (y0 + oy + o < Hi && x0 + x < Wi) sum += (double)s;
            }
        }
    }

    if (!publish_and_draw(sum, 0u, &a.ws->ticket, a.ws->part_sum, nullptr, s_wave, nullptr, &s_flag)) return;
    // the last workgroup: everyone has published (and has long read the range keys); the workspace back to zero
    if (tid < 4u) __hip_atomic_store(&a.ws->key[tid], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double total = sum_partials(a.ws->part_sum, nullptr, reinterpret_cast<double *>(s_h), nullptr, nullptr);
    if (tid == 0) {
        const double value = total / (3.0 * (double)Hi * (double)Wi);
        a.rec->ssim_sum += value;                                        // SSIMMeter.V
        a.rec->last = value;
        a.rec->images += 1;                                              // SSIMMeter.N
        __hip_atomic_store(&a.ws->nan_seen, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&a.ws->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_image_ssim_accumulate(const float *pred, uint32_t pred_stride, const float *truth, uint32_t truth_stride, uint32_t H, uint32_t W,
                                float data_range, sn_ssim_record *record, void *workspace, sn_stream_t stream) {
    SN_REQUIRE(pred && truth && record && workspace, "image_ssim_accumulate: NULL pointer");
    SN_REQUIRE(pred_stride >= 3 && truth_stride >= 3, "image_ssim_accumulate: row strides %u / %u floats, at least 3", pred_stride, truth_stride);
    SN_UNSUPPORTED(pred_stride <= SS_MAX_STRIDE && truth_stride <= SS_MAX_STRIDE,
                   "image_ssim_accumulate: row strides %u / %u floats, at most %u (the halo is read as whole rows: pack a sparser image first)",
                   pred_stride, truth_stride, SS_MAX_STRIDE);
    if (H < SS_TAPS || W < SS_TAPS) {
        set_error("image_ssim_accumulate: a %u x %u image is smaller than the %u x %u window", H, W, SS_TAPS, SS_TAPS);
        return SN_ERR_WINDOW;
    }
    SN_UNSUPPORTED((uint64_t)H * W < (1ull << 31), "image_ssim_accumulate: H * W must stay below 2^31 (got %u x %u)", H, W);
    SN_REQUIRE(((reinterpret_cast<uintptr_t>(record) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
               "image_ssim_accumulate: record / workspace must be 8-byte aligned");
    SsimArgs a;
    a.pred = pred; a.truth = truth; a.pred_stride = pred_stride; a.truth_stride = truth_stride; a.H = H; a.W = W;
    a.tiles_x = div_up(W - 2u * SS_R, SS_TW);
    a.tiles = a.tiles_x * div_up(H - 2u * SS_R, SS_TH);
    a.derive = data_range > 0.0f ? 0 : 1;
    a.data_range = data_range;
    double g[SS_TAPS], norm = 0.0;                                       // exp(-(d / 1.5)^2 / 2), d = -5 .. 5, over its sum
    for (uint32_t k = 0; k < SS_TAPS; ++k) {
        const double d = ((double)k - (double)SS_R) / 1.5;
        g[k] = exp(-0.5 * d * d);
        norm += g[k];
    }
    for (uint32_t k = 0; k < SS_TAPS; ++k) a.g[k] = (float)(g[k] / norm);
    a.rec = record;
    a.ws = static_cast<SsimWorkspace *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t N = H * W;
    if (a.derive) {
        const uint32_t blocks = div_up(N, SS_THREADS) < SS_MAX_RANGE_BLOCKS ? div_up(N, SS_THREADS) : SS_MAX_RANGE_BLOCKS;
        hipLaunchKernelGGL(k_image_range, dim3(blocks), dim3(SS_THREADS), 0, st, pred, pred_stride, truth, truth_stride, N, a.ws);
        SN_LAUNCH_CHECK("k_image_range");
    }
    const uint32_t blocks = a.tiles < SS_MAX_PARTIALS ? a.tiles : SS_MAX_PARTIALS;
    hipLaunchKernelGGL(k_image_ssim, dim3(blocks), dim3(SS_THREADS), 0, st, a);
    SN_LAUNCH_CHECK("k_image_ssim");
    return SN_OK;
}

}  // extern "C"
