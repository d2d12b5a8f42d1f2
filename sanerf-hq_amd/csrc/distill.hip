// distill.hip — the loss tail of the SAM-feature distillation step (nerf/trainer.py:540-550 in training, :664-670 in evaluation) for gfx950:
//   sn_rm_feature_distill_loss   k_feature_distill [+ k_feature_distill_pull]  -- bilinear resize, MSE and the gradient with respect to the
//                                rendered features; one launch when h, w == Ho, Wo (the reference's usual case), two otherwise
//   sn_rm_feature_map            k_feature_distill without a target            -- the resize alone: [h w, C] rows -> packed [C, Ho, Wo]
// The reference spells this out as reshape / permute / contiguous / F.interpolate(mode="bilinear") / MSELoss / mean and their autograd
// mirror images.  The quantity (include/sanerf_hip.h states it in full): the taps of an axis are axis_tap() below, an fp32 chain;
//   pred = l0y (l0x f[y0,x0] + l1x f[y0,x1]) + l1y (l0x f[y1,x0] + l1x f[y1,x1]),  d = pred - target in fp32,  loss = sum d^2 / n in double,
//   grad_feat = coef sum_o w(o -> pixel) d[o],  coef = (scale * *scale_dev) * (2 / n).
//
// Conventions of mask_output.hip / ssim.hip: nothing contracted (-ffp-contract=off, no fmaf here at all), no float atomics, nothing
// synchronises with the host, every floating-point sum has a fixed order: two runs give the same bits.
//
// Layout.  `target` and `resized` are contiguous along ox, `feat` and `grad_feat` along c.  A workgroup of 256 lanes owns tiles of
// 64 channels x 32 ox of one output row and walks its tiles in ascending order.  Per tile:
//   stage    target into LDS with lanes along ox: a 32-lane group reads 32 consecutive floats of one channel's row (a whole 128-byte
//            segment where Wo is a multiple of 32), 8 channels per instruction, 8 instructions;
//   compute  with lanes along c: a wave owns an ox (its x taps are wave-uniform, the y taps workgroup-uniform), its 64 lanes read 64
//            consecutive dwords of each of the four feat rows (one row on the identity path, which reads no zero-weight neighbour);
//            pred, d = pred - target (LDS), d * d added to the lane's double; the identity path stores coef * d to grad_feat, the general
//            path d to the channels-last buffer [Ho, Wo, C] of the workspace -- both as 64 consecutive dwords;
//   unstage  (when `resized` is asked for) pred goes back through the same LDS cell and out with lanes along ox.
// LDS banks (ds_read_b32 / ds_write_b32: 32 banks, serviced per group of 32 lanes): the tile's rows are 33 floats apart.  With lanes along
// ox a group addresses 32 consecutive dwords of one row; with lanes along c it addresses one column of 32 consecutive rows, bank
// (33 c + ox) mod 32 = (c + ox) mod 32 -- every bank once either way.
//
// The gradient is a pull (k_feature_distill_pull, general path only): the outputs whose taps reach source row y are those with
// y - 1 <= i0(o) <= y, a contiguous range because i0 is monotone in o; its ends are found by bisection on axis_tap() itself, so forward
// and backward cannot disagree.  A lane owns 4 channels (1 when C is no multiple of 4) of one source pixel, adds wy (sum_ox wx d) in
// ascending order and writes its element exactly once -- 0 where no output reaches the pixel; the caller does not clear grad_feat.
//
// Reduction: the ticket reduction of sn_reduce.h.  A lane adds its elements in ascending tile order in double; the workgroup that draws
// the last ticket sums the partials, divides, stores the loss and returns the fixed part of the workspace to zero.
#include "sn_reduce.h"

namespace sn {

int g_distill_general = 0;       // sn_debug_set("distill_general", 1): the identity shapes take the general (four-tap, two-launch) path too

constexpr uint32_t DI_THREADS = SN_REDUCE_THREADS;
constexpr uint32_t DI_CT = 64, DI_OT = 32;        // a tile: channels x ox
constexpr uint32_t DI_ROW = DI_OT + 1;            // floats between the tile's rows in LDS
constexpr uint32_t DI_MAX_PARTIALS = 1024;        // workgroups of k_feature_distill (a workgroup loops over tiles beyond)
static_assert(DI_THREADS == 8 * DI_OT && DI_THREADS == 4 * DI_CT && DI_CT % 8 == 0 && DI_OT % 4 == 0, "8 channels per staging step, 4 ox per compute step");

// the fixed part of the workspace (SN_DISTILL_WORKSPACE_FIXED_BYTES, zero at rest); the general path's d buffer follows it
struct DistillWorkspace {
    uint32_t ticket, pad[15];
    double part_sum[DI_MAX_PARTIALS];
};
static_assert(sizeof(DistillWorkspace) == SN_DISTILL_WORKSPACE_FIXED_BYTES && SN_DISTILL_WORKSPACE_FIXED_BYTES % 16 == 0, "the workspace constant of the header");

// The two taps of output index o on an axis of n_in source samples, s = float(n_in) / float(n_out): the contract's fp32 chain.
struct Tap {
    uint32_t i0, i1;
    float l0, l1;
};
__host__ __device__ __forceinline__ Tap axis_tap(uint32_t o, uint32_t n_in, float s) {
    float src = ((float)o + 0.5f) * s - 0.5f;
    src = src > 0.0f ? src : 0.0f;
    const uint32_t i = (uint32_t)src;
    Tap t;
    t.i0 = i < n_in - 1u ? i : n_in - 1u;
    t.i1 = t.i0 + (t.i0 < n_in - 1u ? 1u : 0u);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}
// what output o gives source sample i (both taps land on the last sample when i0 is clamped there)
__device__ __forceinline__ float tap_weight(const Tap &t, uint32_t i) { return (t.i0 == i ? t.l0 : 0.0f) + (t.i1 == i ? t.l1 : 0.0f); }
// the first o in [0, n_out] with i0(o) >= v (n_out: none); i0 is monotone in o
__device__ __forceinline__ uint32_t first_tap_at_least(uint32_t v, uint32_t n_in, uint32_t n_out, float s) {
    uint32_t lo = 0, hi = n_out;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (axis_tap(mid, n_in, s).i0 >= v) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

struct DistillArgs {
    const float *feat, *target, *scale_dev;
    float *loss, *grad, *resized, *dbuf;          // each may be NULL; dbuf: the general path's d, channels-last [Ho, Wo, C]
    DistillWorkspace *ws;
    uint32_t stride, h, w, C, Ho, Wo, n;
    uint32_t tiles_x, tiles;
    float sy, sx, scale;
};

__device__ __forceinline__ float distill_coef(float scale, const float *scale_dev, uint32_t n) {
    const float sd = scale_dev ? *scale_dev : 1.0f;
    return (scale * sd) * (2.0f / (float)n);
}

template <bool IDENT>
__global__ __launch_bounds__(256) void k_feature_distill(const DistillArgs a) {
    SN_POISON_ALL();
    __shared__ float s_t[DI_CT * DI_ROW];                                // target, then pred: [channel][ox]
    __shared__ double s_part[DI_MAX_PARTIALS];
    __shared__ double s_wave[4];
    __shared__ uint32_t s_flag;
    const uint32_t tid = threadIdx.x;
    const uint32_t lx = tid & (DI_OT - 1u), lc = tid / DI_OT;           // staging: a lane an ox, a 32-lane group a channel (8 at a time)
    const uint32_t cc = tid & (DI_CT - 1u), og = tid / DI_CT;           // compute: a lane a channel, a wave an ox (4 at a time)
    const size_t plane = (size_t)a.Ho * a.Wo;
    const float coef = (IDENT && a.grad) ? distill_coef(a.scale, a.scale_dev, a.n) : 0.0f;

    double sum = 0.0;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const uint32_t tx = t % a.tiles_x, r = t / a.tiles_x, oy = r % a.Ho, tc = r / a.Ho;
        const uint32_t ox0 = tx * DI_OT, c0 = tc * DI_CT;
        if (t != blockIdx.x) __syncthreads();                            // the previous tile's cells have been read
        if (a.target) {
            const uint32_t ox = ox0 + lx;
#pragma unroll
            for (uint32_t k = 0; k < DI_CT / 8u; ++k) {
                const uint32_t c = lc + 8u * k;
                if (ox < a.Wo && c0 + c < a.C) s_t[c * DI_ROW + lx] = a.target[(size_t)(c0 + c) * plane + (size_t)oy * a.Wo + ox];
            }
            __syncthreads();
        }
        const uint32_t c = c0 + cc;
        Tap ty;
        if (!IDENT) ty = axis_tap(oy, a.h, a.sy);
#pragma unroll
        for (uint32_t k = 0; k < DI_OT / 4u; ++k) {
            const uint32_t oxl = og + 4u * k, ox = ox0 + oxl;
            if (ox >= a.Wo || c >= a.C) continue;
            float pred;
            if (IDENT) {
                pred = a.feat[((size_t)oy * a.w + ox) * a.stride + c];
            } else {
                const Tap tx_ = axis_tap(ox, a.w, a.sx);
                const float *r0 = a.feat + (size_t)ty.i0 * a.w * a.stride + c, *r1 = a.feat + (size_t)ty.i1 * a.w * a.stride + c;
                const float f00 = r0[(size_t)tx_.i0 * a.stride], f01 = r0[(size_t)tx_.i1 * a.stride];
                const float f10 = r1[(size_t)tx_.i0 * a.stride], f11 = r1[(size_t)tx_.i1 * a.stride];
                pred = ty.l0 * (tx_.l0 * f00 + tx_.l1 * f01) + ty.l1 * (tx_.l0 * f10 + tx_.l1 * f11);
            }
            float *cell = s_t + cc * DI_ROW + oxl;
            if (a.target) {
                const float d = pred - *cell;
                sum += (double)d * (double)d;
                const size_t e = ((size_t)oy * a.Wo + ox) * a.C + c;
                if (IDENT) { if (a.grad) a.grad[e] = coef * d; }
                else if (a.dbuf) a.dbuf[e] = d;
            }
            if (a.resized) *cell = pred;
        }
        if (a.resized) {
            __syncthreads();
            const uint32_t ox = ox0 + lx;
#pragma unroll
            for (uint32_t k = 0; k < DI_CT / 8u; ++k) {
                const uint32_t cs = lc + 8u * k;
                if (ox < a.Wo && c0 + cs < a.C) a.resized[(size_t)(c0 + cs) * plane + (size_t)oy * a.Wo + ox] = s_t[cs * DI_ROW + lx];
            }
        }
    }
    if (!a.loss) return;                                                 // sn_rm_feature_map: nothing to reduce (uniform over the launch)

    if (!publish_and_draw(sum, 0u, &a.ws->ticket, a.ws->part_sum, nullptr, s_wave, nullptr, &s_flag)) return;
    const double total = sum_partials(a.ws->part_sum, nullptr, s_part, nullptr, nullptr);
    if (tid == 0) {
        *a.loss = (float)(total / (double)a.n);
        __hip_atomic_store(&a.ws->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct PullArgs {
    const float *dbuf, *scale_dev;
    float *grad;
    uint32_t h, w, C, Ho, Wo, n, elems;           // elems = h w (C / VEC)
    float sy, sx, scale;
};

// grad_feat[p, c] = coef sum_oy wy(oy -> y) sum_ox wx(ox -> x) d[oy, ox, c]: a lane VEC channels of one source pixel
template <int VEC>
__global__ __launch_bounds__(256) void k_feature_distill_pull(const PullArgs a) {
    const uint32_t e = blockIdx.x * DI_THREADS + threadIdx.x;
    if (e >= a.elems) return;
    const uint32_t cv = a.C / (uint32_t)VEC, c = (e % cv) * (uint32_t)VEC, p = e / cv, y = p / a.w, x = p - y * a.w;
    const uint32_t oy_lo = y ? first_tap_at_least(y - 1u, a.h, a.Ho, a.sy) : 0u, oy_hi = first_tap_at_least(y + 1u, a.h, a.Ho, a.sy);
    const uint32_t ox_lo = x ? first_tap_at_least(x - 1u, a.w, a.Wo, a.sx) : 0u, ox_hi = first_tap_at_least(x + 1u, a.w, a.Wo, a.sx);
    const float coef = distill_coef(a.scale, a.scale_dev, a.n);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0f;
    for (uint32_t oy = oy_lo; oy < oy_hi; ++oy) {
        const float wy = tap_weight(axis_tap(oy, a.h, a.sy), y);
        float row[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) row[j] = 0.0f;
        const float *drow = a.dbuf + (size_t)oy * a.Wo * a.C + c;
        for (uint32_t ox = ox_lo; ox < ox_hi; ++ox) {
            const float wx = tap_weight(axis_tap(ox, a.w, a.sx), x);
            const float *dp = drow + (size_t)ox * a.C;
            if constexpr (VEC == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(dp);
                row[0] += wx * v.x; row[1] += wx * v.y; row[2] += wx * v.z; row[3] += wx * v.w;
            } else {
                row[0] += wx * dp[0];
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += wy * row[j];
    }
    float *g = a.grad + (size_t)p * a.C + c;
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(g) = make_float4(coef * acc[0], coef * acc[1], coef * acc[2], coef * acc[3]);
    else g[0] = coef * acc[0];
}

// sizes >= 1, h w C and n = C Ho Wo below 2^31
static int distill_shape(const char *who, uint32_t feat_stride, uint32_t h, uint32_t w, uint32_t C, uint32_t Ho, uint32_t Wo) {
    SN_REQUIRE(h >= 1 && w >= 1 && C >= 1 && Ho >= 1 && Wo >= 1, "%s: sizes h=%u w=%u C=%u Ho=%u Wo=%u must all be at least 1", who, h, w, C, Ho, Wo);
    SN_REQUIRE(feat_stride >= C, "%s: feat_stride %u floats is less than C = %u", who, feat_stride, C);
    const bool fits = (uint64_t)h * w < (1ull << 31) && (uint64_t)h * w * C < (1ull << 31) && (uint64_t)Ho * Wo < (1ull << 31) &&
                      (uint64_t)Ho * Wo * C < (1ull << 31);
    SN_UNSUPPORTED(fits, "%s: h * w * C and C * Ho * Wo must stay below 2^31 (got %u x %u -> %u x %u, C = %u)", who, h, w, Ho, Wo, C);
    return SN_OK;
}

static void distill_tiles(DistillArgs &a) {
    a.tiles_x = div_up(a.Wo, DI_OT);
    a.tiles = a.tiles_x * a.Ho * div_up(a.C, DI_CT);                     // <= n < 2^31
}

}  // namespace sn

using namespace sn;

extern "C" {

size_t sn_rm_feature_distill_workspace_bytes(uint32_t h, uint32_t w, uint32_t C, uint32_t Ho, uint32_t Wo) {
    if (distill_shape("feature_distill_workspace_bytes", C, h, w, C, Ho, Wo) != SN_OK) return 0;
    const bool ident = h == Ho && w == Wo && g_distill_general == 0;
    return SN_DISTILL_WORKSPACE_FIXED_BYTES + (ident ? 0 : (size_t)C * Ho * Wo * sizeof(float));
}

int sn_rm_feature_distill_loss(const float *feat, uint32_t feat_stride, uint32_t h, uint32_t w, uint32_t C, const float *target, uint32_t Ho,
                               uint32_t Wo, float scale, const float *scale_dev, float *loss, float *grad_feat, float *resized, void *workspace,
                               size_t workspace_bytes, sn_stream_t stream) {
    SN_REQUIRE(feat && target && loss && workspace, "feature_distill_loss: NULL pointer");
    const int rc = distill_shape("feature_distill_loss", feat_stride, h, w, C, Ho, Wo);
    if (rc != SN_OK) return rc;
    SN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "feature_distill_loss: workspace must be 8-byte aligned");
    const bool ident = h == Ho && w == Wo && g_distill_general == 0;
    const uint32_t n = C * Ho * Wo;
    const bool pull = !ident && grad_feat != nullptr;
    const size_t need = SN_DISTILL_WORKSPACE_FIXED_BYTES + (pull ? (size_t)n * sizeof(float) : 0);
    if (workspace_bytes < need) {
        set_error("feature_distill_loss: workspace of %zu bytes, %zu needed (sn_rm_feature_distill_workspace_bytes)", workspace_bytes, need);
        return SN_ERR_WORKSPACE;
    }
    DistillArgs a;
    a.feat = feat; a.target = target; a.scale_dev = scale_dev; a.loss = loss; a.grad = grad_feat; a.resized = resized;
    a.ws = static_cast<DistillWorkspace *>(workspace);
    a.dbuf = pull ? reinterpret_cast<float *>(static_cast<char *>(workspace) + SN_DISTILL_WORKSPACE_FIXED_BYTES) : nullptr;
    a.stride = feat_stride; a.h = h; a.w = w; a.C = C; a.Ho = Ho; a.Wo = Wo; a.n = n;
    a.sy = (float)h / (float)Ho; a.sx = (float)w / (float)Wo; a.scale = scale;
    distill_tiles(a);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t blocks = a.tiles < DI_MAX_PARTIALS ? a.tiles : DI_MAX_PARTIALS;
    if (ident) hipLaunchKernelGGL(k_feature_distill<true>, dim3(blocks), dim3(DI_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_feature_distill<false>, dim3(blocks), dim3(DI_THREADS), 0, st, a);
    SN_LAUNCH_CHECK("k_feature_distill");
    if (pull) {
        PullArgs p;
        p.dbuf = a.dbuf; p.scale_dev = scale_dev; p.grad = grad_feat;
        p.h = h; p.w = w; p.C = C; p.Ho = Ho; p.Wo = Wo; p.n = n; p.sy = a.sy; p.sx = a.sx; p.scale = scale;
        // four channels a lane where the rows of d and grad_feat are 16-byte aligned (the d buffer starts a multiple of 16 into the workspace)
        const bool vec4 = C % 4u == 0 && ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(grad_feat)) & 15u) == 0;
        p.elems = h * w * (vec4 ? C / 4u : C);
        if (vec4) hipLaunchKernelGGL(k_feature_distill_pull<4>, dim3(div_up(p.elems, DI_THREADS)), dim3(DI_THREADS), 0, st, p);
        else hipLaunchKernelGGL(k_feature_distill_pull<1>, dim3(div_up(p.elems, DI_THREADS)), dim3(DI_THREADS), 0, st, p);
        SN_LAUNCH_CHECK("k_feature_distill_pull");
    }
    return SN_OK;
}

int sn_rm_feature_map(const float *feat, uint32_t feat_stride, uint32_t h, uint32_t w, uint32_t C, uint32_t Ho, uint32_t Wo, float *out,
                      sn_stream_t stream) {
    SN_REQUIRE(feat && out, "feature_map: NULL pointer");
    const int rc = distill_shape("feature_map", feat_stride, h, w, C, Ho, Wo);
    if (rc != SN_OK) return rc;
    DistillArgs a;
    a.feat = feat; a.target = nullptr; a.scale_dev = nullptr; a.loss = nullptr; a.grad = nullptr; a.resized = out; a.dbuf = nullptr; a.ws = nullptr;
    a.stride = feat_stride; a.h = h; a.w = w; a.C = C; a.Ho = Ho; a.Wo = Wo; a.n = C * Ho * Wo;
    a.sy = (float)h / (float)Ho; a.sx = (float)w / (float)Wo; a.scale = 0.0f;
    distill_tiles(a);
    const uint32_t blocks = a.tiles < DI_MAX_PARTIALS ? a.tiles : DI_MAX_PARTIALS;
    if (h == Ho && w == Wo && g_distill_general == 0) hipLaunchKernelGGL(k_feature_distill<true>, dim3(blocks), dim3(DI_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_feature_distill<false>, dim3(blocks), dim3(DI_THREADS), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_feature_distill");
    return SN_OK;
}

}  // extern "C"
