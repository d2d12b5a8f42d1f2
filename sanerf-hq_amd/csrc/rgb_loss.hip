// rgb_loss.hip — the loss tail of the RGB training step (nerf/trainer.py:364-392; evaluation :586-595) for gfx950:
//   sn_rm_rgb_loss   k_rgb_loss   -- the RGBA blend of the ground truth, the per-ray background term of the prediction, MSE, the entropy
//                                    of weights_sum, the folded-in extras, and the gradients with respect to image and weights_sum: one launch
// The reference spells this out as slices / mul / add / MSELoss(reduction='none') / mean / clamp / log2 / mean and their autograd mirror
// images.  The quantity (include/sanerf_hip.h states it in full), per ray in fp32, b_c the ray's background:
//   gt = truth_c a + b_c (1 - a)  (RGBA; truth_c otherwise),  pred = image_c [+ (1 - weights_sum) b_c],  d = pred - gt,
//   c = clamp(weights_sum, 1e-5, 1 - 1e-5),  e = -c log2 c - (1 - c) log2(1 - c),
//   grad_image = 2 d / (3 N),  grad_weights_sum = -sum_c grad_image_c b_c  +  lambda_entropy / N (log2(1 - c) - log2 c) inside the clamp.
// The background term of the prediction is linear in bg, so a render over bg = 0 plus this tail equals the render over a per-ray
// background (renderer.py:353): the fused training route serves `--background random` without any of its kernels knowing.
//
// Conventions of mask_output.hip / ssim.hip / distill.hip: nothing contracted (-ffp-contract=off, no fmaf here at all), no float atomics,
// nothing synchronises with the host, every floating-point sum has a fixed order: two runs give the same bits.
//
// Layout: a workgroup of 256 lanes, a ray per lane, a grid-stride loop; at most RL_MAX_PARTIALS workgroups, so that the last one's two
// rows of partials fit the LDS it hands to sn_reduce.h (2 x 512 doubles = 8 KiB).  A lane adds its rays' d^2 (three per ray, c ascending)
// and e in ascending ray order, each in its own double; both go through the ticket reduction (publish_and_draw2 / sum_partials2).  The
// workgroup that draws the last ticket divides, reads the extras, stores the record and returns the workspace to zero.
//
// Non-finite values: the comparisons of the clamp are written so that a NaN stays a NaN, as torch.clamp keeps it, and
// torch's clamp backward (inclusive bounds, false for a NaN) decides the entropy gradient; everything else is the same chain of fp32
// operations torch runs, so a NaN or Inf reaches the outputs it reaches there.
#include "sn_reduce.h"

namespace sn {

constexpr uint32_t RL_THREADS = SN_REDUCE_THREADS;
constexpr uint32_t RL_MAX_PARTIALS = SN_RGB_LOSS_MAX_WORKGROUPS;     // workgroups of k_rgb_loss (a lane loops over rays beyond)

struct RgbLossWorkspace {
    uint32_t ticket, pad[15];
    double part_sq[RL_MAX_PARTIALS];
    double part_ent[RL_MAX_PARTIALS];
};
static_assert(sizeof(RgbLossWorkspace) == SN_RGB_LOSS_WORKSPACE_BYTES && SN_RGB_LOSS_WORKSPACE_BYTES % 8 == 0, "the workspace constant of the header");
static_assert(sizeof(sn_rgb_loss_record) == 16, "four floats");

struct RgbLossArgs {
    const float *image, *weights_sum, *truth, *bg, *extra0, *extra1;
    float *pred, *gt, *grad_image, *grad_ws;                            // each may be NULL
    sn_rgb_loss_record *record;
    RgbLossWorkspace *ws;
    uint32_t image_stride, truth_stride, N;
    float bg_value, lambda_entropy, coef0, coef1;
};

// torch.clamp(x, lo, hi) at every input: a NaN fails both comparisons and stays
__device__ __forceinline__ float clamp_keep_nan(float x, float lo, float hi) {
    float c = x < lo ? lo : x;
    c = c > hi ? hi : c;
    return c;
}

// RGBA: truth has four channels; BG: 0 = bg_value, 1 = one colour, 2 = a colour per ray; HAS_BG: image already contains its background term
template <bool RGBA, int BG, bool HAS_BG>
__global__ __launch_bounds__(256) void k_rgb_loss(const RgbLossArgs a) {
    SN_POISON_ALL();
    __shared__ double s_part[2 * RL_MAX_PARTIALS];
    __shared__ double s_wave[8];
    __shared__ uint32_t s_flag;
    const uint32_t tid = threadIdx.x;
    const bool entropy_on = a.lambda_entropy != 0.0f;
    const float lo = 1e-5f, hi = (float)(1.0 - 1e-5);
    const float inv_n3 = 1.0f / (float)(3u * a.N);                      // N < 2^30: 3 N fits
    const float ent_coef = a.lambda_entropy / (float)a.N;
    float b1[3] = {a.bg_value, a.bg_value, a.bg_value};
    if (BG == 1) { b1[0] = a.bg[0]; b1[1] = a.bg[1]; b1[2] = a.bg[2]; }

    double sq = 0.0, ent = 0.0;
    for (uint32_t i = blockIdx.x * RL_THREADS + tid; i < a.N; i += gridDim.x * RL_THREADS) {
        const float *im = a.image + (size_t)i * a.image_stride, *tr = a.truth + (size_t)i * a.truth_stride;
        const float w = a.weights_sum[i];
        float b[3] = {b1[0], b1[1], b1[2]};
        if (BG == 2) { b[0] = a.bg[(size_t)3 * i]; b[1] = a.bg[(size_t)3 * i + 1]; b[2] = a.bg[(size_t)3 * i + 2]; }
        const float alpha = RGBA ? tr[3] : 1.0f;
        const float one_minus_a = 1.0f - alpha, one_minus_w = 1.0f - w;
        float g[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gt = RGBA ? tr[c] * alpha + b[c] * one_minus_a : tr[c];
            const float pred = HAS_BG ? im[c] : im[c] + one_minus_w * b[c];
            const float d = pred - gt;
            sq += (double)d * (double)d;
            g[c] = (2.0f * d) * inv_n3;
            if (a.pred) a.pred[(size_t)3 * i + c] = pred;
            if (a.gt) a.gt[(size_t)3 * i + c] = gt;
            if (a.grad_image) a.grad_image[(size_t)3 * i + c] = g[c];
        }
        float gw = HAS_BG ? 0.0f : -((g[0] * b[0] + g[1] * b[1]) + g[2] * b[2]);
        if (entropy_on) {
            const float c = clamp_keep_nan(w, lo, hi), omc = 1.0f - c;
            const float l0 = log2f(c), l1 = log2f(omc);
            const float e = (-c) * l0 - omc * l1;
            ent += (double)e;
            if (w >= lo && w <= hi) gw = gw + ent_coef * (l1 - l0);
        }
        if (a.grad_ws) a.grad_ws[i] = gw;
    }

    if (!publish_and_draw2(sq, ent, &a.ws->ticket, a.ws->part_sq, a.ws->part_ent, s_wave, &s_flag)) return;
    double ent_total;
    const double sq_total = sum_partials2(a.ws->part_sq, a.ws->part_ent, s_part, s_part + RL_MAX_PARTIALS, &ent_total);
    if (tid == 0) {
        const float mse = (float)(sq_total / (3.0 * (double)a.N));
        const float entropy = entropy_on ? (float)(ent_total / (double)a.N) : 0.0f;
        float total = mse + a.lambda_entropy * entropy;
        if (a.extra0) total = total + a.coef0 * *a.extra0;
        if (a.extra1) total = total + a.coef1 * *a.extra1;
        a.record->total = total;
        a.record->mse = mse;
        a.record->entropy = entropy;
        a.record->reserved = 0.0f;
        __hip_atomic_store(&a.ws->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool RGBA, int BG>
static void launch_rgb_loss(bool has_bg, uint32_t blocks, hipStream_t st, const RgbLossArgs &a) {
    if (has_bg) hipLaunchKernelGGL((k_rgb_loss<RGBA, BG, true>), dim3(blocks), dim3(RL_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_rgb_loss<RGBA, BG, false>), dim3(blocks), dim3(RL_THREADS), 0, st, a);
}

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_rgb_loss(const float *image, uint32_t image_stride, const float *weights_sum, const float *truth, uint32_t truth_stride,
                   uint32_t truth_channels, uint32_t N, float bg_value, const float *bg, uint32_t bg_rows, int image_has_bg, float lambda_entropy,
                   const float *extra0, float coef0, const float *extra1, float coef1, float *pred_rgb, float *gt_rgb, sn_rgb_loss_record *record,
                   float *grad_image, float *grad_weights_sum, void *workspace, sn_stream_t stream) {
    SN_REQUIRE(image && weights_sum && truth && record && workspace, "rgb_loss: NULL pointer (image, weights_sum, truth, record and workspace are required)");
    SN_REQUIRE(truth_channels == 3 || truth_channels == 4, "rgb_loss: truth_channels %u must be 3 or 4", truth_channels);
    SN_REQUIRE(image_stride >= 3, "rgb_loss: image_stride %u floats is less than 3", image_stride);
    SN_REQUIRE(truth_stride >= truth_channels, "rgb_loss: truth_stride %u floats is less than truth_channels = %u", truth_stride, truth_channels);
    SN_REQUIRE(N >= 1, "rgb_loss: N must be at least 1");
    SN_REQUIRE(bg_rows == 0 || bg_rows == 1 || bg_rows == N, "rgb_loss: bg_rows %u must be 0, 1 or N = %u", bg_rows, N);
    SN_REQUIRE(bg_rows == 0 || bg, "rgb_loss: NULL bg with bg_rows = %u", bg_rows);
    SN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "rgb_loss: workspace must be 8-byte aligned");
    SN_UNSUPPORTED(N < (1u << 30), "rgb_loss: N = %u must stay below 2^30", N);
    RgbLossArgs a;
    a.image = image; a.weights_sum = weights_sum; a.truth = truth; a.bg = bg_rows ? bg : nullptr; a.extra0 = extra0; a.extra1 = extra1;
    a.pred = pred_rgb; a.gt = gt_rgb; a.grad_image = grad_image; a.grad_ws = grad_weights_sum;
    a.record = record; a.ws = static_cast<RgbLossWorkspace *>(workspace);
    a.image_stride = image_stride; a.truth_stride = truth_stride; a.N = N;
    a.bg_value = bg_value; a.lambda_entropy = lambda_entropy; a.coef0 = coef0; a.coef1 = coef1;
    const uint32_t need = div_up(N, RL_THREADS), blocks = need < RL_MAX_PARTIALS ? need : RL_MAX_PARTIALS;
    hipStream_t st = (hipStream_t)stream;
    const bool rgba = truth_channels == 4, has_bg = image_has_bg != 0;
    const int mode = bg_rows == 0 ? 0 : (bg_rows == 1 ? 1 : 2);          // N == 1 with bg_rows == 1: one colour, the same thing
    if (rgba) {
        if (mode == 0) launch_rgb_loss<true, 0>(has_bg, blocks, st, a);
        else if (mode == 1) launch_rgb_loss<true, 1>(has_bg, blocks, st, a);
        else launch_rgb_loss<true, 2>(has_bg, blocks, st, a);
    } else {
        if (mode == 0) launch_rgb_loss<false, 0>(has_bg, blocks, st, a);
        else if (mode == 1) launch_rgb_loss<false, 1>(has_bg, blocks, st, a);
        else launch_rgb_loss<false, 2>(has_bg, blocks, st, a);
    }
    SN_LAUNCH_CHECK("k_rgb_loss");
    return SN_OK;
}

}  // extern "C"
