// object.hip — render a segmented object alone: the gated re-integration of a ray (sn_rm_object_composite), for gfx950.
//
// Definition (include/sanerf_hip.h states it in full; tests/object_ref64.py is its fp64 twin).  For one ray and the T samples of the last stage,
// with densities sigma_i, real bin edges b_0 .. b_T, per-sample labels (sn_rm_mask_point_labels) and the 15 geometry channels geo_i:
//   g_i  = (label_i in S) xor invert                    S = the set bits of keep_mask; a label >= 32 (255 = "not evaluated") is in no S
//   y_i  = g_i ? (b_{i+1} - b_i) * sigma_i : 0          a select, not a product: a gated-out sigma = inf gives 0, not NaN
//          last_sample_opaque: y_{T-1} = g_{T-1} ? +inf : 0
//   w'_i = (1 - exp(-y_i)) * exp(-sum_{j<i} y_j)        NaN -> 0, as sn_rm_weights_from_sigma
//   weights_sum = sum w'_i;  depth = sum w'_i t_i, t_i = (b_{i+1} + b_i) / 2;  f_image = [sum w'_i geo_i | SH4(d / |d|) * weights_sum]
// w'_i can be non-zero where the ordinary weight is exactly 0 (the occluder in front is gated away), so nothing here is keyed on a weight.
//
// Shape: k_ray_composite's -- 16 lanes per ray, lane 0 owns weights_sum and depth, lane c >= 1 geometry channel c - 1, SH once per ray -- with
// the transmittance scan inside: per block of 16 samples lane c makes y of sample 16 b + c, the exclusive prefix is summed in fp64 in sample
// order (every lane adds the same 16 values in the same order, as k_weights_wave), lane c makes w' of its sample, and the 16 weights go round
// the group in sample order for the channel sums.  The order of every sum is a function of T alone: results do not depend on N or on the
// launch grid.  Plain vector loads and stores.
#include "sn_common.h"
#include "sh_basis.inc"

namespace sn {

constexpr uint32_t OBJ_GEO = 15;          // geometry channels of the reference field (network.py:94: grid_mlp's 16 outputs but sigma)

__global__ __launch_bounds__(256) void k_object_composite(const uint8_t *__restrict__ labels, const float *__restrict__ sigmas,
                                                          const float *__restrict__ real_bins, const float *__restrict__ geo,
                                                          const float *__restrict__ rays_d, uint32_t N, uint32_t T, uint32_t keep_mask, int invert,
                                                          int last_opaque, float *__restrict__ wsum, float *__restrict__ depth,
                                                          float *__restrict__ f_image, float *__restrict__ weights) {
    SN_POISON_ALL();
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x, n_raw = gid >> 4, c = gid & 15u;
    const uint32_t n = n_raw < N ? n_raw : N - 1u;
    const bool store = n_raw < N;
    const float *rb = real_bins + (size_t)n * (T + 1u), *sg = sigmas + (size_t)n * T, *gf = geo + (size_t)n * T * OBJ_GEO + (c ? c - 1u : 0u);
    const uint8_t *lb = labels + (size_t)n * T;
    double cum = 0.0;                      // sum of y over the samples in front of the current block
    float acc = 0.0f, dsum = 0.0f;
    for (uint32_t j0 = 0; j0 < T; j0 += 16u) {
        const uint32_t j = j0 + c;
        const bool live = j < T;
        float y = 0.0f, tm = 0.0f;
        if (live) {
            const float b0 = rb[j], b1 = rb[j + 1u];
            const uint32_t lab = lb[j];
            const bool in_set = lab < 32u && ((keep_mask >> lab) & 1u) != 0u;
            const bool gate = in_set != (invert != 0);
            const float ds = (b1 - b0) * sg[j];
            y = gate ? ((last_opaque && j == T - 1u) ? __builtin_inff() : ds) : 0.0f;
            tm = (b1 + b0) / 2.0f;        // k_sample_positions' mid-point
        }
        double excl = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float d = __shfl(y, q, 16);
            if (c == (uint32_t)q) excl = cum;
            cum += (double)d;
        }
        float w = 0.0f;
        if (live) {
            const float alpha = 1.0f - expf_det(-y);
            const float tr = expf_det(-(float)excl);
            w = alpha * tr;
            if (w != w) w = 0.0f;
            if (weights && store) weights[(size_t)n * T + j] = w;
        }
        const uint32_t cnt = T - j0 < 16u ? T - j0 : 16u;
        for (uint32_t q = 0; q < cnt; ++q) {
            const float wq = __shfl(w, (int)q, 16), tq = __shfl(tm, (int)q, 16);
            if (c == 0u) { acc += wq; dsum = __builtin_fmaf(wq, tq, dsum); }
            else acc = __builtin_fmaf(wq, gf[(size_t)(j0 + q) * OBJ_GEO], acc);
        }
    }
    const float ws = __shfl(acc, 0, 16);
    float x = rays_d[(size_t)n * 3], yd = rays_d[(size_t)n * 3 + 1], z = rays_d[(size_t)n * 3 + 2];
    const float inv = 1.0f / sqrtf(x * x + yd * yd + z * z);               // renderer.py:294
    x *= inv; const float y = yd * inv; z *= inv;
    float sh[16];
    {
        const unsigned C = 4u;
        SN_SH_POWERS
        (void)x4; (void)x5; (void)x6; (void)x7; (void)y4; (void)y5; (void)y6; (void)y7; (void)z4; (void)z5; (void)z6; (void)z7;
        SN_SH_VALUES(sh);
    }
    float mine = sh[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) mine = c == (uint32_t)k ? sh[k] : mine;
    if (!store) return;
    float *f = f_image + (size_t)n * 31u;
    if (c == 0u) { wsum[n] = acc; depth[n] = dsum; }
    else f[c - 1u] = acc;
    f[15u + c] = mine * ws;
}

}  // namespace sn

using namespace sn;

extern "C" int sn_rm_object_composite(const uint8_t *labels, const float *sigmas, const float *real_bins, const float *geo_feat, const float *rays_d,
                                      uint32_t N, uint32_t T, uint32_t keep_mask, int32_t invert, int32_t last_sample_opaque, float *weights_sum,
                                      float *depth, float *f_image, float *weights, sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(labels && sigmas && real_bins && geo_feat && rays_d && weights_sum && depth && f_image, "object_composite: NULL pointer");
    SN_REQUIRE(T >= 1u, "object_composite: T must be >= 1");
    SN_REQUIRE((uint64_t)N * 16u < (1ull << 32), "object_composite: at most 2^28 - 1 rays per call (got %u)", N);
    hipLaunchKernelGGL(k_object_composite, dim3(div_up((uint64_t)N * 16u, 256)), dim3(256), 0, (hipStream_t)stream, labels, sigmas, real_bins, geo_feat,
                       rays_d, N, T, keep_mask, (int)invert, (int)last_sample_opaque, weights_sum, depth, f_image, weights);
    SN_LAUNCH_CHECK("k_object_composite");
    return SN_OK;
}
