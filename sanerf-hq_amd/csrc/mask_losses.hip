// mask_losses.hip — the object-field ("mask mode") training extras of nerf/trainer.py for gfx950: the ray-pair RGB loss (:260-305), the
// error measure exp(-w cos(p, onehot(gt)) - eps) of the per-step error-map EMA (:457-464) and of the whole-map rebuild (:1424-1432).
//
// The reference states each of them as a chain of torch element-wise ops plus torch.multinomial; here each is one launch (the EMA: two, so
// that every new value is computed from the map as it was before the call), without atomics: every sum has a fixed order and two runs give
// the same bits.  exp is sn::expf_det, division and sqrt are IEEE-rounded (Makefile flags), nothing is contracted into an fma.
#include "sn_reduce.h"

namespace sn {

constexpr uint32_t RP_MAX_S = 64;        // samples (pairs) per group
constexpr uint32_t RP_MAX_K = 32;        // instances
constexpr float COS_EPS = 1e-8f;         // F.cosine_similarity's eps

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// One row of `masks` as probabilities in registers: the softmax of torch (exp(x - max) / sum, ascending k) when the row holds logits.
template <int KT>
__device__ __forceinline__ void load_probs(const float *__restrict__ row, uint32_t K, bool from_logits, float (&p)[KT]) {
#pragma unroll
    for (int k = 0; k < KT; ++k) p[k] = (uint32_t)k < K ? row[k] : 0.0f;
    if (from_logits) softmax_row<KT>(p, K);
}

template <int KT>
__device__ __forceinline__ float norm2(const float (&p)[KT]) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < KT; ++k) s += p[k] * p[k];       // entries past K are 0
    return sqrtf(s);
}

// Step 1 of the ray-pair loss without torch.multinomial: the S candidates of a group with the smallest uniform value (lower index first
// on a tie), in ascending order of that value.  One wave per group; round r finds the smallest (value, index) key above round r-1's.
__global__ __launch_bounds__(256) void k_ray_pair_select(const float *__restrict__ incoherent, const float *__restrict__ uniform, uint32_t G,
                                                         uint32_t P, uint32_t S, int64_t *__restrict__ sample_index) {
    SN_POISON_ALL();
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (g >= G) return;
    const float *inc = incoherent + (size_t)g * P, *u = uniform + (size_t)g * P;
    uint32_t mine = 0;
    for (uint32_t i = lane; i < P; i += 64u) mine += (1.0f - inc[i]) > 0.8f ? 1u : 0u;
    const uint32_t cand = wave_sum(mine);
    const bool all = cand == 0u;                     // trainer.py:270-273: a group without candidates draws from all its pixels
    uint64_t prev = 0;
    bool have_prev = false;
    for (uint32_t r = 0; r < S; ++r) {
        uint64_t best = ~0ull;
        for (uint32_t i = lane; i < P; i += 64u) {
            if (!all && !((1.0f - inc[i]) > 0.8f)) continue;
            uint32_t b = __float_as_uint(u[i] + 0.0f);                       // -0 -> +0
            b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;                      // float order -> unsigned order
            const uint64_t key = ((uint64_t)b << 32) | i;
            if (have_prev && key <= prev) continue;
            best = key < best ? key : best;
        }
        best = wave_min_u64(best);
        if (lane == 0) sample_index[(size_t)g * S + r] = best == ~0ull ? (int64_t)-1 : (int64_t)(best & 0xffffffffu);
        if (best == ~0ull) {                         // fewer candidates than slots: the rest are no pairs
            if (lane == 0) for (uint32_t q = r + 1; q < S; ++q) sample_index[(size_t)g * S + q] = -1;
            break;
        }
        prev = best; have_prev = true;
    }
}

// trainer.py:276-303 for one group per workgroup, value and gradient.
//   phase 0: the sampled pixels' colours and (detached) mask vectors q into LDS; the number of pairs of the whole call (every workgroup reads
//            all G * S indices for it: 8 G S bytes from L2 per group, nothing beside the group's own G-independent work up to a few thousand
//            groups -- the loss is built for the handful of local patches of a training step, see the header)
//   phase A: one wave owns a pair, lane = pixel (64-pixel strides): match count by ballot / popcount, masked sum of exp(-w cos - eps)
//   phase B: one lane owns a pixel and walks the group's pairs in ascending s: its gradient over all pairs, stored once
template <int KT>
__global__ __launch_bounds__(256) void k_ray_pair_rgb_loss(const float *__restrict__ rgb, const float *__restrict__ masks, int from_logits,
                                                           const int64_t *__restrict__ sample_index, uint32_t G, uint32_t P, uint32_t S, uint32_t K,
                                                           float thr, float w, float eps, int use_pred, float scale,
                                                           const float *__restrict__ scale_dev, float *__restrict__ loss_per_pair,
                                                           float *__restrict__ pair_count, float *__restrict__ grad_masks) {
    SN_POISON_ALL();
    __shared__ float s_q[RP_MAX_S][KT];              // q / max(|q|, 1e-8)
    __shared__ float s_rgb[RP_MAX_S][3];
    __shared__ float s_coef[RP_MAX_S];               // total scale / match count of the pair (0: no pair)
    __shared__ int32_t s_idx[RP_MAX_S];
    __shared__ uint32_t s_cnt[4];
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float *grgb = rgb + (size_t)g * P * 3;
    const float *gm = masks + (size_t)g * P * K;

    // phase 0
    uint32_t valid = 0;
    for (uint64_t t = tid; t < (uint64_t)G * S; t += 256u) {
        const int64_t v = sample_index[t];
        valid += (v >= 0 && v < (int64_t)P) ? 1u : 0u;
    }
    valid = wave_sum(valid);
    if (lane == 0) s_cnt[wave] = valid;
    if (tid < S) {
        const int64_t v = sample_index[(size_t)g * S + tid];
        const bool ok = v >= 0 && v < (int64_t)P;    // -1 (or anything outside the group) is no pair and is never dereferenced
        s_idx[tid] = ok ? (int32_t)v : -1;
        float q[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) q[k] = 0.0f;
        if (ok) {
            load_probs<KT>(gm + (size_t)v * K, K, from_logits != 0, q);
            if (!use_pred) {                         // trainer.py:284-287: one-hot of the argmax (first maximum)
                int arg = 0;
                float best = q[0];
#pragma unroll
                for (int k = 1; k < KT; ++k) if ((uint32_t)k < K && q[k] > best) { best = q[k]; arg = k; }
#pragma unroll
                for (int k = 0; k < KT; ++k) q[k] = k == arg ? 1.0f : 0.0f;
            }
            const float qn = fmaxf(norm2<KT>(q), COS_EPS);
#pragma unroll
            for (int k = 0; k < KT; ++k) q[k] = q[k] / qn;
            for (int c = 0; c < 3; ++c) s_rgb[tid][c] = grgb[(size_t)v * 3 + c];
        } else {
            for (int c = 0; c < 3; ++c) s_rgb[tid][c] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) s_q[tid][k] = q[k];
    }
    __syncthreads();
    const uint32_t n_pairs = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (pair_count && g == 0 && tid == 0) *pair_count = (float)(n_pairs ? n_pairs : 1u);
    const float total = n_pairs ? scale * (scale_dev ? *scale_dev : 1.0f) / (float)n_pairs : 0.0f;

    // phase A
    for (uint32_t s = wave; s < S; s += 4u) {
        if (s_idx[s] < 0) {
            if (lane == 0) { s_coef[s] = 0.0f; if (loss_per_pair) loss_per_pair[(size_t)g * S + s] = 0.0f; }
            continue;
        }
        const float r0 = s_rgb[s][0], r1 = s_rgb[s][1], r2 = s_rgb[s][2];
        uint32_t cnt = 0;
        float acc = 0.0f;
        for (uint32_t base = 0; base < P; base += 64u) {
            const uint32_t i = base + lane;
            bool sim = false;
            float e = 0.0f;
            if (i < P) {
                const float dx = grgb[(size_t)i * 3] - r0, dy = grgb[(size_t)i * 3 + 1] - r1, dz = grgb[(size_t)i * 3 + 2] - r2;
                sim = sqrtf(dx * dx + dy * dy + dz * dz) < thr;
                if (sim) {
                    float p[KT];
                    load_probs<KT>(gm + (size_t)i * K, K, from_logits != 0, p);
                    const float pn = fmaxf(norm2<KT>(p), COS_EPS);
                    float dot = 0.0f;
#pragma unroll
                    for (int k = 0; k < KT; ++k) dot += p[k] * s_q[s][k];
                    e = expf_det(-w * (dot / pn) - eps);
                }
            }
            cnt += (uint32_t)__popcll(__ballot(sim));
            acc += e;
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            s_coef[s] = cnt ? total / (float)cnt : 0.0f;
            if (loss_per_pair) loss_per_pair[(size_t)g * S + s] = acc / (float)cnt;      // 0 matches (NaN colours): 0 / 0 like the reference
        }
    }
    if (!grad_masks) return;
    __syncthreads();

    // phase B: d pair / d p_i = sim / count * (-w) e * d cos / d p_i, with d cos / d p = (q^ - cos p / |p|) / |p| (q^ = q / max(|q|, 1e-8))
    for (uint32_t i = tid; i < P; i += 256u) {
        float p[KT], a[KT];
        load_probs<KT>(gm + (size_t)i * K, K, from_logits != 0, p);
        const float pnr = norm2<KT>(p), pn = fmaxf(pnr, COS_EPS);
        const float x = grgb[(size_t)i * 3], y = grgb[(size_t)i * 3 + 1], z = grgb[(size_t)i * 3 + 2];
#pragma unroll
        for (int k = 0; k < KT; ++k) a[k] = 0.0f;
        float bsum = 0.0f;
        for (uint32_t s = 0; s < S; ++s) {
            const float coef = s_coef[s];
            if (coef == 0.0f) continue;
            const float dx = x - s_rgb[s][0], dy = y - s_rgb[s][1], dz = z - s_rgb[s][2];
            if (!(sqrtf(dx * dx + dy * dy + dz * dz) < thr)) continue;
            float dot = 0.0f;
#pragma unroll
            for (int k = 0; k < KT; ++k) dot += p[k] * s_q[s][k];
            const float cs = dot / pn;
            const float f = coef * (-w) * expf_det(-w * cs - eps);
#pragma unroll
            for (int k = 0; k < KT; ++k) a[k] += f * s_q[s][k];
            bsum += f * cs;
        }
        // |p| above the clamp: (a - bsum p / |p|) / |p|;  at or below it the denominator is the constant 1e-8: a / 1e-8
        const bool clamped = !(pnr > COS_EPS);
        float gsum = 0.0f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            a[k] = clamped ? a[k] / COS_EPS : (a[k] - bsum * (p[k] / pn)) / pn;
            gsum += a[k] * p[k];
        }
        float *out = grad_masks + ((size_t)g * P + i) * K;
        if (from_logits) {                           // softmax backward: p_k (g_k - sum_j g_j p_j)
#pragma unroll
            for (int k = 0; k < KT; ++k) a[k] = p[k] * (a[k] - gsum);
        }
        if (K == 2u && (((uintptr_t)out) & 7u) == 0) {
            *reinterpret_cast<float2 *>(out) = make_float2(a[0], a[1]);
        } else if constexpr (KT >= 4) {
            if (K == 4u && (((uintptr_t)out) & 15u) == 0) {
                *reinterpret_cast<float4 *>(out) = make_float4(a[0], a[1], a[2], a[3]);
            } else {
#pragma unroll
                for (int k = 0; k < KT; ++k) if ((uint32_t)k < K) out[k] = a[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < KT; ++k) if ((uint32_t)k < K) out[k] = a[k];
        }
    }
}

// error[n] = exp(-w cos(p_n, onehot(label_n)) - eps) = exp(-w p[label] / max(|p|, 1e-8) - eps); a label outside 0..K-1: the zero vector.
__device__ __forceinline__ float mask_error_one(const float *__restrict__ row, uint32_t K, bool from_logits, int64_t y, float w, float eps) {
    float mx = 0.0f, sum = 1.0f;
    if (from_logits) {
        mx = row[0];
        for (uint32_t k = 1; k < K; ++k) mx = fmaxf(mx, row[k]);
        sum = 0.0f;
        for (uint32_t k = 0; k < K; ++k) sum += expf_det(row[k] - mx);
    }
    float sq = 0.0f, py = 0.0f;
    for (uint32_t k = 0; k < K; ++k) {
        const float pk = from_logits ? expf_det(row[k] - mx) / sum : row[k];
        sq += pk * pk;
        if ((int64_t)k == y) py = pk;
    }
    const float cs = py / fmaxf(sqrtf(sq), COS_EPS);
    return expf_det(-w * cs - eps);
}

__global__ __launch_bounds__(256) void k_mask_error(const float *__restrict__ masks, int from_logits, const int64_t *__restrict__ labels, uint32_t N,
                                                    uint32_t K, float w, float eps, float *__restrict__ error) {
    SN_POISON_ALL();
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    error[n] = mask_error_one(masks + (size_t)n * K, K, from_logits != 0, labels[n], w, eps);
}

// trainer.py:457-464, first launch: every new map value from the map as it is (nothing is written to the map here)
__global__ __launch_bounds__(256) void k_error_map_stage(const float *__restrict__ masks, int from_logits, const int64_t *__restrict__ labels,
                                                         const int64_t *__restrict__ rows, uint32_t row_step, const int64_t *__restrict__ cols,
                                                         uint32_t N, uint32_t K, float w, float eps, uint32_t map_rows, uint32_t row_stride,
                                                         const float *__restrict__ error_map, float *__restrict__ stage, float *__restrict__ error) {
    SN_POISON_ALL();
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float e = mask_error_one(masks + (size_t)n * K, K, from_logits != 0, labels[n], w, eps);
    if (error) error[n] = e;
    const int64_t r = rows[(size_t)n * row_step], c = cols[n];
    const bool inside = r >= 0 && r < (int64_t)map_rows && c >= 0 && c < (int64_t)row_stride;
    stage[n] = inside ? 0.1f * error_map[(size_t)r * row_stride + (size_t)c] + 0.9f * e : 0.0f;
}

// second launch: the scatter (duplicate targets: one of their values stays)
__global__ __launch_bounds__(256) void k_error_map_scatter(const int64_t *__restrict__ rows, uint32_t row_step, const int64_t *__restrict__ cols, uint32_t N,
                                                           uint32_t map_rows, uint32_t row_stride, const float *__restrict__ stage,
                                                           float *__restrict__ error_map) {
    SN_POISON_ALL();
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int64_t r = rows[(size_t)n * row_step], c = cols[n];
    if (r >= 0 && r < (int64_t)map_rows && c >= 0 && c < (int64_t)row_stride) error_map[(size_t)r * row_stride + (size_t)c] = stage[n];
}

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_ray_pair_select(const float *incoherent, const float *uniform, uint32_t G, uint32_t P, uint32_t S, int64_t *sample_index,
                          sn_stream_t stream) {
    if (G == 0 || S == 0) return SN_OK;
    SN_REQUIRE(incoherent && uniform && sample_index, "ray_pair_select: NULL pointer");
    SN_REQUIRE(P >= 1, "ray_pair_select: at least one pixel per group");
    SN_UNSUPPORTED(S <= RP_MAX_S, "ray_pair_select: at most %u samples per group (got %u)", RP_MAX_S, S);
    SN_UNSUPPORTED((uint64_t)G * P < (1ull << 31), "ray_pair_select: G * P must stay below 2^31 (got %u x %u)", G, P);
    hipLaunchKernelGGL(k_ray_pair_select, dim3(div_up(G, 4)), dim3(256), 0, (hipStream_t)stream, incoherent, uniform, G, P, S, sample_index);
    SN_LAUNCH_CHECK("k_ray_pair_select");
    return SN_OK;
}

int sn_rm_ray_pair_rgb_loss(const float *rgb, const float *masks, int from_logits, const int64_t *sample_index, uint32_t G, uint32_t P, uint32_t S,
                            uint32_t K, float thr, float w, float eps, int use_pred_logistics, float scale, const float *scale_dev,
                            float *loss_per_pair, float *pair_count, float *grad_masks, sn_stream_t stream) {
    if (G == 0) return SN_OK;
    SN_REQUIRE(rgb && masks && sample_index, "ray_pair_rgb_loss: NULL pointer");
    SN_REQUIRE(loss_per_pair || grad_masks, "ray_pair_rgb_loss: neither loss_per_pair nor grad_masks given");
    SN_REQUIRE(P >= 1 && S >= 1 && K >= 1, "ray_pair_rgb_loss: G, P, S, K must be >= 1 (got P=%u S=%u K=%u)", P, S, K);
    SN_REQUIRE(thr > 0.0f, "ray_pair_rgb_loss: the colour threshold must be > 0 (a sampled pixel has to match itself), got %g", (double)thr);
    SN_UNSUPPORTED(K <= RP_MAX_K, "ray_pair_rgb_loss: at most %u instances (got K=%u)", RP_MAX_K, K);
    SN_UNSUPPORTED(S <= RP_MAX_S, "ray_pair_rgb_loss: at most %u samples per group (got S=%u)", RP_MAX_S, S);
    SN_UNSUPPORTED((uint64_t)G * P < (1ull << 31), "ray_pair_rgb_loss: G * P must stay below 2^31 (got %u x %u)", G, P);
    hipStream_t st = (hipStream_t)stream;
#define SN_RP_LAUNCH(KT)                                                                                                                       \
    hipLaunchKernelGGL(k_ray_pair_rgb_loss<KT>, dim3(G), dim3(256), 0, st, rgb, masks, from_logits, sample_index, G, P, S, K, thr, w, eps,        \
                       use_pred_logistics, scale, scale_dev, loss_per_pair, pair_count, grad_masks)
    SN_DISPATCH_KT(K, SN_RP_LAUNCH);
#undef SN_RP_LAUNCH
    SN_LAUNCH_CHECK("k_ray_pair_rgb_loss");
    return SN_OK;
}

int sn_rm_mask_error(const float *masks, int from_logits, const int64_t *labels, uint32_t N, uint32_t K, float w, float eps, float *error,
                     sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(masks && labels && error, "mask_error: NULL pointer");
    SN_REQUIRE(K >= 1, "mask_error: at least one instance");
    hipLaunchKernelGGL(k_mask_error, dim3(div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, masks, from_logits, labels, N, K, w, eps, error);
    SN_LAUNCH_CHECK("k_mask_error");
    return SN_OK;
}

int sn_rm_error_map_update(const float *masks, int from_logits, const int64_t *labels, const int64_t *rows, uint32_t n_rows, const int64_t *cols,
                           uint32_t N, uint32_t K, float w, float eps, uint32_t map_rows, uint32_t row_stride, float *error_map, float *stage,
                           float *error, sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(masks && labels && rows && cols && error_map && stage, "error_map_update: NULL pointer");
    SN_REQUIRE(K >= 1, "error_map_update: at least one instance");
    SN_REQUIRE(n_rows == 1 || n_rows == N, "error_map_update: %u map rows for %u rays (must be 1 or N)", n_rows, N);
    SN_REQUIRE(map_rows >= 1 && row_stride >= 1, "error_map_update: empty error map (%u x %u)", map_rows, row_stride);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t row_step = n_rows == 1 ? 0u : 1u;
    hipLaunchKernelGGL(k_error_map_stage, dim3(div_up(N, 256)), dim3(256), 0, st, masks, from_logits, labels, rows, row_step, cols, N, K, w, eps,
                       map_rows, row_stride, error_map, stage, error);
    SN_LAUNCH_CHECK("k_error_map_stage");
    hipLaunchKernelGGL(k_error_map_scatter, dim3(div_up(N, 256)), dim3(256), 0, st, rows, row_step, cols, N, map_rows, row_stride, stage, error_map);
    SN_LAUNCH_CHECK("k_error_map_scatter");
    return SN_OK;
}

}  // extern "C"
