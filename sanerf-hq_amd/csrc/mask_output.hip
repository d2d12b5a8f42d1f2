// mask_output.hip — what the reference does between the mask field's logits and what a user sees or scores, for gfx950:
//   sn_rm_mask_output            test_step's mask branch (nerf/trainer.py:730-777 + the overlays of nerf/utils.py:49-77 + the (x * 255).astype(uint8)
//                                of :780-781): softmax / sigmoid, max, argmax, colour-table lookup, overlay, 8-bit image -- one launch per image
//   sn_rm_mask_eval_accumulate   eval_step's mask branch (trainer.py:599-627) plus MeanIoUMeter.update (nerf/metrics.py:165-179) and the
//                                loss.item() of evaluate_one_epoch (trainer.py:1603-1604) -- one launch per image, no host read
//   sn_rm_image_sqerr_accumulate MSEMeter.update / PSNRMeter.update (metrics.py:28-38, 217-221) -- one launch per image, no host read
//
// All three are streaming kernels: a workgroup owns tiles of 256 consecutive pixels, one lane per pixel, the K <= 32 logits of a pixel in
// registers.  Conventions of mask_losses.hip: exp is sn::expf_det, division is IEEE-rounded, nothing is contracted into an fma, no float
// atomics, every floating-point sum has a fixed order: two runs give the same bits, the accumulators included.
//
// Loads.  K <= 4: one vector load per lane (dword, dwordx2, 3 dwords, dwordx4) -- consecutive lanes read consecutive rows, a wave's
// load covers whole 128-byte lines.  K > 4: a lane-per-row load would touch 64 lines per instruction and use 4 bytes of each, so the
// tile's 256 * K floats -- one contiguous range -- are read as consecutive dwords (a wave instruction = two whole lines) into LDS rows of
// KT + 1 floats (odd stride: the row reads are bank-conflict free) and each lane picks up its row from there.  The probabilities leave
// the same way.
// Stores.  rgb8 is 3 bytes a pixel: the tile's 768 bytes (192 per wave) are staged in LDS and leave as 192 dword stores; only the
// last <= 3 bytes of an image whose size is not a multiple of 4 bytes are byte stores.  The float rgb is staged alike (consecutive dwords).
//
// The two accumulating kernels end with the ticket reduction of sn_reduce.h: a workgroup publishes its partial sum (and adds its LDS class
// histogram to the workspace's counts with one integer atomic per class), takes a ticket, and the workgroup that draws the last ticket
// sums the partials in ascending order, forms the image's values, adds them to the caller's record and puts the workspace back to zero.
// Nobody waits for anybody, the host reads nothing.
#include "sn_reduce.h"

namespace sn {

constexpr uint32_t MO_MAX_K = SN_MASK_MAX_CLASSES;
constexpr uint32_t MO_TILE = 256;                  // pixels per tile = threads per workgroup
constexpr uint32_t MO_MAX_PARTIALS = 512;          // workgroups of an accumulating launch (grid-stride over tiles beyond)

// workspace of the accumulating kernels (SN_MASK_EVAL_WORKSPACE_BYTES, zero at rest)
struct EvalWorkspace {
    uint32_t ticket, pad;
    unsigned long long counts[3 * MO_MAX_K];       // inter | pred | truth of the image at hand
    double part_sum[MO_MAX_PARTIALS];
    uint32_t part_cnt[MO_MAX_PARTIALS];
};
static_assert(sizeof(EvalWorkspace) <= SN_MASK_EVAL_WORKSPACE_BYTES, "the workspace constant of the header is too small");
static_assert(MO_TILE == SN_REDUCE_THREADS, "the accumulating kernels end with the reduction of sn_reduce.h");

static inline uint32_t mo_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

template <int KT> struct Tile {
    static constexpr bool STAGED = KT > 4;
    static constexpr int KP = KT + 1;              // LDS row stride in floats
    static constexpr int LDS_FLOATS = STAGED ? (int)MO_TILE * KP : 1;
};

// The tile's rows [n0, n0 + cnt) of a [N,K] array: row tid into x (entries past K, and lanes past cnt: 0).  Every lane of the workgroup calls it.
template <int KT>
__device__ __forceinline__ void tile_load(const float *__restrict__ base, uint32_t n0, uint32_t cnt, uint32_t K, float *s_rows, float (&x)[KT]) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < KT; ++k) x[k] = 0.0f;
    if constexpr (Tile<KT>::STAGED) {
        const float *src = base + (size_t)n0 * K;
        const uint32_t total = cnt * K, step_r = MO_TILE / K, step_c = MO_TILE % K;
        uint32_t r = tid / K, c = tid % K;
        for (uint32_t i = tid; i < total; i += MO_TILE) {          // i = r * K + c
            s_rows[r * Tile<KT>::KP + c] = src[i];
            r += step_r; c += step_c;
            if (c >= K) { c -= K; ++r; }
        }
        __syncthreads();
        if (tid < cnt) {
#pragma unroll
            for (int k = 0; k < KT; ++k) if ((uint32_t)k < K) x[k] = s_rows[tid * Tile<KT>::KP + k];
        }
    } else {
        if (tid >= cnt) return;
        const float *row = base + (size_t)(n0 + tid) * K;
        if (K == 2u && (((uintptr_t)base) & 7u) == 0) {
            const float2 v = *reinterpret_cast<const float2 *>(row);
            x[0] = v.x; x[1] = v.y;
        } else if (KT >= 4 && K == 4u && (((uintptr_t)base) & 15u) == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(row);
            x[0] = v.x; x[1] = v.y; x[KT >= 4 ? 2 : 0] = v.z; x[KT >= 4 ? 3 : 0] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < KT; ++k) if ((uint32_t)k < K) x[k] = row[k];
        }
    }
}

// The reverse: row tid of the tile from x.  Every lane of the workgroup calls it; s_rows is the buffer tile_load used (each lane has read
// only its own row of it, so it may be overwritten without a barrier in between).
template <int KT>
__device__ __forceinline__ void tile_store(float *__restrict__ base, uint32_t n0, uint32_t cnt, uint32_t K, float *s_rows, const float (&x)[KT]) {
    const uint32_t tid = threadIdx.x;
    if constexpr (Tile<KT>::STAGED) {
#pragma unroll
        for (int k = 0; k < KT; ++k) if ((uint32_t)k < K) s_rows[tid * Tile<KT>::KP + k] = x[k];
        __syncthreads();
        float *dst = base + (size_t)n0 * K;
        const uint32_t total = cnt * K, step_r = MO_TILE / K, step_c = MO_TILE % K;
        uint32_t r = tid / K, c = tid % K;
        for (uint32_t i = tid; i < total; i += MO_TILE) {
            dst[i] = s_rows[r * Tile<KT>::KP + c];
            r += step_r; c += step_c;
            if (c >= K) { c -= K; ++r; }
        }
    } else {
        if (tid >= cnt) return;
        float *row = base + (size_t)(n0 + tid) * K;
        if (K == 2u && (((uintptr_t)base) & 7u) == 0) {
            *reinterpret_cast<float2 *>(row) = make_float2(x[0], x[1]);
        } else if (KT >= 4 && K == 4u && (((uintptr_t)base) & 15u) == 0) {
            *reinterpret_cast<float4 *>(row) = make_float4(x[0], x[1], x[KT >= 4 ? 2 : 0], x[KT >= 4 ? 3 : 0]);
        } else {
#pragma unroll
            for (int k = 0; k < KT; ++k) if ((uint32_t)k < K) row[k] = x[k];
        }
    }
}

// trainer.py:734-739 / 608-613: K > 1: torch's softmax (exp(x - max) / sum, ascending k); K = 1: torch's sigmoid 1 / (1 + exp(-x)).
// A NaN or +inf logit (or a row of -inf) makes the whole row NaN, as in torch.  Then torch.max / argmax over the probabilities: the
// first maximum, a NaN counting as the greatest value.
template <int KT>
__device__ __forceinline__ void probs_argmax(float (&p)[KT], uint32_t K, int &arg, float &conf) {
    if (K == 1u) {
        p[0] = 1.0f / (1.0f + expf_det(-p[0]));
    } else {
        softmax_row<KT>(p, K);
    }
    arg = 0; conf = p[0];
#pragma unroll
    for (int k = 1; k < KT; ++k)
        if ((uint32_t)k < K && conf == conf && (p[k] > conf || p[k] != p[k])) { conf = p[k]; arg = k; }
}

template <int KT>
__device__ __forceinline__ float pick(const float (&p)[KT], int which) {
    // the bits of the one entry OR-ed out under a per-entry mask: a select chain over p[] is rewritten by the compiler into a dynamically
    // indexed load, which moves the whole row from registers to scratch
    uint32_t bits = 0u;
#pragma unroll
    for (int k = 0; k < KT; ++k) bits |= __float_as_uint(p[k]) & (k == which ? 0xffffffffu : 0u);
    return __uint_as_float(bits);
}

struct MaskOutArgs {
    const float *logits, *image, *color_map, *bg;
    uint32_t N, K, image_stride;
    int mode, render_id;
    float alpha;
    float *probs;
    int64_t *instance_id;
    float *confidence, *rgb;
    uint8_t *rgb8;
};

template <int KT>
__global__ __launch_bounds__(256) void k_mask_output(const MaskOutArgs a) {
    SN_POISON_ALL();
    __shared__ float s_rows[Tile<KT>::LDS_FLOATS];
    __shared__ float s_rgb[MO_TILE * 3];
    __shared__ uint32_t s_rgb8[MO_TILE * 3 / 4];
    const uint32_t tid = threadIdx.x, n0 = blockIdx.x * MO_TILE, cnt = umin(MO_TILE, a.N - n0), n = n0 + tid;
    const bool active = tid < cnt;
    float p[KT];
    tile_load<KT>(a.logits, n0, cnt, a.K, s_rows, p);
    int id;
    float conf;
    probs_argmax<KT>(p, a.K, id, conf);
    if (a.probs) tile_store<KT>(a.probs, n0, cnt, a.K, s_rows, p);
    if (active) {
        if (a.instance_id) a.instance_id[n] = (int64_t)id;
        if (a.confidence) a.confidence[n] = conf;
    }
    if (!a.rgb && !a.rgb8) return;                              // uniform over the workgroup

    float c[3] = {0.0f, 0.0f, 0.0f};
    if (active) {
        float img[3] = {0.0f, 0.0f, 0.0f};
        if (a.image) {
#pragma unroll
            for (int j = 0; j < 3; ++j) img[j] = a.image[(size_t)n * a.image_stride + j];
        }
        const int rid = a.render_id;
        if (a.mode == SN_MASK_OUT_HEATMAP) {                     // trainer.py:741-751, utils.py:63-77
            const bool one = rid >= 0 && rid < (int)a.K;
            const int cid = one ? rid : id;
            const float m = one ? pick<KT>(p, rid) : conf;
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = a.color_map[cid * 3 + j] * m;
        } else if (a.mode == SN_MASK_OUT_COMPOSITION) {          // trainer.py:752-762, utils.py:49-60
            const bool paint = rid == -1 || id == rid;
            const float rest = 1.0f - a.alpha;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float over = paint ? a.color_map[id * 3 + j] : img[j];
                c[j] = img[j] * a.alpha + over * rest;
            }
        } else if (a.mode == SN_MASK_OUT_MASK) {                 // trainer.py:763-777
            const float m = id == rid ? 1.0f : 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = img[j] * m + (1.0f - m) * a.bg[j];
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = img[j];
        }
    }
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
            const uint32_t i = tid + j * MO_TILE;
            if (i < cnt * 3u) dst[i] = s_rgb[i];
        }
    }
    if (a.rgb8 && tid < MO_TILE * 3 / 4) {
        uint8_t *dst = a.rgb8 + (size_t)n0 * 3;                  // n0 * 3 = blockIdx.x * 768: a dword boundary (the base is 4-byte aligned)
        const uint32_t bytes = cnt * 3u, b0 = tid * 4u;
        if (b0 + 4u <= bytes) {
            reinterpret_cast<uint32_t *>(dst)[tid] = s_rgb8[tid];
        } else {
            for (uint32_t b = b0; b < bytes; ++b) dst[b] = s_bytes[b];    // the image's last <= 3 bytes
        }
    }
}

template <int KT>
__global__ __launch_bounds__(256) void k_mask_eval_accumulate(const float *__restrict__ logits, const int64_t *__restrict__ labels, uint32_t N, uint32_t K,
                                                              uint32_t C, float eps, sn_eval_record *__restrict__ rec, EvalWorkspace *__restrict__ ws) {
    SN_POISON_ALL();
    __shared__ float s_rows[Tile<KT>::LDS_FLOATS];
    __shared__ uint32_t s_hist[3 * MO_MAX_K];                    // inter | pred | truth
    __shared__ double s_part[MO_MAX_PARTIALS];
    __shared__ uint32_t s_pcnt[MO_MAX_PARTIALS];
    __shared__ double s_wave[4];
    __shared__ uint32_t s_cnt[4], s_flag;
    __shared__ double s_iou[MO_MAX_K];
    __shared__ unsigned long long s_cls[3 * MO_MAX_K];
    const uint32_t tid = threadIdx.x;
    if (tid < 3 * MO_MAX_K) s_hist[tid] = 0u;
    __syncthreads();
    double sum = 0.0;
    uint32_t labelled = 0;
    const uint32_t tiles = (N + MO_TILE - 1) / MO_TILE;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t n0 = t * MO_TILE, cnt = umin(MO_TILE, N - n0);
        float p[KT];
        if (Tile<KT>::STAGED && t != blockIdx.x) __syncthreads();            // the previous tile's rows have been read
        tile_load<KT>(logits, n0, cnt, K, s_rows, p);
        if (tid >= cnt) continue;                                // (no barrier below in this iteration)
        int id;
        float conf;
        probs_argmax<KT>(p, K, id, conf);
        const int64_t y = labels[n0 + tid];
        // eval_step's loss (trainer.py:617-622), per pixel as sn_rm_mask_nll: -log(clamp(p[y], eps, 1 - eps)); a label outside 0..K-1: 0
        const bool valid = y >= 0 && y < (int64_t)K;
        const float py = valid ? pick<KT>(p, (int)y) : 1.0f;
        const float cl = fminf(fmaxf(py, eps), 1.0f - eps);
        sum += (double)(valid ? -logf(cl) : 0.0f);
        labelled += y != -1 ? 1u : 0u;
        // MeanIoUMeter.update on (id, y): a label outside 0..C-1 matches no class, its pixel still counts for its predicted class
        atomicAdd(&s_hist[MO_MAX_K + id], 1u);
        if (y >= 0 && y < (int64_t)C) {
            atomicAdd(&s_hist[2 * MO_MAX_K + (uint32_t)y], 1u);
            if (y == (int64_t)id) atomicAdd(&s_hist[id], 1u);
        }
    }
    __syncthreads();
    if (tid < 3 * MO_MAX_K && s_hist[tid] != 0u) atomicAdd(&ws->counts[tid], (unsigned long long)s_hist[tid]);
    if (!publish_and_draw(sum, labelled, &ws->ticket, ws->part_sum, ws->part_cnt, s_wave, s_cnt, &s_flag)) return;

    uint64_t n_lab;
    const double total = sum_partials(ws->part_sum, ws->part_cnt, s_part, s_pcnt, &n_lab);
    uint64_t mine = 0;
    if (tid < 3 * MO_MAX_K) {
        mine = __hip_atomic_load(&ws->counts[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (tid < MO_MAX_K ? rec->inter : tid < 2 * MO_MAX_K ? rec->pred : rec->truth)[tid % MO_MAX_K] = mine;
        __hip_atomic_store(&ws->counts[tid], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // per class: inter / union in double, union = pred + truth - inter (metrics.py:171-175); -1: the class is in neither
    if (tid < 3 * MO_MAX_K) s_cls[tid] = mine;
    __syncthreads();
    if (tid < MO_MAX_K) {
        const uint64_t in = s_cls[tid], un = s_cls[MO_MAX_K + tid] + s_cls[2 * MO_MAX_K + tid] - in;
        s_iou[tid] = un ? (double)in / (double)un : -1.0;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        uint32_t classes = 0;
        for (uint32_t i = 0; i < C; ++i) if (s_iou[i] >= 0.0) { acc += s_iou[i]; ++classes; }
        rec->miou_sum += classes ? acc / (double)classes : 0.0;
        rec->nll_mean_sum += n_lab ? total / (double)n_lab : 0.0;
        rec->images += 1;
        __hip_atomic_store(&ws->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_image_sqerr_accumulate(const float *__restrict__ pred, uint32_t pred_stride, const float *__restrict__ truth,
                                                                uint32_t truth_stride, uint32_t N, sn_eval_record *__restrict__ rec,
                                                                EvalWorkspace *__restrict__ ws) {
    SN_POISON_ALL();
    __shared__ double s_part[MO_MAX_PARTIALS];
    __shared__ uint32_t s_pcnt[MO_MAX_PARTIALS];
    __shared__ double s_wave[4];
    __shared__ uint32_t s_cnt[4], s_flag;
    double sum = 0.0;
    for (uint32_t n = blockIdx.x * MO_TILE + threadIdx.x; n < N; n += gridDim.x * MO_TILE) {
        const float *a = pred + (size_t)n * pred_stride, *b = truth + (size_t)n * truth_stride;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double d = (double)(a[j] - b[j]);              // the difference in fp32 as numpy takes it, squared and summed in double
            sum += d * d;
        }
    }
    if (!publish_and_draw(sum, 0u, &ws->ticket, ws->part_sum, ws->part_cnt, s_wave, s_cnt, &s_flag)) return;
    uint64_t unused;
    const double total = sum_partials(ws->part_sum, ws->part_cnt, s_part, s_pcnt, &unused);
    if (threadIdx.x == 0) {
        const double mse = total / (3.0 * (double)N);
        rec->mse_sum += mse;                                     // MSEMeter.update
        rec->psnr_sum += -10.0 * log10(mse);                     // PSNRMeter.update (max pixel value 1)
        rec->rgb_images += 1;
        __hip_atomic_store(&ws->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_mask_output(const float *logits, uint32_t N, uint32_t K, const float *image, uint32_t image_stride, const float *color_map, uint32_t C,
                      int mode, int render_id, float alpha, const float *bg, float *probs, int64_t *instance_id, float *confidence, float *rgb,
                      uint8_t *rgb8, sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(logits, "mask_output: NULL logits");
    SN_REQUIRE(K >= 1, "mask_output: at least one instance logit (K = 0)");
    SN_UNSUPPORTED(K <= MO_MAX_K, "mask_output: at most %u instances (got K=%u)", MO_MAX_K, K);
    SN_UNSUPPORTED(N < (1u << 31), "mask_output: N must stay below 2^31 (got %u)", N);
    SN_REQUIRE(mode >= SN_MASK_OUT_NONE && mode <= SN_MASK_OUT_MASK, "mask_output: unknown mode %d", mode);
    SN_REQUIRE(probs || instance_id || confidence || rgb || rgb8, "mask_output: no output given");
    const bool colour = rgb || rgb8;
    if (colour) {
        if (mode != SN_MASK_OUT_HEATMAP) {
            SN_REQUIRE(image, "mask_output: NULL image (every mode but the heatmap reads it)");
            SN_REQUIRE(image_stride >= 3, "mask_output: image row stride %u floats, at least 3", image_stride);
        }
        if (mode == SN_MASK_OUT_HEATMAP || mode == SN_MASK_OUT_COMPOSITION) {
            SN_REQUIRE(color_map, "mask_output: NULL color_map");
            SN_REQUIRE(C >= K, "mask_output: a colour table of C=%u rows cannot serve K=%u instance ids (C >= K)", C, K);
        }
        if (mode == SN_MASK_OUT_MASK) SN_REQUIRE(bg, "mask_output: NULL bg (the mask mode's background, 3 floats on the device)");
        SN_REQUIRE((reinterpret_cast<uintptr_t>(rgb8) & 3u) == 0, "mask_output: rgb8 must be 4-byte aligned (it is stored as dwords)");
    }
    MaskOutArgs a;
    a.logits = logits; a.image = image; a.color_map = color_map; a.bg = bg; a.N = N; a.K = K; a.image_stride = image_stride;
    a.mode = mode; a.render_id = render_id; a.alpha = alpha;
    a.probs = probs; a.instance_id = instance_id; a.confidence = confidence; a.rgb = rgb; a.rgb8 = rgb8;
    hipStream_t st = (hipStream_t)stream;
#define SN_MO_LAUNCH(KT) hipLaunchKernelGGL(k_mask_output<KT>, dim3(div_up(N, MO_TILE)), dim3(MO_TILE), 0, st, a)
    SN_DISPATCH_KT(K, SN_MO_LAUNCH);
#undef SN_MO_LAUNCH
    SN_LAUNCH_CHECK("k_mask_output");
    return SN_OK;
}

int sn_rm_mask_eval_accumulate(const float *logits, const int64_t *labels, uint32_t N, uint32_t K, uint32_t C, float eps, sn_eval_record *record,
                               void *workspace, sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(logits && labels && record && workspace, "mask_eval_accumulate: NULL pointer");
    SN_REQUIRE(K >= 1, "mask_eval_accumulate: at least one instance logit (K = 0)");
    SN_UNSUPPORTED(K <= MO_MAX_K, "mask_eval_accumulate: at most %u instances (got K=%u)", MO_MAX_K, K);
    SN_REQUIRE(C >= K, "mask_eval_accumulate: C=%u classes for K=%u instance ids (C >= K)", C, K);
    SN_UNSUPPORTED(C <= MO_MAX_K, "mask_eval_accumulate: at most %u classes (got C=%u)", MO_MAX_K, C);
    SN_UNSUPPORTED(N < (1u << 31), "mask_eval_accumulate: N must stay below 2^31 (got %u)", N);
    SN_REQUIRE(((reinterpret_cast<uintptr_t>(record) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
               "mask_eval_accumulate: record / workspace must be 8-byte aligned");
    const uint32_t blocks = mo_min(div_up(N, MO_TILE), MO_MAX_PARTIALS);
    hipStream_t st = (hipStream_t)stream;
    EvalWorkspace *ws = static_cast<EvalWorkspace *>(workspace);
#define SN_ME_LAUNCH(KT) hipLaunchKernelGGL(k_mask_eval_accumulate<KT>, dim3(blocks), dim3(MO_TILE), 0, st, logits, labels, N, K, C, eps, record, ws)
    SN_DISPATCH_KT(K, SN_ME_LAUNCH);
#undef SN_ME_LAUNCH
    SN_LAUNCH_CHECK("k_mask_eval_accumulate");
    return SN_OK;
}

int sn_rm_image_sqerr_accumulate(const float *pred, uint32_t pred_stride, const float *truth, uint32_t truth_stride, uint32_t N,
                                 sn_eval_record *record, void *workspace, sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(pred && truth && record && workspace, "image_sqerr_accumulate: NULL pointer");
    SN_REQUIRE(pred_stride >= 3 && truth_stride >= 3, "image_sqerr_accumulate: row strides %u / %u floats, at least 3", pred_stride, truth_stride);
    SN_UNSUPPORTED(N < (1u << 31), "image_sqerr_accumulate: N must stay below 2^31 (got %u)", N);
    SN_REQUIRE(((reinterpret_cast<uintptr_t>(record) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
               "image_sqerr_accumulate: record / workspace must be 8-byte aligned");
    const uint32_t blocks = mo_min(div_up(N, MO_TILE), MO_MAX_PARTIALS);
    hipLaunchKernelGGL(k_image_sqerr_accumulate, dim3(blocks), dim3(MO_TILE), 0, (hipStream_t)stream, pred, pred_stride, truth, truth_stride, N, record,
                       static_cast<EvalWorkspace *>(workspace));
    SN_LAUNCH_CHECK("k_image_sqerr_accumulate");
    return SN_OK;
}

}  // extern "C"
