// render_prop.h -- fused renderer: the proposal stages (k_prop_stage: one lane per ray; k_prop_stage_sp: several lanes per ray).
#ifndef SN_RENDER_PROP_H
#define SN_RENDER_PROP_H
#include "render_knobs.h"
#include "render_gather.h"
#include "render_dense.h"

namespace sn {

// ------------------------------------------------------------------------------------------
// proposal stage
// ------------------------------------------------------------------------------------------
struct PropArgs {
    RayCommon rc;
    GridLevels g;
    const void *table;
    const float *w0, *w1;        // MLP weights (device), [HID][IN], [1][HID]
    uint32_t T, Tn;              // steps of this stage; bins of the next stage = Tn + 1
    const float *bins_in;        // scratch [T+1][Npad] or NULL (stage 0)
    const float *bins0_tab;      // device [T+1] (bins0_stride 0) or per ray [N][bins0_stride], or NULL (stage 0 only)
    const float *u_tab;          // device [Tn+1] (u_stride 0) or per ray [N][u_stride], or NULL
    uint32_t bins0_stride, u_stride;
    float *dbg_bins_next;        // [N,Tn+1] or NULL: the resampled bins in the reference's layout (io->skip_final)
    float *w_scr;                // scratch [T][Npad]
    float *bins_out;             // scratch [Tn+1][Npad]
    float *dbg_bins, *dbg_w, *dbg_sigma;  // [N,T+1], [N,T], [N,T] or NULL
    int32_t *dbg_inds;                    // [N,Tn+1] or NULL
    PairTab pairs;                        // dense levels as aligned x-pairs
    int skip_miss;                        // the last stage runs k_final_stage_cmp: waves whose rays all miss the aabb leave at once
};

// renderer.py:133-135: near = far = 1e9 marks a ray that misses the aabb
__device__ __forceinline__ bool ray_misses(const RayCommon &rc, const RaySetup &rs) {
    float nr, fr;
    near_far_one(rs.o, rs.d, rc.aabb, rc.min_near, nr, fr);
    return nr == 1e9f && fr == 1e9f;
}

// UN: samples of a ray evaluated together in pass 1 (their gathers and their MLP chains interleave: two dependent chains per wave instead of
// one).  Every sample goes through the same arithmetic and the weights / the normaliser are formed in the same order: bit-identical to UN = 1.
template <typename TT, int L, int C, int HID, int K, int UN = 1>
__global__ __launch_bounds__(256, (UN == 1 ? SN_PROP_WAVES : SN_PROP_WAVES_U2)) void k_prop_stage(PropArgs a) {
    SN_POISON_ALL();
    constexpr int IN = L * C;
    __shared__ __attribute__((aligned(16))) float lds_w0[IN * PadIn<HID>::value];   // k-major [IN][HID]
    __shared__ __attribute__((aligned(16))) float lds_w1[PadIn<HID>::value];        // [1][HID]
    stage_weights_t<IN, HID>(lds_w0, a.w0);
    stage_weights<HID, 1>(lds_w1, a.w1);
    __syncthreads();
    uint32_t n;
    const uint32_t wg = tile_id(a.rc);
    const bool ok = ray_of_lane(a.rc, wg, n);
    const uint32_t r = wg * 256u + threadIdx.x;           // scratch column
    const uint32_t Npad = a.rc.Npad;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    // opt-in compaction (cfg->compact_live): k_final_stage_cmp gives rays that miss the aabb (and lanes beyond the image
    // edge) no samples and never reads their bins, so a wave made of such rays only has nothing to produce (no barrier follows)
    if (a.skip_miss && __all(!ok || ray_misses(a.rc, rs))) return;
    const uint32_t T = a.T;
    const float b0step = 1.0f / (float)T;                 // (1-0)/(steps-1), steps = T+1

    auto bin_at = [&](uint32_t j) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + r];
        if (a.bins0_tab) return a.bins0_tab[(size_t)n * a.bins0_stride + j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };

    // ---- pass 1: sigma -> weights (renderer.py:277-325) ----
    float bprev = bin_at(0);
    float rb_prev = real_bin(rs, bprev);
    if (ok && a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1)] = bprev;
    double cum = 0.0, wacc = 0.0;
    const TT *table = reinterpret_cast<const TT *>(a.table);
    const bool early_out = !a.dbg_bins && !a.dbg_sigma && !a.dbg_w;
    // samples j .. j+U-1; returns true once the transmittance of all 64 rays of the wave has underflowed to exactly 0
    auto march = [&](auto un_tag, uint32_t j) -> bool {
        constexpr int U = decltype(un_tag)::value;
        float bnext[U], rb_next[U], x01[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bnext[u] = bin_at(j + (uint32_t)u + 1u);
            rb_next[u] = real_bin(rs, bnext[u]);
            const float tmid = (rb_next[u] + (u ? rb_next[u ? u - 1 : 0] : rb_prev)) / 2.0f;
            float p[3];
            sample_x01(a.rc, rs, tmid, p, x01[u]);
        }
        float feat[U][L * C], raw[U];
        if constexpr (U == 1) encode_levels<TT, L, C, K, true, (sizeof(TT) == 4 ? SN_PROP_GROUP : SN_PROP_GROUP_H)>(table, a.g, x01[0], feat[0], &a.pairs);
        else encode_levels_multi<TT, L, C, K, true, SN_PROP_GROUP_U2, U>(table, a.g, x01, feat, &a.pairs);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float h[HID], r1[1];
            const uint32_t oz = opaque_zero();
            dense_ldsw_t<IN, HID, 1, (U > 1)>(lds_w0 + oz, feat[u], h);
            dense_ldsw<HID, 1, 0>(lds_w1 + oz, h, r1);
            raw[u] = r1[0];
        }
        bool dark = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t ju = j + (uint32_t)u;
            const float rbp = u ? rb_next[u ? u - 1 : 0] : rb_prev;
            const float sigma = expf_det(raw[u]);                // trunc_exp forward (activation.py:9)
            const float delta = rb_next[u] - rbp;
            float ds = delta * sigma;
            if (a.rc.last_opaque && ju == T - 1u) ds = __builtin_inff();
            const float alpha = 1.0f - expf_det(-ds);
            const float tr = expf_det(-(float)cum);
            float w = alpha * tr;
            if (w != w) w = 0.0f;
            a.w_scr[(size_t)ju * Npad + r] = w;
            cum += (double)ds;
            wacc += (double)(w + 0.01f);
            if (ok) {
                if (a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1) + ju + 1] = bnext[u];
                if (a.dbg_sigma) a.dbg_sigma[(size_t)n * T + ju] = sigma;
                if (a.dbg_w) a.dbg_w[(size_t)n * T + ju] = w;
            }
            // EXACT early-out (round 4): once the transmittance of all 64 rays of the wave has underflowed to exactly 0 it stays 0 (the optical
            // depth never decreases), so every later weight is alpha * 0 = 0 whatever the density: the remaining samples are not evaluated, their
            // weights are written as 0 and the pdf normaliser keeps taking its (0 + 0.01) terms in the same order.  Opaque scenes only; bit-identical.
            // (with U > 1 the samples of the group that follow the underflow are still evaluated: their weights come out as the same zeros)
            if (u == U - 1) dark = early_out && __all(tr == 0.0f);
        }
        rb_prev = rb_next[U - 1];
        return dark;
    };
    {
        uint32_t j = 0;
        bool dark = false;
        if constexpr (UN > 1) {
            for (; j + (uint32_t)UN <= T && !dark; j += (uint32_t)UN) dark = march(std::integral_constant<int, UN>{}, j);
        }
        for (; j < T && !dark; ++j) dark = march(std::integral_constant<int, 1>{}, j);
        for (; j < T; ++j) {                                   // (only after an early-out)
            a.w_scr[(size_t)j * Npad + r] = 0.0f;
            wacc += (double)(0.0f + 0.01f);
        }
    }

    // ---- pass 2: sample_pdf (renderer.py:84-119) as one merge of cdf against u ----
    // The cdf is walked in blocks of PB entries: the block's weights and bins are fetched with independent, coalesced loads
    // (the former one-entry-at-a-time merge chained T dependent global loads per ray and cost 19 % of the stage), its PB
    // prefix values are formed in the oracle's order (fp64 running sum of the pdf, rounded per prefix, clamped at 1), and
    // every lane then emits the outputs whose searchsorted(right=True) count falls inside the block.
    const float wsum = (float)wacc;
    const uint32_t Tq = a.Tn + 1u;
    const float ustart = (float)(0.5 / Tq), uend = (float)(1 - 0.5 / Tq);
    const float ustep = (uend - ustart) / (float)(Tq - 1u);
    auto u_at = [&](uint32_t j) -> float { return a.u_tab ? a.u_tab[(size_t)n * a.u_stride + (j < Tq ? j : Tq - 1u)] : linspace_at(ustart, uend, ustep, Tq, j); };
    constexpr uint32_t PB = SN_PROP_PB;
    uint32_t jq = 0;
    float uj = u_at(0);
    double acc = 0.0;
    float c_start = 0.0f, b_start = bin_at(0);              // cdf[ib], bins[ib]
    for (uint32_t ib = 0; ib < T; ib += PB) {
        const bool last_block = ib + PB >= T;
        float e_c[PB + 1], e_b[PB + 1];                     // entries ib .. ib+PB of the cdf and the bins (past T: repeats of entry T)
        e_c[0] = c_start; e_b[0] = b_start;
        float wv[PB];
#pragma unroll
        for (uint32_t k = 0; k < PB; ++k) {
            const uint32_t idx = ib + k < T ? ib + k : T - 1u;
            wv[k] = a.w_scr[(size_t)idx * Npad + r];
            e_b[k + 1] = bin_at(idx + 1u);
        }
#pragma unroll
        for (uint32_t k = 0; k < PB; ++k) {
            if (ib + k < T) {                               // uniform
                const float pdf = (wv[k] + 0.01f) / wsum;
                acc += (double)pdf;
                const float c = (float)acc;
                e_c[k + 1] = c > 1.0f ? 1.0f : c;
            } else {
                e_c[k + 1] = e_c[k];
            }
        }
        const uint32_t nb = last_block ? T - ib : PB;       // real entries after e[0] in this block
        // outputs of this block: all whose u is below the block's last cdf value; in the last block all that remain
        while (jq < Tq && (last_block || e_c[PB] > uj)) {
            uint32_t cnt = 0;                                // entries e[0..nb] that are <= uj (e is non-decreasing)
#pragma unroll
            for (uint32_t m = 0; m <= PB; ++m) cnt += (m <= nb && e_c[m] <= uj) ? 1u : 0u;
            const uint32_t i = ib + cnt;                     // = searchsorted(cdf, u, right=True): every entry before ib is <= e[0]
            // below = entry i-1, above = entry i; i == 0 -> both entry 0; i > T -> both entry T (renderer.py:104-107 clamps)
            const uint32_t lo_m = cnt == 0u ? 0u : cnt - 1u, hi_m = cnt > nb ? nb : cnt;
            float c0 = e_c[0], c1 = e_c[0], bb0 = e_b[0], bb1 = e_b[0];
#pragma unroll
            for (uint32_t m = 1; m <= PB; ++m) {
                c0 = lo_m == m ? e_c[m] : c0; bb0 = lo_m == m ? e_b[m] : bb0;
                c1 = hi_m == m ? e_c[m] : c1; bb1 = hi_m == m ? e_b[m] : bb1;
            }
            if (cnt > nb) { c0 = c1; bb0 = bb1; }            // i > T: below = above = the last entry
            float t = nan_to_num((uj - c0) / (c1 - c0));
            t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
            const float m = t * (bb1 - bb0);
            a.bins_out[(size_t)jq * Npad + r] = bb0 + m;
            if (ok && a.dbg_bins_next) a.dbg_bins_next[(size_t)n * Tq + jq] = bb0 + m;
            if (ok && a.dbg_inds) a.dbg_inds[(size_t)n * Tq + jq] = (int32_t)i;
            ++jq;
            uj = u_at(jq);
        }
        c_start = e_c[PB]; b_start = e_b[PB];
    }
}

// ------------------------------------------------------------------------------------------
// proposal stage, sample-parallel variant for small ray batches (training steps: a few thousand rays)
// ------------------------------------------------------------------------------------------
// k_prop_stage walks one ray per lane: 4096 rays are 64 waves on a 1024-SIMD chip, each alone with its memory
// latency, and a 128-sample stage takes 128 serial steps (0.55 ms for 4096 rays).  Here 8 lanes share a ray: each
// evaluates a contiguous chunk of T/8 samples (the expensive part: position, grid, MLP), everything that must keep
// the oracle's sequential order -- the fp64 optical-depth prefix, the cdf -- is done by the ray's first lane over
// values parked in LDS (a few adds per sample), and the T_next + 1 resampled bins are found by a binary search
// per output, 8 outputs at a time.  Same arithmetic, same order where order matters: bit-identical results.
// Linear ray order only (scratch column = ray index), T <= SP_MAX_T.
// Round 6: the lanes per ray are a template parameter (8, 16 or 32: 32, 16 or 8 rays per workgroup).  With 8 lanes a 4096-ray training batch is
// 128 workgroups on 256 CUs and every lane walks T/8 = 16 samples one after the other; the launcher now picks the smallest count that gives
// >= 512 workgroups (4096 rays: 32 lanes, 4 samples per lane).  The serial parts (prefix, cdf) and every sample's arithmetic are unchanged and
// the fp64 sum of the weights is exact in any order: bit-identical for every choice (sn_render_tuning.prop_sp_lanes forces one).
constexpr uint32_t SP_MAX_T = 128;        // 3 arrays x (256 / LPR) rays x (T+4) floats: 50 KiB of static LDS at 8 lanes per ray
constexpr uint32_t SP_STRIDE = SP_MAX_T + 4;   // floats per ray per LDS array

template <typename TT, int L, int C, int HID, int K, uint32_t SP_LPR = 8>
__global__ __launch_bounds__(256, 3) void k_prop_stage_sp(PropArgs a) {
    SN_POISON_ALL();
    static_assert(SP_LPR == 8 || SP_LPR == 16 || SP_LPR == 32, "a ray's lanes live in one wave");
    constexpr uint32_t RPB = 256u / SP_LPR;      // rays per workgroup
    constexpr int IN = L * C;
    __shared__ __attribute__((aligned(16))) float lds_w0[IN * PadIn<HID>::value];
    __shared__ __attribute__((aligned(16))) float lds_w1[PadIn<HID>::value];
    __shared__ float l_bins[RPB][SP_STRIDE];    // stage bins b_0..b_T of the rays of this workgroup
    __shared__ float l_ds[RPB][SP_STRIDE];      // delta*sigma, then reused for the weights
    __shared__ float l_cum[RPB][SP_STRIDE];     // (float) of the fp64 exclusive prefix of delta*sigma, then the cdf
    stage_weights_t<IN, HID>(lds_w0, a.w0);
    stage_weights<HID, 1>(lds_w1, a.w1);
    const uint32_t tid = threadIdx.x, c = tid & (SP_LPR - 1u), rl = tid / SP_LPR;      // chunk index, local ray
    const uint32_t n_raw = blockIdx.x * RPB + rl;
    const bool ok = n_raw < a.rc.N;
    const uint32_t n = ok ? n_raw : 0u, r = n_raw;                                     // scratch column = ray index (linear order)
    const uint32_t Npad = a.rc.Npad, T = a.T;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    const float b0step = 1.0f / (float)T;
    auto bin_src = [&](uint32_t j) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + r];
        if (a.bins0_tab) return a.bins0_tab[(size_t)n * a.bins0_stride + j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };
    for (uint32_t j = c; j <= T; j += SP_LPR) l_bins[rl][j] = bin_src(j);
    __syncthreads();                                                                   // weights + bins in LDS
    if (ok && a.dbg_bins) for (uint32_t j = c; j <= T; j += SP_LPR) a.dbg_bins[(size_t)n * (T + 1) + j] = l_bins[rl][j];

    // ---- per-sample work, T / SP_LPR consecutive samples per lane ----
    const uint32_t spl = (T + SP_LPR - 1u) / SP_LPR;
    const TT *table = reinterpret_cast<const TT *>(a.table);
    for (uint32_t i = 0; i < spl; ++i) {
        const uint32_t jr = c * spl + i;
        const uint32_t j = jr < T ? jr : T - 1u;                                       // lanes past the end redo the last sample
        const float rb_prev = real_bin(rs, l_bins[rl][j]), rb_next = real_bin(rs, l_bins[rl][j + 1u]);
        const float tmid = (rb_next + rb_prev) / 2.0f;
        float p[3], x01[3];
        sample_x01(a.rc, rs, tmid, p, x01);
        float feat[L * C];
        encode_levels<TT, L, C, K, true>(table, a.g, x01, feat, &a.pairs);
        float h[HID], raw[1];
        const uint32_t oz = opaque_zero();
        dense_ldsw_t<IN, HID, 1>(lds_w0 + oz, feat, h);
        dense_ldsw<HID, 1, 0>(lds_w1 + oz, h, raw);
        const float sigma = expf_det(raw[0]);
        float ds = (rb_next - rb_prev) * sigma;
        if (a.rc.last_opaque && j == T - 1u) ds = __builtin_inff();
        if (jr < T) {
            l_ds[rl][j] = ds;
            if (ok && a.dbg_sigma) a.dbg_sigma[(size_t)n * T + j] = sigma;
        }
    }
    __syncthreads();
    // ---- exclusive prefix of delta*sigma in the oracle's order: fp64 running sum, rounded per prefix ----
    if (c == 0u) {
        double cum = 0.0;
        for (uint32_t j = 0; j < T; ++j) { l_cum[rl][j] = (float)cum; cum += (double)l_ds[rl][j]; }
    }
    __syncthreads();
    // ---- weights (renderer.py:308-325); their fp64 sum is exact in any order (addends within 2^7 of each other) ----
    double wacc = 0.0;
    for (uint32_t i = 0; i < spl; ++i) {
        const uint32_t j = c * spl + i;
        if (j < T) {
            const float alpha = 1.0f - expf_det(-l_ds[rl][j]);
            const float tr = expf_det(-l_cum[rl][j]);
            float w = alpha * tr;
            if (w != w) w = 0.0f;
            wacc += (double)(w + 0.01f);
            l_ds[rl][j] = w;                                                             // own slot: no hazard
            a.w_scr[(size_t)j * Npad + r] = w;                                           // padding columns too, like k_prop_stage
            if (ok && a.dbg_w) a.dbg_w[(size_t)n * T + j] = w;
        }
    }
#pragma unroll
    for (int d = 1; d < (int)SP_LPR; d <<= 1) wacc += __shfl_xor(wacc, d, SP_LPR);
    const float wsum = (float)wacc;
    __syncthreads();
    // ---- cdf (renderer.py:92-96): fp64 running sum of the pdf, rounded per prefix, clamped at 1 ----
    if (c == 0u) {
        double acc = 0.0;
        l_cum[rl][0] = 0.0f;
        for (uint32_t j = 0; j < T; ++j) {
            const float pdf = (l_ds[rl][j] + 0.01f) / wsum;
            acc += (double)pdf;
            const float cv = (float)acc;
            l_cum[rl][j + 1u] = cv > 1.0f ? 1.0f : cv;
        }
    }
    __syncthreads();
    // ---- resample: searchsorted(cdf, u, right=True) per output, then the interpolation of renderer.py:104-119 ----
    const uint32_t Tq = a.Tn + 1u;
    const float ustart = (float)(0.5 / Tq), uend = (float)(1 - 0.5 / Tq);
    const float ustep = (uend - ustart) / (float)(Tq - 1u);
    for (uint32_t jq = c; jq < Tq; jq += SP_LPR) {
        const float uj = a.u_tab ? a.u_tab[(size_t)n * a.u_stride + jq] : linspace_at(ustart, uend, ustep, Tq, jq);
        uint32_t lo = 0u, hi = T + 1u;                                                   // number of cdf[0..T] entries <= uj
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (l_cum[rl][mid] <= uj) lo = mid + 1u; else hi = mid;
        }
        const uint32_t i = lo;
        float c0, c1, bb0, bb1;
        if (i == 0u) { c0 = c1 = l_cum[rl][0]; bb0 = bb1 = l_bins[rl][0]; }
        else if (i > T) { c0 = c1 = l_cum[rl][T]; bb0 = bb1 = l_bins[rl][T]; }
        else { c0 = l_cum[rl][i - 1u]; c1 = l_cum[rl][i]; bb0 = l_bins[rl][i - 1u]; bb1 = l_bins[rl][i]; }
        float t = nan_to_num((uj - c0) / (c1 - c0));
        t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
        const float m = t * (bb1 - bb0);
        a.bins_out[(size_t)jq * Npad + r] = bb0 + m;
        if (ok && a.dbg_bins_next) a.dbg_bins_next[(size_t)n * Tq + jq] = bb0 + m;
        if (ok && a.dbg_inds) a.dbg_inds[(size_t)n * Tq + jq] = (int32_t)i;
    }
}

}  // namespace sn

#endif  // SN_RENDER_PROP_H
