// render.hip — fused whole-path renderer for gfx950 (sn_rm_render_rays).
//
// Replaces the torch op chain of NeRFRenderer.run (nerf/renderer.py:221-357) together with
// NeRFNetwork.density / forward (nerf/network.py:146-186) for perturb=False rendering.
//
// Mapping: ONE LANE = ONE RAY for the whole march.  A wave owns an 8x8 pixel
// tile, a 256-thread workgroup a 16x16 tile, and all 64 lanes step through the samples in
// lock-step, so at step j the wave's 64 gathers per corner land in one small 3-D patch:
// coarse levels collapse to a handful of cache lines and fine levels share vertices between
// neighbouring pixels.  Per-ray state (transmittance, colour accumulators, cdf merge
// cursors) lives in registers, in order, so the fp64 prefix sums that decide the sample
// indices are sequential exactly like the CPU oracle's.
//
//   k_prop_stage   stage k < last: bins -> xyz -> contract -> hash grid (L<=8,C=2) ->
//                  tiny MLP (VALU fmaf chains, weights in SGPRs) -> sigma -> weights
//                  (scratch [T][Npad]) -> in-kernel sample_pdf merge -> next bins (scratch).
//   k_final_stage  last stage: hash grid (L=16,C=2) -> 32->64->64->16 MLP on the matrix
//                  cores (v_mfma_f32_32x32x2_f32, exact fp32; operands exchanged between the
//                  two half-waves with v_permlane32_swap, weights pre-packed in LDS in
//                  A-operand order) -> sigma/geo features -> ordered compositing in
//                  registers -> per-ray view MLP -> sigmoid -> image/depth/weights_sum.
//   k_final_stage_pt  the same code per ray (final_stage_rays) under a persistent launch: one 8-wave
//                  workgroup per CU, every wave pulls 8x8 tiles from per-XCD queues.
//
// One translation unit.  The code up to and including the matrix phase lives in headers, included in this order (definitions and
// instantiations keep it, so a pure move leaves the device code unchanged: tools/render_isa_sha.sh, profiles/render_split_isa.txt):
//   render_knobs.h   every build-time SN_* constant of this file with its measured history
//   render_rays.h    RayCommon, tile orders (xcd_tile_id, wave_tile_of, tile_queue_range), ray_of_lane, setup_ray, bins -> sample position
//   render_gather.h  Corner, two-phase level groups, XSWAP and PARITY helpers, PairTab, encode_levels*, GroupRegs, FinalLv, FinalSpans
//   render_dense.h   PadIn, stage_weights*, dense_ldsw*: the VALU layers of the proposal and colour heads
//   render_prop.h    PropArgs, ray_misses, k_prop_stage, k_prop_stage_sp
//   render_mfma.h    pack layouts, k_pack_grid_mlp*, the matrix phase up to grid_mlp_mfma16_l12_spread, the VALU fallback
// This file: the last stage (FinalArgs, clock probe, final_stage_rays and its launch forms, _any / _cmp / _sp), the feature stage, the route
// planner, the launch glue and the C entry points.
#include "render_knobs.h"
#include "render_rays.h"
#include "render_gather.h"
#include "render_dense.h"
#include "render_prop.h"
#include "render_mfma.h"

#include <float.h>
#include <stdlib.h>
#include <string.h>
#include <cstdio>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace sn {

// ------------------------------------------------------------------------------------------
// final stage
// ------------------------------------------------------------------------------------------
struct FinalArgs {
    RayCommon rc;
    GridLevels g;
    const void *table;
    const float *mlp_pack;       // MFMA path: A-operand-ordered weights (floats, PACK_FLOATS)
    const float *w[3];           // VALU path: raw [out][in] weights of grid_mlp
    const float *vw[3];          // view_mlp weights
    uint32_t T;
    const float *bins_in;        // scratch [T+1][Npad] or NULL (single-stage)
    const float *bins0_tab;
    uint32_t bins0_stride;       // 0: bins0_tab is one shared table; else per ray [N][bins0_stride]
    uint32_t sh_degree;
    float *image, *depth, *wsum;
    uint32_t istride, sstride;   // floats between consecutive rays of image / of depth and wsum (3 and 1, or sn_render_io.out_stride for both)
    float *dbg_bins, *dbg_w, *dbg_sigma, *dbg_xyz, *dbg_geo, *dbg_fimg;
    uint32_t fimg_stride;        // floats between consecutive rays of dbg_fimg (geo + 16, or sn_render_io.head_stride)
    float *head_rgbd;            // sn_render_io.head_stride: rgb | depth of ray n also go to head_rgbd[n * fimg_stride + 0..3] (the SAM head's MLP input), or NULL
    float *w_out;                // scratch [T][Npad] for the feature stage, or NULL
    float stop_cum;              // > 0: a wave leaves the march once every lane's optical depth exceeds this (-ln eps)
    PairTab pairs;               // dense levels of the main grid as aligned x-pairs (K > 0 instantiations)
    FinalLv lv;                  // per-level constants of the K > 0 instantiations
};

// shader-clock probe of the measurement hook: s_memtime ticks at the shader clock, s_memrealtime at the constant
// wall-clock rate (hipDeviceAttributeWallClockRate); their ratio over one workgroup's lifetime is the clock the
// kernel actually ran at (DVFS: well below the 2.4 GHz peak under this kernel), which prices the cycle-count ceilings
// (device globals rather than a kernel argument: the final stage has no scalar registers to spare)
__device__ int g_clk_on = 0;
__device__ unsigned long long g_clk_buf[4];
__device__ __forceinline__ void clock_probe(int slot) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && g_clk_on) {
        g_clk_buf[2 * slot] = __builtin_readcyclecounter();
        g_clk_buf[2 * slot + 1] = __builtin_amdgcn_s_memrealtime();
    }
}


// AUX: the instantiation that also serves the feature stage (weights -> scratch) and the opt-in early termination;
// the plain one carries neither (one spilled register less in the march of the headline configuration)
// PORD: the matrix phase of the linear-tail form in the order it had before grid_mlp_mfma16_l12_spread (tile by tile, vector work in clumps):
// the A/B partner of the spread order, instantiated by experiments builds only (SN_EXP_MATRIX_CLUMPED)
// CANON: the hashed levels of the FinalLv path in the canonical corner order instead of by cell parity (round 10): the A/B partner of the parity
// order, instantiated by experiments builds only (SN_EXP_GATHER_CANONICAL)
// What one wave needs of the workgroup's LDS to march a wave tile: the carve-up the launch form made (k_final_stage: per workgroup tile;
// k_final_stage_pt: once per resident workgroup)
struct FinalLds {
    float *lds;                 // base: packed grid-MLP weights (matrix-core forms), w3p inside
    float *fe;                  // this lane's feature column base
    uint32_t fstride;           // distance between consecutive features of one lane
    float *actB;                // VALU form
    float *lds_vw;              // view_mlp weights (padded rows), all three layers back to back
    uint32_t *slab_hi, *slab_lo;      // MLP_F16X3: this wave's split feature images
    const uint32_t *l0tab;      // L0L: level 0 of the main grid
};

// The last stage of ONE wave tile (g, wave-uniform): ray set-up, the march, the per-ray colour head, the output stores.  Both launch forms
// run this code.  PT (persistent launch): the view weights are resident (no barrier, no staging behind the march) and the clock probe
// belongs to the caller's loop.
template <typename TT, int L, int C, int H1, int H2, int NOUT, int VH, int MODE, int K, bool AUX, bool LT, bool L0L, bool EO, int NP, bool PORD, bool CANON, bool PT>
__device__ __forceinline__ void final_stage_rays(const FinalArgs &a, const FinalLds &fl, const uint32_t g) {
    constexpr int SLAB_DW = L0L ? 16 : SLAB_STRIDE;       // dwords per slab row
    constexpr bool MFMA = MODE != MLP_VALU;
    constexpr int IN = L * C;
    constexpr int GEO = NOUT - 1;
    constexpr int NSH = 16;                       // sh degree 4 (network.py:97)
    constexpr int NCOL = GEO + NSH;
    constexpr int VW0 = VH * PadIn<NCOL>::value, VW1 = VH * PadIn<VH>::value;   // third layer: 3 * PadIn<VH> floats follow
    float *const lds = fl.lds, *const fe = fl.fe, *const actB = fl.actB, *const lds_vw = fl.lds_vw;
    const uint32_t fstride = fl.fstride;
    uint32_t *const slab_hi = fl.slab_hi, *const slab_lo = fl.slab_lo;
    const uint32_t *const l0tab = fl.l0tab;
    (void)SLAB_DW; (void)MFMA; (void)actB; (void)l0tab; (void)VW0; (void)VW1;

    uint32_t n;
    const bool ok = ray_of_wave_tile(a.rc, g, threadIdx.x & 63u, n);
    const uint32_t r = g * 64u + (threadIdx.x & 63u);          // scratch column (= tile id * 256 + threadIdx.x of the ordinary launch)
    const uint32_t Npad = a.rc.Npad;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    const uint32_t T = a.T;
    const float b0step = 1.0f / (float)T;
    auto bin_at = [&](uint32_t j) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + r];
        if (a.bins0_tab) return a.bins0_tab[(size_t)n * a.bins0_stride + j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };

    // view direction, normalised twice like the reference (renderer.py:294, sphere_harmonics.py:82)
    float dirn[3] = {rs.d[0], rs.d[1], rs.d[2]};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const float aa = dirn[0] * dirn[0], bb = dirn[1] * dirn[1], cc = dirn[2] * dirn[2];
        const float nrm = sqrtf((aa + bb) + cc);
        dirn[0] = dirn[0] / nrm; dirn[1] = dirn[1] / nrm; dirn[2] = dirn[2] / nrm;
    }

    float fimg[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) fimg[c] = 0.0f;
    float dep = 0.0f;
    double cum = 0.0, wsum = 0.0;
    float tr_seen = 1.0f;                                  // this lane's ray: transmittance in front of the sample just evaluated
    uint32_t j_stop = a.T;                                 // first sample index NOT evaluated (exact early-out below)
    const bool per_sample_export = a.dbg_bins || a.dbg_w || a.dbg_sigma || a.dbg_xyz || a.dbg_geo;
    const TT *table = reinterpret_cast<const TT *>(a.table);
    // linear tail: sum_j w_j relu(h2_j) of the lane's 32 hidden rows, for the tile-0 and the tile-1 sample it shares
    float hacc[LT ? 2 : 1][LT ? 32 : 1];
    if constexpr (LT) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 32; ++i) hacc[t][i] = 0.0f;
    }
    const float *w3p = lds + W3P_OFFSET + (threadIdx.x & 32u) * 16u;          // this half-wave's rows: [o][32]

    float bprev = bin_at(0);
    float rb_prev = real_bin(rs, bprev);
    if (ok && a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1)] = bprev;
    // software pipeline (MLP_F16X3): group 0 of sample j+1 is issued before the matrix-core phase of sample j
    constexpr int PG = 4;                                   // levels per gather group (generic instantiations)
    constexpr bool LV = MODE == MLP_F16X3 && K >= PG && K <= 8;   // FinalLv path; the prefetched span is all dense
    using SP = FinalSpans<LV ? (LT ? (sizeof(TT) == 2 ? SN_FINAL_SPANS_LT_H : SN_FINAL_SPANS_LT) : 0) : 0>;   // FinalLv path: gather spans (span 0 crosses the matrix-core phase)
    constexpr int G0 = LV ? SP::B[1] : PG;
    static_assert(!LV || (L == 16 && SP::B[SP::N] == L && G0 <= K), "spans cover the 16 levels; span 0 is dense");
    GroupRegs<TT, 2, G0> g0;
    float bnext_n = bin_at(1);
    float rb_next_n = real_bin(rs, bnext_n);
    float tmid_n = (rb_next_n + rb_prev) / 2.0f;
    float p_n[3], x01_n[3];
    sample_x01(a.rc, rs, tmid_n, p_n, x01_n);
    bool fast_n = false;
    if constexpr (LV) {
        fast_n = all_interior(a.lv, x01_n);
        if constexpr (L0L) {
            issue_level0_lds<0>(a.lv, l0tab, x01_n, g0.pos[0], g0.cv[0]);             // level 0 from LDS, the rest of span 0 through the texture path
            static_for<1, G0>([&](auto kk) { constexpr int k = decltype(kk)::value; issue_level_lv<TT, true, false, false, k>(a.lv, x01_n, g0.pos[k], g0.cv[k]); });
        } else issue_span_lv<TT, 0, G0, K, false>(a.lv, x01_n, g0);
        __builtin_amdgcn_sched_barrier(0);
    } else if constexpr (MODE == MLP_F16X3) {
        issue_group<TT, 2, PG, K, 0>(table, a.g, x01_n, g0, a.pairs);
        __builtin_amdgcn_sched_barrier(0);
    }
    for (uint32_t j = 0; j < T; ++j) {
        const float bnext = bnext_n;
        const float rb_next = rb_next_n;
        const float tmid = tmid_n;
        float p[3] = {p_n[0], p_n[1], p_n[2]}, x01[3] = {x01_n[0], x01_n[1], x01_n[2]};
        float h[NOUT];
        if constexpr (MODE == MLP_F16X3) {
            const uint32_t lane = threadIdx.x & 63u;
            uint32_t *row_hi = slab_hi + lane * SLAB_STRIDE, *row_lo = slab_lo + lane * SLAB_STRIDE;
            auto emit = [&](int l, const float (&acc)[2]) {
                if constexpr (NP < 3) { row_hi[l] = pack_h2(acc[0], acc[1]); return; }      // fp16-rounded features: no lo image
                uint32_t ph, pl;
                split2(acc[0], acc[1], ph, pl);
                if constexpr (L0L) { const uint32_t o = slab_dword<true>(lane, (uint32_t)l); slab_hi[o] = ph; slab_lo[o] = pl; }
                else { row_hi[l] = ph; row_lo[l] = pl; }
            };
            if constexpr (LV) blend_span<TT, 0, G0, K>(g0, emit);
            else blend_group<TT, 2, PG, K, 0>(g0, emit);
            __builtin_amdgcn_sched_barrier(0);
            auto zero_oob = [&]() {
                const bool oob = (x01[0] < 0.0f || x01[0] > 1.0f) || (x01[1] < 0.0f || x01[1] > 1.0f) || (x01[2] < 0.0f || x01[2] > 1.0f);
                if (__builtin_expect(__any(oob), 0)) {      // gridencoder.cu:105-130: zeros outside [0,1]
                    if (oob) for (int l = 0; l < L; ++l) {
                        if constexpr (L0L) { const uint32_t o = slab_dword<true>(lane, (uint32_t)l); slab_hi[o] = 0u; slab_lo[o] = 0u; }
                        else { row_hi[l] = 0u; row_lo[l] = 0u; }
                    }
                }
            };
            if constexpr (LV) {
                auto rest = [&](auto fast_tag) {
                    constexpr bool FAST = decltype(fast_tag)::value;
                    static_for<1, SP::N>([&](auto gg) {
                        constexpr int SPAN = decltype(gg)::value, L0 = SP::B[SPAN], G = SP::B[SPAN + 1] - L0;
                        GroupRegs<TT, 2, G> gr;
                        issue_span_lv<TT, L0, G, K, FAST, !CANON>(a.lv, x01, gr);
                        __builtin_amdgcn_sched_barrier(0);
                        blend_span<TT, L0, G, K, !CANON>(gr, emit);
                        __builtin_amdgcn_sched_barrier(0);
                    });
                };
                if (__builtin_expect(fast_n, 1)) rest(std::true_type{});          // fast_n: decided for this sample one iteration ago
                else { rest(std::false_type{}); zero_oob(); }
            } else {
                static_for<1, L / PG>([&](auto gg) {
                    constexpr int GRP = decltype(gg)::value;
                    GroupRegs<TT, 2, PG> gr;
                    issue_group<TT, 2, PG, K, GRP>(table, a.g, x01, gr, a.pairs);
                    __builtin_amdgcn_sched_barrier(0);
                    blend_group<TT, 2, PG, K, GRP>(gr, emit);
                    __builtin_amdgcn_sched_barrier(0);
                });
                zero_oob();
            }
            {   // geometry of the next sample (the last iteration re-issues its own sample: in bounds, unused)
                const uint32_t jn = j + 2u <= T ? j + 2u : T;
                bnext_n = bin_at(jn);
                rb_next_n = real_bin(rs, bnext_n);
                const float rbp = j + 2u <= T ? rb_next : rb_prev;
                tmid_n = (rb_next_n + rbp) / 2.0f;
                sample_x01(a.rc, rs, tmid_n, p_n, x01_n);
                if constexpr (LV) {
                    fast_n = all_interior(a.lv, x01_n);
                    if constexpr (L0L) {
                        issue_level0_lds<0>(a.lv, l0tab, x01_n, g0.pos[0], g0.cv[0]);             // level 0 from LDS, the rest of span 0 through the texture path
                        static_for<1, G0>([&](auto kk) { constexpr int k = decltype(kk)::value; issue_level_lv<TT, true, false, false, k>(a.lv, x01_n, g0.pos[k], g0.cv[k]); });
                    } else issue_span_lv<TT, 0, G0, K, false>(a.lv, x01_n, g0);
                } else {
                    issue_group<TT, 2, PG, K, 0>(table, a.g, x01_n, g0, a.pairs);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_wave_barrier();
            if constexpr (!LT) grid_mlp_mfma16(reinterpret_cast<const uint4 *>(lds) + opaque_zero(), slab_hi, slab_lo, h);
            __builtin_amdgcn_wave_barrier();
        } else if constexpr (MODE == MLP_F32) {
            encode_levels_lds<TT, L, C, 2, K>(table, a.g, x01, fe, fstride);
            // the slab is private to this wave and LDS serves a wave's requests in order
            __builtin_amdgcn_wave_barrier();
            grid_mlp_mfma(lds + opaque_zero(), fe - (threadIdx.x & 63u), h);
            __builtin_amdgcn_wave_barrier();
        } else {
            encode_levels_lds<TT, L, C, 2, K>(table, a.g, x01, fe, fstride);
            dense_lds<IN, H1, 1>(a.w[0], fe, actB, fstride);
            dense_lds<H1, H2, 1>(a.w[1], actB, fe, fstride);
            dense_lds<H2, NOUT, 0>(a.w[2], fe, actB, fstride);
#pragma unroll
            for (int k = 0; k < NOUT; ++k) h[k] = actB[k * fstride];
        }
        if constexpr (LT && (sizeof(TT) == 2 ? 0 : 0)) {
            // tile by tile: layers 1-2, density dot, the compositing step of that tile's home lanes, the accumulator update -- the
            // 32 activations of tile 0 are dead before tile 1's matrix phase begins (one compositing pass over both tiles would hold
            // them across it: 32 registers the kernel does not have)
            const float delta = rb_next - rb_prev;
            const uint32_t oz = opaque_zero();
            const uint32_t my_half = (threadIdx.x >> 5) & 1u;
            static_for<0, 2>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                float x[32];
                grid_mlp_mfma16_l12<L0L>(reinterpret_cast<const uint4 *>(lds) + oz, slab_hi, slab_lo, t, x);
                const float part = dot32_lds(w3p + oz, x);                            // this half's share of the density row
                auto pr = __builtin_amdgcn_permlane32_swap(__float_as_uint(part), __float_as_uint(part), false, false);
                const float h0 = __uint_as_float(pr[0]) + __uint_as_float(pr[1]);     // half 0's share + half 1's share, in every lane
                float wv = 0.0f;
                if (my_half == (uint32_t)t) {                                         // home lanes of this tile's samples
                    const float sigma = expf_det(h0);                                 // network.py:151
                    float ds = delta * sigma;
                    if (a.rc.last_opaque && j == T - 1u) ds = __builtin_inff();
                    const float alpha = 1.0f - expf_det(-ds);
                    const float tr = expf_det(-(float)cum);
                    tr_seen = tr;
                    float w = alpha * tr;
                    if (w != w) w = 0.0f;
                    cum += (double)ds;
                    wsum += (double)w;
                    dep = __builtin_fmaf(w, tmid, dep);
                    if constexpr (AUX) { if (a.w_out) a.w_out[(size_t)j * Npad + r] = w; }
                    wv = w;
                }
                // every lane holds 32 hidden rows of this tile's sample (lane & 31): its weight comes from the home lane
                auto ww = __builtin_amdgcn_permlane32_swap(__float_as_uint(wv), __float_as_uint(wv), false, false);
                const float wt = __uint_as_float(ww[t]);
#pragma unroll
                for (int i = 0; i < 32; i += 2) {
                    const f2v r = __builtin_elementwise_fma(f2v{wt, wt}, f2v{x[i], x[i + 1]}, f2v{hacc[t][i], hacc[t][i + 1]});
                    hacc[t][i] = r.x; hacc[t][i + 1] = r.y;
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            if constexpr (AUX) { if (a.stop_cum > 0.0f && __all((float)cum > a.stop_cum)) break; }
            if constexpr (EO) { if (!per_sample_export && __all(tr_seen == 0.0f)) { j_stop = j + 1u; break; } }      // exact early-out (see below)
            rb_prev = rb_next;
            continue;
        }
        float xh[LT ? 2 : 1][LT ? 32 : 1];
        if constexpr (LT) {
            const uint32_t oz = opaque_zero();
            float part[2];
            if constexpr (NP == 3 && !PORD) {
                grid_mlp_mfma16_l12_spread<L0L>(reinterpret_cast<const uint4 *>(lds) + oz, slab_hi, slab_lo, w3p + oz, xh, part);
            } else {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    grid_mlp_mfma16_l12<L0L, NP>(reinterpret_cast<const uint4 *>(lds) + oz, slab_hi, slab_lo, t, xh[t]);
                    part[t] = dot32_lds(w3p + oz, xh[t]);                              // this half's share of the density row
                }
            }
            __builtin_amdgcn_wave_barrier();
            // lanes 0-31 are the home of the tile-0 samples, lanes 32-63 of the tile-1 samples: half 0's share + half 1's share
            auto pr = __builtin_amdgcn_permlane32_swap(__float_as_uint(part[0]), __float_as_uint(part[1]), false, false);
            h[0] = __uint_as_float(pr[0]) + __uint_as_float(pr[1]);
        }
        const float sigma = expf_det(h[0]);                  // network.py:151
        const float delta = rb_next - rb_prev;
        float ds = delta * sigma;
        if (a.rc.last_opaque && j == T - 1u) ds = __builtin_inff();
        const float alpha = 1.0f - expf_det(-ds);
        const float tr = expf_det(-(float)cum);
        tr_seen = tr;
        float w = alpha * tr;
        if (w != w) w = 0.0f;
        cum += (double)ds;
        wsum += (double)w;
        dep = __builtin_fmaf(w, tmid, dep);
        if constexpr (LT) {
            // every lane needs the weights of BOTH samples whose hidden rows it holds: w of ray (lane & 31) and of ray 32 + (lane & 31)
            auto ww = __builtin_amdgcn_permlane32_swap(__float_as_uint(w), __float_as_uint(w), false, false);
            const float w0 = __uint_as_float(ww[0]), w1 = __uint_as_float(ww[1]);
#pragma unroll
            for (int i = 0; i < 32; i += 2) {
                const f2v r0 = __builtin_elementwise_fma(f2v{w0, w0}, f2v{xh[0][i], xh[0][i + 1]}, f2v{hacc[0][i], hacc[0][i + 1]});
                const f2v r1 = __builtin_elementwise_fma(f2v{w1, w1}, f2v{xh[1][i], xh[1][i + 1]}, f2v{hacc[1][i], hacc[1][i + 1]});
                hacc[0][i] = r0.x; hacc[0][i + 1] = r0.y; hacc[1][i] = r1.x; hacc[1][i + 1] = r1.y;
            }
        } else {
#pragma unroll
            for (int c = 0; c < GEO; ++c) fimg[c] = __builtin_fmaf(w, h[1 + c], fimg[c]);
        }
        if constexpr (AUX) { if (a.w_out) a.w_out[(size_t)j * Npad + r] = w; }
        if constexpr (!LT) if (ok) {                         // (the linear-tail instantiation is not chosen when per-sample tensors are wanted)
            if (a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1) + j + 1] = bnext;
            if (a.dbg_sigma) a.dbg_sigma[(size_t)n * T + j] = sigma;
            if (a.dbg_w) a.dbg_w[(size_t)n * T + j] = w;
            if (a.dbg_xyz) { float *q = a.dbg_xyz + ((size_t)n * T + j) * 3; q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
            if (a.dbg_geo) { float *q = a.dbg_geo + ((size_t)n * T + j) * GEO;
#pragma unroll
                for (int c = 0; c < GEO; ++c) q[c] = h[1 + c]; }
        }
        // opt-in early termination (not reference behaviour): all 64 rays of the wave are opaque to
        // within eps -> the remaining samples could add at most eps to any weight sum
        if constexpr (AUX) { if (a.stop_cum > 0.0f && __all((float)cum > a.stop_cum)) break; }
        // EXACT early-out (round 4, always on when no per-sample tensor is exported): once the transmittance exp(-optical depth) of all 64
        // rays of the wave has underflowed to exactly 0 it stays 0 (the optical depth never decreases), every later weight is alpha * 0 = 0
        // and adds nothing to image, depth or weights_sum: the march ends.  Opaque scenes only (optical depth > 103); bit-identical.  A template
        // switch (EO instantiations, chosen by sn_render_tuning.exact_early_out): in the kernel of the single-stage bench line the test --
        // a compare and a branch per sample -- perturbs the schedule by 0.5-1 % (same-box A/B), so that launch keeps the plain instantiation.
        if constexpr (EO) { if (!per_sample_export && __all(tr_seen == 0.0f)) { j_stop = j + 1u; break; } }
        rb_prev = rb_next;
        if constexpr (MODE != MLP_F16X3) {   // un-pipelined modes: geometry of the next sample
            const uint32_t jn = j + 2u <= T ? j + 2u : T;
            bnext_n = bin_at(jn);
            rb_next_n = real_bin(rs, bnext_n);
            tmid_n = (rb_next_n + (j + 2u <= T ? rb_next : rb_prev)) / 2.0f;
            sample_x01(a.rc, rs, tmid_n, p_n, x01_n);
        }
    }

    if constexpr (!PT) clock_probe(1);
    if constexpr (AUX) {            // the feature stage reads every weight: the samples behind the exact early-out carry weight 0 (and are skipped there too)
        if (a.w_out) for (uint32_t jj = j_stop; jj < T; ++jj) a.w_out[(size_t)jj * Npad + r] = 0.0f;
    }
    if constexpr (LT) {
        // geometry channels, once per ray: W3[1 + c] . (sum_j w_j relu(h2_j)); both tiles' shares, then the half-wave exchange
#pragma unroll 1
        for (int c = 0; c < GEO; ++c) {
            const float *wr = w3p + (1 + c) * 32;
            const float q0 = dot32_lds(wr, hacc[0]), q1 = dot32_lds(wr, hacc[1]);
            auto qq = __builtin_amdgcn_permlane32_swap(__float_as_uint(q0), __float_as_uint(q1), false, false);
            const float v = __uint_as_float(qq[0]) + __uint_as_float(qq[1]);
            // (runtime c: keeps the loop rolled; fimg is indexed statically below)
            switch (c) {
#define SN_FIMG_CASE(I) case I: fimg[I] = v; break;
                SN_FIMG_CASE(0) SN_FIMG_CASE(1) SN_FIMG_CASE(2) SN_FIMG_CASE(3) SN_FIMG_CASE(4) SN_FIMG_CASE(5) SN_FIMG_CASE(6) SN_FIMG_CASE(7)
                SN_FIMG_CASE(8) SN_FIMG_CASE(9) SN_FIMG_CASE(10) SN_FIMG_CASE(11) SN_FIMG_CASE(12) SN_FIMG_CASE(13) SN_FIMG_CASE(14)
#undef SN_FIMG_CASE
                default: break;
            }
        }
    }
    // ---- per-ray colour head: view_mlp(f_image) -> sigmoid -> + (1 - wsum) * bg (renderer.py:340-357) ----
    static_assert(VH <= IN && NCOL <= IN && IN * 64 <= 2 * 64 * SLAB_DW, "view MLP activations reuse the feature column / slab");
    if constexpr (MFMA && !PT) {
        // every wave marches the same T steps: once all are done the 32 KiB of packed MLP weights are dead and
        // the view-MLP weights take their place (keeps the workgroup under 80 KiB of LDS = 2 workgroups per CU).
        // (The persistent launch keeps the view weights in a region of their own: no wave waits for another there.)
        __syncthreads();
        stage_weights<NCOL, VH>(lds_vw, a.vw[0]);
        stage_weights<VH, VH>(lds_vw + VW0, a.vw[1]);
        stage_weights<VH, 3>(lds_vw + VW0 + VW1, a.vw[2]);
        __syncthreads();
    }
    __builtin_amdgcn_wave_barrier();
    float rgb[3];
    const float ws = (float)wsum;
    {   // sum_t w_t * SH_c(d) = SH_c(d) * sum_t w_t: the direction is constant along the ray
        // (renderer.py:293-295 evaluates it per sample), so the basis is evaluated once per ray.
        float sh[NSH];
        sh_degree4(dirn[0], dirn[1], dirn[2], sh);
#pragma unroll
        for (int c = 0; c < NSH; ++c) fimg[GEO + c] = sh[c] * ws;
    }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) fe[c * fstride] = fimg[c];
    dense_ldsw_col<NCOL, VH, 1>(lds_vw, fe, fe, fstride);
    dense_ldsw_col<VH, VH, 1>(lds_vw + VW0, fe, fe, fstride);
    {
        float v2[VH];
#pragma unroll
        for (int k = 0; k < VH; ++k) v2[k] = fe[k * fstride];
        dense_ldsw<VH, 3, 0>(lds_vw + VW0 + VW1, v2, rgb);
    }
    if (ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sg = 1.0f / (1.0f + expf_det(-rgb[c]));
            const float bgm = (1.0f - ws) * a.rc.bg;
            a.image[(size_t)n * a.istride + c] = sg + bgm;
        }
        a.depth[(size_t)n * a.sstride] = dep;
        a.wsum[(size_t)n * a.sstride] = ws;
        if (a.dbg_fimg) {
#pragma unroll
            for (int c = 0; c < NCOL; ++c) a.dbg_fimg[(size_t)n * a.fimg_stride + c] = fimg[c];
        }
        if (a.head_rgbd) {
            float *q = a.head_rgbd + (size_t)n * a.fimg_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = a.image[(size_t)n * a.istride + c];
            q[3] = dep;
        }
    }
}

template <typename TT, int L, int C, int H1, int H2, int NOUT, int VH, int MODE, int K, bool AUX = false, bool LT = false, bool L0L = false, bool EO = false, int NP = 3, bool PORD = false,
          bool CANON = false>
__global__ __launch_bounds__(256, MODE == MLP_VALU ? 1 : SN_FINAL_WAVES) void k_final_stage(FinalArgs a) {
    SN_POISON_ALL();
    static_assert(NP == 3 || (LT && !L0L && !AUX), "reduced-product MLP forms: plain linear-tail instantiations only");
    static_assert(!LT || (MODE == MLP_F16X3 && K >= 4 && K <= 8), "linear tail: split-fp16 MLP on the FinalLv path");
    static_assert(!L0L || (LT && sizeof(TT) == 2), "LDS-resident level 0: fp16 tables, linear-tail instantiation (80 KiB: 32 packed weights + 4 x 8 swizzled slabs + 16 level 0)");
    constexpr int SLAB_DW = L0L ? 16 : SLAB_STRIDE;       // dwords per slab row
    constexpr bool MFMA = MODE != MLP_VALU;
    constexpr int IN = L * C;
    constexpr int GEO = NOUT - 1;
    constexpr int NSH = 16;                       // sh degree 4 (network.py:97)
    constexpr int NCOL = GEO + NSH;
    static_assert(!MFMA || (IN == 32 && H1 == 64 && H2 == 64 && NOUT == 16), "MFMA path is the 32-64-64-16 MLP");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // ---- LDS carve-up ----
    //  MFMA : [ packed weights 32 KiB | per-wave feature slabs fe[IN][64] x 4 ]
    //  VALU : [ activation columns actA[64][256] | actB[64][256] ]  (weights read through the scalar cache)
    float *fe;            // this lane's feature column base
    uint32_t fstride;     // distance between consecutive features of one lane
    float *actB = nullptr;
    constexpr int VW0 = VH * PadIn<NCOL>::value, VW1 = VH * PadIn<VH>::value;   // third layer: 3 * PadIn<VH> floats follow
    float *lds_vw;        // view_mlp weights (padded rows), all three layers back to back
    uint32_t *slab_hi = nullptr, *slab_lo = nullptr;      // MLP_F16X3: this wave's split feature images
    if constexpr (MODE == MLP_F16X3) {
        static_assert(PACK16_U4 * 4 == PACK_FLOATS, "both packings fill the same 32 KiB");
        for (uint32_t i = threadIdx.x; i < (uint32_t)PACK16_U4; i += 256u)
            reinterpret_cast<uint4 *>(lds)[i] = reinterpret_cast<const uint4 *>(a.mlp_pack)[i];
        if constexpr (LT) { __syncthreads(); stage_w3p(lds + W3P_OFFSET, a.w[2]); }     // over the (unused) packed layer-3 operands
        constexpr int WAVE_SLAB = 2 * 64 * SLAB_DW;       // dwords: hi image + lo image
        float *wave_base = lds + PACK_FLOATS + (threadIdx.x >> 6) * WAVE_SLAB;
        slab_hi = reinterpret_cast<uint32_t *>(wave_base);
        slab_lo = slab_hi + 64 * SLAB_DW;
        if constexpr (L0L) {                              // level 0 of the main grid, rows as stored (half2 = one dword per vertex)
            uint32_t *l0w = reinterpret_cast<uint32_t *>(lds + PACK_FLOATS + 4 * WAVE_SLAB);
            const uint32_t rows0 = a.g.res[0] * a.g.res[0] * a.g.res[0];
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.table) + a.g.off[0];
            for (uint32_t i = threadIdx.x; i < rows0; i += 256u) l0w[i] = src[i];
        }
        fe = wave_base + (threadIdx.x & 63u);             // after the march the slab is reused as fp32 columns
        fstride = 64u;
        lds_vw = lds;                                     // overlays the packed weights once the march is over
    } else if constexpr (MODE == MLP_F32) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)PACK_FLOATS / 4u; i += 256u)
            reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(a.mlp_pack)[i];
        fe = lds + PACK_FLOATS + (threadIdx.x >> 6) * (IN * 64) + (threadIdx.x & 63u);
        fstride = 64u;
        lds_vw = lds;
    } else {
        fe = lds + threadIdx.x;
        actB = lds + 64 * 256 + threadIdx.x;
        fstride = 256u;
        lds_vw = lds + 2 * 64 * 256;
    }
    if constexpr (!MFMA) {
        stage_weights<NCOL, VH>(lds_vw, a.vw[0]);
        stage_weights<VH, VH>(lds_vw + VW0, a.vw[1]);
        stage_weights<VH, 3>(lds_vw + VW0 + VW1, a.vw[2]);
    }
    __syncthreads();
    clock_probe(0);
    const uint32_t *l0tab = reinterpret_cast<const uint32_t *>(lds + PACK_FLOATS + 4 * 2 * 64 * SLAB_DW);   // L0L: level 0 of the main grid

    FinalLds fl;
    fl.lds = lds; fl.fe = fe; fl.fstride = fstride; fl.actB = actB; fl.lds_vw = lds_vw; fl.slab_hi = slab_hi; fl.slab_lo = slab_lo; fl.l0tab = l0tab;
    // four consecutive wave tiles per workgroup tile (ray_of_lane)
    final_stage_rays<TT, L, C, H1, H2, NOUT, VH, MODE, K, AUX, LT, L0L, EO, NP, PORD, CANON, false>(a, fl, tile_id(a.rc) * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}

// ------------------------------------------------------------------------------------------
// persistent launch of the plain linear-tail final stage (k_final_stage_pt)
// ------------------------------------------------------------------------------------------
// The ordinary launch hands the dispatcher one 4-wave workgroup per 16x16-pixel tile, with barriers inside: the stage's time steps at
// multiples of 256 workgroups (tools/staircase.py), every workgroup stages 32 KiB of weights, and every wave waits at the end of its march
// for the slowest of the four.  Here ONE 8-wave workgroup per CU stays resident, stages all weights once -- the packed image with w3p in its
// place, the view weights in a region of their own, eight wave slabs: 32 + 80 + 8.4 KiB -- behind ONE barrier, and every wave then pulls
// wave tiles (the ids wave_tile_of takes) from eight queues: tile_queue_range().  A wave starts at queue blockIdx.x & 7 (the XCD the
// dispatcher is observed to place the workgroup on: speed only), and walks on to the next queue when one is exhausted; it ends after the
// eighth.  A fetch is one lane's atomicAdd on the queue's counter (zeroed on the stream ahead of the launch).  After the barrier no wave
// waits for another: no barrier, no flag, no spin; the loop is bounded by the fetches -- each one either takes a tile or retires a queue.
// Every ray is computed by final_stage_rays, the code of the ordinary launch: bit-identical outputs.
struct TileQueueArgs {
    uint32_t *ctr;       // [8] fetch counters, zero at the start of the launch
    uint32_t units;      // workgroup tiles (256 rays) of the ordinary launch of the same rays: blocks_for()
};
// the queues' counters back to zero, on the stream ahead of the launch that fetches from them (a kernel like every other node of the
// call: captured and replayed with it)
__global__ void k_tile_queue_reset(uint32_t *ctr) {
    if (blockIdx.x == 0 && threadIdx.x < 8u) ctr[threadIdx.x] = 0u;
}
template <typename TT, int K>
__global__ __launch_bounds__(512, 2) void k_final_stage_pt(FinalArgs a, TileQueueArgs q) {
    SN_POISON_ALL();
    constexpr int VIEW_FLOATS = 32 * PadIn<31>::value + 32 * PadIn<32>::value + 3 * PadIn<32>::value;
    constexpr int WAVE_SLAB = 2 * 64 * SLAB_STRIDE;       // dwords: hi image + lo image
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *const lds_vw = lds + PACK_FLOATS + 8 * WAVE_SLAB;
    static_assert(W3P_OFFSET % 4 == 0 && W3P_FLOATS % 4 == 0, "w3p is a whole number of 16-byte pieces of the weight image");
    // the weight image but for the (unused) packed layer-3 operands w3p replaces: nothing below writes a word twice
    for (uint32_t i = threadIdx.x; i < (uint32_t)PACK16_U4; i += 512u)
        if (i < (uint32_t)(W3P_OFFSET / 4) || i >= (uint32_t)((W3P_OFFSET + W3P_FLOATS) / 4)) reinterpret_cast<uint4 *>(lds)[i] = reinterpret_cast<const uint4 *>(a.mlp_pack)[i];
    stage_w3p(lds + W3P_OFFSET, a.w[2]);
    stage_weights<31, 32>(lds_vw, a.vw[0]);
    stage_weights<32, 32>(lds_vw + 32 * PadIn<31>::value, a.vw[1]);
    stage_weights<32, 3>(lds_vw + 32 * PadIn<31>::value + 32 * PadIn<32>::value, a.vw[2]);
    static_assert(VIEW_FLOATS == 32 * 32 + 32 * 32 + 3 * 32, "the view weights' region (LDS_F16X3_PT)");
    __syncthreads();                                      // the only one
    clock_probe(0);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    float *wave_base = lds + PACK_FLOATS + wave * WAVE_SLAB;
    FinalLds fl;
    fl.lds = lds; fl.fe = wave_base + lane; fl.fstride = 64u; fl.actB = nullptr; fl.lds_vw = lds_vw;
    fl.slab_hi = reinterpret_cast<uint32_t *>(wave_base); fl.slab_lo = fl.slab_hi + 64 * SLAB_STRIDE; fl.l0tab = nullptr;
    // wave tiles that hold rays (ids beyond them are the padding of the last workgroup tile: nothing to compute, nothing to store)
    uint32_t ntiles;
    if (a.rc.W) {
        const uint32_t tlw = a.rc.tlw, tlh = 6u - tlw;
        ntiles = ((a.rc.W + (1u << tlw) - 1u) >> tlw) * ((a.rc.rows + (1u << tlh) - 1u) >> tlh);
    } else ntiles = (a.rc.N + 63u) >> 6;
    const uint32_t home = blockIdx.x & 7u;
    for (uint32_t k = 0; k < 8u;) {                       // queues home, home + 1, ... (mod 8)
        const uint32_t x = (home + k) & 7u;
        uint32_t begin, end;
        tile_queue_range(x, q.units, a.rc.xcd_swizzle, begin, end);
        if (begin >= end) { ++k; continue; }
        uint32_t t = 0;
        if (lane == 0u) t = atomicAdd(&q.ctr[x], 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t >= end - begin) { ++k; continue; }          // exhausted: on to the next queue
        const uint32_t g = begin + t;
        if (g < ntiles) {
            // The arguments are read again for every tile, through a pointer the optimiser cannot see through: hoisted out of this loop,
            // the scalar loads of the whole march stay live across it and their spills cost the march vector registers it does not have.
            // (FinalArgs is the kernel's first argument: offset 0 of the kernarg segment.)
            typedef __attribute__((address_space(4))) const FinalArgs cst_final_args;
            cst_final_args *ap = (cst_final_args *)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ap));
            final_stage_rays<TT, 16, 2, 64, 64, 16, 32, MLP_F16X3, K, false, true, false, false, 3, false, false, true>(*(const FinalArgs *)ap, fl, g);
        }
    }
    clock_probe(1);
}

// ------------------------------------------------------------------------------------------
// final stage for fields of OTHER sizes (k_final_stage_any)
// ------------------------------------------------------------------------------------------
// renderer.py:221-357 does not care how large the field is: run() calls self.density / self(...) of whatever subclass it is
// given (BASELINE configs[0]: L = 8 levels, T = 2^14, a 16-32-16 grid_mlp and a 31-32-3 view_mlp).  The kernels above are
// instantiated for NeRFNetwork's own sizes (network.py:93-98); this one takes every size at run time, for any field of the
// same STRUCTURE -- hash / tiled grid with level_dim 2 (up to 16 levels), bias-free ReLU grid_mlp -> [sigma_raw | geo_feat],
// trunc_exp, compositing, degree-4 SH of the view direction, bias-free ReLU view_mlp, sigmoid -- with up to 4 layers per
// MLP, layers up to 64 wide and up to 31 geometry channels.  One lane = one ray as everywhere; a lane's activations live in
// its own LDS columns ([row][256 lanes]: two ping-pong buffers of 16 / 32 / 64 rows + the compositing rows; 160 KiB at the widest),
// the weights are wave-uniform and come through the scalar cache, every neuron is one k-ascending fmaf chain and the grid
// blend is k_grid_forward's (grid.hip) -- i.e. the oracle's arithmetic in the oracle's order.  No matrix cores: a field
// this small is bound by its launch, and the proposal stages in front of it (if the field has the reference's) stay fused.
struct AnyShape {
    uint32_t ng, nv;               // linear layers of grid_mlp / view_mlp
    uint32_t dg[5], dv[5];         // widths: dg[0] = L * 2 ... dg[ng] = 1 + geo;  dv[0] = geo + 16 ... dv[nv] = 3
    const float *wg[4], *wv[4];    // nn.Linear.weight [out][in]
    uint32_t rows;                 // LDS rows per activation buffer (16 / 32 / 64); 2 * rows + geo rows of 256 floats in all
};
constexpr uint32_t ANY_W = 64, ANY_GEO = 31, ANY_LAYERS = 4;

// one layer: the lane's inputs come out of its LDS column ONCE into registers (a first version read them inside the k loop: one LDS round
// trip per multiply-add, 2.2 ms for a 64x64 image of the configs[0] field); the weights are wave-uniform (scalar loads, 8 at a time); the k
// loop is unrolled for the bucket INB >= in, whole groups of 8 beyond `in` are skipped, a partial group multiplies clamped weights by 0 --
// fmaf(0, x, acc) = acc -- so every neuron is still the oracle's k-ascending chain
template <int INB>
__device__ __forceinline__ void dense_any_b(const float *__restrict__ W, uint32_t in, uint32_t out, bool relu, const float *xin, float *yout) {
    float x[INB];
#pragma unroll
    for (int k = 0; k < INB; ++k) {      // rows beyond `in` exist (buffers hold the bucket) but may hold anything, NaN included: 0 * NaN is NaN, so they read as 0
        const float t = xin[(uint32_t)k * 256u];
        x[k] = (uint32_t)k < in ? t : 0.0f;
    }
    // four neurons at a time: their scalar weight loads are in flight together and their four chains interleave (one wave per SIMD when the
    // batch is small: a single dependent chain would run at the latency of every instruction)
    for (uint32_t o0 = 0; o0 < out; o0 += 4u) {
        const float *w[4];
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) w[q] = W + (size_t)umin(o0 + q, out - 1u) * in;      // (a tail group repeats the last neuron: not stored)
#pragma unroll
        for (int g = 0; g < INB / 8; ++g) {
            if (8u * (uint32_t)g < in) {
                if (8u * (uint32_t)g + 8u <= in) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
#pragma unroll
                        for (uint32_t q = 0; q < 4u; ++q) acc[q] = __builtin_fmaf(w[q][8 * g + j], x[8 * g + j], acc[q]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t kk = 8u * (uint32_t)g + (uint32_t)j;
#pragma unroll
                        for (uint32_t q = 0; q < 4u; ++q) {
                            const float wk = w[q][kk < in ? kk : in - 1u];
                            acc[q] = __builtin_fmaf(kk < in ? wk : 0.0f, x[8 * g + j], acc[q]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            if (o0 + q < out) yout[(o0 + q) * 256u] = relu ? relu_ieee(acc[q]) : acc[q];
        }
    }
}
__device__ __forceinline__ void dense_any(const float *__restrict__ W, uint32_t in, uint32_t out, bool relu, const float *xin, float *yout) {
    if (in <= 16u) dense_any_b<16>(W, in, out, relu, xin, yout);
    else if (in <= 32u) dense_any_b<32>(W, in, out, relu, xin, yout);
    else dense_any_b<64>(W, in, out, relu, xin, yout);
}

template <typename TT>
__global__ __launch_bounds__(256) void k_final_stage_any(FinalArgs a, AnyShape s) {
    SN_POISON_ALL();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t rows = s.rows;                      // rows of a ping-pong buffer: the widest layer, rounded up to the unroll bucket
    float *bufA = lds + threadIdx.x, *bufB = lds + rows * 256u + threadIdx.x, *accf = lds + 2u * rows * 256u + threadIdx.x;
    uint32_t n;
    const uint32_t wg = tile_id(a.rc);
    const bool ok = ray_of_lane(a.rc, wg, n);
    const uint32_t r = wg * 256u + threadIdx.x;
    const uint32_t Npad = a.rc.Npad;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    const uint32_t T = a.T, L = a.g.L, GEO = s.dg[s.ng] - 1u, NCOL = GEO + 16u;
    const float b0step = 1.0f / (float)T;
    auto bin_at = [&](uint32_t j) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + r];
        if (a.bins0_tab) return a.bins0_tab[(size_t)n * a.bins0_stride + j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };
    float dirn[3] = {rs.d[0], rs.d[1], rs.d[2]};     // normalised twice like the reference (renderer.py:294, sphere_harmonics.py:82)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const float aa = dirn[0] * dirn[0], bb = dirn[1] * dirn[1], cc = dirn[2] * dirn[2];
        const float nrm = sqrtf((aa + bb) + cc);
        dirn[0] = dirn[0] / nrm; dirn[1] = dirn[1] / nrm; dirn[2] = dirn[2] / nrm;
    }
    for (uint32_t c = 0; c < GEO; ++c) accf[c * 256u] = 0.0f;
    float dep = 0.0f;
    double cum = 0.0, wsum = 0.0;
    const TT *table = reinterpret_cast<const TT *>(a.table);
    float bprev = bin_at(0);
    float rb_prev = real_bin(rs, bprev);
    if (ok && a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1)] = bprev;
    for (uint32_t j = 0; j < T; ++j) {
        const float bnext = bin_at(j + 1u);
        const float rb_next = real_bin(rs, bnext);
        const float tmid = (rb_next + rb_prev) / 2.0f;
        float p[3], x01[3];
        sample_x01(a.rc, rs, tmid, p, x01);
        // ---- grid features: gridencoder.cu:94-201 as k_grid_forward states it; four levels' rows requested before the first blend ----
        const bool oob = (x01[0] < 0.0f || x01[0] > 1.0f) || (x01[1] < 0.0f || x01[1] > 1.0f) || (x01[2] < 0.0f || x01[2] > 1.0f);
        for (uint32_t l0 = 0; l0 < L; l0 += 4u) {
            float pos[4][3], v[4][8][2];
#pragma unroll
            for (uint32_t gi = 0; gi < 4u; ++gi) {
                const uint32_t l = umin(l0 + gi, L - 1u);                   // (a group's tail repeats the last level: fetched, not stored)
                const uint32_t res = a.g.res[l], size = a.g.size[l], mode = a.g.mode[l];
                const TT *tab = table + (size_t)a.g.off[l] * 2u;
                float deriv[3];
                uint32_t cell[3];
                grid_locate<3>(x01, res, a.g.align_corners != 0, a.g.interp, pos[gi], deriv, cell);
#pragma unroll
                for (uint32_t idx = 0; idx < 8u; ++idx) {
                    uint32_t q[3];
#pragma unroll
                    for (uint32_t d = 0; d < 3u; ++d) q[d] = (idx & (1u << d)) ? umin(cell[d] + 1u, res - 1u) : cell[d];
                    load_row<TT, 2>(tab + (size_t)grid_row<3>(q, res, size, mode) * 2u, v[gi][idx]);
                }
            }
#pragma unroll
            for (uint32_t gi = 0; gi < 4u; ++gi) {
                float acc[2] = {0.0f, 0.0f};
#pragma unroll
                for (uint32_t idx = 0; idx < 8u; ++idx) {
                    float w = 1.0f;
#pragma unroll
                    for (uint32_t d = 0; d < 3u; ++d) w *= (idx & (1u << d)) ? pos[gi][d] : 1.0f - pos[gi][d];
                    acc[0] = __builtin_fmaf(w, v[gi][idx][0], acc[0]);
                    acc[1] = __builtin_fmaf(w, v[gi][idx][1], acc[1]);
                }
                if (l0 + gi < L) {
                    bufA[(2u * (l0 + gi)) * 256u] = oob ? 0.0f : acc[0];
                    bufA[(2u * (l0 + gi) + 1u) * 256u] = oob ? 0.0f : acc[1];
                }
            }
        }
        // ---- grid_mlp (network.py:146-153): the lane's own LDS columns, in -> out ping-pong ----
        float *xin = bufA, *xout = bufB;
        for (uint32_t i = 0; i < s.ng; ++i) {
            dense_any(s.wg[i], s.dg[i], s.dg[i + 1u], i + 1u < s.ng, xin, xout);
            float *t = xin; xin = xout; xout = t;
        }
        const float sigma = expf_det(xin[0]);                // network.py:151
        const float delta = rb_next - rb_prev;
        float ds = delta * sigma;
        if (a.rc.last_opaque && j == T - 1u) ds = __builtin_inff();
        const float alpha = 1.0f - expf_det(-ds);
        const float tr = expf_det(-(float)cum);
        float w = alpha * tr;
        if (w != w) w = 0.0f;
        cum += (double)ds;
        wsum += (double)w;
        dep = __builtin_fmaf(w, tmid, dep);
        for (uint32_t c = 0; c < GEO; ++c) accf[c * 256u] = __builtin_fmaf(w, xin[(1u + c) * 256u], accf[c * 256u]);
        if (a.w_out) a.w_out[(size_t)j * Npad + r] = w;
        if (ok) {
            if (a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1) + j + 1] = bnext;
            if (a.dbg_sigma) a.dbg_sigma[(size_t)n * T + j] = sigma;
            if (a.dbg_w) a.dbg_w[(size_t)n * T + j] = w;
            if (a.dbg_xyz) { float *q = a.dbg_xyz + ((size_t)n * T + j) * 3; q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
            if (a.dbg_geo) { float *q = a.dbg_geo + ((size_t)n * T + j) * GEO; for (uint32_t c = 0; c < GEO; ++c) q[c] = xin[(1u + c) * 256u]; }
        }
        if (a.stop_cum > 0.0f && __all((float)cum > a.stop_cum)) break;
        rb_prev = rb_next;
    }
    // ---- per-ray colour head: view_mlp([f_geo | SH(d) * sum w]) -> sigmoid -> + (1 - sum w) * bg (renderer.py:340-357) ----
    const float ws = (float)wsum;
    {
        float sh[16];
        sh_degree4(dirn[0], dirn[1], dirn[2], sh);
        for (uint32_t c = 0; c < GEO; ++c) bufA[c * 256u] = accf[c * 256u];
#pragma unroll
        for (uint32_t c = 0; c < 16u; ++c) bufA[(GEO + c) * 256u] = sh[c] * ws;
    }
    if (ok && a.dbg_fimg) for (uint32_t c = 0; c < NCOL; ++c) a.dbg_fimg[(size_t)n * a.fimg_stride + c] = bufA[c * 256u];
    float *xin = bufA, *xout = bufB;
    for (uint32_t i = 0; i < s.nv; ++i) {
        dense_any(s.wv[i], s.dv[i], s.dv[i + 1u], i + 1u < s.nv, xin, xout);
        float *t = xin; xin = xout; xout = t;
    }
    if (ok) {
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            const float sg = 1.0f / (1.0f + expf_det(-xin[c * 256u]));
            const float bgm = (1.0f - ws) * a.rc.bg;
            a.image[(size_t)n * a.istride + c] = sg + bgm;
        }
        a.depth[(size_t)n * a.sstride] = dep;
        a.wsum[(size_t)n * a.sstride] = ws;
    }
}

#ifdef SN_EXPERIMENTS
#include "render_experiments.inc"
#endif

// ------------------------------------------------------------------------------------------
// final stage with per-ray termination and wave-level compaction of live samples (opt-in: cfg->compact_live)
// ------------------------------------------------------------------------------------------
// k_final_stage walks every ray of a wave through all T samples in lock-step; a gather instruction, an MFMA or a vector
// instruction costs the same with 1 or 64 lanes active, so a ray that is already opaque (early_stop_eps), a ray that
// misses the aabb (renderer.py:133-135) or a lane beyond the image edge only saves time once the WHOLE wave is dead.
// Here a lane is no longer tied to a ray during the sample evaluation:
//   * home lane r keeps ray r's compositing state (optical depth, colour features, next unassigned sample);
//   * every iteration the wave ballots the rays that still want samples, ranks them with mbcnt (prefix count of the
//     ballot) and deals its 64 evaluation slots out to them round-robin: slot s evaluates sample j_r + s / L of the
//     (s mod L)-th live ray (ds_permute builds the compacted list, ds_bpermute hands out ray ids and cursors), up to
//     CMP_KMAX consecutive samples per ray and iteration -> the 64 rows of every MFMA tile and every gather instruction
//     are filled with live samples only;
//   * slots write (delta*sigma, geometry features, t_mid) to LDS, home lanes composite their own samples in ascending
//     order exactly like k_final_stage (fp64 optical depth, one fmaf chain per channel) and decide termination.
// The assignment of iteration i+1 is made before iteration i has been composited (its first gather group is in flight
// across the matrix-core phase, as in k_final_stage), so a ray that dies in iteration i still occupies its slots of
// iteration i+1; their results are dropped.  With nothing to skip (every ray live for all T samples) slot s IS ray s and
// the outputs are bit-identical to k_final_stage.  Per-ray state of the slots (origin, direction, spacing) sits in the 4
// padding dwords of the wave's two feature-slab images, the per-sample records reuse the slab rows: no extra LDS.
constexpr uint32_t CMP_KMAX = 4;

template <typename TT, int K, bool CANON = false>
__global__ __launch_bounds__(256, 2) void k_final_stage_cmp(FinalArgs a) {
    SN_POISON_ALL();
    constexpr int L = 16, GEO = 15, NSH = 16, NCOL = GEO + NSH, VH = 32, PG = 4, IN = 32;
    constexpr int VW0 = VH * PadIn<NCOL>::value, VW1 = VH * PadIn<VH>::value;
    constexpr int WAVE_SLAB = 2 * 64 * SLAB_STRIDE;
    static_assert(K >= PG && K <= 8, "FinalLv instantiation");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    for (uint32_t i = threadIdx.x; i < (uint32_t)PACK16_U4; i += 256u)
        reinterpret_cast<uint4 *>(lds)[i] = reinterpret_cast<const uint4 *>(a.mlp_pack)[i];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float *wave_base = lds + PACK_FLOATS + wave * WAVE_SLAB;
    uint32_t *slab_hi = reinterpret_cast<uint32_t *>(wave_base), *slab_lo = slab_hi + 64 * SLAB_STRIDE;
    float *fe = wave_base + lane;
    __syncthreads();
    clock_probe(0);

    uint32_t n;
    const uint32_t wg = tile_id(a.rc);
    const bool ok = ray_of_lane(a.rc, wg, n);
    const uint32_t col0 = wg * 256u + wave * 64u;                 // scratch column of the wave's lane 0
    const uint32_t Npad = a.rc.Npad, T = a.T;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    bool alive = ok;
    if (ray_misses(a.rc, rs)) alive = false;              // renderer.py:133-135; it is skipped here (weights 0)
    // ray table in the slab's padding columns (dwords 16..19 of each 20-dword row)
    *reinterpret_cast<float4 *>(slab_hi + lane * SLAB_STRIDE + 16) = make_float4(rs.o[0], rs.o[1], rs.o[2], rs.s_near);
    *reinterpret_cast<float4 *>(slab_lo + lane * SLAB_STRIDE + 16) = make_float4(rs.d[0], rs.d[1], rs.d[2], rs.s_far);
    __builtin_amdgcn_wave_barrier();
    const float b0step = 1.0f / (float)T;
    auto bin_col = [&](uint32_t j, uint32_t col) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + col];
        if (a.bins0_tab) return a.bins0_tab[j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };

    // ---- home-lane state ----
    float fimg[GEO];
#pragma unroll
    for (int c = 0; c < GEO; ++c) fimg[c] = 0.0f;
    float dep = 0.0f;
    double cum = 0.0, wsum = 0.0;
    uint32_t j_cur = 0;                                           // next sample of this ray not yet assigned to a slot

    // ---- assignment of the wave's 64 slots ----
    struct Assign { uint32_t L, rank, n; };                       // live rays (uniform); this ray's rank and sample count
    uint32_t s_ray = lane, s_j = 0;                               // slot view: ray (lane index inside the wave) and sample
    auto assign = [&](Assign &as) {
        const bool want = alive && j_cur < T;
        const uint64_t M = __ballot(want);
        const uint32_t Lc = (uint32_t)__popcll(M);
        as.L = Lc; as.rank = 0; as.n = 0;
        if (Lc == 0u) { s_ray = lane; s_j = T - 1u; return; }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
        const uint32_t dst = want ? rank : Lc + (lane - rank);    // a permutation: live rays first, in lane order
        const uint32_t list = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)lane);
        const uint32_t inv = (uint32_t)(65536.0f / (float)Lc) + 1u;   // (x * inv) >> 16 == x / Lc for x < 64, Lc <= 64
        const uint32_t q = (lane * inv) >> 16, rnk = lane - q * Lc;
        s_ray = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(rnk << 2), (int)list);
        const uint32_t jr = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(s_ray << 2), (int)j_cur);
        const uint32_t sj = jr + q;
        s_j = (q < CMP_KMAX && sj < T) ? sj : T - 1u;             // surplus slots redo an in-range sample; nobody reads them
        uint32_t cnt = (((63u - rank) * inv) >> 16) + 1u;         // slots rank, rank + L, ... below 64
        cnt = umin(umin(cnt, CMP_KMAX), T - umin(j_cur, T));
        as.rank = rank; as.n = want ? cnt : 0u;
        j_cur += as.n;
    };
    float tmid_n, delta_n, p_n[3], x01_n[3];
    bool last_n;
    auto slot_geometry = [&]() {
        const float4 A = *reinterpret_cast<const float4 *>(slab_hi + s_ray * SLAB_STRIDE + 16);
        const float4 B = *reinterpret_cast<const float4 *>(slab_lo + s_ray * SLAB_STRIDE + 16);
        RaySetup q;
        q.o[0] = A.x; q.o[1] = A.y; q.o[2] = A.z; q.s_near = A.w;
        q.d[0] = B.x; q.d[1] = B.y; q.d[2] = B.z; q.s_far = B.w;
        const uint32_t col = col0 + s_ray;
        const float rb_prev = real_bin(q, bin_col(s_j, col)), rb_next = real_bin(q, bin_col(s_j + 1u, col));
        tmid_n = (rb_next + rb_prev) / 2.0f;
        delta_n = rb_next - rb_prev;
        last_n = s_j == T - 1u;
        sample_x01(a.rc, q, tmid_n, p_n, x01_n);
    };

    Assign cur, nxt;
    GroupRegs<TT, 2, PG> g0;
    assign(cur);
    slot_geometry();
    bool fast_n = all_interior(a.lv, x01_n);
    issue_group_lv<TT, PG, K, 0, false>(a.lv, x01_n, g0);
    __builtin_amdgcn_sched_barrier(0);
    while (cur.L != 0u) {
        const float tmid = tmid_n, delta = delta_n;
        const bool last = last_n;
        const float x01[3] = {x01_n[0], x01_n[1], x01_n[2]};
        float h[16];
        uint32_t *row_hi = slab_hi + lane * SLAB_STRIDE, *row_lo = slab_lo + lane * SLAB_STRIDE;
        auto emit = [&](int l, const float (&acc)[2]) {
            uint32_t ph, pl;
            split2(acc[0], acc[1], ph, pl);
            row_hi[l] = ph;
            row_lo[l] = pl;
        };
        blend_group<TT, 2, PG, K, 0>(g0, emit);
        __builtin_amdgcn_sched_barrier(0);
        auto rest = [&](auto fast_tag) {
            constexpr bool FAST = decltype(fast_tag)::value;
            static_for<1, L / PG>([&](auto gg) {
                constexpr int GRP = decltype(gg)::value;
                GroupRegs<TT, 2, PG> gr;
                issue_group_lv<TT, PG, K, GRP, FAST, !CANON>(a.lv, x01, gr);
                __builtin_amdgcn_sched_barrier(0);
                blend_span<TT, GRP * PG, PG, K, !CANON>(gr, emit);
                __builtin_amdgcn_sched_barrier(0);
            });
        };
        if (__builtin_expect(fast_n, 1)) rest(std::true_type{});
        else {
            rest(std::false_type{});
            const bool oob = (x01[0] < 0.0f || x01[0] > 1.0f) || (x01[1] < 0.0f || x01[1] > 1.0f) || (x01[2] < 0.0f || x01[2] > 1.0f);
            if (__builtin_expect(__any(oob), 0)) {
                if (oob) for (int l = 0; l < L; ++l) { row_hi[l] = 0u; row_lo[l] = 0u; }
            }
        }
        // next assignment (from the termination state of one iteration ago) + its first gather group
        assign(nxt);
        slot_geometry();
        fast_n = all_interior(a.lv, x01_n);
        issue_group_lv<TT, PG, K, 0, false>(a.lv, x01_n, g0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_wave_barrier();
        grid_mlp_mfma16(reinterpret_cast<const uint4 *>(lds) + opaque_zero(), slab_hi, slab_lo, h);
        __builtin_amdgcn_wave_barrier();
        {   // per-sample record of this slot: [delta*sigma | 15 geometry features] in its hi row, t_mid in its lo row
            const float sigma = expf_det(h[0]);
            float ds = delta * sigma;
            if (a.rc.last_opaque && last) ds = __builtin_inff();
            float4 *rec = reinterpret_cast<float4 *>(row_hi);
            rec[0] = make_float4(ds, h[1], h[2], h[3]);
            rec[1] = make_float4(h[4], h[5], h[6], h[7]);
            rec[2] = make_float4(h[8], h[9], h[10], h[11]);
            rec[3] = make_float4(h[12], h[13], h[14], h[15]);
            reinterpret_cast<float *>(row_lo)[0] = tmid;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- compositing by the home lanes, samples in ascending order (renderer.py:308-338) ----
#pragma unroll 1
        for (uint32_t k = 0; k < CMP_KMAX; ++k) {
            const bool mine = k < cur.n && alive;
            if (!__any(mine)) break;
            if (mine) {
                const uint32_t slot = cur.rank + k * cur.L;
                const float4 *rec = reinterpret_cast<const float4 *>(slab_hi + slot * SLAB_STRIDE);
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const float tm = reinterpret_cast<const float *>(slab_lo + slot * SLAB_STRIDE)[0];
                const float g[GEO] = {r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
                const float ds = r0.x;
                const float alpha = 1.0f - expf_det(-ds);
                const float tr = expf_det(-(float)cum);
                float w = alpha * tr;
                if (w != w) w = 0.0f;
                cum += (double)ds;
                wsum += (double)w;
                dep = __builtin_fmaf(w, tm, dep);
#pragma unroll
                for (int c = 0; c < GEO; ++c) fimg[c] = __builtin_fmaf(w, g[c], fimg[c]);
                if (a.stop_cum > 0.0f && (float)cum > a.stop_cum) alive = false;   // remaining weights sum to < eps
            }
        }
        __builtin_amdgcn_wave_barrier();
        cur = nxt;
    }
    clock_probe(1);

    // ---- per-ray colour head (as in k_final_stage) ----
    __syncthreads();
    stage_weights<NCOL, VH>(lds, a.vw[0]);
    stage_weights<VH, VH>(lds + VW0, a.vw[1]);
    stage_weights<VH, 3>(lds + VW0 + VW1, a.vw[2]);
    __syncthreads();
    float dirn[3] = {rs.d[0], rs.d[1], rs.d[2]};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const float aa = dirn[0] * dirn[0], bb = dirn[1] * dirn[1], cc = dirn[2] * dirn[2];
        const float nrm = sqrtf((aa + bb) + cc);
        dirn[0] = dirn[0] / nrm; dirn[1] = dirn[1] / nrm; dirn[2] = dirn[2] / nrm;
    }
    const float ws = (float)wsum;
    float sh[NSH];
    sh_degree4(dirn[0], dirn[1], dirn[2], sh);
#pragma unroll
    for (int c = 0; c < GEO; ++c) fe[c * 64] = fimg[c];
#pragma unroll
    for (int c = 0; c < NSH; ++c) fe[(GEO + c) * 64] = sh[c] * ws;
    static_assert(IN * 64 <= 2 * 64 * SLAB_STRIDE, "view MLP activations reuse the slab");
    dense_ldsw_col<NCOL, VH, 1>(lds, fe, fe, 64u);
    dense_ldsw_col<VH, VH, 1>(lds + VW0, fe, fe, 64u);
    float rgb[3];
    {
        float v2[VH];
#pragma unroll
        for (int k = 0; k < VH; ++k) v2[k] = fe[k * 64];
        dense_ldsw<VH, 3, 0>(lds + VW0 + VW1, v2, rgb);
    }
    if (ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sg = 1.0f / (1.0f + expf_det(-rgb[c]));
            const float bgm = (1.0f - ws) * a.rc.bg;
            a.image[(size_t)n * a.istride + c] = sg + bgm;
        }
        a.depth[(size_t)n * a.sstride] = dep;
        a.wsum[(size_t)n * a.sstride] = ws;
        if (a.dbg_fimg) {
#pragma unroll
            for (int c = 0; c < GEO; ++c) a.dbg_fimg[(size_t)n * a.fimg_stride + c] = fimg[c];
#pragma unroll
            for (int c = 0; c < NSH; ++c) a.dbg_fimg[(size_t)n * a.fimg_stride + GEO + c] = sh[c] * ws;
        }
        if (a.head_rgbd) {
            float *q = a.head_rgbd + (size_t)n * a.fimg_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = a.image[(size_t)n * a.istride + c];
            q[3] = dep;
        }
    }
}

// ------------------------------------------------------------------------------------------
// final stage, sample-parallel variant for small linear-order batches (the counterpart of k_prop_stage_sp)
// ------------------------------------------------------------------------------------------
// 4096 rays are 16 workgroups of k_final_stage, each wave alone on its SIMD for T serial samples of ~19 us.  Here
// lpr = 2^lpr_log2 lanes share a ray and evaluate spl consecutive samples each (lpr * spl >= T) with the same
// pipelined gather / split-f16 MFMA code; per-sample results (delta*sigma, 15 geometry features, t_mid) are parked
// in LDS.  The order-sensitive parts then run exactly as in the one-lane-per-ray kernel: the ray's first lane forms
// the fp64 optical-depth prefix, every lane turns its own samples into weights, and each output channel is one
// sample-ascending fmaf chain (channels dealt out to the ray's lanes).  The view MLP runs redundantly on all lanes of
// a ray; the first one stores.  Bit-identical to k_final_stage<MLP_F16X3>.  No early termination here.
constexpr int FSP_ROW = 65;                  // floats per (sample slot, channel) row: 64 lanes + 1 (bank spread)
constexpr int FSP_CH = 16;                   // 15 geometry features + t_mid
constexpr int FSP_DEPTH_ROW = 31;            // activation row that carries the depth (view MLP reads rows 0..30)
constexpr uint32_t FSP_MAX_SPL = 4;
static size_t final_sp_lds_floats(uint32_t spl) {
    return (size_t)PACK_FLOATS + 4 * 2 * 64 * SLAB_STRIDE + 4 * 512 + 4 * (size_t)spl * FSP_CH * FSP_ROW;
}

template <typename TT, int K>
__global__ __launch_bounds__(256, 1) void k_final_stage_sp(FinalArgs a, uint32_t lpr_log2, uint32_t spl_log2) {
    SN_POISON_ALL();
    constexpr int L = 16, GEO = 15, NSH = 16, NCOL = GEO + NSH, VH = 32, PG = 4;
    constexpr int VW0 = VH * PadIn<NCOL>::value, VW1 = VH * PadIn<VH>::value;
    constexpr int WAVE_SLAB = 2 * 64 * SLAB_STRIDE;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    for (uint32_t i = threadIdx.x; i < (uint32_t)PACK16_U4; i += 256u)
        reinterpret_cast<uint4 *>(lds)[i] = reinterpret_cast<const uint4 *>(a.mlp_pack)[i];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, spl = 1u << spl_log2;
    float *wave_base = lds + PACK_FLOATS + wave * WAVE_SLAB;
    uint32_t *slab_hi = reinterpret_cast<uint32_t *>(wave_base), *slab_lo = slab_hi + 64 * SLAB_STRIDE;
    float *fe = wave_base + lane;                           // activation column of this lane (after the march)
    float *l_w = lds + PACK_FLOATS + 4 * WAVE_SLAB + wave * 512u;     // [ray][sample]: delta*sigma, then the weight
    float *l_cum = l_w + 256;                                         // [ray][sample]: (float) fp64 prefix of delta*sigma
    float *hs = lds + PACK_FLOATS + 4 * WAVE_SLAB + 4 * 512 + wave * (spl * FSP_CH * FSP_ROW);   // [slot][channel][lane]
    __syncthreads();

    const uint32_t lpr = 1u << lpr_log2, c = lane & (lpr - 1u), rw = lane >> lpr_log2, rpw = 64u >> lpr_log2;
    const uint32_t r = (blockIdx.x * 4u + wave) * rpw + rw;           // scratch column = ray index; the grid covers Npad
    const bool ok = r < a.rc.N;
    const uint32_t n = ok ? r : 0u;
    const uint32_t Npad = a.rc.Npad, T = a.T;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    const float b0step = 1.0f / (float)T;
    auto bin_at = [&](uint32_t j) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + r];
        if (a.bins0_tab) return a.bins0_tab[(size_t)n * a.bins0_stride + j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };
    float dirn[3] = {rs.d[0], rs.d[1], rs.d[2]};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const float aa = dirn[0] * dirn[0], bb = dirn[1] * dirn[1], cc = dirn[2] * dirn[2];
        const float nrm = sqrtf((aa + bb) + cc);
        dirn[0] = dirn[0] / nrm; dirn[1] = dirn[1] / nrm; dirn[2] = dirn[2] / nrm;
    }
    const TT *table = reinterpret_cast<const TT *>(a.table);
    const uint32_t jbase = c << spl_log2, rbase = rw << (lpr_log2 + spl_log2);   // first sample of this lane; ray's LDS row
    if (ok && a.dbg_bins && c == 0u) a.dbg_bins[(size_t)n * (T + 1)] = bin_at(0);

    // ---- march over this lane's samples; slots past T redo sample T-1 and store nothing ----
    GroupRegs<TT, 2, PG> g0;
    uint32_t j_n = jbase < T ? jbase : T - 1u;
    float rb_prev_n = real_bin(rs, bin_at(j_n));
    float bnext_n = bin_at(j_n + 1u);
    float rb_next_n = real_bin(rs, bnext_n);
    float tmid_n = (rb_next_n + rb_prev_n) / 2.0f;
    float p_n[3], x01_n[3];
    sample_x01(a.rc, rs, tmid_n, p_n, x01_n);
    issue_group<TT, 2, PG, K, 0>(table, a.g, x01_n, g0, a.pairs);
    __builtin_amdgcn_sched_barrier(0);
    for (uint32_t i = 0; i < spl; ++i) {
        const uint32_t jr = jbase + i, j = j_n;
        const float bnext = bnext_n, rb_next = rb_next_n, rb_prev = rb_prev_n, tmid = tmid_n;
        const float p[3] = {p_n[0], p_n[1], p_n[2]}, x01[3] = {x01_n[0], x01_n[1], x01_n[2]};
        float h[16];
        uint32_t *row_hi = slab_hi + lane * SLAB_STRIDE, *row_lo = slab_lo + lane * SLAB_STRIDE;
        auto emit = [&](int l, const float (&acc)[2]) {
            uint32_t ph, pl;
            split2(acc[0], acc[1], ph, pl);
            row_hi[l] = ph;
            row_lo[l] = pl;
        };
        blend_group<TT, 2, PG, K, 0>(g0, emit);
        __builtin_amdgcn_sched_barrier(0);
        static_for<1, L / PG>([&](auto gg) {
            constexpr int GRP = decltype(gg)::value;
            GroupRegs<TT, 2, PG> gr;
            issue_group<TT, 2, PG, K, GRP>(table, a.g, x01, gr, a.pairs);
            __builtin_amdgcn_sched_barrier(0);
            blend_group<TT, 2, PG, K, GRP>(gr, emit);
            __builtin_amdgcn_sched_barrier(0);
        });
        {
            const bool oob = (x01[0] < 0.0f || x01[0] > 1.0f) || (x01[1] < 0.0f || x01[1] > 1.0f) || (x01[2] < 0.0f || x01[2] > 1.0f);
            if (__builtin_expect(__any(oob), 0)) {
                if (oob) for (int l = 0; l < L; ++l) { row_hi[l] = 0u; row_lo[l] = 0u; }
            }
        }
        {   // geometry and first gather group of this lane's next sample (the last slot re-issues its own)
            const uint32_t jq = jr + 1u;
            j_n = (i + 1u < spl && jq < T) ? jq : j;
            rb_prev_n = real_bin(rs, bin_at(j_n));
            bnext_n = bin_at(j_n + 1u);
            rb_next_n = real_bin(rs, bnext_n);
            tmid_n = (rb_next_n + rb_prev_n) / 2.0f;
            sample_x01(a.rc, rs, tmid_n, p_n, x01_n);
            issue_group<TT, 2, PG, K, 0>(table, a.g, x01_n, g0, a.pairs);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_wave_barrier();
        grid_mlp_mfma16(reinterpret_cast<const uint4 *>(lds) + opaque_zero(), slab_hi, slab_lo, h);
        __builtin_amdgcn_wave_barrier();
        const float sigma = expf_det(h[0]);
        float ds = (rb_next - rb_prev) * sigma;
        if (a.rc.last_opaque && j == T - 1u) ds = __builtin_inff();
        if (jr < T) {
            l_w[rbase + jr] = ds;
            float *rec = hs + (size_t)(i * FSP_CH) * FSP_ROW + lane;
#pragma unroll
            for (int ch = 0; ch < GEO; ++ch) rec[ch * FSP_ROW] = h[1 + ch];
            rec[GEO * FSP_ROW] = tmid;
            if (ok) {
                if (a.dbg_bins) a.dbg_bins[(size_t)n * (T + 1) + jr + 1] = bnext;
                if (a.dbg_sigma) a.dbg_sigma[(size_t)n * T + jr] = sigma;
                if (a.dbg_xyz) { float *q = a.dbg_xyz + ((size_t)n * T + jr) * 3; q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
                if (a.dbg_geo) { float *q = a.dbg_geo + ((size_t)n * T + jr) * GEO;
#pragma unroll
                    for (int ch = 0; ch < GEO; ++ch) q[ch] = h[1 + ch]; }
            }
        }
    }
    __syncthreads();                          // per-sample records visible; the packed MLP weights are dead
    stage_weights<NCOL, VH>(lds, a.vw[0]);
    stage_weights<VH, VH>(lds + VW0, a.vw[1]);
    stage_weights<VH, 3>(lds + VW0 + VW1, a.vw[2]);
    if (c == 0u) {                            // optical depth before each sample: fp64 running sum, rounded per prefix
        double cum = 0.0;
        for (uint32_t j = 0; j < T; ++j) { l_cum[rbase + j] = (float)cum; cum += (double)l_w[rbase + j]; }
    }
    __syncthreads();
    for (uint32_t i = 0; i < spl; ++i) {      // weights of this lane's samples (renderer.py:308-325)
        const uint32_t j = jbase + i;
        if (j < T) {
            const float alpha = 1.0f - expf_det(-l_w[rbase + j]);
            const float tr = expf_det(-l_cum[rbase + j]);
            float w = alpha * tr;
            if (w != w) w = 0.0f;
            l_w[rbase + j] = w;
            if (a.w_out) a.w_out[(size_t)j * Npad + r] = w;
            if (ok && a.dbg_w) a.dbg_w[(size_t)n * T + j] = w;
        }
    }
    __syncthreads();
    // ---- compositing: one sample-ascending fmaf chain per channel, channels dealt out to the ray's lanes ----
    double wsum = 0.0;
    for (uint32_t j = 0; j < T; ++j) wsum += (double)l_w[rbase + j];
    float *ray_col = wave_base + (rw << lpr_log2);           // activation column of the ray's first lane (slab is dead)
    for (uint32_t ch = c; ch < (uint32_t)FSP_CH; ch += lpr) {
        float acc = 0.0f;
        for (uint32_t j = 0; j < T; ++j) {
            const uint32_t cj = j >> spl_log2, ij = j & (spl - 1u);
            acc = __builtin_fmaf(l_w[rbase + j], hs[(size_t)(ij * FSP_CH + ch) * FSP_ROW + (rw << lpr_log2) + cj], acc);
        }
        ray_col[(ch < (uint32_t)GEO ? ch : (uint32_t)FSP_DEPTH_ROW) * 64u] = acc;
    }
    const float ws = (float)wsum;
    if (c == 0u) {
        float sh[NSH];
        sh_degree4(dirn[0], dirn[1], dirn[2], sh);
#pragma unroll
        for (int k = 0; k < NSH; ++k) ray_col[(GEO + k) * 64] = sh[k] * ws;
    }
    __builtin_amdgcn_wave_barrier();          // the ray's lanes live in one wave; LDS serves a wave in order
    const float dep = ray_col[FSP_DEPTH_ROW * 64];
    if (ok && c == 0u && a.dbg_fimg) {
        for (int k = 0; k < NCOL; ++k) a.dbg_fimg[(size_t)n * a.fimg_stride + k] = ray_col[k * 64];
    }
    __builtin_amdgcn_wave_barrier();
    float rgb[3];
    dense_ldsw_col<NCOL, VH, 1>(lds, ray_col, fe, 64u);       // every lane of the ray: same inputs, own output column
    dense_ldsw_col<VH, VH, 1>(lds + VW0, fe, fe, 64u);
    {
        float v2[VH];
#pragma unroll
        for (int k = 0; k < VH; ++k) v2[k] = fe[k * 64];
        dense_ldsw<VH, 3, 0>(lds + VW0 + VW1, v2, rgb);
    }
    if (ok && c == 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float sg = 1.0f / (1.0f + expf_det(-rgb[k]));
            const float bgm = (1.0f - ws) * a.rc.bg;
            a.image[(size_t)n * a.istride + k] = sg + bgm;
        }
        a.depth[(size_t)n * a.sstride] = dep;
        a.wsum[(size_t)n * a.sstride] = ws;
        if (a.head_rgbd) {
            float *q = a.head_rgbd + (size_t)n * a.fimg_stride;
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = a.image[(size_t)n * a.istride + k];
            q[3] = dep;
        }
    }
}

// ------------------------------------------------------------------------------------------
// feature stage: f[n, :] = sum_j w[n,j] * feat_grid(xyz[n,j])   (renderer.py:301-302 + 361, the SAM head's f_sam)
// ------------------------------------------------------------------------------------------
// Runs after the final stage on the same lane -> ray mapping.  Sample positions are recomputed from the last
// stage's bins (scratch, coalesced) with the very same code the final stage uses, weights come from the final
// stage's scratch column; nothing per-sample is written.  A workgroup pass covers LG levels (blockIdx.y).
struct FeatArgs {
    RayCommon rc;
    GridLevels g;
    const void *table;
    uint32_t T;
    const float *bins_in;        // scratch [T+1][Npad] or NULL (single-stage)
    const float *bins0_tab;
    uint32_t bins0_stride;
    const float *w_in;           // scratch [T][Npad]
    float *out;                  // [N, L*C], rows out_stride floats apart
    uint32_t out_stride;         // L*C, or sn_render_io.head_stride
    uint32_t level0;             // first level of this launch (blockIdx.y counts passes of LG levels from here)
};

// wave-wide minimum / maximum of a float in six DPP steps (row_shr 1, 2, 4, 8 bring a row's extremum to its lane 15, row_bcast:15 / :31 carry
// it across the four rows to lane 63), returned wave-uniform.
template <bool MAXI>
__device__ __forceinline__ float wave_extremum(float v) {
    auto step = [&](auto ctrl_tag, auto rmask_tag) {
        constexpr int ctrl = decltype(ctrl_tag)::value, rmask = decltype(rmask_tag)::value;
        const float t = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp((int)__float_as_uint(v), (int)__float_as_uint(v), ctrl, rmask, 0xf, false));
        v = MAXI ? fmaxf(v, t) : fminf(v, t);
    };
    using I = std::integral_constant<int, 0>;
    (void)sizeof(I);
    step(std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), 63));
}

// PATCH (round 6; north_star "LDS staging of per-tile grid voxels"): on a DENSE level the 64 rays of a wave tile at one sample
// index occupy a handful of cells -- the bounding box of their vertices is 10-17 rows on levels 0-6 of the heads' grid
// (profiles/r06/gather_lines_per_level.txt) -- yet every lane issues its own 8 corner fetches (16 gather instructions per level with 32-byte
// rows, each at the texture path's per-instruction floor).  Here the wave fetches the box ONCE (lane v loads vertex v: one or two gather
// instructions), parks it in LDS and every lane reads its 8 corners from there.  Same rows, same blend: bit-identical.  A box beyond 64 vertices
// (wave-uniform test) and every hashed level take the ordinary path: on hashed levels a box fetches MORE lines than the direct gathers (same file).
// MEASURED SLOWER (profiles/r06/feat_patch_ab.json, same box): configs[2] 400x400 2.46 -> 2.64 ms (fp32 tables), 2.08 -> 2.22 (fp16); 800x800 6.81 -> 7.43 /
// 5.79 -> 6.32; one level per pass: 2.47 -> 2.53.  The dense levels' direct gathers touch 1.3-2.2 lines per instruction -- the texture path's best
// case -- while the staged form adds a box computation (six wave reductions per sample), an LDS write -> read round trip inside every level's
// dependent chain and twice the registers (192 vs 92: 2 instead of 5 waves per SIMD).  Third measured negative of LDS voxel staging on this chip
// (round 2: per-wave vertex cache in the last stage, round 3: LDS-resident level 0).  Opt-in: sn_render_tuning.feat_patch = 1.
constexpr uint32_t FEAT_PATCH_ROWS = 64;

template <typename TT, int C, int LG, bool PATCH = false>
__global__ __launch_bounds__(256) void k_feat_stage(FeatArgs a) {
    SN_POISON_ALL();
    __shared__ __attribute__((aligned(16))) TT patch_lds[PATCH ? 4 * LG * FEAT_PATCH_ROWS * C : 1];
    uint32_t n;
    const uint32_t wg = tile_id_x(a.rc, blockIdx.x, gridDim.x);
    const bool ok = ray_of_lane(a.rc, wg, n);
    const uint32_t r = wg * 256u + threadIdx.x;
    const uint32_t Npad = a.rc.Npad;
    RaySetup rs;
    setup_ray(a.rc, n, rs);
    const uint32_t T = a.T;
    const float b0step = 1.0f / (float)T;
    auto bin_at = [&](uint32_t j) -> float {
        if (a.bins_in) return a.bins_in[(size_t)j * Npad + r];
        if (a.bins0_tab) return a.bins0_tab[(size_t)n * a.bins0_stride + j];
        return linspace_at(0.0f, 1.0f, b0step, T + 1u, j);
    };
    const uint32_t l0 = a.level0 + blockIdx.y * LG;
    const TT *table = reinterpret_cast<const TT *>(a.table);
    const uint32_t lane = threadIdx.x & 63u;
    TT *my_patch = patch_lds + (PATCH ? (threadIdx.x >> 6) * (LG * FEAT_PATCH_ROWS * C) : 0u);
    float acc[LG][C];
#pragma unroll
    for (int i = 0; i < LG; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[i][c] = 0.0f;
    float rb_prev = real_bin(rs, bin_at(0));
    for (uint32_t j = 0; j < T; ++j) {
        const float rb_next = real_bin(rs, bin_at(j + 1u));
        const float tmid = (rb_next + rb_prev) / 2.0f;
        rb_prev = rb_next;
        const float w = a.w_in[(size_t)j * Npad + r];
        // a sample index at which all 64 rays of the wave carry weight exactly 0 (behind an opaque surface, in empty space) adds
        // fmaf(0, feature, acc) = acc: no position, no gathers.  Bit-identical (table values are finite).
        if (__all(w == 0.0f)) continue;
        float p[3], x01[3];
        sample_x01(a.rc, rs, tmid, p, x01);
        bool oob = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) if (x01[d] < 0.0f || x01[d] > 1.0f) oob = true;     // gridencoder.cu:105-130
        const float wz = oob ? 0.0f : w;
        float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        if constexpr (PATCH) {       // bounding box (in table coordinates) of the lanes whose sample counts; wave-uniform
            const bool act = wz != 0.0f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = wave_extremum<false>(act ? x01[d] : __builtin_inff());
                hi[d] = wave_extremum<true>(act ? x01[d] : -__builtin_inff());
            }
            if (!(lo[0] <= hi[0])) continue;              // no lane counts: every fmaf(0, feature, acc) would leave acc as it is
        }
        auto blend = [&](int i, const float (&ps)[3], const float (&cvi)[8][C]) {
            float feat[C];
#pragma unroll
            for (int c = 0; c < C; ++c) feat[c] = 0.0f;
#pragma unroll
            for (uint32_t idx = 0; idx < 8u; ++idx) {       // gridencoder.cu:171-192
                float cw = 1.0f;
#pragma unroll
                for (uint32_t d = 0; d < 3u; ++d) cw *= (idx & (1u << d)) ? ps[d] : 1.0f - ps[d];
#pragma unroll
                for (int c = 0; c < C; ++c) feat[c] = __builtin_fmaf(cw, cvi[idx][c], feat[c]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[i][c] = __builtin_fmaf(wz, feat[c], acc[i][c]);
        };
        if constexpr (!PATCH) {
            float pos[LG][3];
            float cv[LG][8][C];
#pragma unroll
            for (int i = 0; i < LG; ++i) {
                const uint32_t l = l0 + i;
                uint32_t cell[3], offs[8];
                locate_linear(x01, a.g.res[l], pos[i], cell);
                corner_offsets<-1, (uint32_t)(C * sizeof(TT))>(cell, a.g.res[l], a.g.size[l], a.g.mode[l], offs);
                const char *tab = reinterpret_cast<const char *>(table + (size_t)a.g.off[l] * C);
#pragma unroll
                for (int k = 0; k < 8; ++k) load_row<TT, C>(reinterpret_cast<const TT *>(tab + offs[k]), cv[i][k]);
            }
#pragma unroll
            for (int i = 0; i < LG; ++i) blend(i, pos[i], cv[i]);
        } else {
            // the boxes of all LG levels are fetched first (their gathers fly together), then every level is read back and blended
            uint32_t c0[LG][3], nd[LG][3];
            bool staged[LG];
#pragma unroll
            for (int i = 0; i < LG; ++i) {
                const uint32_t l = l0 + i;
                const uint32_t res = a.g.res[l];
                // vertices of the box: cells of lo .. hi (locate_linear is monotone in x01) plus the +1 corners, clamped like them (gridencoder.cu:182)
                const float rf = (float)res, top = (float)(res - 1u);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float p0 = __builtin_amdgcn_fmed3f(__builtin_fmaf(lo[d], rf, -0.5f), 0.0f, top);
                    const float p1 = __builtin_amdgcn_fmed3f(__builtin_fmaf(hi[d], rf, -0.5f), 0.0f, top);
                    c0[i][d] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p0);
                    const uint32_t c1 = umin((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p1) + 1u, res - 1u);
                    nd[i][d] = c1 - c0[i][d] + 1u;
                }
                const uint32_t nxy = nd[i][0] * nd[i][1], total = nxy * nd[i][2];
                const uint32_t mode = a.g.mode[l];
                staged[i] = (mode & 1u) == 0u && ((mode >> 4) & 15u) == 3u && ((mode >> 1) & 3u) == 0u && total <= FEAT_PATCH_ROWS;    // dense level, box fits
                if (staged[i]) {     // lane v fetches vertex v = ix + nx (iy + ny iz) of the box
                    TT *pl = my_patch + (uint32_t)i * (FEAT_PATCH_ROWS * C);
                    const char *tab = reinterpret_cast<const char *>(table + (size_t)a.g.off[l] * C);
                    const uint32_t iz = (uint32_t)(((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)nxy));
                    const uint32_t rem = lane - iz * nxy;
                    const uint32_t iy = (uint32_t)(((float)rem + 0.5f) * __builtin_amdgcn_rcpf((float)nd[i][0]));
                    const uint32_t ix = rem - iy * nd[i][0];
                    if (lane < total) {
                        const uint32_t row = (c0[i][0] + ix) + res * ((c0[i][1] + iy) + res * (c0[i][2] + iz));
                        const TT *src = reinterpret_cast<const TT *>(tab + (size_t)row * (C * sizeof(TT)));      // the row as it is stored
                        constexpr int RB = C * (int)sizeof(TT);
                        if constexpr (RB % 16 == 0) {
#pragma unroll
                            for (int q = 0; q < RB / 16; ++q) reinterpret_cast<uint4 *>(pl + lane * C)[q] = reinterpret_cast<const uint4 *>(src)[q];
                        } else {
#pragma unroll
                            for (int c = 0; c < C; ++c) pl[lane * C + c] = src[c];
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < LG; ++i) {
                const uint32_t l = l0 + i;
                const uint32_t res = a.g.res[l];
                uint32_t cell[3];
                float ps[3];
                float cvi[8][C];
                locate_linear(x01, res, ps, cell);
                if (staged[i]) {
                    // this lane's corners inside the box (a lane that does not count may lie outside: any row will do, its weight is 0)
                    const TT *pl = my_patch + (uint32_t)i * (FEAT_PATCH_ROWS * C);
                    uint32_t q0[3], q1[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        q0[d] = umin(cell[d] - c0[i][d], nd[i][d] - 1u);
                        q1[d] = umin(q0[d] + (cell[d] < res - 1u ? 1u : 0u), nd[i][d] - 1u);
                    }
#pragma unroll
                    for (uint32_t k = 0; k < 8u; ++k) {
                        const uint32_t v = ((k & 1u) ? q1[0] : q0[0]) + nd[i][0] * (((k & 2u) ? q1[1] : q0[1]) + nd[i][1] * ((k & 4u) ? q1[2] : q0[2]));
                        load_row<TT, C>(pl + v * C, cvi[k]);
                    }
                    blend(i, ps, cvi);
                } else {
                    uint32_t offs[8];
                    corner_offsets<-1, (uint32_t)(C * sizeof(TT))>(cell, res, a.g.size[l], a.g.mode[l], offs);
                    const char *tab = reinterpret_cast<const char *>(table + (size_t)a.g.off[l] * C);
#pragma unroll
                    for (int k = 0; k < 8; ++k) load_row<TT, C>(reinterpret_cast<const TT *>(tab + offs[k]), cvi[k]);
                    blend(i, ps, cvi);
                }
            }
            __builtin_amdgcn_wave_barrier();      // the next sample's box overwrites the patch: every lane has read its corners
        }
    }
    if (!ok) return;
    float *o = a.out + (size_t)n * a.out_stride + (size_t)l0 * C;
    const bool vec_ok = (a.out_stride & 3u) == 0u;          // (a [N, 163] head input: rows are not 16-byte aligned)
#pragma unroll
    for (int i = 0; i < LG; ++i) {
        if (C % 4 == 0 && vec_ok) {
#pragma unroll
            for (int q = 0; q < C / 4; ++q)
                reinterpret_cast<float4 *>(o + i * C)[q] = make_float4(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) o[i * C + c] = acc[i][c];
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// ---- optional per-kernel timing (bench.py's roofline leg) ---------------------------------
// When enabled, every kernel launched by sn_rm_render_rays is bracketed by hipEvents recorded
// on the caller's stream; sn_rm_profile_read() synchronises them and returns, per kernel class,
// the launch count and the summed device time.  Off by default (no events, no overhead).
// pair rows (fp32: row, +x neighbour) / quad rows (fp16: row, +x, +y, +x+y) of the dense levels (see PairTab): one
// thread per (level < K, row); 16 bytes per vertex either way
template <typename T>
__global__ void k_pack_pairs(const T *__restrict__ table, GridLevels g, PairTab pt, uint32_t K) {
    SN_POISON_ALL();
    const uint32_t l = blockIdx.y;
    if (l >= K) return;
    const uint32_t res = g.res[l], rows = res * res * res;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    // vertex (x, y, z) -> its row through the level's OWN index function (gridencoder.cu:45-79): for a dense level that is i itself;
    // a hashed level that is "densified" for this render (densify_levels below) is looked up through the hash, once per vertex, here
    const uint32_t x = i % res, y = (i / res) % res, z = i / (res * res);
    const uint32_t x1 = x + 1u < res ? x + 1u : x, y1 = y + 1u < res ? y + 1u : y;      // gridencoder.cu:182: the +1 neighbour is clamped to res-1
    const uint32_t size = g.size[l], mode = g.mode[l];
    auto row = [&](uint32_t xx, uint32_t yy) { const uint32_t p[3] = {xx, yy, z}; return grid_row<3>(p, res, size, mode); };
    const T *tab = table + (size_t)g.off[l] * 2u;
    if constexpr (sizeof(T) == 4) {
        const float2 a = reinterpret_cast<const float2 *>(tab)[row(x, y)], b = reinterpret_cast<const float2 *>(tab)[row(x1, y)];
        reinterpret_cast<float4 *>(const_cast<void *>(pt.base))[pt.off[l] + i] = make_float4(a.x, a.y, b.x, b.y);
    } else {
        const uint32_t *tw = reinterpret_cast<const uint32_t *>(tab);
        reinterpret_cast<uint4 *>(const_cast<void *>(pt.base))[pt.off[l] + i] = make_uint4(tw[row(x, y)], tw[row(x1, y)], tw[row(x, y1)], tw[row(x1, y1)]);
    }
}

// pair-row offsets of the dense prefix; returns the total number of pair rows (0 if the grid has no usable prefix)
static uint32_t pair_layout(const GridLevels &g, int K, uint32_t (&off)[8]) {
    uint32_t total = 0;
    for (int l = 0; l < 8; ++l) off[l] = 0;
    if (K <= 0 || K > 8 || g.C != 2) return 0;
    for (int l = 0; l < K; ++l) { off[l] = total; total += g.res[l] * g.res[l] * g.res[l]; }
    return total;
}

// FinalLv of a grid whose levels are "K dense (packed as pair / quad rows in pt), then hashed, equal-sized and contiguous".
// Returns false when the grid does not have that shape (the generic instantiation then runs).
static bool build_final_lv(const GridLevels &g, int K, const PairTab &pt, const void *table, uint32_t row_bytes, FinalLv &lv) {
    memset(&lv, 0, sizeof(lv));
    if (g.L > 16 || (uint32_t)K >= g.L || g.C != 2 || K < 1 || K > 8 || pt.base == nullptr) return false;
    const uint32_t size = g.size[K];
    if ((size & (size - 1)) != 0 || (uint64_t)size * row_bytes > (1u << 24)) return false;      // 24-bit multiplies cover the mask
    for (uint32_t l = (uint32_t)K; l < g.L; ++l) {
        if (g.size[l] != size || (l + 1 < g.L && g.off[l + 1] != g.off[l] + size) || g.res[l] >= (1u << 24)) return false;
        lv.h_off[l] = (g.off[l] - g.off[K]) * row_bytes;
    }
    lv.h_mask = (size - 1u) * row_bytes;
    lv.hash_base = reinterpret_cast<const char *>(table) + (size_t)g.off[K] * row_bytes;
    lv.pair_base = reinterpret_cast<const char *>(pt.base);
    for (uint32_t l = 0; l < g.L; ++l) { lv.res_f[l] = (float)g.res[l]; lv.top_f[l] = (float)(g.res[l] - 1u); }
    for (uint32_t l = 0; l < (uint32_t)K; ++l) {
        const uint32_t res = g.res[l];
        lv.d_sy[l] = res * 16u; lv.d_sz[l] = res * res * 16u;
        lv.d_ylim[l] = (res - 1u) * lv.d_sy[l]; lv.d_zlim[l] = (res - 1u) * lv.d_sz[l];
        lv.d_off[l] = pt.off[l] * 16u;
    }
    // one and a half cells of the coarsest hashed level: fl(x * res_l - 0.5) stays inside [0.99, res_l - 1.99] on every hashed level
    lv.in_lo = 1.5f / (float)g.res[K];
    lv.in_hi = 1.0f - 1.5f / (float)g.res[K];
    return true;
}

static thread_local sn_launch_info g_launch = {};

enum { PK_PACK = 0, PK_PROP0, PK_PROP1, PK_PROP2, PK_FINAL, PK_FEAT, PK_CLASSES };
struct ProfSpan { hipEvent_t a, b; int cls; };
static bool g_prof_on = false;
static std::vector<ProfSpan> g_prof;

struct ProfScope {
    hipStream_t st; int idx = -1;
    ProfScope(hipStream_t s, int cls) : st(s) {
        if (!g_prof_on) return;
        ProfSpan sp; sp.cls = cls;
        if (hipEventCreate(&sp.a) != hipSuccess || hipEventCreate(&sp.b) != hipSuccess) return;
        (void)hipEventRecord(sp.a, st);
        g_prof.push_back(sp); idx = (int)g_prof.size() - 1;
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(g_prof[idx].b, st); }
};

static int to_levels(GridLevels *g, const sn_grid_desc *d) {
    SN_REQUIRE(d->D == 3, "render: grids must be 3-D (got D=%u)", d->D);
    return build_grid_levels(g, d->offsets, d->D, d->C, d->L, d->S, d->H, d->gridtype, (int)d->align_corners, d->interp);
}

// number of leading dense levels if the grid is "dense prefix, hashed tail" (every grid the reference builds is:
// resolution grows with the level), else -1 (generic run-time level kind)
static int dense_prefix(const GridLevels &g) {
    uint32_t k = 0;
    while (k < g.L && (g.mode[k] & 1u) == 0u) ++k;
    for (uint32_t l = k; l < g.L; ++l) if ((g.mode[l] & 1u) == 0u) return -1;
    if (k == g.L) return -1;   // the paired x-loads of dense levels rely on a hashed level following the dense prefix
    return (int)k;
}

static bool mlp_is(const sn_mlp_desc *m, uint32_t nl, const uint32_t *dims) {
    if (m->num_layers != nl || m->activation != 0 || m->skip_mask != 0) return false;
    for (uint32_t l = 0; l <= nl; ++l) if (m->dims[l] != dims[l]) return false;
    for (uint32_t l = 0; l < nl; ++l) if (m->bias[l] != nullptr || m->weight[l] == nullptr) return false;
    return true;
}

static uint32_t chunk_rays(uint32_t N, uint32_t W) {
    // keep a launch's scratch bounded; image mode splits on 16-row boundaries
    const uint32_t cap = 1u << 21;
    if (N <= cap) return N;
    if (W) { uint32_t rows = (cap / W) & ~15u; if (rows < 16) rows = 16; return rows * W; }
    return cap;
}

// rays per render_rays chunk up to which the stages run sample-parallel (sn_render_tuning: 0 = the default, < 0 = never)
static uint32_t prop_sp_max_rays(const sn_render_cfg *cfg) {
    const int32_t v = cfg->tuning.prop_sp_max_rays;
    return v == 0 ? 32768u : v < 0 ? 0u : (uint32_t)v;        // tools/prop_sp_ab.py: faster up to 32k rays, slower from 64k
}

// Two samples per lane at once in the proposal stages (bit-neutral): pays where the launch leaves the SIMDs short of waves.
// Measured (profiles/r06/prop_pair_ab.json, [128,64,32], proposal stages only): a wave alone on its SIMD issues one vector instruction per
// ~7 cycles whatever its instruction-level parallelism, so the gain is what the interleaved gathers hide -- 64-256 workgroups -11 %,
// 361 -7 %, 484 -4 %, 625 +-1 %, 1406 and more +5 ... +17 % (3 waves per SIMD instead of 5).
static bool prop_pair_auto(uint32_t workgroups_in_flight) { return workgroups_in_flight <= 512u; }

static uint32_t final_sp_max_rays(const sn_render_cfg *cfg) {
    const int32_t v = cfg->tuning.final_sp_max_rays;
    return v == 0 ? 16384u : v < 0 ? 0u : (uint32_t)v;
}

// the linear-tail form of the default final stage (third layer's geometry rows applied once per ray) is used wherever no
// per-sample tensor leaves the kernel; tuning.per_sample_form keeps the per-sample form (bit-identical to the compacting /
// several-lanes-per-ray / role-split kernels, which all evaluate the third layer per sample)
static bool lt_enabled(const sn_render_cfg *cfg) { return cfg->tuning.per_sample_form == 0; }

static uint32_t tile_log2w(const sn_render_cfg *cfg) { return (cfg && cfg->tuning.wave_tile >= 1 && cfg->tuning.wave_tile <= 5) ? (uint32_t)cfg->tuning.wave_tile : 3u; }
// tuning.linear_tile_order -> the switches of RayCommon.  1: workgroup b renders tile b, tiles in row pairs (the order of rounds 1-2);
// 2: each XCD owns a contiguous range of tile ids (xcd_tile_id), tiles in row pairs (rounds 3-7); 3 and 4: the same ranges over super-tiles
// (wave_tile_of) of 128 x 128 pixels (8 x 8 workgroup blocks: the 64 workgroups an XCD holds are one compact square) and of 48 x 48 pixels
// (3 x 3 blocks); 0: the default, SN_DEFAULT_TILE_ORDER.  Every order launches blocks_for() workgroups.  Measured at 800x800 [128] with fp16
// tables (profiles/r08/): 3 sends 6 % fewer L2 requests on to the fabric than 2 and is 2.3 % SLOWER; 4 is 2 % faster than 2.
#define SN_DEFAULT_TILE_ORDER 4
struct TileOrder { int xcd; uint32_t st_w, st_h; };
static TileOrder tile_order_of(int32_t v, uint32_t tlw) {
    if (v == 0) v = SN_DEFAULT_TILE_ORDER;
    // a unit is 2^tlw x 2^(7 - tlw) pixels
    const uint32_t px = v == 3 ? 128u : v == 4 ? 48u : 0u;
    const uint32_t w = px >> tlw, h = px >> (7u - tlw);
    return TileOrder{v >= 2 && v <= 4, px ? (w ? w : 1u) : 0u, px ? (h ? h : 1u) : 0u};      // (any other value: 1)
}
static uint32_t blocks_for(uint32_t n, uint32_t W, uint32_t tlw) {
    if (W) {                                                      // four wave tiles of 2^tlw x 2^(6 - tlw) pixels each (ray_of_lane)
        const uint32_t rows = (n + W - 1) / W, tw = 1u << tlw, th = 64u >> tlw;
        return div_up(((W + tw - 1u) >> tlw) * ((rows + th - 1u) / th), 4u);
    }
    return div_up(n, 256);
}

static size_t stage_scratch_floats(const sn_render_cfg *cfg, uint32_t Npad) {
    size_t f = 0;
    for (uint32_t k = 0; k + 1 < cfg->num_stages; ++k) f += (size_t)cfg->num_steps[k] * Npad;          // weights
    for (uint32_t k = 1; k < cfg->num_stages; ++k) f += (size_t)(cfg->num_steps[k] + 1) * Npad;       // bins
    if (cfg->with_feat) f += (size_t)cfg->num_steps[cfg->num_stages - 1] * Npad;                      // last-stage weights
    return f;
}


// Row bands on two streams (round 4, tuning.band_streams).  A schedule with proposal stages is three kernels of different character --
// the proposal stages are bound by the vector ALU, the last stage by the texture path and the matrix cores -- that a single stream runs one
// after the other, each with its own ramp and tail.  Rendered as TWO row bands on two streams the kernels of one band overlap those of the
// other (measured through captured graphs, tools/band_streams_ab.py: 800x800 [128,64,32] 4.36 -> 4.07 ms fp32, 3.85 -> 3.71 ms fp16; 1600x1600
// 14.76 -> 14.04 / 13.43 -> 12.98; nothing at 400x400, where the stages' latency floors decide).  Same kernels over sub-ranges of the tiles:
// bit-identical images.  The second stream is owned by the library (one per device), forked from and joined to the caller's stream with
// events inside the call, so the call stays asynchronous, ordered on the caller's stream and capturable into a HIP graph.
struct BandPlan { uint32_t chunk, slots; };
static BandPlan band_plan(const sn_render_cfg *cfg, uint32_t N, uint32_t W) {
    BandPlan p;
    p.chunk = chunk_rays(N, W);
    p.slots = 1;
    const int mode = cfg ? cfg->tuning.band_streams : 1;
    if (mode == 1 || W == 0 || !cfg || cfg->num_stages < 2 || N % W != 0) return p;
    // automatic: from 768 workgroups; with the in-render feature stage -- a fourth kernel, bound by the texture path alone -- from 512
    // (400x400 + SAM-feature head, BASELINE configs[2]: 3.00 -> 2.82 ms, 2.58 -> 2.41 with fp16 tables).  Without it (profiles/r06/band_small_ab.json,
    // fp32 / fp16 tables): 361 workgroups -2 / -4 %, 484 -0 / -3 %, 625 (400x400) +0.5 / -2 %, 784 -5 / -8 %, 1024 -6 / -9 %, 1444 -4 / -7 %, 2500 -7 / -4 %:
    // the last stage holds 512 workgroups at a time, and a band's share of a partly filled last round overlaps the other band's proposal stages.
    if (mode == 0 && blocks_for(N, W, tile_log2w(cfg)) < (cfg->with_feat ? 512u : 768u)) return p;
    const uint32_t rows = N / W;
    const uint32_t nbands = mode > 2 ? (uint32_t)mode : 2u;              // band_streams = K > 2: K bands, dealt alternately to the two streams (A/B; measured: see DESIGN section 7)
    const uint32_t half_rows = (((rows + nbands - 1u) / nbands + 15u) / 16u) * 16u;   // whole 16-row tile rows; the first bands take the odd ones
    if (half_rows == 0u || half_rows >= rows) return p;
    const uint64_t c = (uint64_t)half_rows * W;
    if (c < p.chunk) p.chunk = (uint32_t)c;                               // (images beyond the scratch cap keep its chunks and alternate them)
    p.slots = 2;
    return p;
}

// One library-owned side stream per (device, CALLER stream): two host threads that render on different streams of a device get different side
// streams (a shared one would serialise them, and a thread that forks it while capturing a graph would pull the other thread's launches into its
// capture -- advisor, round 4); callers that share a stream are ordered by that stream anyway.
static hipStream_t band_side_stream(hipStream_t caller) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, hipStream_t> streams;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, caller);
    auto it = streams.find(key);
    if (it != streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    streams[key] = s;
    return s;
}

// fork on construction (the side stream waits for everything the caller's stream holds so far), join on destruction -- on every path out
// of sn_rm_render_rays, error returns included (an unjoined fork would invalidate a stream capture)
struct BandFork {
    hipStream_t main_st, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    BandFork(hipStream_t m, bool want) : main_st(m) {
        if (!want) return;
        hipStream_t s = band_side_stream(m);
        if (!s) return;
        if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) { ev_fork = nullptr; return; }
        if (hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(ev_fork); ev_fork = ev_join = nullptr; return; }
        if (hipEventRecord(ev_fork, main_st) != hipSuccess || hipStreamWaitEvent(s, ev_fork, 0) != hipSuccess) {
            (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join); ev_fork = ev_join = nullptr; return;
        }
        side = s;
    }
    ~BandFork() {
        if (!side) return;
        (void)hipEventRecord(ev_join, side);
        (void)hipStreamWaitEvent(main_st, ev_join, 0);
        (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join);      // (released by the runtime once the recorded work has passed)
    }
};
}  // namespace sn

using namespace sn;

extern "C" {

int sn_build_flags(void) {
    int f = 0;
#ifdef SN_EXPERIMENTS
    f |= SN_BUILD_EXPERIMENTS;
#endif
#ifdef SN_POISON_LDS
    f |= SN_BUILD_POISON_LDS;
#endif
    return f;
}

int sn_rm_last_launch_info(sn_launch_info *info) {
    SN_REQUIRE(info, "last_launch_info: NULL output");
    *info = g_launch;
    return SN_OK;
}

void sn_rm_profile_enable(int on) {
    g_prof_on = on != 0;
    {   // arm / disarm the final stage's clock probe (see clock_probe)
        const int flag = g_prof_on ? 1 : 0;
        const unsigned long long zero[4] = {0, 0, 0, 0};
        if (g_prof_on) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_clk_buf), zero, sizeof(zero));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_clk_on), &flag, sizeof(flag));
    }
    if (!g_prof_on) {
        for (auto &sp : g_prof) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
        g_prof.clear();
    }
}

int sn_rm_profile_shader_clock(float *shader_mhz, float *probe_ms) {
    SN_REQUIRE(shader_mhz, "profile_shader_clock: NULL output");
    *shader_mhz = 0.0f;
    if (probe_ms) *probe_ms = 0.0f;
    unsigned long long h[4];
    SN_HIP_OK(hipDeviceSynchronize());
    SN_HIP_OK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_clk_buf), sizeof(h)));
    int dev = 0, wall_khz = 0;
    SN_HIP_OK(hipGetDevice(&dev));
    SN_HIP_OK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, dev));
    if (h[3] <= h[1] || h[2] <= h[0] || wall_khz <= 0) return SN_OK;       // no final-stage launch since enable
    const double wall_s = (double)(h[3] - h[1]) / ((double)wall_khz * 1e3);
    *shader_mhz = (float)((double)(h[2] - h[0]) / wall_s / 1e6);
    if (probe_ms) *probe_ms = (float)(wall_s * 1e3);
    return SN_OK;
}

int sn_rm_profile_read(float *ms_per_class, int32_t *launches_per_class, int n_classes) {
    SN_REQUIRE(ms_per_class && launches_per_class && n_classes >= PK_CLASSES, "profile_read: need %d classes", (int)PK_CLASSES);
    for (int i = 0; i < n_classes; ++i) { ms_per_class[i] = 0.0f; launches_per_class[i] = 0; }
    for (auto &sp : g_prof) {
        SN_HIP_OK(hipEventSynchronize(sp.b));
        float ms = 0.0f;
        SN_HIP_OK(hipEventElapsedTime(&ms, sp.a, sp.b));
        ms_per_class[sp.cls] += ms; launches_per_class[sp.cls] += 1;
        (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b);
    }
    g_prof.clear();
    return SN_OK;
}

/* Diagnostics: occupancy-API answer (workgroups per CU) for the fused kernels at their launch LDS sizes.
 * out[0] = k_prop_stage<float>, out[1] = k_final_stage f16x3 <float>, out[2] = f32-MFMA <float>; lds[i] = dynamic LDS bytes used. */
int sn_rm_debug_occupancy(int32_t *out, int32_t *lds, int n) {
    SN_REQUIRE(out && lds && n >= 3, "debug_occupancy: need 3 slots");
    int v = 0;
    SN_HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_prop_stage<float, 5, 2, 16, 3>, 256, 0));
    out[0] = v; lds[0] = 0;
    size_t l1 = (size_t)(PACK_FLOATS + 4 * 2 * 64 * SLAB_STRIDE) * sizeof(float);
    SN_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_final_stage<float, 16, 2, 64, 64, 16, 32, MLP_F16X3, 5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l1));
    SN_HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_final_stage<float, 16, 2, 64, 64, 16, 32, MLP_F16X3, 5>, 256, l1));
    out[1] = v; lds[1] = (int32_t)l1;
    size_t l2 = (size_t)(PACK_FLOATS + 4 * 32 * 64) * sizeof(float);
    SN_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_final_stage<float, 16, 2, 64, 64, 16, 32, MLP_F32, -1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l2));
    SN_HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_final_stage<float, 16, 2, 64, 64, 16, 32, MLP_F32, -1>, 256, l2));
    out[2] = v; lds[2] = (int32_t)l2;
    return SN_OK;
}

}  // extern "C"

namespace sn {

// Densified levels (round 3).  The first hashed levels of the main grid have few enough vertices (102^3, 148^3) to be re-laid out per
// render call like the dense ones: one 16-byte pair / quad row per VERTEX, fetched through the hash once per vertex by k_pack_pairs
// instead of once per sample-corner by the march.  The final stage then reads them with 4 (fp32) / 2 (fp16) aligned, spatially coherent
// gathers instead of 8 scattered ones -- 12 fewer gather instructions per wave-sample of 98 -- at the price of a 69 MB pack per call
// (~60 us), so only for renders with enough samples to pay for it.  Same values, same arithmetic: bit-identical.
// SN_RENDER_DENSIFY: unset = automatic, 0 = never, 1 / 2 = force that many levels.
constexpr uint64_t DENSIFY_MIN_SAMPLES = 64ull << 20;       // rays x samples of the last stage (the 69 MB pack costs ~55 us more than the plain one and buys 1.6 % of the kernel: break-even near 45 M)
constexpr uint64_t DENSIFY_MAX_VERTICES = 6ull << 20;       // 96 MB of 16-byte rows
// mode = sn_render_tuning.densify: 0 automatic, 1 never, 2 whenever the kernel exists
static int densify_levels(const GridLevels &g, int K, uint64_t samples, bool f16, int mode) {
    if (K != 5 || g.L != 16 || g.C != 2) return K;           // (the K + 2 = 7 instantiation is built for the main grid's shape)
    // automatic for fp16 tables only: 800x800 [128] 6.35 -> 6.22 ms incl. the pack; with fp32 tables the K = 7 instantiation spills 14
    // registers and the call comes out 0.4 % slower (6.957 -> 6.983 ms)
    const bool want = mode == 2 || (mode == 0 && samples >= DENSIFY_MIN_SAMPLES && f16);
    if (!want) return K;                                     // one extra level alone is not instantiated
    uint64_t v = 0;
    for (int l = 0; l < K + 2; ++l) {
        if ((uint64_t)g.res[l] * g.res[l] * 16u >= (1u << 24)) return K;      // dense byte strides go through 24-bit multiplies
        v += (uint64_t)g.res[l] * g.res[l] * g.res[l];
    }
    return v <= DENSIFY_MAX_VERTICES ? K + 2 : K;
}

// floats of a grid's packed pair / quad rows; densify_samples != 0: the main grid, whose levels 5-6 may be densified for this call
// (sized by table dtype and tuning.densify alone, so that the size does not depend on the outputs a call asks for)
static size_t pair_floats_of(const sn_grid_desc *d, uint64_t densify_samples = 0, int densify_mode = 1) {
    GridLevels g;
    if (d->D != 3 || d->C != 2 || build_grid_levels(&g, d->offsets, d->D, d->C, d->L, d->S, d->H, d->gridtype, (int)d->align_corners, d->interp) != SN_OK) return 0;
    if (!levels_fast(g)) return 0;
    uint32_t off[8];
    const int K = dense_prefix(g);
    return (size_t)pair_layout(g, densify_samples ? densify_levels(g, K, densify_samples, d->table_dtype == SN_F16, densify_mode) : K, off) * 4u;
}

// does the grid have the FinalLv shape with K dense levels (given that its pair rows are packed)?
static bool final_lv_fits(const GridLevels &g, int K, uint32_t row_bytes) {
    FinalLv probe;
    PairTab pt;
    pt.base = &probe;
    for (int l = 0; l < 8; ++l) pt.off[l] = 0;
    return build_final_lv(g, K, pt, &probe, row_bytes, probe);
}

// ---- the route of a render call: what sn_rm_render_rays launches, decided on the host before anything is launched ----------------------
// plan_render() is the only place where a kernel instantiation, a launch geometry or a workspace size is chosen; sn_rm_render_rays
// launches what the route says, sn_rm_render_route_info reports it, sn_rm_render_workspace_bytes sizes the workspace with plan_workspace().

constexpr int VIEW_W = 32 * 32 + 32 * 32 + 3 * 32;     // padded view_mlp rows
static_assert(VIEW_W <= PACK_FLOATS, "view weights overlay the packed MLP weights");
constexpr size_t LDS_F16X3 = (size_t)(PACK_FLOATS + 4 * 2 * 64 * SLAB_STRIDE) * sizeof(float);      // 72 KiB: packed weights + two sample slabs per wave
constexpr size_t LDS_F16X3_PT = (size_t)(PACK_FLOATS + 8 * 2 * 64 * SLAB_STRIDE + VIEW_W) * sizeof(float);   // 120.4 KiB: k_final_stage_pt, one workgroup of 8 waves per CU
constexpr size_t LDS_F16X3_L0 = (size_t)(PACK_FLOATS + 4 * 2 * 64 * 16 + L0_MAX_ROWS) * sizeof(float);
constexpr size_t LDS_MFMA32 = (size_t)(PACK_FLOATS + 4 * 32 * 64) * sizeof(float);                  // 64 KiB
constexpr size_t LDS_VALU = (size_t)(2 * 64 * 256 + VIEW_W) * sizeof(float);                        // 136 KiB + the view weights

// tuning.experiment as this build honours it (plan_render refuses a non-zero value on a build without the experiments)
static int experiment_of(const sn_render_cfg *cfg) {
#ifdef SN_EXPERIMENTS
    return cfg->tuning.experiment;
#else
    (void)cfg;
    return SN_EXP_NONE;
#endif
}

constexpr uint32_t SN_TILE_QUEUES = 8;
struct FinalRoute {
    enum Family { NONE, ANY, SP, CMP, RS, LT, LT_L0, PER_SAMPLE, MFMA32, VALU };
    Family family = NONE;                  // NONE: skip_final
    bool f16 = false;                      // table type
    int K = -1;                            // dense levels the instantiation reads as packed rows (-1: level kind at run time)
    bool aux = false, eo = false;          // AUX (last-stage weights out / early stop), EO (exact early-out)
    int np = 3;                            // products per split multiply
    bool clumped = false;                  // LT: the matrix phase in its clumped order (SN_EXP_MATRIX_CLUMPED, experiments builds)
    bool canon = false;                    // FinalLv kernels: hashed levels in the canonical corner order (SN_EXP_GATHER_CANONICAL, experiments builds)
    uint32_t grid = 0, block = 256;
    size_t lds = 0;                        // dynamic LDS bytes of the launch
    const char *name = "";                 // what sn_launch_info reports, with the two figures below
    int dense = 0;
    uint32_t gathers = 0;
    uint32_t lpr_log2 = 0, spl_log2 = 0;   // SP: lanes per ray, samples per lane
    bool pt = false;                       // LT, plain: the persistent launch (k_final_stage_pt); grid stays the count of 256-ray tile units,
    uint32_t pt_grid = 0;                  // the real grid is pt_grid workgroups of 512 threads
};
struct PropRoute {
    int K = -1;                            // dense prefix the instantiation is built for (3, 2, or -1: run time)
    bool f16 = false, sp = false, pair = false;
    uint32_t lanes = 32, grid = 0;         // sp: lanes per ray
};
struct FeatRoute {
    uint32_t C = 0, lg = 2, patch_levels = 0;        // level_dim, levels per workgroup pass, leading levels that run the LDS-patch instantiation
    bool f16 = false;
};
struct ChunkRoute {                        // what depends on the rays of one chunk only through their number
    uint32_t n = 0, nblk = 0, Npad = 0;
    PropRoute prop[SN_MAX_STAGES];
    FinalRoute fin;
};
struct WorkspacePlan {
    BandPlan bands;
    size_t pair_main = 0, pair_prop[SN_MAX_STAGES] = {};   // floats of the packed pair rows: main grid (sized for its densified layout), proposal grids
    size_t pair_floats = 0, slot_floats = 0;         // all pair rows; stage scratch of one band slot
    size_t head_floats() const { return (size_t)PACK_FLOATS + pair_floats; }
    // the tile-queue counters of the persistent last stage: 8 x uint32 per band slot, behind everything else (launches of one slot are
    // ordered on its stream, and every launch zeroes its counters on that stream first)
    size_t ctr_words() const { return (size_t)bands.slots * SN_TILE_QUEUES; }
    size_t ctr_offset_floats() const { return (size_t)bands.slots * slot_floats + head_floats(); }
    size_t bytes() const { return (ctr_offset_floats() + ctr_words()) * sizeof(float); }
};
struct RenderRoute {
    GridLevels gl_prop[SN_MAX_STAGES], gl_main, gl_feat;
    bool is_main = false, is_any = false;
    AnyShape any;
    int mlp_mode = MLP_F16X3, mlp_np = 3;
    bool use_cmp = false;
    int Kmain = -1;                        // dense prefix of the main grid if it has the FinalLv shape, else -1
    int Kv_main = 0;                       // levels of the main grid packed as pair rows for this call (7: levels 5-6 densified)
    float stop_cum = 0.0f;
    WorkspacePlan ws;
    FinalRoute fin;                        // the last stage but for what depends on a chunk's ray count (plan_chunk completes it)
    FeatRoute feat;
    uint32_t chunks = 0;
    uint32_t cus = 0;                      // compute units of the device the call runs on (0: not known -- the automatic rule of the persistent launch stays off)
    ChunkRoute full, last;                 // every chunk but the last one; the last one (the only one of a call that fits one chunk)
};

static WorkspacePlan plan_workspace(const sn_render_cfg *cfg, uint32_t N, uint32_t W) {
    WorkspacePlan w;
    w.bands = band_plan(cfg, N, W);
    const uint32_t nc = w.bands.chunk < N ? w.bands.chunk : N;
    w.slot_floats = stage_scratch_floats(cfg, blocks_for(nc, W, tile_log2w(cfg)) * 256u);
    w.pair_floats = w.pair_main = pair_floats_of(&cfg->grid, (uint64_t)N * cfg->num_steps[cfg->num_stages - 1], cfg->tuning.densify);
    for (uint32_t k = 0; k + 1 < cfg->num_stages; ++k) w.pair_floats += w.pair_prop[k] = pair_floats_of(&cfg->prop_grid[k]);
    return w;
}

// the io pointers every call needs (sn_rm_render_rays and sn_rm_render_route_info check them before plan_render)
static int check_io_pointers(const sn_render_cfg *cfg, const sn_render_io *io) {
    SN_REQUIRE(io->rays_o && io->rays_d, "render_rays: rays must be device pointers");
    if (io->skip_final) SN_REQUIRE(cfg->num_stages >= 2 && (cfg->num_stages > SN_MAX_STAGES /* refused below, by the num_stages check */ || io->bins[cfg->num_stages - 1]) && !cfg->with_feat,
                                   "render_rays: skip_final needs >= 2 stages, io->bins[last] for the resampled bins, and no feature stage");
    else SN_REQUIRE(io->image && io->depth && io->weights_sum, "render_rays: outputs must be device pointers");
    return SN_OK;
}

// The last stage of the call, but for what depends on a chunk's ray count (plan_chunk).  The chain below is the ONE statement of which
// kernel family runs when.
static void plan_final(const sn_render_cfg *cfg, const sn_render_io *io, RenderRoute *r) {
    const uint32_t S = cfg->num_stages;
    const bool f16 = cfg->grid.table_dtype == SN_F16;
    const int dp = dense_prefix(r->gl_main);
    const uint64_t main_samples = (uint64_t)io->N * cfg->num_steps[S - 1];
    r->Kv_main = r->is_any ? 0 : dp;
    // pair rows of the main grid exist whenever it has a packable dense prefix; the kernels that read FinalLv need them
    const bool have_pairs = !r->is_any && dp > 0 && r->ws.pair_main != 0;
    r->Kmain = have_pairs && final_lv_fits(r->gl_main, dp, 2u * (f16 ? 2u : 4u)) ? dp : -1;      // the K = 5 instantiations read FinalLv
    // opt-in compaction: k_final_stage_cmp replaces the last stage when nothing per-sample leaves the call (those tensors
    // must be complete) and the table has the FinalLv shape; the proposal stages then drop waves of missed rays as well
    if (cfg->compact_live && r->mlp_mode == MLP_F16X3 && !cfg->with_feat && !io->xyzs_last && !io->geo_feat_last && !io->skip_final &&
        io->bins0_ray_stride == 0) {
        bool any_dbg = false;
        for (uint32_t k = 1; k < S; ++k) any_dbg = any_dbg || io->u_ray_stride[k] != 0;      // per-ray jitter tables: the default kernels
        for (uint32_t k = 0; k < S; ++k) any_dbg = any_dbg || io->bins[k] || io->weights[k] || io->sigmas[k] || io->inds[k];
        r->use_cmp = !any_dbg && dp == 5 && r->Kmain == 5;
    }
    if (io->skip_final) return;            // proposal stages only
    // early termination is honoured only when nothing per-sample leaves the kernel (those tensors would be left unwritten past the stop)
    const bool dbg_last = io->bins[S - 1] || io->weights[S - 1] || io->sigmas[S - 1] || io->xyzs_last || io->geo_feat_last;
    const bool per_sample_out = dbg_last || cfg->with_feat;
    r->stop_cum = (cfg->early_stop_eps > 0.0f && cfg->early_stop_eps < 1.0f && !per_sample_out) ? -logf(cfg->early_stop_eps) : 0.0f;
    // gather instructions of one wave-sample = dense levels as packed rows (fp32 tables: pair rows, 4 loads; fp16: quad rows, 2 loads)
    // + 8 corners per hashed level
    auto lv_gathers = [&](int kd) -> uint32_t { return (uint32_t)kd * (f16 ? 2u : 4u) + (uint32_t)(16 - kd) * 8u; };
    FinalRoute &f = r->fin;
    f.f16 = f16;
    f.aux = cfg->with_feat || r->stop_cum > 0.0f;
    // exact early-out of the LAST stage (linear-tail instantiations): opt-in (tuning.exact_early_out = 2).  Measured on the opaque field
    // (profiles/r04/bench_configs.json): behind proposal stages the last stage's 32 samples sit around the surface and the test buys nothing
    // (1.953 vs 1.952 ms -- the proposal stages' own early-out, always on, is what takes that render from 3.19 to 1.95 ms) while it costs a
    // semi-transparent scene 0.2-0.3 %; a single-stage schedule gains (6.07 -> 4.43 ms) but its kernel is the bench line's (0.5-1 % cost).
    f.eo = cfg->tuning.exact_early_out == 2;
    const int xp = experiment_of(cfg);
    const bool f16x3 = r->mlp_mode == MLP_F16X3;
    // SN_EXP_GATHER_CANONICAL (round 10): the A/B partner of the parity order of the hashed-level gathers, same bits; the linear-tail (full
    // product form), per-sample K = 5 and compaction kernels carry it
    f.canon = xp == SN_EXP_GATHER_CANONICAL;
    if (r->is_any) {      // sizes at run time.  (io->head_stride is accepted here although this kernel never writes the rgb | depth columns:
                          //  ADVICE.md; plan_render's head_stride check is the place to refuse it)
        f.family = FinalRoute::ANY; f.name = "k_final_stage_any";
        f.lds = (size_t)(2u * r->any.rows + (r->any.dg[r->any.ng] - 1u)) * 256u * sizeof(float);
        f.dense = 0; f.gathers = cfg->grid.L * 8u;
    } else if (r->use_cmp) {
        // per-ray termination + live-sample compaction (k_final_stage_cmp); f_image stays available
        f.family = FinalRoute::CMP; f.name = "k_final_stage_cmp"; f.K = 5; f.lds = LDS_F16X3; f.dense = 5; f.gathers = lv_gathers(5);
    } else if (f16x3 && r->Kmain == 5 && !f.aux && !per_sample_out && xp == SN_EXP_ROLE_SPLIT) {
        // role-split waves (k_final_stage_rs, experiments builds): 768-thread workgroups over 32x16-pixel tiles (512 rays in linear order)
        f.family = FinalRoute::RS; f.name = "k_final_stage_rs"; f.K = 5; f.dense = 5; f.gathers = lv_gathers(5);
    } else if (f16x3 && r->Kmain == 5 && !dbg_last && lt_enabled(cfg)) {
        // linear tail: layer 3 off the matrix cores (per-sample geometry features are not available in this form)
        // SN_EXP_LDS_LEVEL0 (opt-in, experiments builds): fp16 tables whose level 0 fits 16 KiB keep that level LDS-resident.  Bit-identical
        // and measured SLOWER than the texture path (800x800 [128]: 6.44 -> 6.58 ms, profiles/r03/ab_round3_experiments.txt): with fp16
        // tables the kernel is not bound by the texture addressers, and the 8 ds_read_b32 + swizzled slab addressing cost more than 2 gathers save
        const bool l0 = f16 && (uint64_t)r->gl_main.res[0] * r->gl_main.res[0] * r->gl_main.res[0] <= (uint64_t)L0_MAX_ROWS && xp == SN_EXP_LDS_LEVEL0;
        // levels 5 and 6 densified for this call (densify_levels): only the plain instantiation reads them, and compact_live keeps K = 5
        if (!f.aux && !cfg->compact_live) r->Kv_main = densify_levels(r->gl_main, 5, main_samples, f16, cfg->tuning.densify);
        const bool dens = r->Kv_main == 7 && !l0 && final_lv_fits(r->gl_main, 7, 2u * (f16 ? 2u : 4u));
        f.family = l0 ? FinalRoute::LT_L0 : FinalRoute::LT;
        f.K = dens ? 7 : 5;
        f.name = l0 ? "k_final_stage<lt,K=5,lds-level0>" : dens ? "k_final_stage<lt,K=7>" : f.aux ? "k_final_stage<lt,K=5,aux>" : "k_final_stage<lt,K=5>";
        f.dense = f.K; f.gathers = lv_gathers(f.K) - (l0 ? 2u : 0u);
        // SN_MLP_F16X1: the reduced form of the plain launch with fp16 tables
        if (f16 && !f.eo && r->mlp_np == 1 && !f.aux && !l0) f.np = 1;
        // SN_EXP_MATRIX_CLUMPED (round 9): the A/B partner of the spread matrix phase, same bits (the reduced-product form has no spread order)
        f.clumped = xp == SN_EXP_MATRIX_CLUMPED && f.np == 3 && !l0;
        // SN_EXP_FINAL_ONE_WG (round 6): the last stage asks for 84 KiB of LDS, so only ONE of its workgroups fits a CU and half of every SIMD's
        // registers stay free for the proposal-stage workgroups of the OTHER row band (tuning.band_streams): vector-ALU-bound waves beside
        // texture-bound ones on the same SIMD instead of on different CUs
        f.lds = l0 ? LDS_F16X3_L0 : (xp == SN_EXP_FINAL_ONE_WG && !dens && f.np == 3) ? (size_t)(84 * 1024) : LDS_F16X3;
    } else if (f16x3) {
        f.family = FinalRoute::PER_SAMPLE; f.K = r->Kmain == 5 ? 5 : -1; f.lds = LDS_F16X3;           // main grid: levels 0-4 dense
        f.name = r->Kmain == 5 ? "k_final_stage<per-sample,K=5>" : "k_final_stage<per-sample,generic>";
        f.dense = r->Kmain; f.gathers = r->Kmain == 5 ? lv_gathers(5) : (uint32_t)dp * 4u + (16u - (uint32_t)dp) * 8u;
    } else if (r->mlp_mode == MLP_F32) {
        f.family = FinalRoute::MFMA32; f.name = "k_final_stage<mfma32>"; f.aux = true; f.lds = LDS_MFMA32; f.dense = -1; f.gathers = 16u * 8u;
    } else {
        f.family = FinalRoute::VALU; f.name = "k_final_stage<valu>"; f.aux = true; f.lds = LDS_VALU; f.dense = -1; f.gathers = 16u * 8u;
    }
}

// the launches of one chunk of n rays
static ChunkRoute plan_chunk(const sn_render_cfg *cfg, const sn_render_io *io, const RenderRoute &r, uint32_t n) {
    const uint32_t S = cfg->num_stages, W = io->tile_w;
    ChunkRoute c;
    c.n = n; c.nblk = blocks_for(n, W, tile_log2w(cfg)); c.Npad = c.nblk * 256u;
    for (uint32_t k = 0; k + 1 < S; ++k) {
        PropRoute &p = c.prop[k];
        const int K = dense_prefix(r.gl_prop[k]);
        p.K = (K == 3 || K == 2) ? K : -1;       // prop0: res 16, 27, 46 dense (network.py:135); prop1: res 16, 32 dense (network.py:140)
        p.f16 = cfg->prop_grid[k].table_dtype != SN_F32;
        // few rays in linear order (training batches): several lanes per ray instead of one (k_prop_stage_sp)
        p.sp = W == 0 && n <= prop_sp_max_rays(cfg) && cfg->num_steps[k] <= SP_MAX_T;
        // lanes per ray of the small-batch kernel (tuning.prop_sp_lanes forces 8 / 16 / 32)
        p.lanes = 32u;      // (measured, profiles/r06/prop_sp_lanes_ab.json: 32 lanes are the fastest from 1024 to 32768 rays)
        if (cfg->tuning.prop_sp_lanes == 8 || cfg->tuning.prop_sp_lanes == 16 || cfg->tuning.prop_sp_lanes == 32) p.lanes = (uint32_t)cfg->tuning.prop_sp_lanes;
        // two samples of a ray at once (k_prop_stage<..., UN = 2>): tuning.prop_pair 2 = always, 1 = never, 0 = automatic
        p.pair = cfg->tuning.prop_pair == 2 ||
                 (cfg->tuning.prop_pair == 0 && prop_pair_auto(r.ws.bands.slots == 2u ? blocks_for(io->N, W, tile_log2w(cfg)) : c.nblk));   // (two bands run side by side)
        p.grid = p.sp ? c.Npad / (256u / p.lanes) : c.nblk;   // sp: every scratch column, like the one-lane-per-ray launch
    }
    c.fin = r.fin;
    FinalRoute &f = c.fin;
    f.grid = c.nblk;
    const uint32_t T = cfg->num_steps[S - 1];
    // The persistent launch (k_final_stage_pt; tuning.persistent_tiles 2 = always, 1 = never, 0 = automatic): the plain linear-tail instantiation
    // with the full product form, the parity gather order and no exact early-out.  Automatic: only when the launch has
    // more wave tiles than the device has resident wave slots (8 per CU) -- below that every wave tile gets a wave at once and there is
    // nothing to balance -- and only when the CU count is known.
    if (f.family == FinalRoute::LT && !f.aux && !f.eo && f.np == 3 && !f.clumped && !f.canon && cfg->tuning.persistent_tiles != 1) {
        const uint32_t cus = r.cus ? r.cus : 256u;           // (forced without a known device: the part this library is built for)
        const uint32_t wgs = cfg->tuning.persistent_wgs > 0 ? (uint32_t)cfg->tuning.persistent_wgs : cus;
        // Two row bands on two streams (tuning.band_streams): two persistent launches serialise -- each wants every CU -- where two ordinary ones
        // overlap their tails.  Measured (profiles/r11/): 800x800 [128,64,32], 5000 wave tiles per band, +0.6 % per frame; 1600x1600, 20 000 per
        // band, -2.0 %.  Such a call takes the form from four times the slot count.
        const uint64_t slots = (uint64_t)SN_TILE_QUEUES * r.cus * (r.ws.bands.slots == 2u ? 4u : 1u);
        if (cfg->tuning.persistent_tiles == 2 || (r.cus != 0u && (uint64_t)c.nblk * 4u > slots)) {
            f.pt = true; f.pt_grid = wgs; f.lds = LDS_F16X3_PT;
        }
    }
#ifdef SN_EXPERIMENTS
    if (f.family == FinalRoute::RS) {
        f.grid = W ? ((W + 31u) >> 5) * ((n / W + 15u) >> 4) : div_up(n, (uint32_t)(RS_PROD * 64));
        f.block = RS_THREADS; f.lds = (size_t)RS_LDS_FLOATS * sizeof(float);
    }
#endif
    // few rays in linear order: lanes share rays (k_final_stage_sp); fewer samples per lane while CUs would idle
    if (f.family != FinalRoute::NONE && f.family != FinalRoute::ANY && W == 0 && r.mlp_mode == MLP_F16X3 && r.stop_cum == 0.0f && !r.use_cmp &&
        n <= final_sp_max_rays(cfg) && T <= 64u * FSP_MAX_SPL) {
        auto lpr_log2_of = [&](uint32_t sl) { const uint32_t need = div_up(T, 1u << sl); uint32_t l2 = 0; while ((1u << l2) < need) ++l2; return l2; };
        uint32_t spl_log2 = 2;
        while (spl_log2 > 0 && div_up(T, 1u << (spl_log2 - 1)) <= 64u && (((size_t)c.Npad << lpr_log2_of(spl_log2)) >> 8) < SN_FINAL_SP_MIN_BLOCKS) --spl_log2;
        FinalRoute sp;
        sp.family = FinalRoute::SP; sp.name = "k_final_stage_sp"; sp.f16 = f.f16; sp.K = r.Kmain == 5 ? 5 : -1;
        sp.spl_log2 = spl_log2; sp.lpr_log2 = lpr_log2_of(spl_log2);
        sp.grid = (uint32_t)(((size_t)c.Npad << sp.lpr_log2) >> 8);
        sp.lds = final_sp_lds_floats(1u << spl_log2) * sizeof(float);
        sp.dense = r.Kmain; sp.gathers = r.Kmain == 5 ? (uint32_t)5 * (f.f16 ? 2u : 4u) + 11u * 8u : 16u * 8u;
        f = sp;
    }
    return c;
}

static void plan_chunks(const sn_render_cfg *cfg, const sn_render_io *io, RenderRoute *r) {
    const uint32_t chunk = r->ws.bands.chunk;
    r->chunks = div_up(io->N, chunk);
    r->full = plan_chunk(cfg, io, *r, io->N < chunk ? io->N : chunk);
    const uint32_t n_last = io->N - (r->chunks - 1u) * chunk;
    r->last = n_last == r->full.n ? r->full : plan_chunk(cfg, io, *r, n_last);
}

// Validates cfg / io (all but the workspace) and fills *r.  Calls no HIP API, touches no global.  io->N >= 1 and check_io_pointers() passed.
static int plan_render(const sn_render_cfg *cfg, const sn_render_io *io, uint32_t cus, RenderRoute *r) {
    r->cus = cus;
    SN_REQUIRE(cfg->tuning.persistent_tiles >= 0 && cfg->tuning.persistent_tiles <= 2, "render_rays: tuning.persistent_tiles %d outside 0..2", cfg->tuning.persistent_tiles);
    SN_REQUIRE(cfg->tuning.persistent_wgs >= 0 && cfg->tuning.persistent_wgs <= 65535, "render_rays: tuning.persistent_wgs %d outside 0..65535", cfg->tuning.persistent_wgs);
    SN_REQUIRE(io->out_stride == 0u || io->out_stride >= 5u, "render_rays: out_stride %u must be 0 (dense outputs) or at least 5 floats (rgb | depth | weights_sum per row)", io->out_stride);
    SN_REQUIRE(io->head_stride == 0u || (io->f_image && io->head_stride >= 31u + 4u && !io->skip_final),
               "render_rays: head_stride %u needs f_image and room for f_image | rgb | depth (>= 35 floats per row)", io->head_stride);
    SN_REQUIRE(cfg->tuning.wave_tile >= 0 && cfg->tuning.wave_tile <= 5, "render_rays: tuning.wave_tile %d outside 0..5", cfg->tuning.wave_tile);
    SN_REQUIRE(!(experiment_of(cfg) == SN_EXP_ROLE_SPLIT && cfg->tuning.wave_tile != 0 && cfg->tuning.wave_tile != 3), "render_rays: the role-split experiment is built for 8x8 wave tiles (tuning.wave_tile 0 or 3)");
    const uint32_t S = cfg->num_stages;
    SN_REQUIRE(S >= 1 && S <= SN_MAX_STAGES, "render_rays: num_stages=%u outside 1..%d", S, SN_MAX_STAGES);
    for (uint32_t k = 0; k < S; ++k) SN_REQUIRE(cfg->num_steps[k] >= 1, "render_rays: num_steps[%u] must be >= 1", k);
    SN_REQUIRE(cfg->sh_degree == 4, "render_rays: fused path is built for SH degree 4 (network.py:97), got %u", cfg->sh_degree);
    if (io->tile_w) SN_REQUIRE(io->N % io->tile_w == 0, "render_rays: N=%u is not a multiple of tile_w=%u", io->N, io->tile_w);
    // per-ray tables: a row holds T+1 values (sanerf_hip.h); a shorter stride would read past the caller's rows
    SN_REQUIRE(io->bins0_ray_stride == 0 || (io->bins0_table && io->bins0_ray_stride >= cfg->num_steps[0] + 1u),
               "render_rays: bins0_ray_stride=%u needs bins0_table and at least num_steps[0]+1=%u values per ray", io->bins0_ray_stride, cfg->num_steps[0] + 1u);
    for (uint32_t k = 1; k < S; ++k)
        SN_REQUIRE(io->u_ray_stride[k] == 0 || (io->u_table[k] && io->u_ray_stride[k] >= cfg->num_steps[k] + 1u),
                   "render_rays: u_ray_stride[%u]=%u needs u_table[%u] and at least num_steps[%u]+1=%u values per ray", k, io->u_ray_stride[k], k, k, cfg->num_steps[k] + 1u);

    // ---- which field is this? ----
    static const uint32_t d_prop[3] = {10, 16, 1};
    static const uint32_t d_main[4] = {32, 64, 64, 16};
    static const uint32_t d_view[4] = {31, 32, 32, 3};
    for (uint32_t k = 0; k + 1 < S; ++k) {
        int rc = to_levels(&r->gl_prop[k], &cfg->prop_grid[k]);
        if (rc) return rc;
        if (!(cfg->prop_grid[k].L == 5 && cfg->prop_grid[k].C == 2 && mlp_is(&cfg->prop_mlp[k], 2, d_prop) && levels_fast(r->gl_prop[k]))) {
            set_error("render_rays: proposal stage %u is not the L=5,F=2 grid + 10-16-1 bias-free ReLU MLP this build fuses (network.py:135-143)", k);
            return SN_ERR_UNSUPPORTED;
        }
    }
    {
        int rc = to_levels(&r->gl_main, &cfg->grid);
        if (rc) return rc;
    }
    r->is_main = cfg->grid.L == 16 && cfg->grid.C == 2 && mlp_is(&cfg->grid_mlp, 3, d_main) && mlp_is(&cfg->view_mlp, 3, d_view) && levels_fast(r->gl_main);
    // any other field of the same structure (sizes at run time: k_final_stage_any; BASELINE configs[0] is one)
    memset(&r->any, 0, sizeof(r->any));
    if (!r->is_main) {
        const sn_mlp_desc *gm = &cfg->grid_mlp, *vm = &cfg->view_mlp;
        auto plain = [](const sn_mlp_desc *m) {
            if (m->num_layers < 1u || m->num_layers > ANY_LAYERS || m->activation != 0u || m->skip_mask != 0u) return false;
            for (uint32_t l = 0; l < m->num_layers; ++l) if (m->bias[l] != nullptr || m->weight[l] == nullptr) return false;
            for (uint32_t l = 0; l <= m->num_layers; ++l) if (m->dims[l] < 1u || m->dims[l] > ANY_W) return false;
            return true;
        };
        r->is_any = cfg->grid.D == 3 && cfg->grid.C == 2 && cfg->grid.L >= 1 && cfg->grid.L * 2u <= ANY_W && plain(gm) && plain(vm) &&
                    gm->dims[0] == cfg->grid.L * 2u && gm->dims[gm->num_layers] >= 2u && gm->dims[gm->num_layers] - 1u <= ANY_GEO &&
                    cfg->sh_degree == 4u && vm->dims[0] == gm->dims[gm->num_layers] - 1u + 16u && vm->dims[vm->num_layers] == 3u;
        if (r->is_any) {
            AnyShape &a = r->any;
            a.ng = gm->num_layers; a.nv = vm->num_layers;
            for (uint32_t l = 0; l <= gm->num_layers; ++l) a.dg[l] = gm->dims[l];
            for (uint32_t l = 0; l <= vm->num_layers; ++l) a.dv[l] = vm->dims[l];
            for (uint32_t l = 0; l < gm->num_layers; ++l) a.wg[l] = gm->weight[l];
            for (uint32_t l = 0; l < vm->num_layers; ++l) a.wv[l] = vm->weight[l];
            uint32_t wmax = 0;
            for (uint32_t l = 0; l <= gm->num_layers; ++l) wmax = gm->dims[l] > wmax ? gm->dims[l] : wmax;
            for (uint32_t l = 0; l <= vm->num_layers; ++l) wmax = vm->dims[l] > wmax ? vm->dims[l] : wmax;
            a.rows = wmax <= 16u ? 16u : wmax <= 32u ? 32u : 64u;
        }
    }
    if (!r->is_main && !r->is_any) {
        set_error("render_rays: the field is neither the L=16,F=2 grid + 32-64-64-16 / 31-32-32-3 MLPs (network.py:93-98) nor of the shape the "
                  "size-agnostic final stage takes (3-D grid with level_dim 2 and <= 32 levels' worth of 64 features, bias-free ReLU MLPs of "
                  "<= 4 layers and <= 64 neurons, <= 31 geometry channels, degree-4 SH)");
        return SN_ERR_UNSUPPORTED;
    }
    if (r->is_any && (cfg->compact_live || cfg->with_feat)) {
        set_error("render_rays: compact_live / the in-render feature stage are instantiated for the reference network's sizes only");
        return SN_ERR_UNSUPPORTED;
    }
    if (cfg->with_feat) {
        SN_REQUIRE(io->f_feat, "render_rays: with_feat is set but io->f_feat is NULL");
        SN_REQUIRE(cfg->feat_grid.embeddings && table_aligned(cfg->feat_grid.embeddings) && table_aligned(io->f_feat),
                   "render_rays: feature grid table / f_feat must be 16-byte aligned device pointers");
        int rc = to_levels(&r->gl_feat, &cfg->feat_grid);
        if (rc) return rc;
        const GridLevels &gf = r->gl_feat;
        if (!levels_fast(gf) || !(gf.C == 2 || gf.C == 4 || gf.C == 8)) {
            set_error("render_rays: feature grid must be a hash grid with level_dim 2/4/8, align_corners=False, linear "
                      "interpolation (network.py:103); use sn_rm_grid_composite for other grids");
            return SN_ERR_UNSUPPORTED;
        }
        int lg = 2;   // levels per workgroup pass of the feature stage (more passes = more workgroups, fewer registers)
        if (cfg->tuning.feat_levels) lg = cfg->tuning.feat_levels;
        if (lg != 1 && lg != 2 && lg != 4) lg = 2;
        while (gf.L % (uint32_t)lg) lg >>= 1;
        FeatRoute &ft = r->feat;
        ft.C = gf.C; ft.lg = (uint32_t)lg; ft.f16 = cfg->feat_grid.table_dtype == SN_F16;
        // dense prefix of the feature grid: its passes run the LDS-patch instantiation (k_feat_stage<..., PATCH = true>), the hashed rest the plain one
        uint32_t n_dense = 0;
        while (n_dense < gf.L && (gf.mode[n_dense] & 1u) == 0u) ++n_dense;
        const uint32_t whole = ((n_dense + ft.lg - 1u) / ft.lg) * ft.lg;
        ft.patch_levels = cfg->tuning.feat_patch != 1 ? 0u : whole > gf.L ? gf.L : whole;
    }
    // tuning.mlp_mode: SN_MLP_AUTO (fp16 hi/lo split on the matrix cores, fp32 accumulate, unless cfg->mlp_exact_fp32), SN_MLP_F16X3 (forced),
    //                  SN_MLP_MFMA32 (exact fp32 v_mfma_f32_32x32x2_f32), SN_MLP_VALU (vector-ALU fallback)
    r->mlp_mode = cfg->mlp_exact_fp32 ? MLP_F32 : MLP_F16X3;
    r->mlp_np = 3;                // products per split multiply (SN_MLP_F16X1: opt-in reduced form of the plain linear-tail launch with fp16 tables)
    switch (cfg->tuning.mlp_mode) {
        case SN_MLP_F16X1: r->mlp_mode = MLP_F16X3; r->mlp_np = 1; break;
        case SN_MLP_AUTO: break;
        case SN_MLP_F16X3: r->mlp_mode = MLP_F16X3; break;
        case SN_MLP_MFMA32: r->mlp_mode = MLP_F32; break;
        case SN_MLP_VALU: r->mlp_mode = MLP_VALU; break;
        default: set_error("render_rays: unknown tuning.mlp_mode=%d", cfg->tuning.mlp_mode); return SN_ERR_INVALID;
    }
    if (cfg->tuning.experiment != SN_EXP_NONE && !(sn_build_flags() & SN_BUILD_EXPERIMENTS)) {
        set_error("render_rays: tuning.experiment=%d needs a library built with -DSN_EXPERIMENTS (make exp)", cfg->tuning.experiment);
        return SN_ERR_UNSUPPORTED;
    }
    r->ws = plan_workspace(cfg, io->N, io->tile_w);
    plan_final(cfg, io, r);
    plan_chunks(cfg, io, r);
    return SN_OK;
}

// sn_launch_info of one last-stage launch (launches accumulates over the chunks of a call)
static void note_final(const FinalRoute &f, sn_launch_info *info) {
    snprintf(info->final_kernel, sizeof(info->final_kernel), "%s", f.name);
    info->workgroups = f.grid; info->lds_bytes = (uint32_t)f.lds; info->dense_levels = (uint32_t)(f.dense < 0 ? 0 : f.dense);
    info->gathers_per_wave_sample = f.gathers; info->launches += 1u;
    info->persistent_tiles = f.pt ? 1u : 0u; info->grid_workgroups = f.pt ? f.pt_grid : f.grid;
}

// ---- launching what a route says ----------------------------------------------------------------------------------------------------
template <typename... P, typename... A>
static int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...args) {
    if (lds) SN_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    return SN_OK;
}

using PropKern = void (*)(PropArgs);
template <typename TT, int K> static PropKern prop_kernel_of(const PropRoute &p) {
    if (p.sp) {
        if (p.lanes == 8u) return k_prop_stage_sp<TT, 5, 2, 16, K, 8>;
        if (p.lanes == 16u) return k_prop_stage_sp<TT, 5, 2, 16, K, 16>;
        return k_prop_stage_sp<TT, 5, 2, 16, K, 32>;
    }
    if (p.pair) return k_prop_stage<TT, 5, 2, 16, K, 2>;
    return k_prop_stage<TT, 5, 2, 16, K>;
}
static PropKern prop_kernel(const PropRoute &p) {
    switch (p.K) {
        case 3: return p.f16 ? prop_kernel_of<__half, 3>(p) : prop_kernel_of<float, 3>(p);
        case 2: return p.f16 ? prop_kernel_of<__half, 2>(p) : prop_kernel_of<float, 2>(p);
        default: return p.f16 ? prop_kernel_of<__half, -1>(p) : prop_kernel_of<float, -1>(p);
    }
}

using FinalKern = void (*)(FinalArgs);
// k_final_stage at the reference network's sizes; its boolean template parameters as one flag word (the names are k_final_stage's)
enum : unsigned { FS_AUX = 1u, FS_LT = 2u, FS_L0L = 4u, FS_EO = 8u, FS_PORD = 16u, FS_CANON = 32u };
template <typename TT, int MODE, int K, unsigned F = 0u, int NP = 3>
static FinalKern fs() {
    return k_final_stage<TT, 16, 2, 64, 64, 16, 32, MODE, K, (F & FS_AUX) != 0u, (F & FS_LT) != 0u, (F & FS_L0L) != 0u, (F & FS_EO) != 0u, NP, (F & FS_PORD) != 0u, (F & FS_CANON) != 0u>;
}
template <typename TT> static FinalKern final_kernel_of(const FinalRoute &f) {
    constexpr bool half = std::is_same<TT, __half>::value;
    switch (f.family) {
#ifdef SN_EXPERIMENTS
        case FinalRoute::CMP: return f.canon ? k_final_stage_cmp<TT, 5, true> : k_final_stage_cmp<TT, 5>;
#else
        case FinalRoute::CMP: return k_final_stage_cmp<TT, 5>;
#endif
#ifdef SN_EXPERIMENTS
        case FinalRoute::RS: return k_final_stage_rs<TT, 5>;
        case FinalRoute::LT_L0:
            if constexpr (half) return f.aux ? fs<__half, MLP_F16X3, 5, FS_AUX | FS_LT | FS_L0L>() : fs<__half, MLP_F16X3, 5, FS_LT | FS_L0L>();
            return nullptr;
#endif
        case FinalRoute::LT:
            if constexpr (half) {
                if (f.np == 1) return f.K == 7 ? fs<__half, MLP_F16X3, 7, FS_LT, 1>() : fs<__half, MLP_F16X3, 5, FS_LT, 1>();
            }
#ifdef SN_EXPERIMENTS
            if (f.clumped) {
                if (f.K == 7) return f.eo ? fs<TT, MLP_F16X3, 7, FS_LT | FS_EO | FS_PORD>() : fs<TT, MLP_F16X3, 7, FS_LT | FS_PORD>();
                if (f.aux) return f.eo ? fs<TT, MLP_F16X3, 5, FS_AUX | FS_LT | FS_EO | FS_PORD>() : fs<TT, MLP_F16X3, 5, FS_AUX | FS_LT | FS_PORD>();
                return f.eo ? fs<TT, MLP_F16X3, 5, FS_LT | FS_EO | FS_PORD>() : fs<TT, MLP_F16X3, 5, FS_LT | FS_PORD>();
            }
            if (f.canon && f.np == 3) {
                if (f.K == 7) return f.eo ? fs<TT, MLP_F16X3, 7, FS_LT | FS_EO | FS_CANON>() : fs<TT, MLP_F16X3, 7, FS_LT | FS_CANON>();
                if (f.aux) return f.eo ? fs<TT, MLP_F16X3, 5, FS_AUX | FS_LT | FS_EO | FS_CANON>() : fs<TT, MLP_F16X3, 5, FS_AUX | FS_LT | FS_CANON>();
                return f.eo ? fs<TT, MLP_F16X3, 5, FS_LT | FS_EO | FS_CANON>() : fs<TT, MLP_F16X3, 5, FS_LT | FS_CANON>();
            }
#endif
            if (f.K == 7) return f.eo ? fs<TT, MLP_F16X3, 7, FS_LT | FS_EO>() : fs<TT, MLP_F16X3, 7, FS_LT>();
            if (f.aux) return f.eo ? fs<TT, MLP_F16X3, 5, FS_AUX | FS_LT | FS_EO>() : fs<TT, MLP_F16X3, 5, FS_AUX | FS_LT>();
            return f.eo ? fs<TT, MLP_F16X3, 5, FS_LT | FS_EO>() : fs<TT, MLP_F16X3, 5, FS_LT>();
        case FinalRoute::PER_SAMPLE:      // the plain instantiation unless the extras are on
#ifdef SN_EXPERIMENTS
            if (f.canon && f.K == 5) return f.aux ? fs<TT, MLP_F16X3, 5, FS_AUX | FS_CANON>() : fs<TT, MLP_F16X3, 5, FS_CANON>();
#endif
            if (f.K == 5) return f.aux ? fs<TT, MLP_F16X3, 5, FS_AUX>() : fs<TT, MLP_F16X3, 5>();
            return f.aux ? fs<TT, MLP_F16X3, -1, FS_AUX>() : fs<TT, MLP_F16X3, -1>();
        case FinalRoute::MFMA32: return fs<TT, MLP_F32, -1, FS_AUX>();
        case FinalRoute::VALU: return fs<TT, MLP_VALU, -1, FS_AUX>();
        default: return nullptr;          // (ANY and SP take further arguments: launch_final names them)
    }
}

static int launch_final(const FinalRoute &f, hipStream_t st, const FinalArgs &fa, const AnyShape &any, uint32_t *queue_ctr) {
    const dim3 grid(f.grid), block(f.block);
    if (f.pt) {
        // the queues' counters start from zero on every launch, whatever the previous one left: ordered on the launch's stream, capturable
        SN_REQUIRE(queue_ctr != nullptr, "render_rays: the persistent last stage has no counters");
        static_assert(SN_TILE_QUEUES == 8, "k_tile_queue_reset clears eight counters");
        const int rcz = launch(k_tile_queue_reset, dim3(1), dim3(64), 0, st, queue_ctr);
        if (rcz) return rcz;
        const TileQueueArgs q{queue_ctr, f.grid};
        const dim3 pgrid(f.pt_grid), pblock(512);
        if (f.K == 7) return f.f16 ? launch(k_final_stage_pt<__half, 7>, pgrid, pblock, f.lds, st, fa, q) : launch(k_final_stage_pt<float, 7>, pgrid, pblock, f.lds, st, fa, q);
        return f.f16 ? launch(k_final_stage_pt<__half, 5>, pgrid, pblock, f.lds, st, fa, q) : launch(k_final_stage_pt<float, 5>, pgrid, pblock, f.lds, st, fa, q);
    }
    switch (f.family) {
        case FinalRoute::ANY:
            return f.f16 ? launch(k_final_stage_any<__half>, grid, block, f.lds, st, fa, any) : launch(k_final_stage_any<float>, grid, block, f.lds, st, fa, any);
        case FinalRoute::SP:
            if (f.K == 5) return f.f16 ? launch(k_final_stage_sp<__half, 5>, grid, block, f.lds, st, fa, f.lpr_log2, f.spl_log2) : launch(k_final_stage_sp<float, 5>, grid, block, f.lds, st, fa, f.lpr_log2, f.spl_log2);
            return f.f16 ? launch(k_final_stage_sp<__half, -1>, grid, block, f.lds, st, fa, f.lpr_log2, f.spl_log2) : launch(k_final_stage_sp<float, -1>, grid, block, f.lds, st, fa, f.lpr_log2, f.spl_log2);
        default: {
            const FinalKern kern = f.f16 ? final_kernel_of<__half>(f) : final_kernel_of<float>(f);
            if (!kern) { set_error("render_rays: no kernel for the last-stage route %s", f.name); return SN_ERR_UNSUPPORTED; }
            return launch(kern, grid, block, f.lds, st, fa);
        }
    }
}

using FeatKern = void (*)(FeatArgs);
template <typename TT, int C> static FeatKern feat_kernel_of(uint32_t lg, bool patch) {
    if (patch) {
        if (lg == 4u) return k_feat_stage<TT, C, 4, true>;
        if (lg == 2u) return k_feat_stage<TT, C, 2, true>;
        return k_feat_stage<TT, C, 1, true>;
    }
    if (lg == 4u) return k_feat_stage<TT, C, 4>;
    if (lg == 2u) return k_feat_stage<TT, C, 2>;
    return k_feat_stage<TT, C, 1>;
}
static FeatKern feat_kernel(const FeatRoute &ft, bool patch) {
    switch (ft.C) {
        case 8: return ft.f16 ? feat_kernel_of<__half, 8>(ft.lg, patch) : feat_kernel_of<float, 8>(ft.lg, patch);
        case 4: return ft.f16 ? feat_kernel_of<__half, 4>(ft.lg, patch) : feat_kernel_of<float, 4>(ft.lg, patch);
        default: return ft.f16 ? feat_kernel_of<__half, 2>(ft.lg, patch) : feat_kernel_of<float, 2>(ft.lg, patch);
    }
}
// compute units of the current device, asked once per device and thread-safe; 0 where there is no device (the planner then leaves the
// automatic rule of the persistent launch off, and everything that needs a device fails where it always did)
static uint32_t device_compute_units() {
    static std::mutex mu;
    static std::map<int, uint32_t> known;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0u; }
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(dev);
    if (it != known.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 0) { (void)hipGetLastError(); n = 0; }
    known[dev] = (uint32_t)n;
    return (uint32_t)n;
}
}  // namespace sn

extern "C" {

size_t sn_rm_render_workspace_bytes(const sn_render_cfg *cfg, uint32_t N, uint32_t tile_w) {
    if (!cfg || N == 0 || cfg->num_stages < 1 || cfg->num_stages > SN_MAX_STAGES) return (size_t)PACK_FLOATS * sizeof(float);   // (sn_rm_render_rays refuses such a schedule)
    return plan_workspace(cfg, N, tile_w).bytes();
}

int sn_rm_render_route_info_cus(const sn_render_cfg *cfg, const sn_render_io *io, uint32_t compute_units, sn_launch_info *out) {
    SN_REQUIRE(cfg && io && out, "render_route_info: cfg/io/out is NULL");
    *out = sn_launch_info{};
    if (io->N == 0) return SN_OK;
    int rc = check_io_pointers(cfg, io);
    if (rc) return rc;
    RenderRoute route;
    rc = plan_render(cfg, io, compute_units, &route);
    if (rc) return rc;
    if (io->skip_final) return SN_OK;
    note_final(route.last.fin, out);
    out->launches = route.chunks;
    return SN_OK;
}
int sn_rm_render_route_info(const sn_render_cfg *cfg, const sn_render_io *io, sn_launch_info *out) { return sn_rm_render_route_info_cus(cfg, io, 0u, out); }

int sn_rm_tile_queue_info(uint32_t units, int32_t order, int32_t wave_tile, uint32_t queue, sn_tile_queue_info *out) {
    SN_REQUIRE(out, "tile_queue_info: out is NULL");
    SN_REQUIRE(queue < SN_TILE_QUEUES, "tile_queue_info: queue %u outside 0..7", queue);
    SN_REQUIRE(units <= 0x3fffffffu, "tile_queue_info: %u workgroup tiles are more than a launch holds", units);
    SN_REQUIRE(wave_tile >= 0 && wave_tile <= 5, "tile_queue_info: wave_tile %d outside 0..5", wave_tile);
    const TileOrder to = tile_order_of(order, wave_tile ? (uint32_t)wave_tile : 3u);
    *out = sn_tile_queue_info{};
    tile_queue_range(queue, units, to.xcd, out->begin, out->end);
    out->queues = SN_TILE_QUEUES; out->wave_tiles = 4u * units;
    return SN_OK;
}

static_assert(sizeof(sn_render_io) == 312 && offsetof(sn_render_io, pack_valid) == 292 && offsetof(sn_render_io, workspace) == 296,
              "sn_render_io.pack_valid sits in the padding after head_stride: the struct's layout is ABI 12's");

int sn_rm_tile_order_info(uint32_t W, uint32_t rows, int32_t wave_tile, int32_t order, uint32_t workgroup, sn_tile_order_info *out) {
    SN_REQUIRE(out, "tile_order_info: out is NULL");
    SN_REQUIRE(W >= 1u && rows >= 1u && (uint64_t)W * rows <= 0xffffffffull, "tile_order_info: W=%u rows=%u is not an image of 1..2^32-1 rays", W, rows);
    SN_REQUIRE(wave_tile >= 0 && wave_tile <= 5, "tile_order_info: wave_tile %d outside 0..5", wave_tile);
    const uint32_t tlw = wave_tile ? (uint32_t)wave_tile : 3u, tlh = 6u - tlw, tw = 1u << tlw, th = 1u << tlh;
    const uint32_t nwg = blocks_for(W * rows, W, tlw);
    SN_REQUIRE(workgroup < nwg, "tile_order_info: workgroup %u outside the launch of %u", workgroup, nwg);
    const TileOrder to = tile_order_of(order, tlw);
    const uint32_t tx8 = (W + tw - 1u) >> tlw, ty8 = (rows + th - 1u) >> tlh;
    *out = sn_tile_order_info{};
    out->workgroups = nwg;
    out->tile_id = to.xcd ? xcd_tile_id(workgroup, nwg) : workgroup;
    out->tile_w = tw; out->tile_h = th;
    for (uint32_t wave = 0; wave < 4u; ++wave) {       // ray_of_lane, lane 0
        uint32_t wx, wy;
        wave_tile_of(out->tile_id * 4u + wave, tx8, ty8, to.st_w, to.st_h, wx, wy);
        const bool ok = wx < tx8 && (wy << tlh) < rows;
        out->x[wave] = ok ? (int32_t)(wx << tlw) : -1;
        out->y[wave] = ok ? (int32_t)(wy << tlh) : -1;
    }
    return SN_OK;
}

int sn_rm_render_rays(const sn_render_cfg *cfg, const sn_render_io *io, sn_stream_t stream) {
    SN_REQUIRE(cfg && io, "render_rays: cfg/io is NULL");
    if (io->N == 0) return SN_OK;   // empty batch: nothing to launch, pointers may be NULL
    g_launch = sn_launch_info{};
    // ---- 1. pointers, 2. the route ----
    int rc = check_io_pointers(cfg, io);
    if (rc) return rc;
    RenderRoute route;
    rc = plan_render(cfg, io, device_compute_units(), &route);
    if (rc) return rc;
    SN_REQUIRE(io->workspace != nullptr, "render_rays: workspace is NULL");
    SN_REQUIRE(table_aligned(io->workspace), "render_rays: workspace must be 16-byte aligned");
    // Checked before anything is written to the workspace, for what sn_rm_render_workspace_bytes states: the packs' region too (a single-stage
    // call has no scratch behind it), and both band slots even if the side stream should turn out not to be available below.
    if (io->workspace_bytes / sizeof(float) < route.ws.bytes() / sizeof(float)) {
        set_error("render_rays: workspace too small (%zu bytes, need %zu)", io->workspace_bytes, route.ws.bytes());
        return SN_ERR_WORKSPACE;
    }
    const uint32_t S = cfg->num_stages, W = io->tile_w;
    const hipStream_t st_main = (hipStream_t)stream;
    const GridLevels &gl_main = route.gl_main;
    float *pack = reinterpret_cast<float *>(io->workspace);
    float *pair_mem = pack + PACK_FLOATS;
    float *scratch = pair_mem + route.ws.pair_floats;

    // ---- 3. weights and pair rows, packed on the caller's stream ----
    // io->pack_valid == SN_PACK_VALID: the caller vouches that this workspace still holds what the previous call with the same cfg packed
    // (same tables, weights, dtypes, tuning and route): the regions are laid out as always and read as they are, nothing is launched here
    const bool packed_before = io->pack_valid == SN_PACK_VALID;
    if (route.mlp_mode != MLP_VALU && !route.is_any && !packed_before) {
        ProfScope ps(st_main, PK_PACK);
        if (route.mlp_mode == MLP_F16X3)
            rc = launch(k_pack_grid_mlp_f16, dim3(PACK16_VECS * 64 / 256), dim3(256), 0, st_main, cfg->grid_mlp.weight[0], cfg->grid_mlp.weight[1],
                        cfg->grid_mlp.weight[2], reinterpret_cast<uint4 *>(pack));
        else
            rc = launch(k_pack_grid_mlp, dim3(PACK_FLOATS / 256), dim3(256), 0, st_main, cfg->grid_mlp.weight[0], cfg->grid_mlp.weight[1], cfg->grid_mlp.weight[2], pack);
        if (rc) return rc;
        SN_LAUNCH_CHECK("k_pack_grid_mlp");
    }
    // aligned x-pair rows of every grid's dense levels (PairTab), re-packed on every call unless the caller vouches for them: the library stays stateless
    PairTab pairs, prop_pairs[SN_MAX_STAGES];
    {
        float *cursor = pair_mem;
        auto pack_pairs = [&](const sn_grid_desc *d, const GridLevels &gl, PairTab &pt, int Kp, size_t fl) -> int {
            pt.base = nullptr;
            for (int l = 0; l < 8; ++l) pt.off[l] = 0;
            if (fl == 0 || Kp <= 0) return SN_OK;
            pair_layout(gl, Kp, pt.off);
            pt.base = cursor;
            cursor += fl;
            if (packed_before) return SN_OK;
            uint32_t max_rows = 0;
            for (int l = 0; l < Kp; ++l) { const uint32_t r3 = gl.res[l] * gl.res[l] * gl.res[l]; if (r3 > max_rows) max_rows = r3; }
            const dim3 gp(div_up(max_rows, 256), (uint32_t)Kp);
            const int rcl = d->table_dtype == SN_F16 ? launch(k_pack_pairs<__half>, gp, dim3(256), 0, st_main, (const __half *)d->embeddings, gl, pt, (uint32_t)Kp)
                                                     : launch(k_pack_pairs<float>, gp, dim3(256), 0, st_main, (const float *)d->embeddings, gl, pt, (uint32_t)Kp);
            if (rcl) return rcl;
            SN_LAUNCH_CHECK("k_pack_pairs");
            return SN_OK;
        };
        ProfScope ps(st_main, PK_PACK);
        // (the main grid's region is sized for the densified layout whenever the sample count allows it; levels 5-6 are packed only
        //  when the kernel that reads them will run)
        rc = pack_pairs(&cfg->grid, gl_main, pairs, route.Kv_main, route.ws.pair_main);
        if (rc) return rc;
        for (uint32_t k = 0; k + 1 < S; ++k) {
            rc = pack_pairs(&cfg->prop_grid[k], route.gl_prop[k], prop_pairs[k], dense_prefix(route.gl_prop[k]), route.ws.pair_prop[k]);
            if (rc) return rc;
        }
    }

    // ---- 4. the chunks ----
    // two bands on two streams: everything above (weight and pair packs) is on the caller's stream, the fork waits for it
    BandFork fork(st_main, route.ws.bands.slots == 2u);
    if (route.ws.bands.slots == 2u && !fork.side) {      // no side stream: the bands run one after the other in one slot, which the proposal routes count on
        route.ws.bands.slots = 1u;
        plan_chunks(cfg, io, &route);
    }
    const uint32_t chunk = route.ws.bands.chunk;
    for (uint32_t ci = 0; ci < route.chunks; ++ci) {
        const uint32_t first = ci * chunk;
        const ChunkRoute &cr = ci + 1u < route.chunks ? route.full : route.last;
        const uint32_t n = cr.n, Npad = cr.Npad;
        const uint32_t slot = fork.side ? (ci & 1u) : 0u;
        const hipStream_t st = slot ? fork.side : st_main;                  // this chunk's kernels and profile spans
        RayCommon rays;
        rays.rays_o = io->rays_o + (size_t)first * 3; rays.rays_d = io->rays_d + (size_t)first * 3;
        rays.cnf = io->cam_near_far ? io->cam_near_far + (size_t)first * 2 : nullptr;
        rays.N = n; rays.W = W; rays.rows = W ? n / W : 0; rays.Npad = Npad;
        for (int i = 0; i < 6; ++i) rays.aabb[i] = cfg->aabb[i];
        rays.min_near = cfg->min_near; rays.bound = cfg->bound; rays.contract = cfg->contract;
        rays.last_opaque = cfg->last_sample_opaque; rays.bg = cfg->bg_color;
        {
            int e = 0;
            const float m = frexpf(2.0f * cfg->bound, &e);
            rays.inv_den = (m == 0.5f && e > -100 && e < 100) ? 1.0f / (2.0f * cfg->bound) : 0.0f;
        }
        {   // tuning.linear_tile_order: which image tile a workgroup renders (tile_order_of; bit-neutral)
            rays.tlw = tile_log2w(cfg);
            const TileOrder to = tile_order_of(cfg->tuning.linear_tile_order, rays.tlw);
            rays.xcd_swizzle = to.xcd; rays.st_w = to.st_w; rays.st_h = to.st_h;
            // compaction: workgroups differ in cost by the number of live rays of their tile; a contiguous tile range per
            // XCD would leave the XCDs that own empty image bands idle (measured on the small-aabb scene: 4.4 instead of
            // 3.0 ms), so tiles go round-robin over the XCDs in dispatch order
            if (route.use_cmp) rays.xcd_swizzle = 0;
            // the role-split experiment's own tiling states the scratch columns of the row-pair order (rs_ray_of_lane)
            if (cr.fin.family == FinalRoute::RS) rays.st_w = rays.st_h = 0;
        }

        // scratch carve-up
        float *w_scr[SN_MAX_STAGES] = {nullptr}, *b_scr[SN_MAX_STAGES] = {nullptr};
        float *cur = scratch + (size_t)slot * route.ws.slot_floats;           // (bands in flight on two streams: a scratch region each)
        for (uint32_t k = 0; k + 1 < S; ++k) { w_scr[k] = cur; cur += (size_t)cfg->num_steps[k] * Npad; }
        for (uint32_t k = 1; k < S; ++k) { b_scr[k] = cur; cur += (size_t)(cfg->num_steps[k] + 1) * Npad; }
        if (cfg->with_feat) { w_scr[S - 1] = cur; cur += (size_t)cfg->num_steps[S - 1] * Npad; }

        for (uint32_t k = 0; k + 1 < S; ++k) {
            PropArgs pa;
            pa.rc = rays; pa.g = route.gl_prop[k]; pa.table = cfg->prop_grid[k].embeddings;
            pa.w0 = cfg->prop_mlp[k].weight[0]; pa.w1 = cfg->prop_mlp[k].weight[1];
            pa.T = cfg->num_steps[k]; pa.Tn = cfg->num_steps[k + 1];
            pa.bins_in = b_scr[k];
            pa.bins0_stride = io->bins0_ray_stride; pa.u_stride = io->u_ray_stride[k + 1];
            pa.bins0_tab = (k == 0 && io->bins0_table) ? io->bins0_table + (size_t)first * pa.bins0_stride : nullptr;
            pa.u_tab = io->u_table[k + 1] ? io->u_table[k + 1] + (size_t)first * pa.u_stride : nullptr;
            pa.dbg_bins_next = (io->skip_final && k + 2 == S && io->bins[S - 1]) ? io->bins[S - 1] + (size_t)first * (cfg->num_steps[S - 1] + 1) : nullptr;
            pa.w_scr = w_scr[k]; pa.bins_out = b_scr[k + 1];
            pa.dbg_bins = io->bins[k] ? io->bins[k] + (size_t)first * (pa.T + 1) : nullptr;
            pa.dbg_w = io->weights[k] ? io->weights[k] + (size_t)first * pa.T : nullptr;
            pa.dbg_sigma = io->sigmas[k] ? io->sigmas[k] + (size_t)first * pa.T : nullptr;
            pa.dbg_inds = io->inds[k + 1] ? io->inds[k + 1] + (size_t)first * (pa.Tn + 1) : nullptr;
            pa.pairs = prop_pairs[k];
            pa.skip_miss = route.use_cmp ? 1 : 0;
            {
                ProfScope ps(st, PK_PROP0 + (int)k);
                rc = launch(prop_kernel(cr.prop[k]), dim3(cr.prop[k].grid), dim3(256), 0, st, pa);
                if (rc) return rc;
            }
            SN_LAUNCH_CHECK("k_prop_stage");
        }
        if (io->skip_final) continue;                      // proposal stages only: their last resampled bins went to io->bins[S-1]
        const FinalRoute &fr = cr.fin;
        FinalArgs fa;
        fa.rc = rays; fa.g = gl_main; fa.table = cfg->grid.embeddings; fa.mlp_pack = pack;
        for (int l = 0; l < 3; ++l) { fa.w[l] = cfg->grid_mlp.weight[l]; fa.vw[l] = cfg->view_mlp.weight[l]; }
        fa.T = cfg->num_steps[S - 1];
        fa.bins_in = b_scr[S - 1]; fa.bins0_stride = io->bins0_ray_stride;
        fa.bins0_tab = (S == 1 && io->bins0_table) ? io->bins0_table + (size_t)first * fa.bins0_stride : nullptr;
        fa.sh_degree = cfg->sh_degree;
        fa.istride = io->out_stride ? io->out_stride : 3u; fa.sstride = io->out_stride ? io->out_stride : 1u;
        fa.image = io->image + (size_t)first * fa.istride; fa.depth = io->depth + (size_t)first * fa.sstride; fa.wsum = io->weights_sum + (size_t)first * fa.sstride;
        fa.dbg_bins = io->bins[S - 1] ? io->bins[S - 1] + (size_t)first * (fa.T + 1) : nullptr;
        fa.dbg_w = io->weights[S - 1] ? io->weights[S - 1] + (size_t)first * fa.T : nullptr;
        fa.dbg_sigma = io->sigmas[S - 1] ? io->sigmas[S - 1] + (size_t)first * fa.T : nullptr;
        fa.dbg_xyz = io->xyzs_last ? io->xyzs_last + (size_t)first * fa.T * 3 : nullptr;
        const uint32_t geo = route.is_any ? route.any.dg[route.any.ng] - 1u : 15u;      // geometry channels
        fa.dbg_geo = io->geo_feat_last ? io->geo_feat_last + (size_t)first * fa.T * geo : nullptr;
        fa.fimg_stride = io->head_stride ? io->head_stride : geo + 16u;
        fa.dbg_fimg = io->f_image ? io->f_image + (size_t)first * fa.fimg_stride : nullptr;
        fa.head_rgbd = (io->head_stride && io->f_image && !route.is_any) ? fa.dbg_fimg + 31 : nullptr;
        fa.pairs = pairs;
        build_final_lv(gl_main, fr.K == 7 ? 7 : dense_prefix(gl_main), pairs, cfg->grid.embeddings, 2u * (fr.f16 ? 2u : 4u), fa.lv);
        fa.w_out = cfg->with_feat ? w_scr[S - 1] : nullptr;
        fa.stop_cum = route.stop_cum;
        {
            ProfScope ps_final(st, PK_FINAL);
            note_final(fr, &g_launch);
            rc = launch_final(fr, st, fa, route.any, reinterpret_cast<uint32_t *>(pack + route.ws.ctr_offset_floats()) + (size_t)slot * SN_TILE_QUEUES);
            if (rc) return rc;
            SN_LAUNCH_CHECK(fr.family == FinalRoute::ANY ? "k_final_stage_any" : "k_final_stage");
        }
        if (cfg->with_feat) {
            const GridLevels &gf = route.gl_feat;
            const FeatRoute &feat = route.feat;
            FeatArgs ft;
            ft.rc = rays; ft.g = gf; ft.table = cfg->feat_grid.embeddings; ft.T = cfg->num_steps[S - 1];
            ft.bins_in = b_scr[S - 1]; ft.bins0_stride = io->bins0_ray_stride;
            ft.bins0_tab = (S == 1 && io->bins0_table) ? io->bins0_table + (size_t)first * ft.bins0_stride : nullptr;
            ft.w_in = w_scr[S - 1];
            ft.out_stride = io->head_stride ? io->head_stride : gf.L * gf.C;
            ft.out = io->f_feat + (size_t)first * ft.out_stride;
            ProfScope ps_feat(st, PK_FEAT);
            if (feat.patch_levels) {
                ft.level0 = 0;
                rc = launch(feat_kernel(feat, true), dim3(cr.nblk, feat.patch_levels / feat.lg), dim3(256), 0, st, ft);
                if (rc) return rc;
            }
            if (feat.patch_levels < gf.L) {
                ft.level0 = feat.patch_levels;
                rc = launch(feat_kernel(feat, false), dim3(cr.nblk, (gf.L - feat.patch_levels) / feat.lg), dim3(256), 0, st, ft);
                if (rc) return rc;
            }
            SN_LAUNCH_CHECK("k_feat_stage");
        }
    }
    return SN_OK;
}

}  // extern "C"
