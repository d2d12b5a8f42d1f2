// mlp16.inc -- the 256-wide perceptrons on v_mfma_f32_16x16x32_f16 with TWO waves per SIMD (round 5).  Included by mlp.hip inside namespace sn.
//
// Why a second skeleton.  k_mlp_wide_j gives a wave 32 rows and all 256 outputs of a layer: 128 accumulators + the previous layer's 128 raw
// outputs = every register of a SIMD, so ONE in-order wave per SIMD has to interleave its own matrix work with its own vector work, LDS reads,
// LDS-DMA issue and (fused mask head) gather latency.  Measured: a plain hidden-layer k-step takes 1.1-1.2 k cycles against 768 of matrix-pipe
// time, a gather k-step 2.9 k (profiles/r04/mask_head_traces.txt, profiles/r05/run1_trace.txt); re-ordering the MFMAs of a k-step so that no
// filler sits between an MFMA and its consumer changed nothing (profiles/r05/run1_ab.txt).  A single wave's vector instruction issues every 5-7
// cycles on this chip, two waves on a SIMD get one every ~2.9 (profiles/r04/ubench_valu_rate.txt), and an LDS-DMA piece blocks its wave for 60-185
// cycles of issue (MI355X_MICROARCH.md) -- time in which nothing else of that SIMD can run when the wave is alone.
//
// Here a wave owns 16 rows: the 16x16x32 tile's accumulator is 4 registers, 16 output tiles = 64, the previous layer's raw outputs another 64, and
// the kernel fits the 256-register budget of a 512-thread workgroup -- 8 waves, two per SIMD, sharing ONE weight ring.  Whatever one wave of a SIMD
// cannot issue (it waits for a gather, sits in a DMA issue, converts operands) the other one's MFMAs fill.
//
//   * transposed formulation as before, H^T = W X^T: A = weights (16 neurons x 32 inputs), B = activations (32 inputs x 16 rows);
//     lane l holds row l & 15 and the 8 consecutive k of group q = l >> 4; accumulator register r of lane l = D[4 q + r][l & 15];
//   * the accumulators of tiles 2 k and 2 k + 1 are therefore a valid B operand of k-step k of the next layer: slot j of group q = neuron
//     32 k + 16 (j >> 2) + 4 q + (j & 3); k_pack_mlp16 permutes the weights' k order to match, once;
//   * split-fp16 products, three per tile and k-step, small terms first (mfma3h's recipe); operands made just in time between the MFMAs
//     (k_mlp_wide_j's scheme): finished tiles leave the accumulators for `prev` two tiles behind the matrix pipe, the B operand of k-step k + 1 is
//     activated and split during k-step k;
//   * weights: one chunk = one k-step x 16 output tiles x (hi, lo) = 32 KiB, ring of 4 in LDS filled by LDS-DMA three chunks ahead, every wave
//     copies 4 KiB of each chunk; A operands are read four tiles ahead of their MFMAs.
//
// Fused mask head (XMODE 3; renderer.py:376-385, network.py:118-123): a workgroup owns 32 consecutive rays and walks their T samples in T / 4
// tiles of 128 rows -- wave w takes depth index 4 p + (w >> 1) of rays 16 (w & 1) .. + 15.  An input k-step carries FOUR levels of the C = 8 grid:
// lanes (row, q) and (row, q ^ 2) are lanes l and l ^ 32 and share the row's sample, as in k_mlp_wide_j: each locates one level (4 kx + (q & 1)
// + 2 (q >> 1)), one v_permlane32_swap per value hands offsets and weights across, and each fetches ONE 16-byte half (channels 4 (q >> 1) ..)
// of the 8 corner rows of BOTH levels -- a gather instruction touches 32 rows (16 samples x 2 levels) and no data is exchanged.
// Operand slot j of group q = level 4 kx + (q & 1) + 2 (j >> 2), channel 4 (q >> 1) + (j & 3) (k_pack_mlp16 applies the permutation).
// Results differ from k_mlp_wide_j's in the last bits only (an MFMA sums 32 products instead of 16); tests hold both to the same oracle.

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int W16_MT = WIDE / 16;                 // output tiles of a hidden layer
constexpr int W16_HKS = WIDE / 32;                // k-steps that consume a hidden layer
constexpr int W16_CHUNK_U4 = W16_MT * 2 * 64;     // uint4 per chunk (one k-step, 16 output tiles, hi | lo) = 32 KiB
// One workgroup of 512 threads per CU (WAVES = 8), 128 rows per tile, ring of 2 weight chunks (the LDS also holds the staged operands, see k_mask16).
// (WAVES = 4 -- TWO workgroups of 256 threads per CU, so that one workgroup's gather k-steps run beside the other's hidden layers -- was built and
//  measured: every workgroup streams the weights for 64 rows instead of 128 (8 LDS-DMA pieces per wave and chunk: 8.3 ms per 400x400 mask render
//  against 7.6), and results were not reproducible run to run while two workgroups shared a CU (errors of 1e-4 in a few 16-ray groups, never with
//  one workgroup per CU: profiles/r05/mlp16_determinism.txt).  Removed.)
template <int WAVES> struct W16Cfg {
    static_assert(WAVES == 8, "two 256-thread workgroups per CU (WAVES = 4) are not supported: see above");
    static constexpr int THREADS = 64 * WAVES, NBUF = 2, PIECES = W16_CHUNK_U4 / (64 * WAVES), ROWS = 16 * WAVES, GROUPS = WAVES / 4;
};
constexpr int W16_AHEAD = 2;                      // A operands are read this many tiles ahead of their MFMAs (4: 128 B of scratch per lane, 6.26 instead of 5.80 ms)

__host__ __device__ constexpr int w16_piece_of(int mt) { return (mt >= 4 && mt <= 10 && (mt & 1) == 0) ? (mt - 4) / 2 : -1; }   // operand pieces ride behind tiles 4, 6, 8, 10

#ifndef SN_W16_BBSPLIT
#define SN_W16_BBSPLIT 1     // chunks start in their own basic block: the diagnostics build, whose trace points split the blocks, ran 6.2 ms where the
#endif                       // straight-line product build ran 7.6 (profiles/r05/mlp16_ab_v1.txt): the scheduler's moves across chunk boundaries cost more than they hide
#ifndef SN_W16_JV
#define SN_W16_JV 4          // vector instructions the scheduler may place behind each MFMA
#endif

// one thread per (layer, k-step, output tile, lane): 8 weights -> (hi, lo) uint4
__global__ void k_pack_mlp16(PackArgs a) {
    SN_POISON_ALL();
    const uint32_t layer = blockIdx.y;
    const WideLayer L = a.layer[layer];
    const uint32_t nks = (L.uses_h ? (uint32_t)W16_HKS : 0u) + L.x_ks;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nks * (uint32_t)W16_MT * 64u) return;
    const uint32_t lane = t & 63u, mt = (t >> 6) % (uint32_t)W16_MT, ks = (t >> 6) / (uint32_t)W16_MT;
    const uint32_t m = mt * 16u + (lane & 15u), q = lane >> 4;
    if (L.narrow && mt != 0u) return;
    const float *Wt = a.w[layer];
    const uint32_t row = a.in_dim[layer];
    float v[8];
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        uint32_t col;
        bool valid = m < L.out;
        if (L.uses_h && ks < (uint32_t)W16_HKS) {
            col = 32u * ks + 16u * (j >> 2) + 4u * q + (j & 3u);          // register j & 3 of tile 2 ks + (j >> 2) of the previous layer
        } else {
            const uint32_t kx = ks - (L.uses_h ? (uint32_t)W16_HKS : 0u);
            uint32_t c;
            if (layer == 0u && kx < a.pair_ks) {                          // fused mask head: four grid levels per k-step (see the header)
                const uint32_t level = 4u * kx + (q & 1u) + 2u * (j >> 2);
                c = 8u * level + 4u * (q >> 1) + (j & 3u);
                valid = valid && level < a.pair_levels;
            } else if (layer == 0u && a.pair_ks) {
                c = 8u * a.pair_levels + 32u * (kx - a.pair_ks) + 8u * q + j;   // the appended channels, in their own k-step(s)
            } else {
                c = 32u * kx + 8u * q + j;
            }
            valid = valid && c < a.din;
            col = (L.uses_h ? (uint32_t)WIDE : 0u) + c;                   // skip layers see cat([h, x]) (network.py:61-63)
        }
        v[j] = valid ? (a.transposed ? Wt[(size_t)col * row + m] : Wt[(size_t)m * row + col]) : 0.0f;
    }
    uint4 ph, pl;
    split2h(v[0], v[1], ph.x, pl.x); split2h(v[2], v[3], ph.y, pl.y);
    split2h(v[4], v[5], ph.z, pl.z); split2h(v[6], v[7], ph.w, pl.w);
    // [k-step][mt][hi|lo][lane]: one chunk per k-step; a narrow last layer (<= 16 outputs): ONE chunk [k-step][hi|lo][lane] of its only tile
    const size_t base = L.narrow ? (size_t)L.w_off + (size_t)ks * 128u : (size_t)L.w_off + (size_t)ks * W16_CHUNK_U4 + (size_t)mt * 128u;
    a.pack[base + lane] = ph;
    a.pack[base + 64u + lane] = pl;
}

// k_mask16: the fused mask head (renderer.py:376-385, network.py:118-123).  One 512-thread workgroup per CU: 32 consecutive rays, T / 4 tiles of
// 128 rows (wave w: depth index 4 p + (w >> 1) of rays 16 (w & 1) .. + 15).
//
// Tile pipeline (the reason this version exists).  The gather k-steps of a tile are bound by the texture-address path (512 wave-gathers per tile
// and CU at ~45 cycles = 23 k cycles), the hidden layers by instruction issue and the matrix pipe (~24 k): run one after the other -- as
// k_mlp_wide_j<3> and the first version of this kernel do -- each leaves the other unit idle (profiles/r05/mlp16_trace_v1.txt).  Here the first
// layer's operands of tile p + 1 are made DURING the hidden layer of tile p, as eight small background units, one per hidden k-step: a unit
// locates its level, requests 4 corners x 2 levels (8 gathers into 32 registers) behind the chunk's first tile and blends them behind its
// tenth -- consumed inside the chunk, so that nothing is in flight at the chunk's synchronisation and no chunk holds both the layer state
// (128 registers) and a full landing set (70) -- and every second unit splits the finished 8 values and parks them in an LDS staging area
// (5 k-steps x 32 bytes per lane = 80 KiB).  The appended channels follow during the narrow last layer.  Layer 0 of the next tile then reads
// its operands from LDS: no gather, no blend, nothing to wait for.  (LDS: ring of 2 chunks 64 KiB + staging 80 KiB + biases and level table.)
//
// LDS life cycle of this kernel (round 6; why the shipping form is free of the hazard that made two faster variants irreproducible --
// background units whose gathers stayed in flight across a chunk boundary, and units spread over layer 0's chunks:
// profiles/r05/mask16_units_ab.txt, mask16_trace_halfunits_l0_nondeterministic.txt).  Four regions, three rules:
//   (R1) staging area lds_stage[k-step][hi | lo][tid] and the appended channels' lds_ex[hi | lo][wave * 32 + (lane & 31)]: every slot is written
//        and read by ONE thread only (the index carries tid / the lane's own slot; lanes with q >= 2 read a neighbour's lds_ex slot and DISCARD
//        it).  A wave's LDS instructions execute in issue order, so the only hazards are program-order ones: tile p + 1's operand is parked
//        (park_levels / park_extra) strictly after this thread's stage_read / read_extra of tile p's -- layer 0 of tile p has finished reading
//        k-step kx before the hidden layer's unit 2 kx + 1 parks k-step kx of the tile ahead.  No barrier is involved and none is needed.
//   (R2) weight ring: chunk g lives in buffer g % 2.  The LDS-DMA of chunk g + 1 into buffer (g + 1) % 2 is issued by sync_and_refill(g), i.e.
//        AFTER `s_waitcnt vmcnt(0) lgkmcnt(0)` + the workgroup barrier that every wave passes behind tile 14 of chunk g - 1: at that point each
//        wave has issued AND completed all its A-operand reads of chunk g - 1 (tiles 0..15 are read two tiles ahead, so the read of tile 15 is
//        issued behind tile 13), and its own share of chunk g has landed (vmcnt(0)); the barrier makes both true for the whole workgroup.
//        Nothing else of a wave is in flight at that barrier: a background unit is requested and blended inside ONE chunk (the variants that
//        carried 8 gathers across it are the irreproducible ones).
//   (R3) the narrow layer's weights (lds_nw), the level table (lds_lv) and the live-tile mask are written once before the first barrier and
//        only read afterwards; the final reduction reuses the ring only after vmcnt(0) + a barrier.
// `make poison` (every LDS word a signalling NaN at entry) + the 30-repetition determinism run + the GPU suite under that build exercise
// these rules once per round (profiles/r06/pytest_gpu_poison_build.txt, stress_determinism.txt).  What the two fast variants broke is R2's
// "nothing else in flight at the barrier"; the cause inside the hardware (the order in which LDS-DMA writes and returning gathers retire
// against vmcnt) was not isolated.  Round 6, second look: the LDS-DMA helpers lacked the wait state the ISA asks for between the SALU write of
// M0 and the DMA that reads it (dma16 / dma16x4 in mlp.hip: fixed, M0 saved and restored) -- a real hazard, but not this one: the
// cross-chunk variant rebuilt on the fixed helpers is still irreproducible, with a counted wait and with a full drain at the synchronisation
// alike, and slower than this order (profiles/r06/mask16_cross_ab_rejected.txt); it is not in the tree.
//
// EPI selects the epilogue behind the narrow layer; everything in front of it is one source path.
//   MASK16_COMPOSITE  out[ray, m] = sum_t wts[ray, t] * logit[ray, t, m] (sn_rm_mask_head): per-wave sums, then the fixed-order cross-wave sum.
//   MASK16_LABELS     labels[ray, t] = the lowest index attaining max_m logit[ray, t, m] (sn_rm_mask_point_labels): nothing is summed, `wts` only
//                     says which tiles are live (the caller passes y = delta * sigma).  Lane 16 q + nloc holds neurons 4 q .. 4 q + 3 of row
//                     nloc: a max with lowest-index tie-break over the lane's valid neurons, then two cross-lane steps on (value, index) pairs
//                     (v_permlane16_swap joins rows 0|1 and 2|3, v_permlane32_swap the halves -- no LDS, no counter), and lanes 0..15 store
//                     one byte per row; a.out != NULL: every lane also stores its valid logits to out[row][m].  A NaN logit never wins a
//                     comparison; a row whose logits are all NaN or -inf gets label 0.  Plain stores, issued right behind the narrow layer;
//                     the next sync_and_refill's vmcnt(0) (or the kernel's last one) drains them: no counted wait, nothing else crosses a chunk.
//                     Skipped tiles are not written: the host fills labels with 0xFF (and logits with 0) on the stream first.
constexpr int MASK16_COMPOSITE = 0, MASK16_LABELS = 1;
template <int WAVES, int EPI = MASK16_COMPOSITE>
__global__ __launch_bounds__(64 * WAVES, 2) void k_mask16(WideArgs a) {
    SN_POISON_ALL();
    typedef W16Cfg<WAVES> Cfg;
    constexpr int W16_NBUF = Cfg::NBUF, W16_THREADS = Cfg::THREADS;
    constexpr uint32_t STAGE_KS = 4;       // staged k-steps: up to 4 of grid levels (16 levels); the appended channels' operand stays in registers
    constexpr uint32_t NARROW_U4 = W16_HKS * 128;      // the narrow last layer's weights, resident: [k-step][hi | lo][lane] = 16 KiB
    extern __shared__ __attribute__((aligned(16))) uint4 lds_w[];        // W16_NBUF x W16_CHUNK_U4, then the staging area, then floats
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nloc = lane & 15u, q = lane >> 4, half = lane >> 5, u = q & 1u;
    uint4 *lds_stage = lds_w + W16_NBUF * W16_CHUNK_U4;                                  // [STAGE_KS][hi | lo][THREADS]
    uint4 *lds_nw = lds_stage + STAGE_KS * 2u * (uint32_t)W16_THREADS;                    // [NARROW_U4]
    uint4 *lds_ex = lds_nw + NARROW_U4;                                                   // [hi | lo][THREADS / 2]: the appended channels' operand (E <= 16: lanes with q < 2 hold them)
    uint32_t *lds_lv = reinterpret_cast<uint32_t *>(lds_ex + (uint32_t)W16_THREADS);     // [4][SN_MAX_LEVELS]: res, size, mode, off; then one word: live-tile mask
    // (no biases: the reference's mask_mlp has none, network.py:118-123, and the host sends stacks with biases to k_mlp_wide_j<3> -- a layer
    //  starts from zero accumulators through the C operand of its first k-step)
    if (tid < (uint32_t)SN_MAX_LEVELS) {
        lds_lv[tid] = a.g.res[tid]; lds_lv[SN_MAX_LEVELS + tid] = a.g.size[tid];
        lds_lv[2 * SN_MAX_LEVELS + tid] = a.g.mode[tid]; lds_lv[3 * SN_MAX_LEVELS + tid] = a.g.off[tid];
    }
    if (tid == 0u) lds_lv[4 * SN_MAX_LEVELS] = 0u;
    typedef __attribute__((address_space(3))) void lds_void;

    const uint32_t ntiles = a.T >> 2;
    const uint32_t ray = blockIdx.x * (16u * Cfg::GROUPS) + 16u * (wave % (uint32_t)Cfg::GROUPS) + nloc;   // 16 rays per wave, depth phase wave / GROUPS
    const uint32_t phase = wave / (uint32_t)Cfg::GROUPS;
    const bool ok = ray < a.N / a.T;
    const uint32_t row0 = (ok ? ray : 0u) * a.T + phase;                  // this lane's row of tile t: row0 + 4 t
    const uint32_t Lg = a.g.L, gks = (Lg + 3u) >> 2;                      // k-steps that carry grid levels; one more for the appended channels
    float x01[3] = {0.0f, 0.0f, 0.0f};     // table coordinates of the sample whose operands are being made (the tile AHEAD in steady state)
    bool x_oob = false;
    auto set_sample = [&](const float (&p)[3]) {
        x_oob = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {   // grid.py:156
            const float v = p[d] + a.bound;
            x01[d] = a.inv_den != 0.0f ? v * a.inv_den : v / (2.0f * a.bound);
            x_oob = x_oob || x01[d] < 0.0f || x01[d] > 1.0f;                // gridencoder.cu:105-130: zeros outside [0,1]
        }
    };
    auto fetch_sample = [&](uint32_t tile, float &w, float (&p)[3]) { // weight and position of this lane's sample of `tile`
        const uint32_t nn = row0 + 4u * tile;
        w = ok ? a.wts[nn] : 0.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] = a.xyz[(size_t)nn * 3u + d];
    };
    auto load_extra = [&](uint32_t tile, float (&e)[8]) {            // this lane's 8 appended channels, extra[row][8 q + 0..7], zero padded
        const float *row = a.extra + (size_t)(row0 + 4u * tile) * (a.E ? a.E : 1u);
        uint32_t qq = q;
        asm volatile("" : "+v"(qq));       // (opaque: otherwise the 8 clamped column offsets are hoisted out of the tile loop as 8 address pairs, spilled, and
                                           //  every reload waits for ALL loads in flight -- the tile top cost 9.6 k cycles that way)
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const uint32_t c = 8u * qq + i;
            const float v = a.E ? row[c < a.E ? c : a.E - 1u] : 0.0f;
            e[i] = c < a.E ? v : 0.0f;
        }
    };
    auto stage_write = [&](uint32_t kx, const uint32_t (&h)[4], const uint32_t (&l)[4]) {
        lds_stage[(2u * kx) * (uint32_t)W16_THREADS + tid] = make_uint4(h[0], h[1], h[2], h[3]);
        lds_stage[(2u * kx + 1u) * (uint32_t)W16_THREADS + tid] = make_uint4(l[0], l[1], l[2], l[3]);
    };
    auto stage_read = [&](uint32_t kx, uint32_t (&h)[4], uint32_t (&l)[4]) {
        const uint4 vh = lds_stage[(2u * kx) * (uint32_t)W16_THREADS + tid], vl = lds_stage[(2u * kx + 1u) * (uint32_t)W16_THREADS + tid];
        h[0] = vh.x; h[1] = vh.y; h[2] = vh.z; h[3] = vh.w; l[0] = vl.x; l[1] = vl.y; l[2] = vl.z; l[3] = vl.w;
    };

    floatx4 acc[W16_MT];
    float prev[4 * W16_MT];                // the previous layer's outputs before the activation: prev[4 t + r] = register r of its tile t
    uint32_t g = 0;                        // chunks consumed so far
    const uint32_t tile_chunks = a.total_chunks - 1u;       // (the narrow last layer's chunk, the stream's last one, is resident in LDS)
    const uint32_t total_chunks = tile_chunks * ntiles;     // the workgroup's whole stream: the other layers' packed weights, once per tile, back to back
    constexpr uint32_t CHUNK_BYTES = W16_CHUNK_U4 * sizeof(uint4), WAVE_U4 = 64u * Cfg::PIECES;                 // a wave copies WAVE_U4 uint4 of every chunk
    const uint32_t lds_w_off4 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void *)lds_w) + wave * (WAVE_U4 * 16u);
    auto dma_chunk = [&](uint32_t c) {     // this wave's share of chunk c into its ring buffer
        const uint4 *src = a.pack + (size_t)(c % tile_chunks) * W16_CHUNK_U4 + wave * WAVE_U4 + lane;
        dma16x4(src, lds_w_off4 + (c % (uint32_t)W16_NBUF) * CHUNK_BYTES);
    };
    static_assert(Cfg::PIECES == 4 && Cfg::NBUF == 2, "one dma16x4 per wave and chunk, one chunk ahead");
    {   // the narrow layer's weights: 16 KiB, once; every wave copies 2 KiB
        const uint4 *src = a.pack + (size_t)a.layer[a.nl - 1u].w_off + wave * 128u + lane;
        const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void *)lds_nw) + wave * 2048u;
        dma16(src, dst); dma16(src + 64, dst + 1024u);
    }
    dma_chunk(0u);
    __syncthreads();                       // publishes lds_bias / lds_lv

    // ---- weight ring: chunk g in buffer g % 2, chunk g + 1 requested at the synchronisation on chunk g.  Nothing else of this wave is in
    //      flight there: a background unit is requested AND blended inside one chunk.  (Units whose 8 gathers stayed in flight across the chunk
    //      boundary -- requested in chunk k, blended in chunk k + 1, vmcnt(8) at the synchronisation -- gave results that differed from run to run in
    //      ~5 % of the 16-ray groups, with vmcnt(0) at the synchronisation too; the same units inside one chunk are exact and were faster:
    //      profiles/r05/mask16_units_ab.txt.) ----
    auto sync_and_refill = [&](uint32_t gn) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : : : "memory");
        __syncthreads();
        // every wave has finished reading chunk gn - 1 (its last reads were waited for above): its buffer takes chunk gn + 1
        if (gn + 1u < total_chunks) dma_chunk(gn + 1u);
    };
    uint4 ah[W16_AHEAD], al[W16_AHEAD];    // A operands of the next tiles (slot = tile & (AHEAD - 1)); across a chunk boundary: the first tiles of the next chunk
    auto read_a = [&](uint32_t gn, int tile, int slot) {
        const uint4 *buf = lds_w + (gn % (uint32_t)W16_NBUF) * W16_CHUNK_U4 + lane;
        ah[slot] = buf[tile * 128]; al[slot] = buf[tile * 128 + 64];
    };
    sync_and_refill(0u);
#pragma unroll
    for (int i = 0; i < W16_AHEAD; ++i) read_a(0u, i, i);

    const bool leaky = a.leaky != 0u;
    auto act = [&](float t) { return relu_or_leaky(t, leaky); };   // network.py:65-66, as in k_mlp_wide
    auto escape_tile = [&](auto tc) {      // (the empty asm makes the moved value opaque: see k_mlp_wide_j)
        constexpr int t = decltype(tc)::value;
        static_for<4>([&](auto rc) { constexpr int r = decltype(rc)::value; float v = acc[t][r]; asm("" : "+v"(v)); prev[4 * t + r] = v; });
    };
    auto mfma3 = [&](const uint4 &Ah4, const uint4 &Al4, const half8_t &Bh, const half8_t &Bl, floatx4 c) {
        const half8_t Ah = __builtin_bit_cast(half8_t, Ah4), Al = __builtin_bit_cast(half8_t, Al4);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Bh, c, 0, 0, 0);   // small terms first
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bh, c, 0, 0, 0);
        return c;
    };

    // one chunk = one k-step x 16 output tiles.  FIRST: the layer's first k-step (accumulators start from the bias through the C operand);
    // ESC: its last one (finished tiles leave for `prev` two tiles behind the matrix pipe, tiles 14 and 15 in the next layer's FIRST chunk).
    // prep(mt): whatever rides behind tile mt.  Behind tile 16 - AHEAD the workgroup synchronises on chunk g + 1; the tiles after it read
    // the first tiles of that chunk.
    auto chunk16 = [&](auto first_tag, auto esc_tag, const uint32_t (&ob_h)[4], const uint32_t (&ob_l)[4], auto &&prep) {
        constexpr bool FIRST = decltype(first_tag)::value, ESC = decltype(esc_tag)::value;
        if (g < 128u) wide_trace(g);
#if SN_W16_BBSPLIT
        if (__builtin_expect(tid == 0xffffu, 0)) asm volatile("s_nop 0");     // a basic-block boundary per chunk (never taken): see SN_W16_BBSPLIT
#endif
        const half8_t Bh = __builtin_bit_cast(half8_t, make_uint4(ob_h[0], ob_h[1], ob_h[2], ob_h[3]));
        const half8_t Bl = __builtin_bit_cast(half8_t, make_uint4(ob_l[0], ob_l[1], ob_l[2], ob_l[3]));
        static_for<W16_MT>([&](auto mtc) {
            constexpr int mt = decltype(mtc)::value, s = mt & (W16_AHEAD - 1);
            floatx4 c;
            if constexpr (FIRST) c = floatx4{0.0f, 0.0f, 0.0f, 0.0f}; else c = acc[mt];
            acc[mt] = mfma3(ah[s], al[s], Bh, Bl, c);
            if constexpr (mt + W16_AHEAD == W16_MT) {
                if (g + 1u < total_chunks) sync_and_refill(g + 1u);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (mt + W16_AHEAD < W16_MT) read_a(g, mt + W16_AHEAD, s);
            else read_a(g + 1u, mt + W16_AHEAD - W16_MT, s);            // (past the last chunk: reads LDS that nobody uses)
            if constexpr (FIRST && mt < 2) escape_tile(int_tag<W16_MT - 2 + mt>{});
            if constexpr (ESC && mt >= 2) escape_tile(int_tag<mt - 2>{});
            prep(mtc);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, SN_W16_JV, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, SN_W16_JV, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, SN_W16_JV, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
        ++g;
    };

    uint32_t bh[4], bl[4], nbh[4] = {0u, 0u, 0u, 0u}, nbl[4] = {0u, 0u, 0u, 0u};   // operand of the chunk about to run / of the one after it
    auto advance = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) { bh[p] = nbh[p]; bl[p] = nbl[p]; }
    };
    auto h_piece = [&](auto kc, auto pc) {      // pair p (0..3) of h k-step k: prev[8 k + 2 p], + 1 -> nbh / nbl
        constexpr int k = decltype(kc)::value, p = decltype(pc)::value;
        split2h(act(prev[8 * k + 2 * p]), act(prev[8 * k + 2 * p + 1]), nbh[p], nbl[p]);
    };

    // ---- grid levels.  This lane LOCATES level 4 kx + u + 2 half and FETCHES channels 4 half .. + 3 of levels A = 4 kx + u, B = A + 2 (header) ----
    auto corner_weight = [](const float (&p)[3], int idx) {              // gridencoder.cu:315-327: ((wx wy) wz)
        const float wx = (idx & 1) ? p[0] : 1.0f - p[0], wy = (idx & 2) ? p[1] : 1.0f - p[1], wz = (idx & 4) ? p[2] : 1.0f - p[2];
        return (wx * wy) * wz;
    };
    // NC corners starting at C0 of both levels of k-step kx, for the sample in x01: request ...
    struct Landing { float pA[3], pB[3]; float4 rA[4], rB[4]; };
    auto request = [&](uint32_t kx, auto c0_tag, Landing &r) {
        constexpr int C0 = decltype(c0_tag)::value;
        const uint32_t level = umin(4u * kx + u + 2u * half, Lg - 1u);
        const uint32_t res = lds_lv[level], size = lds_lv[SN_MAX_LEVELS + level], mode = lds_lv[2 * SN_MAX_LEVELS + level];
        const uint32_t base = lds_lv[3 * SN_MAX_LEVELS + level];
        float pos[3];
        uint32_t cell[3], offs[8];
        locate_linear(x01, res, pos, cell);
        corner_offsets<-1, 32u>(cell, res, size, mode, offs);           // bytes from the level's first row (unused corners fold away)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const auto pp = __builtin_amdgcn_permlane32_swap(__float_as_uint(pos[d]), __float_as_uint(pos[d]), false, false);   // [A | A], [B | B]
            r.pA[d] = __uint_as_float(pp[0]); r.pB[d] = __uint_as_float(pp[1]);
        }
        const char *tabh = reinterpret_cast<const char *>(a.table) + 16u * half;                         // this lane's half of every row
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t off = base * 32u + offs[C0 + i];               // bytes from the table's start (< 2^32: checked on the host)
            const auto po = __builtin_amdgcn_permlane32_swap(off, off, false, false);
            r.rA[i] = *reinterpret_cast<const float4 *>(tabh + po[0]);
            r.rB[i] = *reinterpret_cast<const float4 *>(tabh + po[1]);
        }
    };
    // ... and blend (corner 0 starts the sums)
    auto blend = [&](auto c0_tag, const Landing &r, float (&v)[8]) {
        constexpr int C0 = decltype(c0_tag)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = C0 + i;
            const float wA = corner_weight(r.pA, idx), wB = corner_weight(r.pB, idx);
            const float ra[4] = {r.rA[i].x, r.rA[i].y, r.rA[i].z, r.rA[i].w}, rb[4] = {r.rB[i].x, r.rB[i].y, r.rB[i].z, r.rB[i].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] = __builtin_fmaf(wA, ra[c], idx == 0 ? 0.0f : v[c]);
                v[4 + c] = __builtin_fmaf(wB, rb[c], idx == 0 ? 0.0f : v[4 + c]);
            }
        }
    };
    auto park_levels = [&](uint32_t kx, const float (&v)[8]) {         // zero what is outside the box / beyond the last level, split, stage
        const bool zA = x_oob || 4u * kx + u >= Lg, zB = x_oob || 4u * kx + u + 2u >= Lg;
        uint32_t h[4], l[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) { const bool z = p < 2 ? zA : zB; split2h(z ? 0.0f : v[2 * p], z ? 0.0f : v[2 * p + 1], h[p], l[p]); }
        stage_write(kx, h, l);
    };
    // the appended channels' operand: E <= 16 (host), so only the lanes with q < 2 carry channels -- 256 slots of 2 x 16 bytes
    const uint32_t ex_slot = wave * 32u + (lane & 31u);
    auto park_extra = [&](const float (&e)[8]) {
        uint32_t h[4], l[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) split2h(e[2 * p], e[2 * p + 1], h[p], l[p]);
        if (q < 2u) {
            lds_ex[ex_slot] = make_uint4(h[0], h[1], h[2], h[3]);
            lds_ex[(uint32_t)W16_THREADS / 2u + ex_slot] = make_uint4(l[0], l[1], l[2], l[3]);
        }
    };
    auto read_extra = [&](uint32_t (&h)[4], uint32_t (&l)[4]) {
        const uint4 vh = lds_ex[ex_slot], vl = lds_ex[(uint32_t)W16_THREADS / 2u + ex_slot];       // (q >= 2: another lane's slot, discarded)
        const bool has = q < 2u;
        h[0] = has ? vh.x : 0u; h[1] = has ? vh.y : 0u; h[2] = has ? vh.z : 0u; h[3] = has ? vh.w : 0u;
        l[0] = has ? vl.x : 0u; l[1] = has ? vl.y : 0u; l[2] = has ? vl.z : 0u; l[3] = has ? vl.w : 0u;
    };

    const uint32_t K0 = gks + (a.E ? 1u : 0u);     // input k-steps of layer 0
    float out_acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // sum over this wave's samples of weight x logit, per ray (neurons 4 q + r)
    float bv[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // the background units' running blend (two units per k-step)
    Landing R;                                     // the unit in flight
    // Live tiles, once per workgroup.  A tile whose 128 samples all carry weight exactly 0 adds nothing to any ray and is skipped whole
    // (k_mlp_wide_j; INTEGRATION.md states the one observable difference: the reference's 0 * inf = NaN for a diverged mask MLP).  Bit t of
    // `live` = tile t has a nonzero weight: every lane reads its T / 4 weights, a ballot per tile, one LDS word, one barrier -- no vote and no
    // dependent weight load at a tile's top afterwards (the votes of the first version cost ~5 k cycles per tile behind their loads).
    uint32_t live = 0u;
    {
        uint32_t mine = 0u;
        for (uint32_t t = 0; t < ntiles; ++t) {
            const float w = ok ? a.wts[row0 + 4u * t] : 0.0f;
            mine |= (__ballot(w != 0.0f) != 0ull ? 1u : 0u) << t;
        }
        if (lane == 0u && mine) atomicOr(&lds_lv[4 * SN_MAX_LEVELS], mine);
        __syncthreads();
        live = __builtin_amdgcn_readfirstlane(lds_lv[4 * SN_MAX_LEVELS]);
    }
    auto next_live = [&](uint32_t from) {          // first live tile >= from, or ntiles
        const uint32_t rest = from < 32u ? live >> from : 0u;
        return rest ? from + (uint32_t)__builtin_ctz(rest) : ntiles;
    };
    uint32_t tile = next_live(0u), nt = ntiles;
    float wt = 0.0f, nx[3] = {0.0f, 0.0f, 0.0f};
    if (tile < ntiles) {                           // the first live tile's operands, in the open (once per workgroup)
        fetch_sample(tile, wt, nx);
        set_sample(nx);
        float e[8];
        load_extra(tile, e);
        for (uint32_t kx = 0; kx < gks; ++kx) {
            Landing r1;
            float v[8];
            request(kx, int_tag<0>{}, R); request(kx, int_tag<4>{}, r1);
            blend(int_tag<0>{}, R, v); blend(int_tag<4>{}, r1, v);
            park_levels(kx, v);
        }
        park_extra(e);
    }
#pragma clang loop unroll(disable)
    while (tile < ntiles) {
        // the tile AHEAD: its weight (used at its own end), position (the background units work on it from this tile's last layer-0 chunk on) and
        // appended channels (parked behind this tile's own have been read) are requested now and land under layer 0
        nt = next_live(tile + 1u);
        const uint32_t na = nt < ntiles ? nt : tile;   // (past the last tile: the units run on this tile's coordinates again, results never read)
        float wt_next, e[8];
        fetch_sample(na, wt_next, nx);
        load_extra(na, e);
        // ---- layer 0: its operands are staged in LDS ----
#pragma unroll
        for (int mt = 0; mt < W16_MT; ++mt) acc[mt] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
        if (tile == 0u) wide_trace(128u);
        wide_trace(143u);
        if (gks) stage_read(0u, bh, bl); else read_extra(bh, bl);
#pragma clang loop unroll(disable)
        for (uint32_t c = 0; c + 1u < K0; ++c) {
            chunk16(bool_tag<false>{}, bool_tag<false>{}, bh, bl, [&](auto mtc) {
                if constexpr (decltype(mtc)::value == 2) {
                    if (c + 1u < gks) stage_read(c + 1u, nbh, nbl); else read_extra(nbh, nbl);   // the k-step behind the last grid one is the appended channels'
                }
            });
            advance();
        }
        set_sample(nx);
        // the chunk that hands layer 0 over parks the tile ahead's appended channels (this tile's own have been read)
        chunk16(bool_tag<false>{}, bool_tag<true>{}, bh, bl, [&](auto mtc) {
            constexpr int mt = decltype(mtc)::value, p = w16_piece_of(mt);
            if constexpr (p >= 0) h_piece(int_tag<0>{}, int_tag<p>{});        // next operand = tiles 0, 1 (escaped behind tiles 2, 3)
            if constexpr (mt == 12) park_extra(e);
        });
        advance();

        // ---- layer 1 (hidden): k-step k carries background unit k of the tile ahead -- corners 4 (k & 1) .. + 3 of grid k-step k >> 1: requested
        // behind tile 0, blended behind tile 12, and every second unit parks the finished k-step behind tile 13 ----
        if (tile == 0u) wide_trace(129u);
        static_for<W16_HKS>([&](auto kc) {
            constexpr int k = decltype(kc)::value, kx = k >> 1, C0 = 4 * (k & 1);
            auto prep = [&](auto mtc) {
                constexpr int mt = decltype(mtc)::value, p = w16_piece_of(mt);
                if constexpr (mt == 0) request((uint32_t)kx, int_tag<C0>{}, R);
                if constexpr (p >= 0) {
                    if constexpr (k + 1 < W16_HKS) h_piece(int_tag<k + 1>{}, int_tag<p>{});
                    else h_piece(int_tag<0>{}, int_tag<p>{});     // the layer's last k-step: the next layer's first operand (tiles 0, 1 escaped behind tiles 2, 3)
                }
                if constexpr (mt == 12) blend(int_tag<C0>{}, R, bv);
                if constexpr (C0 == 4 && mt == 13) park_levels((uint32_t)kx, bv);
            };
            if constexpr (k == 0) chunk16(bool_tag<true>{}, bool_tag<false>{}, bh, bl, prep);
            else if constexpr (k + 1 < W16_HKS) chunk16(bool_tag<false>{}, bool_tag<false>{}, bh, bl, prep);
            else chunk16(bool_tag<false>{}, bool_tag<true>{}, bh, bl, prep);
            advance();
        });

        // ---- layer 2 (narrow, <= 16 outputs): its 8 k-steps x 1 tile from the resident weights, no ring slot, no synchronisation; the operand of
        // k-step k + 1 is made between the MFMAs of k-step k.  Tiles 14 and 15 of the hidden layer leave the accumulators first ----
        {
            if (tile == 0u) wide_trace(130u);
            escape_tile(int_tag<W16_MT - 2>{}); escape_tile(int_tag<W16_MT - 1>{});
            wide_trace(140u);
            uint4 nh[2], nlo[2];
            nh[0] = lds_nw[lane]; nlo[0] = lds_nw[64u + lane]; nh[1] = lds_nw[128u + lane]; nlo[1] = lds_nw[192u + lane];
            floatx4 c0 = {0.0f, 0.0f, 0.0f, 0.0f};
            static_for<W16_HKS>([&](auto kc) {
                constexpr int k = decltype(kc)::value, s = k & 1;
                const half8_t Bh = __builtin_bit_cast(half8_t, make_uint4(bh[0], bh[1], bh[2], bh[3]));
                const half8_t Bl = __builtin_bit_cast(half8_t, make_uint4(bl[0], bl[1], bl[2], bl[3]));
                c0 = mfma3(nh[s], nlo[s], Bh, Bl, c0);
                if constexpr (k + 2 < W16_HKS) { nh[s] = lds_nw[(k + 2) * 128 + lane]; nlo[s] = lds_nw[(k + 2) * 128 + 64 + lane]; }
                if constexpr (k + 1 < W16_HKS) static_for<4>([&](auto pc) { h_piece(int_tag<k + 1>{}, pc); });
                __builtin_amdgcn_sched_barrier(0);
                advance();
            });
            acc[0] = c0;
            wide_trace(141u);
        }

        {   // range check of the split-fp16 arithmetic (k_mlp_wide's): an activation beyond 65504 reaches the last layer as inf / NaN.  (Only
            // tile 0 is an output; reading the other fifteen here would keep 60 registers alive through the narrow layer.)
            float chk = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) chk = __builtin_fmaf(acc[0][r], 0.0f, chk);
            if (ok && chk != chk) g_wide_overflow = 1;
        }
        if constexpr (EPI == MASK16_LABELS) {
            const uint32_t K = a.layer[a.nl - 1u].out, nn = row0 + 4u * tile;     // this lane's row of the tile: sample (ray, 4 tile + phase)
            float best = -__builtin_inff();
            uint32_t bi = 4u * q;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t m = 4u * q + (uint32_t)r;
                const float v = acc[0][r];
                if (m < K && v > best) { best = v; bi = m; }
                if (a.out && ok && m < K) a.out[(size_t)nn * K + m] = v;
            }
            auto join = [&](float v0, uint32_t i0, float v1, uint32_t i1) {     // (value, index) pairs: the larger value, the lower index on a tie
                const bool second = v1 > v0 || (v1 == v0 && i1 < i0);
                best = second ? v1 : v0; bi = second ? i1 : i0;
            };
            {
                const auto pv = __builtin_amdgcn_permlane16_swap(__float_as_uint(best), __float_as_uint(best), false, false);   // [r0 r0 r2 r2], [r1 r1 r3 r3]
                const auto pi = __builtin_amdgcn_permlane16_swap(bi, bi, false, false);
                join(__uint_as_float(pv[0]), pi[0], __uint_as_float(pv[1]), pi[1]);
            }
            {
                const auto pv = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);   // [lo | lo], [hi | hi]
                const auto pi = __builtin_amdgcn_permlane32_swap(bi, bi, false, false);
                join(__uint_as_float(pv[0]), pi[0], __uint_as_float(pv[1]), pi[1]);
            }
            if (ok && q == 0u) a.labels[nn] = (uint8_t)bi;
            (void)wt; (void)out_acc;
        } else {
            // renderer.py:384: out[ray, m] = sum_t w[ray, t] * logits[ray, t, m]: this wave's t of this tile
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float t = wt * acc[0][r]; out_acc[r] = out_acc[r] + t; }
        }
        wt = wt_next; tile = nt;
        wide_trace(142u);
    }                                      // tiles
    wide_trace(160u);
    if constexpr (EPI == MASK16_LABELS) {
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");         // (skipped tiles leave a prefetched weight chunk in flight: it lands before the LDS is given back)
        __syncthreads();
        return;
    }
    const WideLayer LL = a.layer[a.nl - 1u];
    // waves GROUPS d + group, d = 0..3, hold the depth phases of the same 16 rays: fixed-order sum through LDS (the weight ring is dead)
    float *part = reinterpret_cast<float *>(lds_w);                  // [WAVES][16 rays][16 neurons]
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");             // (skipped tiles leave a prefetched weight chunk in flight)
    __syncthreads();
    *reinterpret_cast<float4 *>(part + (wave * 16u + nloc) * 16u + 4u * q) = make_float4(out_acc[0], out_acc[1], out_acc[2], out_acc[3]);
    __syncthreads();
    if (wave < (uint32_t)Cfg::GROUPS && ok) {
        constexpr uint32_t G = Cfg::GROUPS;
        float *orow = a.out + (size_t)ray * LL.out;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t m = 4u * q + r;
            const float t = ((part[((0u * G + wave) * 16u + nloc) * 16u + m] + part[((1u * G + wave) * 16u + nloc) * 16u + m]) + part[((2u * G + wave) * 16u + nloc) * 16u + m])
                            + part[((3u * G + wave) * 16u + nloc) * 16u + m];
            if (m < LL.out) orow[m] = t;
        }
    }
}
