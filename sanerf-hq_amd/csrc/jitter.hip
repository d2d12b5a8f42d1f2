// jitter.hip — the jitter tables of a perturbed render from a counter-based generator on the device, for gfx950.
//   sn_rm_jitter_tables     per-ray stage-0 bins and sample_pdf u of EVERY stage of a schedule (what sn_render_io takes as bins0_table /
//                           u_table[k] with a ray stride) in one launch (and one thread's worth of a second): no torch generator, no uniform scratch buffer, capturable, and a
//                           replayed graph draws fresh jitter on every replay
//
// Value of an element (stage k, global ray g = ray_base + n, column j of a row of T1 = num_steps[k] + 1):
//   w       = philox4x32_10(counter = (g, (k << 24) | (j >> 2), draw_lo, draw_hi), key = (seed_lo, seed_hi))[j & 3]
//   uniform = float(w >> 8) * 2^-24                                       (24 bits: exact in fp32, in [0, 1))
//   entry   = jitter_value(uniform, T1, j, kind = k == 0 ? 0 : 1)         (sn_common.h: k_jitter's arithmetic, so the table is bit-equal to
//                                                                          sn_rm_jitter fed with the same uniforms)
// A value depends on (seed, draw, k, g, j) only -- not on N, the grid or how an image is cut into chunks.  Philox4x32-10 is the
// generator of Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11); its multiplications are 32x32 -> 64
// (__umulhi + the low product).
//
// State: four uint64 on the device -- seed, draw, ticket, reserved.  Every lane reads (seed, draw) when it starts.  With advance != 0 a
// one-thread launch behind the table launch stores draw + 1: the kernel boundary is what puts every workgroup's read in front of the write.
// (A ticket on state[2] in the manner of sn_reduce.h / k_adam_multi -- the workgroup that draws the last one advances -- was built first and
// measured: with an acq_rel agent-scope add per workgroup -- its release writes back the XCD's L2 behind the tile's fresh stores -- the
// 38 700 workgroups of an 800x800 image with the schedule [128, 64, 32] took 4.4 ms, about 110 ns per ticket, for a table that takes a
// fraction of that to compute; a ticket fits the few hundred workgroups of the meters, not a grid of this size.  The word stays in the
// layout, zero at rest, and nobody touches it.)  Both launches are captured like any other, so a replayed graph draws fresh jitter on
// every replay.
//
// Shape: a workgroup of 256 lanes owns a tile that is CONTIGUOUS in the table: whole rows (a multiple of four of them, so that a tile
// starts on a 16-byte boundary whenever the table does -- rows are T1 floats and in general not 16-byte aligned), or, for rows longer than
// JT_ROW_MAX, one JT_TILE-column piece of one row.  A lane owns whole Philox groups: four consecutive columns of one row, never past the
// row's end.  The values go to their place in an LDS image of the tile; after a barrier the image leaves as consecutive 16-byte stores
// (consecutive dwords where the tile is not aligned, and for its last len % 4 values).  Plain vector stores only.
#include "sn_common.h"

namespace sn {

constexpr uint32_t JT_THREADS = 256;
constexpr uint32_t JT_TILE = 4096;                   // floats of LDS per workgroup (16 KiB); a multiple of 4: column pieces start on a Philox group
constexpr uint32_t JT_ROW_MAX = JT_TILE / 4;         // longer rows are cut into column pieces (four whole rows no longer fit)
constexpr uint32_t JT_MAX_T1 = 1u << 26;             // (j >> 2) has 24 bits of the counter

struct JitterArgs {
    uint64_t *state;
    float *out[SN_MAX_STAGES];                       // NULL: the stage has no tiles
    uint32_t T1[SN_MAX_STAGES];                      // row length
    uint32_t rows[SN_MAX_STAGES];                    // rows per tile (whole-row tiles); 1 with column pieces
    uint32_t pieces[SN_MAX_STAGES];                  // column pieces per row (1: whole rows)
    uint32_t tile_end[SN_MAX_STAGES];                // first workgroup past the stage's tiles
    uint32_t N, ray_base, num_stages;
};

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
        const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
        k0 += W0; k1 += W1;
    }
}

__global__ __launch_bounds__(256) void k_jitter_tables(const JitterArgs a) {
    SN_POISON_ALL();
    __shared__ __align__(16) float s_tile[JT_TILE];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint64_t seed = a.state[0], draw = a.state[1];             // (nobody writes them during this launch)
    uint32_t k = 0, first = 0;
    while (k + 1u < a.num_stages && b >= a.tile_end[k]) { first = a.tile_end[k]; ++k; }      // (the grid is the tiles: b < tile_end[num_stages - 1])
    const uint32_t T1 = a.T1[k], t = b - first, pieces = a.pieces[k];
    uint32_t r0, nrows, j0, cw;
    if (pieces == 1u) { r0 = t * a.rows[k]; nrows = umin(a.rows[k], a.N - r0); j0 = 0u; cw = T1; }
    else { r0 = t / pieces; nrows = 1u; j0 = (t - r0 * pieces) * JT_TILE; cw = umin(JT_TILE, T1 - j0); }
    const uint32_t gw = (cw + 3u) >> 2, groups = nrows * gw, kind = k == 0u ? 0 : 1;
    for (uint32_t idx = tid; idx < groups; idx += JT_THREADS) {
        const uint32_t rl = idx / gw, q = idx - rl * gw, j = j0 + 4u * q;
        uint32_t c[4] = {a.ray_base + r0 + rl, (k << 24) | (j >> 2), (uint32_t)draw, (uint32_t)(draw >> 32)};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        float *s = s_tile + rl * cw + 4u * q;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (4u * q + e < cw) s[e] = jitter_value(true, (float)(c[e] >> 8) * 5.9604644775390625e-08f, T1, j + e, (int)kind);
    }
    __syncthreads();
    const uint32_t len = nrows * cw;                             // <= JT_TILE
    float *dst = a.out[k] + ((size_t)r0 * T1 + j0);
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {
        const uint32_t quads = len >> 2;
        for (uint32_t i = tid; i < quads; i += JT_THREADS) reinterpret_cast<float4 *>(dst)[i] = reinterpret_cast<const float4 *>(s_tile)[i];
        const uint32_t i = (quads << 2) + tid;
        if (i < len) dst[i] = s_tile[i];
    } else {
        for (uint32_t i = tid; i < len; i += JT_THREADS) dst[i] = s_tile[i];
    }
}

// draw + 1, behind k_jitter_tables on the same stream: every workgroup of that launch has read the state
__global__ void k_jitter_advance(uint64_t *state) { state[1] = state[1] + 1ull; }

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_jitter_tables(uint64_t *state, uint32_t N, uint32_t ray_base, uint32_t num_stages, const uint32_t *num_steps, float *bins0, float *const *u,
                        int32_t advance, sn_stream_t stream) {
    if (N == 0) return SN_OK;
    SN_REQUIRE(state, "jitter_tables: NULL state");
    SN_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15u) == 0, "jitter_tables: the state must be 16-byte aligned");
    SN_REQUIRE(num_stages >= 1 && num_stages <= SN_MAX_STAGES, "jitter_tables: num_stages=%u outside 1..%d", num_stages, SN_MAX_STAGES);
    SN_REQUIRE(num_steps, "jitter_tables: NULL num_steps");
    SN_REQUIRE((uint64_t)ray_base + N <= (1ull << 32), "jitter_tables: ray_base + N = %llu rays do not fit the 32-bit ray counter",
               (unsigned long long)ray_base + N);
    JitterArgs a = {};
    a.state = state; a.N = N; a.ray_base = ray_base; a.num_stages = num_stages;
    uint64_t tiles = 0;
    for (uint32_t k = 0; k < num_stages; ++k) {
        SN_REQUIRE(num_steps[k] >= 1 && num_steps[k] < JT_MAX_T1, "jitter_tables: num_steps[%u] = %u outside 1 .. 2^26 - 1 (rows of at most 2^26 values)",
                   k, num_steps[k]);
        const uint32_t T1 = num_steps[k] + 1u;
        a.T1[k] = T1;
        a.out[k] = k == 0 ? bins0 : (u ? u[k] : nullptr);
        if (T1 <= JT_ROW_MAX) { a.rows[k] = (JT_TILE / T1) & ~3u; a.pieces[k] = 1u; }
        else { a.rows[k] = 1u; a.pieces[k] = div_up(T1, JT_TILE); }
        if (a.out[k]) {
            SN_REQUIRE((reinterpret_cast<uintptr_t>(a.out[k]) & 3u) == 0, "jitter_tables: the table of stage %u is not 4-byte aligned", k);
            tiles += a.pieces[k] == 1u ? div_up(N, a.rows[k]) : (uint64_t)N * a.pieces[k];
        }
        SN_UNSUPPORTED(tiles < (1ull << 31), "jitter_tables: N=%u rows of %u values need more than 2^31 workgroups", N, T1);
        a.tile_end[k] = (uint32_t)tiles;
    }
    if (tiles) {                                                     // (no table asked for: the call only advances the draw)
        hipLaunchKernelGGL(k_jitter_tables, dim3((uint32_t)tiles), dim3(JT_THREADS), 0, (hipStream_t)stream, a);
        SN_LAUNCH_CHECK("k_jitter_tables");
    }
    if (advance) {
        hipLaunchKernelGGL(k_jitter_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
        SN_LAUNCH_CHECK("k_jitter_advance");
    }
    return SN_OK;
}

}  // extern "C"
