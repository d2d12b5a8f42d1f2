// mlp_f32.inc — training-time forward of a bias-free perceptron with 256-wide hidden layers in TRUE fp32 on the matrix cores
// (v_mfma_f32_32x32x2_f32), activation fused, every hidden output saved for the backward pass (sn_mlp_wide_forward_train).
// Included by mlp.hip inside namespace sn.
//
// What it replaces: F.linear + leaky_relu per layer (reference nerf/network.py:31-66; the per-sample mask head in training,
// network.py:118-123, trainer.py:401-428).  Through BLAS that is one GEMM per layer (0.129 + 0.129 + 0.028 ms for the mask head's
// 131 072 x (143 -> 256 -> 256 -> 16) on MI355X: 62 % of the fp32 matrix peak) plus one elementwise pass over [N, 256] per hidden layer
// (2 x 0.039 ms).  Why fp32 and not the split-fp16 products of the render path: the backward pass takes the LeakyReLU branch from the sign
// of the saved output; a pre-activation rounded differently flips the branch of ~1e-6 of the units, which alone spends the 1e-3
// gradient budget (ops.py, _wide_mlp_train).  fp32 products and accumulation differ from BLAS only in summation order.
//
// Shape of the work: a workgroup (8 waves, two per SIMD) owns 64 rows and walks the layers.  D[row][n] = sum_k H[row][k] W[n][k]:
//   A operand  lane l supplies H[row = r0 + l%32][k + l/32]  from LDS, stored TRANSPOSED Ht[k][row] with a row stride of 65 words
//              (bank = (k + row) % 32: the 32 rows of a half-wave hit 32 banks; written from accumulators, lanes along n: also conflict-free)
//   B operand  lane l supplies W[n = n0 + l%32][k + l/32]     from LDS, a chunk of 32 k's stored [n][33]  (bank = (n + k) % 32)
//   wave (rh, cq) computes rows rh*32..+32 x column tiles 2 cq, 2 cq + 1 (2 accumulator tiles = 32 registers): 2 MFMAs (128 cycles) per
//              3 ds_read_b32 -- the LDS is nowhere near a limit, the matrix pipe is the bound (floor for the mask head: 0.177 ms)
// Weight chunks (256 x 32 floats = 32 KiB, rows of nn.Linear.weight as they lie in memory: no packing pass) stream through two LDS
// buffers: the next chunk's global loads are issued before a chunk's 64 MFMAs and parked in LDS after them; one barrier per chunk.
// A layer's epilogue applies the activation, stores the output row-major to global (lanes along n: 128-byte runs) and, for a hidden
// layer, writes it to Ht for the next layer.  LDS: 65 KiB (Ht, 256 x 65 words) + 2 x 33 KiB = 131 KiB: one workgroup per CU.

#ifndef SN_F32_EXP
#define SN_F32_EXP 0      // timing experiments (wrong results): 1 = no weight streaming, 2 = no MFMAs
#endif
constexpr int F32_ROWS = 64, F32_KC = 32, F32_HT_STRIDE = 65, F32_W_STRIDE = 33, F32_THREADS = 512;
constexpr size_t F32_LDS_BYTES = (size_t)(256 * F32_HT_STRIDE + 2 * 256 * F32_W_STRIDE) * sizeof(float);

struct F32Args {
    const float *x;                       // [n_rows, K0] row-major
    const float *w[SN_MAX_LAYERS];        // [N_l, K_l] row-major (nn.Linear.weight)
    float *h[SN_MAX_LAYERS];              // output of layer l: [n_rows, N_l] (hidden: post-activation; last: linear)
    uint32_t N[SN_MAX_LAYERS];
    uint32_t n_rows, K0, nl, leaky;
};

// 8 waves = TWO per SIMD: wave (rh, cq) computes rows rh*32..+32 x column tiles 2 cq, 2 cq + 1 (32 accumulator registers).
//
// MEASURED (round 5, profiles/r05/mlp_f32_trace.txt): 0.555 ms for 131 072 x (143 -> 256 -> 256 -> 16) = 50 TFLOP/s, against 0.377 ms for
// the three BLAS GEMMs + two activation kernels (74 TFLOP/s) -- so ops.py keeps the BLAS forward by default and this kernel is the tested
// opt-in (ops.WIDE_MLP_FORWARD_NATIVE).  Cycle trace per 32-k chunk: 7.0 k cycles against 4.1 k of matrix work; without the weight stream
// 5.0 k, the stream alone 2.2 k: the two do not overlap, and no arrangement made them -- one or two waves per SIMD, loads and parking
// interleaved with the MFMAs one per k-step behind scheduling barriers (7.6 k), requested two chunks ahead with explicit wait counters
// (8.3 k).  Reading: v_mfma_f32_32x32x2_f32 runs at exactly the packed-fp32 vector rate (64 FLOP / clk / SIMD) -- it occupies the vector
// ALUs, so the address arithmetic, selects and moves of the stream (~10 vector instructions per load) are not hidden under it the way
// they are under an fp16 MFMA (k_mask16).  What would be left to try: a stream with no vector instructions at all (LDS-DMA with a
// rotated layout instead of padding, addresses in scalar registers), persistent workgroups that fetch the next tile's rows under the last
// layer (a tile's start-up is 16 k of its ~125 k cycles).  Priced at 0.30 ms at best -- 0.08 ms under BLAS -- and not built.
__global__ __launch_bounds__(F32_THREADS, 1) void k_mlp_f32_train(F32Args a) {
    SN_POISON_ALL();
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    float *Ht = lds_f;                                         // [k][65]
    float *Wl = lds_f + 256 * F32_HT_STRIDE;                   // [2][256][33]
    const uint32_t tid = threadIdx.x, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u, lo = lane & 31u, hi = lane >> 5;
    const uint32_t rh = wave & 1u, cq = wave >> 1;
    const uint32_t row0 = blockIdx.x * F32_ROWS;

    // ---- the tile's input rows, transposed into Ht (k >= K0 up to the next multiple of 32: zeros) ----
    const uint32_t K0 = a.K0, K0p = (K0 + F32_KC - 1u) / F32_KC * F32_KC;
    wide_trace(0u);
    {   // (all of a thread's loads are issued before the first one is used: one memory latency per tile)
        float xv[8][4];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const uint32_t row = row0 + wave + 8u * i;
            const bool rv = row < a.n_rows;
            const float *src = a.x + (size_t)(rv ? row : 0u) * K0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t k = lane + 64u * j;
                const float v = src[k < K0 ? k : 0u];
                xv[i][j] = (rv && k < K0) ? v : 0.0f;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t k = lane + 64u * j;
                if (k < K0p) Ht[k * F32_HT_STRIDE + wave + 8u * i] = xv[i][j];
            }
    }

    // chunk c of a layer: weights W[n][c*32 .. c*32+32) for n < N (zeros beyond N and beyond K) -> registers -> Wl[buf]
    // element e = q * 512 + tid of the 256 x 32 chunk: n = e / 32, k = e % 32: a wave reads two 128-byte row pieces per instruction
    float wreg[16];
    auto load_chunk = [&](const float *__restrict__ W, uint32_t N, uint32_t K, uint32_t c) {
#pragma unroll
        for (uint32_t q = 0; q < 16u; ++q) {
            const uint32_t e = q * (uint32_t)F32_THREADS + tid, n = e >> 5, k = c * F32_KC + (e & 31u);
            const bool ok = n < N && k < K;
            const float v = W[ok ? (size_t)n * K + k : (size_t)0];
            wreg[q] = ok ? v : 0.0f;
        }
    };
    auto park_chunk = [&](uint32_t buf) {
        float *dst = Wl + buf * (256 * F32_W_STRIDE);
#pragma unroll
        for (uint32_t q = 0; q < 16u; ++q) {
            const uint32_t e = q * (uint32_t)F32_THREADS + tid;
            dst[(e >> 5) * F32_W_STRIDE + (e & 31u)] = wreg[q];
        }
    };

    uint32_t buf = 0, tslot = 2u;
    (void)tslot;
    wide_trace(1u);
    load_chunk(a.w[0], a.N[0], K0, 0u);
    park_chunk(0u);
    __syncthreads();
    wide_trace(tslot++);
    for (uint32_t l = 0; l < a.nl; ++l) {
        const uint32_t K = l == 0 ? K0 : 256u, N = a.N[l], nchunks = (K + F32_KC - 1u) / F32_KC;
        const uint32_t nt = (N + 31u) >> 5;                                   // column tiles of this layer
        const uint32_t my_tiles = nt > cq * 2u ? (nt - cq * 2u < 2u ? nt - cq * 2u : 2u) : 0u;
        floatx16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t] = floatx16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t c = 0; c < nchunks; ++c) {
            // the chunk after this one (the next layer's first chunk after the last): loads in flight under the MFMAs
            const bool last = c + 1u == nchunks, more = !last || l + 1u < a.nl;
#if !(SN_F32_EXP & 1)
            if (more) {
                if (!last) load_chunk(a.w[l], N, K, c + 1u);
                else load_chunk(a.w[l + 1u], a.N[l + 1u], 256u, 0u);
            }
#endif
            const float *wb = Wl + buf * (256 * F32_W_STRIDE) + (cq * 64u + lo) * F32_W_STRIDE + hi;
            const float *hb = Ht + (c * F32_KC + hi) * F32_HT_STRIDE + rh * 32u + lo;
#if SN_F32_EXP & 2
            if (false) {
#else
            if (my_tiles) {
#endif
                float av[F32_KC / 2], bv[F32_KC / 2][2];
#pragma unroll
                for (uint32_t s = 0; s < (uint32_t)F32_KC / 2u; ++s) {
                    av[s] = hb[2u * s * F32_HT_STRIDE];
#pragma unroll
                    for (int t = 0; t < 2; ++t) bv[s][t] = wb[t * 32 * F32_W_STRIDE + 2u * s];       // (a tile beyond N holds zero weights)
                }
                if (my_tiles == 2u) {
#pragma unroll
                    for (uint32_t s = 0; s < (uint32_t)F32_KC / 2u; ++s) {
#pragma unroll
                        for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s][t], acc[t], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (uint32_t s = 0; s < (uint32_t)F32_KC / 2u; ++s) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s][0], acc[0], 0, 0, 0);
                }
            }
#if !(SN_F32_EXP & 1)
            if (more) park_chunk(buf ^ 1u);
#endif
            __syncthreads();            // everyone is done with Wl[buf] (and, after the last chunk, with Ht); Wl[buf ^ 1] is complete
            buf ^= 1u;
            wide_trace(tslot++);
        }
        // ---- epilogue: activation, row-major store, and the next layer's operand ----
        const bool hidden = l + 1u < a.nl;
        float *out = a.h[l];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if ((uint32_t)t >= my_tiles) continue;
            const uint32_t n = (cq * 2u + (uint32_t)t) * 32u + lo;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t rr = rh * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;      // accumulator register r of lane l: D[(r&3) + 8 (r>>2) + 4 (l>>5)][l & 31]
                float v = acc[t][r];
                if (hidden) {
                    v = relu_or_leaky(v, a.leaky);
                    Ht[n * F32_HT_STRIDE + rr] = v;
                }
                if (row0 + rr < a.n_rows && n < N) out[(size_t)(row0 + rr) * N + n] = v;
            }
        }
        __syncthreads();
        wide_trace(tslot++);
    }
}
