// render_mfma.h -- fused renderer: the last stage's 32->64->64->16 MLP on the matrix cores.  Weight packing (k_pack_grid_mlp*), the matrix phase in its
// exact-fp32 and split-fp16 forms up to grid_mlp_mfma16_l12_spread, and the vector-ALU fallback.
#ifndef SN_RENDER_MFMA_H
#define SN_RENDER_MFMA_H
#include "render_gather.h"
#include "render_dense.h"

namespace sn {

// A-operand packing for the 32->64->64->16 MLP on v_mfma_f32_32x32x2_f32.
//   D[m][j] += sum_k A[m][k] * B[k][j],  A = weights (m = output neuron), B = activations
//   (j = sample).  Lane l supplies A[m = l&31][k = l>>5] and B[k = l>>5][j = l&31]; the
//   accumulator register r of lane l holds D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
//   Because that accumulator layout IS a valid B-operand layout (low half-wave: row h0(r),
//   high half-wave: row h0(r)+4), layer n+1 consumes layer n's accumulators in place; only
//   the weights are permuted, once, here.
constexpr int PACK_L1 = 0;                       // [mt 2][step 16][64]
constexpr int PACK_L2 = PACK_L1 + 2 * 16 * 64;   // [mt 2][step 32][64]
constexpr int PACK_L3 = PACK_L2 + 2 * 32 * 64;   // [step 32][64]
constexpr int PACK_FLOATS = PACK_L3 + 32 * 64;   // 8192 floats = 32 KiB

__global__ void k_pack_grid_mlp(const float *__restrict__ w1, const float *__restrict__ w2, const float *__restrict__ w3,
                                float *__restrict__ pack) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint32_t)PACK_FLOATS) return;
    const uint32_t lane = t & 63u, vec = t >> 6;
    const uint32_t m = lane & 31u, hi = lane >> 5;
    float v;
    if (vec < 32u) {                       // layer 1: in 32 -> out 64
        const uint32_t mt = vec >> 4, s = vec & 15u;
        v = w1[(mt * 32u + m) * 32u + 2u * s + hi];
    } else if (vec < 96u) {                // layer 2: in 64 -> out 64
        const uint32_t q = vec - 32u, mt = q >> 5, s = q & 31u, src_mt = s >> 4, r = s & 15u;
        const uint32_t h = src_mt * 32u + (r & 3u) + 8u * (r >> 2) + 4u * hi;
        v = w2[(mt * 32u + m) * 64u + h];
    } else {                               // layer 3: in 64 -> out 16 (rows 16..31 are zero padding)
        const uint32_t s = vec - 96u, src_mt = s >> 4, r = s & 15u;
        const uint32_t h = src_mt * 32u + (r & 3u) + 8u * (r >> 2) + 4u * hi;
        v = m < 16u ? w3[m * 64u + h] : 0.0f;
    }
    pack[t] = v;
}


// max(t, 0) of matrix-core results, one IEEE maximum each (relu_ieee: -0 -> +0, a NaN of either sign stays NaN like torch.relu).
// fmaxf would cost two instructions there: the compiler cannot prove an MFMA output canonical and puts a v_max_f32 t, t, t in front of
// every v_max_f32 0, t; the maximum needs no canonical input.
__device__ __forceinline__ floatx16 relu16(floatx16 v) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = relu_ieee(v[i]);
    return v;
}

// 32 -> 64 -> 64 -> 16 for the wave's 64 samples (lane = sample).
// Features arrive through the wave's LDS slab fe[k][lane] (written by encode_levels_lds), which
// is already a B-operand image: step s of sample tile t reads fe[2s + (lane>>5)][32t + (lane&31)].
__device__ __forceinline__ void grid_mlp_mfma(const float *__restrict__ lds_pack, const float *__restrict__ fe, float (&out)[16]) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = lane & 31u, hi = lane >> 5;
    float res[2][8];
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
        floatx16 h1[2], h2[2], o3;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 16; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_pack[PACK_L1 + (mt * 16 + s) * 64 + lane],
                                                           fe[(2 * s + hi) * 64 + tile * 32 + lo], acc, 0, 0, 0);
            h1[mt] = relu16(acc);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 32; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_pack[PACK_L2 + (mt * 32 + s) * 64 + lane], h1[s >> 4][s & 15], acc, 0, 0, 0);
            h2[mt] = relu16(acc);
        }
        {
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 32; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_pack[PACK_L3 + s * 64 + lane], h2[s >> 4][s & 15], acc, 0, 0, 0);
            o3 = acc;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) res[tile][r] = o3[r];
    }
    // bring every sample's 16 outputs to its own lane: accumulator reg r of tile t holds rows
    // base(r) [low half-wave] / base(r)+4 [high half-wave] of sample 32t + (lane&31)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        auto rr = __builtin_amdgcn_permlane32_swap(__float_as_uint(res[0][r]), __float_as_uint(res[1][r]), false, false);
        const int base = (r & 3) + 8 * (r >> 2);
        out[base] = __uint_as_float(rr[0]);
        out[base + 4] = __uint_as_float(rr[1]);
    }
}

// ------------------------------------------------------------------------------------------
// fp16 hi/lo split path of the same MLP (MLP_F16X3, the default).
// fp32 MFMA issues at the vector-ALU rate (64 cycles per 32x32x2), which made the matrix pipe the
// co-bound of the final stage.  Writing every operand as x = hi + lo with hi = f16(x),
// lo = f16(x - hi) (22 significant bits) and accumulating the three products hi*hi + hi*lo + lo*hi
// in fp32 on v_mfma_f32_32x32x16_f16 costs 3 x 32 cycles per 32x32x16 block instead of 8 x 64:
// 5.3x fewer matrix-pipe cycles at ~2^-22 relative error per product (f16 x f16 is exact in fp32;
// the dropped lo*lo term is 2^-22).  Range: |activation| must stay below 65504.
//   A operand (weights):     lane l holds W[m = l&31][k = 8*(l>>5) + 0..7] of the k-step
//   B operand (activations): lane l holds X[k = 8*(l>>5) + 0..7][j = l&31]
//   C/D layout as for every 32x32 MFMA: reg r of lane l = D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]
// so 8 consecutive accumulator registers of a lane are a valid B operand of the next layer
// (low half-wave rows {0-3, 8-11} / high half-wave rows {4-7, 12-15} of that 16-row block); only
// the weights' k order is permuted, once, by k_pack_grid_mlp_f16.
// ------------------------------------------------------------------------------------------
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
constexpr int PACK16_VECS = 4 + 8 + 4;                 // layer1 [mt 2][s 2], layer2 [mt 2][q 4], layer3 [q 4]
constexpr int PACK16_U4 = PACK16_VECS * 2 * 64;        // x (hi, lo) x 64 lanes, 16 B each = 32 KiB
constexpr int SLAB_STRIDE = 20;                        // dwords per sample row (16 levels + 4 pad: conflict-free b128 reads)

__device__ __forceinline__ void split2(float a, float b, uint32_t &hi, uint32_t &lo) {
    const half2_t h = {(_Float16)a, (_Float16)b};
    hi = __builtin_bit_cast(uint32_t, h);
    // x - hi (exact in fp32: hi is x rounded to 11 bits) straight from the packed halves with the mixed-precision fma:
    // v_fma_mix_f32 widens its f16 operand for free, where the compiler's form was two v_cvt_f32_f16 + one v_pk_add_f32
    // (5 -> 4 instructions per pair, 80 pairs per sample in the final stage)
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hi), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hi), "v"(b));
    const half2_t l = {(_Float16)l0, (_Float16)l1};
    lo = __builtin_bit_cast(uint32_t, l);
}

__global__ void k_pack_grid_mlp_f16(const float *__restrict__ w1, const float *__restrict__ w2, const float *__restrict__ w3,
                                    uint4 *__restrict__ pack) {
    SN_POISON_ALL();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;        // one thread per (vec, lane)
    if (t >= (uint32_t)PACK16_VECS * 64u) return;
    const uint32_t lane = t & 63u, vec = t >> 6;
    const uint32_t m = lane & 31u, hi = lane >> 5;
    float v[8];
    if (vec < 4u) {                       // layer 1: k = 16 s + 8 hi + i  (feature 2*level + c)
        const uint32_t mt = vec >> 1, sst = vec & 1u;
        for (uint32_t i = 0; i < 8; ++i) v[i] = w1[(mt * 32u + m) * 32u + 16u * sst + 8u * hi + i];
    } else {
        const bool l3 = vec >= 12u;
        const uint32_t q = l3 ? vec - 12u : (vec - 4u) & 3u, mt = l3 ? 0u : (vec - 4u) >> 2;
        const uint32_t src_mt = q >> 1, half = q & 1u;
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t r = 8u * half + i;
            const uint32_t h = src_mt * 32u + (r & 3u) + 8u * (r >> 2) + 4u * hi;
            v[i] = l3 ? (m < 16u ? w3[m * 64u + h] : 0.0f) : w2[(mt * 32u + m) * 64u + h];
        }
    }
    uint4 ph, pl;
    split2(v[0], v[1], ph.x, pl.x); split2(v[2], v[3], ph.y, pl.y);
    split2(v[4], v[5], ph.z, pl.z); split2(v[6], v[7], ph.w, pl.w);
    pack[(vec * 2u + 0u) * 64u + lane] = ph;
    pack[(vec * 2u + 1u) * 64u + lane] = pl;
}

__device__ __forceinline__ floatx16 mfma3(const uint4 &ah, const uint4 &al, const uint4 &bh, const uint4 &bl, floatx16 acc) {
    const half8_t Ah = __builtin_bit_cast(half8_t, ah), Al = __builtin_bit_cast(half8_t, al);
    const half8_t Bh = __builtin_bit_cast(half8_t, bh), Bl = __builtin_bit_cast(half8_t, bl);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc, 0, 0, 0);   // small terms first
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
    return acc;
}

// Reduced-product form of the split arithmetic (sn_render_tuning.mlp_mode = SN_MLP_F16X1; opt-in, NOT fp32-class, NOT within the 1e-4 bar):
//   NP = 3  Al*Bh + Ah*Bl + Ah*Bh   (the default: every product to 2^-22)
//   NP = 1  Ah*Bh                   plain fp16 operands with fp32 accumulation -- what an autocast fp16 run of the reference multiplies
// Measured in round 6 (profiles/r06/mlp_modes_ab.json): 800x800 [128] 6.19 -> 5.44 ms, and max |dRGB| against the reference's own output on
// the stress-init fixtures 3.2e-4 / 3.5e-4 (x3: 6e-7 / 7e-6) -- over the north star's 1e-4, so it can never be the default.  A two-product
// form (weights exact, activations rounded to fp16) was measured too: 1.9e-4 / 2.6e-4, i.e. over the bar as well, and dropped.
template <int NP>
__device__ __forceinline__ floatx16 mfma_np(const uint4 &ah, const uint4 &al, const uint4 &bh, const uint4 &bl, floatx16 acc) {
    if constexpr (NP == 3) return mfma3(ah, al, bh, bl, acc);
    const half8_t Ah = __builtin_bit_cast(half8_t, ah), Bh = __builtin_bit_cast(half8_t, bh);
    if constexpr (NP == 2) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, al), Bh, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
}
__device__ __forceinline__ uint32_t pack_h2(float a, float b) {
    const half2_t h = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, h);
}
// relu + fp16 rounding only (NP < 3: the lo image of an activation is never multiplied)
__device__ __forceinline__ void acc_to_b_hi(const floatx16 &v, int half, uint4 &bh) {
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = relu_ieee(v[8 * half + i]);
    bh.x = pack_h2(x[0], x[1]); bh.y = pack_h2(x[2], x[3]); bh.z = pack_h2(x[4], x[5]); bh.w = pack_h2(x[6], x[7]);
}

// relu + split of 8 consecutive accumulator registers -> (hi, lo) B operand of the next layer
__device__ __forceinline__ void acc_to_b(const floatx16 &v, int half, uint4 &bh, uint4 &bl) {
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = relu_ieee(v[8 * half + i]);
    split2(x[0], x[1], bh.x, bl.x); split2(x[2], x[3], bh.y, bl.y);
    split2(x[4], x[5], bh.z, bl.z); split2(x[6], x[7], bh.w, bl.w);
}

// slab_hi / slab_lo: this wave's [64 samples][SLAB_STRIDE dwords] images written by encode_levels_split
__device__ __forceinline__ void grid_mlp_mfma16(const uint4 *__restrict__ pk, const uint32_t *__restrict__ slab_hi,
                                                const uint32_t *__restrict__ slab_lo, float (&out)[16]) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = lane & 31u, hi = lane >> 5;
    float res[2][8];
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
        const uint32_t row = (tile * 32u + lo) * SLAB_STRIDE + 4u * hi;
        floatx16 h1[2], h2[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const uint4 bh = *reinterpret_cast<const uint4 *>(slab_hi + row + 8 * st);
                const uint4 bl = *reinterpret_cast<const uint4 *>(slab_lo + row + 8 * st);
                const int vec = mt * 2 + st;
                acc = mfma3(pk[(vec * 2 + 0) * 64 + lane], pk[(vec * 2 + 1) * 64 + lane], bh, bl, acc);
            }
            h1[mt] = acc;
            __builtin_amdgcn_sched_barrier(0);   // keep the next block's operand reads from being hoisted (VGPR pressure)
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint4 bh, bl;
                acc_to_b(h1[q >> 1], q & 1, bh, bl);
                const int vec = 4 + mt * 4 + q;
                acc = mfma3(pk[(vec * 2 + 0) * 64 + lane], pk[(vec * 2 + 1) * 64 + lane], bh, bl, acc);
            }
            h2[mt] = acc;
            __builtin_amdgcn_sched_barrier(0);
        }
        floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint4 bh, bl;
            acc_to_b(h2[q >> 1], q & 1, bh, bl);
            const int vec = 12 + q;
            acc = mfma3(pk[(vec * 2 + 0) * 64 + lane], pk[(vec * 2 + 1) * 64 + lane], bh, bl, acc);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) res[tile][r] = acc[r];
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        auto rr = __builtin_amdgcn_permlane32_swap(__float_as_uint(res[0][r]), __float_as_uint(res[1][r]), false, false);
        const int base = (r & 3) + 8 * (r >> 2);
        out[base] = __uint_as_float(rr[0]);
        out[base + 4] = __uint_as_float(rr[1]);
    }
}

// The same MLP with BOTH 32-sample tiles of the wave advancing together: every weight operand is read from LDS once per
// wave-sample instead of once per tile (64 -> 32 ds_read_b128 of 1 KiB; the weight stream was 12 % of the final stage:
// timing with the reads removed, profiles/r03/ab_round3_experiments.txt) and the matrix pipe always has two to four
// independent accumulators in flight.  Every accumulator still receives exactly the same sequence of products (k-steps
// ascending, small terms first), so the results are bit-identical to grid_mlp_mfma16.  Costs 64 more live registers at
// the layer-2 peak (both tiles' h1 and all four layer-2 accumulators), paid for with a shorter prefetched gather span.
__device__ __forceinline__ void grid_mlp_mfma16_2t(const uint4 *__restrict__ pk, const uint32_t *__restrict__ slab_hi,
                                                   const uint32_t *__restrict__ slab_lo, float (&out)[16]) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = lane & 31u, hi = lane >> 5;
    const floatx16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    floatx16 h1[2][2];                                    // [tile][mt]
#pragma unroll
    for (int t = 0; t < 2; ++t) { h1[t][0] = zero16; h1[t][1] = zero16; }
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        uint4 bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t row = (t * 32u + lo) * SLAB_STRIDE + 4u * hi + 8u * st;
            bh[t] = *reinterpret_cast<const uint4 *>(slab_hi + row);
            bl[t] = *reinterpret_cast<const uint4 *>(slab_lo + row);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int vec = mt * 2 + st;
            const uint4 ah = pk[(vec * 2 + 0) * 64 + lane], al = pk[(vec * 2 + 1) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 2; ++t) h1[t][mt] = mfma3(ah, al, bh[t], bl[t], h1[t][mt]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    floatx16 h2[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) { h2[t][0] = zero16; h2[t][1] = zero16; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint4 bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) acc_to_b(h1[t][q >> 1], q & 1, bh[t], bl[t]);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int vec = 4 + mt * 4 + q;
            const uint4 ah = pk[(vec * 2 + 0) * 64 + lane], al = pk[(vec * 2 + 1) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 2; ++t) h2[t][mt] = mfma3(ah, al, bh[t], bl[t], h2[t][mt]);
        }
        __builtin_amdgcn_sched_barrier(0);                // one k-step at a time: h1 dies in halves behind this loop
    }
    floatx16 o3[2] = {zero16, zero16};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint4 bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) acc_to_b(h2[t][q >> 1], q & 1, bh[t], bl[t]);
        const int vec = 12 + q;
        const uint4 ah = pk[(vec * 2 + 0) * 64 + lane], al = pk[(vec * 2 + 1) * 64 + lane];
#pragma unroll
        for (int t = 0; t < 2; ++t) o3[t] = mfma3(ah, al, bh[t], bl[t], o3[t]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        auto rr = __builtin_amdgcn_permlane32_swap(__float_as_uint(o3[0][r]), __float_as_uint(o3[1][r]), false, false);
        const int base = (r & 3) + 8 * (r >> 2);
        out[base] = __uint_as_float(rr[0]);
        out[base + 4] = __uint_as_float(rr[1]);
    }
}

// Slab row addressing.  Padded form: 20 dwords per sample row.  Swizzled form (SW): 16 dwords per row, the four 16-byte blocks
// of a row XOR-ed with (row >> 2) & 3 -- conflict-free for the ds_read_b128 of the B operands without the 4 padding dwords,
// which frees 8 KiB per workgroup for the LDS-resident coarse level below.
template <bool SW>
__device__ __forceinline__ uint32_t slab_dword(uint32_t row, uint32_t d) {
    if constexpr (SW) return row * 16u + ((((d >> 2) ^ (row >> 2)) & 3u) << 2) + (d & 3u);
    else return row * (uint32_t)SLAB_STRIDE + d;
}

// LDS-resident level 0 (north_star: "LDS staging of per-tile grid voxels"; the reference's only gesture at table locality is its
// level-major launch, gridencoder.cu:383-399).  The coarsest level of the main grid is 16^3 vertices = 16 KiB of fp16 rows: every
// workgroup stages it once and its 2 x 128 samples per lane read their 8 corners with ds_read_b32 instead of two 16-byte gathers
// through the texture path (98 -> 96 gather instructions per wave-sample).  Arithmetic as issue_level_lv's dense branch.
[[maybe_unused]] constexpr int L0_MAX_ROWS = 4096;   // (used by experiments builds only)
template <int l>
__device__ __forceinline__ void issue_level0_lds(const FinalLv &lv, const uint32_t *__restrict__ l0tab, const float (&x01)[3], float (&pos)[3],
                                                 Corner<__half, 2> (&cv)[8]) {
    static_assert(l == 0, "level 0 only");
    const float rf = lv.res_f[0];
    uint32_t cell[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float p = __builtin_fmaf(x01[d], rf, -0.5f);
        p = __builtin_amdgcn_fmed3f(p, 0.0f, lv.top_f[0]);
        cell[d] = (uint32_t)p;
        pos[d] = __builtin_amdgcn_fractf(p);
    }
    // vertex index in dwords: x + res * y + res^2 * z (the quad-row strides of FinalLv are 16 bytes per vertex: >> 4)
    const uint32_t sy = lv.d_sy[0] >> 4, sz = lv.d_sz[0] >> 4, top = (uint32_t)lv.top_f[0];
    const uint32_t X0 = cell[0], X1 = umin(X0 + 1u, top);
    const uint32_t Y0 = __umul24(cell[1], sy), Y1 = umin(Y0 + sy, lv.d_ylim[0] >> 4);
    const uint32_t Z0 = __umul24(cell[2], sz), Z1 = umin(Z0 + sz, lv.d_zlim[0] >> 4);
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        corner_set_half2(cv[i], l0tab[((i & 1u) ? X1 : X0) + ((i & 2u) ? Y1 : Y0) + ((i & 4u) ? Z1 : Z0)]);
    }
}

// "Linear tail" form of the final stage (k_final_stage<..., LT = true>).  The third layer has no activation behind it and the
// compositing is linear in what it produces, so for the 15 geometry channels
//     sum_j w_j * (W3[1:16] relu(h2_j))  =  W3[1:16] * (sum_j w_j relu(h2_j)),
// (renderer.py:332-336 composites `color`, network.py:175-186 forms it from grid_mlp's outputs 1..15): only the density row of
// the third layer is needed per sample -- one 64-term dot product, in true fp32 on the vector ALU -- while the geometry rows are
// applied ONCE per ray to the weight-accumulated hidden vector.  That takes the third layer off the matrix cores: 72 instead
// of 96 MFMAs per wave-sample and 48 instead of 64 KiB of LDS weight reads, which matters because the kernel runs at the
// clock the power management allows (the matrix-core MLP costs ~4 % in cycles and ~14 % in clock).
// A documented re-association like SH(d) * sum_j w_j; fp32 round-off class, not bit-identical to the
// per-sample form the other final-stage kernels (and per-sample geometry outputs) keep.
//
// layers 1 and 2 of ONE tile (32 samples): x[mt * 16 + r] = relu(h2) of hidden row mt*32 + (r&3) + 8*(r>>2) + 4*(lane>>5)
template <bool SW = false, int NP = 3>
__device__ __forceinline__ void grid_mlp_mfma16_l12(const uint4 *__restrict__ pk, const uint32_t *__restrict__ slab_hi,
                                                    const uint32_t *__restrict__ slab_lo, int tile, float (&x)[32]) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = lane & 31u, hi = lane >> 5;
    const uint32_t srow = (uint32_t)tile * 32u + lo;
    floatx16 h1[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const uint32_t off = slab_dword<SW>(srow, 4u * hi + 8u * (uint32_t)st);
            const uint4 bh = *reinterpret_cast<const uint4 *>(slab_hi + off);
            uint4 bl = bh;
            if constexpr (NP == 3) bl = *reinterpret_cast<const uint4 *>(slab_lo + off);
            const int vec = mt * 2 + st;
            const uint4 ah = pk[(vec * 2 + 0) * 64 + lane];
            uint4 al = ah;
            if constexpr (NP >= 2) al = pk[(vec * 2 + 1) * 64 + lane];
            acc = mfma_np<NP>(ah, al, bh, bl, acc);
        }
        h1[mt] = acc;
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint4 bh, bl;
            if constexpr (NP == 3) acc_to_b(h1[q >> 1], q & 1, bh, bl);
            else { acc_to_b_hi(h1[q >> 1], q & 1, bh); bl = bh; }
            const int vec = 4 + mt * 4 + q;
            const uint4 ah = pk[(vec * 2 + 0) * 64 + lane];
            uint4 al = ah;
            if constexpr (NP >= 2) al = pk[(vec * 2 + 1) * 64 + lane];
            acc = mfma_np<NP>(ah, al, bh, bl, acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) x[mt * 16 + r] = relu_ieee(acc[r]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// W3 re-ordered for the linear tail: w3p[half][o][i] = W3[o][mt*32 + (r&3) + 8*(r>>2) + 4*half], i = mt*16 + r -- the hidden
// rows a lane of that half-wave holds, in its register order (o = 0: density row, 1..15: geometry rows)
constexpr int W3P_FLOATS = 2 * 16 * 32;
constexpr int W3P_OFFSET = (12 * 2) * 64 * 4;            // floats: the packed layer-3 operands' place in the LDS weight image (unused here)
static_assert(W3P_OFFSET + W3P_FLOATS <= PACK_FLOATS, "the re-ordered W3 fits where the packed layer-3 operands were");
__device__ __forceinline__ void stage_w3p(float *__restrict__ dst, const float *__restrict__ w3) {
    for (uint32_t t = threadIdx.x; t < (uint32_t)W3P_FLOATS; t += blockDim.x) {
        const uint32_t i = t & 31u, o = (t >> 5) & 15u, half = t >> 9;
        const uint32_t mt = i >> 4, r = i & 15u;
        dst[t] = w3[o * 64u + mt * 32u + (r & 3u) + 8u * (r >> 2) + 4u * half];
    }
}
// sum_i w[i] * x[i] over the lane's 32 hidden rows: four interleaved ascending fmaf chains, combined (s0 + s1) + (s2 + s3)
typedef float f2v __attribute__((ext_vector_type(2)));
// (one step of the four chains and their closing sum stand alone: the spread matrix phase below issues them apart, in the same order)
__device__ __forceinline__ void dot32_step(const float4 &ww, float x0, float x1, float x2, float x3, f2v &s01, f2v &s23) {
    s01 = __builtin_elementwise_fma(f2v{ww.x, ww.y}, f2v{x0, x1}, s01);
    s23 = __builtin_elementwise_fma(f2v{ww.z, ww.w}, f2v{x2, x3}, s23);
}
__device__ __forceinline__ float dot32_sum(const f2v &s01, const f2v &s23) { return (s01.x + s01.y) + (s23.x + s23.y); }
__device__ __forceinline__ float dot32_lds(const float *__restrict__ w, const float (&x)[32]) {
    f2v s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f};
#pragma unroll
    for (int i4 = 0; i4 < 8; ++i4) {
        const float4 ww = *reinterpret_cast<const float4 *>(w + 4 * i4);
        dot32_step(ww, x[4 * i4 + 0], x[4 * i4 + 1], x[4 * i4 + 2], x[4 * i4 + 3], s01, s23);
    }
    return dot32_sum(s01, s23);
}

// The matrix phase of one wave-sample in the linear-tail kernel -- layers 1 and 2 of BOTH tiles and each tile's share of the density row --
// with its vector work issued UNDER its MFMAs.  grid_mlp_mfma16_l12 + dot32_lds above issue the same instructions in clumps: the 12 layer-1
// MFMAs of a tile back to back with empty gaps, then ReLU + split blocks with the matrix pipe idle, every weight fragment requested right
// in front of the wait that consumes it.  An MFMA of this shape holds the SIMD's vector issue for 8 of its 32 cycles, so about five vector
// instructions per gap are (nearly) free and a clump is paid in full.  Here every gap between two MFMAs is one scheduling region (closed
// by a sched_barrier) that holds what the table below puts there, one "piece" of about six vector instructions at a time:
//   W(s)      the (hi, lo) weight fragment of step s is requested under step s - 1: lo behind its first MFMA (the only one that reads a lo
//             image), hi behind its last -- each into registers that have just died, so the prefetch costs none (the waits are counted:
//             later requests are in flight behind it)
//   S(q, p)   ReLU + split of one register pair of h1 -> dword p of the layer-2 B operand q:  q = 0, 1 under the layer-1 mt = 1 chain,
//             q = 2, 3 under the first layer-2 steps; each is complete one gap before the MFMA that reads it
//   X(i4)     ReLU of four h2 registers + their step of the density dot: the mt = 0 half under the layer-2 mt = 1 chain, the mt = 1 half
//             of tile 0 under tile 1's layer-1 chain (tile 1's own is the tail of the phase)
//   B(t + 1)  tile 1's slab rows are requested under tile 0's layer 2, when the registers of tile 0's rows are free again
// Every accumulator receives the products of its chain in the order of grid_mlp_mfma16_l12 (Al Bh, Ah Bl, Ah Bh; k ascending) and the
// dot keeps dot32_lds's four chains: the results are equal bit for bit (tests/test_gpu_final_matrix_phase.py holds the two orders together).
template <bool SW>
__device__ __forceinline__ void grid_mlp_mfma16_l12_spread(const uint4 *__restrict__ pk, const uint32_t *__restrict__ slab_hi,
                                                           const uint32_t *__restrict__ slab_lo, const float *__restrict__ w3,
                                                           float (&xh)[2][32], float (&part)[2]) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = lane & 31u, hi = lane >> 5;
    const floatx16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint4 W[2][2];                  // [step & 1][0 = hi image, 1 = lo image]
    uint4 B[2][2];                  // layer-1 B operand: [st][hi, lo]
    uint32_t bb[4][2][4];           // layer-2 B operands: [q][hi, lo][dword]
    floatx16 h1[2], h2[2][2];       // h2[tile][mt]
    float4 ww[2][8];                // [tile][i4]: rows of the density row, requested a gap or two ahead of their step
    f2v s01[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, s23[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    // tile 1 reads the weights tile 0 read: behind an offset of its own, or the optimiser keeps all 24 fragments of tile 0 in registers for it
    const uint32_t oz1 = opaque_zero();
    const uint4 *const pkT[2] = {pk, pk + oz1};
    const float *const w3T[2] = {w3, w3 + oz1};
    auto rdW = [&](int S, int im) { W[S & 1][im] = pkT[S / 12][((S % 12) * 2 + im) * 64 + lane]; };
    auto rdB = [&](int t, int st, int im) {
        const uint32_t off = slab_dword<SW>((uint32_t)t * 32u + lo, 4u * hi + 8u * (uint32_t)st);
        B[st][im] = *reinterpret_cast<const uint4 *>((im ? slab_lo : slab_hi) + off);
    };
    auto rdw3 = [&](int t, int i4) { ww[t][i4] = *reinterpret_cast<const float4 *>(w3T[t] + 4 * i4); };
    auto S_ = [&](int q, int p) {
        const floatx16 &v = h1[q >> 1];
        const int i = 8 * (q & 1) + 2 * p;
        split2(relu_ieee(v[i]), relu_ieee(v[i + 1]), bb[q][0][p], bb[q][1][p]);
    };
    auto X_ = [&](int t, int i4) {
        const floatx16 &v = h2[t][i4 >> 2];
        const int r = 4 * (i4 & 3);
        float (&x)[32] = xh[t];
        x[4 * i4 + 0] = relu_ieee(v[r + 0]); x[4 * i4 + 1] = relu_ieee(v[r + 1]);
        x[4 * i4 + 2] = relu_ieee(v[r + 2]); x[4 * i4 + 3] = relu_ieee(v[r + 3]);
        dot32_step(ww[t][i4], x[4 * i4 + 0], x[4 * i4 + 1], x[4 * i4 + 2], x[4 * i4 + 3], s01[t], s23[t]);
    };
    // head: what the first MFMA reads first
    rdW(0, 1); rdB(0, 0, 0); rdW(0, 0); rdB(0, 0, 1); rdB(0, 1, 0); rdB(0, 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, 2>([&](auto tt) {
        constexpr int t = decltype(tt)::value;
        static_for<0, 36>([&](auto mm) {
            constexpr int m = decltype(mm)::value, s = m / 3, k = m % 3, S = 12 * t + s;
            // ---- MFMA m of the tile: product k of step s ----
            uint4 bh, bl;
            if constexpr (s < 4) { bh = B[s & 1][0]; bl = B[s & 1][1]; }
            else {
                constexpr int q = s & 3;
                bh = uint4{bb[q][0][0], bb[q][0][1], bb[q][0][2], bb[q][0][3]};
                bl = uint4{bb[q][1][0], bb[q][1][1], bb[q][1][2], bb[q][1][3]};
            }
            floatx16 &acc = s < 4 ? h1[(s >> 1) & 1] : h2[t][s < 4 ? 0 : (s - 4) >> 2];
            if constexpr (k == 0 && (s == 0 || s == 2 || s == 4 || s == 8)) acc = zero16;
            const half8_t Ah = __builtin_bit_cast(half8_t, W[S & 1][0]), Al = __builtin_bit_cast(half8_t, W[S & 1][1]);
            const half8_t Bh = __builtin_bit_cast(half8_t, bh), Bl = __builtin_bit_cast(half8_t, bl);
            if constexpr (k == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc, 0, 0, 0);   // small terms first (mfma3)
            if constexpr (k == 1) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc, 0, 0, 0);
            if constexpr (k == 2) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
            // ---- the gap behind it ----
            if constexpr (k == 0 && S + 1 < 24) rdW(S + 1, 1);       // the lo image was read by product 0 only: its registers take the next step's
            if constexpr (k == 2 && S + 1 < 24) rdW(S + 1, 0);       // and the hi image's behind the step's last product
            if constexpr (t == 1) {           // tile 0's tail
                if constexpr (m == 0) { X_(0, 4); rdw3(0, 5); }
                if constexpr (m == 1) { rdw3(0, 6); rdw3(0, 7); }
                if constexpr (m == 3) X_(0, 5);
                if constexpr (m == 4) X_(0, 6);
                if constexpr (m == 5) { X_(0, 7); part[0] = dot32_sum(s01[0], s23[0]); }
            }
            if constexpr (m >= 6 && m < 14) S_((m - 6) >> 2, (m - 6) & 3);
            if constexpr (m == 14) S_(2, 0);
            if constexpr (m == 15) S_(2, 1);
            if constexpr (m == 16) { S_(2, 2); S_(2, 3); }
            if constexpr (m == 17) S_(3, 0);
            if constexpr (m == 18) S_(3, 1);
            if constexpr (m == 19) { S_(3, 2); S_(3, 3); }
            if constexpr (t == 0) {           // tile 1's slab rows, into the registers the layer-2 operands q = 0..2 leave behind
                if constexpr (m == 30) rdB(1, 0, 0);
                if constexpr (m == 32) rdB(1, 0, 1);
                if constexpr (m == 33) rdB(1, 1, 0);
                if constexpr (m == 34) rdB(1, 1, 1);
            }
            if constexpr (m == 24) rdw3(t, 0);
            if constexpr (m == 26) rdw3(t, 1);
            if constexpr (m == 28) rdw3(t, 2);
            if constexpr (m == 30) rdw3(t, 3);
            if constexpr (m == 32) rdw3(t, 4);
            if constexpr (m == 26) X_(t, 0);
            if constexpr (m == 28) X_(t, 1);
            if constexpr (m == 30) X_(t, 2);
            if constexpr (m == 32) X_(t, 3);
            if constexpr (t == 1) {           // the rows of the tail, while the last MFMAs run (no tile follows: the slab-row registers are free)
                if constexpr (m == 33) rdw3(1, 5);
                if constexpr (m == 34) rdw3(1, 6);
                if constexpr (m == 35) rdw3(1, 7);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    });
    // tail: tile 1's mt = 1 half
    X_(1, 4); X_(1, 5); X_(1, 6); X_(1, 7);
    part[1] = dot32_sum(s01[1], s23[1]);
}

// hash-grid features of one position, split into f16 hi / lo and written to this lane's slab rows
// (dword l = the level's two features as a half2).
template <typename T, int L, int GROUP, int K>
__device__ __forceinline__ void encode_levels_split(const T *__restrict__ table, const GridLevels &g, const float (&x01)[3],
                                                    uint32_t *__restrict__ row_hi, uint32_t *__restrict__ row_lo) {
    const bool oob = encode_grouped<T, L, 2, GROUP, K, false>(table, g, x01, [&](int l, const float (&acc)[2]) {
        uint32_t ph, pl;
        split2(acc[0], acc[1], ph, pl);
        row_hi[l] = ph;
        row_lo[l] = pl;
    });
    if (__builtin_expect(__any(oob), 0)) {
        if (oob) for (int l = 0; l < L; ++l) { row_hi[l] = 0u; row_lo[l] = 0u; }
    }
}

// Scalar-pipe fallback of the same MLP (SN_RENDER_MLP=valu): activations live in per-thread LDS
// columns act[k][tid]; every neuron is one k-ascending fmaf chain (the oracle's order).
template <int IN, int OUT, int ACT>
__device__ __forceinline__ void dense_lds(const float *__restrict__ W, const float *__restrict__ xin, float *__restrict__ yout, uint32_t stride) {
    float x[IN];
#pragma unroll
    for (int k = 0; k < IN; ++k) x[k] = xin[k * stride];
#pragma unroll 1
    for (int o = 0; o < OUT; ++o) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < IN; ++k) acc = __builtin_fmaf(W[o * IN + k], x[k], acc);
        if (ACT == 1) acc = relu_ieee(acc);                  // ReLU as one v_maximum_f32 (a NaN stays NaN, as torch.relu)
        yout[o * stride] = acc;
    }
}

// hash-grid features of one position written to an LDS column fe[k * stride]
template <typename T, int L, int C, int GROUP, int K, bool PAIRX = false>
__device__ __forceinline__ void encode_levels_lds(const T *__restrict__ table, const GridLevels &g, const float (&x01)[3],
                                                  float *__restrict__ fe, uint32_t stride) {
    const bool oob = encode_grouped<T, L, C, GROUP, K, PAIRX>(table, g, x01, [&](int l, const float (&acc)[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) fe[(l * C + c) * stride] = acc[c];
    });
    if (__builtin_expect(__any(oob), 0)) {
        if (oob) for (int i = 0; i < L * C; ++i) fe[i * stride] = 0.0f;
    }
}

enum { MLP_VALU = 0, MLP_F32 = 1, MLP_F16X3 = 2 };

}  // namespace sn

#endif  // SN_RENDER_MFMA_H
