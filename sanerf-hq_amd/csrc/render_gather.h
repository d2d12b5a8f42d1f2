// render_gather.h -- fused renderer: the hash-grid gathers.  Two-phase level groups, the x-swap and the parity order of the hashed levels,
// pair tables of the dense levels, encode_levels*, and the last stage's per-level constants (FinalLv) with its gather spans.
#ifndef SN_RENDER_GATHER_H
#define SN_RENDER_GATHER_H
#include "render_knobs.h"
#include "render_rays.h"

namespace sn {

// ---- two-phase level groups -----------------------------------------------------------------
// hipcc schedules "8 loads, wait, 16 fmas" level by level if the source is written level by level,
// which leaves 8 gathers in flight per lane and exposes one full memory latency per level.  The
// march therefore handles GROUP levels at a time in two explicit phases separated by scheduling
// barriers: (1) locate + row indices + ISSUE all GROUP*8 gathers (32-bit byte offsets from a
// wave-uniform base -> saddr-form global loads, one address VGPR each), (2) blend.
template <typename T, int C>
struct Corner { float v[C]; };

// fp16 tables, C = 2: a fetched row stays PACKED (its half2 bit pattern in v[0]) and the blend multiplies it with
// v_fma_mix_f32, which widens an f16 operand on the fly -- the same fp32 fma on the same exactly-converted value as
// v_cvt_f32_f16 + v_fma_f32, so results are bit-identical, but the 16 conversions per level (256 of ~1500 vector
// instructions per sample of the final stage, 80 of ~700 in a proposal stage) disappear.
template <typename T, int C>
__device__ __forceinline__ void corner_set_half2(Corner<T, C> &c, uint32_t bits) {
    static_assert(C == 2 && sizeof(T) == 2, "packed rows: fp16 tables with two features per level");
    c.v[0] = __uint_as_float(bits); c.v[1] = 0.0f;
}
__device__ __forceinline__ float fma_mix_lo(float w, uint32_t packed, float acc) {      // fmaf(w, (float)packed.lo, acc)
    float d;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(packed), "v"(acc));
    return d;
}
__device__ __forceinline__ float fma_mix_hi(float w, uint32_t packed, float acc) {      // fmaf(w, (float)packed.hi, acc)
    float d;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(packed), "v"(acc));
    return d;
}

// XSWAP (hashed fine levels of the final stage): the two x-corners of a cell sit in the same 128-byte line 15 times
// out of 16 (index = x ^ y*P1 ^ z*P2: x and x+1 differ in the low bits only), but as two instructions each line is
// looked up twice and a fine-level instruction already touches ~40 distinct lines (its cost).
// The half-waves therefore trade addresses with one v_permlane32_swap per corner pair: the first load serves BOTH
// x-corners of lanes 0-31, the second those of lanes 32-63 -- about half the distinct lines per instruction, same
// instruction count -- and blend_level_x swaps the fetched values back.
template <typename T, int KIND, int l>
constexpr bool xswap_level() {
    return KIND == 1 && l >= 0;
}
// PARITY (round 10, hashed levels of the FinalLv path): instruction (dy, dz) of a level used to fetch the corner (cell.y + dy, cell.z + dz),
// so two rays in y-adjacent cells asked for the hash row they share in two different instructions.  Instead every lane puts into
// instruction (a, b) the corner whose ABSOLUTE y has parity a and whose absolute z has parity b: lanes with an odd cell coordinate
// exchange their two slots along that axis.  Requests for one row then meet in one instruction, where the address unit merges them
// (n consecutive cells along an axis: n + 1 distinct rows instead of 2n).  The exchange is a lane-wise permutation of a lane's eight
// requests, undone on the landed values before the blend (blend_level_par): every corner value reaches the same slot of the same
// corner-ascending fma chain, so results are bit-identical.  The parity bits travel from issue to blend in the sign bits of the level's
// pos[1] / pos[2] (fract never sets a sign), which costs no register.
template <typename T, int AXIS, int l>
constexpr bool parity_level() {
    return l >= SN_PARITY_FIRST && (AXIS == 2 || (AXIS == 1 && SN_PARITY_AXES == 2));
}
__device__ __forceinline__ float parity_tag(float frac, uint32_t cell) {     // frac >= 0 with the cell's parity as its sign
    return __uint_as_float(__float_as_uint(frac) | (cell << 31));
}
__device__ __forceinline__ bool parity_of(float tagged) { return (__float_as_uint(tagged) >> 31) != 0u; }
// lanes with `odd` set trade a and b
__device__ __forceinline__ void swap_if(bool odd, uint32_t &a, uint32_t &b) {
#if SN_PARITY_UNDO == 1
    const uint64_t m = __builtin_amdgcn_ballot_w64(odd);
    uint64_t sv;
    asm("s_and_saveexec_b64 %[sv], %[m]\n\tv_swap_b32 %[a], %[b]\n\ts_mov_b64 exec, %[sv]" : [a] "+v"(a), [b] "+v"(b), [sv] "=&s"(sv) : [m] "s"(m) : "scc");
#else
    const uint32_t t = a;
    a = odd ? b : a; b = odd ? t : b;
#endif
}
__device__ __forceinline__ void swap_if4(bool odd, uint32_t &a0, uint32_t &b0, uint32_t &a1, uint32_t &b1, uint32_t &a2, uint32_t &b2, uint32_t &a3, uint32_t &b3) {
#if SN_PARITY_UNDO == 1
    const uint64_t m = __builtin_amdgcn_ballot_w64(odd);
    uint64_t sv;
    asm("s_and_saveexec_b64 %[sv], %[m]\n\t"
        "v_swap_b32 %[a0], %[b0]\n\tv_swap_b32 %[a1], %[b1]\n\tv_swap_b32 %[a2], %[b2]\n\tv_swap_b32 %[a3], %[b3]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [a0] "+v"(a0), [b0] "+v"(b0), [a1] "+v"(a1), [b1] "+v"(b1), [a2] "+v"(a2), [b2] "+v"(b2), [a3] "+v"(a3), [b3] "+v"(b3), [sv] "=&s"(sv)
        : [m] "s"(m)
        : "scc");
#else
    uint32_t t;
    t = a0; a0 = odd ? b0 : a0; b0 = odd ? t : b0;
    t = a1; a1 = odd ? b1 : a1; b1 = odd ? t : b1;
    t = a2; a2 = odd ? b2 : a2; b2 = odd ? t : b2;
    t = a3; a3 = odd ? b3 : a3; b3 = odd ? t : b3;
#endif
}

__device__ __forceinline__ void half_wave_swap(uint32_t &a, uint32_t &b) {
#if SN_XSWAP_MODE == 0
    // a' = [a.lanes0-31 | b.lanes0-31], b' = [a.lanes32-63 | b.lanes32-63]
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
#elif SN_XSWAP_MODE == 1
    // lane 2i: a' = a, b' = a of lane 2i+1;  lane 2i+1: a' = b of lane 2i, b' = b  (its own inverse, like the half-wave swap)
    const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    const uint32_t na = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, 0xB1, 0xF, 0xF, true);
    const bool odd = (threadIdx.x & 1u) != 0u;
    a = odd ? nb : a; b = odd ? b : na;
#else
    auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0]; b = r[1];
#endif
}

// Dense levels re-laid out for the final stage (k_pack_pairs, once per render call, a few MB): pair row i of a level
// = (row i, row of the +1 neighbour in x, clamped at the border) -> the two x-corners of a cell come from ONE
// naturally aligned 16-byte load and the border case needs no select (fp16: quad rows, the y-neighbours too).  The gather address
// rate (one wave instruction per 17.5 cycles per CU) is what bounds the final stage: 4 loads
// instead of 8 on the 5 dense levels = 108 instead of 128 gather instructions per sample.
struct PairTab {
    const void *base;            // device; NULL = not available
    uint32_t off[8];             // first pair row of each dense level
};

template <typename T, int C, int KIND, bool PAIRA, bool XSWAP = false>
__device__ __forceinline__ void issue_level(const T *__restrict__ table, const GridLevels &g, int l, const float (&x01)[3],
                                            float (&pos)[3], Corner<T, C> (&cv)[8], const PairTab *pt = nullptr) {
    const uint32_t res = g.res[l], size = g.size[l], mode = g.mode[l];
    const T *tab = table + (size_t)g.off[l] * C;
    uint32_t cell[3], offs[8];
    locate_linear(x01, res, pos, cell);
    if constexpr (PAIRA && KIND == 0 && C == 2 && sizeof(T) == 2) {
        // fp16 rows are 4 bytes: a 16-byte load (which costs what an 8-byte one costs) carries the x- AND the
        // y-neighbour: quad row i = rows (x,y), (x+1,y), (x,y+1), (x+1,y+1), clamped -> 2 loads per level
        constexpr uint32_t QB = 16u;
        const uint32_t sy = res * QB, sz = res * res * QB, top = res - 1u;
        const uint32_t base_off = cell[0] * QB + __umul24(cell[1], sy);
        const uint32_t Z0 = __umul24(cell[2], sz), Z1 = umin(Z0 + sz, top * sz);
        const char *pbase = reinterpret_cast<const char *>(pt->base) + (size_t)pt->off[l] * QB;
#pragma unroll
        for (int zi = 0; zi < 2; ++zi) {
            const uint4 t = *reinterpret_cast<const uint4 *>(pbase + base_off + (zi ? Z1 : Z0));
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) corner_set_half2(cv[4 * zi + q], w[q]);   // q = x + 2 y -> corner index x + 2 y + 4 z
        }
        return;
    }
    if constexpr (PAIRA && KIND == 0 && C == 2) {
        constexpr uint32_t PB = (uint32_t)(2 * C * sizeof(T));
        const uint32_t sy = res * PB, sz = res * res * PB, top = res - 1u;
        const uint32_t X0 = cell[0] * PB, Y0 = __umul24(cell[1], sy), Z0 = __umul24(cell[2], sz);
        const uint32_t Y1 = umin(Y0 + sy, top * sy), Z1 = umin(Z0 + sz, top * sz);
        const char *pbase = reinterpret_cast<const char *>(pt->base) + (size_t)pt->off[l] * PB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t off = X0 + ((i & 1) ? Y1 : Y0) + ((i & 2) ? Z1 : Z0);
            if constexpr (sizeof(T) == 4) {
                const float4 t = *reinterpret_cast<const float4 *>(pbase + off);
                cv[2 * i].v[0] = t.x; cv[2 * i].v[1] = t.y; cv[2 * i + 1].v[0] = t.z; cv[2 * i + 1].v[1] = t.w;
            } else {
                const uint2 t = *reinterpret_cast<const uint2 *>(pbase + off);
                corner_set_half2(cv[2 * i], t.x); corner_set_half2(cv[2 * i + 1], t.y);
            }
        }
        return;
    }
    corner_offsets<KIND, (uint32_t)(C * sizeof(T))>(cell, res, size, mode, offs);
    if constexpr (XSWAP) {
#pragma unroll
        for (int p = 0; p < 4; ++p) half_wave_swap(offs[2 * p], offs[2 * p + 1]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const T *row = reinterpret_cast<const T *>(reinterpret_cast<const char *>(tab) + offs[i]);
        if constexpr (C == 2 && sizeof(T) == 4) {
            const float2 t = *reinterpret_cast<const float2 *>(row);
            cv[i].v[0] = t.x; cv[i].v[1] = t.y;
        } else if constexpr (C == 2 && sizeof(T) == 2) {
            if constexpr (XSWAP) {   // keep the packed row: blend_level_x swaps one register per corner, then unpacks
                cv[i].v[0] = __uint_as_float(*reinterpret_cast<const uint32_t *>(row));
                cv[i].v[1] = 0.0f;
            } else {
                corner_set_half2(cv[i], *reinterpret_cast<const uint32_t *>(row));
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) cv[i].v[c] = table_ld<T>(row + c);
        }
    }
}

// PKW: the 8 corner weights as 6 packed multiplies (x-pairs: (wx0, wx1) * wy, then * wz) instead of 12 scalar ones;
// every weight is still (wx * wy) * wz, every channel still one corner-ascending fma chain.  Final stage only (the
// proposal kernels have no registers to spare for the even-aligned pairs).
template <typename T, int C, bool PKW = false>
__device__ __forceinline__ void blend_level(const float (&pos)[3], const Corner<T, C> (&cv)[8], float (&acc)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    if constexpr (C == 2 && sizeof(T) == 2) {   // packed fp16 rows (corner_set_half2): widening fma, same order
        float w[8];
        if constexpr (PKW) {                // the 8 corner weights as 6 packed multiplies: every weight still (wx * wy) * wz
            typedef float f2 __attribute__((ext_vector_type(2)));
            const f2 wx = {1.0f - pos[0], pos[0]};
            const float wy0 = 1.0f - pos[1], wz0 = 1.0f - pos[2];
            const f2 xy0 = wx * f2{wy0, wy0}, xy1 = wx * f2{pos[1], pos[1]};
            const f2 w01 = xy0 * f2{wz0, wz0}, w23 = xy1 * f2{wz0, wz0}, w45 = xy0 * f2{pos[2], pos[2]}, w67 = xy1 * f2{pos[2], pos[2]};
            w[0] = w01.x; w[1] = w01.y; w[2] = w23.x; w[3] = w23.y; w[4] = w45.x; w[5] = w45.y; w[6] = w67.x; w[7] = w67.y;
        } else {
#pragma unroll
            for (uint32_t idx = 0; idx < 8; ++idx) {
                float t = 1.0f;
#pragma unroll
                for (uint32_t d = 0; d < 3; ++d) t *= (idx & (1u << d)) ? pos[d] : 1.0f - pos[d];
                w[idx] = t;
            }
        }
#pragma unroll
        for (uint32_t idx = 0; idx < 8; ++idx) {
            const uint32_t bits = __float_as_uint(cv[idx].v[0]);
            acc[0] = fma_mix_lo(w[idx], bits, acc[0]);
            acc[1] = fma_mix_hi(w[idx], bits, acc[1]);
        }
        return;
    }
    if constexpr (PKW && C == 2) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const f2 wx = {1.0f - pos[0], pos[0]};
        const float wy0 = 1.0f - pos[1], wz0 = 1.0f - pos[2];
        const f2 xy0 = wx * f2{wy0, wy0}, xy1 = wx * f2{pos[1], pos[1]};
        const f2 w01 = xy0 * f2{wz0, wz0}, w23 = xy1 * f2{wz0, wz0}, w45 = xy0 * f2{pos[2], pos[2]}, w67 = xy1 * f2{pos[2], pos[2]};
        const float w[8] = {w01.x, w01.y, w23.x, w23.y, w45.x, w45.y, w67.x, w67.y};
        f2 a = {0.0f, 0.0f};
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) a = __builtin_elementwise_fma(f2{w[idx], w[idx]}, f2{cv[idx].v[0], cv[idx].v[1]}, a);
        acc[0] = a.x; acc[1] = a.y;
        return;
    }
#pragma unroll
    for (uint32_t idx = 0; idx < 8; ++idx) {   // corner order and weight products exactly as gridencoder.cu:171-192
        float w = 1.0f;
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) w *= (idx & (1u << d)) ? pos[d] : 1.0f - pos[d];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __builtin_fmaf(w, cv[idx].v[c], acc[c]);
    }
}

// blend of a level whose gathers were issued with XSWAP: first give every lane its own corner values back
template <typename T, int C, bool PKW = false>
__device__ __forceinline__ void blend_level_x(const float (&pos)[3], const Corner<T, C> (&cv)[8], float (&acc)[C]) {
    Corner<T, C> own[8];
    if constexpr (C == 2 && sizeof(T) == 2) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            uint32_t a = __float_as_uint(cv[2 * p].v[0]), b = __float_as_uint(cv[2 * p + 1].v[0]);
            half_wave_swap(a, b);
            corner_set_half2(own[2 * p], a); corner_set_half2(own[2 * p + 1], b);
        }
        blend_level<T, C, PKW>(pos, own, acc);
        return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            uint32_t a = __float_as_uint(cv[2 * p].v[c]), b = __float_as_uint(cv[2 * p + 1].v[c]);
            half_wave_swap(a, b);
            own[2 * p].v[c] = __uint_as_float(a); own[2 * p + 1].v[c] = __uint_as_float(b);
        }
    }
    blend_level<T, C, PKW>(pos, own, acc);
}

// blend of a hashed FinalLv level issued with XSWAP and by parity (issue_level_lv<..., PY, PZ>): the half-wave exchange back, then lanes
// whose cell was odd along z trade the landed values of slots i and i + 4, then those odd along y the slots i and i + 2 -- the issue
// order undone in reverse -- and the unchanged blend on |pos| (the signs of pos[1] / pos[2] carried the parities)
template <typename T, bool PY, bool PZ>
__device__ __forceinline__ void blend_level_par(const float (&pos)[3], const Corner<T, 2> (&cv)[8], float (&acc)[2]) {
    constexpr int NW = sizeof(T) == 2 ? 1 : 2;          // dwords per landed row: fp16 rows stay packed in v[0]
    uint32_t w[8][NW];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            uint32_t a = __float_as_uint(cv[2 * p].v[c]), b = __float_as_uint(cv[2 * p + 1].v[c]);
            half_wave_swap(a, b);
            w[2 * p][c] = a; w[2 * p + 1][c] = b;
        }
    }
    float ap[3] = {pos[0], pos[1], pos[2]};
    if constexpr (PZ) {
        const bool odd = parity_of(pos[2]);
        ap[2] = __builtin_fabsf(pos[2]);
#pragma unroll
        for (int c = 0; c < NW; ++c) swap_if4(odd, w[0][c], w[4][c], w[1][c], w[5][c], w[2][c], w[6][c], w[3][c], w[7][c]);
    }
    if constexpr (PY) {
        const bool odd = parity_of(pos[1]);
        ap[1] = __builtin_fabsf(pos[1]);
#pragma unroll
        for (int c = 0; c < NW; ++c) swap_if4(odd, w[0][c], w[2][c], w[1][c], w[3][c], w[4][c], w[6][c], w[5][c], w[7][c]);
    }
    Corner<T, 2> own[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (sizeof(T) == 2) corner_set_half2(own[i], w[i][0]);
        else { own[i].v[0] = __uint_as_float(w[i][0]); own[i].v[1] = __uint_as_float(w[i][1]); }
    }
    blend_level<T, 2, true>(ap, own, acc);
}

// Encodes all L levels; `emit(l, acc)` receives each level's C features (zeros when out of range).
// K = number of leading dense levels (levels >= K are hashed); K < 0: level kind decided at run time.
// Returns true for lanes whose coordinate is outside [0,1] (gridencoder.cu:105-130 writes zeros for them): the
// caller zeroes those lanes' features on a wave-uniform, practically never taken branch instead of paying a
// select per level (positions are contracted into [0,1] on this path).
template <typename T, int L, int C, int GROUP, int K, bool PAIR, typename Emit>
__device__ __forceinline__ bool encode_grouped(const T *__restrict__ table, const GridLevels &g, const float (&x01)[3], Emit emit,
                                               const PairTab *pt = nullptr) {
    // (a last, shorter group is allowed: L = 5 levels in groups of 3 + 2)
    bool oob = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) oob |= (x01[d] < 0.0f || x01[d] > 1.0f);
    constexpr int G = GROUP >= L ? L : GROUP;
    static_for<0, (L + G - 1) / G>([&](auto grp) {
        constexpr int l0 = decltype(grp)::value * G;
        constexpr int GN = (L - l0) < G ? (L - l0) : G;        // levels in this group
        float pos[GN][3];
        Corner<T, C> cv[GN][8];
        static_for<0, GN>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            constexpr int KIND = K < 0 ? -1 : ((l0 + k) < K ? 0 : 1);
            issue_level<T, C, KIND, (PAIR && K > 0 && K <= 8)>(table, g, l0 + k, x01, pos[k], cv[k], pt);
        });
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < GN; ++k) {
            float acc[C];
            blend_level<T, C>(pos[k], cv[k], acc);
            emit(l0 + k, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    return oob;
}

// ---- software-pipelined form of encode_grouped ------------------------------------------------
// issue_group<GRP> starts the GROUP*8 gathers of level group GRP; blend_group<GRP> consumes them.
// The final stage uses the pair to keep the FIRST group of sample j+1 in flight across the
// matrix-core phase of sample j (the compiler never hoists loads over the loop back-edge).
template <typename T, int C, int G>
struct GroupRegs {
    float pos[G][3];
    Corner<T, C> cv[G][8];
    bool oob;
};

template <typename T, int C, int G, int K, int GRP>
__device__ __forceinline__ void issue_group(const T *__restrict__ table, const GridLevels &g, const float (&x01)[3],
                                            GroupRegs<T, C, G> &r, const PairTab &pt) {
    r.oob = false;   // out-of-range lanes are fixed up by the caller on a wave-uniform rare path
    static_for<0, G>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        constexpr int l = GRP * G + k;
        constexpr int KIND = K < 0 ? -1 : (l < K ? 0 : 1);
        issue_level<T, C, KIND, (K > 0 && K <= 8), xswap_level<T, KIND, l>()>(table, g, l, x01, r.pos[k], r.cv[k], &pt);
    });
}

template <typename T, int C, int G, int K, int GRP, typename Emit>
__device__ __forceinline__ void blend_group(const GroupRegs<T, C, G> &r, Emit emit) {
    static_for<0, G>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        constexpr int l = GRP * G + k;
        constexpr int KIND = K < 0 ? -1 : (l < K ? 0 : 1);
        float acc[C];
        if constexpr (xswap_level<T, KIND, l>()) blend_level_x<T, C, true>(r.pos[k], r.cv[k], acc);
        else blend_level<T, C, true>(r.pos[k], r.cv[k], acc);
        emit(l, acc);
    });
}

// ---- final stage, specialised instantiations (K > 0: dense prefix + hashed tail): per-level constants from the host ----
// The generic code above derives every per-level quantity from GridLevels inside the march: u32 -> f32 conversions of the
// resolutions, 64-bit base pointers per level (more than the scalar file holds: ~150 v_readlane / v_writelane spill
// instructions per sample), border selects and clamps on every level.  The final stage issues one instruction per
// 4 cycles per SIMD whatever its type and is bound by exactly that, so this variant removes
// instructions, bit-identically:
//   * resolutions / limits arrive as floats and byte quantities in the kernel argument (FinalLv);
//   * hashed levels of a GridEncoder table are equal-sized and contiguous (grid.py:121-136: a level is hashed iff it hit
//     the 2^log2_hashmap_size cap), so ONE base pointer + a per-level byte offset OR-ed into the masked x term serves all
//     of them; the two prime multiplies become full-rate 24-bit multiplies (only the bits under the mask matter);
//   * FAST (wave-uniform, decided per sample): every lane's coordinate is at least one coarsest-hashed-level cell away
//     from the border of [0,1]^3 -> on hashed levels neither the position clamp nor the clamp of the +1 neighbour
//     (gridencoder.cu:148,182) can trigger, and out-of-range zeroing cannot apply.  Otherwise the general form runs.
struct FinalLv {
    float res_f[16];                 // level resolution (gridencoder.cu:133) as float
    float top_f[16];                 // res - 1
    uint32_t d_sy[8], d_sz[8];       // dense levels inside the pair / quad-row table (PairTab): y and z strides in bytes,
    uint32_t d_ylim[8], d_zlim[8];   //   (res - 1) * stride, the clamp of the +1 neighbour,
    uint32_t d_off[8];               //   byte offset of the level
    uint32_t h_off[16];              // hashed levels: byte offset from the first hashed level (a multiple of size * row bytes)
    uint32_t h_mask;                 // (size - 1) * row bytes, the same for every hashed level
    float in_lo, in_hi;              // FAST <=> in_lo <= x01[d] <= in_hi for all lanes and dimensions
    const char *pair_base, *hash_base;
};

template <typename T, bool DENSE, bool FAST, bool XSWAP, int l, bool PY = false, bool PZ = false>
__device__ __forceinline__ void issue_level_lv(const FinalLv &lv, const float (&x01)[3], float (&pos)[3], Corner<T, 2> (&cv)[8]) {
    static_assert(!(PY || PZ) || (!DENSE && XSWAP), "parity grouping: hashed levels, in front of the half-wave exchange");
    constexpr uint32_t RB = 2u * (uint32_t)sizeof(T);              // bytes per table row (C = 2)
    const float rf = lv.res_f[l];
    uint32_t cell[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float p = __builtin_fmaf(x01[d], rf, -0.5f);
        if constexpr (DENSE || !FAST) p = __builtin_amdgcn_fmed3f(p, 0.0f, lv.top_f[l]);   // = min(max(p, 0), res-1), gridencoder.cu:148
        cell[d] = (uint32_t)p;
        pos[d] = __builtin_amdgcn_fractf(p);
    }
    if constexpr (DENSE) {
        const uint32_t sy = lv.d_sy[l], sz = lv.d_sz[l];
        const uint32_t X0 = __umul24(cell[0], 16u) + lv.d_off[l];
        const uint32_t Y0 = __umul24(cell[1], sy), Z0 = __umul24(cell[2], sz);
        const uint32_t Y1 = umin(Y0 + sy, lv.d_ylim[l]), Z1 = umin(Z0 + sz, lv.d_zlim[l]);
        if constexpr (sizeof(T) == 2) {          // quad rows: (x,y), (x+1,y), (x,y+1), (x+1,y+1)
#pragma unroll
            for (int zi = 0; zi < 2; ++zi) {
                const uint4 t = *reinterpret_cast<const uint4 *>(lv.pair_base + (X0 + Y0 + (zi ? Z1 : Z0)));
                const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) corner_set_half2(cv[4 * zi + q], w[q]);
            }
        } else {                                 // pair rows: (x, x+1)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t off = X0 + ((i & 1) ? Y1 : Y0) + ((i & 2) ? Z1 : Z0);
                const float4 t = *reinterpret_cast<const float4 *>(lv.pair_base + off);
                cv[2 * i].v[0] = t.x; cv[2 * i].v[1] = t.y; cv[2 * i + 1].v[0] = t.z; cv[2 * i + 1].v[1] = t.w;
            }
        }
    } else {
        constexpr uint32_t MY = (2654435761u * RB) & 0xFFFFFFu, MZ = (805459861u * RB) & 0xFFFFFFu;   // gridencoder.cu:49, low 24 bits
        const uint32_t mask = lv.h_mask, ho = lv.h_off[l];
        const uint32_t X0 = cell[0] * RB, Y0 = __umul24(cell[1], MY), Z0 = __umul24(cell[2], MZ);
        uint32_t X1 = X0 + RB, Y1 = Y0 + MY, Z1 = Z0 + MZ;
        if constexpr (!FAST) {                   // the +1 neighbour is clamped to res-1 (gridencoder.cu:182)
            const uint32_t top = (uint32_t)lv.top_f[l];
            X1 = cell[0] < top ? X1 : X0; Y1 = cell[1] < top ? Y1 : Y0; Z1 = cell[2] < top ? Z1 : Z0;
        }
        const uint32_t X0m = (X0 & mask) | ho, X1m = (X1 & mask) | ho;
        uint32_t Y0m = Y0 & mask, Y1m = Y1 & mask, Z0m = Z0 & mask, Z1m = Z1 & mask;
        // PARITY: slot a of an axis takes the corner whose absolute coordinate has parity a -- odd cells trade their two terms (with the
        // clamped neighbour both terms are equal: the rule is only a grouping); the parity rides in the sign of pos[d] to the blend
        if constexpr (PY) {
            pos[1] = parity_tag(pos[1], cell[1]);
            swap_if(parity_of(pos[1]), Y0m, Y1m);
        }
        if constexpr (PZ) {
            pos[2] = parity_tag(pos[2], cell[2]);
            swap_if(parity_of(pos[2]), Z0m, Z1m);
        }
        uint32_t offs[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) offs[i] = ((i & 1u) ? X1m : X0m) ^ ((i & 2u) ? Y1m : Y0m) ^ ((i & 4u) ? Z1m : Z0m);
        if constexpr (XSWAP) {
#pragma unroll
            for (int q = 0; q < 4; ++q) half_wave_swap(offs[2 * q], offs[2 * q + 1]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const char *row = lv.hash_base + offs[i];
            if constexpr (sizeof(T) == 4) {
                const float2 t = *reinterpret_cast<const float2 *>(row);
                cv[i].v[0] = t.x; cv[i].v[1] = t.y;
            } else if constexpr (XSWAP) {
                cv[i].v[0] = __uint_as_float(*reinterpret_cast<const uint32_t *>(row)); cv[i].v[1] = 0.0f;
            } else {
                corner_set_half2(cv[i], *reinterpret_cast<const uint32_t *>(row));
            }
        }
    }
}

// levels L0 .. L0+G-1 (a "span": the gather groups of the final stage need not be equally long)
// PAR = false: the canonical corner order on every level (the A/B partner of the parity order, experiments builds: SN_EXP_GATHER_CANONICAL)
template <typename T, int L0, int G, int K, bool FAST, bool PAR = true>
__device__ __forceinline__ void issue_span_lv(const FinalLv &lv, const float (&x01)[3], GroupRegs<T, 2, G> &r) {
    r.oob = false;
    static_for<0, G>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        constexpr int l = L0 + k;
        constexpr bool DENSE = l < K;
        issue_level_lv<T, DENSE, FAST, xswap_level<T, DENSE ? 0 : 1, l>(), l, PAR && !DENSE && parity_level<T, 1, l>(), PAR && !DENSE && parity_level<T, 2, l>()>(
            lv, x01, r.pos[k], r.cv[k]);
    });
}
template <typename T, int G, int K, int GRP, bool FAST, bool PAR = true>
__device__ __forceinline__ void issue_group_lv(const FinalLv &lv, const float (&x01)[3], GroupRegs<T, 2, G> &r) {
    issue_span_lv<T, GRP * G, G, K, FAST, PAR>(lv, x01, r);
}
template <typename T, int L0, int G, int K, bool PAR = true, typename Emit>
__device__ __forceinline__ void blend_span(const GroupRegs<T, 2, G> &r, Emit emit) {
    static_for<0, G>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        constexpr int l = L0 + k;
        constexpr int KIND = K < 0 ? -1 : (l < K ? 0 : 1);
        constexpr bool PY = PAR && KIND == 1 && parity_level<T, 1, l>(), PZ = PAR && KIND == 1 && parity_level<T, 2, l>();
        float acc[2];
        if constexpr (PY || PZ) blend_level_par<T, PY, PZ>(r.pos[k], r.cv[k], acc);
        else if constexpr (xswap_level<T, KIND, l>()) blend_level_x<T, 2, true>(r.pos[k], r.cv[k], acc);
        else blend_level<T, 2, true>(r.pos[k], r.cv[k], acc);
        emit(l, acc);
    });
}
// gather spans of the final stage (FinalLv path).  Span 0 is issued for sample j+1 before the matrix-core phase of sample j
// (its registers are live across that phase), so it has to be short when the MLP needs many registers; it must be all dense.
template <int CFG> struct FinalSpans;
template <> struct FinalSpans<0> { static constexpr int N = 4; static constexpr int B[5] = {0, 4, 8, 12, 16}; };
template <> struct FinalSpans<1> { static constexpr int N = 4; static constexpr int B[5] = {0, 2, 6, 11, 16}; };
template <> struct FinalSpans<2> { static constexpr int N = 4; static constexpr int B[5] = {0, 3, 7, 12, 16}; };
template <> struct FinalSpans<3> { static constexpr int N = 4; static constexpr int B[5] = {0, 1, 6, 11, 16}; };
template <> struct FinalSpans<4> { static constexpr int N = 5; static constexpr int B[6] = {0, 2, 5, 9, 13, 16}; };
template <> struct FinalSpans<5> { static constexpr int N = 5; static constexpr int B[6] = {0, 1, 4, 8, 12, 16}; };
template <> struct FinalSpans<6> { static constexpr int N = 5; static constexpr int B[6] = {0, 2, 4, 8, 12, 16}; };
template <> struct FinalSpans<7> { static constexpr int N = 5; static constexpr int B[6] = {0, 3, 6, 9, 13, 16}; };
template <> struct FinalSpans<8> { static constexpr int N = 5; static constexpr int B[6] = {0, 4, 7, 10, 13, 16}; };
template <> struct FinalSpans<9> { static constexpr int N = 6; static constexpr int B[7] = {0, 2, 5, 8, 11, 14, 16}; };
template <> struct FinalSpans<10> { static constexpr int N = 3; static constexpr int B[4] = {0, 2, 9, 16}; };
template <> struct FinalSpans<11> { static constexpr int N = 4; static constexpr int B[5] = {0, 2, 7, 12, 16}; };
template <> struct FinalSpans<12> { static constexpr int N = 3; static constexpr int B[4] = {0, 4, 10, 16}; };
template <> struct FinalSpans<13> { static constexpr int N = 3; static constexpr int B[4] = {0, 1, 8, 16}; };
template <> struct FinalSpans<14> { static constexpr int N = 2; static constexpr int B[3] = {0, 5, 16}; };
template <> struct FinalSpans<15> { static constexpr int N = 3; static constexpr int B[4] = {0, 3, 9, 16}; };

// FAST test of one sample (see FinalLv): wave-uniform
__device__ __forceinline__ bool all_interior(const FinalLv &lv, const float (&x01)[3]) {
    const bool in = (x01[0] >= lv.in_lo && x01[0] <= lv.in_hi) && (x01[1] >= lv.in_lo && x01[1] <= lv.in_hi) &&
                    (x01[2] >= lv.in_lo && x01[2] <= lv.in_hi);
    return __all(in) != 0;
}

// all levels of one grid at one position into registers; D = 3.  gridencoder.cu:94-201 per level.
template <typename T, int L, int C, int K, bool PAIRX, int GROUP = L>
__device__ __forceinline__ void encode_levels(const T *__restrict__ table, const GridLevels &g, const float (&x01)[3],
                                              float (&feat)[L * C], const PairTab *pt = nullptr) {
    const bool oob = encode_grouped<T, L, C, GROUP, K, PAIRX>(table, g, x01, [&](int l, const float (&acc)[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) feat[l * C + c] = acc[c];
    }, pt);
    // register variant (proposal stages): L*C unconditional selects; a branch here costs more in scheduling than it saves
#pragma unroll
    for (int i = 0; i < L * C; ++i) feat[i] = oob ? 0.0f : feat[i];
}

// U positions of one lane through the same grid at once: every level group issues the gathers of all U positions before the
// first blend, so a wave carries U independent gather -> blend chains (the proposal stage is bound by the length of that chain,
// not by an execution unit).  Values identical to U calls of encode_levels.
template <typename T, int L, int C, int K, bool PAIRX, int GROUP, int U>
__device__ __forceinline__ void encode_levels_multi(const T *__restrict__ table, const GridLevels &g, const float (&x01)[U][3],
                                                    float (&feat)[U][L * C], const PairTab *pt = nullptr) {
    constexpr int G = GROUP >= L ? L : GROUP;
    static_for<0, (L + G - 1) / G>([&](auto grp) {
        constexpr int l0 = decltype(grp)::value * G;
        constexpr int GN = (L - l0) < G ? (L - l0) : G;
        float pos[U][GN][3];
        Corner<T, C> cv[U][GN][8];
        static_for<0, U>([&](auto uu) {
            constexpr int u = decltype(uu)::value;
            static_for<0, GN>([&](auto kk) {
                constexpr int k = decltype(kk)::value;
                constexpr int KIND = K < 0 ? -1 : ((l0 + k) < K ? 0 : 1);
                issue_level<T, C, KIND, (PAIRX && K > 0 && K <= 8)>(table, g, l0 + k, x01[u], pos[u][k], cv[u][k], pt);
            });
        });
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < GN; ++k) {
                float acc[C];
                blend_level<T, C>(pos[u][k], cv[u][k], acc);
#pragma unroll
                for (int c = 0; c < C; ++c) feat[u][(l0 + k) * C + c] = acc[c];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    });
#pragma unroll
    for (int u = 0; u < U; ++u) {
        bool oob = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) oob |= (x01[u][d] < 0.0f || x01[u][d] > 1.0f);
#pragma unroll
        for (int i = 0; i < L * C; ++i) feat[u][i] = oob ? 0.0f : feat[u][i];
    }
}

}  // namespace sn

#endif  // SN_RENDER_GATHER_H
