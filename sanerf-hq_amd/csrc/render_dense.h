// render_dense.h -- fused renderer: the small dense layers on the vector ALU (proposal MLP, colour head): weights staged in LDS, k-ascending fmaf chains.
#ifndef SN_RENDER_DENSE_H
#define SN_RENDER_DENSE_H
#include "sn_common.h"
#include "sh_basis.inc"
#include <float.h>

namespace sn {

// y = act(W x), W [OUT][IN] row-major at a wave-uniform address (SGPR / scalar-cache loads);
// each output is one k-ascending fmaf chain (the oracle's order).
template <int IN, int OUT, int ACT>
__device__ __forceinline__ void dense_uniform(const float *__restrict__ W, const float (&x)[IN], float (&y)[OUT]) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < IN; ++k) acc = __builtin_fmaf(W[o * IN + k], x[k], acc);
        if (ACT == 1) acc = relu_ieee(acc);                  // ReLU as one v_maximum_f32 (a NaN stays NaN, as torch.relu)
        y[o] = acc;
    }
}

// An always-zero offset the optimiser cannot see through.  Adding it to an LDS index inside the
// sample loop stops loop-invariant code motion from hoisting every (loop-invariant) weight
// read out of the loop and pinning hundreds of VGPRs for the whole march.
__device__ __forceinline__ uint32_t opaque_zero() {
    uint32_t z = 0;
    asm volatile("" : "+v"(z));
    return z;
}

// Tiny-MLP weights are staged once per workgroup in LDS with rows padded to a multiple of 4
// floats, and read back at wave-uniform addresses (LDS broadcast, one ds_read_b128 per 4
// weights).  Reading them through global pointers makes hipcc hoist hundreds of vector loads
// (it cannot prove the buffers read-only next to the kernel's stores) and wrecks occupancy.
template <int IN> struct PadIn { static constexpr int value = (IN + 3) & ~3; };

// dst[k * OUTP + o] = W[o][k]  (k-major; rows padded to a multiple of 4 outputs)
template <int IN, int OUT>
__device__ __forceinline__ void stage_weights_t(float *__restrict__ dst, const float *__restrict__ src) {
    constexpr int OUTP = PadIn<OUT>::value;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(IN * OUTP); i += blockDim.x) {
        const uint32_t k = i / OUTP, o = i - k * OUTP;
        dst[i] = o < (uint32_t)OUT ? src[o * IN + k] : 0.0f;
    }
}

// y = act(W x), W k-major in LDS at a wave-uniform address (broadcast ds_read_b128 of 4 adjacent outputs);
// every output is still ONE k-ascending fmaf chain starting from 0 (the oracle's order), the chains of
// adjacent outputs just advance together, which lets the compiler use packed fp32 FMAs without shuffles.
// PIN: the weights of input k+1 are fetched under the FMAs of input k and never earlier -- their address carries a fake dependence on the
// accumulators of step k-1 (an empty asm).  In a register-hungry caller the scheduler otherwise fetches all IN * OUT weights ahead (160 registers).
template <int IN, int OUT, int ACT, bool PIN = false>
__device__ __forceinline__ void dense_ldsw_t(const float *__restrict__ Wl, const float (&x)[IN], float (&y)[OUT]) {
    constexpr int OUTP = PadIn<OUT>::value;
    float acc[OUTP];
#pragma unroll
    for (int o = 0; o < OUTP; ++o) acc[o] = 0.0f;
    uint32_t z = 0;
    float4 w[2][OUTP / 4];
    if (PIN) {
#pragma unroll
        for (int o4 = 0; o4 < OUTP / 4; ++o4) w[0][o4] = *reinterpret_cast<const float4 *>(Wl + 4 * o4);
    }
#pragma unroll
    for (int k = 0; k < IN; ++k) {
#pragma unroll
        for (int o4 = 0; o4 < OUTP / 4; ++o4) {
            const float4 wk = PIN ? w[k & 1][o4] : *reinterpret_cast<const float4 *>(Wl + k * OUTP + 4 * o4);
            if (PIN && o4 == 0 && k + 1 < IN) {
                static_assert(!PIN || OUTP == 16, "the fake dependence lists 16 accumulators");
                // (all accumulators as they stand after step k-1: the fetch of step k+1 cannot start before step k-1 is complete)
                asm volatile("" : "+v"(z) : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]),
                                            "v"(acc[8 % OUTP]), "v"(acc[9 % OUTP]), "v"(acc[10 % OUTP]), "v"(acc[11 % OUTP]), "v"(acc[12 % OUTP]), "v"(acc[13 % OUTP]),
                                            "v"(acc[14 % OUTP]), "v"(acc[15 % OUTP]));
#pragma unroll
                for (int q = 0; q < OUTP / 4; ++q) w[(k + 1) & 1][q] = *reinterpret_cast<const float4 *>(Wl + z + (k + 1) * OUTP + 4 * q);
            }
            acc[4 * o4 + 0] = __builtin_fmaf(wk.x, x[k], acc[4 * o4 + 0]);
            acc[4 * o4 + 1] = __builtin_fmaf(wk.y, x[k], acc[4 * o4 + 1]);
            acc[4 * o4 + 2] = __builtin_fmaf(wk.z, x[k], acc[4 * o4 + 2]);
            acc[4 * o4 + 3] = __builtin_fmaf(wk.w, x[k], acc[4 * o4 + 3]);
        }
    }
#pragma unroll
    for (int o = 0; o < OUT; ++o) y[o] = (ACT == 1) ? relu_ieee(acc[o]) : acc[o];
}

// Tiny-MLP weights in the [out][in_padded] layout (view MLP, evaluated once per ray)
template <int IN, int OUT>
__device__ __forceinline__ void stage_weights(float *__restrict__ dst, const float *__restrict__ src) {
    constexpr int INP = PadIn<IN>::value;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(OUT * INP); i += blockDim.x) {
        const uint32_t o = i / INP, k = i - o * INP;
        dst[i] = k < (uint32_t)IN ? src[o * IN + k] : 0.0f;
    }
}

// y = act(W x) with W in LDS (padded rows), fully unrolled; k-ascending fmaf chain per output.
template <int IN, int OUT, int ACT>
__device__ __forceinline__ void dense_ldsw(const float *__restrict__ Wl, const float (&x)[IN], float (&y)[OUT]) {
    constexpr int INP = PadIn<IN>::value;
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float acc = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < INP / 4; ++k4) {
            const float4 w = *reinterpret_cast<const float4 *>(Wl + o * INP + 4 * k4);
            if (4 * k4 + 0 < IN) acc = __builtin_fmaf(w.x, x[4 * k4 + 0], acc);
            if (4 * k4 + 1 < IN) acc = __builtin_fmaf(w.y, x[4 * k4 + 1], acc);
            if (4 * k4 + 2 < IN) acc = __builtin_fmaf(w.z, x[4 * k4 + 2], acc);
            if (4 * k4 + 3 < IN) acc = __builtin_fmaf(w.w, x[4 * k4 + 3], acc);
        }
        if (ACT == 1) acc = relu_ieee(acc);                  // ReLU as one v_maximum_f32 (a NaN stays NaN, as torch.relu)
        y[o] = acc;
    }
}

// same, but the output loop stays rolled and activations travel through an LDS column
// (xin[k*stride] -> yout[o*stride]); x is read completely before the first write, so
// xin == yout is allowed.
template <int IN, int OUT, int ACT>
__device__ __forceinline__ void dense_ldsw_col(const float *__restrict__ Wl, const float *xin, float *yout, uint32_t stride) {
    constexpr int INP = PadIn<IN>::value;
    float x[IN];
#pragma unroll
    for (int k = 0; k < IN; ++k) x[k] = xin[k * stride];
#pragma unroll 1
    for (int o = 0; o < OUT; ++o) {
        float acc = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < INP / 4; ++k4) {
            const float4 w = *reinterpret_cast<const float4 *>(Wl + o * INP + 4 * k4);
            if (4 * k4 + 0 < IN) acc = __builtin_fmaf(w.x, x[4 * k4 + 0], acc);
            if (4 * k4 + 1 < IN) acc = __builtin_fmaf(w.y, x[4 * k4 + 1], acc);
            if (4 * k4 + 2 < IN) acc = __builtin_fmaf(w.z, x[4 * k4 + 2], acc);
            if (4 * k4 + 3 < IN) acc = __builtin_fmaf(w.w, x[4 * k4 + 3], acc);
        }
        if (ACT == 1) acc = relu_ieee(acc);                  // ReLU as one v_maximum_f32 (a NaN stays NaN, as torch.relu)
        yout[o * stride] = acc;
    }
}

// degree-4 real SH (16 values) of a unit vector; basis generated by tools/gen_sh.py
__device__ __forceinline__ void sh_degree4(float x, float y, float z, float (&o)[16]) {
    const uint32_t C = 4u;
    SN_SH_POWERS
    (void)x4; (void)x5; (void)x6; (void)x7; (void)y4; (void)y5; (void)y6; (void)y7; (void)z4; (void)z5; (void)z6; (void)z7;
    SN_SH_VALUES(o);
}

__device__ __forceinline__ float nan_to_num(float v) {
    if (v != v) return 0.0f;
    if (v == __builtin_inff()) return FLT_MAX;
    if (v == -__builtin_inff()) return -FLT_MAX;
    return v;
}

}  // namespace sn

#endif  // SN_RENDER_DENSE_H
