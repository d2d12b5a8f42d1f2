// sn_reduce.h — the fixed-order ticket reduction of the device-side meters and losses (k_mask_eval_accumulate, k_image_sqerr_accumulate,
// k_image_ssim, k_feature_distill): one launch turns a double per lane into one value on the device.  Nobody waits for anybody, the host
// reads nothing, two runs give the same bits, and the workspace is zero when the launch ends.
//
// The sum, whose order is part of each entry point's contract:
//   lane -> wave        each lane arrives with a double; a 64-lane butterfly (wave_sum) adds them, the same order in every run;
//   wave -> workgroup   the four wave values go through LDS and thread 0 adds them as ((w0 + w1) + w2) + w3;
//   workgroup -> image  thread 0 of the workgroup that drew the last ticket adds the partials 0 .. gridDim.x - 1 in ascending order.
// An optional uint32_t count per lane travels the same way (integer, so its order does not matter).
//
// Memory ordering, why the last workgroup sees every partial:
//   1. Thread 0 stores the workgroup's partial into its own slot part_sum[blockIdx.x] (a plain store); other lanes may have published
//      values of the caller's before the call (the class histogram of k_mask_eval_accumulate: integer atomics).
//   2. Every lane executes __threadfence(): its own earlier stores and atomics are visible at agent scope before anything it does later.
//      The barrier that follows puts all 256 fences before thread 0's next step.
//   3. Thread 0 adds 1 to the ticket, acq_rel at agent scope.  The release half orders the workgroup's published values before the
//      increment; the adds of all workgroups form one modification order of the ticket, so the workgroup that reads gridDim.x - 1 comes
//      after every other increment, and the acquire half makes what preceded those increments visible to thread 0.
//   4. The draw goes to the other lanes through LDS and a barrier.  They have acquired nothing themselves, so every lane of the last
//      workgroup executes __threadfence() once more and then reads the slots with relaxed agent-scope atomic loads, which no stale
//      cache line can serve.
//   5. The lane that read a slot stores 0 to it; thread 0 stores 0 to the ticket as its last statement (at the call site, after the
//      kernel's own end-of-launch work).  Every other workgroup is past its last access to the workspace by then -- that is what the last
//      ticket means -- and the next launch on the stream starts after this one has ended: the workspace is zero at rest.
// No workgroup spins on another: one that does not draw the last ticket returns.
//
// The functions are for workgroups of SN_REDUCE_THREADS = 256 lanes in x (four waves) and grids in x; every lane of the workgroup calls
// them.  The LDS they use is handed in by the caller, who knows what else lives there (k_image_ssim sums its partials out of the LDS of its
// maps).  k_adam_multi (optim.hip) takes a ticket of the same kind for another purpose -- one wave, no partials, no LDS -- and keeps its own
// few lines.
#pragma once

#include "sn_common.h"

namespace sn {

constexpr uint32_t SN_REDUCE_THREADS = 256;

// The sum of v over the wave in every lane, for double, float and uint32_t.  A butterfly: the same order of additions in every run.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Steps 1-4: the workgroup's partial sum (and count, where part_cnt and s_cnt are given) into slot blockIdx.x, then the ticket.  True in
// every lane of the workgroup that drew the last ticket: all the others have published.  s_wave (and s_cnt): 4 entries of LDS; s_flag: one.
__device__ __forceinline__ bool publish_and_draw(double sum, uint32_t count, uint32_t *ticket, double *part_sum, uint32_t *part_cnt, double *s_wave,
                                                 uint32_t *s_cnt, uint32_t *s_flag) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    sum = wave_sum(sum);
    if (part_cnt) count = wave_sum(count);
    if (lane == 0) {
        s_wave[wave] = sum;
        if (part_cnt) s_cnt[wave] = count;
    }
    __syncthreads();
    if (tid == 0) {
        part_sum[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        if (part_cnt) part_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const uint32_t mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        *s_flag = mine == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    const bool last = *s_flag != 0u;
    if (last) __threadfence();
    return last;
}

// Step 5 and the last sum, in the last workgroup: the partials through s_part (and s_pcnt) -- gridDim.x entries of LDS -- in ascending
// order; their slots go back to zero.  Thread 0's return value (and *count) are the ones to use.
__device__ __forceinline__ double sum_partials(double *part_sum, uint32_t *part_cnt, double *s_part, uint32_t *s_pcnt, uint64_t *count) {
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += SN_REDUCE_THREADS) {
        s_part[i] = __hip_atomic_load(&part_sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (part_cnt) s_pcnt[i] = __hip_atomic_load(&part_cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part_sum[i], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (part_cnt) __hip_atomic_store(&part_cnt[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    double total = 0.0;
    uint64_t n = 0;
    if (threadIdx.x == 0)
        for (uint32_t i = 0; i < gridDim.x; ++i) {
            total += s_part[i];
            if (part_cnt) n += s_pcnt[i];
        }
    if (part_cnt) *count = n;
    return total;
}

// Two sums that travel together (k_rgb_loss: the squared error and the entropy): the same five steps on one ticket, each value with
// the order of additions stated at the top.  part0 / part1: gridDim.x slots each; s_wave: 8 entries of LDS (4 per value); s_flag: one.
__device__ __forceinline__ bool publish_and_draw2(double sum0, double sum1, uint32_t *ticket, double *part0, double *part1, double *s_wave,
                                                  uint32_t *s_flag) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    sum0 = wave_sum(sum0);
    sum1 = wave_sum(sum1);
    if (lane == 0) {
        s_wave[wave] = sum0;
        s_wave[4u + wave] = sum1;
    }
    __syncthreads();
    if (tid == 0) {
        part0[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        part1[blockIdx.x] = ((s_wave[4] + s_wave[5]) + s_wave[6]) + s_wave[7];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const uint32_t mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        *s_flag = mine == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    const bool last = *s_flag != 0u;
    if (last) __threadfence();
    return last;
}

// Step 5 and the last sums of publish_and_draw2, in the last workgroup: s_part0 / s_part1: gridDim.x entries of LDS each; the slots go
// back to zero.  Thread 0's return value (the first sum) and *second are the ones to use.
__device__ __forceinline__ double sum_partials2(double *part0, double *part1, double *s_part0, double *s_part1, double *second) {
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += SN_REDUCE_THREADS) {
        s_part0[i] = __hip_atomic_load(&part0[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_part1[i] = __hip_atomic_load(&part1[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part0[i], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part1[i], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    double t0 = 0.0, t1 = 0.0;
    if (threadIdx.x == 0)
        for (uint32_t i = 0; i < gridDim.x; ++i) {
            t0 += s_part0[i];
            t1 += s_part1[i];
        }
    *second = t1;
    return t0;
}

}  // namespace sn
