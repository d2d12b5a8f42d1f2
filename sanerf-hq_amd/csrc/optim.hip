// optim.hip — dense Adam over a parameter tensor in ONE pass (gfx950).
//
// The reference trains with torch.optim.Adam(model.get_params(lr), eps=1e-15) (main.py:283): dense state, every row of
// every hash table moves each step by its decaying momentum, touched or not (gridencoder/grid.py:83 hands autograd a
// dense zeros_like gradient).  A lazy / touched-rows-only update is a different optimiser, so what can be saved is the
// memory traffic of the update itself: torch's default (foreach) implementation walks the 160 MiB mask-grid state in
// ~20 multi-tensor kernels (0.77 ms per step, profiles/r02/kernel_stats_train_mask.txt); the arithmetic below is the
// single-tensor recipe of torch/optim/adam.py (_single_tensor_adam) applied once per element with 16-byte accesses:
// 4 streams read (param, grad, exp_avg, exp_avg_sq), 3 written.  Elements whose gradient and both moments are exactly
// zero -- table rows no sample has reached yet -- are left untouched (their update is exactly 0): no stores for them.
//
// Opt-in LAZY mode (flags & SN_ADAM_LAZY; SURVEY 8 f2 "fused Adam over touched table rows only"): elements whose gradient is
// exactly zero in THIS step are skipped altogether -- moments do not decay, the parameter does not coast on its momentum -- the
// semantics of torch.optim.SparseAdam with the dense gradient's non-zeros as the sparse pattern.  A different optimiser from
// the reference's (hence opt-in): a hash table of which a 4096-ray batch touches a few percent then costs a read of the
// gradient stream plus the touched elements instead of seven full streams.
#include "sn_common.h"

namespace sn {

struct AdamArgs {
    float *p, *g, *m, *v;
    uint64_t n;
    float one_minus_beta1, beta2, one_minus_beta2, step_size, inv_bc2_sqrt, eps, weight_decay;
    int zero_grad, maximize, lazy;
    const float *step_dev;        // capturable form: the step count lives on the device (a captured HIP graph replays this launch with other counts)
    double lr, beta1_d, beta2_d;  // ... and the two bias corrections are formed from it in the kernel, in double like the host path
};

__device__ __forceinline__ bool adam_one(float &p, float g, float &m, float &v, const AdamArgs &a) {
    if (a.maximize) g = -g;
    if (a.weight_decay != 0.0f) g = g + a.weight_decay * p;              // grad.add(param, alpha=weight_decay)
    if (g == 0.0f && (a.lazy || (m == 0.0f && v == 0.0f))) return false; // update is exactly zero -- or, lazy: element not touched this step
    m = m + a.one_minus_beta1 * (g - m);                                 // exp_avg.lerp_(grad, 1 - beta1), weight < 0.5 branch
    const float gg = g * g;
    v = v * a.beta2 + a.one_minus_beta2 * gg;                            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) * a.inv_bc2_sqrt + a.eps;               // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - a.step_size * (m / denom);                                   // param.addcdiv_(exp_avg, denom, value=-step_size)
    return true;
}

// SN_ADAM_ZERO_GRAD clears what is STORED, not what was updated: elements that adam_one leaves alone can still hold a non-zero gradient
// (maximize / weight decay: -+g + wd p cancelled to exactly 0 on zero moments), and an accumulating caller would add the next step's on top.
__device__ __forceinline__ bool holds_gradient(const float4 &g) { return g.x != 0.0f || g.y != 0.0f || g.z != 0.0f || g.w != 0.0f; }

__global__ __launch_bounds__(256) void k_adam(AdamArgs a) {
    SN_POISON_ALL();
    if (a.step_dev) {
        const double step = (double)*a.step_dev;
        const double bc1 = 1.0 - pow(a.beta1_d, step), bc2 = 1.0 - pow(a.beta2_d, step);
        a.step_size = (float)(a.lr / bc1);
        a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    }
    const uint64_t nq = a.n >> 2;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        float4 p = reinterpret_cast<float4 *>(a.p)[i], m = reinterpret_cast<float4 *>(a.m)[i], v = reinterpret_cast<float4 *>(a.v)[i];
        const float4 g = reinterpret_cast<const float4 *>(a.g)[i];
        bool any = adam_one(p.x, g.x, m.x, v.x, a);
        any |= adam_one(p.y, g.y, m.y, v.y, a);
        any |= adam_one(p.z, g.z, m.z, v.z, a);
        any |= adam_one(p.w, g.w, m.w, v.w, a);
        if (any) {
            reinterpret_cast<float4 *>(a.p)[i] = p; reinterpret_cast<float4 *>(a.m)[i] = m; reinterpret_cast<float4 *>(a.v)[i] = v;
        }
        if (a.zero_grad && (any || holds_gradient(g))) reinterpret_cast<float4 *>(a.g)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    // tail (n not a multiple of 4)
    const uint64_t t = (nq << 2) + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.n) {
        float p = a.p[t], m = a.m[t], v = a.v[t];
        const float g = a.g[t];
        const bool any = adam_one(p, g, m, v, a);
        if (any) {
            a.p[t] = p; a.m[t] = m; a.v[t] = v;
        }
        if (a.zero_grad && (any || g != 0.0f)) a.g[t] = 0.0f;
    }
}

// ---- many tensors, one launch (sn_adam_step_multi) ---------------------------------------------------------------------------
// The records sit in the kernel arguments (2.8 KiB of the 4 KiB limit): eager steps hand over fresh gradient addresses every step
// without a copy, a captured graph keeps them.  A chunk is 4096 floats = four 16-byte accesses per thread and stream; a workgroup
// walks chunk ids blockIdx.x, blockIdx.x + gridDim.x, ... and finds the tensor of each by scanning the prefix of chunk counts
// (ids only grow, so the scan never restarts; every value involved is uniform over the workgroup: scalar loads, no LDS).
constexpr uint32_t MULTI_CHUNK = 4096;

struct AdamMultiTensor {
    float *p, *g, *m, *v;
    uint64_t n;
    float *step_dev;              // device count (capturable form) or NULL
    double bc1;                   // host count: 1 - beta1^step, formed on the host as sn_adam_step forms it ...
    float inv_bc2_sqrt;           // ... and 1 / sqrt(1 - beta2^step)
    uint32_t group;
};
struct AdamMultiGroup {
    double lr, beta1_d, beta2_d;
    float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
    uint32_t bits;                // 1 zero_grad, 2 maximize, 4 lazy
};
struct AdamMultiArgs {
    AdamMultiTensor t[SN_ADAM_MULTI_MAX_TENSORS];
    AdamMultiGroup grp[SN_ADAM_MULTI_MAX_GROUPS];
    uint32_t first_chunk[SN_ADAM_MULTI_MAX_TENSORS + 1];
    uint32_t n_tensors;
    const float *lr_scale;
    uint32_t *ticket;
};
static_assert(sizeof(AdamMultiArgs) <= 4096, "the records must fit the kernel-argument block");
static_assert(SN_ADAM_MULTI_MAX_TENSORS <= 64, "one wave stores the new step counts");

__global__ __launch_bounds__(256) void k_adam_multi(const AdamMultiArgs a) {
    SN_POISON_ALL();
    const double lr_scale = a.lr_scale ? (double)*a.lr_scale : 1.0;
    const uint32_t total = a.first_chunk[a.n_tensors];
    uint32_t ti = 0, loaded = ~0u;
    AdamArgs s;                                                              // the tensor at hand, in the form adam_one reads
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        while (c >= a.first_chunk[ti + 1]) ++ti;
        if (ti != loaded) {
            loaded = ti;
            const AdamMultiTensor &t = a.t[ti];
            const AdamMultiGroup &g = a.grp[t.group];
            s.p = t.p; s.g = t.g; s.m = t.m; s.v = t.v; s.n = t.n;
            s.one_minus_beta1 = g.one_minus_beta1; s.beta2 = g.beta2; s.one_minus_beta2 = g.one_minus_beta2; s.eps = g.eps; s.weight_decay = g.weight_decay;
            s.zero_grad = g.bits & 1; s.maximize = (g.bits >> 1) & 1; s.lazy = (g.bits >> 2) & 1;
            const double lr = a.lr_scale ? g.lr * lr_scale : g.lr;
            double bc1 = t.bc1;
            s.inv_bc2_sqrt = t.inv_bc2_sqrt;
            if (t.step_dev) {                                                // as k_adam: both corrections from the device count, in double
                const float count = *t.step_dev;
                const double step = (double)(a.ticket ? count + 1.0f : count);
                bc1 = 1.0 - pow(g.beta1_d, step);
                s.inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow(g.beta2_d, step)));
            }
            s.step_size = (float)(lr / bc1);
        }
        const uint64_t nq = s.n >> 2;
        const uint64_t q0 = (uint64_t)(c - a.first_chunk[ti]) * (MULTI_CHUNK / 4) + threadIdx.x;
#pragma unroll
        for (uint32_t k = 0; k < MULTI_CHUNK / 4 / 256; ++k) {
            const uint64_t i = q0 + k * 256u;
            if (i < nq) {
                float4 p = reinterpret_cast<float4 *>(s.p)[i], m = reinterpret_cast<float4 *>(s.m)[i], v = reinterpret_cast<float4 *>(s.v)[i];
                const float4 g = reinterpret_cast<const float4 *>(s.g)[i];
                bool any = adam_one(p.x, g.x, m.x, v.x, s);
                any |= adam_one(p.y, g.y, m.y, v.y, s);
                any |= adam_one(p.z, g.z, m.z, v.z, s);
                any |= adam_one(p.w, g.w, m.w, v.w, s);
                if (any) {
                    reinterpret_cast<float4 *>(s.p)[i] = p; reinterpret_cast<float4 *>(s.m)[i] = m; reinterpret_cast<float4 *>(s.v)[i] = v;
                }
                if (s.zero_grad && (any || holds_gradient(g))) reinterpret_cast<float4 *>(s.g)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        // the tensor's last chunk takes the n % 4 elements behind the last whole quad
        const uint64_t e = (nq << 2) + threadIdx.x;
        if (c + 1 == a.first_chunk[ti + 1] && e < s.n) {
            float p = s.p[e], m = s.m[e], v = s.v[e];
            const float g = s.g[e];
            const bool any = adam_one(p, g, m, v, s);
            if (any) {
                s.p[e] = p; s.m[e] = m; s.v[e] = v;
            }
            if (s.zero_grad && (any || g != 0.0f)) s.g[e] = 0.0f;
        }
    }
    // Advancing the device counts: nobody may store a new count while a workgroup can still read the old one.  Each workgroup takes
    // one ticket after its last read (the barrier: all its waves are through the loop; the acq_rel add: this wave's own loads have
    // returned before the add is issued).  The workgroup whose ticket is the last one knows every other is past its reads, stores
    // count + 1 for each tensor and puts the ticket back to zero for the next launch.  Nobody waits for anybody.
    // (sn_reduce.h builds the meters' reduction on the same ticket and states the ordering argument in full.)
    if (a.ticket) {
        __syncthreads();
        if (threadIdx.x < 64) {
            uint32_t mine = 0;
            if (threadIdx.x == 0) mine = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            mine = (uint32_t)__builtin_amdgcn_readfirstlane((int)mine);
            if (mine == gridDim.x - 1) {
                if (threadIdx.x < a.n_tensors) {
                    float *count = a.t[threadIdx.x].step_dev;
                    if (count) *count = *count + 1.0f;
                }
                if (threadIdx.x == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// ---- parameter average, many tensors, one launch (sn_ema_update_multi) ---------------------------------------------------------
// torch_ema's update after the optimiser step: shadow = shadow - (shadow - param) * omd, three fp32 roundings (the build's
// -ffp-contract=off keeps them apart; no fmaf here).  12 bytes per element: two streams read, one written.  The layout is
// k_adam_multi's -- records in the kernel arguments, chunks of MULTI_CHUNK floats, the same prefix scan from chunk id to tensor, the
// same grid cap -- restated here and not shared as code: k_adam_multi stays the kernel it was.
struct EmaMultiTensor {
    float *s;
    const float *p;
    uint64_t n;
};
struct EmaMultiArgs {
    EmaMultiTensor t[SN_EMA_MULTI_MAX_TENSORS];
    uint32_t first_chunk[SN_EMA_MULTI_MAX_TENSORS + 1];
    uint32_t n_tensors;
    float omd;                    // host form: (float)(1 - decay)
    double decay;
    uint64_t *count;              // device form: torch_ema's num_updates, read when the kernel runs -- or NULL
    uint32_t *ticket;             // given: the last workgroup stores count + 1
};
static_assert(sizeof(EmaMultiArgs) <= 4096, "the records must fit the kernel-argument block");

__device__ __forceinline__ float ema_one(float s, float p, float omd) {
    const float tmp = s - p;                                                 // tmp = s_param - param
    const float scaled = tmp * omd;                                          // tmp.mul_(one_minus_decay)
    float r = s - scaled;                                                    // s_param.sub_(tmp)
    // The contract is the bit pattern of that statement as torch evaluates it on the host, and IEEE 754 leaves open WHICH NaN an
    // operation delivers.  The host's SSE / AVX units deliver the first NaN operand, quieted, and 0xffc00000 where an operation
    // without a NaN operand is invalid (inf - inf, inf * 0); gfx950 delivers 0x7fc00000 there (measured: the only elements of the
    // bit-equality test that differed).  So a NaN result is restated as the host forms it; every other result is untouched.
    if (r != r) {
        const float first = s != s ? s : p;                                  // (omd is never NaN)
        r = first != first ? __uint_as_float(__float_as_uint(first) | 0x00400000u) : __uint_as_float(0xffc00000u);
    }
    return r;
}

__global__ __launch_bounds__(256) void k_ema_multi(const EmaMultiArgs a) {
    SN_POISON_ALL();
    float omd = a.omd;
    uint64_t n = 0;
    if (a.count) {                                                           // decay = min(decay, (1 + n) / (10 + n)), as Python forms it: in double
        n = __hip_atomic_load(a.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        const double warm = (1.0 + (double)n) / (10.0 + (double)n);
        const double d = warm < a.decay ? warm : a.decay;
        omd = (float)(1.0 - d);
    }
    const uint32_t total = a.first_chunk[a.n_tensors];
    uint32_t ti = 0;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        while (c >= a.first_chunk[ti + 1]) ++ti;
        const EmaMultiTensor &t = a.t[ti];
        float *s = t.s;
        const float *p = t.p;
        const uint64_t nq = t.n >> 2;
        const uint64_t q0 = (uint64_t)(c - a.first_chunk[ti]) * (MULTI_CHUNK / 4) + threadIdx.x;
        // all eight loads of the chunk first (the compiler may not move a load of p above a store to s on its own), then the stores
        constexpr uint32_t Q = MULTI_CHUNK / 4 / 256;
        float4 sv[Q], pv[Q];
#pragma unroll
        for (uint32_t k = 0; k < Q; ++k) {
            const uint64_t i = q0 + k * 256u;
            if (i < nq) {
                sv[k] = reinterpret_cast<const float4 *>(s)[i];
                pv[k] = reinterpret_cast<const float4 *>(p)[i];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < Q; ++k) {
            const uint64_t i = q0 + k * 256u;
            if (i < nq) {
                float4 r;
                r.x = ema_one(sv[k].x, pv[k].x, omd); r.y = ema_one(sv[k].y, pv[k].y, omd);
                r.z = ema_one(sv[k].z, pv[k].z, omd); r.w = ema_one(sv[k].w, pv[k].w, omd);
                reinterpret_cast<float4 *>(s)[i] = r;
            }
        }
        // the tensor's last chunk takes the n % 4 elements behind the last whole quad
        const uint64_t e = (nq << 2) + threadIdx.x;
        if (c + 1 == a.first_chunk[ti + 1] && e < t.n) s[e] = ema_one(s[e], p[e], omd);
    }
    // Advancing the count: k_adam_multi's ticket -- each workgroup draws one after its read of the count, the one that draws the last
    // knows that all the others are past theirs, stores n and puts the ticket back to zero; nobody waits -- with a lighter draw.
    // What has to hold is that no USED read of the count comes after the store.  The count is read and stored with relaxed agent-scope
    // atomic accesses (no data race; neither L1 nor the scalar cache serves them).  A wave that stores a shadow element has its count
    // by then -- the value is in omd, which every stored element carries -- so it has it before it reaches the barrier, and thread 0
    // draws behind the barrier.  (A wave with nothing to store never uses what it read.)  The draws are read-modify-writes of one
    // word, totally ordered where they execute; the store of n depends on the value the last draw returned, so it is issued after
    // every other workgroup's draw.  Nothing is PUBLISHED through the ticket -- the shadows reach the next launch through the end of
    // this one -- so the agent-scope release of k_adam_multi's acq_rel draw, a write-back of the XCD's L2 just filled with 16 KiB of
    // shadow lines per workgroup, is left out: it cost 0.08 ms of the 0.14 ms of an update of the RGB-mode model
    // (profiles/r07/README.md).
    if (a.ticket) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t mine = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mine == gridDim.x - 1) {
                __hip_atomic_store(a.count, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

}  // namespace sn

using namespace sn;

extern "C" int sn_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, uint64_t n, double lr, double beta1, double beta2,
                            double eps, double weight_decay, uint32_t step, const float *step_device, int maximize, int flags, sn_stream_t stream) {
    if (n == 0) return SN_OK;
    SN_REQUIRE(param && grad && exp_avg && exp_avg_sq, "adam_step: param/grad/exp_avg/exp_avg_sq must be device pointers");
    SN_REQUIRE(table_aligned(param) && table_aligned(grad) && table_aligned(exp_avg) && table_aligned(exp_avg_sq), "adam_step: tensors must be 16-byte aligned");
    SN_REQUIRE(step >= 1 || step_device, "adam_step: step counts from 1");
    SN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && lr >= 0.0 && eps >= 0.0, "adam_step: invalid hyper-parameters");
    // scalars exactly as torch/optim/adam.py computes them: Python doubles (hence double arguments: 1 - beta2 formed from a
    // float beta2 is off by 1e-5 relative), rounded to fp32 where they meet the tensors
    const double hstep = step_device ? 1.0 : (double)step;             // (device step: the kernel recomputes both corrections)
    const double bc1 = 1.0 - pow(beta1, hstep), bc2 = 1.0 - pow(beta2, hstep);
    AdamArgs a;
    a.step_dev = step_device; a.lr = lr; a.beta1_d = beta1; a.beta2_d = beta2;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
    a.one_minus_beta1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.one_minus_beta2 = (float)(1.0 - beta2);
    a.step_size = (float)(lr / bc1);
    a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    a.eps = (float)eps; a.weight_decay = (float)weight_decay; a.zero_grad = flags & SN_ADAM_ZERO_GRAD; a.maximize = maximize;
    a.lazy = (flags & SN_ADAM_LAZY) ? 1 : 0;
    SN_REQUIRE(!(a.lazy && weight_decay != 0.0), "adam_step: lazy mode is defined for weight_decay = 0 (a decayed zero gradient is not a skipped element)");
    const uint64_t nq = n >> 2;
    uint64_t blocks = (nq + 255) / 256;
    if (blocks > 256u * 16u) blocks = 256u * 16u;                         // 16 workgroups per CU, grid-stride beyond
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_adam, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_adam");
    return SN_OK;
}

extern "C" int sn_adam_step_multi(const sn_adam_tensor *tensors, uint32_t n_tensors, const sn_adam_group *groups, uint32_t n_groups,
                                  const float *lr_scale_device, uint32_t *ticket, sn_stream_t stream) {
    SN_REQUIRE(n_tensors <= SN_ADAM_MULTI_MAX_TENSORS, "adam_step_multi: %u tensors, at most %d per call (split the model into several calls)", n_tensors, SN_ADAM_MULTI_MAX_TENSORS);
    SN_REQUIRE(n_groups <= SN_ADAM_MULTI_MAX_GROUPS, "adam_step_multi: %u groups, at most %d per call", n_groups, SN_ADAM_MULTI_MAX_GROUPS);
    if (n_tensors == 0) return SN_OK;
    SN_REQUIRE(tensors && groups && n_groups >= 1, "adam_step_multi: tensors and groups must be host arrays");
    SN_REQUIRE((reinterpret_cast<uintptr_t>(lr_scale_device) & 3u) == 0 && (reinterpret_cast<uintptr_t>(ticket) & 3u) == 0, "adam_step_multi: lr_scale_device / ticket must be 4-byte aligned");
    AdamMultiArgs a = {};
    for (uint32_t j = 0; j < n_groups; ++j) {
        const sn_adam_group &g = groups[j];
        SN_REQUIRE(g.beta1 >= 0.0 && g.beta1 < 1.0 && g.beta2 >= 0.0 && g.beta2 < 1.0 && g.lr >= 0.0 && g.eps >= 0.0, "adam_step_multi: invalid hyper-parameters (group %u)", j);
        SN_REQUIRE(!((g.flags & SN_ADAM_LAZY) && g.weight_decay != 0.0), "adam_step_multi: lazy mode is defined for weight_decay = 0 (a decayed zero gradient is not a skipped element)");
        AdamMultiGroup &d = a.grp[j];
        d.lr = g.lr; d.beta1_d = g.beta1; d.beta2_d = g.beta2;
        d.one_minus_beta1 = (float)(1.0 - g.beta1); d.beta2 = (float)g.beta2; d.one_minus_beta2 = (float)(1.0 - g.beta2);
        d.eps = (float)g.eps; d.weight_decay = (float)g.weight_decay;
        d.bits = ((g.flags & SN_ADAM_ZERO_GRAD) ? 1u : 0u) | (g.maximize ? 2u : 0u) | ((g.flags & SN_ADAM_LAZY) ? 4u : 0u);
    }
    uint64_t chunks = 0;
    for (uint32_t i = 0; i < n_tensors; ++i) {
        const sn_adam_tensor &t = tensors[i];
        SN_REQUIRE(t.group < n_groups, "adam_step_multi: tensor %u names group %u of %u", i, t.group, n_groups);
        if (t.n) {
            SN_REQUIRE(t.param && t.grad && t.exp_avg && t.exp_avg_sq, "adam_step_multi: param/grad/exp_avg/exp_avg_sq must be device pointers (tensor %u)", i);
            SN_REQUIRE(table_aligned(t.param) && table_aligned(t.grad) && table_aligned(t.exp_avg) && table_aligned(t.exp_avg_sq), "adam_step_multi: tensors must be 16-byte aligned (tensor %u)", i);
        }
        SN_REQUIRE(t.step >= 1 || t.step_device, "adam_step_multi: step counts from 1 (tensor %u)", i);
        SN_REQUIRE((reinterpret_cast<uintptr_t>(t.step_device) & 3u) == 0, "adam_step_multi: step_device must be 4-byte aligned (tensor %u)", i);
        for (uint32_t k = 0; k < i && t.step_device; ++k)
            SN_REQUIRE(tensors[k].step_device != t.step_device, "adam_step_multi: tensors %u and %u share one device step count", k, i);
        const sn_adam_group &g = groups[t.group];
        const double hstep = t.step_device ? 1.0 : (double)t.step;       // (device count: the kernel recomputes both corrections)
        AdamMultiTensor &d = a.t[i];
        d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq; d.n = t.n; d.step_dev = t.step_device; d.group = t.group;
        d.bc1 = 1.0 - pow(g.beta1, hstep);
        d.inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow(g.beta2, hstep)));
        a.first_chunk[i] = (uint32_t)chunks;
        chunks += (t.n + MULTI_CHUNK - 1) / MULTI_CHUNK;
        SN_REQUIRE(chunks < (1ull << 31), "adam_step_multi: more than 2^43 elements in one call");
    }
    a.first_chunk[n_tensors] = (uint32_t)chunks;
    a.n_tensors = n_tensors; a.lr_scale = lr_scale_device; a.ticket = ticket;
    if (chunks == 0 && !ticket) return SN_OK;
    uint64_t blocks = chunks;
    if (blocks > 256u * 16u) blocks = 256u * 16u;                         // 16 workgroups per CU, grid-stride beyond
    if (blocks == 0) blocks = 1;                                          // nothing to update, counts to advance
    hipLaunchKernelGGL(k_adam_multi, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_adam_multi");
    return SN_OK;
}

extern "C" int sn_ema_update_multi(const sn_ema_tensor *tensors, uint32_t n_tensors, double decay, uint64_t *num_updates_device,
                                   uint32_t *ticket, int flags, sn_stream_t stream) {
    const bool advance = (flags & SN_EMA_ADVANCE) != 0;
    SN_REQUIRE(n_tensors <= SN_EMA_MULTI_MAX_TENSORS, "ema_update_multi: %u tensors, at most %d per call (split the model into several calls)", n_tensors, SN_EMA_MULTI_MAX_TENSORS);
    SN_REQUIRE((flags & ~SN_EMA_ADVANCE) == 0, "ema_update_multi: unknown flags 0x%x", (unsigned)flags);
    SN_REQUIRE(decay >= 0.0 && decay <= 1.0, "ema_update_multi: decay must lie in [0, 1]");
    SN_REQUIRE(!advance || num_updates_device, "ema_update_multi: SN_EMA_ADVANCE needs num_updates_device (there is no count to advance)");
    SN_REQUIRE(!advance || ticket, "ema_update_multi: SN_EMA_ADVANCE needs a ticket");
    SN_REQUIRE((reinterpret_cast<uintptr_t>(num_updates_device) & 7u) == 0, "ema_update_multi: num_updates_device must be 8-byte aligned");
    SN_REQUIRE((reinterpret_cast<uintptr_t>(ticket) & 3u) == 0, "ema_update_multi: ticket must be 4-byte aligned");
    SN_REQUIRE(tensors || n_tensors == 0, "ema_update_multi: tensors must be a host array");
    EmaMultiArgs a = {};
    uint64_t chunks = 0;
    for (uint32_t i = 0; i < n_tensors; ++i) {
        const sn_ema_tensor &t = tensors[i];
        if (t.n) {
            SN_REQUIRE(t.shadow && t.param, "ema_update_multi: shadow/param must be device pointers (tensor %u)", i);
            SN_REQUIRE(table_aligned(t.shadow) && table_aligned(t.param), "ema_update_multi: tensors must be 16-byte aligned (tensor %u)", i);
            SN_REQUIRE(t.shadow != t.param, "ema_update_multi: shadow and param are the same tensor (tensor %u)", i);
        }
        EmaMultiTensor &d = a.t[i];
        d.s = t.shadow; d.p = t.param; d.n = t.n;
        a.first_chunk[i] = (uint32_t)chunks;
        chunks += (t.n + MULTI_CHUNK - 1) / MULTI_CHUNK;
        SN_REQUIRE(chunks < (1ull << 31), "ema_update_multi: more than 2^43 elements in one call");
    }
    a.first_chunk[n_tensors] = (uint32_t)chunks;
    a.n_tensors = n_tensors;
    a.decay = decay;
    a.omd = (float)(1.0 - decay);
    a.count = num_updates_device;
    a.ticket = advance ? ticket : nullptr;                                // (a ticket without SN_EMA_ADVANCE is not touched)
    if (chunks == 0 && !advance) return SN_OK;
    uint64_t blocks = chunks;
    if (blocks > 256u * 16u) blocks = 256u * 16u;                         // k_adam_multi's cap: 16 workgroups per CU, grid-stride beyond
    if (blocks == 0) blocks = 1;                                          // nothing to update, a count to advance
    hipLaunchKernelGGL(k_ema_multi, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_ema_multi");
    return SN_OK;
}
