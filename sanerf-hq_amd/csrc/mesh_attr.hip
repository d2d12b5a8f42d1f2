// mesh_attr.hip — vertex colours and instance labels of an exported mesh: surface probes (sn_rm_vertex_probe_points,
// sn_rm_vertex_probe_composite), for gfx950.
//
// Definition (include/sanerf_hip.h states it in full; tests/mesh_attr_ref64.py is its fp64 twin).  A vertex v with mesh normal n (pointing
// out of the inside) is shaded the way a pixel is, by a short ray of K samples, step h, that enters the surface head-on:
//   d    = -n / |n|                                         (0, 0, -1) where |n| is 0 or not finite
//   t_i  = (i + 1/2 - K/2) h,  p_i = v + t_i d             product and sum rounded separately; contract: then sn_rm_contract's arithmetic
//   g_i  = (label_i in S) xor invert (true without labels);  y_i = g_i ? h sigma_i : 0      a select, not a product
//   w_i  = (1 - exp(-y_i)) exp(-sum_{j<i} y_j)              the prefix in fp64 in sample order, NaN -> 0: k_object_composite's weight
//   W    = sum w_i (the coverage);  g = (sum w_i geo_i) / W where W >= 2^-126, else (sum_i geo_i) (1 / K), ungated
//   f    = [g | SH4(d / |d|)], 31 values: the input of the per-ray colour head
//   vote_l = sum_{i: label_i = l} w_i (l < 32), fp32 in sample order;  vertex label = the lowest l attaining the maximum if that is > 0, else 255
//
// Shape of k_vertex_probe_composite: k_object_composite's -- 16 lanes per vertex, lane 0 owns the coverage, lane c >= 1 geometry channel
// c - 1, the transmittance scan inside, SH once per vertex -- but the kernel is bound by the 60 K bytes of geometry per vertex, and lane c
// reading channel c - 1 of one sample touches 60 bytes of four different vertices per wave instruction.  So the workgroup's 16 vertices
// own ONE contiguous block of 16 K 15 floats, which the 256 lanes read as consecutive 16-byte pieces (whole lines, every byte used once)
// into LDS, and the channel sums read it back from there.  Lane c also owns the votes of labels c and c + 16.  The order of every sum is
// a function of K alone: results do not depend on V or on the launch grid.  Plain vector loads and stores.
#include "sn_common.h"
#include "sh_basis.inc"

namespace sn {

constexpr uint32_t VA_GEO = 15;            // geometry channels of the reference field (network.py:94)
constexpr uint32_t VA_GROUP = 16;          // vertices per workgroup of 256 lanes

// d = -n / |n| without overflow or underflow of the squares: n is scaled by its largest magnitude first.
__device__ __forceinline__ void probe_direction(float nx, float ny, float nz, float &dx, float &dy, float &dz) {
    float m = fmaxf(fmaxf(fabsf(nx), fabsf(ny)), fabsf(nz));
    if (nx != nx || ny != ny || nz != nz) m = __builtin_nanf("");
    dx = 0.0f; dy = 0.0f; dz = -1.0f;
    if (!(m > 0.0f && m < __builtin_inff())) return;
    const float sx = nx / m, sy = ny / m, sz = nz / m;
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);        // in [1, sqrt 3]
    dx = -(sx / len); dy = -(sy / len); dz = -(sz / len);
}

__global__ __launch_bounds__(256) void k_vertex_probe_points(const float *__restrict__ vertices, const float *__restrict__ normals, uint32_t first,
                                                             uint32_t count, uint32_t K, float h, int contract, float *__restrict__ xyz,
                                                             float *__restrict__ dirs) {
    SN_POISON_ALL();
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;          // count * K < 2^32 (checked on the host)
    const uint32_t n = gid / K, i = gid - n * K;
    if (n >= count) return;
    const float *v = vertices + (size_t)(first + n) * 3u, *nr = normals + (size_t)(first + n) * 3u;
    float dx, dy, dz;
    probe_direction(nr[0], nr[1], nr[2], dx, dy, dz);
    const float t = ((float)i + 0.5f - (float)(K / 2u)) * h;       // the factor is exact: one rounding
    float x = v[0] + t * dx, y = v[1] + t * dy, z = v[2] + t * dz;
    if (contract) contract3(x, y, z);
    float *p = xyz + (size_t)gid * 3u;
    p[0] = x; p[1] = y; p[2] = z;
    if (i == 0u) { float *d = dirs + (size_t)n * 3u; d[0] = dx; d[1] = dy; d[2] = dz; }
}

// Value c of SH4(d / |d|), k_object_composite's arithmetic (a function of its own: the generated table is not template code).
__device__ __forceinline__ float probe_sh_of_lane(const float *__restrict__ d, uint32_t c) {
    float x = d[0], yd = d[1], z = d[2];
    const float inv = 1.0f / sqrtf(x * x + yd * yd + z * z);               // renderer.py:294
    x *= inv; const float y = yd * inv; z *= inv;
    float sh[16];
    {
        const unsigned C = 4u;
        SN_SH_POWERS
        (void)x4; (void)x5; (void)x6; (void)x7; (void)y4; (void)y5; (void)y6; (void)y7; (void)z4; (void)z5; (void)z6; (void)z7;
        SN_SH_VALUES(sh);
    }
    float mine = sh[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) mine = c == (uint32_t)k ? sh[k] : mine;
    return mine;
}

template <uint32_t K>
__global__ __launch_bounds__(256) void k_vertex_probe_composite(const uint8_t *__restrict__ labels, const float *__restrict__ sigmas,
                                                                const float *__restrict__ geo, const float *__restrict__ dirs, uint32_t V, float h,
                                                                uint32_t keep_mask, int invert, float *__restrict__ f_out,
                                                                float *__restrict__ coverage, uint8_t *__restrict__ vertex_label) {
    constexpr uint32_t ROW = K * VA_GEO;                           // floats of one vertex
    constexpr uint32_t PIECES = VA_GROUP * ROW / 4u;               // 16-byte pieces of the workgroup's block
    __shared__ float4 s_geo4[PIECES];
    SN_POISON_ALL();
    // ---- the block's geometry: consecutive 16-byte pieces, guarded by the end of the array (V K 15 floats, a multiple of 4)
    {
        const uint64_t base = (uint64_t)blockIdx.x * PIECES, total = (uint64_t)V * (ROW / 4u);
        const float4 *src = reinterpret_cast<const float4 *>(geo);
        for (uint32_t p = threadIdx.x; p < PIECES; p += 256u)
            if (base + p < total) s_geo4[p] = src[base + p];
    }
    __syncthreads();
    const float *s_geo = reinterpret_cast<const float *>(s_geo4);
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x, n_raw = gid >> 4, c = gid & 15u, slot = threadIdx.x >> 4;
    const uint32_t n = n_raw < V ? n_raw : V - 1u;
    const bool store = n_raw < V;
    const float *sg = sigmas + (size_t)n * K;
    const float *gf = s_geo + slot * ROW + (c ? c - 1u : 0u);      // (a slot past V holds stale LDS: its lanes store nothing)
    const uint8_t *lb = labels ? labels + (size_t)n * K : nullptr;
    double cum = 0.0;                      // sum of y over the samples in front of the current block of 16
    float acc = 0.0f, plain = 0.0f, vote0 = 0.0f, vote1 = 0.0f;
#pragma unroll
    for (uint32_t j0 = 0; j0 < K; j0 += 16u) {
        const uint32_t j = j0 + c;
        const bool live = j < K;
        float y = 0.0f;
        uint32_t lab = 255u;
        if (live) {
            bool gate = true;
            if (lb) {
                lab = lb[j];
                const bool in_set = lab < 32u && ((keep_mask >> lab) & 1u) != 0u;
                gate = in_set != (invert != 0);
            }
            const float ds = h * sg[j];
            y = gate ? ds : 0.0f;
        }
        double excl = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float d = __shfl(y, q, 16);
            if (c == (uint32_t)q) excl = cum;
            cum += (double)d;
        }
        float w = 0.0f;
        if (live) {
            const float alpha = 1.0f - expf_det(-y);
            const float tr = expf_det(-(float)excl);
            w = alpha * tr;
            if (w != w) w = 0.0f;
        }
        constexpr uint32_t CNT = K < 16u ? K : 16u;
#pragma unroll
        for (uint32_t q = 0; q < CNT; ++q) {
            const float wq = __shfl(w, (int)q, 16);
            const uint32_t lq = (uint32_t)__shfl((int)lab, (int)q, 16);
            if (lq == c) vote0 += wq;
            if (lq == c + 16u) vote1 += wq;
            if (c == 0u) acc += wq;
            else {
                const float gq = gf[(j0 + q) * VA_GEO];
                acc = __builtin_fmaf(wq, gq, acc);
                plain += gq;
            }
        }
    }
    const float ws = __shfl(acc, 0, 16);
    // ---- the vertex label: the lowest label attaining the largest vote (votes are never NaN and never negative)
    float best = vote0;
    uint32_t arg = c;
    if (vote1 > best) { best = vote1; arg = c + 16u; }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 16);
        const uint32_t oa = (uint32_t)__shfl_xor((int)arg, m, 16);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    // ---- SH of the probe direction, once per vertex (k_object_composite's arithmetic)
    const float mine = probe_sh_of_lane(dirs + (size_t)n * 3u, c);
    if (!store) return;
    float *f = f_out + (size_t)n * 31u;
    if (c == 0u) {
        coverage[n] = acc;
        if (vertex_label) vertex_label[n] = best > 0.0f ? (uint8_t)arg : (uint8_t)255u;
    } else {
        f[c - 1u] = ws >= 1.17549435e-38f ? acc / ws : plain * (1.0f / (float)K);
    }
    f[15u + c] = mine;
}

}  // namespace sn

using namespace sn;

extern "C" int sn_rm_vertex_probe_points(const float *vertices, const float *normals, uint32_t V_total, uint32_t first, uint32_t count, uint32_t K,
                                         float h, int32_t contract, float *xyz, float *dirs, sn_stream_t stream) {
    SN_UNSUPPORTED(K == 4u || K == 8u || K == 16u || K == 32u, "vertex_probe_points: K = %u samples (4, 8, 16 or 32)", K);
    SN_REQUIRE(h > 0.0f && h < __builtin_inff(), "vertex_probe_points: the probe step must be positive and finite");
    SN_REQUIRE((uint64_t)first + count <= V_total, "vertex_probe_points: vertices %u .. %llu outside the mesh of %u", first,
               (unsigned long long)first + count - 1u, V_total);
    if (count == 0) return SN_OK;
    SN_REQUIRE(vertices && normals && xyz && dirs, "vertex_probe_points: NULL pointer");
    SN_REQUIRE((uint64_t)count * K < (1ull << 32), "vertex_probe_points: at most 2^32 - 1 samples per call (got %u x %u)", count, K);
    hipLaunchKernelGGL(k_vertex_probe_points, dim3(div_up((uint64_t)count * K, 256)), dim3(256), 0, (hipStream_t)stream, vertices, normals, first,
                       count, K, h, (int)contract, xyz, dirs);
    SN_LAUNCH_CHECK("k_vertex_probe_points");
    return SN_OK;
}

extern "C" int sn_rm_vertex_probe_composite(const uint8_t *labels, const float *sigmas, const float *geo_feat, const float *dirs, uint32_t V, uint32_t K,
                                            float h, uint32_t keep_mask, int32_t invert, float *f, float *coverage, uint8_t *vertex_label,
                                            sn_stream_t stream) {
    SN_UNSUPPORTED(K == 4u || K == 8u || K == 16u || K == 32u, "vertex_probe_composite: K = %u samples (4, 8, 16 or 32)", K);
    SN_REQUIRE(h > 0.0f && h < __builtin_inff(), "vertex_probe_composite: the probe step must be positive and finite");
    if (V == 0) return SN_OK;
    SN_REQUIRE(sigmas && geo_feat && dirs && f && coverage, "vertex_probe_composite: NULL pointer");
    SN_REQUIRE(labels || !vertex_label, "vertex_probe_composite: vertex labels need the per-sample labels");
    SN_REQUIRE(table_aligned(geo_feat), "vertex_probe_composite: geo_feat must be 16-byte aligned");
    SN_REQUIRE((uint64_t)V * 16u < (1ull << 32), "vertex_probe_composite: at most 2^28 - 1 vertices per call (got %u)", V);
    const dim3 grid(div_up((uint64_t)V * 16u, 256)), block(256);
#define SN_VA_LAUNCH(KK)                                                                                                                  \
    hipLaunchKernelGGL(k_vertex_probe_composite<KK>, grid, block, 0, (hipStream_t)stream, labels, sigmas, geo_feat, dirs, V, h, keep_mask, \
                       (int)invert, f, coverage, vertex_label)
    if (K == 4u) SN_VA_LAUNCH(4u);
    else if (K == 8u) SN_VA_LAUNCH(8u);
    else if (K == 16u) SN_VA_LAUNCH(16u);
    else SN_VA_LAUNCH(32u);
#undef SN_VA_LAUNCH
    SN_LAUNCH_CHECK("k_vertex_probe_composite");
    return SN_OK;
}
