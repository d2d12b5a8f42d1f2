// collate.hip — a training batch drawn on the device, for gfx950: the device-side core of the reference's NeRFDataset.collate
// (provider.py:894-1114) as two entry points whose launches can be captured in a HIP graph in front of render -> loss -> Adam.
//   sn_rm_weighted_draw     weighted sampling without replacement (torch.multinomial's exponential race, utils.py:218, :248) from
//                           caller-supplied exponential variates: the n smallest (expo / weight, cell) of a row, in ascending cell order
//   sn_rm_collate_gather    camera choice, pixel draws, rays and every supervision gather (provider.py:908-1068, utils.py:209-300)
//                           written straight into caller-owned tensors, one lane per ray, main part and local patches in one launch
//
// Conventions of mask_output.hip / prompts.hip: division is IEEE-rounded, every fused multiply-add is an explicit fmaf, no float atomics,
// nothing synchronises, nothing is read on the host: a batch is a pure function of (dataset, random tensors) and two runs give the same bits.
//
// Draw: one workgroup of 256 threads per row.  A selectable key is a non-negative finite float, so keys order as their bit patterns.
// n == 1 (the local-patch centres): the minimum of (key bits, cell) through a fixed xor butterfly.  n > 1: a most-significant-digit
// radix select on the key bits -- four 8-bit passes, each a 256-bin histogram in LDS (integer LDS atomics: counts do not depend on the
// order of arrival) and a scan of the bins that narrows (prefix, rank) -- leaves the threshold key T and how many cells that tie at T
// belong to the draw; ties go to the smaller cell.  One order-preserving compaction pass then walks the row in chunks of 256 cells: the
// lanes below T, and the tying lanes below the tie quota, are ranked by ballot + mbcnt above a running base (the slot dealing of
// prompts.hip and render.hip), so the cells leave in ascending order with one writer each.  Keys are recomputed from global memory in
// every pass: a row is at most 64 KiB of weights and 64 KiB of variates and stays in L2; no key array sits in LDS.
#include "sn_common.h"

namespace sn {

constexpr uint32_t CD_THREADS = 256;
constexpr uint32_t CD_MAX_C = SN_DRAW_MAX_CELLS;
constexpr uint32_t CD_NONE = 0xffffffffu;            // an unselectable cell: above every key
constexpr uint32_t CD_INF = 0x7f800000u;             // every selectable key is below

// min((int)(u * n), n - 1) with the product in fp32; the min guards the upper end, and a u outside [0, 1) or a NaN, which a caller's
// torch.rand never produces, lands inside 0 .. n-1 instead of indexing out of bounds.
__device__ __forceinline__ uint32_t pick(float u, uint32_t n) {
    const float f = u * (float)n;
    return f >= 0.0f ? (f < (float)n ? (uint32_t)f : n - 1u) : 0u;
}
// trunc(f) clamped into 0 .. n-1 (NaN -> 0)
__device__ __forceinline__ uint32_t trunc_below(float f, uint32_t n) { return f >= 0.0f ? (f < (float)n ? (uint32_t)f : n - 1u) : 0u; }

// The row of `weights` that row r draws from: itself, the camera its uniform variate picks, or an entry of an index table (clamped)
__device__ __forceinline__ uint32_t source_row(const float *__restrict__ row_u, const int64_t *__restrict__ row_index, uint32_t M, uint32_t r) {
    if (row_index) { const int64_t i = row_index[r]; return i < 0 ? 0u : i >= (int64_t)M ? M - 1u : (uint32_t)i; }
    return row_u ? pick(row_u[r], M) : r;
}

// The key of a cell as its bit pattern; CD_NONE for a cell that is never selected: weight <= 0 or NaN, key not finite, key negative.
__device__ __forceinline__ uint32_t draw_key(const float *__restrict__ w, const float *__restrict__ e, uint32_t c) {
    const float wt = w[c];
    const float key = e[c] / wt;
    const uint32_t b = key == 0.0f ? 0u : __float_as_uint(key);      // -0 is 0
    return (wt > 0.0f && b < CD_INF) ? b : CD_NONE;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

// ---- draw, n == 1 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_weighted_draw_one(const float *__restrict__ weights, const float *__restrict__ expo, uint32_t C,
                                                           const float *__restrict__ row_u, const int64_t *__restrict__ row_index, uint32_t M, int64_t *__restrict__ out,
                                                           int32_t *__restrict__ status) {
    SN_POISON_ALL();
    __shared__ uint32_t s_key[4], s_cell[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = blockIdx.x;
    const float *w = weights + (size_t)source_row(row_u, row_index, M, r) * C, *e = expo + (size_t)r * C;
    uint32_t bk = CD_NONE, bc = CD_NONE;
    for (uint32_t c = tid; c < C; c += CD_THREADS) {                 // ascending cells: a later equal key does not replace an earlier one
        const uint32_t b = draw_key(w, e, c);
        if (b < bk) { bk = b; bc = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)bk, off), oc = (uint32_t)__shfl_xor((int)bc, off);
        if (ok < bk || (ok == bk && oc < bc)) { bk = ok; bc = oc; }
    }
    if (lane == 0) { s_key[wave] = bk; s_cell[wave] = bc; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (uint32_t v = 1; v < 4; ++v) {
            const uint32_t ok = s_key[v], oc = s_cell[v];
            if (ok < bk || (ok == bk && oc < bc)) { bk = ok; bc = oc; }
        }
        out[r] = bk == CD_NONE ? -1 : (int64_t)bc;
        if (bk == CD_NONE) *status = 1;
    }
}

// ---- draw, n > 1 --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_weighted_draw(const float *__restrict__ weights, const float *__restrict__ expo, uint32_t C, uint32_t n,
                                                       const float *__restrict__ row_u, const int64_t *__restrict__ row_index, uint32_t M, int64_t *__restrict__ out,
                                                       int32_t *__restrict__ status) {
    SN_POISON_ALL();
    __shared__ uint32_t s_hist[256], s_wave[4], s_pick[4][2], s_cnt[2][8];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = blockIdx.x;
    const float *w = weights + (size_t)source_row(row_u, row_index, M, r) * C, *e = expo + (size_t)r * C;
    if (tid < 4u) s_pick[tid][0] = 256u;                             // no bin picked
    uint32_t prefix = 0u, k = n;                                     // the k-th smallest of the keys that start with `prefix`
    bool short_row = false;
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        const uint32_t shift = 24u - 8u * pass;
        const uint32_t himask = pass == 0u ? 0u : 0xffffffffu << (shift + 8u);
        s_hist[tid] = 0u;
        __syncthreads();
        for (uint32_t c = tid; c < C; c += CD_THREADS) {
            const uint32_t b = draw_key(w, e, c);
            if (b != CD_NONE && (b & himask) == prefix) atomicAdd(&s_hist[(b >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t v = s_hist[tid];
        uint32_t inc = v;                                            // inclusive scan of the 256 bins: per wave, then the wave totals
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, off);
            if (lane >= off) inc += t;
        }
        if (lane == 63u) s_wave[wave] = inc;
        __syncthreads();
#pragma unroll
        for (uint32_t v2 = 0; v2 < 4u; ++v2) inc += v2 < wave ? s_wave[v2] : 0u;
        const uint32_t exc = inc - v;
        if (exc < k && k <= inc) { s_pick[pass][0] = tid; s_pick[pass][1] = k - exc; }      // at most one bin
        __syncthreads();
        const uint32_t d = s_pick[pass][0];
        if (d == 256u) { short_row = true; break; }                  // fewer than n selectable cells (uniform; only pass 0 can find it)
        prefix |= d << shift;
        k = s_pick[pass][1];
    }
    // keys below T are in, and the first `quota` cells whose key is T.  A short row takes every selectable cell.
    const uint32_t T = short_row ? CD_INF : prefix, quota = short_row ? 0u : k;
    int64_t *o = out + (size_t)r * n;
    uint32_t base_lt = 0u, base_tie = 0u;
    const uint32_t chunks = (C + CD_THREADS - 1u) / CD_THREADS;
    for (uint32_t ch = 0; ch < chunks; ++ch) {                       // whole chunks: every lane reaches the ballots and the barrier
        const uint32_t c = ch * CD_THREADS + tid, buf = ch & 1u;
        const uint32_t b = c < C ? draw_key(w, e, c) : CD_NONE;
        const bool lt = b < T, tie = b == T;
        const uint64_t m_lt = __ballot(lt), m_tie = __ballot(tie);
        if (lane == 0) { s_cnt[buf][wave] = (uint32_t)__popcll(m_lt); s_cnt[buf][4u + wave] = (uint32_t)__popcll(m_tie); }
        __syncthreads();                                             // two buffers: the next chunk's counts do not overtake this chunk's readers
        uint32_t lt_before = base_lt + lanes_below(m_lt), tie_before = base_tie + lanes_below(m_tie);
#pragma unroll
        for (uint32_t v = 0; v < 4u; ++v) {
            const uint32_t a = s_cnt[buf][v], t = s_cnt[buf][4u + v];
            lt_before += v < wave ? a : 0u; tie_before += v < wave ? t : 0u;
            base_lt += a; base_tie += t;
        }
        const uint32_t slot = lt_before + umin(tie_before, quota);
        if ((lt || (tie && tie_before < quota)) && slot < n) o[slot] = (int64_t)c;      // slot < n by construction; the test costs nothing
    }
    const uint32_t total = base_lt + umin(base_tie, quota);
    for (uint32_t j = total + tid; j < n; j += CD_THREADS) o[j] = -1;
    if (tid == 0 && total < n) *status = 1;
}

// ---- gather -------------------------------------------------------------------------------------------------------------------------
struct GatherArgs {
    sn_collate_desc d;
    float sx, sy;                    // (float)((double)H / S), (float)((double)W / S): cell -> pixel
    float ej, ei;                    // (float)((double)S / H), (float)((double)S / W): pixel -> error-map cell
    float cj, ci;                    // the same for coarse_size: pixel -> inds_coarse
    uint32_t main_blocks;
};

// One ray's outputs.  The ray arithmetic is k_rays_from_pixels' (raymarch.hip), operation for operation.
__device__ __forceinline__ void emit(const sn_collate_desc &d, const GatherArgs &a, uint32_t o, uint32_t cam, uint32_t row, uint32_t col, bool valid,
                                     int64_t coarse, bool main_part) {
    const float *m = d.poses + (size_t)cam * 16;
    const float *k4 = d.intrinsics + (d.n_intrinsics > 1u ? (size_t)cam * 4 : 0);
    const float nan = __builtin_nanf("");
    if (d.rays_o || d.rays_d) {
        const float i = (float)col + 0.5f, j = (float)row + 0.5f;
        const float xs = (i - k4[2]) / k4[0];
        const float ys = -(j - k4[3]) / k4[1];
        const float zs = -1.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float acc = xs * m[k * 4 + 0];
            acc = __builtin_fmaf(ys, m[k * 4 + 1], acc);
            acc = __builtin_fmaf(zs, m[k * 4 + 2], acc);
            if (d.rays_d) d.rays_d[(size_t)o * d.rays_d_stride + k] = valid ? acc : nan;
            if (d.rays_o) d.rays_o[(size_t)o * d.rays_o_stride + k] = valid ? m[k * 4 + 3] : nan;
        }
    }
    if (d.index_out) d.index_out[(size_t)o * d.index_stride] = (int64_t)cam;
    if (d.i_out) d.i_out[(size_t)o * d.i_stride] = valid ? (int64_t)col : -1;
    if (d.j_out) d.j_out[(size_t)o * d.j_stride] = valid ? (int64_t)row : -1;
    if (d.inds_coarse) d.inds_coarse[(size_t)o * d.inds_coarse_stride] = valid ? coarse : -1;
    const size_t pixel = ((size_t)cam * d.H + row) * d.W + col;
    if (d.images_out && main_part) {
        const uint8_t *px = d.images + pixel * d.image_channels;
        for (uint32_t c = 0; c < d.image_channels; ++c) d.images_out[(size_t)o * d.images_stride + c] = valid ? (float)px[c] / 255.0f : nan;
    }
    if (d.masks_out) {
        const size_t src = pixel * d.mask_channels, dst = (size_t)o * d.masks_stride;
        for (uint32_t c = 0; c < d.mask_channels; ++c) {             // raw bytes: int64, float32 and uint8 masks alike; an undrawn ray gets zeros
            if (d.mask_elem_bytes == 8u) ((uint64_t *)d.masks_out)[dst + c] = valid ? ((const uint64_t *)d.masks)[src + c] : 0ull;
            else if (d.mask_elem_bytes == 4u) ((uint32_t *)d.masks_out)[dst + c] = valid ? ((const uint32_t *)d.masks)[src + c] : 0u;
            else ((uint8_t *)d.masks_out)[dst + c] = valid ? ((const uint8_t *)d.masks)[src + c] : (uint8_t)0;
        }
    }
    if (d.error_maps_out) {
        const uint32_t gj = umin((uint32_t)((float)row * a.ej), d.S - 1u), gi = umin((uint32_t)((float)col * a.ei), d.S - 1u);
        d.error_maps_out[(size_t)o * d.error_maps_stride] = valid ? d.error_map[(size_t)cam * d.S * d.S + (size_t)gj * d.S + gi] : nan;
    }
    if (d.cam_near_far_out) {
#pragma unroll
        for (int k = 0; k < 2; ++k) d.cam_near_far_out[(size_t)o * d.cam_near_far_stride + k] = d.cam_near_far[(size_t)cam * 2 + k];
    }
    if (d.poses_out) {
#pragma unroll
        for (int k = 0; k < 16; ++k) d.poses_out[(size_t)o * d.poses_stride + k] = m[k];
    }
    if (d.intrinsics_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) d.intrinsics_out[(size_t)o * d.intrinsics_stride + k] = k4[k];
    }
}

__global__ __launch_bounds__(256) void k_collate_gather(const GatherArgs a) {
    SN_POISON_ALL();
    const sn_collate_desc &d = a.d;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < a.main_blocks) {                                // the main part: N rays
        const uint32_t n = blockIdx.x * 256u + tid;
        if (n >= d.N) return;
        uint32_t cam, row, col;
        bool valid = true;
        int64_t coarse;
        if (d.mode == SN_COLLATE_UNIFORM) {                          // provider.py:910, utils.py:260: one camera and one pixel per ray
            cam = pick(d.u[3 * (size_t)n], d.M);
            row = pick(d.u[3 * (size_t)n + 1], d.H);
            col = pick(d.u[3 * (size_t)n + 2], d.W);
            coarse = (int64_t)((float)row * a.cj) * (int64_t)d.coarse_size + (int64_t)((float)col * a.ci);      // utils.py:294-300
        } else {                                                     // utils.py:247-256: a pixel inside the drawn error-map cell
            const int64_t ix = d.index_dev ? *d.index_dev : (int64_t)d.index;
            cam = ix < 0 ? 0u : ix >= (int64_t)d.M ? d.M - 1u : (uint32_t)ix;
            const int64_t cell = d.cells[n];
            valid = cell >= 0 && cell < (int64_t)d.S * d.S;
            const uint32_t cl = valid ? (uint32_t)cell : 0u, gx = cl / d.S, gy = cl - gx * d.S;
            const float fx = (float)gx * a.sx, ux = d.u[2 * (size_t)n] * a.sx, fy = (float)gy * a.sy, uy = d.u[2 * (size_t)n + 1] * a.sy;
            row = trunc_below(fx + ux, d.H);
            col = trunc_below(fy + uy, d.W);
            coarse = cell;
        }
        emit(d, a, n, cam, row, col, valid, coarse, true);
    } else {                                                         // provider.py:982-993, utils.py:217-244: L patches of p x p rays
        const uint32_t t = (blockIdx.x - a.main_blocks) * 256u + tid, pp = d.p * d.p;
        if (t >= d.L * pp) return;
        const uint32_t k = t / pp, r = t - k * pp, di = r / d.p, dj = r - di * d.p;      // meshgrid(indexing="ij") order
        const uint32_t cam = pick(d.ul[k], d.M);
        const int64_t cell = d.centres[k];
        const bool valid = cell >= 0 && cell < (int64_t)d.S * d.S;
        const uint32_t cl = valid ? (uint32_t)cell : 0u, cx = cl / d.S, cy = cl - cx * d.S;
        // the reference scales both cell coordinates to pixels, takes half a patch off and clamps so that the patch stays inside
        const float half = (float)(d.p / 2u);
        const float fx = (float)cx * a.sx - half, fy = (float)cy * a.sy - half;
        const float hx = (float)(d.H - d.p - 1u), hy = (float)(d.W - d.p - 1u);
        const uint32_t row = (uint32_t)fminf(fmaxf(fx, 0.0f), hx) + di, col = (uint32_t)fminf(fmaxf(fy, 0.0f), hy) + dj;
        const int64_t coarse = (int64_t)((float)row * a.cj) * (int64_t)d.coarse_size + (int64_t)((float)col * a.ci);
        emit(d, a, d.N + t, cam, row, col, valid, coarse, false);
    }
}

}  // namespace sn

using namespace sn;

extern "C" {

int sn_rm_weighted_draw(const float *weights, const float *expo, uint32_t R, uint32_t C, uint32_t n, const float *row_u, const int64_t *row_index, uint32_t M, int64_t *out,
                        int32_t *status, sn_stream_t stream) {
    if (R == 0) return SN_OK;
    SN_REQUIRE(weights && expo && out && status, "weighted_draw: NULL pointer (weights, expo, out and status are all needed)");
    SN_REQUIRE(C >= 1, "weighted_draw: rows of 0 cells");
    SN_UNSUPPORTED(C <= CD_MAX_C, "weighted_draw: at most %u cells per row (got C=%u)", CD_MAX_C, C);
    SN_REQUIRE(n >= 1, "weighted_draw: n = 0 draws");
    SN_REQUIRE(n <= C, "weighted_draw: n=%u draws without replacement from C=%u cells", n, C);
    SN_REQUIRE(!(row_u && row_index), "weighted_draw: both row_u and row_index given (one table chooses the rows)");
    SN_REQUIRE(!(row_u || row_index) || M >= 1, "weighted_draw: a row table with M = 0 rows of weights");
    SN_UNSUPPORTED(R < (1u << 16) && (!row_u || M < (1u << 24)), "weighted_draw: R must stay below 2^16 and M below 2^24 (got R=%u, M=%u)", R, M);
    if (n == 1)
        hipLaunchKernelGGL(k_weighted_draw_one, dim3(R), dim3(CD_THREADS), 0, (hipStream_t)stream, weights, expo, C, row_u, row_index, M, out, status);
    else
        hipLaunchKernelGGL(k_weighted_draw, dim3(R), dim3(CD_THREADS), 0, (hipStream_t)stream, weights, expo, C, n, row_u, row_index, M, out, status);
    SN_LAUNCH_CHECK("k_weighted_draw");
    return SN_OK;
}

int sn_rm_collate_gather(const sn_collate_desc *desc, sn_stream_t stream) {
    SN_REQUIRE(desc, "collate_gather: NULL descriptor");
    const sn_collate_desc &d = *desc;
    const uint64_t local = (uint64_t)d.L * d.p * d.p, total = (uint64_t)d.N + local;
    if (total == 0) return SN_OK;
    SN_REQUIRE(d.poses && d.intrinsics, "collate_gather: NULL poses / intrinsics");
    SN_REQUIRE(d.M >= 1 && d.H >= 1 && d.W >= 1, "collate_gather: %u images of %u x %u pixels", d.M, d.H, d.W);
    SN_REQUIRE(d.n_intrinsics == 1 || d.n_intrinsics == d.M, "collate_gather: %u intrinsics for %u images (1 or M)", d.n_intrinsics, d.M);
    SN_UNSUPPORTED(d.M < (1u << 24) && d.H < (1u << 24) && d.W < (1u << 24), "collate_gather: M, H and W must stay below 2^24 (got %u, %u, %u)", d.M, d.H, d.W);
    SN_UNSUPPORTED(total < (1ull << 31), "collate_gather: N + L * p * p must stay below 2^31");
    SN_REQUIRE(d.mode == SN_COLLATE_UNIFORM || d.mode == SN_COLLATE_ERROR_MAP, "collate_gather: mode %d (0 uniform, 1 error map)", d.mode);
    const bool need_s = d.mode == SN_COLLATE_ERROR_MAP || d.L > 0 || d.error_maps_out;
    if (need_s) {
        SN_REQUIRE(d.S >= 1, "collate_gather: an error map of size S = 0");
        SN_UNSUPPORTED(d.S <= 32768, "collate_gather: S at most 32768 (got %u)", d.S);
    }
    if (d.N > 0) {
        SN_REQUIRE(d.u, "collate_gather: NULL u for N=%u rays", d.N);
        if (d.mode == SN_COLLATE_ERROR_MAP) {
            SN_REQUIRE(d.cells, "collate_gather: NULL cells in error-map mode");
            SN_REQUIRE(d.index_dev || (d.index >= 0 && (uint32_t)d.index < d.M), "collate_gather: image index %d outside the %u images", d.index, d.M);
        }
    }
    if (d.L > 0) {
        SN_REQUIRE(d.ul && d.centres, "collate_gather: NULL ul / centres for L=%u patches", d.L);
        SN_REQUIRE(d.p >= 1, "collate_gather: patches of 0 x 0 rays");
        SN_REQUIRE(d.p < d.H && d.p < d.W, "collate_gather: a patch of p=%u does not fit a %u x %u image (p < H and p < W)", d.p, d.H, d.W);
    }
    SN_REQUIRE(d.coarse_size >= 1 || !d.inds_coarse, "collate_gather: inds_coarse with coarse_size 0");
    SN_UNSUPPORTED(d.coarse_size < (1u << 24), "collate_gather: coarse_size must stay below 2^24 (got %u)", d.coarse_size);
    if (d.images || d.images_out) {
        SN_REQUIRE(d.image_channels == 3 || d.image_channels == 4, "collate_gather: images of %u channels (3 or 4)", d.image_channels);
        SN_REQUIRE(d.images || !d.images_out, "collate_gather: an images output without the dataset's images");
        SN_REQUIRE(!d.images_out || d.images_stride >= d.image_channels, "collate_gather: images row stride %u below %u channels", d.images_stride, d.image_channels);
    }
    if (d.masks || d.masks_out) {
        SN_REQUIRE(d.mask_elem_bytes == 1 || d.mask_elem_bytes == 4 || d.mask_elem_bytes == 8,
                   "collate_gather: mask elements of %u bytes (1, 4 or 8)", d.mask_elem_bytes);
        SN_REQUIRE(d.mask_channels >= 1, "collate_gather: masks of 0 channels");
        SN_REQUIRE(d.masks || !d.masks_out, "collate_gather: a masks output without the dataset's masks");
        SN_REQUIRE(!d.masks_out || d.masks_stride >= d.mask_channels, "collate_gather: masks row stride %u below %u channels", d.masks_stride, d.mask_channels);
        SN_REQUIRE(((reinterpret_cast<uintptr_t>(d.masks) | reinterpret_cast<uintptr_t>(d.masks_out)) & (d.mask_elem_bytes - 1u)) == 0,
                   "collate_gather: masks must be aligned to their %u-byte elements", d.mask_elem_bytes);
    }
    SN_REQUIRE(d.error_map || !d.error_maps_out, "collate_gather: an error_maps output without the dataset's error map");
    SN_REQUIRE(d.cam_near_far || !d.cam_near_far_out, "collate_gather: a cam_near_far output without the dataset's cam_near_far");
    SN_REQUIRE((!d.rays_o || d.rays_o_stride >= 3) && (!d.rays_d || d.rays_d_stride >= 3), "collate_gather: rays row stride below 3 floats");
    SN_REQUIRE((!d.index_out || d.index_stride >= 1) && (!d.i_out || d.i_stride >= 1) && (!d.j_out || d.j_stride >= 1) &&
               (!d.inds_coarse || d.inds_coarse_stride >= 1) && (!d.error_maps_out || d.error_maps_stride >= 1),
               "collate_gather: row stride 0 of a one-column output");
    SN_REQUIRE(!d.cam_near_far_out || d.cam_near_far_stride >= 2, "collate_gather: cam_near_far row stride below 2 floats");
    SN_REQUIRE(!d.poses_out || d.poses_stride >= 16, "collate_gather: poses row stride below 16 floats");
    SN_REQUIRE(!d.intrinsics_out || d.intrinsics_stride >= 4, "collate_gather: intrinsics row stride below 4 floats");
    GatherArgs a;
    a.d = d;
    const double S = need_s ? (double)d.S : 1.0, Sc = d.coarse_size ? (double)d.coarse_size : 1.0;
    a.sx = (float)((double)d.H / S); a.sy = (float)((double)d.W / S);
    a.ej = (float)(S / (double)d.H); a.ei = (float)(S / (double)d.W);
    a.cj = (float)(Sc / (double)d.H); a.ci = (float)(Sc / (double)d.W);
    if (!need_s) a.d.S = 1u;
    if (!d.coarse_size) a.d.coarse_size = 1u;
    a.main_blocks = div_up(d.N, 256);
    hipLaunchKernelGGL(k_collate_gather, dim3(a.main_blocks + div_up(local, 256)), dim3(256), 0, (hipStream_t)stream, a);
    SN_LAUNCH_CHECK("k_collate_gather");
    return SN_OK;
}

}  // extern "C"
