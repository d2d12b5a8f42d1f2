/*
 * sanerf_hip.h — C ABI of libsanerf_hip.so, the MI355X (gfx950) implementation of
 * SANeRF-HQ's volumetric-rendering hot path.
 *
 * Boundary contract
 *   - plain `extern "C"`, raw DEVICE pointers + sizes + a hipStream_t passed as void*;
 *     no torch / ATen types.  Small per-level / per-layer tables (offsets, dims) are
 *     HOST data, as noted per argument.
 *   - the caller allocates every output (the reference does the same:
 *     gridencoder/grid.py:49,55,83,86); functions write in place.
 *   - every function returns 0 on success or a negative sn_status; it never throws.
 *     sn_last_error() returns a thread-local message for the last failure
 *     (the reference raises RuntimeError through TORCH_CHECK, gridencoder.cu:15-18,392).
 *   - all work is enqueued on `stream` (the reference launches on the legacy default
 *     stream, gridencoder.cu:386); nothing synchronises.
 *
 * Each entry point names the reference interface (file:line under /root/reference)
 * it replaces.  INTEGRATION.md shows the ctypes binding the reference side would add.
 */
#ifndef SANERF_HIP_H
#define SANERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN_MAX_LEVELS 32
#define SN_MAX_LAYERS 8
#define SN_MAX_STAGES 4
#define SN_ABI_VERSION 12

typedef void *sn_stream_t; /* hipStream_t */

typedef enum {
    SN_OK = 0,
    SN_ERR_INVALID = -1,     /* bad argument (null pointer, unsupported D/C, ...) */
    SN_ERR_UNSUPPORTED = -2, /* valid in the reference but not built here */
    SN_ERR_HIP = -3,         /* HIP runtime error (launch failed, no device) */
    SN_ERR_WORKSPACE = -4,   /* workspace too small */
    SN_ERR_WINDOW = -5       /* an image smaller than the operator's window (sn_rm_image_ssim_accumulate: H or W < 11) */
} sn_status;

enum { SN_F32 = 0, SN_F16 = 1 };                 /* table storage type */
enum { SN_LAYOUT_LBC = 0, SN_LAYOUT_BLC = 1 };   /* [L,B,C] (reference kernel) or [B,L*C] (what grid.py:63 returns) */

int sn_abi_version(void);
/* How this library was built: bit 0 (SN_BUILD_EXPERIMENTS) = -DSN_EXPERIMENTS, the measured-and-rejected kernel variants are compiled in
 * (sn_render_tuning.experiment, sn_debug_set); bit 1 (SN_BUILD_POISON_LDS) = -DSN_POISON_LDS, every kernel that uses LDS fills it with
 * signalling NaNs at entry (a read-before-write shows up as NaN in the result: the r03 bug class of k_final_stage_any).  The product
 * library (`make`) carries neither. */
#define SN_BUILD_EXPERIMENTS 1
#define SN_BUILD_POISON_LDS 2
int sn_build_flags(void);
/* Experiments builds only (SN_ERR_UNSUPPORTED otherwise): process-wide A/B switches of variants that are not reachable through a
 * descriptor.  Keys: "wide_jit" (0: the superseded k_mlp_wide forward instead of k_mlp_wide_j).
 * One key is honoured by every build: "distill_general" (1: sn_rm_feature_distill_loss / sn_rm_feature_map take the general four-tap path
 * also where h, w == Ho, Wo, so that the identity fast path can be compared with it; sn_rm_feature_distill_workspace_bytes follows). */
int sn_debug_set(const char *key, int value);
const char *sn_last_error(void);
/* number of HIP devices visible; <0 on error.  Lets hosts fail loudly before any launch. */
int sn_device_count(void);

/* ------------------------------------------------------------------------------------------
 * gridencoder  — replaces gridencoder/src/gridencoder.h:12-16 (pybind: bindings.cpp:5-9)
 * inputs  [B,D] f32 in [0,1] (device);  embeddings [rows,C] (device, table_dtype);
 * offsets [L+1] int32 on the HOST (the reference keeps them on the device and re-reads them in
 * every thread; here the per-level table — resolution per gridencoder.cu:133, size, dense/hash —
 * is computed once on the host and passed by value);  S = (float)log2(per_level_scale);
 * outputs f32, layout per `layout`;  dy_dx [B,L,D,C] f32 or NULL.
 * ------------------------------------------------------------------------------------------ */
int sn_grid_encode_forward(const float *inputs, const void *embeddings, int table_dtype,
                           const int32_t *offsets_host, float *outputs,
                           uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level,
                           float S, uint32_t H, float *dy_dx,
                           uint32_t gridtype, int align_corners, uint32_t interp,
                           int layout, sn_stream_t stream);
/* outputs [B, L*C + E] = cat([grid_encode(inputs) in the [B, L*C] layout, extra [B, E]], -1): the mask head's MLP input
 * (nerf/renderer.py:380) in one pass.  D = 3, C in {2, 4, 8}, forward only (inference). */
int sn_grid_encode_forward_cat(const float *inputs, const void *embeddings, int table_dtype, const int32_t *offsets_host,
                               const float *extra, uint32_t E, float *outputs, uint32_t B, uint32_t C, uint32_t L,
                               float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, sn_stream_t stream);
/* grad f32 in `layout`; grad_embeddings [rows,C] f32, zero-initialised by the caller
 * (grid.py:83); grad_inputs [B,D] f32 written when dy_dx != NULL. */
int sn_grid_encode_backward(const float *grad, const float *inputs, const void *embeddings, int table_dtype,
                            const int32_t *offsets_host, float *grad_embeddings,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level,
                            float S, uint32_t H, const float *dy_dx, float *grad_inputs,
                            uint32_t gridtype, int align_corners, uint32_t interp,
                            int layout, sn_stream_t stream);
/* Same result as sn_grid_encode_backward (embedding gradient only; replaces the scatter of gridencoder.cu:252-349 / grid.py:71-95)
 * without the reference's atomics-per-corner: a level's rows are cut into bins sized to what a workgroup holds in LDS, the
 * (row, contribution) pairs are partitioned by bin in one pass and every bin is counting-sorted and summed in LDS by the workgroup(s)
 * that own it (grid_binned.hip; rounds 1-3 sorted the pairs with a library radix sort instead).  D in {2,3}; C a power of two <= 32;
 * B*max_level*2^D < 2^31; every level at most 4096 bins of 4096 rows -- sn_grid_backward_binned_workspace_bytes() returns 0 for shapes
 * outside that, which then take sn_grid_encode_backward.  workspace >= that many device bytes (bin counters, work lists, 2-byte row keys
 * and the B*max_level*2^D*C pre-multiplied contributions, partial-sum slabs of split bins <= twice the table), 16-byte aligned like grad;
 * grad_embeddings zero-initialised by the caller, rows without contribution are not written.  offsets_host = the L+1 level offsets
 * (host memory).  No host synchronisation, static grids (graph-capturable).  Sums are order-nondeterministic in the last bits, like the
 * reference's atomicAdd.  Several times faster than the atomic path at the sizes of the training steps. */
/* sn_grid_encode_backward_binned on a gradient whose rows are grad_row_stride floats apart ([B, L*C] layout only; 0 = L*C): the gradient of a
 * wider tensor that carries the grid features in its first L*C columns -- the mask head's MLP input cat([m_grid(x), geo_feat]) of
 * renderer.py:380 -- is read in place, without the slice copy.  Rows need only 4-byte alignment. */
int sn_grid_encode_backward_binned_rows(const float *grad, uint32_t grad_row_stride, const float *inputs, const int32_t *offsets_host, float *grad_embeddings,
                                        uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level,
                                        float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp,
                                        int layout, void *workspace, size_t workspace_bytes, sn_stream_t stream);
size_t sn_grid_backward_binned_workspace_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level, const int32_t *offsets_host);
int sn_grid_encode_backward_binned(const float *grad, const float *inputs, const int32_t *offsets_host, float *grad_embeddings,
                                   uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level,
                                   float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp,
                                   int layout, void *workspace, size_t workspace_bytes, sn_stream_t stream);
/* gridencoder.h:15 / grid.py:170-191.  D, C, L and the offsets are checked first (SN_ERR_INVALID); B = 0 on a valid grid then returns
 * SN_OK without looking at the device pointers, which may be NULL (an empty tensor's data pointer is). */
int sn_grad_total_variation(const float *inputs, const float *embeddings, float *grad,
                            const int32_t *offsets_host, float weight,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                            float S, uint32_t H, uint32_t gridtype, int align_corners,
                            sn_stream_t stream);
/* gridencoder.h:16 / grid.py:193-204.  B = number of table rows. */
int sn_grad_weight_decay(const float *embeddings, float *grad, const int32_t *offsets_host,
                         float weight, uint32_t B, uint32_t C, uint32_t L, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * shencoder — replaces shencoder/src/shencoder.h:9-10.  inputs [B,3] f32 (unit vectors),
 * outputs [B,degree^2], dy_dx [B,3,degree^2] or NULL; degree in 1..8.
 * ------------------------------------------------------------------------------------------ */
int sn_sh_encode_forward(const float *inputs, float *outputs, uint32_t B, uint32_t D, uint32_t degree,
                         float *dy_dx, sn_stream_t stream);
/* accumulates into grad_inputs [B,3] (zero-initialised by the caller, sphere_harmonics.py:50) */
int sn_sh_encode_backward(const float *grad, const float *inputs, uint32_t B, uint32_t D, uint32_t degree,
                          const float *dy_dx, float *grad_inputs, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * freqencoder — replaces freqencoder/src/freqencoder.h:6-9.  C = D + 2*D*deg.
 * ------------------------------------------------------------------------------------------ */
int sn_freq_encode_forward(const float *inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                           float *outputs, sn_stream_t stream);
int sn_freq_encode_backward(const float *grad, const float *outputs, uint32_t B, uint32_t D, uint32_t deg,
                            uint32_t C, float *grad_inputs, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * raymarching — the reference has no native twin for these (README.md:32-34 mentions a
 * `raymarching` extension that is not in the tree); each replaces a block of torch ops.
 * ------------------------------------------------------------------------------------------ */
/* nerf/utils.py:201-205,269-287 (full image).  pose: 16 floats row-major cam2world, HOST. */
int sn_rm_generate_rays(const float *pose_host, float fx, float fy, float cx, float cy,
                        uint32_t H, uint32_t W, uint32_t row_begin, uint32_t row_end,
                        float *rays_o, float *rays_d, sn_stream_t stream);
/* nerf/utils.py:209-287 for a drawn pixel subset (a training step's rays): ray n looks through flat pixel index inds[n]
 * (int64, row-major in an image of width W) of camera poses[n].  poses: DEVICE, n_poses x 16 floats row-major cam2world,
 * n_poses = 1 (one camera for all rays) or N (one camera per ray: provider.py:908-913 `random_image_batch`);
 * intrinsics: DEVICE, n_intrinsics x (fx, fy, cx, cy), 1 or N.  No host round trip. */
int sn_rm_rays_from_pixels(const float *poses, uint32_t n_poses, const float *intrinsics, uint32_t n_intrinsics, const int64_t *inds,
                           uint32_t W, uint32_t N, float *rays_o, float *rays_d, sn_stream_t stream);
/* nerf/renderer.py:122-139.  aabb: 6 floats, HOST.  nears/fars [N]. */
int sn_rm_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb_host,
                             float min_near, uint32_t N, float *nears, float *fars, sn_stream_t stream);
/* nerf/renderer.py:60-69.  x,z [N,3]. */
int sn_rm_contract(const float *x, uint32_t N, float *z, sn_stream_t stream);
/* nerf/renderer.py:84-119.  bins [N,T0+1], weights [N,T0] -> out_bins [N,T];
 * inds int32 [N,T] or NULL (the torch.searchsorted result);
 * u: NULL (the linspace of renderer.py:98), a shared device table [T] (u_stride = 0), or per-ray
 * rows [N,T] (u_stride = T; what perturb=True needs, renderer.py:101-102). */
int sn_rm_sample_pdf(const float *bins, const float *weights, uint32_t N, uint32_t T0, uint32_t T,
                     const float *u, uint32_t u_stride, float *out_bins, int32_t *inds, sn_stream_t stream);
/* nerf/renderer.py:308-325.  real_bins [N,T+1], sigmas [N,T] -> weights [N,T]. */
int sn_rm_weights_from_sigma(const float *real_bins, const float *sigmas, uint32_t N, uint32_t T,
                             int last_sample_opaque, float *weights, sn_stream_t stream);
/* Backward of sn_rm_weights_from_sigma w.r.t. sigmas (what autograd derives from renderer.py:308-325; the bin edges
 * carry no gradient on this path).  grad_weights [N,T] -> grad_sigmas [N,T]; any T <= 131072 (T <= 256: one pass in registers; longer rays keep
 * the fp64 prefix of every 64-sample segment and evaluate the terms again on the way back -- the same bits). */
int sn_rm_weights_from_sigma_backward(const float *real_bins, const float *sigmas, const float *grad_weights, uint32_t N, uint32_t T,
                                      int last_sample_opaque, float *grad_sigmas, sn_stream_t stream);

/* Inter-level proposal loss of one proposal stage (nerf/renderer.py:30-57): bins [N,T+1], weights [N,T] of the proposal
 * stage against ref_bins [N,Tr+1], ref_weights [N,Tr] of the final stage (detached in the reference).
 * Forward (loss_per_ray != NULL, grad_weights NULL): loss_per_ray[n] = sum_j max(rw_j - bound_j, 0)^2 / (rw_j + 1e-8);
 * the reference's value is sum(loss_per_ray) / (N * Tr).  Backward (grad_weights != NULL, loss_per_ray NULL):
 * grad_weights[n,i] = d(sum_j term_j)/d w_i (scale by upstream / (N * Tr)).  Deterministic (no atomics). */
int sn_rm_proposal_loss(const float *bins, const float *weights, const float *ref_bins, const float *ref_weights, uint32_t N, uint32_t T,
                        uint32_t Tr, float *loss_per_ray, float *grad_weights, sn_stream_t stream);

/* Distortion loss (nerf/renderer.py:17-27 -> torch_efficient_distloss.eff_distloss, third party, not vendored: the
 * published value is mean over rays of (1/3) sum_i w_i^2 d_i + sum_ij w_i w_j |m_i - m_j|) on bins [N,T+1], weights [N,T]:
 * loss_per_ray [N] (the reference's value is its mean) and grad_weights [N,T] = d loss_per_ray / d w, in one pass. */
int sn_rm_distort_loss(const float *bins, const float *weights, uint32_t N, uint32_t T, float *loss_per_ray, float *grad_weights,
                       sn_stream_t stream);

/* Mask-field NLL per ray (nerf/trainer.py:419-428): loss_per_ray[n] = -log(clamp(softmax(logits[n, :])[labels[n]], eps, 1 - eps)) -- the
 * reference's `loss` before its .mean() -- and, when grad_logits != NULL, d loss_per_ray[n] / d logits[n, :] in the same pass (zero where
 * the clamp binds, like torch.clamp's backward).  logits [N,K] f32, labels [N] int64 (a label outside 0..K-1: loss 0, no gradient). */
int sn_rm_mask_nll(const float *logits, const int64_t *labels, uint32_t N, uint32_t K, float eps, float *loss_per_ray, float *grad_logits,
                   sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The object-field training extras of nerf/trainer.py (scripts/train_obj_nerf.sh: --ray_pair_rgb_loss_weight, --mixed_sampling,
 * --error_map).  `masks` [.., K] holds softmax probabilities (from_logits = 0: the reference's own signature, un-clamped) or the logits
 * themselves (from_logits != 0: the softmax runs inside and gradients are with respect to the logits).  No atomics anywhere: two calls on
 * the same inputs give the same bits.  Limits: K <= 32, S <= 64, G * P < 2^31 (SN_ERR_UNSUPPORTED beyond them).
 * ------------------------------------------------------------------------------------------ */

/* Which pixels of each group the ray-pair loss compares against (trainer.py:268-276) without torch.multinomial and without a host round
 * trip: incoherent [G,P] (the rays' error-map values), uniform [G,P] in [0,1) from the caller (one torch.rand per step, like sn_rm_jitter).
 * Candidates of a group are its pixels with (1 - incoherent) > 0.8, or all its pixels if there is none; sample_index [G,S] int64 receives the S
 * candidates with the smallest uniform value (lower index first on a tie) in ascending order of that value -- for 0/1 weights the
 * exponential-race draw that multinomial(replacement=False) makes, so the same distribution.  A group with c < S candidates (the reference
 * raises there) gets -1 in slots c..S-1. */
int sn_rm_ray_pair_select(const float *incoherent, const float *uniform, uint32_t G, uint32_t P, uint32_t S, int64_t *sample_index,
                          sn_stream_t stream);

/* Ray-pair RGB loss (trainer.py:276-303) on rgb [G,P,3], masks [G,P,K], sample_index [G,S]: with q = masks[g, sample_index[g,s]] (detached;
 * one-hot of its argmax unless use_pred_logistics) and sim_i = |rgb[g,i] - rgb[g,sample_index[g,s]]|_2 < thr,
 *   loss_per_pair[g,s] = sum_i sim_i exp(-w cos(masks[g,i], q) - eps) / sum_i sim_i        (the reference's loss is its mean)
 * and, in the same launch, grad_masks [G,P,K] = scale * (scale_dev ? *scale_dev : 1) / n_pairs * d sum(loss_per_pair) / d masks, written for
 * every element (the caller does not clear it).  rgb gets no gradient (the comparison is boolean), q gets none (detached).  A slot whose
 * index is -1 (or outside 0..P-1) is no pair: 0 in loss_per_pair, no gradient, not counted in n_pairs (no pairs at all: zero gradient).
 * pair_count [1] or NULL receives max(n_pairs, 1) as a float, so that the mean is sum(loss_per_pair) / *pair_count without a pass over
 * sample_index.  loss_per_pair / grad_masks: either may be NULL, not both.  thr > 0.  Cost to know: every group's workgroup counts the call's
 * pairs itself (G * S index reads per group), so the work grows with G^2 S; meant for the few groups of a training step (the reference: 2-4),
 * fine up to a few thousand. */
int sn_rm_ray_pair_rgb_loss(const float *rgb, const float *masks, int from_logits, const int64_t *sample_index, uint32_t G, uint32_t P, uint32_t S,
                            uint32_t K, float thr, float w, float eps, int use_pred_logistics, float scale, const float *scale_dev,
                            float *loss_per_pair, float *pair_count, float *grad_masks, sn_stream_t stream);

/* The error measure of the error map (trainer.py:1426-1432): error[n] = exp(-w cos(masks[n], onehot(labels[n])) - eps)
 * = exp(-w p[label] / max(|p|, 1e-8) - eps); masks [N,K], labels [N] int64 (a label outside 0..K-1: the zero vector, exp(-eps)). */
int sn_rm_mask_error(const float *masks, int from_logits, const int64_t *labels, uint32_t N, uint32_t K, float w, float eps, float *error,
                     sn_stream_t stream);

/* The per-step update of the error map (trainer.py:457-464), in place on error_map [map_rows, row_stride]:
 *   error_map[rows[n], cols[n]] = 0.1 * error_map[rows[n], cols[n]] + 0.9 * error[n],   error as sn_rm_mask_error
 * rows int64 [n_rows], n_rows = 1 (one image for all rays) or N; cols int64 [N].  Every new value is computed from the map as it was
 * before the call (first launch, into stage [N], a scratch buffer of the caller) and written by a second launch; of several rays with the
 * same target any one's value is kept, as with torch's indexed assignment.  Targets outside the map are skipped.  error [N] or NULL. */
int sn_rm_error_map_update(const float *masks, int from_logits, const int64_t *labels, const int64_t *rows, uint32_t n_rows, const int64_t *cols,
                           uint32_t N, uint32_t K, float w, float eps, uint32_t map_rows, uint32_t row_stride, float *error_map, float *stage,
                           float *error, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The mask field's output stage and the device-side evaluation meters: everything the reference does between
 * `instance_mask_logits` and what a user sees (test_step) or scores (eval_step, nerf/metrics.py).  Streaming kernels, one launch per
 * image each, nothing synchronises, no float atomics, two calls on the same inputs give the same bits (the accumulators included).
 * Limits: K <= 32, C <= 32 classes for the meters, N < 2^31 (SN_ERR_UNSUPPORTED beyond them).  N = 0 returns SN_OK and does nothing.
 * ------------------------------------------------------------------------------------------ */
#define SN_MASK_MAX_CLASSES 32
enum { SN_MASK_OUT_NONE = 0, SN_MASK_OUT_HEATMAP = 1, SN_MASK_OUT_COMPOSITION = 2, SN_MASK_OUT_MASK = 3 };

/* test_step's mask branch (nerf/trainer.py:730-777), the overlays it calls (nerf/utils.py:49-60 overlay_mask_composition, :63-77
 * overlay_mask_heatmap) and the host-side (x * 255).astype(np.uint8) of trainer.py:726-727 / 780-781, in one launch:
 *   p = softmax(logits[n, :]) (K = 1: sigmoid, trainer.py:734-739);  conf, id = max, argmax of p (the lowest index on a tie, a NaN as the
 *   greatest value: torch's rules; K = 1: id = 0, conf = p);
 *   mode HEATMAP      rgb = color_map[id] * conf, or color_map[render_id] * p[render_id] when 0 <= render_id < K
 *   mode COMPOSITION  rgb = image * alpha + (render_id == -1 || id == render_id ? color_map[id] : image) * (1 - alpha)
 *   mode MASK         rgb = image * m + (1 - m) * bg,  m = (id == render_id)
 *   mode NONE         rgb = image                       (the plain render's 8-bit image)
 *   rgb8 = trunc(clamp(255 * rgb, 0, 255)), NaN -> 0.  On [0,1] that is the reference's astype(np.uint8); outside [0,1] the reference's
 *   cast wraps modulo 256 (and is undefined for NaN) where this one saturates.
 * logits [N,K] f32; image: rows of image_stride >= 3 floats (3: a packed [N,3] image; 5: the [N,5] rgb|depth|weights_sum render buffer
 * read in place), may be NULL for HEATMAP; color_map [C,3] f32 on the device with C >= K (an id >= C cannot occur then), read by
 * HEATMAP and COMPOSITION; bg: 3 floats on the device, read by MASK.  Outputs, each may be NULL (at least one is given): probs [N,K],
 * instance_id [N] int64, confidence [N], rgb [N,3] f32, rgb8 [N,3] uint8 (4-byte aligned: the 3-byte pixels are staged in LDS and
 * stored as dwords).  A NULL output is not touched. */
int sn_rm_mask_output(const float *logits, uint32_t N, uint32_t K, const float *image, uint32_t image_stride, const float *color_map, uint32_t C,
                      int mode, int render_id, float alpha, const float *bg, float *probs, int64_t *instance_id, float *confidence, float *rgb,
                      uint8_t *rgb8, sn_stream_t stream);

/* The evaluation record of a validation epoch, on the device, 8-byte aligned, zeroed by the caller before the first image.  The
 * reference's meters keep V (a running sum of per-image values) and N (images); so does this record, for all four of them. */
typedef struct sn_eval_record {
    double nll_mean_sum;   /* sum over images of eval_step's loss (trainer.py:1603-1604 total_loss += loss.item()) */
    double miou_sum;       /* MeanIoUMeter.V */
    double mse_sum;        /* MSEMeter.V */
    double psnr_sum;       /* PSNRMeter.V */
    uint64_t images;       /* images seen by sn_rm_mask_eval_accumulate */
    uint64_t rgb_images;   /* images seen by sn_rm_image_sqerr_accumulate */
    uint64_t inter[SN_MASK_MAX_CLASSES], pred[SN_MASK_MAX_CLASSES], truth[SN_MASK_MAX_CLASSES];   /* the LAST image's class counts, for inspection */
} sn_eval_record;

/* Scratch of the two accumulating entry points: SN_MASK_EVAL_WORKSPACE_BYTES on the device, 8-byte aligned, zeroed ONCE by the caller;
 * every launch leaves it zeroed again.  Launches that share a workspace must be ordered (one stream). */
#define SN_MASK_EVAL_WORKSPACE_BYTES 8192

/* eval_step's mask branch (trainer.py:599-627: softmax / sigmoid, clamp, NLL over the labelled pixels, its `labeled.sum() > 0` host branch
 * as a device-side select) + evaluate_one_epoch's loss.item() (:1603-1604) + MeanIoUMeter.update (nerf/metrics.py:165-179), one launch:
 *   nll_mean_sum += sum_n nll[n] / #{labels[n] != -1}   (0 when no pixel is labelled), nll[n] = -log(clamp(p[n, labels[n]], eps, 1 - eps))
 *                   per pixel as sn_rm_mask_nll defines it (a label outside 0..K-1: 0), p as in sn_rm_mask_output, summed in double in a fixed order;
 *   miou_sum     += mean over the classes i < C with union_i > 0 of inter_i / union_i (double), on (argmax id, label): pred_i = #{id = i},
 *                   truth_i = #{label = i}, inter_i = #{id = label = i}, union_i = pred_i + truth_i - inter_i.  A label outside 0..C-1 (-1:
 *                   unlabelled) matches no class, but its pixel still counts in the union of its predicted class, as np.logical_or does.
 *                   Stated difference: the reference hands its meter the float probabilities, which the meter's astype(int64) turns into
 *                   zeros; here the meter gets the ids.
 *   images       += 1;  inter / pred / truth = this image's counts.
 * logits [N,K] f32, labels [N] int64, K <= C <= 32. */
int sn_rm_mask_eval_accumulate(const float *logits, const int64_t *labels, uint32_t N, uint32_t K, uint32_t C, float eps, sn_eval_record *record,
                               void *workspace, sn_stream_t stream);

/* MSEMeter.update and PSNRMeter.update (nerf/metrics.py:217-221, 28-38) for one image: pred, truth: N rows of >= 3 floats (row strides in
 * floats: 3 = packed, 5 = the render buffer).  The difference is taken in fp32, squared and summed in double in a fixed order:
 *   mse = sum / (3 N);  mse_sum += mse;  psnr_sum += -10 log10(mse);  rgb_images += 1. */
int sn_rm_image_sqerr_accumulate(const float *pred, uint32_t pred_stride, const float *truth, uint32_t truth_stride, uint32_t N,
                                 sn_eval_record *record, void *workspace, sn_stream_t stream);

/* SSIMMeter.update (nerf/metrics.py:124-131) for one image pair, without a host read.  The reference calls torchmetrics'
 * structural_similarity_index_measure at its defaults; the quantity, stated here because the package is not a dependency:
 *   g = exp(-(d / 1.5)^2 / 2), d = -5 .. 5, divided by its sum; the window is w = g (x) g (11 x 11);
 *   data_range = the given value if > 0, else max(pred.max - pred.min, truth.max - truth.min) over all pixels and channels of each image;
 *   c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2;
 *   per channel and pixel, w-weighted over the window: mu_p, mu_t, E[pp], E[tt], E[pt];  s_p^2 = max(E[pp] - mu_p^2, 0), s_t^2 alike,
 *   s_pt = E[pt] - mu_p mu_t;  ssim = ((2 mu_p mu_t + c1)(2 s_pt + c2)) / ((mu_p^2 + mu_t^2 + c1)(s_p^2 + s_t^2 + c2));
 *   value = mean of ssim over the 3 channels and the pixels 5 <= y < H - 5, 5 <= x < W - 5 (the package reflect-pads by 5 and crops 5: the
 *   padding never reaches a kept pixel).
 * Evaluated in fp32 on moments centred on a per-tile pivot (variances and the covariance do not change under a shift; raw fp32 moments
 * cancel when data_range is small), summed in double in a fixed order: equal bits run to run.  A NaN anywhere gives NaN; two constant
 * images with a derived data_range give 0 / 0 = NaN.
 * The record: on the device, 8-byte aligned, zeroed by the caller before the first image. */
typedef struct sn_ssim_record {
    double ssim_sum;       /* SSIMMeter.V */
    double last;           /* the last image's value */
    uint64_t images;       /* SSIMMeter.N */
} sn_ssim_record;

/* Scratch of sn_rm_image_ssim_accumulate: on the device, 8-byte aligned, zeroed ONCE by the caller; every call leaves it zeroed again.
 * Calls that share a workspace must be ordered (one stream). */
#define SN_SSIM_WORKSPACE_BYTES 8192

/* ssim_sum += value; last = value; images += 1.  pred, truth: H * W rows of >= 3 floats (row strides in floats, 3 .. 64: 3 = packed, 5 =
 * the render buffer read in place; beyond 64: SN_ERR_UNSUPPORTED).  data_range <= 0: derived on the device (one more launch).
 * H or W < 11: SN_ERR_WINDOW (the package's reflect pad fails there too); H * W >= 2^31: SN_ERR_UNSUPPORTED. */
int sn_rm_image_ssim_accumulate(const float *pred, uint32_t pred_stride, const float *truth, uint32_t truth_stride, uint32_t H, uint32_t W,
                                float data_range /* <= 0: derive */, sn_ssim_record *record, void *workspace, sn_stream_t stream);

/* The loss tail of the SAM-feature distillation step (nerf/trainer.py:540-550; evaluation :664-670), without a host read:
 *   pred = F.interpolate(samvit.reshape(1, h, w, C).permute(0, 3, 1, 2), (Ho, Wo), mode="bilinear");  loss = MSELoss(pred, target).mean()
 * and the gradient of the loss with respect to samvit.  The quantity, stated here because no torch backend is the contract (torch's fp32
 * CPU kernel rounds its weights differently, by up to 7e-6).  The taps of output index o on an axis of n_in samples resized to n_out,
 * by exactly this fp32 chain (nothing contracted):
 *   s = float(n_in) / float(n_out);  src = max((o + 0.5f) * s - 0.5f, 0);  i0 = min(int(src), n_in - 1);  i1 = i0 + (i0 < n_in - 1);
 *   l1 = src - i0;  l0 = 1 - l1.
 * With (y0, y1, l0y, l1y) the taps of oy on h -> Ho and (x0, x1, l0x, l1x) those of ox on w -> Wo, f[y, x, c] = feat[(y w + x) feat_stride + c]:
 *   pred[c, oy, ox] = l0y (l0x f[y0,x0,c] + l1x f[y0,x1,c]) + l1y (l0x f[y1,x0,c] + l1x f[y1,x1,c])        in fp32;
 *   d = pred - target in fp32;  loss = sum d^2 / n, n = C Ho Wo, squared and summed in double in a fixed order (no float atomics: two
 *   calls on the same inputs give equal bits), stored as a float;
 *   grad_feat[y w + x, c] = (scale * (scale_dev ? *scale_dev : 1)) * (2 / float(n)) * sum_oy wy(oy -> y) sum_ox wx(ox -> x) d[c, oy, ox],
 *   w(o -> i) = (i0(o) == i ? l0 : 0) + (i1(o) == i ? l1 : 0), over the contiguous range of outputs with i - 1 <= i0(o) <= i, in ascending
 *   order in fp32.  Every element of grad_feat is written exactly once (0 where no output reaches the pixel, e.g. 64 -> 16); the caller does
 *   not clear it.
 * Stated differences from torch: where h, w == Ho, Wo every l1 is 0 and a fast path (one launch) reads f[oy, ox, c] alone -- on finite
 * inputs its values are equal to the general path's; a non-finite value in a zero-weight neighbour (0 * inf) does not reach the result
 * there, as it does in torch and in the general path.  Otherwise NaN and Inf propagate: a non-finite input with a non-zero weight gives a
 * non-finite loss.
 * feat: h w rows of C floats, feat_stride >= C floats apart (the render's `samvit`, read in place); target, resized: packed [C, Ho, Wo];
 * loss [1]; grad_feat packed [h w, C]; grad_feat and resized may each be NULL.  Any sizes >= 1; h w C and n below 2^31 (beyond:
 * SN_ERR_UNSUPPORTED).  Launches: one where h, w == Ho, Wo or grad_feat is NULL, else two.
 * The workspace: on the device, 8-byte aligned.  Its first SN_DISTILL_WORKSPACE_FIXED_BYTES are zeroed ONCE by the caller and left zeroed by
 * every call (calls that share a workspace must be ordered: one stream); a resize with a gradient needs n more floats behind them, which
 * every such call writes before it reads and which carry nothing from call to call (SN_ERR_WORKSPACE when workspace_bytes is too small). */
#define SN_DISTILL_WORKSPACE_FIXED_BYTES 8256
size_t sn_rm_feature_distill_workspace_bytes(uint32_t h, uint32_t w, uint32_t C, uint32_t Ho, uint32_t Wo);   /* 0: sizes not supported */
int sn_rm_feature_distill_loss(const float *feat, uint32_t feat_stride, uint32_t h, uint32_t w, uint32_t C, const float *target, uint32_t Ho,
                               uint32_t Wo, float scale, const float *scale_dev, float *loss, float *grad_feat, float *resized, void *workspace,
                               size_t workspace_bytes, sn_stream_t stream);
/* The forward half alone: out [C, Ho, Wo] = pred above (what decode_step, trainer.py:928-930, and store_sam_feautres need). */
int sn_rm_feature_map(const float *feat, uint32_t feat_stride, uint32_t h, uint32_t w, uint32_t C, uint32_t Ho, uint32_t Wo, float *out,
                      sn_stream_t stream);

/* The loss tail of the RGB training step (nerf/trainer.py:364-392; evaluation :586-595), without a host read, in ONE launch: the RGBA
 * blend of the ground truth, the background term of the prediction, MSELoss(reduction='none').mean(), the entropy of weights_sum, the
 * extras (proposal and distortion loss) folded into the total, and the gradients with respect to image and weights_sum.
 * The quantity, per ray and in fp32 (nothing contracted); b_c is the ray's background: bg_value (bg_rows == 0), bg[c] (bg_rows == 1)
 * or bg[3 ray + c] (bg_rows == N):
 *   a      = truth[3]                                  (truth_channels == 4)
 *   gt_c   = truth_c * a + b_c * (1 - a)               (4 channels; trainer.py:366-368)      gt_c = truth_c   (3 channels)
 *   pred_c = image_c                                   (image_has_bg)
 *   pred_c = image_c + (1 - weights_sum) * b_c         (otherwise; renderer.py:353 -- the image was rendered over bg = 0)
 *   d_c    = pred_c - gt_c
 *   mse    = sum d_c^2 / (3 N)                         squared and summed in double in a fixed order, stored as a float
 *   c      = min(max(weights_sum, (float)1e-5), (float)(1 - 1e-5));   e = (-c) log2f(c) - (1 - c) log2f(1 - c)
 *   entropy = sum e / N                                summed in double in a fixed order (not evaluated, and 0, when lambda_entropy == 0)
 *   total  = ((mse + lambda_entropy * entropy) + coef0 * *extra0) + coef1 * *extra1          in fp32; a NULL extra contributes nothing
 *   grad_image_c     = (2 d_c) * (1 / float(3 N))
 *   grad_weights_sum = (image_has_bg ? 0 : -((g_0 b_0 + g_1 b_1) + g_2 b_2)),  g = grad_image,
 *                    + (lambda_entropy != 0 and (float)1e-5 <= weights_sum <= (float)(1 - 1e-5) ?
 *                                                          (lambda_entropy / float(N)) * (log2f(1 - c) - log2f(c)) : 0)
 * The second term is torch's clamp backward: the bounds are inclusive, a NaN is outside.  No gradient goes to truth or bg.  A NaN or Inf
 * in image, weights_sum, truth or bg reaches the outputs that torch's chain gives it (the clamp keeps a NaN, as torch.clamp does).
 * image: N rows of >= 3 floats, image_stride floats apart (3 = packed, 5 = the render buffer read in place); truth: N rows of
 * truth_channels floats, truth_stride apart; weights_sum [N]; bg: packed [3] or [N,3]; extra0, extra1: device scalars or NULL;
 * pred_rgb, gt_rgb, grad_image: packed [N,3], grad_weights_sum [N]: each may be NULL and is then not written; record: on the device.
 * 256 lanes a workgroup, a ray a lane, at most SN_RGB_LOSS_MAX_WORKGROUPS workgroups (a lane loops over rays beyond
 * SN_RGB_LOSS_MAX_WORKGROUPS * 256: the cap is what the last workgroup's two rows of partials take of its LDS, 2 x 512 doubles = 8 KiB).
 * Two calls on the same inputs give equal bits.  SN_ERR_INVALID: a NULL image, weights_sum, truth, record or workspace; a stride below
 * the channel count; truth_channels not 3 or 4; bg_rows not 0, 1 or N, or a NULL bg with bg_rows != 0; N == 0; a workspace that is not
 * 8-byte aligned.  SN_ERR_UNSUPPORTED: N >= 2^30.
 * The workspace: on the device, 8-byte aligned, SN_RGB_LOSS_WORKSPACE_BYTES, zeroed ONCE by the caller, left zeroed by every call (calls
 * that share a workspace must be ordered: one stream). */
typedef struct sn_rgb_loss_record { float total, mse, entropy, reserved; } sn_rgb_loss_record;
#define SN_RGB_LOSS_MAX_WORKGROUPS 512
#define SN_RGB_LOSS_WORKSPACE_BYTES 8256   /* a ticket (64 bytes) and 2 x SN_RGB_LOSS_MAX_WORKGROUPS doubles */
int sn_rm_rgb_loss(const float *image, uint32_t image_stride, const float *weights_sum, const float *truth, uint32_t truth_stride,
                   uint32_t truth_channels, uint32_t N, float bg_value, const float *bg, uint32_t bg_rows, int image_has_bg,
                   float lambda_entropy, const float *extra0, float coef0, const float *extra1, float coef1, float *pred_rgb, float *gt_rgb,
                   sn_rgb_loss_record *record, float *grad_image, float *grad_weights_sum, void *workspace, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Propagation of 3D point prompts across views and the decode overlays (prompts.hip): what the reference does between a click and the
 * SAM decoder's prompt, and between the decoder's masks and the picture it returns.  Labels, crucial flags, counts and states are int32
 * on the device, coordinates are int32 (x, y) pairs.  Nothing synchronises, no atomics, every output has one writer: two calls on the
 * same inputs give the same bits.  An empty problem returns SN_OK and touches nothing.
 * ------------------------------------------------------------------------------------------ */
#define SN_PROMPT_MAX_POINTS 1024   /* capacity of a point store; points of one sn_rm_prompt_overlay call */

/* test_step's "remember new point_3d" (nerf/trainer.py:803-809): pixels [M,2] (x, y) on the device, rays_o / rays_d [H*W,3], depth: H*W
 * values depth_stride floats apart (1: a plain [H,W] image; 5: the depth column of the packed [N,5] render buffer, read in place):
 *   point_3d[m] = o + d * depth at pixel (x, y), evaluated as fl(o + fl(d * depth)).
 * The clicks are on the device, so one outside the image cannot be refused: it writes NaN, and nothing is read out of bounds. */
int sn_rm_points_lift(const int32_t *pixels, uint32_t M, const float *rays_o, const float *rays_d, const float *depth, uint32_t depth_stride,
                      uint32_t H, uint32_t W, float *point_3d, sn_stream_t stream);

/* The add-or-remove rule of the remembered points (trainer.py:812-834) for ONE new point (what the reference's broadcast supports) on a
 * fixed-capacity store on the device: xyz [cap,3], labels [cap], crucial [cap], count [1]; point [3] and label [1] on the device too.
 *   dist_i = sqrt(sum_j (xyz[i,j] - point[j])^2) in fp32 over the stored points;
 *   count == 0:                      the point becomes entry 0;
 *   every dist_i > dist_thresh:      appended with crucial 0; with count == cap nothing changes and status[3] is set to 1;
 *   otherwise:                       every stored point with dist_i <= dist_thresh (or a NaN distance) is removed, the others keep their
 *                                    order; none left: the store is empty.
 * Extension: the reference never touches crucial_point_label on this path (its flags and its points part ways after the first click);
 * here crucial is compacted alongside and a new point is not crucial.
 * status [4] int32 on the device: {what happened (0 first entry, 1 appended, 2 removed, 3 full), count before, count after, overflow}.
 * The overflow word is only ever set: clear it once, look at it after any number of updates.  Entries behind count keep stale values.
 * One workgroup, one launch, the count is not read on the host.  cap in 1 .. SN_PROMPT_MAX_POINTS (beyond: SN_ERR_UNSUPPORTED). */
int sn_rm_point_store_update(float *xyz, int32_t *labels, int32_t *crucial, int32_t *count, uint32_t cap, const float *point, const int32_t *label,
                             float dist_thresh, int32_t *status, sn_stream_t stream);

/* The remembered points in V views (trainer.py:838-875 for test_step, :931-976 for decode_step; V > 1 scores every training view against
 * the depth stack of update_depth, :1388-1402), one wave per view:
 *   points [N,3], labels [N], crucial [N] or NULL; n_points: int32 on the device or NULL (= N), clamped to 0 .. N;
 *   poses [V,16]: row-major cam2world, taken as affine -- the fourth row is NOT read; intrinsics [n_intr,4] (fx, fy, cx, cy), n_intr 1 or V;
 *   depth: V images of H*W values, depth_stride floats apart (image v starts at v * H * W * depth_stride).
 * Per view and point: the pose's upper 3 x 4 is inverted in fp64 (adjugate over determinant: the error of the reference's fp32
 * torch.inverse is removed, not imitated) and the point transformed in fp64, the camera coordinates rounded to fp32; from there fp32 in
 * the reference's order: px = W - ((fx * x) / z + cx), py = (fy * y) / z + cy.  With equal camera coordinates these equal torch's bits.
 *   on screen iff px > -1 && px < W && py > -1 && py < H, tested in float: the reference's .long() truncates toward zero, so (-1, 0) is
 *   pixel 0; a non-finite coordinate (z == 0) is off screen, where .long() is undefined.  The pixel is ((int)px, (int)py);
 *   kept iff |(-z) - depth[py, px]| <= depth_tol (a NaN depth rejects the point).
 * Compacted outputs, original order kept: coords [V,N,2], labels_out [V,N], kept_index [V,N] (index into points); with resize_ratio > 0
 * (1024 / max(H, W) in the reference) also sam_coords = (int)((float)c * (float)ratio) and overlay_coords = (int)((double)sam / ratio),
 * which are numpy's (c.astype(float32) * r).astype(int32) and (pc / r).astype(int32) of trainer.py:872-875.  Behind the kept points the
 * rows are always filled: coordinates 0, labels -1 (SAM's padding label), index -1 -- a fixed-shape prompt needs no count.
 * Uncompacted outputs, each may be NULL: cam [V,N,3], uv [V,N,2] (px, py), state [V,N] (0 off screen or not a point, 1 occluded, 2 kept).
 * counts [V,4] = {on screen, kept, crucial kept (0 without crucial), is_valid}; is_valid = kept > 0 && crucial kept >= crucial_count &&
 * kept >= valid_threshold (trainer.py:969-971). */
int sn_rm_points_project(const float *points, const int32_t *labels, const int32_t *crucial, uint32_t N, const int32_t *n_points, const float *poses,
                         uint32_t V, const float *intrinsics, uint32_t n_intr, const float *depth, uint32_t depth_stride, uint32_t H, uint32_t W,
                         float depth_tol, int32_t crucial_count, int32_t valid_threshold, double resize_ratio /* 0: no sam / overlay coords */,
                         int32_t *coords, int32_t *labels_out, int32_t *kept_index, int32_t *sam_coords, int32_t *overlay_coords, float *cam,
                         float *uv, int32_t *state, int32_t *counts, sn_stream_t stream);

/* decode_step's tail (trainer.py:979-991; test_step's :881-884) with overlay_mask and overlay_point (nerf/utils.py:23-29, 80-98), one launch:
 *   image: H*W rows of image_stride >= 3 floats (3: packed; 5: the render buffer read in place); masks [M,H,W] uint8 or NULL (points only);
 *   scores [M] on the device, or NULL with a fixed mask_index; coords [N,2], labels [N]; count: int32 on the device or NULL (= N).
 *   selected = the first j whose score exceeds the running maximum, which starts at 0 with index 0: all scores <= 0 select mask 0, a NaN
 *   is never selected;
 *   count == 0: rgb = image, pred_mask = 0, selected = -1 (decode_step's else branch);
 *   otherwise rgb = fl(fl(image * a) + fl(over * b)), a = (float)alpha, b = (float)(1.0 - alpha), over = (1,0,0) under the selected mask
 *   and image elsewhere (masks NULL: rgb = image, as test_step draws the points without a decoder); on top the LAST point whose rectangle covers the pixel: green (0,1,0) for label 0, red otherwise.  The rectangle
 *   is Python's slice [c - radius : c + radius] per axis: a negative start counts from the end (start += len), both bounds are clamped
 *   to [0, len], start >= stop is empty -- a point closer than radius to the top or left edge is not drawn, one near the bottom or right
 *   edge is clipped and drawn.
 * Outputs: rgb [H,W,3] f32, rgb8 [H,W,3] uint8 (sn_rm_mask_output's conversion; 4-byte aligned), pred_mask [H,W] uint8 (the selected
 * mask), each may be NULL (at least one is given); selected [1] int32 (-1 also without masks).
 * N <= SN_PROMPT_MAX_POINTS, H and W <= 32767 (beyond: SN_ERR_UNSUPPORTED). */
int sn_rm_prompt_overlay(const float *image, uint32_t image_stride, uint32_t H, uint32_t W, const uint8_t *masks, uint32_t M, const float *scores,
                         int32_t mask_index, const int32_t *coords, const int32_t *labels, uint32_t N, const int32_t *count, int32_t radius, double alpha,
                         float *rgb, uint8_t *rgb8, uint8_t *pred_mask, int32_t *selected, sn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A training batch drawn on the device (collate.hip): the device-side core of NeRFDataset.collate (provider.py:894-1114) as one gather
 * launch plus one draw launch per part that draws cells, with all randomness in tensors the caller fills (torch.rand, Tensor.exponential_(): both capturable), so that
 * collate -> render -> loss -> Adam can be one HIP graph and a batch is a pure function of (dataset, random tensors).  Division is
 * IEEE-rounded, no float atomics, nothing synchronises, nothing is read on the host: two calls on the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------ */
#define SN_DRAW_MAX_CELLS 65536     /* cells of one row of sn_rm_weighted_draw */

/* Weighted sampling without replacement -- torch.multinomial's own exponential race (utils.py:218, :248): the same distribution, other bits.
 *   expo [R,C]: standard exponential variates from the caller; out [R,n] int64; status: one int32 on the device, only ever set.
 *   Row r draws from weights row r of weights [R,C] (row_u NULL), or -- the centres of the local patches, provider.py:982-993, whose
 *   cameras are drawn on the device -- from row min((int)(row_u[r] * M), M - 1) of weights [M,C]: the row-index table is the table of
 *   uniform variates that sn_rm_collate_gather turns into the patches' cameras with the same formula, so no row is gathered beforehand;
 *   or (row_index [R] int64 on the device, clamped to 0 .. M-1: the loader's image index of a single-image batch) from that row.
 * Per row the n smallest of (key, cell) in lexicographic order, key = expo / weights as an fp32 IEEE division, in ASCENDING CELL INDEX
 * (torch returns them in key order; nothing downstream depends on the order of a ray batch, inds_coarse stays aligned with its rays).
 * A cell is never selected if its weight is <= 0 or NaN, or if its key is not finite (or negative, which no exponential variate gives; -0
 * is 0).  A row with fewer than n selectable cells (the reference raises there) gets -1 in the tail of its row and *status = 1 -- the
 * choice of sn_rm_ray_pair_select.  One workgroup per row: n == 1 a (key, cell) minimum through a fixed butterfly; n > 1 a radix select
 * on the key bits (four 8-bit passes over a 256-bin LDS histogram, ties at the threshold to the smaller cell) and one order-preserving
 * compaction pass.  1 <= n <= C <= SN_DRAW_MAX_CELLS (a longer row: SN_ERR_UNSUPPORTED). */
int sn_rm_weighted_draw(const float *weights, const float *expo, uint32_t R, uint32_t C, uint32_t n, const float *row_u, const int64_t *row_index,
                        uint32_t M, int64_t *out, int32_t *status, sn_stream_t stream);

/* Draw -> rays + supervision, one lane per ray, one launch (the first ceil(N / 256) workgroups: the main part; the rest: the patches).
 * Dataset tensors, read in place: poses [M,16] row-major cam2world, intrinsics [n_intrinsics,4] (1 or M), images [M,H,W,3|4] uint8,
 * masks [M,H,W,mask_channels] of 1-, 4- or 8-byte elements copied as raw bytes (uint8, float32, int64 alike), error_map [M,S*S],
 * cam_near_far [M,2]; the last four may be NULL.  With pick(u, n) = min((int)(u * n), n - 1), the product in fp32 (the min guards the
 * upper end; a u outside [0,1) or a NaN is clamped into the range rather than indexing out of bounds):
 *   main part, N rays, mode SN_COLLATE_UNIFORM (random_image_batch, provider.py:910, utils.py:260): u [N,3];
 *     cam = pick(u0, M), row = pick(u1, H), col = pick(u2, W);
 *   mode SN_COLLATE_ERROR_MAP (one image: index, or *index_dev when given, clamped to 0 .. M-1; utils.py:247-256): cells [N] from
 *     sn_rm_weighted_draw and u [N,2]; gx = cell / S, gy = cell % S, row = min((int)(fl(fl(gx * sx) + fl(u0 * sx))), H - 1) with
 *     sx = (float)((double)H / S), col likewise from gy, u1 and sy = (float)((double)W / S);
 *   local part, L patches of p x p rays appended after the main part (provider.py:982-993, utils.py:217-244): patch k has camera
 *     pick(ul[k], M) and centre cell centres[k] (sn_rm_weighted_draw with n = 1 and row_u = ul); its corner is
 *     trunc(clamp(fl(fl(cx * sx) - p / 2), 0, H - p - 1)) with cx = cell / S and the integer p / 2, likewise for W with cell % S and sy (what
 *     the reference does); offsets in meshgrid(indexing="ij") order.  p < H and p < W.
 * A cell outside 0 .. S*S-1 (the -1 of a short draw) gives rays and float supervision of NaN, -1 in i / j / inds_coarse, zero mask bytes;
 * index, cam_near_far and poses still describe the ray's camera.
 * Outputs, rows N + L*p*p unless noted, each with its own row stride in ELEMENTS and each may be NULL: rays_o / rays_d (3 floats; the exact
 * operation sequence of sn_rm_rays_from_pixels: equal bits), index_out / i_out (column) / j_out (row) / inds_coarse int64 (utils.py:294-300:
 * the cell in error-map mode, else (int)(row * (float)(coarse_size / H)) * coarse_size + (int)(col * (float)(coarse_size / W))), images_out
 * [N only, 3|4] = (float)byte / 255.0f, masks_out, error_maps_out = error_map[cam, (int)(row * (float)(S / H)) * S + (int)(col * (float)(S / W))]
 * (the column scale S / W of nerf.utils.collate_rays), cam_near_far_out (2), poses_out (16), intrinsics_out (4: the camera's fx, fy, cx, cy). */
enum { SN_COLLATE_UNIFORM = 0, SN_COLLATE_ERROR_MAP = 1 };
typedef struct sn_collate_desc {
    const float   *poses, *intrinsics;
    const uint8_t *images;
    const void    *masks;
    const float   *error_map, *cam_near_far;
    uint32_t       M, n_intrinsics, H, W, image_channels, mask_channels, mask_elem_bytes, S, coarse_size;
    uint32_t       N;
    int32_t        mode, index;
    const int64_t *index_dev;
    const float   *u;
    const int64_t *cells;
    uint32_t       L, p;
    const float   *ul;
    const int64_t *centres;
    float         *rays_o, *rays_d;
    int64_t       *index_out, *i_out, *j_out, *inds_coarse;
    float         *images_out;
    void          *masks_out;
    float         *error_maps_out, *cam_near_far_out, *poses_out, *intrinsics_out;
    uint32_t       rays_o_stride, rays_d_stride, index_stride, i_stride, j_stride, inds_coarse_stride, images_stride, masks_stride,
                   error_maps_stride, cam_near_far_stride, poses_stride, intrinsics_stride;
} sn_collate_desc;
int sn_rm_collate_gather(const sn_collate_desc *desc, sn_stream_t stream);

/* One stage's sample geometry (renderer.py:277-285): bins [N,T+1] in [0,1] -> real_bins [N,T+1] (distances along the
 * ray through the Mip-360 spacing of nears/fars [N]), rays_t [N,T] (mid-points), xyzs [N,T,3] (positions, contracted
 * into [-2,2]^3 like sn_rm_contract if `contract`).  Nothing here is differentiated by the reference. */
int sn_rm_sample_positions(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *bins,
                           uint32_t N, uint32_t T, int contract, float *real_bins, float *rays_t, float *xyzs, sn_stream_t stream);

/* The same with the grid encoder's first step folded in (gridencoder/grid.py:156): grid_bound > 0 makes `xyzs` receive
 * (x + grid_bound) / (2 grid_bound), the unit-cube coordinates sn_grid_encode_forward takes; grid_bound = 0 = sn_rm_sample_positions. */
int sn_rm_sample_positions_ex(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *bins,
                              uint32_t N, uint32_t T, int contract, float grid_bound, float *real_bins, float *rays_t, float *xyzs,
                              sn_stream_t stream);

/* Training-time jitter of the sampling positions (perturb=True) from a caller-supplied uniform [0,1) tensor `uniform` [N,T] (NULL: none):
 *   kind 0 (renderer.py:262-270, stage-0 bins, T = num_steps[0] + 1): out = clamp(linspace(0, 1, T) + (uniform - 0.5) / (T - 1), 0, 1)
 *   kind 1 (renderer.py:97-102, sample_pdf's u):                       out = linspace(0.5/T, 1 - 0.5/T, T) + (uniform - 0.5) / T
 * out [N,T].  The reference draws torch.rand_like per stage; one draw for all stages, sliced, is statistically the same. */
int sn_rm_jitter(const float *uniform, uint32_t N, uint32_t T, int kind, float *out, sn_stream_t stream);

/* The jitter tables of every stage of a schedule in ONE table launch, from a counter-based generator whose state lives on the device
 * (csrc/jitter.hip): what sn_render_io takes as per-ray bins0_table / u_table[k], without a torch generator or a uniform scratch buffer.
 *   state      device [4], 16-byte aligned: seed, draw, ticket (zero at rest; unused), reserved
 *   N          rows written; ray_base: the global index of row 0 (ray_base + N <= 2^32)
 *   num_steps  host [num_stages], 1..SN_MAX_STAGES stages, 1 <= num_steps[k] and num_steps[k] + 1 <= 2^26 (else SN_ERR_INVALID)
 *   bins0      device [N, num_steps[0]+1] or NULL (not written)
 *   u          host array [num_stages] (or NULL: no u table); u[0] is ignored; u[k] device [N, num_steps[k]+1] or NULL (not written)
 * Element j of row n of stage k, with g = ray_base + n:
 *   w = philox4x32_10(counter = (g, (k << 24) | (j >> 2), draw_lo, draw_hi), key = (seed_lo, seed_hi))[j & 3]     (Salmon et al., SC'11)
 *   uniform = float(w >> 8) * 2^-24;   entry = what sn_rm_jitter makes of that uniform (kind 0 for k = 0, kind 1 for k >= 1), bit for bit.
 * A value depends on (seed, draw, k, g, j) only: not on N, the launch grid or how an image is cut into chunks (give chunk [head, tail) the
 * ray_base head).  advance != 0: `draw` goes up by one, once per call, in a one-thread launch behind the table launch (the kernel boundary
 * puts every workgroup's read of the state in front of the write; a ticket on state[2] was measured and dropped: csrc/jitter.hip), so a
 * replayed graph draws fresh jitter on every replay; with every table NULL the call only advances.  advance == 0: the state is left as
 * it was (all chunks of one image but the last).  state[2] and state[3] are never written.  N == 0: SN_OK, nothing is launched and the
 * state stays.  Tables need 4-byte alignment only; a 16-byte aligned table is written with 16-byte stores. */
int sn_rm_jitter_tables(uint64_t *state, uint32_t N, uint32_t ray_base, uint32_t num_stages, const uint32_t *num_steps, float *bins0,
                        float *const *u, int32_t advance, sn_stream_t stream);

/* Per-ray sums of the training path in one pass (renderer.py:327-347 with network.py:164-170's colour = cat([geo_feat, SH(d)])):
 *   weights_sum[n] = sum_t w;  depth[n] = sum_t w rays_t;  f_image[n, 0:15] = sum_t w raw[n,t,1:16];  f_image[n, 15:31] = SH4(d/|d|) weights_sum
 * raw [N,T,16] = grid_mlp's output ([sigma_raw | 15 geometry channels], network.py:94,151-153), rays_d [N,3] un-normalised.
 * The backward entry returns d/d weights [N,T] and d/d raw [N,T,16] (channel 0 = 0) from the gradients of the three outputs
 * (each may be NULL = zero).  raw / grad_raw 16-byte aligned. */
int sn_rm_ray_composite(const float *weights, const float *rays_t, const float *raw, const float *rays_d, uint32_t N, uint32_t T,
                        float *weights_sum, float *depth, float *f_image, sn_stream_t stream);
int sn_rm_ray_composite_backward(const float *weights, const float *rays_t, const float *raw, const float *rays_d, const float *grad_weights_sum,
                                 const float *grad_depth, const float *grad_f_image, uint32_t N, uint32_t T, float *grad_weights, float *grad_raw,
                                 sn_stream_t stream);

/* sn_rm_proposal_loss with every written value multiplied by scale * (scale_dev ? *scale_dev : 1): the mean's 1 / (N Tr) and autograd's
 * incoming (device-resident) gradient scalar without extra elementwise passes. */
int sn_rm_proposal_loss_scaled(const float *bins, const float *weights, const float *ref_bins, const float *ref_weights, uint32_t N, uint32_t T,
                               uint32_t Tr, float scale, const float *scale_dev, float *loss_per_ray, float *grad_weights, sn_stream_t stream);

/* The same for ANY number of samples per ray (T, Tr <= 512 run exactly sn_rm_proposal_loss_scaled's launch and need no workspace; longer rays keep
 * their prefix sums and search tables in `workspace` -- 8-byte aligned, sn_rm_proposal_loss_workspace_bytes(N, T, Tr, backward) bytes, at most
 * 64 MiB -- and a wave walks several rays: the same operations in the same order, the same bits). */
size_t sn_rm_proposal_loss_workspace_bytes(uint32_t N, uint32_t T, uint32_t Tr, int backward);
int sn_rm_proposal_loss_long(const float *bins, const float *weights, const float *ref_bins, const float *ref_weights, uint32_t N, uint32_t T,
                             uint32_t Tr, float scale, const float *scale_dev, float *loss_per_ray, float *grad_weights, void *workspace,
                             size_t workspace_bytes, sn_stream_t stream);

/* Clears `bytes` bytes at `ptr` (both multiples of 16) with a kernel on `stream` -- capturable in a HIP graph, unlike a memset node whose
 * replays faulted once the allocator had reused the memory (round 4); the zeros_like of gridencoder/grid.py:83. */
int sn_zero(void *ptr, size_t bytes, sn_stream_t stream);

/* nerf/renderer.py:333-338,361,384: out[n,k] = sum_t weights[n,t] * values[n,t,k]  (K may be 1). */
int sn_rm_composite(const float *weights, const float *values, uint32_t N, uint32_t T, uint32_t K,
                    float *out, sn_stream_t stream);
/* backward of sn_rm_composite w.r.t. values: grad_values[n,t,k] = weights[n,t] * grad_out[n,k] */
int sn_rm_composite_backward(const float *weights, const float *grad_out, uint32_t N, uint32_t T, uint32_t K,
                             float *grad_values, sn_stream_t stream);

/* ---- fused whole-path render: nerf/renderer.py:221-357 + network.py:146-186 ---- */
typedef struct sn_grid_desc {
    const void *embeddings;                 /* device */
    int32_t     table_dtype;                /* SN_F32 / SN_F16 */
    int32_t     offsets[SN_MAX_LEVELS + 1]; /* host values */
    uint32_t    D, C, L;
    float       S;                          /* (float)log2(per_level_scale) */
    uint32_t    H;                          /* base resolution */
    uint32_t    gridtype, align_corners, interp;
} sn_grid_desc;

typedef struct sn_mlp_desc {
    const float *weight[SN_MAX_LAYERS];     /* device, [out,in] row-major = nn.Linear.weight */
    const float *bias[SN_MAX_LAYERS];       /* device or NULL */
    uint32_t     dims[SN_MAX_LAYERS + 1];
    uint32_t     num_layers;
    uint32_t     activation;                /* 0 relu, 1 leaky_relu(0.01) */
    uint32_t     skip_mask;
} sn_mlp_desc;

/* Kernel selection of sn_rm_render_rays, read from the caller's cfg on every call (ABI <= 6 read process-wide environment variables
 * instead).  All zero = the defaults.  None of these changes WHAT is computed beyond fp32 round-off; the notes say which are bit-neutral. */
enum { SN_MLP_AUTO = 0, SN_MLP_F16X3 = 1, SN_MLP_MFMA32 = 2, SN_MLP_VALU = 3, SN_MLP_F16X1 = 5 };
enum { SN_EXP_NONE = 0, SN_EXP_ROLE_SPLIT = 1, SN_EXP_LDS_LEVEL0 = 2, SN_EXP_FINAL_ONE_WG = 3,
       SN_EXP_MATRIX_CLUMPED = 4,    /* linear-tail last stage: the matrix phase in its order before round 9 (tile by tile, vector work in clumps); bit-identical */
       SN_EXP_GATHER_CANONICAL = 5   /* last stage on packed levels: hashed-level gathers in the canonical corner order instead of grouped by cell parity (round 10); bit-identical */ };
typedef struct sn_render_tuning {
    int32_t mlp_mode;            /* SN_MLP_AUTO: split-fp16 on the matrix cores unless cfg.mlp_exact_fp32; SN_MLP_F16X3 forces it (overrides the
                                  * range guard); SN_MLP_MFMA32: exact fp32 v_mfma_f32_32x32x2_f32; SN_MLP_VALU: vector-ALU fallback (A/B of the layouts);
                                  * SN_MLP_F16X1 (opt-in measurement mode, NOT fp32-class: RGB 3e-4 from the reference on the stress-init fixtures, over
                                  * the 1e-4 bar; honoured by the plain last-stage launch with fp16 tables, F16X3 elsewhere): one product per multiply --
                                  * plain fp16 operands, fp32 accumulation: what an autocast fp16 run of the reference multiplies */
    int32_t per_sample_form;     /* 1: the last stage evaluates the third MLP layer per sample everywhere (no "linear tail"): bit-identical to
                                  * the compacting / several-lanes-per-ray kernels, fp32 round-off away from the default */
    int32_t densify;             /* hashed levels 5-6 of the main grid re-laid out per call like dense levels (bit-neutral): 0 automatic (fp16
                                  * tables and >= 64 M last-stage samples), 1 never, 2 whenever the kernel exists for the call */
    int32_t linear_tile_order;   /* image mode: which tile a workgroup renders (bit-neutral; sn_rm_tile_order_info states each order on the host).
                                  * 1: workgroup b renders tile b, tiles walked in whole pairs of wave-tile rows (no XCD-aware remap);
                                  * 2: every XCD owns a contiguous range of tile ids, same walk;
                                  * 3: the same ranges over tiles walked in 128x128-pixel super-tiles (8x8 workgroup blocks), rows of super-tiles in
                                  *    alternating direction: the 64 workgroups in flight on one XCD cover a compact square.  6 % fewer L2 requests go
                                  *    on to the fabric than under 2 -- and the last stage is 2.3 % SLOWER (profiles/r08/): opt-in, for measurements;
                                  * 4: the same with 48x48-pixel super-tiles (3x3 blocks): 2 % faster than 2 at 800x800; 0: the default (4) */
    int32_t prop_sp_max_rays;    /* linear-order batches up to this many rays run the proposal stages with 8 lanes per ray (bit-neutral):
                                  * 0 default (32768), < 0 never */
    int32_t final_sp_max_rays;   /* the same for the last stage (several lanes per ray, per-sample form): 0 default (16384), < 0 never */
    int32_t feat_levels;         /* levels per workgroup pass of the feature stage: 0 default (2), 1, 2 or 4 (bit-neutral) */
    int32_t band_streams;        /* image mode, schedules with proposal stages: the image is rendered as two row bands whose kernels go to TWO HIP streams
                                  * (the caller's and a library-owned one, forked and joined with events inside the call: capturable), so that
                                  * the vector-ALU-bound proposal stages of one band overlap the texture-path-bound last stage of the other
                                  * (bit-neutral): 0 automatic (>= 768 workgroups: 800x800 [128,64,32] 4.36 -> 4.07 ms fp32, 3.85 -> 3.71 fp16; 448x448 2.10 -> 2.00, 1.88 -> 1.74;
                                  * >= 512 with the feature stage: 400x400 + SAM head 3.00 -> 2.82 ms), 1 never, 2 whenever the image has two bands
                                  * of whole tile rows, K > 2: K bands dealt alternately to the two streams (measured, profiles/r05/band_count_ab.txt: two bands
                                  * are the optimum at 400 / 800 / 1600 pixels -- 800x800 fp16: 3.84 none, 3.59 two, 4.18 four; 1600x1600: 13.36, 12.71, 12.70) */
    int32_t exact_early_out;     /* the last stage leaves the march once the transmittance of all 64 rays of a wave has underflowed to EXACTLY 0 (every later
                                  * weight is alpha * 0: bit-neutral; opaque scenes only): 2 = on, 0 / 1 = off (the default: behind proposal stages it buys nothing, in a
                                  * single-stage schedule 6.07 -> 4.43 ms on an opaque field at 0.5-1 % cost on a semi-transparent one).
                                  * The proposal stages always do (their remaining weights are written as 0 without evaluating the density). */
    int32_t wave_tile;           /* image mode: the 64 lanes of a wave cover 2^w x 2^(6-w) pixels: 0 default (8x8), 1..5 = w (2x32 ... 32x2); bit-neutral
                                  * (A/B of the lines a gather instruction touches: profiles/r05/tile_shape_ab.txt) */
    int32_t prop_sp_lanes;       /* small linear-order batches, proposal stages: lanes that share a ray: 0 automatic (32: the fastest from 1024 to
                                  * 32768 rays, profiles/r06/prop_sp_lanes_ab.json), or 8 / 16 / 32 (bit-neutral) */
    int32_t feat_patch;          /* feature stage, dense levels: 1 = a wave fetches the bounding box of its rays' vertices once into LDS and the lanes read their
                                  * corners there (north_star "LDS staging of per-tile grid voxels"; bit-neutral).  0 default = off: measured 3-9 % SLOWER than
                                  * the direct gathers (profiles/r06/feat_patch_ab.json) */
    int32_t prop_pair;           /* proposal stages (one lane per ray): a lane evaluates TWO consecutive samples at once -- their gathers and MLP chains interleave
                                  * (k_prop_stage<..., UN = 2>, 3 waves per SIMD instead of 5; bit-neutral): 0 automatic, 1 never, 2 always */
    int32_t experiment;          /* SN_EXP_*: variants that were built, verified bit-identical and measured SLOWER; honoured only by
                                  * a library built with -DSN_EXPERIMENTS (sn_build_flags), SN_ERR_UNSUPPORTED otherwise */
    int32_t persistent_tiles;    /* last stage, plain linear-tail launch (no feature stage, no early stop or early-out, full product form): ONE resident
                                  * workgroup of 8 waves per CU stages the weights once and every wave pulls 64-ray wave tiles from eight queues, one per
                                  * XCD range of linear_tile_order (sn_rm_tile_queue_info states them), instead of one 4-wave workgroup per 256-ray tile
                                  * (bit-neutral): 0 automatic (launches with more wave tiles than 8 x the device's CUs; with two row bands on two streams, than 32 x),
                                  * 1 never, 2 always */
    int32_t persistent_wgs;      /* workgroups of that launch: 0 = one per CU, n = exactly n (measurements and tests: any n >= 1 renders every tile) */
} sn_render_tuning;

typedef struct sn_render_cfg {
    uint32_t     num_stages;                /* len(opt.num_steps), 1..SN_MAX_STAGES */
    uint32_t     num_steps[SN_MAX_STAGES];
    sn_grid_desc prop_grid[SN_MAX_STAGES];  /* stages 0..num_stages-2 (network.py:131-143) */
    sn_mlp_desc  prop_mlp[SN_MAX_STAGES];
    /* The field.  Two last-stage kernels exist: the reference network's own sizes (network.py:93-98: L=16, level_dim 2,
     * 32-64-64-16 and 31-32-32-3 bias-free ReLU MLPs) run on the matrix cores; any OTHER field of the same structure
     * (renderer.py:221-357 is size-agnostic) -- 3-D grid with level_dim 2 and <= 64 features, bias-free ReLU MLPs of <= 4
     * layers and <= 64 neurons, grid_mlp -> [sigma_raw | <= 31 geometry channels], view_mlp input = geometry channels + 16 SH
     * values, 3 outputs -- runs in a size-agnostic kernel (fp32 fmaf chains).  Other fields: SN_ERR_UNSUPPORTED. */
    sn_grid_desc grid;                      /* network.py:93 */
    sn_mlp_desc  grid_mlp;                  /* network.py:94: -> [sigma_raw | geo_feat] */
    sn_mlp_desc  view_mlp;                  /* network.py:98: per ray, after compositing */
    uint32_t     sh_degree;                 /* network.py:97 */
    float        aabb[6];
    float        min_near;
    float        bound;                     /* grid bound: 2 when opt.contract */
    int32_t      contract;
    int32_t      last_sample_opaque;        /* opt.background == 'last_sample' */
    float        bg_color;
    /* optional feature stage (renderer.py:301-302 + 361): f_feat[n,:] = sum_j w[n,j] * feat_grid(xyz[n,j]) over the
     * last stage's samples -- the SAM head's f_sam with feat_grid = s_grid (network.py:103) */
    sn_grid_desc feat_grid;
    int32_t      with_feat;
    /* opt-in, NOT reference behaviour (the reference always evaluates every sample): in the last stage a wave (8x8
     * pixels) stops marching once the transmittance of all its rays is below this value; 0 = off (default).  Every
     * output changes by at most ~eps * |feature|.  Ignored when per-sample outputs or the feature stage are on. */
    float        early_stop_eps;
    /* Arithmetic of the 32-64-64-16 MLP on the matrix cores.  0 (default): fp16 hi/lo-split products with fp32 accumulation
     * (2^-22 per product) -- requires every weight and activation of that MLP to stay below 65504 in magnitude, which the
     * CALLER guarantees (the Python mirror derives a bound from max|table| and the weights' row norms and sets 1 when it
     * cannot).  1: exact fp32 v_mfma_f32_32x32x2_f32 (no range limit, ~2.2x slower final stage).  tuning.mlp_mode != SN_MLP_AUTO
     * overrides this field. */
    int32_t      mlp_exact_fp32;
    /* opt-in, NOT reference behaviour: the last stage runs with per-ray termination and wave-level compaction of live
     * samples (k_final_stage_cmp).  A ray stops taking samples once its transmittance is below early_stop_eps (if > 0),
     * rays that miss the aabb (renderer.py:133-135: near = far = 1e9) and lanes beyond the image edge take none, and each
     * wave deals its 64 evaluation slots (gather lanes, rows of the MFMA tile) out to the rays still live, found with a
     * ballot + prefix count per iteration.  With nothing to skip the outputs are bit-identical to the default kernel; a
     * terminated ray changes every output by at most ~eps * |feature|; a missed ray gets weights_sum = depth = 0 and the
     * background colour (the reference marches such rays through inf / NaN distances; with its default options every
     * weight comes out 0 as well).  Ignored (default kernel runs) when per-sample outputs or the feature stage are on,
     * for tables the FinalLv fast path does not cover, and in the exact-fp32 / VALU MLP modes. */
    int32_t      compact_live;
    sn_render_tuning tuning;
} sn_render_cfg;

typedef struct sn_render_io {
    /* inputs */
    const float *rays_o, *rays_d;           /* [N,3] device */
    const float *cam_near_far;              /* [N,2] device or NULL */
    uint32_t     N;
    uint32_t     tile_w;                    /* >0: rays are a row-major image of this width; lanes map to 8x8 pixel tiles */
    const float *bins0_table;               /* device [num_steps[0]+1], or per ray [N, bins0_ray_stride], or NULL (-> linspace recipe) */
    const float *u_table[SN_MAX_STAGES];    /* device [num_steps[k]+1] for k>=1, or per ray [N, u_ray_stride[k]], or NULL */
    uint32_t     bins0_ray_stride;          /* 0: bins0_table is one table shared by all rays; else floats per ray (>= num_steps[0]+1):
                                             * the per-ray perturbed bins of a training step (renderer.py:267-270) */
    uint32_t     u_ray_stride[SN_MAX_STAGES]; /* the same for u_table[k]: sample_pdf's perturbed u (renderer.py:101-102) */
    int32_t      skip_final;                /* != 0: run the proposal stages only and write the LAST stage's resampled bins to
                                             * bins[num_stages-1] ([N,T_last+1]); image / depth / weights_sum may be NULL.  A training
                                             * step whose proposal networks are not updated (trainer.py:372-373: 4 steps of 5 after step
                                             * 3000) takes its final-stage sample positions from here and differentiates only that stage */
    /* outputs */
    float       *image;                     /* [N,3] */
    float       *depth;                     /* [N] */
    float       *weights_sum;               /* [N] */
    uint32_t     out_stride;                /* 0: the three outputs above are dense arrays.  s >= 5: each is a COLUMN RANGE of a row-major buffer whose
                                             * rays are s floats apart (image[n*s + 0..2], depth[n*s], weights_sum[n*s]): a band that feeds the
                                             * image all-gather is written straight into its [N,5] payload (image = p, depth = p+3, weights_sum = p+4) */
    /* optional per-stage outputs, [N, ...] row-major like the reference tensors; NULL = not wanted */
    float       *bins[SN_MAX_STAGES];       /* [N,T_k+1] */
    float       *weights[SN_MAX_STAGES];    /* [N,T_k]   */
    float       *sigmas[SN_MAX_STAGES];     /* [N,T_k]   */
    int32_t     *inds[SN_MAX_STAGES];       /* [N,T_k+1], k>=1 */
    float       *xyzs_last;                 /* [N,T_last,3] contracted positions of the last stage */
    float       *geo_feat_last;             /* [N,T_last,geo] per-sample geometry features (feeds the mask head) */
    float       *f_image;                   /* [N, geo+sh] composited colour features (feeds the SAM head) */
    float       *f_feat;                    /* [N, L*C of cfg->feat_grid]; required when cfg->with_feat */
    uint32_t     head_stride;               /* 0: f_image / f_feat are dense arrays.  s > 0: both are COLUMN RANGES of one row-major [N, s] buffer -- the SAM head's
                                             * MLP input cat([f_sam, f_image, image, depth]) of renderer.py:366 written in place of a concatenation: rows are s floats
                                             * apart, and rgb | depth of ray n are written once more at f_image + n*s + 31 (4 floats).  The caller points f_feat at
                                             * column 0 and f_image at column L*C, s = L*C + 31 + 4 (163 for the reference network).  Needs f_image. */
    int32_t      pack_valid;                /* (occupies what was padding: the layout of ABI 12 is unchanged.)  SN_PACK_VALID: the caller vouches that `workspace`
                                             * still holds the packed MLP weights and pair / quad rows that the PREVIOUS sn_rm_render_rays call on it wrote,
                                             * that no other call used it since, and that nothing those packs are made from has changed: the same cfg (tables,
                                             * weights, dtypes, tuning), the same route (N, tile_w, the set of optional outputs) and the same stream.  The
                                             * call then launches no pack kernel and reads the regions as they are -- a frozen field rendered from many
                                             * views.  Any other value (0 from a zeroed struct): the call packs, as it always did */
    /* workspace */
    void        *workspace;                 /* device, >= sn_rm_render_workspace_bytes() */
    size_t       workspace_bytes;
} sn_render_io;

#define SN_PACK_VALID 0x50414b31            /* sn_render_io.pack_valid: a value that uninitialised padding of an older caller will not hold */

/* bytes of device workspace sn_rm_render_rays needs for N rays (tile_w as in sn_render_io).  sn_rm_render_rays checks io->workspace_bytes
 * against this figure before its first launch (SN_ERR_WORKSPACE): for every schedule, single-stage ones included, and for both row-band
 * slots whenever the call is planned as two bands. */
size_t sn_rm_render_workspace_bytes(const sn_render_cfg *cfg, uint32_t N, uint32_t tile_w);
int sn_rm_render_rays(const sn_render_cfg *cfg, const sn_render_io *io, sn_stream_t stream);
/* What the last sn_rm_render_rays call of THIS THREAD launched as its last stage (measurement: bench.py prices the gather stream of the
 * kernel that really ran).  final_kernel: "k_final_stage<lt,K=7>", "k_final_stage_sp", ...; dense_levels: levels of the main grid read
 * as packed pair / quad rows; gathers_per_wave_sample: 64-lane gather instructions one sample of one wave issues in that kernel. */
typedef struct sn_launch_info {
    char     final_kernel[64];
    uint32_t workgroups, lds_bytes, dense_levels, gathers_per_wave_sample, launches;
    /* workgroups counts 256-ray TILE UNITS of the launch (what the grid of the ordinary launch is) whichever form ran; persistent_tiles: 1 when the
     * persistent form ran (tuning.persistent_tiles), whose real grid -- 512-thread workgroups -- is grid_workgroups (= workgroups otherwise) */
    uint32_t persistent_tiles, grid_workgroups;
} sn_launch_info;
int sn_rm_last_launch_info(sn_launch_info *info);
/* Dry run: what sn_rm_last_launch_info would report after a successful sn_rm_render_rays(cfg, io) -- the last chunk's workgroups, launches =
 * last-stage launches over all chunks, all zero for skip_final -- from the same validation and the same route planning, on the host alone:
 * nothing is launched, no pointer is dereferenced, io->workspace is not needed.  Same statuses and messages as sn_rm_render_rays.
 * (lds_bytes is the dynamic LDS of the launch itself, the 84 KiB of SN_EXP_FINAL_ONE_WG included.) */
int sn_rm_render_route_info(const sn_render_cfg *cfg, const sn_render_io *io, sn_launch_info *out);
/* The same for a device of `compute_units` CUs: sn_rm_render_rays asks its device once and plans with that figure; the call above plans
 * with 0 = not known, under which the automatic rule of tuning.persistent_tiles stays off (and a forced persistent launch is sized for 256). */
int sn_rm_render_route_info_cus(const sn_render_cfg *cfg, const sn_render_io *io, uint32_t compute_units, sn_launch_info *out);

/* The tile queues of the persistent last stage (tuning.persistent_tiles), on the host alone (no HIP call, the arithmetic the kernel runs): a
 * launch of `units` 256-ray tile units (sn_launch_info.workgroups) has wave_tiles = 4 * units wave-tile ids, the ids sn_rm_tile_order_info walks
 * as tile_id * 4 + wave; queue `queue` (0..7) holds [begin, end): 4 x the contiguous tile range linear_tile_order = `order` gives XCD `queue`,
 * or, for the orders without that remap (1), everything in queue 0.  The eight ranges partition the ids. */
typedef struct sn_tile_queue_info {
    uint32_t queues, wave_tiles, begin, end;
} sn_tile_queue_info;
int sn_rm_tile_queue_info(uint32_t units, int32_t order, int32_t wave_tile, uint32_t queue, sn_tile_queue_info *out);

/* Which part of a W x rows image (one launch: a whole image, a row band, a row chunk) workgroup `workgroup` (blockIdx.x) of the render stages
 * takes under tuning.wave_tile / tuning.linear_tile_order = `order`, on the host alone: no HIP call, the same arithmetic the kernels run.
 * workgroups: the launch's grid; tile_id: the linear tile the workgroup renders (its column block in the stages' scratch: tile_id * 256);
 * x[w], y[w]: pixel origin of the tile_w x tile_h wave tile of wave w, -1 for the padding of the last workgroup.  Over all workgroups the
 * wave tiles cover every wave tile of the image exactly once, for every order and shape. */
typedef struct sn_tile_order_info {
    uint32_t workgroups, tile_id, tile_w, tile_h;
    int32_t  x[4], y[4];
} sn_tile_order_info;
int sn_rm_tile_order_info(uint32_t W, uint32_t rows, int32_t wave_tile, int32_t order, uint32_t workgroup, sn_tile_order_info *out);

/* Feature-head accumulation, nerf/renderer.py:301-302 + 361: out[n, :] = sum_j weights[n,j] * grid(xyzs[n,j])
 * = composite(weights, s_grid(xyzs, bound)) without materialising the [N*T, L*C] per-sample features.
 * xyzs [N,T,3] (contracted sample positions), weights [N,T], out [N, L*C]; tile_w > 0: rays are a row-major image
 * of that width (lanes map to 8x8 pixel tiles).  Forward only (inference); training goes through
 * sn_grid_encode_* + sn_rm_composite*. */
int sn_rm_grid_composite(const float *xyzs, const float *weights, uint32_t N, uint32_t T, float bound,
                         const sn_grid_desc *grid, uint32_t tile_w, float *out, sn_stream_t stream);

/* Wide perceptron of the feature heads on the matrix cores: nerf/network.py:31-66 (SkipConnMLP) followed by an
 * optional nn.LayerNorm (network.py:115) -- samvit_mlp per ray (renderer.py:359-374), mask_mlp per sample
 * (renderer.py:376-385).  x [N, dims[0]] -> out [N, dims[num_layers]].  Hidden widths must be 256, the output
 * width <= 256; bias optional per layer; activation 0 relu / 1 leaky_relu(0.01); skip_mask bit l: layer l sees
 * cat([h, x]).  fp32 in / out; products run as fp16 hi+lo splits with fp32 accumulation (activations must stay
 * inside the fp16 range, |v| < 65504).  workspace: >= sn_mlp_wide_workspace_bytes(), 16-byte aligned (holds the
 * re-ordered weights, rebuilt on every call: the call is stateless).  ln_weight/ln_bias NULL = no LayerNorm. */
size_t sn_mlp_wide_workspace_bytes(const sn_mlp_desc *mlp);
/* Range check of the split-fp16 arithmetic: sn_mlp_wide_forward raises a sticky device-side flag when an output row is not
 * finite (what an activation beyond the fp16 range produces).  Reads and clears it: *flag = 1 if any call since the last
 * read overflowed.  Synchronises the device. */
int sn_mlp_wide_overflow(int32_t *flag);
int sn_mlp_wide_forward(const sn_mlp_desc *mlp, const float *ln_weight, const float *ln_bias, float ln_eps,
                        const float *x, uint32_t N, float *out, void *workspace, size_t workspace_bytes,
                        sn_stream_t stream);

/* Mask head (nerf/renderer.py:304-305, 376-385; network.py:104, 118-123) in one kernel:
 *   out[n, :] = sum_t weights[n,t] * mask_mlp(cat([m_grid(xyzs[n,t]), extra[n,t]]))        out [N, dims[num_layers]]
 * xyzs [N,T,3] (contracted sample positions; x01 = (xyz + bound) / (2 bound) as gridencoder/grid.py:156), extra [N,T,E]
 * (the detached geometry features, E <= 16), weights [N,T].  The lanes of the matrix-core MLP kernel interpolate the grid
 * levels of their samples straight into the first layer's B operand and the epilogue composites the logits, so neither
 * the [N*T, L*8+E] input nor the [N*T, n_inst] logits are written.  (T >= 4: a workgroup walks the samples of 32
 * consecutive rays -- neighbouring rays at one depth share table lines; rays are expected in image order.)  Needs a 3-D fp32 grid with level_dim 8, hidden width
 * 256, <= 32 outputs, no skip layers, T a power of two <= 128; anything else returns SN_ERR_UNSUPPORTED and the caller
 * composes sn_grid_encode_forward_cat + sn_mlp_wide_forward + sn_rm_composite.  Inference only.  Range of the split-fp16
 * arithmetic as sn_mlp_wide_forward (the overflow flag is not raised by this entry).  workspace >=
 * sn_rm_mask_head_workspace_bytes(), 16-byte aligned. */
size_t sn_rm_mask_head_workspace_bytes(const sn_mlp_desc *mlp);
int sn_rm_mask_head(const float *xyzs, const float *extra, const float *weights, uint32_t N, uint32_t T, uint32_t E,
                    float bound, const sn_grid_desc *grid, const sn_mlp_desc *mlp, float *out,
                    void *workspace, size_t workspace_bytes, sn_stream_t stream);

/* Render a segmented object alone (NeRFRenderer.render_object): a per-sample label gate on the densities of the last stage, in two launches.
 * (The reference names the feature -- main.py:183-185 --render_mesh / --render_mask_instance_id, trainer.py:711-713 outputs['mesh_image'] --
 * and does not deliver it; this is the project's own definition, and tests/object_ref64.py states it in fp64.)
 *
 * Take one ray and the T samples of the LAST stage of the ordinary render (proposal stages are not gated: the sample positions are exactly
 * those of render(..., return_mask=1)): densities sigma_i, real bin edges b_0 .. b_T with delta_i = b_{i+1} - b_i, mid-points
 * t_i = (b_{i+1} + b_i) / 2, geometry channels geo_i in R^15, positions x_i.
 *   1. l_i = mask_mlp(cat[m_grid(x_i), geo_i]) in R^K;  label_i = the lowest index attaining max_k l_i,k
 *   2. g_i = (label_i in S) xor invert;  S = a set of instance ids, passed as a 32-bit keep mask (K <= 32); invert renders the scene
 *      without the object
 *   3. y_i = g_i ? delta_i sigma_i : 0 -- a select, not a product: a gated-out sigma = inf gives 0, not NaN.  With last_sample_opaque
 *      (opt.background == 'last_sample'): y_{T-1} = g_{T-1} ? +inf : 0
 *   4. alpha_i = 1 - exp(-y_i);  T_i = exp(-sum_{j<i} y_j);  w'_i = alpha_i T_i, NaN -> 0 as sn_rm_weights_from_sigma
 *   5. weights_sum = sum w'_i (the object's alpha matte);  depth = sum w'_i t_i;
 *      f_image = [sum w'_i geo_i | (sum w'_i) SH4(d / |d|)], 31 values, as sn_rm_ray_composite builds it;
 *      object_image = sigmoid(view_mlp(f_image)) + (1 - sum w') bg   (the per-ray head, not part of these entries)
 * w'_i can be non-zero where the ordinary weight w_i is exactly 0 (the occluder in front is gated away): nothing is keyed on a weight.
 *
 * sn_rm_mask_point_labels: step 1 in the one-kernel mask head (sn_rm_mask_head's matrix-core kernel with a label epilogue: the logits stay
 * in registers).  xyzs [N,T,3], extra [N,T,E], live [N,T] -> labels [N,T] uint8 and, if logits != NULL (tests, tools; NULL in production),
 * logits [N,T,K] fp32 from the same registers.  `live` is y = delta sigma: a tile of 128 samples (rays 32 r .. 32 r + 31 x depth indices
 * 4 p .. 4 p + 3) whose live values are all exactly 0 is skipped; its labels are 255 and its logits 0 (both outputs are filled on the
 * stream first).  255 appears only where live == 0.  A NaN logit never wins; a row of NaN / -inf logits gets label 0.
 * Accepts what sn_rm_mask_head's 16-row kernel accepts -- 3 bias-free layers, hidden width 256, K <= 16, E <= 16, <= 16 levels of a 3-D
 * fp32 level_dim-8 grid of the fast-path shape, T a power of two in 4 .. 128 -- and answers SN_ERR_UNSUPPORTED (with a message) otherwise:
 * there is no second route.  workspace >= sn_rm_mask_head_workspace_bytes(), 16-byte aligned.  Deterministic: two calls give equal bits.
 *
 * sn_rm_object_composite: steps 2-5 in one launch.  labels [N,T] uint8 (a value >= 32, such as 255, is in no S), sigmas [N,T],
 * real_bins [N,T+1], geo_feat [N,T,15], rays_d [N,3] un-normalised -> weights_sum [N], depth [N], f_image [N,31] and, if != NULL,
 * weights [N,T] = w'.  16 lanes per ray; every sum runs in sample order (the prefix of y in fp64), so a ray's results do not depend on N. */
int sn_rm_mask_point_labels(const float *xyzs, const float *extra, const float *live, uint32_t N, uint32_t T, uint32_t E,
                            float bound, const sn_grid_desc *grid, const sn_mlp_desc *mlp, uint8_t *labels, float *logits,
                            void *workspace, size_t workspace_bytes, sn_stream_t stream);
int sn_rm_object_composite(const uint8_t *labels, const float *sigmas, const float *real_bins, const float *geo_feat, const float *rays_d,
                           uint32_t N, uint32_t T, uint32_t keep_mask, int32_t invert, int32_t last_sample_opaque, float *weights_sum,
                           float *depth, float *f_image, float *weights, sn_stream_t stream);

/* Vertex colours and instance labels of an exported mesh (NeRFRenderer.vertex_attributes, extract_mesh(vertex_colors, vertex_labels)):
 * surface probes.  The colour head is deferred -- pixel = sigmoid(view_mlp([sum w geo | SH4(d)])) -- so a vertex is shaded the way a pixel
 * is: by a short ray that enters the surface head-on, composited and normalised.  (The project's own definition; the reference has none.
 * tests/mesh_attr_ref64.py states it in fp64.)
 *
 * Per vertex: a position v and a mesh normal n that points out of the inside.  K in {4, 8, 16, 32} probe samples, step h (finite, > 0).
 *   1. Direction   d = -n / |n|; (0, 0, -1) where |n| is 0 or not finite (a NaN or inf component included).  In fp32: m = the largest
 *                  |n_a|, s = n / m, len = sqrt((s_x s_x + s_y s_y) + s_z s_z), d_a = -(s_a / len) -- no square overflows or vanishes.
 *   2. Positions   t_i = (i + 1/2 - K/2) h for i = 0 .. K-1 (the factor is exact: one rounding); p_i = v + t_i d per axis, the product and
 *                  the sum rounded separately, as sn_rm_lattice_points; contract != 0: then through sn_rm_contract's arithmetic.  The probe
 *                  starts outside (t < 0) and ends inside.
 *   3. Queries     sigma_i, geo_i in R^15 from the main field at p_i, label_i from the mask head (sn_rm_mask_point_labels) -- the
 *                  existing operators.  A label >= 32 (255 = "not evaluated") is in no set.
 *   4. Gate        g_i = (label_i in S) xor invert; g_i = true when no labels are given.  y_i = g_i ? h sigma_i : 0 -- a select.
 *   5. Weights     w_i = (1 - exp(-y_i)) exp(-sum_{j<i} y_j), the prefix summed in fp64 in sample order, NaN -> 0: exactly
 *                  sn_rm_object_composite's weight.  There is no opaque last sample.
 *   6. Coverage    W = sum w_i;  G = sum w_i geo_i.  Where W >= 2^-126: g = G / W.  Otherwise (nothing kept, or empty space) the fallback
 *                  g = (sum_i geo_i) (1 / K) over all K samples, ungated, in sample order.
 *   7. Colour      f = [g | SH4(d / |d|)], 31 values; colour = sigmoid(view_mlp(f)) -- the per-ray head, not part of these entries.
 *   8. Label vote  (only with labels) vote_l = sum_{i: label_i = l} w_i for l < 32, in fp32 in sample order; the vertex label is the lowest
 *                  l attaining the maximum vote if that maximum is > 0, else 255.
 * The order of every sum is a function of K alone: a vertex's result does not depend on V, on the launch grid or on chunking.
 *
 * sn_rm_vertex_probe_points: steps 1-2 for the vertices first .. first + count - 1 of vertices / normals [V_total,3] -> xyz [count,K,3],
 * dirs [count,3].  count == 0 returns SN_OK without touching a pointer; count K < 2^32.
 * sn_rm_vertex_probe_composite: steps 4-8 but the perceptron, in one launch.  labels [V,K] uint8 or NULL (no gate, no vote), sigmas [V,K],
 * geo_feat [V,K,15] (16-byte aligned), dirs [V,3] -> f [V,31], coverage [V] and, if != NULL (needs labels), vertex_label [V] uint8.
 * 16 lanes per vertex; a workgroup reads the geometry of its 16 vertices as one contiguous block.  V == 0 returns SN_OK; V < 2^28.
 * Both answer SN_ERR_UNSUPPORTED (with a message) for a K outside the set and SN_ERR_INVALID for h.  Deterministic. */
int sn_rm_vertex_probe_points(const float *vertices, const float *normals, uint32_t V_total, uint32_t first, uint32_t count, uint32_t K,
                              float h, int32_t contract, float *xyz, float *dirs, sn_stream_t stream);
int sn_rm_vertex_probe_composite(const uint8_t *labels, const float *sigmas, const float *geo_feat, const float *dirs, uint32_t V, uint32_t K,
                                 float h, uint32_t keep_mask, int32_t invert, float *f, float *coverage, uint8_t *vertex_label,
                                 sn_stream_t stream);

/* Geometry export (NeRFRenderer.density_volume / extract_mesh): the object, or the whole scene, taken out of the field as a triangle mesh.
 * (The reference offers --render_mesh / --density_thresh, main.py:183-185, imports mcubes and trimesh, nerf/renderer.py, and calls neither.
 * The definition below is this project's; tests/mesh_ref.py restates it operation for operation, and topology pins the restatement.)
 *
 * sn_rm_lattice_points: positions of the lattice vertices first .. first + count - 1 of an nx x ny x nz lattice -> xyz [count,3].  Linear
 * index (x ny + y) nz + z, z fastest; p_a = origin_a + (float)i_a * step_a, the product and the sum rounded separately; contract != 0: then
 * through the contraction of sn_rm_contract.  Bit-equal to that operator on the same lattice made with torch; it spares a meshgrid per chunk.
 * origin, step: 3 floats each on the HOST.  count == 0 returns SN_OK without touching a pointer.
 *
 * Marching tetrahedra.  volume [nx,ny,nz] fp32, z fastest.
 *   Inside test     a lattice vertex is inside iff f > iso, evaluated in fp32: NaN is outside, +inf is inside, a value equal to iso is outside.
 *   Edge slots      each lattice vertex owns up to 7 edges: slot e goes to the vertex at offset (1,0,0),(0,1,0),(0,0,1),(1,1,0),(1,0,1),
 *                   (0,1,1),(1,1,1) for e = 0..6, where that vertex is in range.  An edge carries a mesh vertex iff its two ends differ in
 *                   inside-ness.
 *   Position        t = (iso - f_a) / (f_b - f_a) in fp32 with IEEE division, a the owning end; if !(t >= 0 && t <= 1) then t = 0.5 (NaN,
 *                   inf/inf).  Per axis pos = origin + ((float)i + t e) step, each operation rounded on its own (e = the offset's 0 or 1).
 *   Vertex order    by the owning lattice vertex's linear index, then slot: id(v,e) = base[v] + popcount(mask[v] & ((1 << e) - 1)).
 *   Tetrahedra      a cell is identified by its lowest corner; its six tetrahedra are the Kuhn paths v0 = (0,0,0) -> v0 + e_p1 -> + e_p2 ->
 *                   (1,1,1) for the six axis permutations p in lexicographic order.  (The diagonal of every cube face runs from the face's
 *                   lowest to its highest corner, the same for both cubes that share the face: no ambiguous cases, watertight by construction.)
 *   Triangles       per tetrahedron, corners in path order.  One inside corner I and outside corners O0,O1,O2: (I,O0),(I,O1),(I,O2).  Three
 *                   inside corners: (I0,O),(I1,O),(I2,O).  Two: the quad a=(I0,O0), b=(I0,O1), c=(I1,O1), d=(I1,O0) as (a,b,c),(a,c,d).
 *   Orientation     each triangle is flipped (its last two vertices swapped) so that its normal points from inside to outside.  Decided once,
 *                   when the 16 x 6 table is generated (csrc/mesh_table.h, at compile time), from the edge mid-points on the unit lattice and
 *                   the centroids of the inside and outside corners -- never from run-time positions, which lose consistency on zero-area
 *                   triangles.
 *   Triangle order  by cell linear index (x (ny-1) + y)(nz-1) + z, then tetrahedron, then triangle.
 *   Degenerate      zero-area triangles (a mesh vertex sitting on a lattice vertex) are kept: the topology stays manifold.
 *   Normals         lattice gradient by central differences (f[i+1] - f[i-1]) / (2 step), one-sided (f[i+1] - f[i]) / step at the faces;
 *                   g = g_a + t (g_b - g_a) along the edge with the same t; n = -g / |g| (outward for a density), |g| =
 *                   sqrt((gx gx + gy gy) + gz gz); a zero or non-finite length gives (0,0,0).
 *
 * sn_rm_isosurface_workspace_bytes: 8 bytes per 1024 lattice vertices + 4 bytes + 1 byte per lattice vertex (each part rounded up to 16):
 * at most 8 bytes per lattice vertex.  0 (with a message) for an unsupported size: a dimension < 2, or nx ny nz >= 2^31.
 * sn_rm_isosurface_count: classifies every lattice vertex (one byte: inside bit + 7 edge bits), ranks, scans, and leaves
 * counts[0..1] = {n_vertices, n_triangles} (uint32, DEVICE; 2^32 - 1 = more than that) -- two launches, the second a single workgroup.
 * sn_rm_isosurface_emit: vertices [cap_v,3] f32, normals [cap_v,3] f32 or NULL, triangles [cap_t,3] int32, from the workspace the count
 * left.  Every store is guarded by the capacities and the structure is read from the workspace alone: a volume that changed between the
 * two calls, or a capacity that is too small, truncates or misplaces the output and never writes out of bounds.  With both capacities 0
 * it returns SN_OK without touching a pointer.  origin, step: 3 floats each on the HOST.  workspace: 16-byte aligned.
 * No atomics, no workgroup waits on another: the output is identical from run to run and identical in order to the restatement.
 * Errors before any launch: SN_ERR_INVALID (NULL pointer, misaligned workspace), SN_ERR_UNSUPPORTED (size), SN_ERR_WORKSPACE. */
int sn_rm_lattice_points(const float *origin, const float *step, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t first, uint32_t count,
                         int32_t contract, float *xyz, sn_stream_t stream);
size_t sn_rm_isosurface_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int sn_rm_isosurface_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *workspace, size_t workspace_bytes,
                           uint32_t *counts, sn_stream_t stream);
int sn_rm_isosurface_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const float *origin, const float *step,
                          const void *workspace, size_t workspace_bytes, float *vertices, float *normals, int32_t *triangles,
                          uint32_t cap_v, uint32_t cap_t, sn_stream_t stream);

/* Mesh clean-up (raymarching.mesh_components / mesh_clean, NeRFRenderer.extract_mesh(min_component_triangles, keep_largest)): the connected
 * components of an indexed triangle mesh and the removal of the small ones -- floaters, label noise -- on the device (csrc/mesh_clean.hip).
 * The definition is this project's; tests/mesh_clean_ref.py restates it in numpy.
 *
 * Input: triangles [T,3] int32 and a vertex count V.  Any indexed mesh, not only the isosurface's.
 *   Valid triangle  all three indices in [0, V).  An invalid triangle connects nothing, is counted nowhere and is never emitted; every index
 *                   is range-tested before it is used as an address.  Degenerate triangles (a,a,b) and (a,a,a) are valid.  Duplicates are
 *                   valid and each counts.
 *   Component       two vertices are connected iff some valid triangle contains both, closed transitively.  labels[v] (int32) is the
 *                   smallest vertex index of v's component.  A vertex in no valid triangle is its own component with 0 triangles.
 *   Statistics      [V] arrays that are nonzero only at roots (labels[r] == r): triangle_counts[r] = the number of valid triangles of r's
 *                   component (a triangle belongs to the component of its corners), vertex_counts[r] = its number of vertices (int32);
 *                   counts[0] = the number of roots, counts[1] = the number of roots with at least one triangle (uint32, DEVICE).
 *   Key             key[r] = (uint64)triangle_counts[r] << 32 | (0xFFFFFFFF - r).  Keys are unique: a larger key means more triangles,
 *                   then the lower root index.
 *   Selection       a component is kept iff triangle_counts[r] >= max(min_triangles, 1) AND key[r] >= *min_key.  min_key is one uint64 on
 *                   the DEVICE; 0 keeps everything.  "Keep the largest k": *min_key = the k-th largest key (with k at or beyond the number
 *                   of components that have triangles, all of them are kept).
 *   Filtered mesh   a vertex is kept iff its component is; a triangle iff it is valid and its component is kept.  Kept vertices keep their
 *                   relative order, and so do kept triangles.  The new index of a vertex is its rank among the kept vertices; triangle
 *                   indices are remapped to it.  Vertex and normal rows are copied bit for bit.  source_vertex [V'] (int32, optional) =
 *                   the old index of each kept vertex.
 * The labels are a unique fixed point: they depend on neither the algorithm, the launch shape nor the run.
 *
 * sn_rm_mesh_components_init: labels[v] = v.
 * sn_rm_mesh_components_sweep: `rounds` rounds (at most 4096 per call) of two launches each over labels that init, or an earlier sweep,
 * left.  Hook, one lane per triangle: range-test a, b, c; la, lb, lc = their labels, m = the smallest; for each corner x with lx > m,
 * atomicMin(&labels[x], m) and atomicMin(&labels[lx], m).  Jump, one lane per vertex: l = labels[l] until labels[l] == l, stored by
 * atomicMin.  changed [rounds] (uint32, DEVICE; zeroed by the call): changed[i] != 0 iff round i lowered a label.  A round that lowered
 * none proves the fixed point (csrc/mesh_clean.hip has the argument): the caller sweeps until the last round of a call reports 0.  No
 * workgroup waits on another; stale reads only delay convergence; every chain that is followed strictly decreases.
 * sn_rm_mesh_component_stats: the three statistics from final labels (the arrays are zeroed by the call); integer atomic adds.
 * sn_rm_mesh_clean_workspace_bytes(V, T): 4 bytes per vertex + 4 bytes per triangle + 4 bytes per 1024 vertices + 4 bytes per 1024
 * triangles, each of the four parts rounded up to 16.  0 (with a message) if V or T >= 2^31.
 * sn_rm_mesh_filter_count: per vertex and per triangle the keep flag and the rank inside its segment of 1024, the scanned segment totals,
 * and counts[0..1] = {V', T'} (uint32, DEVICE) -- three launches, the last a single workgroup.
 * sn_rm_mesh_filter_emit: out_vertices [cap_v,3], out_normals [cap_v,3] (iff normals != NULL), out_triangles [cap_t,3], source_vertex
 * [cap_v] or NULL, from the workspace the count left and `triangles` alone (labels are not read).  Every store is guarded by the capacities
 * and every index is range-tested again: triangles that changed between the two calls, or a capacity that is too small, truncate or
 * misplace the output (an index out of range is emitted as -1) and never write out of bounds.  workspace: 16-byte aligned.
 * Every entry returns SN_OK without touching a pointer when V == 0 (the empty mesh: the caller knows every count is 0), the sweep also
 * with rounds == 0, the emit also with both capacities 0.  triangles may be NULL when T == 0.
 * Errors before any launch: SN_ERR_INVALID (NULL pointer, misaligned workspace), SN_ERR_UNSUPPORTED (V or T >= 2^31), SN_ERR_WORKSPACE.
 * Nothing is placed by an atomic: the output is identical from run to run and identical in order to the restatement. */
size_t sn_rm_mesh_clean_workspace_bytes(uint32_t V, uint32_t T);
int sn_rm_mesh_components_init(uint32_t V, int32_t *labels, sn_stream_t stream);
int sn_rm_mesh_components_sweep(const int32_t *triangles, uint32_t T, uint32_t V, int32_t *labels, uint32_t rounds, uint32_t *changed,
                                sn_stream_t stream);
int sn_rm_mesh_component_stats(const int32_t *triangles, uint32_t T, uint32_t V, const int32_t *labels, int32_t *triangle_counts,
                               int32_t *vertex_counts, uint32_t *counts, sn_stream_t stream);
int sn_rm_mesh_filter_count(const int32_t *triangles, uint32_t T, uint32_t V, const int32_t *labels, const int32_t *triangle_counts,
                            uint32_t min_triangles, const uint64_t *min_key, void *workspace, size_t workspace_bytes, uint32_t *counts,
                            sn_stream_t stream);
int sn_rm_mesh_filter_emit(const int32_t *triangles, uint32_t T, uint32_t V, const float *vertices, const float *normals,
                           const void *workspace, size_t workspace_bytes, float *out_vertices, float *out_normals, int32_t *out_triangles,
                           int32_t *source_vertex, uint32_t cap_v, uint32_t cap_t, sn_stream_t stream);

/* Mesh split (raymarching.mesh_split, NeRFRenderer.extract_object_meshes): an indexed triangle mesh with an instance label on every vertex,
 * taken apart into one mesh per label on the device (csrc/mesh_split.hip).  The definition is this project's; tests/mesh_split_ref.py
 * restates it in numpy.
 *
 * Input: vertices [V,3] fp32, normals [V,3] fp32 or NULL, triangles [T,3] int32, vertex_labels [V] uint8.  Any indexed mesh.
 *   Parts           P = SN_MESH_SPLIT_PARTS = 33.  part(label) = min(label, 32): part p < 32 is instance id p; part 32 collects every label
 *                   >= 32, 255 = "none" among them, as sn_rm_vertex_probe_composite and the object gate read such labels.
 *   Valid triangle  all three indices in [0, V).  An invalid triangle belongs to no part and is never emitted; every index is range-tested
 *                   before it is used as an address.  Degenerate triangles and duplicates are valid.
 *   Triangle part   the part that at least two of its corners have; with three different parts, the lowest.  The vote does not depend on
 *                   the rotation of the corners.
 *   Membership      vertex v belongs to part p iff some valid triangle of part p has v as a corner.  A vertex may belong to several
 *                   parts -- a seam vertex is duplicated into each -- and a vertex in no valid triangle belongs to none and is dropped.
 *   Output          packed, the parts contiguous and in part order.  part_triangle_offsets [P+1], part_vertex_offsets [P+1] (int32,
 *                   DEVICE): the first row of each part, the totals T' and V' at [P].  out_triangles [T',3]: the triangles of part p in
 *                   their input order (a stable partition) at rows part_triangle_offsets[p] ..; their indices are LOCAL to the part (row
 *                   of the vertex - part_vertex_offsets[p]), so that a slice is a stand-alone mesh.  out_vertices [V',3], and out_normals
 *                   iff normals != NULL: the members of part p in increasing input index, rows copied bit for bit.  source_vertex [V'],
 *                   source_triangle [T'] (int32, either may be NULL): the input index of every output row.  counts [2] = {V', T'} (uint32,
 *                   DEVICE); both are at most 3 T.
 * Every number is an integer or a copied bit pattern; the result depends on neither the launch shape nor the run.
 *
 * sn_rm_mesh_split_workspace_bytes(V, T): 12 bytes per vertex (the 64-bit membership word, the row in the lowest part) + 4 per triangle +
 * 2 P per 64 vertices + 4 P per 1024 vertices + 4 P per 1024 triangles, each of the six parts rounded up to 16.  0 (with a message) if V
 * or T >= 2^31.
 * sn_rm_mesh_split_count: the vote and an integer atomicOr of the part's bit into the membership words of the three corners (it places
 * nothing and is order-independent); per triangle part << 16 | rank inside its segment of 1024; per 64 vertices and part the count inside
 * the segment; the segment totals part-major, scanned by one workgroup; the two offset arrays and counts -- a memset and three launches.
 * sn_rm_mesh_split_emit: out_vertices [cap_v,3], out_normals [cap_v,3] (iff normals != NULL), out_triangles [cap_t,3], source_vertex
 * [cap_v] or NULL, source_triangle [cap_t] or NULL, from the workspace the count left and `triangles` (labels are not read; the workspace
 * is written: one word per vertex).  Every store is guarded by the capacities: a capacity below the count truncates, and the stored prefix
 * is the full result's.  Every index is range-tested again: triangles that changed between the two calls misplace rows (an index that cannot
 * be resolved is emitted as -1) and never write out of bounds.  workspace: 16-byte aligned.
 * V == 0 or T == 0 is the empty result: SN_OK; the count zeroes those of the offsets and counts that are not NULL and looks at no other
 * pointer, the emit looks at none -- nor does it with both capacities 0.
 * Errors before any HIP call: SN_ERR_INVALID (NULL pointer, normals without out_normals, cap_v > 2^31 - 1, misaligned workspace),
 * SN_ERR_UNSUPPORTED (V or T >= 2^31), SN_ERR_WORKSPACE. */
#define SN_MESH_SPLIT_PARTS 33
size_t sn_rm_mesh_split_workspace_bytes(uint32_t V, uint32_t T);
int sn_rm_mesh_split_count(const int32_t *triangles, uint32_t T, uint32_t V, const uint8_t *vertex_labels, void *workspace,
                           size_t workspace_bytes, int32_t *part_triangle_offsets, int32_t *part_vertex_offsets, uint32_t *counts,
                           sn_stream_t stream);
int sn_rm_mesh_split_emit(const int32_t *triangles, uint32_t T, uint32_t V, const float *vertices, const float *normals, void *workspace,
                          size_t workspace_bytes, float *out_vertices, float *out_normals, int32_t *out_triangles, int32_t *source_vertex,
                          int32_t *source_triangle, uint32_t cap_v, uint32_t cap_t, sn_stream_t stream);

/* Mesh simplification (raymarching.mesh_simplify, NeRFRenderer.extract_mesh(simplify)): uniform vertex clustering of an indexed triangle mesh
 * on the device (csrc/mesh_simplify.hip) -- one output vertex per occupied cell of a coarse lattice.  The definition is this project's;
 * tests/mesh_simplify_ref.py restates it in numpy.  Every quantity below is an integer or the correctly rounded result of the stated
 * operations, so the device's output EQUALS the restatement's: triangles, cluster map and counts exactly, vertices and normals bit for bit.
 * (No operation was found whose rounding cannot be pinned: the fp64 division and square root are IEEE on gfx950.)
 *
 * Input: vertices [V,3] fp32, normals [V,3] fp32 or NULL, triangles [T,3] int32 -- any indexed mesh, not only the isosurface's -- and a
 * lattice of cells: origin[3] (fp32, finite), cell[3] (fp32, > 0 and finite), dims[3] (uint32, each >= 1, product < 2^31); HOST arrays.
 *   Cell of a vertex  per axis u = p - origin and s = u / cell in fp32 (IEEE division; two roundings, no contraction), i = (int)floor(s).  A
 *                     vertex with a non-finite coordinate, or with some i outside [0, dims[a]), has NO cell: nothing is clamped, the caller
 *                     chooses a lattice that covers the mesh.  key = (ix dims[1] + iy) dims[2] + iz.
 *   Offset            q = (int)rint((s - (float)i) 65536.0f) in [0, 65536]; the subtraction and the product are exact in fp32.
 *   Triangle classes  invalid: an index outside [0, V) or a corner without a cell (every index is range-tested before it is an address).
 *                     degenerate: valid, and two corners share a cell.  duplicate: valid, not degenerate, and some triangle of LOWER index
 *                     is valid, not degenerate and has the same SET of three keys (orientation is ignored).  kept: every other triangle.
 *                     Kept triangles keep their relative order and their corner order (so their orientation).
 *   Output vertices   a cell is used iff it is a corner of a kept triangle; output vertex j is the j-th used cell in increasing key order.
 *                     Position per axis, in fp64, every operation rounded on its own, stored as fp32 with one rounding:
 *                         origin + cell ((double)i + ((double)sum_q / (double)n) / 65536.0)
 *                     sum_q (unsigned 64-bit) and n run over ALL input vertices of the cell, referenced by a triangle or not.
 *   Output normals    iff normals != NULL.  Per component Q = (int64)rint(n_a 1048576.0f) where that product is finite and below 2^31 in
 *                     magnitude, else 0 (a non-finite or absurd component contributes nothing, and no sum of < 2^31 terms can overflow);
 *                     S = sum Q (signed 64-bit) over the cell's vertices; the result is S / sqrt((Sx Sx + Sy Sy) + Sz Sz) in fp64 ((double)S
 *                     is the conversion's one rounding), no contraction, rounded once to fp32; (0,0,0) when S is zero.
 *   Cluster map       vertex_cluster [V] int32 (optional): the output index of the vertex's cell, -1 without a cell or in an unused one.
 *   Counts            {V', T'} as uint32 on the DEVICE.
 * The sums are integers, so they depend on neither the order of accumulation, the launch shape nor the run.
 *
 * sn_rm_mesh_simplify_workspace_bytes(V, T, cells), cells = the product of dims: with W = ceil(cells / 32) words of cell bitmap and C = the
 * smallest power of two >= max(2T, 1) slots of triangle table,
 *     16 + up(4V) + 2 up(4T) + up(4 ceil(T / 1024)) + up(4C) + 2 up(4W) + up(4 ceil(W / 1024)) + 64V      (up = rounded up to 16)
 * i.e. 68 bytes per vertex (a key and an 8 x 64-bit row of sums; output vertices can number at most V, so the count needs no host read
 * before it accumulates), 16 to 24 bytes per triangle and 2 bits per cell.  0 (with a message) if V, T or cells >= 2^31.
 * sn_rm_mesh_simplify_count: vertex keys; the valid, non-degenerate triangles enter an insert-only open-addressing table keyed by their key
 * set, whose slots end at the set's lowest triangle index (atomicCAS to claim, atomicMin after comparing the occupant's key set; a slot's
 * set never changes and slots never empty, so the result does not depend on the interleaving -- csrc/mesh_simplify.hip has the argument);
 * kept = the slot holds my index; kept corners set their cells' bits; used cells and kept triangles are ranked by segment and scanned by
 * one workgroup; the sums go into one row per OUTPUT vertex by 64-bit integer atomic adds, aggregated over runs of lanes of a wave.
 * counts[0..1] = {V', T'} -- six launches behind two memsets, no workgroup waits on another, no probe loop longer than the table.
 * sn_rm_mesh_simplify_emit: out_vertices [cap_v,3], out_normals [cap_v,3] (iff normals != NULL), out_triangles [cap_t,3], vertex_cluster
 * [V] or NULL, from the workspace the count left and `triangles` (`vertices` is not read, `normals` only says whether normals exist).
 * Every store is guarded by the capacities and every index and key is range-tested again: triangles that changed between the two calls,
 * or a capacity that is too small, truncate or misplace the output (a corner that no longer has a used cell is emitted as -1) and never
 * write out of bounds; a capacity below the count stores the prefix of the full result.  workspace: 16-byte aligned.
 * Both entries return SN_OK without touching a pointer when V == 0, the emit also with both capacities 0 and no cluster map.  triangles
 * may be NULL when T == 0.  Errors before any launch: SN_ERR_INVALID (NULL pointer, misaligned workspace, a cell that is not positive and
 * finite, a non-finite origin, a zero dim), SN_ERR_UNSUPPORTED (V, T or cells >= 2^31), SN_ERR_WORKSPACE.
 * Nothing is placed by an atomic -- atomics compute minima, sets and integer sums only -- so the output is identical from run to run.
 * Not promised: manifoldness (clustering can pinch a thin wall into edges shared by more than two triangles), and nothing here weighs the
 * error it makes: this is not quadric-error decimation. */
size_t sn_rm_mesh_simplify_workspace_bytes(uint32_t V, uint32_t T, uint32_t cells);
int sn_rm_mesh_simplify_count(const float *vertices, const float *normals, const int32_t *triangles, uint32_t V, uint32_t T,
                              const float *origin, const float *cell, const uint32_t *dims, void *workspace, size_t workspace_bytes,
                              uint32_t *counts, sn_stream_t stream);
int sn_rm_mesh_simplify_emit(const float *vertices, const float *normals, const int32_t *triangles, uint32_t V, uint32_t T,
                             const float *origin, const float *cell, const uint32_t *dims, const void *workspace, size_t workspace_bytes,
                             float *out_vertices, float *out_normals, int32_t *out_triangles, int32_t *vertex_cluster, uint32_t cap_v,
                             uint32_t cap_t, sn_stream_t stream);

/* Mesh smoothing and geometric normals (raymarching.mesh_smooth, mesh_vertex_normals, NeRFRenderer.extract_mesh(smooth)): Taubin or plain
 * Laplacian smoothing of an indexed triangle mesh with the uniform umbrella, carried out on integers (csrc/mesh_smooth.hip), and the
 * area-weighted vertex normals of the result.  The definition is this project's; tests/mesh_smooth_ref.py restates it operation for
 * operation in numpy.  Every sum that crosses lanes is a sum of integers, and everything else is the correctly rounded result of the
 * stated operations, so the device's output EQUALS the restatement's: vertices and normals bit for bit, flags exactly.
 *
 * Input: vertices [V,3] fp32, triangles [T,3] int32 -- any indexed mesh -- origin[3] (fp32, finite; a HOST array) and ONE quantum (fp32,
 * > 0 and finite): the integer space is isotropic.
 *   Quantisation      per axis u = p - origin and s = u / quantum in fp32 (IEEE division; two roundings, no contraction), r = rintf(s).  A
 *                     vertex is PLACED iff all three r are finite and 0 <= r < 4194304 (2^22); Q0 = (int32)r.  An unplaced vertex never
 *                     moves and contributes to no sum and to no normal.
 *   Valid triangle    all three indices in [0, V) and pairwise distinct (every index is range-tested before it is an address).  Any other
 *                     row contributes nothing anywhere.
 *   Corner pairs      a valid triangle (a, b, c) gives vertex a the pair (next = b, prev = c), b the pair (c, a) and c the pair (a, b).
 *   Open vertex       mix(i) = the splitmix64 finaliser of (uint64)i + 1: x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) 0xBF58476D1CE4E5B9;
 *                     x = (x ^ x >> 27) 0x94D049BB133111EB; x ^= x >> 31.  v is OPEN iff sum mix(next) != sum mix(prev) modulo 2^64 over
 *                     its pairs.  mix is a bijection: on a consistently oriented mesh whose edges carry at most two triangles, a vertex
 *                     with one triangle fan is open exactly when it lies on an edge that one triangle uses (no collision is possible
 *                     there).  A vertex where the orientation is inconsistent is open too -- the safe side, open vertices being pinned.
 *   Half-step, f      (f fp32, promoted to fp64.)  S (int64 per axis) = the sum of Q over the placed next and the placed prev of v's pairs,
 *                     n = the number of those terms: in a closed manifold every neighbour counts twice, which is the uniform umbrella.
 *                     v is FREE iff it is placed, n > 0, and it is not both open and pinned (pin_open).  A free vertex gets, per axis,
 *                         d = (double)S / (double)n - (double)Q;  r = rint((double)f d), ties to even;  Q' = clamp(Q + (int64)r, 0, 2^22 - 1)
 *                     every operation rounded on its own; any other vertex keeps Q.  All vertices update at once (Jacobi): a half-step
 *                     reads one buffer and writes the other.
 *   Iteration         a half-step with lambda, then one with mu; mu == 0 skips the second (plain Laplacian smoothing).  Accepted:
 *                     0 < lambda <= 1, and mu == 0 or -1 <= mu < -lambda.  iterations = 0 moves nothing.
 *   Output vertices   a vertex whose final Q equals Q0 -- unplaced, pinned, isolated, converged, zero iterations -- keeps its input BITS
 *                     (the emit requantises `vertices` to decide; no copy of Q0 is kept).  Every other vertex gets, per axis,
 *                     fp32((double)origin + (double)quantum (double)Q): product and sum rounded once each in fp64, then once to fp32.
 *   Geometric normals (optional.)  S = the int64 sum, over v's pairs with all three corners placed, of (Q_next - Q_v) x (Q_prev - Q_v) on
 *                     the FINAL integers: each component is a difference of two products below 2^44, so exact; area-weighted; the same
 *                     vector from whichever corner of a triangle it is computed.  The sum wraps modulo 2^64 (no vertex of valence below
 *                     2^18 gets there).  The normal is S / sqrt((Sx Sx + Sy Sy) + Sz Sz) in fp64 ((double)S is the conversion's one
 *                     rounding), no contraction, rounded once to fp32; (0,0,0) when S is zero -- mesh_simplify's formula.  With the
 *                     isosurface's orientation these point outward, like its -g/|g|.
 *   Flags             vertex_flags [V] uint8 (optional): bit 0 placed, bit 1 open, bit 2 moved (placed and Q != Q0).
 * No output depends on the order of accumulation, the launch shape, the order of the vertices or the run.
 *
 * sn_rm_mesh_smooth_workspace_bytes(V, T):
 *     16 + 32V + up(8V) + 2 up(4V) + up(8 ceil(V / 1024)) + up(24T)                                        (up = rounded up to 16)
 * i.e. 48 bytes per vertex (two [V,4] int32 buffers of Q and flags, a 64-bit row start, a degree and a cursor) and 24 per triangle (three
 * int2 pairs).  0 (with a message) if V or T >= 2^31.
 * sn_rm_mesh_smooth_build: counts the pairs of every vertex (integer atomic adds), ranks them by segments of 1024 vertices and scans the
 * segment totals with one workgroup (64 bits: 3T passes 2^32), fills every vertex's row of int2 (next, prev) -- the slot inside a row comes
 * from an integer atomic cursor, an order no output can see because every consumer of a row is an integer sum -- then quantises and
 * derives the open flags: five launches behind one memset.  n is not stored: the half-step counts the placed neighbours it gathers.
 * sn_rm_mesh_smooth_steps: `iterations` iterations on the integers in the workspace, ONE launch per half-step, one lane per vertex (a row
 * of more than 128 pairs is summed by its owner's whole wave): the row, Q[next] and Q[prev] gathered from one buffer, Q' stored to the
 * other; plain loads and stores, no atomics.  The workspace remembers which buffer is current, so calls compose: 3 then 2 iterations equal
 * 5, for either kind of iteration.
 * sn_rm_mesh_smooth_emit: out_vertices [V,3], out_normals [V,3] or NULL, vertex_flags [V] or NULL, from the workspace and `vertices`; the
 * normals by the same gather over the rows.  It changes nothing in the workspace: steps may follow it.
 * All three: SN_OK without touching a pointer when V == 0; triangles may be NULL when T == 0; workspace 16-byte aligned; V, T, origin and
 * quantum must be the build's.  Errors before any launch: SN_ERR_INVALID (NULL pointer, misaligned workspace, a quantum that is not
 * positive and finite, a non-finite origin, lambda or mu outside the ranges above), SN_ERR_UNSUPPORTED (V or T >= 2^31), SN_ERR_WORKSPACE.
 * Every index read from a row is range-tested again and a row is read only inside the workspace's 3T pairs: a workspace that no build
 * filled gives meaningless integers, never an access out of bounds.
 * Not here: cotangent or other geometry-dependent weights (not exact in integers), feature-preserving smoothing. */
size_t sn_rm_mesh_smooth_workspace_bytes(uint32_t V, uint32_t T);
int sn_rm_mesh_smooth_build(const float *vertices, const int32_t *triangles, uint32_t V, uint32_t T, const float *origin, float quantum,
                            void *workspace, size_t workspace_bytes, sn_stream_t stream);
int sn_rm_mesh_smooth_steps(uint32_t V, uint32_t T, uint32_t iterations, float lambda, float mu, int pin_open, void *workspace,
                            size_t workspace_bytes, sn_stream_t stream);
int sn_rm_mesh_smooth_emit(const float *vertices, uint32_t V, uint32_t T, const float *origin, float quantum, const void *workspace,
                           size_t workspace_bytes, float *out_vertices, float *out_normals, uint8_t *vertex_flags, sn_stream_t stream);

/* Mesh rasteriser (raymarching.mesh_rasterize, NeRFRenderer.render_mesh): an indexed triangle mesh seen from one pinhole camera through a
 * depth buffer (csrc/mesh_raster.hip) -- per pixel the triangle, its depth, the coverage and the interpolated vertex attributes.  The
 * definition is this project's; tests/mesh_raster_ref.py restates it operation for operation in numpy.  Everything that decides a pixel is an
 * integer or the correctly rounded result of the stated operations, and the depth test is a maximum, so the device's output EQUALS the
 * restatement's bit for bit, whatever the order of the triangles, the launch shape or the run.
 *
 * Input: vertices [V,3] fp32, triangles [T,3] int32 -- any indexed mesh, the tensors extract_mesh returns -- pose [4,4] fp32 (row-major
 * cam2world: R = its upper-left 3x3 block, o = its last column) and intrinsics [4] fp32 = {fx, fy, cx, cy}, both ON THE DEVICE (read when
 * the kernels run: a captured graph replays with a new camera), in the convention of sn_rm_generate_rays: the camera looks along -z of its
 * frame, x to the right, y up; the centre of pixel (i, j) -- column i, row j -- is at (i + 0.5, j + 0.5).  An image of H rows, W columns.
 *   Camera            d = v - o per axis; c_j = (R[0][j] d_0 + R[1][j] d_1) + R[2][j] d_2 for j = 0, 1, 2 (c = R^T d): fp32, every product and
 *                     sum rounded on its own.  z = -c_2: the depth, which is the field render's `depth` for the unnormalised ray directions
 *                     of sn_rm_generate_rays.  r = 1 / z.  x = (fx c_0) / z + cx and y = -((fy c_1) / z) + cy, with the IEEE division.
 *   Placed vertex     iff its three coordinates are finite, z >= near (near > 0), r is finite (it is unless z is below 2^-128), and the
 *                     snapped coordinates X = rint(256 x), Y = rint(256 y) (ties to even; 256 x is exact) lie in [-2^22, 2^22] -- the guard
 *                     band, 2^14 pixels either side of the pixel grid's origin.  No NaN passes.  X, Y are int32 with 8 sub-pixel bits.
 *   Drawn triangle    iff its three indices are in [0, V) (each is range-tested before it is an address), its three vertices are placed, its
 *                     doubled signed area A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) (int64) is not 0 and, with `cull`, A < 0.  On the
 *                     sign: a triangle that is counter-clockwise seen from outside -- sn_rm_isosurface_emit's promise -- is counter-clockwise
 *                     in the camera's (c_0, c_1) plane when its outside faces the camera; the screen's y points down, which turns it
 *                     around: FRONT faces have A < 0.  Without clip (sn_rm_mesh_raster_draw / _resolve) there is no clipping: a triangle
 *                     with a corner that is not placed is dropped whole.  counts [4] int32 = triangles {drawn, dropped for a bad index or an unplaced corner,
 *                     degenerate (A = 0), culled}, tested in that order; they sum to T.
 *   Coverage          one sample per pixel at its centre P = (256 i + 128, 256 j + 128).  With s = sign(A): edge k runs from corner k + 1 to
 *                     corner k + 2 (mod 3), (dx, dy) = s (that edge's vector), w_k = dx (P_y - Y_{k+1}) - dy (P_x - X_{k+1}): int64, exact
 *                     (every product is below 2^47), w_0 + w_1 + w_2 = |A|, and w_k > 0 inside.  A pixel is covered iff for every k
 *                     w_k > 0, or w_k == 0 and edge k is a top edge (dy == 0, dx > 0) or a left edge (dy < 0): the top-left rule, under
 *                     which two triangles that share an edge cover every pixel on it exactly once, whatever their order or orientation.
 *   Depth key         rho = (((double)w_0 r_0 + (double)w_1 r_1) + (double)w_2 r_2) / (double)|A| in fp64, every operation rounded on its own:
 *                     the inverse depth, linear on the screen.  The pixel keeps the triangle with the LARGEST fp32(rho) (positive: its bits
 *                     order as unsigned integers), on equal bits the LOWEST index t: the maximum of (bits(fp32 rho) << 32) | (0xFFFFFFFF - t)
 *                     as one 64-bit unsigned integer, 0 = empty.  (The device's fp64 quotient is the correctly rounded one: the
 *                     device equals numpy here.)
 *   Resolve           per pixel with winner t, rho recomputed: triangle_id = t, depth = fp32(1.0 / rho) (fp64 division), mask = 1; empty:
 *                     -1, 0, 0.  Perspective-correct weights mu_k = p_k / ((p_0 + p_1) + p_2) with p_k = (double)w_k r_k.
 *                     colors [V,3] fp32 -> image [H,W,3] = fp32((mu_0 a_0 + mu_1 a_1) + mu_2 a_2) per channel in fp64, a_k the attribute
 *                     of corner k; bg_color where empty.  normals [V,3] -> normal [H,W,3]: the same sum, NOT renormalised; 0 where empty.
 *                     labels [V] uint8 -> label [H,W] uint8: the label of the corner with the largest mu, the first corner of the row
 *                     winning ties; 255 where empty.
 *
 *
 * Near-plane clipping (sn_rm_mesh_raster_draw_clip / _resolve_clip, opt-in; tests/mesh_raster_clip_ref.py restates it).  The rows, the
 * projection and the workspace are the ones above; a clipped triangle recomputes the fp32 camera frame c, z of its corners from vertices
 * and pose with the Camera line's expressions in its order.
 *   Corner roles      FRONT: its row is placed.  BEHIND: not placed, its three coordinates finite and z < near (z <= 0 included).  Any other
 *                     corner that is not placed (NaN, guard band, overflowed 1 / z) is BAD.
 *   Triangle classes  three front corners: the triangle above, bit for bit.  A bad index, a bad corner or no front corner: dropped, as
 *                     above.  Otherwise it has one or two behind corners and is CLIPPED.
 *   Crossing point    of an edge between a front corner P and a behind corner Q -- the roles come from the vertices, not from the order in
 *                     the triangle, so two triangles that share the edge compute the same bits.  In fp64 from the fp32 values, every
 *                     operation rounded on its own: s = (z_P - near) / (z_P - z_Q); x = c_P.x + s (c_Q.x - c_P.x), y likewise;
 *                     px = (fx x) / near + cx, py = -((fy y) / near) + cy; X = rint(256 px), Y = rint(256 py) (ties to even);
 *                     r = 1.0f / near in fp32.  Unless |X| <= 2^22 and |Y| <= 2^22 (no NaN passes) the whole triangle is dropped:
 *                     only the near plane clips, the guard band does not.
 *   Polygon           walk the corners k = 0, 1, 2: emit corner k if it is front, then the crossing point of the edge (k, k + 1 mod 3) if
 *                     exactly one of its ends is front.  Three or four points p0 .. in the triangle's winding; the PIECES are
 *                     (p0, p1, p2) and, of four points, (p0, p2, p3).
 *   Pieces            each is set up as a Drawn triangle is from its three {X, Y, r}: A, the edge functions, the top-left rule, rho from
 *                     the piece's three r.  A piece with A = 0 is skipped, one with A > 0 is skipped under `cull`.  Every piece writes the
 *                     Depth key of its PARENT's t with the same 64-bit maximum: the image stays independent of the order of the triangles
 *                     and of the run.  counts: the parent counts once -- drawn if a piece is drawn, else culled if a piece was culled, else
 *                     degenerate.  clip_counts [2] int32 = {clipped triangles (their crossing points inside the guard band), the pieces of
 *                     them that were drawn}.
 *   Resolve           of a winner whose corners are not all front: its pieces are rebuilt (every piece with A != 0; cull plays no part).
 *                     The piece that covers the pixel centre is taken; if both do -- only in a sliver that the snapping made non-convex --
 *                     the one with the larger fp32(rho) bits, then the first.  p_k, their sum, rho and mu_k are that piece's, as above;
 *                     depth = fp32(1.0 / rho).  The attributes go through the parent's corners: lambda_i = ((0.0 + mu_0 B[0][i]) +
 *                     mu_1 B[1][i]) + mu_2 B[2][i], where the row B[k] of the piece's point k is the unit vector of a front corner, or
 *                     1.0 - s at P, s at Q and 0 at the third corner for a crossing point.  colors and normals: the Resolve line's sum of
 *                     the parent's three rows with lambda for mu; label: the parent's corner with the largest lambda, the first winning
 *                     ties.  A winner with three front corners is resolved as above.
 *
 * sn_rm_mesh_raster_workspace_bytes(V, T, H, W):
 *     16 + 16V + 8HW + up(4T)                                                                                (up = rounded up to 16)
 * i.e. a head (the queue's length), a 16-byte row {X, Y, bits(r), placed} per vertex, the 64-bit depth buffer, and a queue of triangle
 * indices.  0 (with a message) unless V, T < 2^31 and H, W are in [1, 8192].
 * sn_rm_mesh_raster_project: one lane per vertex writes its row; the same launch clears the depth buffer, the queue's length and counts.
 * sn_rm_mesh_raster_draw: two launches.  One lane per triangle classifies it and adds to counts (one atomic add per wave and counter);
 * a triangle whose bounding box, clipped to the screen, holds at most small_max_pixels (< 2^31) pixel centres is scanned by its lane; the
 * others are appended to the queue (ballot + mbcnt rank, one atomic add per wave).  Then a fixed grid of waves strides over the queue,
 * whose length is read on the device: the 64 lanes of a wave share one triangle and walk its clipped bounding box in row segments.  The
 * depth test is the plain 64-bit atomic maximum (global_atomic_umax_x2, no compare-and-swap loop).  small_max_pixels moves triangles
 * between the two kernels and changes the time only: 0 (all through the queue) and 2^31 - 1 (none) give the same bits.
 * sn_rm_mesh_raster_resolve: one lane per pixel; triangle_id [H,W] int32, depth [H,W] fp32, mask [H,W] uint8 always; colors with image,
 * normals with normal, labels with label, each pair both given or both NULL (with V == 0 the attribute may be NULL beside its image).  It
 * changes nothing in the workspace.
 * sn_rm_mesh_raster_draw_clip, sn_rm_mesh_raster_resolve_clip: the clipped instantiations of the same three kernels, after the same
 * sn_rm_mesh_raster_project and in the same workspace; vertices, pose, intrinsics and near_plane must be the project's, and pose and
 * intrinsics are again read on the device.  draw_clip clears clip_counts on the stream (an 8-byte memset node in a captured graph); a lane
 * of the first kernel scans its own pieces one after the other; a clipped triangle is queued ONCE if either piece's box exceeds
 * small_max_pixels, and the wave that takes it walks both pieces.  The same checks and refusals as their siblings, and near_plane positive
 * and finite.  The unclipped entries launch the unclipped instantiations, which read none of this.  A draw and its resolve go together:
 * both clipped or neither.
 * All three: vertices may be NULL when V == 0 and triangles when T == 0 -- the project still clears and the resolve still writes the empty
 * image; workspace 16-byte aligned; V, T, H, W must be the project's.  Errors before any launch: SN_ERR_INVALID (NULL pointer, misaligned
 * workspace, a near that is not positive and finite, small_max_pixels >= 2^31, an attribute without its image or the reverse),
 * SN_ERR_UNSUPPORTED (V or T >= 2^31, H or W outside [1, 8192]), SN_ERR_WORKSPACE.  Every index read from `triangles`, from the queue or
 * from the depth buffer is range-tested before it is an address: a workspace that no project filled gives a meaningless image, never an
 * access out of bounds.
 * Not here: guard-band or screen clipping (a triangle with a corner or a crossing point outside the guard band disappears, clipped or
 * not), anti-aliasing, transparency, textures, gradients. */
size_t sn_rm_mesh_raster_workspace_bytes(uint32_t V, uint32_t T, uint32_t H, uint32_t W);
int sn_rm_mesh_raster_project(const float *vertices, uint32_t V, uint32_t T, const float *pose, const float *intrinsics, uint32_t H, uint32_t W,
                              float near_plane, void *workspace, size_t workspace_bytes, int32_t *counts, sn_stream_t stream);
int sn_rm_mesh_raster_draw(const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, int cull, uint32_t small_max_pixels,
                           void *workspace, size_t workspace_bytes, int32_t *counts, sn_stream_t stream);
int sn_rm_mesh_raster_resolve(const int32_t *triangles, uint32_t V, uint32_t T, uint32_t H, uint32_t W, const float *colors,
                              const float *normals, const uint8_t *labels, float bg_color, const void *workspace, size_t workspace_bytes,
                              int32_t *triangle_id, float *depth, uint8_t *mask, float *image, float *normal, uint8_t *label,
                              sn_stream_t stream);
int sn_rm_mesh_raster_draw_clip(const float *vertices, const int32_t *triangles, uint32_t V, uint32_t T, const float *pose, const float *intrinsics,
                                uint32_t H, uint32_t W, float near_plane, int cull, uint32_t small_max_pixels, void *workspace,
                                size_t workspace_bytes, int32_t *counts, int32_t *clip_counts, sn_stream_t stream);
int sn_rm_mesh_raster_resolve_clip(const float *vertices, const int32_t *triangles, uint32_t V, uint32_t T, const float *pose,
                                   const float *intrinsics, uint32_t H, uint32_t W, float near_plane, const float *colors, const float *normals,
                                   const uint8_t *labels, float bg_color, const void *workspace, size_t workspace_bytes, int32_t *triangle_id,
                                   float *depth, uint8_t *mask, float *image, float *normal, uint8_t *label, sn_stream_t stream);

/* Training-time forward of a bias-free perceptron with 256-wide hidden layers and no skip connections (nerf/network.py:31-66: F.linear +
 * activation per layer; the per-sample mask head in training, network.py:118-123, trainer.py:401-428) in ONE kernel, true fp32 products
 * and accumulation on the matrix cores (v_mfma_f32_32x32x2_f32; results differ from a BLAS GEMM only by summation order).
 * x [N, dims[0]] (dims[0] <= 256) -> out [N, dims[nl]] (<= 256, linear); hidden[l] [N, 256] for l < nl-1 receives the POST-activation output
 * of layer l -- what torch's in-place activation leaves for autograd, and what sn_mlp_wide_backward / sn_linear_wgrad read.
 * hidden is a host array of nl-1 device pointers.  All tensors row-major fp32, no alignment requirement beyond 4 bytes. */
int sn_mlp_wide_forward_train(const sn_mlp_desc *mlp, const float *x, uint32_t N, float *const *hidden, float *out, sn_stream_t stream);

/* The same forward on the inference kernel of sn_mlp_wide_forward (split-fp16 x3 products with fp32 accumulation on the matrix cores, ~2^-22
 * per product; any dims[0] <= 1024, biases allowed) with every hidden layer's post-activation output saved: hidden[l] [N, 256], 16-byte
 * aligned.  workspace: sn_mlp_wide_workspace_bytes(mlp), 16-byte aligned.  Activations must stay inside the fp16 range (sn_mlp_wide_overflow). */
int sn_mlp_wide_forward_train_f16x3(const sn_mlp_desc *mlp, const float *x, uint32_t N, float *const *hidden, uint32_t *const *sign_bits,
                                    float *out, void *workspace, size_t workspace_bytes, sn_stream_t stream);
/* sign_bits (NULL, or a host array of nl-1 device pointers, entries may be NULL): sign_bits[l] [N, 8] uint32, 16-byte aligned, receives one
 * bit per hidden unit of layer l (set = output > 0) in the kernels' register order -- an opaque companion of hidden[l] for
 * sn_mlp_wide_backward_bits, which then reads 32 bytes per row and layer instead of 1 KiB. */

/* Backward-data pass of a 256-wide perceptron without skip layers (the autograd of nerf/network.py:31-66 for the per-sample
 * mask head in training, trainer.py:401-428) in one kernel: grad_out [N, dims[nl]] -> grad_in [N, dims[0]], and for every
 * hidden layer l < nl-1 grad_hidden[l] [N, 256] = d loss / d (pre-activation of layer l) -- what sn_linear_wgrad needs.
 * hidden[l] [N, 256] = the forward's saved (post-activation) output of layer l: its sign selects the LeakyReLU / ReLU branch
 * exactly as torch's in-place backward does.  Products as split-fp16 with fp32 accumulation on the matrix cores; every row is
 * scaled by a power of two (exact) so that small gradient rows keep their precision.  hidden / grad_hidden are host arrays of
 * nl-1 device pointers. */
size_t sn_mlp_wide_backward_workspace_bytes(const sn_mlp_desc *mlp);
int sn_mlp_wide_backward_bits(const sn_mlp_desc *mlp, const float *grad_out, const uint32_t *const *sign_bits, uint32_t N,
                              float *grad_in, float *const *grad_hidden, void *workspace, size_t workspace_bytes, sn_stream_t stream);
int sn_mlp_wide_backward(const sn_mlp_desc *mlp, const float *grad_out, const float *const *hidden, uint32_t N,
                         float *grad_in, float *const *grad_hidden, void *workspace, size_t workspace_bytes, sn_stream_t stream);

/* The reference's SMALL bias-free ReLU perceptrons under training (nerf/network.py:9-29 `MLP` as instantiated at network.py:94, 98, 143:
 * grid_mlp 32-64-64-16, view_mlp 31-32-32-3, prop_mlp 10-16-1; also BASELINE configs[0]'s 16-32-16 / 31-32-3), one kernel per direction on
 * the matrix cores in true fp32 (v_mfma_f32_32x32x2_f32: exact products, fixed summation order), replacing F.linear + F.relu per layer.
 *   forward:  out [N, dL] = raw output; hidden[l] [N, d_{l+1}] = post-ReLU output of layer l (l < L-1), 16-byte aligned.
 *             act: SN_SMALL_ACT_TRUNC_EXP0  aux_out [N]     = exp(out[:, 0])                      (trunc_exp, activation.py:5-11, network.py:155,179)
 *                  SN_SMALL_ACT_SIGMOID_BG  aux_out [N, dL] = sigmoid(out) + (1 - aux_in[n]) * bg  (renderer.py:349-353; aux_in = weights_sum, dL <= 4)
 *   backward: the whole data path.  grad_out [N, dL] (gradient of `out`, may be NULL) and grad_aux (gradient of aux_out, may be NULL; the
 *             activation's derivative is applied here: trunc_exp's exp(clamp(x, -15, 15)), activation.py:13-17) are combined into
 *             grad_last [N, dL] (gradient of the last pre-activation), then grad_hidden[l] [N, d_{l+1}] = gradient of layer l's pre-activation
 *             (ReLU branch from the sign of hidden[l], as torch's in-place backward) and grad_in [N, d0] (NULL: not wanted).
 *             grad_aux_in [N] (act SIGMOID_BG, may be NULL) = gradient of aux_in.  Weight gradients: sn_linear_wgrad on
 *             (x, grad_hidden[0]), (hidden[l-1], grad_hidden[l]), (hidden[L-2], grad_last).
 * sn_mlp_small_supported: 1 if this build instantiates the descriptor's widths (others: SN_ERR_UNSUPPORTED, the caller keeps its own layers). */
enum { SN_SMALL_ACT_NONE = 0, SN_SMALL_ACT_TRUNC_EXP0 = 1, SN_SMALL_ACT_SIGMOID_BG = 2 };
int sn_mlp_small_supported(const sn_mlp_desc *mlp);
int sn_mlp_small_forward_train(const sn_mlp_desc *mlp, const float *x, uint32_t N, float *const *hidden, float *out, int32_t act,
                               const float *aux_in, float bg, float *aux_out, sn_stream_t stream);
int sn_mlp_small_backward(const sn_mlp_desc *mlp, const float *grad_out, const float *grad_aux, int32_t act, const float *out_raw, float bg,
                          const float *const *hidden, uint32_t N, float *grad_in, float *const *grad_hidden, float *grad_last, float *grad_aux_in,
                          sn_stream_t stream);

/* General fp32 matrix product on the matrix cores in true fp32 (v_mfma_f32_32x32x2_f32: exact products, one k-ascending chain per output element,
 * deterministic) -- the route of every layer shape the specialised kernels do not instantiate; replaces torch.nn.functional.linear / `@`
 * (nerf/network.py:9-66 with widths other than the reference's):
 *   c[i * c_row + j] = act(sum_k a[i * a_row + k * a_col] * b[k * b_row + j * b_col] + bias[j]),  i < M, j < N, k < K
 * One stride of a and one of b must be 1.  nn.Linear forward: a = x (K, 1), b = weight [N,K] (1, K), bias or NULL; input gradient: a = dy (N, 1),
 * b = weight (K, 1) with K and N swapped; weight gradient: a = dy (1, N) transposed, b = x (K, 1).  act: 0 none, 1 ReLU, 2 leaky ReLU (0.01). */
int sn_gemm_f32(const float *a, int64_t a_row, int64_t a_col, const float *b, int64_t b_row, int64_t b_col, const float *bias, int32_t act,
                uint32_t M, uint32_t N, uint32_t K, float *c, int64_t c_row, sn_stream_t stream);

/* Weight gradient of an nn.Linear over a training batch: dw[N,K] = dy[M,N]^T x[M,K], fp32, summed in a fixed order
 * (deterministic).  K, N <= 64 (the radiance / proposal MLPs, nerf/network.py:9-29): register-tiled VALU kernel.
 * Otherwise N <= 256, any K (the per-sample mask head and the SAM head, network.py:31-66): v_mfma_f32_32x32x2_f32 over
 * row slabs, one per CU.  workspace: >= sn_linear_wgrad_workspace_bytes() (0 = shape not supported), holds the
 * per-slab partial results. */
size_t sn_linear_wgrad_workspace_bytes(uint32_t M, uint32_t K, uint32_t N);
int sn_linear_wgrad(const float *x, const float *dy, uint32_t M, uint32_t K, uint32_t N, float *dw,
                    void *workspace, size_t workspace_bytes, sn_stream_t stream);

/* Dense Adam step of one parameter tensor in a single pass: the single-tensor recipe of torch.optim.Adam (the reference's
 * optimiser, main.py:283: Adam(params, eps=1e-15), betas (0.9, 0.999), no amsgrad) -- exp_avg.lerp_(g, 1-beta1);
 * exp_avg_sq = beta2 * exp_avg_sq + (1-beta2) g^2; param -= lr / (1-beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1-beta2^step) + eps)
 * -- with 16-byte accesses, 4 streams read and 3 written.  Same dense semantics (untouched rows keep moving by their
 * momentum); elements whose gradient and both moments are exactly zero are skipped (their update is exactly zero).
 * Hyper-parameters are doubles like the Python floats torch derives its scalars from.  step counts from 1.  step_device != NULL
 * (capturable form, like torch.optim.Adam(capturable=True)): the count is read from that device float when the kernel RUNS and `step` is
 * ignored, so that the launch can be captured in a HIP graph and replayed.
 * flags: SN_ADAM_ZERO_GRAD -- the gradient is cleared in the same pass (for callers that accumulate in place): every element is zero
 *        after the call, those of elements that the step leaves alone included (a raw gradient that maximize / weight decay cancel);
 *        SN_ADAM_LAZY -- opt-in touched-elements-only update (NOT the reference's optimiser): an element whose gradient
 *        is exactly zero in this step is skipped altogether (moments do not decay, the parameter does not move) -- the semantics of
 *        torch.optim.SparseAdam with the non-zeros of the dense gradient as the sparse pattern; requires weight_decay = 0. */
#define SN_ADAM_ZERO_GRAD 1
#define SN_ADAM_LAZY 2
int sn_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, uint64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, uint32_t step, const float *step_device, int maximize, int flags, sn_stream_t stream);

/* The same update for MANY parameter tensors in ONE launch (an optimiser step of the whole model: 13 tensors in RGB mode).  The
 * records travel to the kernel by value in its kernel arguments -- no host-to-device copy, nothing to synchronise, and a captured
 * HIP graph keeps them -- so one call takes at most SN_ADAM_MULTI_MAX_TENSORS tensors in at most SN_ADAM_MULTI_MAX_GROUPS groups
 * (more is an error: split the model into several calls).  Every tensor is cut into chunks of 4096 floats that the workgroups walk
 * in a grid-stride loop; the arithmetic is sn_adam_step's, element for element (bit-identical results).
 * Per tensor: the four streams and the element count (n = 0 is fine), the index of its group, and its OWN step count -- torch keeps
 * one per parameter, and they diverge when a parameter has no gradient in a step: `step` (host, counts from 1), or `step_device`
 * != NULL (a device float, read when the kernel RUNS; `step` is ignored).  Each device count belongs to one tensor of the call.
 * Per group: the hyper-parameters as doubles, maximize, flags (SN_ADAM_ZERO_GRAD, SN_ADAM_LAZY as above).
 * lr_scale_device != NULL: every group's rate is lr x (double)*lr_scale_device, read when the kernel runs (a learning-rate schedule
 * that a captured graph follows); the step size is formed from it in double.
 * ticket != NULL: the kernel ALSO advances the device step counts: a tensor with a device count is updated with count + 1, and the
 * workgroup that finishes last stores the new counts.  `ticket` is a device word, zero before its first use and left zero by every
 * call; nobody spins or waits on it.  ticket == NULL: the caller has advanced the counts beforehand, as for sn_adam_step.
 * All arguments are checked on the host before anything touches the device. */
#define SN_ADAM_MULTI_MAX_TENSORS 32
#define SN_ADAM_MULTI_MAX_GROUPS 8
typedef struct sn_adam_tensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    uint64_t n;
    float *step_device;       /* NULL: `step` holds the count */
    uint32_t step;
    uint32_t group;           /* index into the call's groups */
} sn_adam_tensor;
typedef struct sn_adam_group {
    double lr, beta1, beta2, eps, weight_decay;
    int32_t maximize;
    int32_t flags;
} sn_adam_group;
int sn_adam_step_multi(const sn_adam_tensor *tensors, uint32_t n_tensors, const sn_adam_group *groups, uint32_t n_groups,
                       const float *lr_scale_device, uint32_t *ticket, sn_stream_t stream);

/* Exponential moving average of MANY parameter tensors in ONE launch: the update of torch_ema.ExponentialMovingAverage, which the
 * reference's trainer runs after every optimiser step (main.py:302 ema_decay=0.95; nerf/trainer.py:1231-1232).  Per element, exactly
 *     shadow = shadow - (shadow - param) * omd
 * in three separately rounded fp32 operations (tmp = s - p; tmp.mul_(omd); s.sub_(tmp)); `param` is only read.  The results have the
 * bit patterns of that statement as torch evaluates it on an x86 host, denormals kept; a NaN result is encoded as the host encodes it
 * (the first NaN operand, quieted; 0xffc00000 where inf - inf or inf * 0 produced it), which IEEE 754 leaves open.  The records travel
 * in the kernel arguments like sn_adam_step_multi's, at most SN_EMA_MULTI_MAX_TENSORS per call (more is an error: several calls on
 * one stream); every tensor is cut into chunks of 4096 floats that the workgroups walk in a grid-stride loop; n = 0 is fine.
 * num_updates_device == NULL: omd = (float)(1.0 - decay), formed on the host.
 * num_updates_device != NULL: torch_ema's warm-up, with the count on the device.  The kernel reads n = *num_updates_device + 1 when
 *     it RUNS and forms d = min(decay, (1.0 + n) / (10.0 + n)), omd = (float)(1.0 - d) in double -- the operations Python performs
 *     on the host, hence the same bits -- so that a launch captured in a HIP graph follows the warm-up when it is replayed.
 * flags & SN_EMA_ADVANCE: the call ALSO advances the count.  The workgroup that finishes last stores n; `ticket` is a device word,
 *     zero before its first use and left zero by every call; nobody spins or waits on it.  A model of more than
 *     SN_EMA_MULTI_MAX_TENSORS tensors is several calls that all read count + 1; only the last one carries SN_EMA_ADVANCE.  A call
 *     with nothing to update but SN_EMA_ADVANCE set still advances the count.
 * decay lies in [0, 1]; shadow and param are 16-byte aligned and distinct; the count is 8-byte, the ticket 4-byte aligned.
 * All arguments are checked on the host before anything touches the device. */
#define SN_EMA_MULTI_MAX_TENSORS 32
#define SN_EMA_ADVANCE 1
typedef struct sn_ema_tensor {
    float *shadow;
    const float *param;
    uint64_t n;
} sn_ema_tensor;
int sn_ema_update_multi(const sn_ema_tensor *tensors, uint32_t n_tensors, double decay, uint64_t *num_updates_device,
                        uint32_t *ticket, int flags, sn_stream_t stream);

/* Measurement hook (bench.py): bracket every kernel sn_rm_render_rays launches with hipEvents on the
 * caller's stream.  Classes: 0 weight pack, 1..3 proposal stage k, 4 final stage.  profile_read
 * synchronises, returns summed device milliseconds and launch counts per class, and resets. */
void sn_rm_profile_enable(int on);
int sn_rm_profile_read(float *ms_per_class, int32_t *launches_per_class, int n_classes);
/* Shader clock the last profiled final-stage launch ran at, MHz: workgroup 0 reads s_memtime (shader cycles) and
 * s_memrealtime (constant wall-clock rate) at entry and exit; shader_mhz = their ratio x the wall-clock rate.  probe_ms
 * (optional) = the wall time the probe spanned.  0 when no final stage ran since sn_rm_profile_enable(1).  Synchronises. */
int sn_rm_profile_shader_clock(float *shader_mhz, float *probe_ms);
/* Test hook: the library's device numerics primitives element-wise, y[i] = f(a[i][, b[i]]).  op 0: exp (the shared
 * deterministic recipe, oracle orc_expf); 1: a / b as compiled (IEEE-rounded); 2 / 3: the Mip-360 spacing function and its
 * inverse (renderer.py:249-252). */
int sn_debug_eval(int op, const float *a, const float *b, uint32_t n, float *y, sn_stream_t stream);
/* Diagnostics: occupancy-API workgroups/CU of the fused kernels (prop, final f16x3, final f32-MFMA) and their dynamic LDS bytes. */
int sn_rm_debug_occupancy(int32_t *out, int32_t *lds, int n);

#ifdef __cplusplus
}
#endif
#endif /* SANERF_HIP_H */
