"""The `raymarching` operator surface over libsanerf_hip.so (see raymarching.py for the table of operators and their places in
the reference).  Jitter of a perturbed render: `jitter(uniform, ...)` turns caller-supplied uniforms into one stage's table;
`jitter_tables(state, N, steps, ...)` / `DeviceJitter(device, seed)` write the tables of every stage in one capturable launch from a
Philox4x32-10 counter on the device -- (seed, draw, stage, ray, column) name a value, `draw` advances once per image."""
from .raymarching import (  # noqa: F401
    jitter_tables, DeviceJitter,
    composite, contract, distort_loss, generate_rays, rays_from_pixels, grid_composite, mask_head, mask_head_fusable, mask_nll, ray_pair_select, ray_pair_rgb_loss, mask_error, error_map_update, mask_output, mask_eval_accumulate, image_sqerr_accumulate, image_ssim_accumulate, ssim_record, ssim_workspace, read_ssim_record, feature_distill_loss, feature_map, rgb_loss, points_lift, point_store, point_store_update, points_project, prompt_overlay, reference_resize_ratio, weighted_draw, collate_gather, COLLATE_OUTPUTS, eval_record, eval_workspace, read_eval_record, mlp_forward, near_far_from_aabb, proposal_loss_stage, render_rays, sample_pdf, sample_positions, weights_from_sigma, jitter, ray_composite, proposal_loss_all, zeros_f32,
    RenderPlan, Tuning, tuning, last_launch_info, route_info, tile_order_info, PROPOSAL_LOSS_MAX_T, WEIGHTS_BACKWARD_MAX_T, DISTORT_LOSS_MAX_T, FP16_SPLIT_LIMIT, mlp_wide_overflow, _host_values,
)
