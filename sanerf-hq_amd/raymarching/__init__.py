from .raymarching import (  # noqa: F401
    composite, contract, distort_loss, generate_rays, rays_from_pixels, grid_composite, mask_head, mask_head_fusable, mask_nll, ray_pair_select, ray_pair_rgb_loss, mask_error, error_map_update, mask_output, mask_eval_accumulate, image_sqerr_accumulate, image_ssim_accumulate, ssim_record, ssim_workspace, read_ssim_record, feature_distill_loss, feature_map, eval_record, eval_workspace, read_eval_record, mlp_forward, near_far_from_aabb, proposal_loss_stage, render_rays, sample_pdf, sample_positions, weights_from_sigma, jitter, ray_composite, proposal_loss_all, zeros_f32,
    RenderPlan, Tuning, tuning, last_launch_info, route_info, PROPOSAL_LOSS_MAX_T, WEIGHTS_BACKWARD_MAX_T, DISTORT_LOSS_MAX_T, FP16_SPLIT_LIMIT, mlp_wide_overflow, _host_values,
)
