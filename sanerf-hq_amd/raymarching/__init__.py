"""`raymarching` operators on MI355X, over libsanerf_hip.so.

The reference's README (README.md:32-34) mentions a `raymarching` extension that is not in its tree; the ray-marching maths lives as torch
code in nerf/utils.py and nerf/renderer.py.  This package is that operator surface, one module per native file of csrc/:

    march     generate_rays        nerf/utils.py:182-304 (full image branch)
              near_far_from_aabb   nerf/renderer.py:122-139
              contract             nerf/renderer.py:60-69
              sample_pdf           nerf/renderer.py:84-119   (+ the integer searchsorted result)
              weights_from_sigma   nerf/renderer.py:308-325
              composite            nerf/renderer.py:333-338, 361, 384  (autograd w.r.t. both operands)
    heads     grid_composite       nerf/renderer.py:301-302 + 361: composite(weights, s_grid(xyzs)) fused (inference)
              mlp_forward          nerf/network.py:31-66 (+ LayerNorm :115): the 256-wide head MLPs on the matrix cores (inference)
              mask_point_labels    per-sample argmax of the mask field in the one-kernel mask head (nothing per-sample but the labels written)
    object    object_composite     re-integration of a ray over the samples whose label is kept: the object alone, or the scene without it
    mesh      lattice_points       positions of a window of a world-space lattice (contracted or not), no meshgrid
              isosurface           marching tetrahedra on a density lattice: vertices, normals, triangles (the size is data-dependent)
              mesh_components      connected components of an indexed mesh: labels, triangle and vertex counts per component
              mesh_clean           the mesh without its small components: by triangle count and / or the largest k
              mesh_split           a labelled mesh taken apart: one stand-alone mesh per instance id, seam vertices duplicated
              mesh_simplify        uniform vertex clustering: one vertex per occupied cell of a coarse lattice, exact to the bit
              mesh_smooth          Taubin / Laplacian smoothing in fixed point, with the geometric normals of the result, exact to the bit
              mesh_vertex_normals  the area-weighted vertex normals of a mesh's own triangles
              mesh_rasterize       the mesh seen from one pinhole camera: triangle id, depth, mask and interpolated attributes, exact to the bit
              mesh_rasterize_clip  the same with the near plane cutting the triangles that cross it: a camera inside the mesh
              vertex_probe_points  the K sample positions of a short ray into the surface at every mesh vertex, and its direction
              vertex_probe_composite  the probes' gated re-integration: colour-head input, coverage and instance label per vertex
    render    render_rays         nerf/renderer.py:221-357 + nerf/network.py:146-186, fused
    jitter    jitter               nerf/renderer.py:262-270, 97-102: one stage's perturbed bins / u from caller-supplied uniforms
              jitter_tables        the same tables for every stage in one launch, uniforms from a Philox counter on the device (DeviceJitter)
    mask, meters, distill, rgb_loss, prompts, collate: the mask field's losses and output stage, the device-side meters, the distillation
    loss, the RGB loss tail, point prompts, the batch draw; _args: their tensor-argument helpers (workspaces: .._buffers)."""
from .._buffers import zeros_f32  # noqa: F401
from .march import (  # noqa: F401
    composite, contract, distort_loss, generate_rays, rays_from_pixels, near_far_from_aabb, proposal_loss_stage, proposal_loss_all, sample_pdf,
    sample_positions, weights_from_sigma, ray_composite, PROPOSAL_LOSS_MAX_T, WEIGHTS_BACKWARD_MAX_T, DISTORT_LOSS_MAX_T, _host_values)
from .jitter import jitter, jitter_tables, DeviceJitter  # noqa: F401
from .mask import mask_nll, ray_pair_select, ray_pair_rgb_loss, mask_error, error_map_update, mask_output  # noqa: F401
from .meters import (  # noqa: F401
    mask_eval_accumulate, image_sqerr_accumulate, image_ssim_accumulate, ssim_record, ssim_workspace, read_ssim_record, eval_record,
    eval_workspace, read_eval_record)
from .distill import feature_distill_loss, feature_map  # noqa: F401
from .rgb_loss import rgb_loss  # noqa: F401
from .prompts import points_lift, point_store, point_store_update, points_project, prompt_overlay, reference_resize_ratio  # noqa: F401
from .collate import weighted_draw, collate_gather, COLLATE_OUTPUTS  # noqa: F401
from .heads import (  # noqa: F401
    grid_composite, mlp_forward, mlp_wide_overflow, mask_head, mask_head_fusable, mask_point_labels, mask_point_labels_fusable)
from .object import object_composite, keep_mask_of, LABEL_SKIPPED  # noqa: F401
from .mesh import lattice_points, isosurface, isosurface_counts, isosurface_emit, ISOSURFACE_MAX_VERTICES  # noqa: F401
from .mesh import mesh_components, mesh_clean, mesh_filter_counts, mesh_filter_emit  # noqa: F401
from .mesh import mesh_split, mesh_split_counts, mesh_split_emit, MESH_SPLIT_PARTS  # noqa: F401
from .mesh import mesh_simplify, mesh_simplify_counts, mesh_simplify_emit  # noqa: F401
from .mesh import mesh_smooth, mesh_vertex_normals, mesh_smooth_build, mesh_smooth_steps, mesh_smooth_emit, smooth_quantisation  # noqa: F401
from .mesh import mesh_rasterize, mesh_rasterize_clip, mesh_raster_project, mesh_raster_draw, mesh_raster_resolve, RASTER_SMALL_MAX_PIXELS, RASTER_MAX_SIDE  # noqa: F401
from .mesh import vertex_probe_points, vertex_probe_composite, PROBE_SAMPLES  # noqa: F401
from .render import RenderPlan, Tuning, tuning, last_launch_info, route_info, tile_order_info, tile_queue_info, render_rays, FP16_SPLIT_LIMIT  # noqa: F401
