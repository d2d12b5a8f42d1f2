"""The layout of the `raymarching` package (no device needed): one module per operator family behind an unchanged package surface, one
`tuning` object, constants that stay patchable on the package, and a buffer module that `ops` shares without importing `raymarching`."""
import importlib
import os
import subprocess
import sys

import pytest

from sanerf_hq_amd import ops, raymarching as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPORTS = """jitter_tables DeviceJitter
composite contract distort_loss generate_rays rays_from_pixels grid_composite mask_head mask_head_fusable mask_nll ray_pair_select
ray_pair_rgb_loss mask_error error_map_update mask_output mask_eval_accumulate image_sqerr_accumulate image_ssim_accumulate ssim_record
ssim_workspace read_ssim_record feature_distill_loss feature_map rgb_loss points_lift point_store point_store_update points_project
prompt_overlay reference_resize_ratio weighted_draw collate_gather COLLATE_OUTPUTS eval_record eval_workspace read_eval_record mlp_forward
near_far_from_aabb proposal_loss_stage render_rays sample_pdf sample_positions weights_from_sigma jitter ray_composite proposal_loss_all
zeros_f32
RenderPlan Tuning tuning last_launch_info route_info tile_order_info PROPOSAL_LOSS_MAX_T WEIGHTS_BACKWARD_MAX_T DISTORT_LOSS_MAX_T
FP16_SPLIT_LIMIT mlp_wide_overflow _host_values""".split()


def _module(name):
    return importlib.import_module("sanerf_hq_amd.raymarching." + name)


def test_package_exports():
    assert len(EXPORTS) == len(set(EXPORTS)) == 60
    assert [n for n in EXPORTS if not hasattr(rm, n)] == []
    assert [n for n in EXPORTS if n.lstrip("_")[0].islower() and n != "tuning" and not callable(getattr(rm, n))] == []


def test_one_tuning_object():
    render = _module("render")
    assert rm.tuning is render.tuning and isinstance(rm.tuning, rm.Tuning)
    assert rm.render_rays.__globals__ is vars(render) and rm.RenderPlan.workspace.__globals__ is vars(render)


@pytest.mark.parametrize("name", ["WEIGHTS_BACKWARD_MAX_T", "PROPOSAL_LOSS_MAX_T", "DISTORT_LOSS_MAX_T"])
def test_constants_on_the_package(name):
    march = _module("march")
    assert getattr(rm, name) == getattr(march, name)
    assert rm.weights_from_sigma.__globals__ is vars(march)         # where a test patches WEIGHTS_BACKWARD_MAX_T


def test_ops_does_not_import_raymarching():
    code = ("import sys; import sanerf_hq_amd.ops; "
            "sys.exit(3 if any(m.startswith('sanerf_hq_amd.raymarching') for m in sys.modules) else 0 if 'sanerf_hq_amd._buffers' in sys.modules else 4)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_monolith_and_duplicate_are_gone():
    package = rm.__name__.rsplit(".", 1)[-1]
    assert not os.path.exists(os.path.join(os.path.dirname(rm.__file__), package + ".py"))       # the module that was named like its package
    assert not hasattr(ops, "_" + rm.zeros_f32.__name__)                                        # ops' private twin of zeros_f32
    assert rm.zeros_f32 is importlib.import_module("sanerf_hq_amd._buffers").zeros_f32
