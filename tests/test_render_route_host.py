"""CPU: the route of the fused render -- which last-stage kernel runs, with how many workgroups, launches, dense levels and gathers --
through sn_rm_render_route_info, the dry run of sn_rm_render_rays' planner.  The descriptors are built with ctypes from the reference
network's real level offsets and MLP shapes; every pointer is an aligned stand-in (nothing is dereferenced, nothing is launched).
The expected values are those the GPU tests of tests/test_gpu_final_stage.py assert after real launches, and the sizes the kernels'
launch code states: 72 KiB = packed weights (8192 floats) + two 64 x 20-float sample slabs per wave; fp32 matrix cores 64 KiB; the
vector-ALU form 2 x 64 x 256 floats + the padded view weights (2144 floats)."""
import ctypes as C
import re

import numpy as np
import pytest

from sanerf_hq_amd import _lib, ops, synth

PTR = 64                      # an aligned stand-in for every device pointer
LDS_F16X3 = (8192 + 4 * 2 * 64 * 20) * 4
LDS_MFMA32 = (8192 + 4 * 32 * 64) * 4
LDS_VALU = (2 * 64 * 256 + (32 * 32 + 32 * 32 + 3 * 32)) * 4


def _grid(desc, num_levels, level_dim, log2_hashmap_size, desired_resolution, f16):
    scale = np.exp2(np.log2(desired_resolution / 16) / (num_levels - 1))
    offs = ops.grid_level_offsets(3, num_levels, scale, 16, log2_hashmap_size)
    desc.embeddings, desc.table_dtype = PTR, _lib.SN_F16 if f16 else _lib.SN_F32
    for i, o in enumerate(offs):
        desc.offsets[i] = int(o)
    desc.D, desc.C, desc.L, desc.S, desc.H = 3, level_dim, num_levels, float(np.float32(np.log2(scale))), 16
    desc.gridtype, desc.align_corners, desc.interp = 0, 0, 0


def _mlp(desc, dims):
    desc.num_layers, desc.activation, desc.skip_mask = len(dims) - 1, 0, 0
    for i, d in enumerate(dims):
        desc.dims[i] = d
    for l in range(len(dims) - 1):
        desc.weight[l], desc.bias[l] = PTR, None


def make_cfg(steps, f16=False, main_mlp=(32, 64, 64, 16), view_mlp=(31, 32, 32, 3), main_levels=16, with_feat=False, **tuning):
    cfg = _lib.RenderCfg()
    cfg.num_stages = len(steps)
    for k, t in enumerate(steps):
        cfg.num_steps[k] = t
    for k in range(len(steps) - 1):
        g = synth.GRIDS[f"prop_encoders.{k}"]
        _grid(cfg.prop_grid[k], g["num_levels"], g["level_dim"], g["log2_hashmap_size"], g["desired_resolution"], f16)
        _mlp(cfg.prop_mlp[k], (10, 16, 1))
    g = synth.GRIDS["grid"]
    _grid(cfg.grid, main_levels, g["level_dim"], g["log2_hashmap_size"], g["desired_resolution"], f16)
    _mlp(cfg.grid_mlp, main_mlp)
    _mlp(cfg.view_mlp, view_mlp)
    cfg.sh_degree = 4
    for i, v in enumerate([-2.0] * 3 + [2.0] * 3):
        cfg.aabb[i] = v
    cfg.min_near, cfg.bound, cfg.contract, cfg.last_sample_opaque, cfg.bg_color = 0.2, 2.0, 1, 1, 1.0
    if with_feat:
        g = synth.GRIDS["s_grid"]
        _grid(cfg.feat_grid, g["num_levels"], g["level_dim"], g["log2_hashmap_size"], g["desired_resolution"], f16)
        cfg.with_feat = 1
    for k, v in tuning.items():
        setattr(cfg.tuning, k, v)
    return cfg


def make_io(cfg, N, tile_w=0, debug=(), skip_final=False):
    io = _lib.RenderIO()
    io.rays_o = io.rays_d = PTR
    io.N, io.tile_w = N, tile_w
    S = cfg.num_stages
    if skip_final:
        io.skip_final = 1
        io.bins[S - 1] = PTR
    else:
        io.image = io.depth = io.weights_sum = PTR
    for name in debug:
        if name in ("bins", "weights", "sigmas"):
            getattr(io, name)[S - 1] = PTR
        else:
            setattr(io, name, PTR)
    if cfg.with_feat:
        io.f_feat = PTR
    return io


def route(cfg, io):
    info = _lib.LaunchInfo()
    rc = _lib.lib().sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info))
    assert rc == 0, _lib.lib().sn_last_error()
    return dict(final_kernel=info.final_kernel.decode(), workgroups=info.workgroups, lds_bytes=info.lds_bytes, dense_levels=info.dense_levels,
                gathers=info.gathers_per_wave_sample, launches=info.launches)


def check_workspace(cfg, io):
    """sn_rm_render_workspace_bytes covers what the route needs, and sn_rm_render_rays refuses one byte less before any launch."""
    l = _lib.lib()
    stated = l.sn_rm_render_workspace_bytes(C.byref(cfg), io.N, io.tile_w)
    io.workspace, io.workspace_bytes = PTR, stated - 1
    assert l.sn_rm_render_rays(C.byref(cfg), C.byref(io), None) == -4, l.sn_last_error()
    need = int(re.search(rb"need (\d+)", l.sn_last_error()).group(1))
    assert stated >= need > stated - 4
    io.workspace, io.workspace_bytes = None, 0


N800 = 800 * 800


@pytest.mark.parametrize("f16,densify,kernel,dense,gathers", [
    (True, 0, "k_final_stage<lt,K=7>", 7, 86),        # 800x800 x 128 samples >= 64 Mi: levels 5-6 densified for fp16 tables
    (False, 2, "k_final_stage<lt,K=7>", 7, 100),
    (True, 1, "k_final_stage<lt,K=5>", 5, 98),
    (False, 1, "k_final_stage<lt,K=5>", 5, 108),
    (False, 0, "k_final_stage<lt,K=5>", 5, 108),      # automatic densification is for fp16 tables only
])
def test_single_stage_800x800_is_one_launch_of_2500_workgroups(f16, densify, kernel, dense, gathers):
    cfg = make_cfg([128], f16, densify=densify)
    io = make_io(cfg, N800, 800)
    assert route(cfg, io) == dict(final_kernel=kernel, workgroups=2500, lds_bytes=LDS_F16X3, dense_levels=dense, gathers=gathers, launches=1)
    check_workspace(cfg, io)


def test_reference_schedule_800x800_renders_two_bands_of_1250_workgroups():
    cfg = make_cfg([128, 64, 32], True)
    io = make_io(cfg, N800, 800)
    assert route(cfg, io) == dict(final_kernel="k_final_stage<lt,K=5>", workgroups=1250, lds_bytes=LDS_F16X3, dense_levels=5, gathers=98, launches=2)
    check_workspace(cfg, io)
    cfg = make_cfg([128, 64, 32], True, band_streams=1)
    r = route(cfg, io)
    assert (r["launches"], r["workgroups"]) == (1, 2500)
    check_workspace(cfg, io)


@pytest.mark.parametrize("debug", ["bins", "weights", "sigmas", "xyzs_last", "geo_feat_last"])
def test_a_per_sample_output_of_the_last_stage_takes_the_per_sample_form(debug):
    cfg = make_cfg([64, 32], False)
    io = make_io(cfg, 64 * 64, 64, debug=(debug,))
    r = route(cfg, io)
    assert r["final_kernel"] == "k_final_stage<per-sample,K=5>" and r["lds_bytes"] == LDS_F16X3 and r["gathers"] == 108
    check_workspace(cfg, io)


def test_compact_live_without_debug_outputs_takes_the_compacting_kernel():
    cfg = make_cfg([64, 32], True)
    cfg.compact_live = 1
    io = make_io(cfg, 64 * 64, 64)
    assert route(cfg, io)["final_kernel"] == "k_final_stage_cmp"
    check_workspace(cfg, io)
    assert "per-sample" in route(cfg, make_io(cfg, 64 * 64, 64, debug=("weights",)))["final_kernel"]


def test_small_linear_batches_share_rays_between_lanes_up_to_16384_rays():
    cfg = make_cfg([64, 32], False)
    io = make_io(cfg, 16384)
    assert route(cfg, io)["final_kernel"] == "k_final_stage_sp"
    check_workspace(cfg, io)
    io = make_io(cfg, 16385)
    r = route(cfg, io)
    assert r["final_kernel"] == "k_final_stage<lt,K=5>" and r["workgroups"] == (16385 + 255) // 256
    check_workspace(cfg, io)
    assert route(cfg, make_io(cfg, 16384, 128))["final_kernel"] == "k_final_stage<lt,K=5>"      # image order: one lane per ray
    cfg.tuning.final_sp_max_rays = -1
    assert route(cfg, make_io(cfg, 1000))["final_kernel"] == "k_final_stage<lt,K=5>"


def test_exact_fp32_and_vector_alu_forms_ask_for_their_lds():
    cfg = make_cfg([32], False)
    cfg.mlp_exact_fp32 = 1
    io = make_io(cfg, 4096, 64)
    assert route(cfg, io) == dict(final_kernel="k_final_stage<mfma32>", workgroups=16, lds_bytes=LDS_MFMA32, dense_levels=0, gathers=128, launches=1)
    check_workspace(cfg, io)
    cfg = make_cfg([32], False, mlp_mode=_lib.MLP_VALU)
    assert route(cfg, io) == dict(final_kernel="k_final_stage<valu>", workgroups=16, lds_bytes=LDS_VALU, dense_levels=0, gathers=128, launches=1)
    check_workspace(cfg, io)


def test_another_field_of_the_same_structure_takes_the_size_agnostic_kernel():
    cfg = make_cfg([48, 16], False, main_mlp=(16, 32, 16), view_mlp=(31, 32, 3), main_levels=8)
    io = make_io(cfg, 40 * 24, 40)
    r = route(cfg, io)
    assert r["final_kernel"] == "k_final_stage_any" and r["gathers"] == 8 * 8 and r["dense_levels"] == 0
    assert r["lds_bytes"] == (2 * 32 + 15) * 256 * 4              # two activation rows of the widest layer (32) + 15 geometry channels per lane
    check_workspace(cfg, io)
    cfg.compact_live = 1
    info = _lib.LaunchInfo()
    assert _lib.lib().sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info)) == -2
    assert b"reference network's sizes only" in _lib.lib().sn_last_error()


def test_skip_final_reports_nothing_and_the_feature_stage_keeps_the_linear_tail():
    cfg = make_cfg([64, 32], False)
    io = make_io(cfg, 4096, 64, skip_final=True)
    assert route(cfg, io) == dict(final_kernel="", workgroups=0, lds_bytes=0, dense_levels=0, gathers=0, launches=0)
    check_workspace(cfg, io)
    cfg = make_cfg([64, 32], False, with_feat=True)
    io = make_io(cfg, 4096, 64)
    assert route(cfg, io)["final_kernel"] == "k_final_stage<lt,K=5,aux>"
    check_workspace(cfg, io)


def test_an_experiment_needs_the_experiments_build():
    l = _lib.lib()
    info = _lib.LaunchInfo()
    cfg = make_cfg([128], True, experiment=_lib.EXP_ROLE_SPLIT)
    io = make_io(cfg, 4096, 64)
    if l.sn_build_flags() & _lib.BUILD_EXPERIMENTS:      # (SN_LIB points at an experiments build: the variant is a route of its own)
        assert route(cfg, io)["final_kernel"] == "k_final_stage_rs"
        return
    for call in (lambda: l.sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info)), lambda: l.sn_rm_render_rays(C.byref(cfg), C.byref(io), None)):
        assert call() == -2
        assert l.sn_last_error() == b"render_rays: tuning.experiment=1 needs a library built with -DSN_EXPERIMENTS (make exp)"


def test_statuses_and_messages_are_those_of_render_rays():
    l = _lib.lib()
    info = _lib.LaunchInfo()
    # an input that trips several checks answers with the first one: the output pointers, before the stride, before the schedule
    cfg = make_cfg([128], True)
    cfg.num_stages = 9
    io = make_io(cfg, 4096, 64)
    io.out_stride = 4
    for call in (lambda: l.sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info)), lambda: l.sn_rm_render_rays(C.byref(cfg), C.byref(io), None)):
        assert call() == -1 and b"out_stride 4" in l.sn_last_error()
        io.image = None
        assert call() == -1 and b"outputs must be device pointers" in l.sn_last_error()
        io.image, io.out_stride = PTR, 0
        assert call() == -1 and b"num_stages=9" in l.sn_last_error()
        io.out_stride = 4
    # proposal-only call with a stage count out of range: the num_stages check answers (no slot of io->bins belongs to stage 9)
    io.out_stride, io.skip_final = 0, 1
    assert l.sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info)) == -1 and b"num_stages=9" in l.sn_last_error()
    assert l.sn_rm_render_workspace_bytes(C.byref(cfg), 4096, 64) == 8192 * 4
    # the workspace is the last thing sn_rm_render_rays asks for, and the dry run never does
    cfg = make_cfg([128], True)
    io = make_io(cfg, 4096, 64)
    assert l.sn_rm_render_rays(C.byref(cfg), C.byref(io), None) == -1 and b"workspace is NULL" in l.sn_last_error()
    io.workspace, io.workspace_bytes = 72, 1 << 30
    assert l.sn_rm_render_rays(C.byref(cfg), C.byref(io), None) == -1 and b"16-byte aligned" in l.sn_last_error()
    assert l.sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info)) == 0
    io.N = 0
    assert l.sn_rm_render_route_info(C.byref(cfg), C.byref(io), C.byref(info)) == 0 and info.launches == 0 and info.final_kernel == b""
