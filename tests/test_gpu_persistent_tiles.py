"""GPU tests of the persistent launch of the last stage (render.hip: k_final_stage_pt; tuning.persistent_tiles): resident 8-wave workgroups
whose waves pull 64-ray wave tiles from eight queues run the code of the ordinary launch on every ray, so image, depth and weights_sum
equal the ordinary launch's (persistent_tiles = 1) bit for bit.  The outputs are filled with NaN before every render: a tile nobody took
stays NaN.  Shapes are the smallest at which the queues can go wrong: one tile (seven of a workgroup's eight waves get nothing), 15 tiles
with an odd last wave-tile row, partial tiles on both axes, rays in linear order, and 625 tile units through one workgroup (every tile
through the same eight waves), through three (queues 3-7 are reached only by waves that ran out of their own) and through the default
grid (more waves than tiles)."""
import pytest
import torch

from helpers import product_model, synthetic_params

pytestmark = pytest.mark.gpu

KEYS = ("image", "depth", "weights_sum")
BASE = dict(final_sp_max_rays=-1, prop_sp_max_rays=-1)      # small linear-order batches: one lane per ray, the launch this form replaces
# name -> (W, rows, rays in linear order, persistent_wgs)
SHAPES = {
    "one_tile_8x8": (8, 8, 0, 0),
    "15_tiles_40x24": (40, 24, 0, 0),
    "partial_tiles_37x29": (37, 29, 0, 0),
    "linear_1000": (40, 25, 1000, 0),
    "200x200_one_workgroup": (200, 200, 0, 1),
    "200x200_three_workgroups": (200, 200, 0, 3),
    "200x200_default_grid": (200, 200, 0, 0),
}

_cache = {}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def model_of(gpu, steps):
    key = ("model", tuple(steps))
    if key not in _cache:
        _cache[key] = product_model(synthetic_params(steps, seed=31), steps, False, gpu)
    return _cache[key]


def plan_of(rm, gpu, steps, f16):
    key = ("plan", tuple(steps), f16)
    if key not in _cache:
        _cache[key] = rm.RenderPlan(model_of(gpu, steps), steps, torch.float16 if f16 else torch.float32)
    return _cache[key]


def rays_of(rm, gpu, W, rows, linear=0, row_begin=0, row_end=None):
    from sanerf_hq_amd import synth
    key = ("rays", W, rows, linear, row_begin, row_end)
    if key not in _cache:
        ro, rd = rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(rows, W), rows, W, device=gpu, row_begin=row_begin, row_end=row_end)
        _cache[key] = (ro[:linear].contiguous(), rd[:linear].contiguous(), 0) if linear else (ro, rd, W)
    return _cache[key]


def render(rm, plan, rays, **tn):
    ro, rd, tile = rays
    N = ro.shape[0]
    nan = float("nan")
    out = {"image": torch.full((N, 3), nan, device=ro.device), "depth": torch.full((N,), nan, device=ro.device), "weights_sum": torch.full((N,), nan, device=ro.device)}
    t = rm.Tuning(**BASE, **tn)
    res = rm.render_rays(plan, ro, rd, tile_w=tile, tuning=t, out=out)
    info = rm.last_launch_info()
    assert info == rm.route_info(plan, N, tile, tuning=t), "the dry run and the launch agree field for field"
    assert all(res[k].data_ptr() == out[k].data_ptr() for k in KEYS), "rendered into the NaN-filled tensors"
    return {k: res[k].clone() for k in KEYS}, info


def check_pair(rm, gpu, plan, rays, wgs=0, **tn):
    ref, iref = render(rm, plan, rays, persistent_tiles=1, **tn)
    got, info = render(rm, plan, rays, persistent_tiles=2, persistent_wgs=wgs, **tn)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert iref["persistent_tiles"] == 0 and iref["grid_workgroups"] == iref["workgroups"], iref
    assert info["persistent_tiles"] == 1 and info["grid_workgroups"] == (wgs or cus), info
    assert (info["final_kernel"], info["workgroups"], info["launches"], info["dense_levels"]) == (iref["final_kernel"], iref["workgroups"], iref["launches"], iref["dense_levels"])
    assert "<lt,K=" in info["final_kernel"] and "aux" not in info["final_kernel"]
    assert not torch.isnan(got["image"]).any() and not torch.isnan(got["weights_sum"]).any(), "a ray nobody rendered"
    for k in KEYS:
        assert same_bits(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    return got, info


@pytest.mark.parametrize("densify", [1, 2])
@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("steps", [[16], [16, 8, 8]])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_persistent_launch_equals_the_ordinary_launch_bit_for_bit(gpu, shape, steps, f16, densify):
    from sanerf_hq_amd import raymarching as rm
    W, rows, linear, wgs = SHAPES[shape]
    _, info = check_pair(rm, gpu, plan_of(rm, gpu, steps, f16), rays_of(rm, gpu, W, rows, linear), wgs, densify=densify, band_streams=1)
    # levels 5-6 are densified for the single-stage schedule's plain launch when asked for (K = 7); the others stay at K = 5
    assert info["dense_levels"] == (7 if densify == 2 else 5)
    assert info["workgroups"] == (-(-linear // 256) if linear else -(-(-(-W // 8) * -(-rows // 8)) // 4))


@pytest.mark.parametrize("f16", [True, False])
def test_two_row_bands_on_two_streams_have_a_counter_set_each(gpu, f16):
    from sanerf_hq_amd import raymarching as rm
    _, info = check_pair(rm, gpu, plan_of(rm, gpu, [16, 8, 8], f16), rays_of(rm, gpu, 200, 200), band_streams=2)
    assert info["launches"] == 2


def test_packed_outputs_and_a_row_band(gpu):
    """sn_render_io.out_stride (rgb | depth | weights_sum as columns of one [N,5] buffer) and the rays of rows 64..136 of the image."""
    from sanerf_hq_amd import raymarching as rm
    plan = plan_of(rm, gpu, [16], True)
    ro, rd, W = rays_of(rm, gpu, 200, 200, row_begin=64, row_end=136)
    assert ro.shape[0] == 72 * 200
    bufs = []
    for pt in (1, 2):
        packed = torch.full((ro.shape[0], 5), float("nan"), device=gpu)
        res = rm.render_rays(plan, ro, rd, tile_w=W, tuning=rm.Tuning(**BASE, persistent_tiles=pt), packed=packed, out={})
        assert rm.last_launch_info()["persistent_tiles"] == pt - 1
        assert res["image"].data_ptr() == packed.data_ptr()
        bufs.append(packed)
    assert not torch.isnan(bufs[1]).any()
    assert same_bits(bufs[0], bufs[1])
    band, _ = check_pair(rm, gpu, plan, (ro, rd, W))
    assert same_bits(band["image"], bufs[1][:, :3].contiguous()) and same_bits(band["depth"], bufs[1][:, 3].contiguous())
    # the band's rays are those rows of the whole image
    whole, _ = render(rm, plan, rays_of(rm, gpu, 200, 200), persistent_tiles=2)
    assert same_bits(whole["image"][64 * 200:136 * 200], band["image"])


def test_three_calls_on_one_plan_and_workspace(gpu):
    """The counters are zeroed ahead of every launch: nothing depends on what the previous one left in the workspace."""
    from sanerf_hq_amd import raymarching as rm
    for steps in ([16], [16, 8, 8]):
        plan = plan_of(rm, gpu, steps, True)
        rays = rays_of(rm, gpu, 200, 200)
        ref, _ = render(rm, plan, rays, persistent_tiles=1)
        ws = plan._ws.data_ptr()
        for wgs in (3, 0, 3):
            got, info = render(rm, plan, rays, persistent_tiles=2, persistent_wgs=wgs)
            assert info["persistent_tiles"] == 1 and plan._ws.data_ptr() == ws
            for k in KEYS:
                assert same_bits(got[k], ref[k]), (steps, wgs, k)


def test_captured_graph_replays(gpu):
    """The single-stream [16] render captured once with torch.cuda.graph: the counters' reset is part of the capture, every replay renders."""
    from sanerf_hq_amd import raymarching as rm
    plan = plan_of(rm, gpu, [16], True)
    ro, rd, W = rays_of(rm, gpu, 200, 200)
    ref, _ = render(rm, plan, (ro, rd, W), persistent_tiles=1)
    t = rm.Tuning(**BASE, persistent_tiles=2)
    out = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rm.render_rays(plan, ro, rd, tile_w=W, tuning=t, out=out)          # warm-up: workspace, outputs
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rm.render_rays(plan, ro, rd, tile_w=W, tuning=t, out=out)
    assert rm.last_launch_info()["persistent_tiles"] == 1
    for _ in range(3):
        for k in KEYS:
            out[k].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert same_bits(out[k], ref[k]), k


def test_the_bench_line_takes_the_persistent_launch_by_itself(gpu):
    """800x800, [128], fp16 tables, default tuning: 10 000 wave tiles are more than the device's resident wave slots, so the automatic rule
    picks the persistent form; the kernel's name and the count of 256-ray tile units are what they were, and so is every bit of the outputs."""
    from sanerf_hq_amd import raymarching as rm
    plan = plan_of(rm, gpu, [128], True)
    rays = rays_of(rm, gpu, 800, 800)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert 10000 > 8 * cus
    ref, iref = render(rm, plan, rays, persistent_tiles=1)
    ro, rd, W = rays
    out = {k: torch.full_like(v, float("nan")) for k, v in ref.items()}
    res = rm.render_rays(plan, ro, rd, tile_w=W, tuning=rm.Tuning(), out=out)
    info = rm.last_launch_info()
    assert info == rm.route_info(plan, ro.shape[0], W, tuning=rm.Tuning())
    assert (info["persistent_tiles"], info["workgroups"], info["final_kernel"], info["grid_workgroups"], info["launches"]) == (1, 2500, "k_final_stage<lt,K=7>", cus, 1), info
    assert (iref["persistent_tiles"], iref["workgroups"], iref["final_kernel"], iref["grid_workgroups"]) == (0, 2500, "k_final_stage<lt,K=7>", 2500), iref
    for k in KEYS:
        assert same_bits(res[k], ref[k]), k
