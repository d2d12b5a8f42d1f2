"""GPU tests of the parity order of the last stage's hashed-level gathers (render_gather.h: issue_level_lv<..., PY, PZ> / blend_level_par): a lane
puts into instruction (a, b) of a level the corner whose absolute y / z has parity a / b, and trades the landed values back before the blend.
A wrong slot is an error of order 1e-2 in the image.  Shapes: a block of the bench camera's 800x800 ray grid, where the lanes of a wave sit in
equal and adjacent cells of the fine levels (merged lines, mixed parities inside one instruction), and a small wide-angle image whose rays each
have their own cells and whose far samples reach the border of [0,1]^3 (the form with the clamped neighbour).  Every kernel that takes the
order is run: the linear-tail form with 7 and with 5 dense levels, the per-sample form, the compaction kernel, and the linear-tail form with
the feature stage behind it; fp16 and fp32 tables; one stage and three."""
import numpy as np
import pytest
import torch

from helpers import camera_rays, oracle_cfg, product_model, synthetic_params

pytestmark = pytest.mark.gpu

# the bounds tests/test_gpu_render.py holds these routes to against the oracle
IMAGE_ATOL = 1e-5
DEPTH_RTOL, DEPTH_ATOL = 1e-5, 1e-5
WSUM_ATOL = 1e-6

STEPS = [[8], [8, 4, 4]]
SHAPES = ["dense_block", "sparse_image"]
# route -> (RenderPlan arguments, render_rays `want`, tuning, what the launched kernel's name must contain)
ROUTES = {
    "linear_tail_K7": (dict(), (), dict(densify=2), "<lt,K=7"),
    "linear_tail_K5": (dict(), (), dict(densify=1), "<lt,K=5"),
    "per_sample": (dict(), ("weights", "bins"), dict(), "<per-sample,K=5"),
    "compact_live": (dict(compact_live=True), (), dict(), "k_final_stage_cmp"),
    "feature_stage": (dict(feat=True), ("f_image",), dict(), "<lt,K=5,aux"),
}
KEYS = ("image", "depth", "weights_sum")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b):
    """equality of the bit patterns (a depth may be NaN, and NaN != NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


_cache = {}


def rays_of(orc, shape):
    if shape == "dense_block":          # 24 rows x 16 columns of the bench camera's 800 x 800 rays, around the image centre
        _, _, ro, rd = camera_rays(orc, 800, 800)
        rows = (np.arange(388, 412)[:, None] * 800 + np.arange(392, 408)[None, :]).ravel()
        return ro[rows], rd[rows], 16
    _, _, ro, rd = camera_rays(orc, 40, 24, radius=1.1, elev=15.0, azim=75.0)
    return ro, rd, 24


def scene(orc, gpu, shape, steps):
    """(params, model, rays) of one case, built once and left unchanged; the oracle's renders are cached per table precision beside them."""
    key = (shape, tuple(steps))
    if key not in _cache:
        if ("rays", shape) not in _cache:
            _cache[("rays", shape)] = rays_of(orc, shape)
        ro, rd, W = _cache[("rays", shape)]
        params = synthetic_params(steps, heads=True, seed=43)
        _cache[key] = dict(params=params, model=product_model(params, steps, True, gpu), ro=ro, rd=rd, W=W, want={})
    return _cache[key]


def oracle_of(orc, sc, steps, f16):
    if f16 not in sc["want"]:
        sc["want"][f16] = orc.render(oracle_cfg(orc, sc["params"], steps, table_f16=f16), sc["ro"], sc["rd"])
    return sc["want"][f16]


def pin_route(monkeypatch, rm):
    monkeypatch.setattr(rm.tuning, "final_sp_max_rays", -1)
    monkeypatch.setattr(rm.tuning, "prop_sp_max_rays", -1)


def plan_of(rm, sc, steps, f16, route):
    args = dict(ROUTES[route][0])
    if args.pop("feat", False):
        args["feat_encoder"] = sc["model"].s_grid
    return rm.RenderPlan(sc["model"], steps, torch.float16 if f16 else torch.float32, **args)


def render(rm, plan, sc, gpu, route, **more):
    _, want, tuning, name = ROUTES[route]
    out = rm.render_rays(plan, T(sc["ro"], gpu), T(sc["rd"], gpu), tile_w=sc["W"], want=want, out={}, tuning=rm.Tuning(**tuning, **more))
    info = rm.last_launch_info()
    assert name in info["final_kernel"], (route, info)
    return {k: v.clone() for k, v in out.items()}, info


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_order_against_the_oracle(gpu, orc, monkeypatch, shape, steps, f16, route):
    """image, depth and weights_sum within the bounds of tests/test_gpu_render.py, equal bits from call to call, and the launch's gather count
    what the canonical order had: the instruction count does not change."""
    from sanerf_hq_amd import raymarching as rm
    pin_route(monkeypatch, rm)
    sc = scene(orc, gpu, shape, steps)
    want = oracle_of(orc, sc, steps, f16)
    plan = plan_of(rm, sc, steps, f16, route)
    a, info = render(rm, plan, sc, gpu, route)
    b, _ = render(rm, plan, sc, gpu, route)
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]), (k, "two renders of one case differ")
    dense = info["dense_levels"]
    assert info["gathers_per_wave_sample"] == dense * (2 if f16 else 4) + (16 - dense) * 8, info
    if route == "linear_tail_K7" and f16:
        assert info["gathers_per_wave_sample"] == 86
    err = float(np.abs(a["image"].cpu().numpy() - want["image"]).max())
    print(f"{shape} {steps} f16={f16} {route}: max|dRGB| = {err:.2e}")
    np.testing.assert_allclose(a["image"].cpu().numpy(), want["image"], rtol=0, atol=IMAGE_ATOL)
    np.testing.assert_allclose(a["depth"].cpu().numpy(), want["depth"], rtol=DEPTH_RTOL, atol=DEPTH_ATOL)
    np.testing.assert_allclose(a["weights_sum"].cpu().numpy(), want["weights_sum"], rtol=0, atol=WSUM_ATOL)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_order_equals_the_canonical_order_bit_for_bit(gpu, orc, monkeypatch, experiments_build, shape, steps, f16, route):
    """The exchange is a lane-wise permutation undone before the blend: every output tensor equals the canonical-order partner's
    (tuning.experiment = EXP_GATHER_CANONICAL, the same instantiation with the switch off)."""
    from sanerf_hq_amd import _lib, raymarching as rm
    pin_route(monkeypatch, rm)
    sc = scene(orc, gpu, shape, steps)
    plan = plan_of(rm, sc, steps, f16, route)
    a, ia = render(rm, plan, sc, gpu, route)
    b, ib = render(rm, plan, sc, gpu, route, experiment=_lib.EXP_GATHER_CANONICAL)
    assert ia["final_kernel"] == ib["final_kernel"] and ia["gathers_per_wave_sample"] == ib["gathers_per_wave_sample"]
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]), (k, float((a[k].float() - b[k].float()).abs().nan_to_num().max()))
    if route == "feature_stage":
        assert "f_feat" in a and float(a["f_feat"].abs().max()) > 0


@pytest.mark.parametrize("steps", STEPS)
def test_the_shapes_reach_what_they_are_meant_to(gpu, orc, monkeypatch, steps):
    """Through the exported sample positions of the last stage: on the sparse image at least one wave holds a sample less than 1.5 cells of
    the coarsest hashed level (level 5 or 7: the wider margin of level 5 is the one tested against) from the border of [0,1]^3, so that wave
    takes the form with the clamped neighbour (single-stage schedule: its samples run out to the far bound; behind proposal stages the last
    stage's few samples sit around the surface, inside); on the dense block the lanes of a wave tile differ in cell parity on levels 12 and 15 and share cells on level 12."""
    from sanerf_hq_amd import raymarching as rm
    pin_route(monkeypatch, rm)
    res = {7: 213, 12: 1352, 15: 4096}
    for shape in SHAPES:
        sc = scene(orc, gpu, shape, steps)
        plan = rm.RenderPlan(sc["model"], steps, torch.float16)
        out = rm.render_rays(plan, T(sc["ro"], gpu), T(sc["rd"], gpu), tile_w=sc["W"], want=("xyzs_last",), out={})
        bound = float(oracle_cfg(orc, sc["params"], steps).bound)
        x01 = (out["xyzs_last"].double().cpu().numpy() + bound) / (2.0 * bound)            # [N, T, 3]
        if shape == "sparse_image":
            if len(steps) > 1:
                continue
            margin = 1.5 / res[7]                     # level 7's margin: inside it, a sample is outside the interior for K = 5 as well
            outside = (x01 < margin) | (x01 > 1.0 - margin)
            assert outside.any(), "no sample near the border: every wave would take the fast form"
            assert not outside.all(axis=(1, 2)).all(), "and some stay inside"
        else:
            for lvl in (12, 15):
                cell = np.floor(np.clip(x01 * res[lvl] - 0.5, 0, res[lvl] - 1)).astype(np.int64)       # [N, T, 3]
                tile = cell.reshape(3, 8, 2, 8, -1, 3)[0, :, 0]                                        # the first 8x8-pixel tile: [8, 8, T, 3]
                par = (tile[..., 1:] & 1).reshape(64, -1, 2)
                assert (par.min(axis=0) != par.max(axis=0)).any(), f"level {lvl}: the lanes of a tile never differ in cell parity"
            flat = np.floor(np.clip(x01 * res[12] - 0.5, 0, res[12] - 1)).astype(np.int64).reshape(3, 8, 2, 8, -1, 3)[0, :, 0].reshape(64, -1, 3)
            assert any(len({tuple(c) for c in flat[:, j]}) < 64 for j in range(flat.shape[1])), "level 12: no two lanes of a tile share a cell"
