"""GPU tests of the matrix phase of the linear-tail last stage (render_mfma.h: grid_mlp_mfma16_l12_spread), whose vector work -- ReLU and
hi/lo splits, the density dot, the weight and slab reads -- is issued under its MFMAs: parity with the CPU oracle, bit equality with the
order it replaces (tuning.experiment = EXP_MATRIX_CLUMPED, experiments builds) and equal bits from call to call, on images of one full
workgroup and of a padded one, sample counts that hit the first, the last and an odd iteration of the march, both table precisions and
both dense-level counts, a camera outside the box and an opaque field with the exact early-out."""
import numpy as np
import pytest
import torch

from helpers import camera_rays, oracle_cfg, product_model, synthetic_params

pytestmark = pytest.mark.gpu

# what tests/test_gpu_final_stage.py holds the linear-tail kernel to against the oracle (test_linear_tail_form_vs_per_sample_form_and_oracle,
# test_wave_tile_workgroups_any_band_shape), and on the gain-40 field with the early-outs (test_opaque_field_vs_oracle_with_early_outs)
IMAGE_ATOL = 1e-5
DEPTH_RTOL, DEPTH_ATOL = 1e-5, 1e-5
OPAQUE_DEPTH_RTOL, OPAQUE_DEPTH_ATOL, OPAQUE_WSUM_ATOL = 1e-4, 1e-5, 1e-5

IMAGES = [(16, 16), (20, 12)]          # one full workgroup; 240 rays: a padded workgroup, partial wave tiles, inactive lanes
STEPS = [[1], [2], [5], [128]]
DENSIFY = [(2, 7), (1, 5)]             # (tuning.densify, dense levels of the instantiation): K = 7 as on the bench line, K = 5
KEYS = ("image", "depth", "weights_sum")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b):
    """torch.equal on the bit patterns: a ray that misses the box carries depth NaN (inf - inf, as in the reference), and NaN != NaN."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def pin_route(monkeypatch, rm):
    """Small batches stay on k_final_stage<lt, ...> (the several-lanes-per-ray kernels keep the per-sample form)."""
    monkeypatch.setattr(rm.tuning, "final_sp_max_rays", -1)
    monkeypatch.setattr(rm.tuning, "prop_sp_max_rays", -1)


_cache = {}


def scene(orc, gpu, steps, gain=4.0, radius=1.0, hw=(16, 16), heads=False):
    """(params, model, rays) of one case, built once; the oracle's render of it is cached per table precision beside them."""
    key = (tuple(steps), gain, radius, hw, heads)
    if key not in _cache:
        params = synthetic_params(steps, heads=heads, seed=43, gain=gain)
        model = product_model(params, steps, heads, gpu)
        _, _, ro, rd = camera_rays(orc, hw[0], hw[1], radius=radius, elev=20.0, azim=30.0)
        _cache[key] = dict(params=params, model=model, ro=ro, rd=rd, want={})
    return _cache[key]


def oracle_of(orc, sc, steps, f16):
    if f16 not in sc["want"]:
        sc["want"][f16] = orc.render(oracle_cfg(orc, sc["params"], steps, table_f16=f16), sc["ro"], sc["rd"])
    return sc["want"][f16]


def render(rm, plan, sc, gpu, W, **tuning):
    out = rm.render_rays(plan, T(sc["ro"], gpu), T(sc["rd"], gpu), tile_w=W, out={}, tuning=rm.Tuning(**tuning))
    info = rm.last_launch_info()
    return {k: v.clone() for k, v in out.items()}, info


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("hw", IMAGES)
def test_parity_with_the_oracle_and_determinism(gpu, orc, monkeypatch, hw, steps, f16):
    from sanerf_hq_amd import raymarching as rm
    pin_route(monkeypatch, rm)
    sc = scene(orc, gpu, steps, hw=hw)
    want = oracle_of(orc, sc, steps, f16)
    plan = rm.RenderPlan(sc["model"], steps, torch.float16 if f16 else torch.float32)
    for densify, K in DENSIFY:
        a, info = render(rm, plan, sc, gpu, hw[1], densify=densify)
        assert "<lt" in info["final_kernel"] and info["dense_levels"] == K, info
        b, _ = render(rm, plan, sc, gpu, hw[1], densify=densify)
        for k in KEYS:
            assert same_bits(a[k], b[k]), (k, K, "two renders of one case differ")
        err = float(np.abs(a["image"].cpu().numpy() - want["image"]).max())
        print(f"{hw} {steps} f16={f16} K={K}: max|dRGB| = {err:.2e}")
        np.testing.assert_allclose(a["image"].cpu().numpy(), want["image"], rtol=0, atol=IMAGE_ATOL)
        np.testing.assert_allclose(a["depth"].cpu().numpy(), want["depth"], rtol=DEPTH_RTOL, atol=DEPTH_ATOL)


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("hw", IMAGES)
def test_camera_outside_the_box(gpu, orc, monkeypatch, hw, f16):
    """Rays that enter the box from outside: samples in border cells take the span code's non-FAST path, samples outside [0, 1] get zero features."""
    from sanerf_hq_amd import raymarching as rm
    pin_route(monkeypatch, rm)
    steps = [128]
    aabb = [-1.0] * 3 + [1.0] * 3
    sc = scene(orc, gpu, steps, radius=3.0, hw=hw)
    key = ("aabb", f16)
    if key not in sc["want"]:
        sc["want"][key] = orc.render(oracle_cfg(orc, sc["params"], steps, table_f16=f16, aabb=aabb), sc["ro"], sc["rd"])
    want = sc["want"][key]
    assert float(np.isfinite(want["depth"]).mean()) > 0.2, "the camera is meant to look at the box"
    monkeypatch.setattr(sc["model"], "aabb_infer", torch.tensor(aabb, device=gpu), raising=False)
    monkeypatch.setattr(sc["model"], "aabb_train", torch.tensor(aabb, device=gpu), raising=False)
    plan = rm.RenderPlan(sc["model"], steps, torch.float16 if f16 else torch.float32)
    for densify, K in DENSIFY:
        a, info = render(rm, plan, sc, gpu, hw[1], densify=densify)
        assert "<lt" in info["final_kernel"] and info["dense_levels"] == K, info
        b, _ = render(rm, plan, sc, gpu, hw[1], densify=densify)
        for k in KEYS:
            assert same_bits(a[k], b[k]), (k, K)
        np.testing.assert_allclose(a["image"].cpu().numpy(), want["image"], rtol=0, atol=IMAGE_ATOL)
        np.testing.assert_allclose(a["depth"].cpu().numpy(), want["depth"], rtol=DEPTH_RTOL, atol=DEPTH_ATOL)


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("hw", IMAGES)
def test_opaque_field_with_the_exact_early_out(gpu, orc, monkeypatch, hw, f16):
    from sanerf_hq_amd import raymarching as rm
    pin_route(monkeypatch, rm)
    steps = [128]
    sc = scene(orc, gpu, steps, gain=40.0, hw=hw)
    want = oracle_of(orc, sc, steps, f16)
    assert float((want["weights_sum"] > 0.999).mean()) > 0.3, "the scene is meant to be mostly opaque"
    plan = rm.RenderPlan(sc["model"], steps, torch.float16 if f16 else torch.float32)
    for densify, K in DENSIFY:
        a, info = render(rm, plan, sc, gpu, hw[1], densify=densify, exact_early_out=2)
        assert "<lt" in info["final_kernel"] and info["dense_levels"] == K, info
        b, _ = render(rm, plan, sc, gpu, hw[1], densify=densify, exact_early_out=2)
        for k in KEYS:
            assert same_bits(a[k], b[k]), (k, K)
        np.testing.assert_allclose(a["image"].cpu().numpy(), want["image"], rtol=0, atol=IMAGE_ATOL)
        np.testing.assert_allclose(a["depth"].cpu().numpy(), want["depth"], rtol=OPAQUE_DEPTH_RTOL, atol=OPAQUE_DEPTH_ATOL)
        np.testing.assert_allclose(a["weights_sum"].cpu().numpy(), want["weights_sum"], rtol=0, atol=OPAQUE_WSUM_ATOL)


def both_orders(rm, _lib, plan, sc, gpu, W, want=(), **tuning):
    ro, rd = T(sc["ro"], gpu), T(sc["rd"], gpu)
    a = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, want=want, out={}, tuning=rm.Tuning(**tuning)).items()}
    name = rm.last_launch_info()["final_kernel"]
    b = rm.render_rays(plan, ro, rd, tile_w=W, want=want, out={}, tuning=rm.Tuning(experiment=_lib.EXP_MATRIX_CLUMPED, **tuning))
    assert "<lt" in name and rm.last_launch_info()["final_kernel"] == name
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]), (k, tuning, float((a[k] - b[k]).abs().nan_to_num().max()))
    return a


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("hw", IMAGES)
def test_spread_order_equals_the_clumped_order_bit_for_bit(gpu, orc, monkeypatch, experiments_build, hw, steps, f16):
    """Every accumulator receives the same products in the same order whichever way the phase is issued: image, depth, weights_sum (and the
    per-ray features, with the feature stage -- the AUX instantiation, whose weights feed it -- the features it accumulates) are equal."""
    from sanerf_hq_amd import _lib, raymarching as rm
    pin_route(monkeypatch, rm)
    sc = scene(orc, gpu, steps, hw=hw, heads=True)
    td = torch.float16 if f16 else torch.float32
    plan = rm.RenderPlan(sc["model"], steps, td)
    for densify, _ in DENSIFY:
        both_orders(rm, _lib, plan, sc, gpu, hw[1], want=("f_image",), densify=densify)
    plan_aux = rm.RenderPlan(sc["model"], steps, td, feat_encoder=sc["model"].s_grid)
    out = both_orders(rm, _lib, plan_aux, sc, gpu, hw[1], want=("f_image",))
    assert "f_feat" in out and float(out["f_feat"].abs().max()) > 0


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("hw", IMAGES)
def test_spread_order_equals_the_clumped_order_outside_camera_and_opaque(gpu, orc, monkeypatch, experiments_build, hw, f16):
    from sanerf_hq_amd import _lib, raymarching as rm
    pin_route(monkeypatch, rm)
    steps = [128]
    td = torch.float16 if f16 else torch.float32
    opaque = scene(orc, gpu, steps, gain=40.0, hw=hw)
    plan = rm.RenderPlan(opaque["model"], steps, td)
    for densify, _ in DENSIFY:
        both_orders(rm, _lib, plan, opaque, gpu, hw[1], densify=densify, exact_early_out=2)
    outside = scene(orc, gpu, steps, radius=3.0, hw=hw)
    aabb = torch.tensor([-1.0] * 3 + [1.0] * 3, device=gpu)
    monkeypatch.setattr(outside["model"], "aabb_infer", aabb, raising=False)
    monkeypatch.setattr(outside["model"], "aabb_train", aabb, raising=False)
    plan = rm.RenderPlan(outside["model"], steps, td)
    for densify, _ in DENSIFY:
        both_orders(rm, _lib, plan, outside, gpu, hw[1], densify=densify)
