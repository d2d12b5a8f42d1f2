"""GPU: the workgroup -> image tile orders of the fused render (tuning.linear_tile_order 0..4) are bit-neutral, and the packed weights /
pair rows a RenderPlan keeps between calls (keep_packs, sn_render_io.pack_valid) render the same bits as packing on every call.

Small images that still take every odd path of the order: an odd number of wave-tile rows with a partial last workgroup (40x24: 5x3 wave
tiles), partial super-tiles in both directions and a second, mirrored super-tile row (136x136: 9x9 blocks), several stages that hand
their scratch columns on (136x40, [8,4,4]) and the feature stage behind the last one (40x24)."""
import pytest
import torch

from helpers import camera_rays, product_model, synthetic_params

pytestmark = pytest.mark.gpu



def _rays(orc, gpu, W, rows):
    _, _, ro, rd = camera_rays(orc, rows, W, radius=1.1, elev=15.0, azim=75.0)
    return torch.from_numpy(ro).to(gpu), torch.from_numpy(rd).to(gpu)


def _render(rm, plan, ro, rd, W, order, want=()):
    out = rm.render_rays(plan, ro, rd, tile_w=W, want=want, tuning=rm.Tuning(linear_tile_order=order), out={})
    return {k: v.clone() for k, v in out.items()}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("W,rows,steps", [(40, 24, [8]), (136, 136, [8]), (136, 40, [8, 4, 4])])
def test_every_tile_order_renders_the_same_bits(gpu, orc, W, rows, steps, f16):
    from sanerf_hq_amd import raymarching as rm
    model = product_model(synthetic_params(steps, seed=41), steps, False, gpu)
    ro, rd = _rays(orc, gpu, W, rows)
    plan = rm.RenderPlan(model, steps, torch.float16 if f16 else torch.float32)
    for want in ((), ("weights", "bins")):              # the default last stage; the per-sample form with every stage's exported tensors
        ref = _render(rm, plan, ro, rd, W, 1, want)
        assert {"image", "depth", "weights_sum"} <= ref.keys() and float(ref["weights_sum"].abs().max()) > 0
        if want:
            assert all(f"weights{k}" in ref and f"bins{k}" in ref for k in range(len(steps)))
        for order in (0, 2, 3, 4):
            _same(_render(rm, plan, ro, rd, W, order, want), ref, f"order {order} vs 1, want={want}")


@pytest.mark.parametrize("f16", [False, True])
def test_every_tile_order_with_the_feature_stage(gpu, orc, f16):
    from sanerf_hq_amd import raymarching as rm
    steps, W, rows = [8, 4], 40, 24
    model = product_model(synthetic_params(steps, heads=True, seed=5), steps, True, gpu)
    ro, rd = _rays(orc, gpu, W, rows)
    plan = rm.RenderPlan(model, steps, torch.float16 if f16 else torch.float32, feat_encoder=model.s_grid)
    ref = _render(rm, plan, ro, rd, W, 1, ("f_image",))
    assert float(ref["f_feat"].abs().max()) > 0
    for order in (0, 2, 3, 4):
        _same(_render(rm, plan, ro, rd, W, order, ("f_image",)), ref, f"order {order} vs 1")


@pytest.mark.parametrize("f16", [False, True])
def test_kept_packs_render_the_bits_of_the_packing_call(gpu, orc, f16):
    from sanerf_hq_amd import raymarching as rm
    steps, W, rows = [8], 40, 24
    model = product_model(synthetic_params(steps, seed=41), steps, False, gpu)
    ro, rd = _rays(orc, gpu, W, rows)
    dtype = torch.float16 if f16 else torch.float32
    plain = {k: v.clone() for k, v in rm.render_rays(rm.RenderPlan(model, steps, dtype), ro, rd, tile_w=W).items()}
    plan = rm.RenderPlan(model, steps, dtype, keep_packs=True)
    first = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
    assert plan.pack_reuses == 0
    _same(first, plain, "a plan that keeps its packs vs one that does not")
    for i in (1, 2):
        again = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
        assert plan.pack_reuses == i, "the call did not run on the kept packs"
        _same(again, first, f"call {i} on kept packs")
    # another route (exported per-sample tensors: other dense prefix / kernel) packs again, and so does the call after it
    rm.render_rays(plan, ro, rd, tile_w=W, want=("weights",), out={})
    assert plan.pack_reuses == 2
    _same({k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}, first, "back on the first route")
    assert plan.pack_reuses == 2
    # a plan that did not opt in never sets the flag
    p0 = rm.RenderPlan(model, steps, dtype)
    rm.render_rays(p0, ro, rd, tile_w=W, out={}); rm.render_rays(p0, ro, rd, tile_w=W, out={})
    assert p0.pack_reuses == 0 and p0._pack_key is None


def test_kept_packs_are_dropped_on_invalidation_and_on_a_version_change(gpu, orc):
    from sanerf_hq_amd import raymarching as rm
    steps, W, rows = [8], 40, 24
    model = product_model(synthetic_params(steps, seed=41), steps, False, gpu)
    ro, rd = _rays(orc, gpu, W, rows)

    def fresh():
        return {k: v.clone() for k, v in rm.render_rays(rm.RenderPlan(model, steps), ro, rd, tile_w=W, out={}).items()}

    plan = rm.RenderPlan(model, steps, keep_packs=True)
    before = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
    rm.render_rays(plan, ro, rd, tile_w=W, out={})
    assert plan.pack_reuses == 1
    # a write the version counters cannot see: the handshake asks the writer for invalidate_range() (as the range guard does)
    with torch.no_grad():
        model.grid.embeddings.data.mul_(0.5)
        model.grid_mlp.net[0].weight.data.mul_(1.25)
    plan.invalidate_range()
    after = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
    assert plan.pack_reuses == 1, "invalidate_range() must make the next call pack again"
    _same(after, fresh(), "after .data writes + invalidate_range()")
    assert not torch.equal(after["image"], before["image"])
    rm.render_rays(plan, ro, rd, tile_w=W, out={})
    assert plan.pack_reuses == 2, "the packs of the call after the invalidation are kept again"
    # a write that moves a version counter is seen without any call
    with torch.no_grad():
        model.grid.embeddings.mul_(1.5)
    bumped = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
    assert plan.pack_reuses == 2, "a bumped version counter must make the plan pack again"
    _same(bumped, fresh(), "after an in-place update that bumps the version")
    with torch.no_grad():
        model.grid_mlp.net[1].weight.mul_(0.75)
    bumped = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
    assert plan.pack_reuses == 2
    _same(bumped, fresh(), "after an MLP weight update that bumps the version")
    # invalidate_packs() alone, and a new workspace
    rm.render_rays(plan, ro, rd, tile_w=W, out={})
    assert plan.pack_reuses == 3
    plan.invalidate_packs()
    rm.render_rays(plan, ro, rd, tile_w=W, out={})
    assert plan.pack_reuses == 3
    plan._ws = None
    _same({k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}, bumped, "a new workspace")
    assert plan.pack_reuses == 3


def test_half_precision_copies_refreshed_in_place_pack_again(gpu, orc):
    from sanerf_hq_amd import raymarching as rm
    steps, W, rows = [8], 40, 24
    model = product_model(synthetic_params(steps, seed=41), steps, False, gpu)
    ro, rd = _rays(orc, gpu, W, rows)
    plan = rm.RenderPlan(model, steps, torch.float16, keep_packs=True)
    rm.render_rays(plan, ro, rd, tile_w=W, out={}); rm.render_rays(plan, ro, rd, tile_w=W, out={})
    assert plan.pack_reuses == 1
    with torch.no_grad():
        model.grid.embeddings.data.mul_(0.5)
    plan.refresh_tables()                               # copy_() into the plan's own fp16 tables moves THEIR version counters
    got = {k: v.clone() for k, v in rm.render_rays(plan, ro, rd, tile_w=W, out={}).items()}
    assert plan.pack_reuses == 1
    _same(got, {k: v.clone() for k, v in rm.render_rays(rm.RenderPlan(model, steps, torch.float16), ro, rd, tile_w=W, out={}).items()}, "refreshed copies")
