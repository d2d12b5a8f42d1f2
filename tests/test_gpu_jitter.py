"""GPU: sn_rm_jitter_tables (csrc/jitter.hip) against the numpy restatement of its generator (tests/philox_ref.py) bit for bit, its
draw counter, chunk invariance, and the perturbed no-grad render that takes its tables through the fused renderer
(NeRFRenderer.fused_perturb): against render_rays on the same tables (bits), the CPU oracle, the operator chain on the same draw, the
feature heads, staging, and graph replay."""
import numpy as np
import pytest
import torch

import philox_ref as pr
from helpers import camera_rays, make_opt, oracle_cfg, product_model, synthetic_params

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4                          # tests/test_gpu_render.py: BASELINE.json north_star
SEED = 0x9E3779B97F4A7C15
DRAW = (1 << 32) - 1                    # the next draw carries into the high word
CANARY = -7.25


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_restated = {}


def restated(seed, draw, steps, ray_base, N, dev):
    """{k: table of stage k} as sn_rm_jitter makes it of the restated uniforms (computed once per case, shared, never written)."""
    from sanerf_hq_amd import raymarching as rm
    key = (seed, draw, tuple(steps), ray_base, N)
    if key not in _restated:
        _restated[key] = {k: rm.jitter(T(pr.table_uniforms(seed, draw, k, ray_base, N, t + 1), dev), N, t + 1, 0 if k == 0 else 1)
                          for k, t in enumerate(steps)}
    return _restated[key]


def guarded(N, steps, stages, pad, dev):
    """A buffer of canaries per stage with the [N, T+1] table as a view `pad` floats in (pad 8: 16-byte aligned; 7: not)."""
    bufs, views = {}, {}
    for k in stages:
        n = N * (steps[k] + 1)
        bufs[k] = torch.full((pad + n + 9,), CANARY, device=dev)
        views[k] = bufs[k][pad:pad + n].view(N, steps[k] + 1)
    return bufs, views


def canaries_intact(bufs, views, pad):
    return all(bool((b[:pad] == CANARY).all()) and bool((b[pad + views[k].numel():] == CANARY).all()) for k, b in bufs.items())


@pytest.mark.parametrize("ray_base", [0, 1000, (1 << 32) - 257])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_tables_are_bit_equal_to_the_restatement(gpu, N, ray_base):
    """Row lengths 4, 33, 6, 7: every remainder mod 4; aligned and unaligned tables; nothing written outside them; with u[2] = NULL and
    bins0 = NULL only the requested tables are written."""
    from sanerf_hq_amd import raymarching as rm
    steps = (3, 32, 5, 6)
    want = restated(SEED, DRAW, steps, ray_base, N, gpu)
    jit = rm.DeviceJitter(gpu, seed=SEED)
    for pad in (8, 7):
        jit.set(draw=DRAW)
        bufs, views = guarded(N, steps, range(4), pad, gpu)
        assert all(v.data_ptr() % 16 == (0 if pad == 8 else 12) for v in views.values())
        b0, u = rm.jitter_tables(jit.state, N, steps, ray_base=ray_base, advance=False, out=views)
        assert b0.data_ptr() == views[0].data_ptr() and sorted(u) == [1, 2, 3]
        for k in range(4):
            assert torch.equal(views[k], want[k]), (k, pad)
        assert canaries_intact(bufs, views, pad)
        # stages 1 and 3 only
        bufs, views = guarded(N, steps, range(4), pad, gpu)
        b0, u = rm.jitter_tables(jit.state, N, steps, ray_base=ray_base, advance=False, want=(1, 3), out=views)
        assert b0 is None and sorted(u) == [1, 3]
        assert torch.equal(u[1], want[1]) and torch.equal(u[3], want[3])
        assert bool((bufs[0] == CANARY).all()) and bool((bufs[2] == CANARY).all()) and canaries_intact(bufs, views, pad)
    b0, u = jit.tables(N, steps, ray_base=ray_base, advance=False)          # tables the operator allocates itself
    assert torch.equal(b0, want[0]) and all(torch.equal(u[k], want[k]) for k in (1, 2, 3))
    assert float(b0.min()) >= 0.0 and float(b0.max()) <= 1.0


def test_rows_longer_than_a_tile_are_written_in_pieces(gpu):
    """Rows above 1024 values leave the whole-row tiles: one piece of a single row (1101), two pieces (4501: 4096 + 405 values)."""
    from sanerf_hq_amd import raymarching as rm
    steps, N = (4500, 1100), 3
    want = restated(1234, 5, steps, 70, N, gpu)
    jit = rm.DeviceJitter(gpu, seed=1234).set(draw=5)
    for pad in (8, 7):
        bufs, views = guarded(N, steps, range(2), pad, gpu)
        rm.jitter_tables(jit.state, N, steps, ray_base=70, advance=False, out=views)
        assert torch.equal(views[0], want[0]) and torch.equal(views[1], want[1]) and canaries_intact(bufs, views, pad)


def test_state_and_draw_counter(gpu):
    from sanerf_hq_amd import raymarching as rm
    steps, N = (3, 32, 5, 6), 63
    jit = rm.DeviceJitter(gpu, seed=SEED).set(draw=DRAW)
    assert jit.state.dtype == torch.int64 and jit.state.shape == (4,) and jit.state.data_ptr() % 16 == 0
    jit.state[3] = 77                                                       # the reserved word is nobody's business
    before = jit.state.clone()
    a0, au = jit.tables(N, steps, advance=False)
    assert torch.equal(jit.state, before), "advance = 0 leaves all four words as they were"
    b0, bu = jit.tables(N, steps, advance=True)
    assert torch.equal(a0, b0) and all(torch.equal(au[k], bu[k]) for k in au), "the same (seed, draw) gives the same bits"
    assert jit.state_dict() == {"seed": SEED, "draw": 1 << 32}, "2^32 - 1 -> 2^32: the carry reaches the high word"
    assert jit.state.tolist()[2:] == [0, 77], "the ticket is 0 at rest"
    c0, cu = jit.tables(N, steps, advance=True)
    assert jit.state_dict()["draw"] == (1 << 32) + 1 and int(jit.state[2]) == 0
    # (stage-0 bins are clamped to [0, 1]: the two end columns of a row of four repeat 0 / 1 in a quarter of the rows, so 7/8 differ at best)
    assert float((c0 != b0).float().mean()) > 0.5 and all(float((cu[k] != bu[k]).float().mean()) > 0.9 for k in cu), "the next draw differs"
    want = restated(SEED, 1 << 32, steps, 0, N, gpu)
    assert torch.equal(c0, want[0]) and all(torch.equal(cu[k], want[k]) for k in cu)
    other = rm.DeviceJitter(gpu, seed=SEED + 1).set(draw=DRAW)
    d0, du = other.tables(N, steps)
    assert float((d0 != a0).float().mean()) > 0.5 and float((du[1] != au[1]).float().mean()) > 0.9, "another seed differs"
    # many workgroups, one advance per launch; .advance() draws no table; state_dict round trip
    jit.set(draw=10)
    jit.tables(5000, (128, 64, 32))
    assert jit.state_dict()["draw"] == 11 and int(jit.state[2]) == 0
    jit.advance()
    assert jit.state_dict() == {"seed": SEED, "draw": 12} and int(jit.state[2]) == 0
    other.load_state_dict(jit.state_dict())
    x0, xu = other.tables(N, steps, advance=False)
    y0, yu = jit.tables(N, steps, advance=False)
    assert torch.equal(x0, y0) and torch.equal(xu[3], yu[3])
    # seed=None: 64 bits of torch's default CPU generator
    torch.manual_seed(5)
    s1 = rm.DeviceJitter(gpu).state_dict()
    torch.manual_seed(5)
    s2 = rm.DeviceJitter(gpu).state_dict()
    assert s1 == s2 and s1["draw"] == 0 and s1["seed"] != rm.DeviceJitter(gpu).state_dict()["seed"]


def test_chunks_make_the_whole_table(gpu):
    """N = 257 at once = chunks of 100 + 157 with ray_base = 100 (the restatement's case), whatever the grid."""
    from sanerf_hq_amd import raymarching as rm
    steps = (3, 32, 5, 6)
    jit = rm.DeviceJitter(gpu, seed=99).set(draw=7)
    w0, wu = jit.tables(257, steps, advance=False)
    a0, au = jit.tables(100, steps, advance=False)
    b0, bu = jit.tables(157, steps, ray_base=100, advance=True)
    assert torch.equal(w0, torch.cat([a0, b0])) and all(torch.equal(wu[k], torch.cat([au[k], bu[k]])) for k in wu)
    assert jit.state_dict()["draw"] == 8
    for k in range(4):
        assert np.array_equal(pr.table_uniforms(99, 7, k, 0, 257, steps[k] + 1),
                              np.concatenate([pr.table_uniforms(99, 7, k, 0, 100, steps[k] + 1), pr.table_uniforms(99, 7, k, 100, 157, steps[k] + 1)]))


# ---- the perturbed render ---------------------------------------------------------------------------------------------------------
STEPS = [32, 16, 8]


@pytest.fixture(scope="module")
def scene(gpu, orc):
    params = synthetic_params(STEPS, seed=5)
    _, _, ro, rd = camera_rays(orc, 16, 16)
    return params, ro, rd, T(ro, gpu), T(rd, gpu)


def fresh_model(scene, gpu, seed=5, draw=0):
    from sanerf_hq_amd import raymarching as rm
    model = product_model(scene[0], STEPS, False, gpu)
    model.jitter = rm.DeviceJitter(gpu, seed=seed).set(draw=draw)
    return model


def test_perturbed_render_is_the_fused_render_on_the_device_tables(gpu, scene):
    """(a) bit-equal to render_rays fed with jitter_tables' output at the same (seed, draw), through a fused last-stage kernel;
    (d) perturb=3 (the viewer's spp) is perturb=True."""
    from sanerf_hq_amd import raymarching as rm
    _, _, _, ro, rd = scene
    model = fresh_model(scene, gpu, draw=3)
    with torch.no_grad():
        got = model.render(ro, rd, staged=False, perturb=True)
        info = rm.last_launch_info()
        assert info["final_kernel"].startswith("k_final_stage") and info["launches"] > 0, info
        assert set(got) == {"image", "depth", "weights_sum"} and model.jitter.state_dict() == {"seed": 5, "draw": 4}
        ref_state = rm.DeviceJitter(gpu, seed=5).set(draw=3)
        b0, u = rm.jitter_tables(ref_state.state, ro.shape[0], STEPS, advance=False)
        want = rm.render_rays(rm.RenderPlan(model, STEPS), ro, rd, bins0_table=b0, u_tables=u, out={})
        for k in ("image", "depth", "weights_sum"):
            assert torch.equal(got[k], want[k]), k
        plain = model.render(ro, rd, staged=False, perturb=False)
        assert float((plain["image"] - got["image"]).abs().max()) > 1e-4, "the jitter moves the image"
        model.jitter.set(draw=3)
        spp = model.render(ro, rd, staged=False, perturb=3)
        assert all(torch.equal(spp[k], got[k]) for k in got) and model.jitter.state_dict()["draw"] == 4


def test_perturbed_render_against_the_oracle_ray_by_ray(gpu, orc, scene):
    """(b) 64 rays, each rendered alone by the CPU oracle (whose tables are shared by the rays of a call) with its own restated rows."""
    from sanerf_hq_amd import raymarching as rm
    params, ro_np, rd_np, ro, rd = scene
    model = fresh_model(scene, gpu, draw=3)
    N = ro.shape[0]
    rows = {k: v.cpu().numpy() for k, v in restated(5, 3, STEPS, 0, N, gpu).items()}
    with torch.no_grad():
        got = model.render(ro, rd, staged=False, perturb=True)
        jit = rm.DeviceJitter(gpu, seed=5).set(draw=3)
        b0, u = jit.tables(N, STEPS)
        dbg = rm.render_rays(rm.RenderPlan(model, STEPS), ro, rd, bins0_table=b0, u_tables=u, want=("inds",), out={})
    assert torch.equal(dbg["image"], got["image"])
    image, inds = got["image"].cpu().numpy(), {k: dbg[f"inds{k}"].cpu().numpy() for k in (1, 2)}
    cfg = oracle_cfg(orc, params, STEPS)
    picks = np.arange(0, N, N // 64)[:64]
    mism = {1: 0, 2: 0}
    err = 0.0
    for i in picks:
        want = orc.render(cfg, ro_np[i:i + 1], rd_np[i:i + 1], debug=True, u_tables={k: rows[k][i] for k in (1, 2)}, bins0_table=rows[0][i])
        err = max(err, float(np.abs(image[i] - want["image"][0]).max()))
        for k in (1, 2):
            mism[k] += int((inds[k][i] != want[f"inds{k}"][0]).sum())
    print(f"64 rays vs oracle: max|dRGB| = {err:.2e}, index mismatches {mism}")
    assert err <= RGB_TOL
    assert mism[1] <= 2 and mism[2] <= 2, "only tie cases may differ (tests/test_gpu_render.py's allowance)"


def test_staged_perturbed_render_does_not_depend_on_the_chunking(gpu, scene):
    """(c) max_ray_batch = 100: three chunks, drawn with ray_base = head; the image equals the unstaged one from the same draw bit for bit,
    and an image costs exactly one draw."""
    _, _, _, ro, rd = scene
    model = fresh_model(scene, gpu, draw=20)
    with torch.no_grad():
        whole = model.render(ro, rd, staged=False, perturb=True)
        assert model.jitter.state_dict()["draw"] == 21
        model.jitter.set(draw=20)
        model.opt.max_ray_batch = 100
        parts = model.render(ro, rd, staged=True, perturb=True)
        assert model.jitter.state_dict()["draw"] == 21
        for k in ("image", "depth", "weights_sum"):
            assert torch.equal(whole[k], parts[k]), k
        again = model.render(ro, rd, staged=True, perturb=True)
        assert model.jitter.state_dict()["draw"] == 22 and not torch.equal(again["image"], parts["image"])


def test_operator_chain_on_the_same_draw_agrees(gpu, scene):
    """(e) fused_perturb = False sends the call down the parent's route; with model.jitter set it takes the same tables, and agrees with the
    fused image to the bound tests/test_gpu_render.py uses for fused against chain (2e-5: the proposal sigmas differ in the last bit)."""
    _, _, _, ro, rd = scene
    model = fresh_model(scene, gpu, draw=3)
    with torch.no_grad():
        fused = model.render(ro, rd, staged=False, perturb=True)["image"].clone()
        for unit in (True, False):                                         # the fused training operators, and the plain stage loop
            model.jitter.set(draw=3)
            model.fused_perturb, model.fused_training_ops = False, unit
            chain = model.render(ro, rd, staged=False, perturb=True)["image"]
            assert model.jitter.state_dict()["draw"] == 4
            d = float((fused - chain).abs().max())
            print(f"fused vs chain (fused_training_ops={unit}): {d:.2e}")
            assert d <= 2e-5


@pytest.mark.parametrize("mode", ["mask", "sam"])
def test_heads_on_the_perturbed_fused_render(gpu, mode):
    """(f) mask-mode model with return_mask=1, SAM-mode model with return_feats=1: fused-perturbed against the chain on the same draw,
    within the bounds tests/test_gpu_heads.py uses for the two routes at perturb=False."""
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf import NeRFNetwork
    steps = [48, 24, 16]
    kw = dict(with_mask=True) if mode == "mask" else dict(with_sam=True)
    model = NeRFNetwork(make_opt(num_steps=steps, **kw))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params(steps, heads=True, seed=77).items()}, strict=False)
    model = model.to(gpu).eval()
    model.jitter = rm.DeviceJitter(gpu, seed=11)
    H = W = 24
    ro, rd = rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(H, W), H, W, device=gpu)
    call = dict(staged=False, perturb=True, H=H, W=W, tile_w=W, **(dict(return_mask=1) if mode == "mask" else dict(return_feats=1)))
    with torch.no_grad():
        a = {k: v.clone() for k, v in model.render(ro, rd, **call).items() if torch.is_tensor(v)}
        assert rm.last_launch_info()["final_kernel"].startswith("k_final_stage")
        plain = model.render(ro, rd, **dict(call, perturb=False))
        model.jitter.set(draw=0)
        model.fused_perturb = False
        b = model.render(ro, rd, **call)
    keys = ("image", "depth") + (("instance_mask_logits",) if mode == "mask" else ("samvit",))
    for k, tol in (("image", 2e-5), ("depth", 1e-4), ("samvit", 1e-4), ("instance_mask_logits", 1e-4)):
        if k not in keys:
            continue
        assert torch.isfinite(a[k]).all(), k
        d = float((a[k].reshape(b[k].shape) - b[k]).abs().max())
        print(f"{mode} {k}: fused vs chain {d:.2e} (scale {float(b[k].abs().max()):.2e})")
        assert d <= tol * max(1.0, float(b[k].abs().max())), k
    assert float((a[keys[-1]].reshape(-1) - plain[keys[-1]].reshape(-1)).abs().max()) > 0, "the jitter reaches the head"


def test_other_backgrounds_and_packed_output(gpu, scene):
    """A tensor background and the packed [N, 5] output work as they do at perturb=False."""
    _, _, _, ro, rd = scene
    model = fresh_model(scene, gpu, draw=3)
    N = ro.shape[0]
    with torch.no_grad():
        base = model.render(ro, rd, staged=False, perturb=True, bg_color=0)
        model.jitter.set(draw=3)
        bg = torch.rand(N, 3, device=gpu)
        got = model.render(ro, rd, staged=False, perturb=True, bg_color=bg)
        assert torch.equal(got["image"], base["image"] + (1 - base["weights_sum"]).unsqueeze(-1) * bg)
        model.jitter.set(draw=3)
        packed = torch.zeros(N, 6, device=gpu)
        out = model.render(ro, rd, staged=False, perturb=True, bg_color=0, packed=packed)
        assert torch.equal(packed[:, :3], base["image"]) and torch.equal(packed[:, 3], base["depth"]) and torch.equal(out["weights_sum"], base["weights_sum"])


def test_without_a_jitter_of_the_callers(gpu, scene):
    """(g) jitter = None: the renderer makes its own state, seeded from torch's CPU generator -- finite, different from the unperturbed
    image, reproducible after torch.manual_seed when the model is rebuilt.  (h) the training routes do not look at that state: a
    training-mode call with gradients draws through torch.rand, same seed, same bits (tests/test_gpu_training.py)."""
    _, _, _, ro, rd = scene
    imgs = []
    for _ in range(2):
        torch.manual_seed(77)
        model = product_model(scene[0], STEPS, False, gpu)
        assert model.jitter is None
        with torch.no_grad():
            imgs.append(model.render(ro, rd, staged=False, perturb=True)["image"].clone())
            plain = model.render(ro, rd, staged=False, perturb=False)["image"]
        assert model.jitter is not None and model.jitter.state_dict()["draw"] == 1
    assert torch.isfinite(imgs[0]).all() and torch.equal(imgs[0], imgs[1]) and float((imgs[0] - plain).abs().max()) > 1e-4
    with torch.no_grad():
        assert not torch.equal(model.render(ro, rd, staged=False, perturb=True)["image"], imgs[0])     # the next draw

    def train_call(m):
        torch.manual_seed(123)
        m.zero_grad(set_to_none=True)
        o = m.render(ro, rd, staged=False, bg_color=1, perturb=True, update_proposal=True)
        o["image"].square().mean().backward()
        return o["image"].detach().clone(), m.grid_mlp.net[0].weight.grad.clone()

    fresh = product_model(scene[0], STEPS, False, gpu).train()
    a = train_call(fresh)
    assert fresh.jitter is None, "a training call makes no device jitter"
    b = train_call(fresh)
    model.train()                                                          # the model that made its own state above
    draw = model.jitter.state_dict()["draw"]
    c = train_call(model)
    assert model.jitter.state_dict()["draw"] == draw, "... and does not use one the renderer made itself"
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_training_route_takes_the_callers_jitter(gpu, scene):
    """model.jitter set by the caller: the autograd routes take their tables from one jitter.tables() call -- same (seed, draw), same image
    and gradients whatever torch's generators hold; each call costs one draw."""
    _, _, _, ro, rd = scene
    model = fresh_model(scene, gpu, draw=40).train()
    runs = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        model.jitter.set(draw=40)
        model.zero_grad(set_to_none=True)
        o = model.render(ro, rd, staged=False, bg_color=1, perturb=True, update_proposal=True)
        o["image"].square().mean().backward()
        assert model.jitter.state_dict()["draw"] == 41
        runs.append((o["image"].detach().clone(), model.grid_mlp.net[0].weight.grad.clone(), model.view_mlp.net[2].weight.grad.clone()))
    assert torch.isfinite(runs[0][0]).all() and all(torch.equal(x, y) for x, y in zip(*runs))
    model.jitter.set(draw=41)
    model.zero_grad(set_to_none=True)
    other = model.render(ro, rd, staged=False, bg_color=1, perturb=True, update_proposal=True)["image"]
    assert not torch.equal(other, runs[0][0]), "another draw, another image"


def test_captured_perturbed_render_draws_fresh_jitter_on_every_replay(gpu, scene):
    """The no-grad perturbed render in a GraphedStep: three replays, three images, the draw up by one each, and replay i equals the eager
    render with the draw set to that value."""
    from sanerf_hq_amd.graph import GraphedStep
    _, _, _, ro, rd = scene
    model = fresh_model(scene, gpu, draw=0)

    def step():
        with torch.no_grad():
            return model.render(ro, rd, staged=False, perturb=True)["image"]

    g = GraphedStep(step, warmup=2)
    model.jitter.set(draw=1000)
    replays = []
    for i in range(3):
        img = g()
        torch.cuda.synchronize()
        replays.append(img.clone())
        assert model.jitter.state_dict() == {"seed": 5, "draw": 1001 + i} and int(model.jitter.state[2]) == 0
    assert not torch.equal(replays[0], replays[1]) and not torch.equal(replays[1], replays[2]) and not torch.equal(replays[0], replays[2])
    for i in range(3):
        model.jitter.set(draw=1000 + i)
        assert torch.equal(step(), replays[i]), i
