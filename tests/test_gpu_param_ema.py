"""GPU: optim.ParamEMA -- sn_ema_update_multi, the average of every tracked tensor in one launch with torch_ema's warm-up formed on the
device -- against torch_ema's statement evaluated on CPU copies (bit for bit, no tolerance), as a captured HIP graph, and through the
store / copy_to / restore / checkpoint plumbing the reference's trainer uses around an evaluation."""
import functools
import math

import pytest
import torch

from helpers import camera_rays, product_model, synthetic_params

pytestmark = pytest.mark.gpu

CYCLE = [1, 3, 4, 5, 0, 1000, 4095, 4096, 4097, 8191, 12289, 4096 * 33 + 3, 1 << 20]   # quad tails, chunk edges, an empty tensor, many chunks
T40 = 40                                                                                # two calls per update
PLANTED = 5                                                                             # the tensor (1000 elements) that carries the special values
SPECIAL = [float("nan"), float("inf"), float("-inf"), -0.0, 1e-42]


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN elements compare equal to themselves, -0.0 differs from 0.0)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


def plant(t, base):
    """The five special values at base .. base + 4 of a flat CPU tensor."""
    t[base:base + 5] = torch.tensor(SPECIAL)
    assert float(t[base + 4]) != 0.0, "the denormal survives on this CPU"


@functools.lru_cache(maxsize=None)
def start_tensors():
    """40 (parameter, shadow) starting values on the CPU, computed once; every test clones what it changes."""
    gen = torch.Generator().manual_seed(1234)
    sizes = [CYCLE[i % len(CYCLE)] for i in range(T40)]
    params = [torch.randn(n, generator=gen) for n in sizes]
    shadows = [torch.randn(n, generator=gen) for n in sizes]
    # special values in the shadow against ordinary parameters, in the parameter against ordinary shadows, and against each other:
    # shadow[100 + k] = SPECIAL[k] meets param[100 + k] = SPECIAL[(k + j) % 5] at 100 + 10 j
    for j in range(5):
        plant(shadows[PLANTED], 100 + 10 * j)
        params[PLANTED][100 + 10 * j:105 + 10 * j] = torch.tensor(SPECIAL[j:] + SPECIAL[:j])
    plant(shadows[PLANTED], 200)
    plant(params[PLANTED], 300)
    return sizes, params, shadows


def perturb(params, step):
    """The parameters move between updates (on the CPU, the device gets the same bits); the planted ones stay planted."""
    gen = torch.Generator().manual_seed(5000 + step)
    for p in params:
        p.add_(torch.randn(p.shape, generator=gen) * 0.05)
    plant(params[PLANTED], 300)
    params[PLANTED][200:205] = torch.tensor([0.0, 1e-42, -1e-42, 1e-38, -0.0])      # against the shadow's special values, denormal differences


def cpu_update(shadows, params, decay, n):
    """torch_ema's update, restated: returns the new count."""
    omd = 1.0 - decay
    if n is not None:
        n += 1
        omd = 1.0 - min(decay, (1 + n) / (10 + n))
    for s, p in zip(shadows, params):
        tmp = s - p
        tmp.mul_(omd)
        s.sub_(tmp)
    return n


def device_twin(gpu, params_cpu, shadows_cpu, decay, **kw):
    """A ParamEMA over device copies of params_cpu whose shadows hold shadows_cpu's bits."""
    from sanerf_hq_amd.optim import ParamEMA
    params = [torch.nn.Parameter(p.to(gpu)) for p in params_cpu]
    ema = ParamEMA(params, decay, **kw)
    assert all(same_bits(s, p) and (s.data_ptr() != p.data_ptr() or p.numel() == 0) for s, p in zip(ema.shadow_params, params)), "shadows are clones"
    for s, c in zip(ema.shadow_params, shadows_cpu):
        s.copy_(c)
    return params, ema


@pytest.mark.parametrize("case", ["decay_0.5_across_its_warm_up", "decay_0.95_loaded_at_168", "no_num_updates"])
def test_update_equals_the_torch_statement_bit_for_bit(gpu, case):
    """40 tensors (two calls per update), the parameters perturbed between updates, NaN, +inf, -inf, -0.0 and 1e-42 planted in one tensor's
    shadow and parameter.  After every update every shadow has the bit pattern of torch_ema's statement evaluated on CPU copies, the count
    matches and no parameter was written.  (The planted values make the statement PRODUCE NaNs, inf - inf: on an x86 host those are
    0xffc00000, and the kernel encodes them so -- as the hardware delivers them, 0x7fc00000, they were the only elements that differed:
    2 after the first update, 8 from the second on.)"""
    sizes, p0, s0 = start_tensors()
    pc, sc = [p.clone() for p in p0], [s.clone() for s in s0]
    if case == "decay_0.5_across_its_warm_up":
        decay, n, updates = 0.5, 0, 12                       # (1 + n) / (10 + n) reaches 0.5 at n = 8
        params, ema = device_twin(gpu, pc, sc, decay)
    elif case == "decay_0.95_loaded_at_168":
        decay, n, updates = 0.95, 168, 4                     # ... and 0.95 at n = 170
        params, ema = device_twin(gpu, pc, [torch.zeros_like(s) for s in sc], 0.3)
        ema.load_state_dict({"decay": decay, "num_updates": n, "shadow_params": sc, "collected_params": None})
        assert ema.decay == decay and ema.num_updates == n
        assert (1 + 169) / (10 + 169) < decay <= (1 + 170) / (10 + 170)
    else:
        decay, n, updates = 0.95, None, 3
        params, ema = device_twin(gpu, pc, sc, decay, use_num_updates=False)
        assert ema.num_updates is None and ema.state_dict()["num_updates"] is None
    assert all(same_bits(s, c) for s, c in zip(ema.shadow_params, sc))
    for step in range(updates):
        perturb(pc, step)
        with torch.no_grad():
            for p, c in zip(params, pc):
                p.copy_(c)
        versions = [p._version for p in params]
        before = [bits(p).clone() for p in params]
        ema.update()
        n = cpu_update(sc, pc, decay, n)
        assert ema.num_updates == n, f"{case}: count after update {step}"
        for i, (s, c) in enumerate(zip(ema.shadow_params, sc)):
            if not same_bits(s, c):
                diff = (bits(s.cpu()) != bits(c)).nonzero().flatten()
                k = int(diff[0])
                pytest.fail(f"{case}: update {step}, tensor {i} ({sizes[i]} elements): {diff.numel()} elements differ, first at {k}: "
                            f"device {float(s[k])!r} ({int(bits(s.cpu())[k]):#x}), CPU {float(c[k])!r} ({int(bits(c)[k]):#x})")
        assert [p._version for p in params] == versions, "update() writes no parameter"
        assert all(torch.equal(bits(p), b) for p, b in zip(params, before))
    planted = ema.shadow_params[PLANTED].cpu()
    assert torch.isnan(planted[100:103]).all() and torch.isnan(planted[300:303]).all(), "the planted values took part"
    assert 0.0 < float(planted[203]) < 1.17549435e-38, "... and a denormal result among them"
    assert int(ema._ticket) == 0, "every launch leaves the ticket at zero"
    assert not any(same_bits(s, c) for s, c in zip(ema.shadow_params, s0) if c.numel() > 16), "the updates moved the shadows"


def test_grid_stride_loop_and_tensor_walk_beyond_the_grid_cap(gpu):
    """More chunks than the grid has workgroups (the cap is 4096): every workgroup walks several chunks, across tensor boundaries."""
    from sanerf_hq_amd.optim import ParamEMA
    gen = torch.Generator().manual_seed(77)
    sizes = [4097, 4096 * (4096 + 37) + 2, 5, 4096 * 3]
    pc = [torch.randn(n, generator=gen) for n in sizes]
    params = [torch.nn.Parameter(p.to(gpu)) for p in pc]
    ema = ParamEMA(params, 0.95)
    sc = [p.clone() for p in pc]
    n = 0
    for step in range(2):
        for p, c in zip(params, pc):
            c.mul_(1.0 + 0.25 * (step + 1))
            p.data.copy_(c)
        ema.update()
        n = cpu_update(sc, pc, 0.95, n)
        assert all(same_bits(s, c) for s, c in zip(ema.shadow_params, sc)), f"update {step}"
    assert ema.num_updates == 2 and int(ema._ticket) == 0


@pytest.mark.parametrize("use_num_updates", [True, False], ids=["device_count", "constant_decay"])
def test_one_update_is_ceil_t_over_32_calls_and_only_the_last_advances(gpu, use_num_updates, monkeypatch):
    from sanerf_hq_amd import _lib
    from sanerf_hq_amd.optim import ParamEMA
    lib = _lib.lib()
    calls = []
    real = lib.sn_ema_update_multi

    def counted(recs, nt, decay, count, ticket, flags, stream):
        calls.append((nt, flags, count, ticket))
        return real(recs, nt, decay, count, ticket, flags, stream)
    monkeypatch.setattr(lib, "sn_ema_update_multi", counted)
    gen = torch.Generator(device=gpu).manual_seed(3)
    for T in (1, 13, 32, 33, 40, 70):
        params = [torch.nn.Parameter(torch.randn(CYCLE[(i * 5) % 11], generator=gen, device=gpu)) for i in range(T)]
        ema = ParamEMA(params, 0.95, use_num_updates=use_num_updates)
        for step in range(2):
            calls.clear()
            ema.update()
            assert len(calls) == math.ceil(T / _lib.EMA_MULTI_MAX_TENSORS), (T, calls)
            assert sum(nt for nt, _, _, _ in calls) == T and all(nt <= _lib.EMA_MULTI_MAX_TENSORS for nt, _, _, _ in calls)
            if use_num_updates:
                assert [f for _, f, _, _ in calls] == [0] * (len(calls) - 1) + [_lib.EMA_ADVANCE], "only the last call advances the count"
                assert all(c == ema._count.data_ptr() for _, _, c, _ in calls), "every call reads the one device count"
            else:
                assert all(f == 0 and c is None for _, f, c, _ in calls)
        assert ema.num_updates == (2 if use_num_updates else None) and int(ema._ticket) == 0


def _toy_step(gpu, seed):
    """A small training step of element-wise operators (the same kernels eagerly and under capture) with the average behind the optimiser."""
    from sanerf_hq_amd.optim import Adam, DeviceLRScale, ParamEMA
    gen = torch.Generator(device=gpu).manual_seed(seed)
    sizes = [4096 * 3 + 1, 1000, 3, 70000]
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, device=gpu)) for n in sizes]
    xs = [torch.randn(n, generator=gen, device=gpu) for n in sizes]
    opt = Adam([dict(params=params[:2], lr=1e-2), dict(params=params[2:], lr=3e-3, weight_decay=1e-3)], eps=1e-15, capturable=True, multi_tensor=True)
    sched = DeviceLRScale(opt, lambda it: 0.1 ** min(it / 5, 1))
    ema = ParamEMA(params, decay=0.5)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = sum(((p * x).sin() - 0.5 * x).pow(2).sum() for p, x in zip(params, xs))
        loss.backward()
        opt.step()
        ema.update()
        return loss.detach()
    return params, sched, ema, step


def test_captured_step_follows_the_warm_up_and_equals_the_eager_steps(gpu):
    """backward, opt.step(), ema.update() captured once by GraphedStep (warm-up 3) and replayed 12 times against 15 eager steps: shadows and
    count bit for bit.  decay = 0.5 leaves its warm-up at n = 8, in the middle of the replays: a decay formed on the host at capture time
    (n = 4) would be replayed for all twelve."""
    from sanerf_hq_amd.graph import GraphedStep
    warm, replays = 3, 12
    pe, se, ee, step_e = _toy_step(gpu, 21)
    for _ in range(warm):
        step_e()
    for _ in range(replays):
        step_e()
        se.step()
    pg, sg, eg, step_g = _toy_step(gpu, 21)
    g = GraphedStep(step_g, warmup=warm)
    assert eg.num_updates == warm, "the capture itself ran nothing and counted nothing"
    for _ in range(replays):
        g()
        sg.step()
    torch.cuda.synchronize()
    assert eg.num_updates == ee.num_updates == warm + replays
    for i, (a, b) in enumerate(zip(pe, pg)):
        assert same_bits(a, b), f"parameter {i}: the steps themselves differ"
    for i, (a, b) in enumerate(zip(ee.shadow_params, eg.shadow_params)):
        assert same_bits(a, b), f"shadow {i}: graph vs eager"
    assert int(eg._ticket) == 0 and int(ee._ticket) == 0
    assert not any(same_bits(s, p) for s, p in zip(eg.shadow_params, pg) if p.numel() > 16), "the average lags the parameters"


def test_store_copy_to_restore_move_bits_versions_and_call_on_write(gpu):
    from sanerf_hq_amd.optim import ParamEMA
    gen = torch.Generator(device=gpu).manual_seed(8)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, device=gpu)) for n in (1000, 3, 4097)]
    writes = []
    ema = ParamEMA(params, 0.5, on_write=lambda: writes.append(1))
    with torch.no_grad():
        for p in params:
            p.mul_(1.5)
    ema.update()
    raw = [p.detach().clone() for p in params]
    assert not any(same_bits(s, p) for s, p in zip(ema.shadow_params, params))
    with pytest.raises(RuntimeError, match="no `store\\(\\)`ed weights"):
        ema.restore()
    assert writes == []
    ema.store()
    assert writes == [] and all(same_bits(c, p) and c.data_ptr() != p.data_ptr() for c, p in zip(ema.collected_params, params))
    v0 = [p._version for p in params]
    ema.copy_to()
    assert all(same_bits(p, s) for p, s in zip(params, ema.shadow_params)), "the parameters take the shadows' bits"
    v1 = [p._version for p in params]
    assert all(b > a for a, b in zip(v0, v1)) and len(writes) == 1
    ema.restore()
    assert all(same_bits(p, r) for p, r in zip(params, raw)), "... and their own again"
    assert all(b > a for a, b in zip(v1, [p._version for p in params])) and len(writes) == 2
    assert all(p.requires_grad and p.is_leaf for p in params)
    # other tensors than the tracked ones: torch_ema's `parameters` argument
    others = [torch.zeros_like(p) for p in params]
    ema.copy_to(others)
    assert all(same_bits(o, s) for o, s in zip(others, ema.shadow_params)) and len(writes) == 3
    with pytest.raises(ValueError, match="different from number of shadow parameters"):
        ema.copy_to(others[:2])


def test_render_under_the_averaged_weights_with_static_half_tables(gpu, orc):
    """A reference-shaped model rendering from half-precision table copies that are NOT refreshed per call (render_tables_static): after
    store(); copy_to() with on_write=model.invalidate_render_plan the image is the one of a second model that was loaded with the shadow
    values; after restore() it is the first image again."""
    from sanerf_hq_amd.optim import ParamEMA
    steps = [64, 32]
    model = product_model(synthetic_params(steps, seed=11), steps, False, gpu)
    model.render_table_dtype, model.render_tables_static = torch.float16, True
    _, _, ro, rd = camera_rays(orc, 64, 64)
    ro_t, rd_t = torch.from_numpy(ro).to(gpu), torch.from_numpy(rd).to(gpu)
    names = [k for k, _ in model.named_parameters()]
    ema = ParamEMA(model.parameters(), 0.5, on_write=model.invalidate_render_plan)
    with torch.no_grad():
        model.render(ro_t, rd_t)                                          # the plan and its half-precision copies exist from here on
        for p in model.parameters():                                      # "training": the weights move away from their average
            p.mul_(0.75)
        ema.update()
        model.invalidate_render_plan()
        first = model.render(ro_t, rd_t)["image"].clone()
        ema.store()
        ema.copy_to()
        averaged = model.render(ro_t, rd_t)["image"].clone()
        second = product_model({k: s.cpu().numpy() for k, s in zip(names, ema.shadow_params)}, steps, False, gpu)
        second.render_table_dtype = torch.float16
        want = second.render(ro_t, rd_t)["image"]
        assert same_bits(averaged, want), "the render under copy_to() is not the render of the shadow values"
        assert not same_bits(averaged, first), "the averaged weights render another image"
        ema.restore()
        assert same_bits(model.render(ro_t, rd_t)["image"], first), "restore() brings the first image back"


def test_checkpoint_round_trip_continues_like_an_uninterrupted_twin(gpu, tmp_path):
    from sanerf_hq_amd.nerf.utils import save_checkpoint
    from sanerf_hq_amd.optim import ParamEMA
    torch.manual_seed(4)
    model = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 3)).to(gpu)
    params = list(model.parameters())
    ema = ParamEMA(params, 0.95)

    def train(step):
        with torch.no_grad():
            for p in params:
                p.mul_(1.0 + 0.1 * (step + 1))
    for step in range(3):
        train(step)
        ema.update()
    ema.store()
    path = str(tmp_path / "ngp_ep0001.pth")
    state = save_checkpoint(model, path, epoch=1, global_step=3, ema=ema)
    assert list(state["ema"]) == ["decay", "num_updates", "shadow_params", "collected_params"]
    assert state["ema"]["decay"] == 0.95 and state["ema"]["num_updates"] == 3 and type(state["ema"]["num_updates"]) is int
    loaded = torch.load(path, map_location="cpu", weights_only=False)["ema"]
    fresh = ParamEMA(params, 0.1)
    count, shadows = fresh._count, [s.data_ptr() for s in fresh.shadow_params]
    fresh.load_state_dict(loaded)
    assert fresh._count is count and [s.data_ptr() for s in fresh.shadow_params] == shadows, "loading copies into the existing device tensors"
    assert fresh.decay == 0.95 and fresh.num_updates == 3
    assert all(c.is_cuda and same_bits(c, d) for c, d in zip(fresh.collected_params, ema.collected_params))
    train(3)
    ema.update(); fresh.update()
    assert ema.num_updates == fresh.num_updates == 4
    assert all(same_bits(a, b) for a, b in zip(ema.shadow_params, fresh.shadow_params))
