"""GPU: optim.Adam(multi_tensor=True) -- sn_adam_step_multi, one launch for every parameter tensor -- against the per-tensor route (bit for
bit), against torch.optim.Adam under the reference's learning-rate schedule (optim.DeviceLRScale against LambdaLR), and as a captured
HIP graph that follows that schedule."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 1000, 4096 * 33 + 3, (1 << 19) * 32, 2048, 64 * 64, 4096, 4097, 8191, 16, 7, 64 * 32, 5, 4095, 12289, 64, 2, 32 * 16, 300]


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN elements compare equal to themselves)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def model_like(gpu, sizes, seed=0):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    return [torch.randn(n, generator=gen, device=gpu) for n in sizes]


def grouped(params, **kw):
    """Four groups over the tensors in turn: plain, weight decay, maximize, lazy -- each with a rate of its own."""
    from sanerf_hq_amd.optim import Adam
    spec = [dict(lr=1e-2), dict(lr=1e-3, weight_decay=1e-3), dict(lr=5e-3, maximize=True), dict(lr=2e-3, lazy=True, betas=(0.8, 0.99))]
    groups = [dict(params=params[k::len(spec)], **s) for k, s in enumerate(spec)]
    return Adam(groups, eps=1e-15, **kw)


def sparse_grads(gpu, sizes, seed):
    """The pattern of test_single_pass_adam_matches_torch_adam: a fifth of the elements touched per step, the first third never."""
    gen = torch.Generator(device=gpu).manual_seed(seed)
    out = []
    for n in sizes:
        g = torch.randn(n, generator=gen, device=gpu) * (torch.rand(n, generator=gen, device=gpu) < 0.2)
        g[: n // 3] = 0.0
        out.append(g)
    return out


def assert_same_state(oa, pa, ob, pb, what=""):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert same_bits(a, b), f"{what} parameter {i} ({a.numel()} elements)"
        sa, sb = oa.state[a], ob.state[b]
        assert len(sa) == len(sb), f"{what} state of parameter {i}"
        if len(sa):
            assert same_bits(sa["exp_avg"], sb["exp_avg"]) and same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), f"{what} moments of parameter {i}"
            assert float(sa["step"]) == float(sb["step"]), f"{what} step count of parameter {i}: {float(sa['step'])} vs {float(sb['step'])}"


@pytest.mark.parametrize("capturable", [False, True], ids=["host_counter", "capturable"])
def test_multi_tensor_route_equals_the_per_tensor_route_bit_for_bit(gpu, capturable):
    """20 tensors of 1 ... 2^19*32 elements in four groups (own rates; weight decay; maximize; lazy), six steps of sparse gradients with a NaN
    and an inf planted in one tensor, one tensor without a gradient in two of the steps: parameters, both moments (bit patterns) and step
    counts equal the per-tensor route's after every step."""
    p0 = model_like(gpu, SIZES)
    pa = [torch.nn.Parameter(p.clone()) for p in p0]
    pb = [torch.nn.Parameter(p.clone()) for p in p0]
    oa, ob = grouped(pa, capturable=capturable), grouped(pb, capturable=capturable, multi_tensor=True)
    idle, planted = 6, 3                                            # tensor 6 (64*64) skips steps 2 and 4; tensor 3 carries the non-finite elements
    for step in range(6):
        grads = sparse_grads(gpu, SIZES, 100 + step)
        grads[planted][SIZES[planted] - 5] = float("nan")
        grads[planted][SIZES[planted] - 9] = float("inf") if step % 2 else float("-inf")
        before = pb[idle].detach().clone()
        for a, b, g in zip(pa, pb, grads):
            a.grad, b.grad = g.clone(), g.clone()
        if step in (2, 4):
            pa[idle].grad = pb[idle].grad = None
        oa.step(); ob.step()
        assert_same_state(oa, pa, ob, pb, f"step {step}:")
        if step in (2, 4):
            assert same_bits(pb[idle], before), "a tensor without a gradient keeps its bits"
    for i, b in enumerate(pb):
        assert float(ob.state[b]["step"]) == (4 if i == idle else 6)
    assert torch.isnan(pb[planted][SIZES[planted] - 5]) and torch.isnan(pa[planted][SIZES[planted] - 5])
    assert not any(same_bits(b, p) for b, p in zip(pb, p0) if b.numel() > 16), "the steps moved the parameters"
    if capturable:
        assert int(ob._ticket) == 0, "every launch leaves the ticket at zero"
        assert all(ob.state[b]["step"].untyped_storage().data_ptr() == ob._counts.untyped_storage().data_ptr() for b in pb), "one shared buffer of counts"


@pytest.mark.parametrize("capturable", [False, True], ids=["host_counter", "capturable"])
def test_device_lr_scale_follows_lambda_lr_of_torch(gpu, capturable):
    """multi_tensor=True + DeviceLRScale against torch.optim.Adam(eps=1e-15, foreach=False) + LambdaLR(0.1 ** min(it / iters, 1)), the
    reference's schedule (main.py:298-303) with iters = 4, to the bars of test_single_pass_adam_matches_torch_adam: per step max|dp| <=
    2e-6 max|p|, moments within 1e-6 relative.  The same steps at the rate the first step ran with must MISS the bar (a captured step that
    froze its rate would)."""
    from sanerf_hq_amd.optim import Adam, DeviceLRScale
    iters = 4
    lam = lambda it: 0.1 ** min(it / iters, 1)                      # noqa: E731
    sizes = [4096 * 33 + 3, 1000, 3, 1 << 20]
    p0 = model_like(gpu, sizes, seed=5)
    split = lambda ps: [dict(params=ps[:2], lr=1e-2), dict(params=ps[2:], lr=3e-3)]          # noqa: E731
    pa, pb, pc = ([torch.nn.Parameter(p.clone()) for p in p0] for _ in range(3))
    oa = Adam(split(pa), eps=1e-15, multi_tensor=True, capturable=capturable)
    ob = torch.optim.Adam(split(pb), eps=1e-15, foreach=False)
    oc = Adam(split(pc), eps=1e-15, multi_tensor=True, capturable=capturable)                 # no scheduler: the rate of step 0 throughout
    sa, sb = DeviceLRScale(oa, lam), torch.optim.lr_scheduler.LambdaLR(ob, lam)
    worst_frozen = 0.0
    for step in range(6):
        grads = sparse_grads(gpu, sizes, 200 + step)
        for a, b, c, g in zip(pa, pb, pc, grads):
            a.grad, b.grad, c.grad = g.clone(), g.clone(), g.clone()
        oa.step(); ob.step(); oc.step()
        sa.step(); sb.step()
        assert sa.get_last_lr() == sb.get_last_lr()
        for i, (a, b, c) in enumerate(zip(pa, pb, pc)):
            scale = float(b.abs().max())
            err, frozen = float((a - b).abs().max()) / scale, float((c - b).abs().max()) / scale
            print(f"step {step} tensor {i}: max|dp| / max|p| = {err:.3e}; at a frozen rate {frozen:.3e}")
            assert err <= 2e-6, (step, i, err)
            worst_frozen = max(worst_frozen, frozen) if step == 5 else worst_frozen
    assert worst_frozen > 2e-6, f"a frozen rate must miss the bar after six steps: {worst_frozen:.3e}"
    for a, b in zip(pa, pb):
        assert float(oa.state[a]["step"]) == float(ob.state[b]["step"]) == 6
        for k in ("exp_avg", "exp_avg_sq"):
            assert float((oa.state[a][k] - ob.state[b][k]).abs().max()) <= 1e-6 * max(float(ob.state[b][k].abs().max()), 1e-30)


def _toy_step(gpu, seed, capturable):
    """A small training step (zero_grad, forward, loss, backward, opt.step()) of element-wise operators: the same kernels eagerly and
    under capture, so that the two can be compared bit for bit."""
    from sanerf_hq_amd.optim import Adam, DeviceLRScale
    gen = torch.Generator(device=gpu).manual_seed(seed)
    sizes = [4096 * 3 + 1, 1000, 3, 70000]
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, device=gpu)) for n in sizes]
    xs = [torch.randn(n, generator=gen, device=gpu) for n in sizes]
    opt = Adam([dict(params=params[:2], lr=1e-2), dict(params=params[2:], lr=3e-3, weight_decay=1e-3)], eps=1e-15, capturable=capturable, multi_tensor=True)
    sched = DeviceLRScale(opt, lambda it: 0.1 ** min(it / 5, 1))

    def step():
        opt.zero_grad(set_to_none=True)
        loss = sum(((p * x).sin() - 0.5 * x).pow(2).sum() for p, x in zip(params, xs))
        loss.backward()
        opt.step()
        return loss.detach()
    return params, opt, sched, step


def test_captured_step_follows_the_schedule_and_equals_the_eager_steps(gpu):
    """The step captured once with GraphedStep and replayed eight times, the scheduler stepped between replays, against the same steps run
    eagerly: parameters, moments and device step counts bit for bit, the ticket left at zero.  (Shape of the graph test in test_gpu_mask_losses.)"""
    from sanerf_hq_amd.graph import GraphedStep
    warm, replays = 2, 8
    pe, oe, se, step_e = _toy_step(gpu, 11, True)
    for _ in range(warm):
        step_e()
    losses_e = []
    for _ in range(replays):
        losses_e.append(float(step_e()))
        se.step()
    pg, og, sg, step_g = _toy_step(gpu, 11, True)
    g = GraphedStep(step_g, warmup=warm)
    losses_g = []
    for _ in range(replays):
        losses_g.append(float(g()))
        sg.step()
    torch.cuda.synchronize()
    print("eager", losses_e, "graph", losses_g)
    assert all(np.isfinite(losses_g)) and np.allclose(losses_e, losses_g, rtol=1e-5)
    assert se.get_last_lr() == sg.get_last_lr() and sg.get_last_lr()[0] == 1e-2 * 0.1
    assert_same_state(oe, pe, og, pg, "graph vs eager:")
    for p in pg:
        assert float(og.state[p]["step"]) == warm + replays and og.state[p]["step"].is_cuda
    assert int(og._ticket) == 0 and int(oe._ticket) == 0
    # ... and the schedule was followed: eight more steps at the captured rate end elsewhere
    pf, of, _, step_f = _toy_step(gpu, 11, True)
    for _ in range(warm + replays):
        step_f()
    assert not any(same_bits(a, b) for a, b in zip(pf[:2], pg[:2])), "a frozen rate gives other parameters"


@pytest.mark.parametrize("capturable", [False, True], ids=["host_counter", "capturable"])
def test_one_step_is_ceil_t_over_max_calls_of_the_multi_entry_and_none_of_the_per_tensor_entry(gpu, capturable, monkeypatch):
    from sanerf_hq_amd import _lib
    lib = _lib.lib()
    calls = {"multi": [], "single": 0}
    multi, single = lib.sn_adam_step_multi, lib.sn_adam_step

    def count_multi(t, nt, g, ng, *rest):
        calls["multi"].append((nt, ng))
        return multi(t, nt, g, ng, *rest)

    def count_single(*args):
        calls["single"] += 1
        return single(*args)
    monkeypatch.setattr(lib, "sn_adam_step_multi", count_multi)
    monkeypatch.setattr(lib, "sn_adam_step", count_single)
    for T in (13, 20, 70):                                          # 70: more tensors than one call takes
        sizes = [SIZES[(i * 7) % len(SIZES)] if SIZES[(i * 7) % len(SIZES)] < (1 << 20) else 33 + i for i in range(T)]
        p0 = model_like(gpu, sizes, seed=T)
        pa = [torch.nn.Parameter(p.clone()) for p in p0]
        pb = [torch.nn.Parameter(p.clone()) for p in p0]
        oa, ob = grouped(pa, capturable=capturable), grouped(pb, capturable=capturable, multi_tensor=True)
        for step in range(3):
            grads = sparse_grads(gpu, sizes, 300 + step)
            for a, b, g in zip(pa, pb, grads):
                a.grad, b.grad = g.clone(), g.clone()
            calls["multi"], calls["single"] = [], 0
            ob.step()
            assert calls["single"] == 0 and len(calls["multi"]) == math.ceil(T / _lib.ADAM_MULTI_MAX_TENSORS), (T, calls)
            assert sum(nt for nt, _ in calls["multi"]) == T and all(ng <= _lib.ADAM_MULTI_MAX_GROUPS for _, ng in calls["multi"])
            oa.step()
            assert calls["single"] == T
            assert_same_state(oa, pa, ob, pb, f"{T} tensors, step {step}:")


def test_version_counters_checks_and_state_dict_interchange(gpu):
    """What tests/test_gpu_final_stage.py asks of the per-tensor route (version counters move on every written tensor), the refusals of
    today, and a state_dict written by either route loading into the other and into torch.optim.Adam."""
    from sanerf_hq_amd.optim import Adam
    sizes = [1000, 3, 4097]
    p0 = model_like(gpu, sizes, seed=9)
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = Adam(ps, lr=1e-2, eps=1e-15, multi_tensor=True)
    for p, g in zip(ps, sparse_grads(gpu, sizes, 1)):
        p.grad = g
    ps[1].grad = None
    v0 = [p._version for p in ps]
    opt.step()
    assert ps[0]._version > v0[0] and ps[2]._version > v0[2] and ps[1]._version == v0[1]
    assert len(opt.state[ps[1]]) == 0
    # refusals
    bad = torch.nn.Parameter(torch.zeros(8, 8, device=gpu).t()[:, :4])
    bad.grad = torch.ones_like(bad)
    with pytest.raises(RuntimeError, match="dense contiguous fp32 CUDA parameters only"):
        Adam([bad], lr=1e-3, multi_tensor=True).step()
    half = torch.nn.Parameter(torch.zeros(8, device=gpu, dtype=torch.float16))
    half.grad = torch.ones_like(half)
    with pytest.raises(RuntimeError, match="dense contiguous fp32 CUDA parameters only"):
        Adam([half], lr=1e-3, multi_tensor=True).step()
    lazy = torch.nn.Parameter(torch.zeros(8, device=gpu))
    lazy.grad = torch.ones_like(lazy)
    with pytest.raises(RuntimeError, match="lazy mode"):
        Adam([dict(params=[lazy], lazy=True)], lr=1e-3, weight_decay=1e-3, multi_tensor=True).step()
    # three steps on one route, the state moved to the other, three more: equal to six steps on either (all four pairings, both counters)
    for capturable in (False, True):
        runs = {}
        for first, second in ((False, False), (False, True), (True, False), (True, True)):
            qs = [torch.nn.Parameter(p.clone()) for p in p0]
            o1 = Adam(qs, lr=1e-2, eps=1e-15, capturable=capturable, multi_tensor=first)
            o2 = Adam(qs, lr=1e-2, eps=1e-15, capturable=capturable, multi_tensor=second)
            for step in range(6):
                for q, g in zip(qs, sparse_grads(gpu, sizes, 400 + step)):
                    q.grad = g
                if step == 3:
                    sd = o1.state_dict()
                    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
                    o2.load_state_dict(sd)
                    torch.optim.Adam(qs, lr=1e-2, eps=1e-15, capturable=capturable).load_state_dict(sd)
                (o1 if step < 3 else o2).step()
            assert all(float(o2.state[q]["step"]) == 6 for q in qs)
            runs[(first, second)] = [q.detach().clone() for q in qs]
        for key, got in runs.items():
            assert all(same_bits(a, b) for a, b in zip(got, runs[(False, False)])), (capturable, key)
