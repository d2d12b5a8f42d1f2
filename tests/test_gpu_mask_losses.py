"""GPU: the object-field training extras as HIP operators (ray_pair_select, ray_pair_rgb_loss, mask_error, error_map_update) and their
assembly nerf.mask_step.mask_train_loss, against tests/golden/mask_losses.npz (the reference's own functions on the CPU) and against the
reference's torch lines (nerf/trainer.py:260-305, 419-464, 1426-1432) restated here."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, make_opt, synthetic_params

pytestmark = pytest.mark.gpu

CASES = ("script_k2", "script_k3", "defaults", "odd_p")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def torch_pair_loss(rgb, inst_masks, sample_index, thr, w, eps, use_pred):
    """trainer.py:279-303 for given indices; a slot of -1 is no pair (the mean runs over the others)."""
    valid = sample_index >= 0
    idx = sample_index.clamp(min=0)
    col = torch.arange(rgb.shape[0], device=rgb.device)[:, None]
    rgb_sample = rgb[col, idx][..., None, :]
    sample_mask = inst_masks[col, idx][..., None, :].detach()
    if not use_pred:
        arg = torch.argmax(sample_mask, -1)
        sample_mask = torch.zeros_like(sample_mask).scatter_(-1, arg[..., None], 1)
    sim = torch.norm(rgb[:, None] - rgb_sample, dim=-1) < thr
    e = torch.exp(-w * F.cosine_similarity(inst_masks[:, None], sample_mask, dim=-1) - eps)
    pair = (sim * e).sum(-1) / sim.sum(-1)
    return (pair * valid).sum() / valid.sum().clamp(min=1), sim


def torch_mask_error(probs, labels, w, eps):
    """trainer.py:457-461"""
    onehot = torch.zeros_like(probs).scatter_(-1, labels[..., None], 1)
    return torch.exp(-w * F.cosine_similarity(probs, onehot, dim=-1) - eps)


def grad_close(got, ref, what):
    d = float((got - ref).abs().max())
    bar = 1e-5 * float(ref.abs().max())
    print(f"{what}: max|diff| {d:.3e}  bar {bar:.3e}")
    assert d <= bar, (what, d, bar)


@pytest.mark.parametrize("use_pred", [False, True])
@pytest.mark.parametrize("from_logits", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_ray_pair_rgb_loss_equals_the_reference_fixture(gpu, case, from_logits, use_pred):
    """Value rtol 1e-5, gradient max|diff| <= 1e-5 max|grad_ref| against the reference's CPU autograd, on its recorded multinomial draw."""
    from sanerf_hq_amd import raymarching as rm
    g = golden("mask_losses")
    name = "pred" if use_pred else "onehot"
    x = T(g[case + (".logits" if from_logits else ".probs")], gpu).requires_grad_(True)
    rgb = T(g[case + ".rgb"], gpu).requires_grad_(True)
    loss = rm.ray_pair_rgb_loss(rgb, x, T(g[case + ".sample_index"], gpu), float(g["thr"]), float(g["exp_weight"]), float(g["epsilon"]),
                                use_pred_logistics=use_pred, from_logits=from_logits)
    (loss * 3.0).backward()
    want = float(g[f"{case}.loss_{name}"])
    print(f"{case} {name} from_logits={from_logits}: loss {loss.item():.8f} reference {want:.8f} rel {abs(loss.item() - want) / want:.2e}")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    assert rgb.grad is None
    grad_close(x.grad.cpu() / 3.0, torch.from_numpy(g[f"{case}.grad_{'logits' if from_logits else 'probs'}_{name}"]), f"{case} {name} grad")


@pytest.mark.parametrize("G,P,S,K", [(1, 64, 1, 2), (5, 200, 7, 5), (3, 1000, 64, 32), (130, 64, 8, 3), (2, 37, 40, 9)])
def test_ray_pair_rgb_loss_equals_the_trainers_torch_lines(gpu, G, P, S, K):
    """Other sizes, random inputs whose colours are quantised to a 0.25 grid (distances 0, 0.25, 0.354, ... : none near thr = 0.3) and
    whose sampled pixels get a clear top class; groups with fewer than S candidates leave -1 slots; two runs give equal bits."""
    from sanerf_hq_amd import raymarching as rm
    torch.manual_seed(G * 1000 + P + S + K)
    thr, w, eps = 0.3, 10.0, 1e-6
    rgb = (torch.randint(0, 3, (G, P, 3), device=gpu).float() * 0.25 + 0.1)
    logits = torch.randn(G, P, K, device=gpu) * 2.0
    inc = torch.rand(G, P, device=gpu) * 0.5
    inc[0, :3] = 0.0
    inc[0, min(P, 3):] = 1.0                                     # group 0 has 3 candidates (or P)
    uni = torch.rand(G, P, device=gpu)
    idx = rm.ray_pair_select(inc, S, uni)
    assert (idx[0] >= 0).sum().item() == min(3, P, S) and (S <= 3 or idx[0, 3:].eq(-1).all())
    col = torch.arange(G, device=gpu)[:, None]
    logits[col, idx.clamp(min=0), 0] += 6.0                      # argmax margin of the sampled pixels
    for use_pred in (False, True):
        for from_logits in (False, True):
            lg = logits.clone().requires_grad_(True)
            probs = torch.softmax(lg, dim=-1)
            ref, sim = torch_pair_loss(rgb, probs, idx, thr, w, eps, use_pred)
            x = lg if from_logits else probs.detach().clone().requires_grad_(True)
            if not from_logits:
                probs.retain_grad()
            ref.backward()
            gref = lg.grad if from_logits else probs.grad
            x2 = x.detach().clone().requires_grad_(True)
            got = rm.ray_pair_rgb_loss(rgb, x2, idx, thr, w, eps, use_pred_logistics=use_pred, from_logits=from_logits)
            got.backward()
            print(f"G{G} P{P} S{S} K{K} pred={use_pred} logits={from_logits}: loss {got.item():.8f} torch {ref.item():.8f}")
            assert abs(got.item() - ref.item()) <= 1e-5 * abs(ref.item())
            grad_close(x2.grad, gref, "grad")
            x3 = x.detach().clone().requires_grad_(True)
            again = rm.ray_pair_rgb_loss(rgb, x3, idx, thr, w, eps, use_pred_logistics=use_pred, from_logits=from_logits)
            again.backward()
            assert torch.equal(again, got) and torch.equal(x3.grad, x2.grad), "two runs must give the same bits"
    assert 0 < sim.float().mean().item() < 1
    # no pair at all: zero loss, zero gradient (written, not left as it was)
    x4 = logits.clone().requires_grad_(True)
    none = rm.ray_pair_rgb_loss(rgb, x4, torch.full_like(idx, -1), thr, w, eps, from_logits=True)
    none.backward()
    assert none.item() == 0.0 and not x4.grad.any()


def test_ray_pair_select_is_the_argsort_of_the_masked_uniforms(gpu):
    from sanerf_hq_amd import raymarching as rm
    torch.manual_seed(5)
    for G, P, S in ((4, 64, 8), (2, 256, 1), (7, 100, 64), (300, 64, 8), (1, 5000, 33)):
        inc = torch.rand(G, P, device=gpu)
        inc[0] = 1.0                                             # all incoherent: falls back to every pixel
        if G > 1:
            inc[1] = 1.0
            inc[1, : min(P, 5)] = 0.0                            # 5 candidates
        uni = torch.rand(G, P, device=gpu)
        uni[:, : P // 2] = (uni[:, : P // 2] * 8).floor() / 8     # ties: the lower index first
        cand = (1.0 - inc) > 0.8
        cand[cand.sum(-1) == 0] = True
        order = torch.argsort(torch.where(cand, uni, torch.full_like(uni, float("inf"))), dim=-1, stable=True)[:, :S]
        want = torch.where(torch.arange(S, device=gpu)[None] < cand.sum(-1, keepdim=True), order, torch.full_like(order, -1))
        got = rm.ray_pair_select(inc, S, uni)
        assert got.dtype == torch.int64 and torch.equal(got, want), (G, P, S)
        assert torch.equal(rm.ray_pair_select(inc[..., None], S, uni), got)
        for row, c in zip(got.tolist(), cand.tolist()):
            sel = [i for i in row if i >= 0]
            assert len(set(sel)) == len(sel) and all(c[i] for i in sel)
        drawn = rm.ray_pair_select(inc, S)                       # its own torch.rand
        assert ((drawn >= 0) == (want >= 0)).all() and torch.gather(cand, 1, drawn.clamp(min=0))[drawn >= 0].all()


def test_mask_error_and_error_map_update(gpu):
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import build_error_map
    g = golden("mask_losses")
    w, eps = float(g["exp_weight"]), float(g["epsilon"])
    labels = T(g["ema_labels"], gpu)
    for from_logits, key in ((True, "ema_logits"), (False, "ema_probs")):
        err = rm.mask_error(T(g[key], gpu), labels, w, eps, from_logits=from_logits)
        np.testing.assert_allclose(err.cpu().numpy(), g["ema_error"], rtol=1e-5)
        emap = T(g["ema_map_before"], gpu)
        err2 = rm.error_map_update(emap, T(g["ema_index"], gpu), T(g["ema_inds"], gpu), T(g[key], gpu), labels, w, eps, from_logits=from_logits)
        assert torch.equal(err2, err)
        np.testing.assert_allclose(emap.cpu().numpy(), g["ema_map_after"], rtol=1e-5)
        untouched = np.ones(g["ema_map_before"].shape, dtype=bool)
        untouched[g["ema_index"], g["ema_inds"]] = False
        assert np.array_equal(emap.cpu().numpy()[untouched], g["ema_map_before"][untouched]), "untouched entries keep their bits"
    # the whole-map rebuild (trainer.py:1414-1434)
    opt = types.SimpleNamespace(error_map_size=int(g["rebuild_size"]), ray_pair_rgb_exp_weight=w, epsilon=eps)
    rebuilt = build_error_map(T(g["rebuild_probs"], gpu), T(g["rebuild_gt_masks"], gpu), opt)
    np.testing.assert_allclose(rebuilt.cpu().numpy(), g["rebuild_error_map"], rtol=1e-5)
    # torch lines on other sizes: one image for all rays, labels outside 0..K-1 (the zero vector), duplicate targets, targets outside the map
    torch.manual_seed(9)
    for N, K in ((1, 1), (777, 5), (5000, 32)):
        logits = torch.randn(N, K, device=gpu) * 3
        lab = torch.randint(0, K, (N,), device=gpu)
        probs = torch.softmax(logits, -1)
        ref = torch_mask_error(probs, lab, w, eps)
        np.testing.assert_allclose(rm.mask_error(logits, lab, w, eps, from_logits=True).cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)
        lab_bad = lab.clone(); lab_bad[::3] = -1; lab_bad[1::7] = K
        bad = rm.mask_error(probs, lab_bad, w, eps)
        expect = torch.where((lab_bad >= 0) & (lab_bad < K), ref, torch.exp(torch.tensor(-eps, device=gpu)))
        np.testing.assert_allclose(bad.cpu().numpy(), expect.cpu().numpy(), rtol=1e-5)
        cells = 4096
        before = torch.rand(3, cells, device=gpu)
        inds = torch.randint(0, 64, (N,), device=gpu) if N > 64 else torch.arange(N, device=gpu)      # many duplicates
        emap = before.clone()
        rm.error_map_update(emap, torch.tensor([1], device=gpu), inds, probs, lab, w, eps)
        cand = 0.1 * before[1, inds] + 0.9 * ref                  # each ray's value from the OLD entry; one of a target's rays stays
        hit = torch.zeros(cells, dtype=torch.bool, device=gpu); hit[inds] = True
        for c in torch.nonzero(hit).reshape(-1).tolist()[:64]:
            vals = cand[inds == c]
            assert ((vals - emap[1, c]).abs() <= 1e-5 * vals.abs()).any(), c
        assert torch.equal(emap[1][~hit], before[1][~hit]) and torch.equal(emap[0], before[0]) and torch.equal(emap[2], before[2])
        # targets outside the map are skipped and nothing else moves: distinct columns, so every written value is one ray's and the whole
        # map can be compared, bit for bit, with an update made without the offending rays
        n2 = min(N, cells)
        outside = torch.randperm(cells, device=gpu)[:n2]
        emap2 = before.clone()
        if n2 == 1:
            rm.error_map_update(emap2, torch.tensor([7], device=gpu), outside, probs, lab, w, eps)                # a row outside the map
            assert torch.equal(emap2, before)
        else:
            good = outside[1:-1].clone()
            outside[0] = cells; outside[-1] = -1
            rm.error_map_update(emap2, torch.tensor([2], device=gpu), outside, probs[:n2], lab[:n2], w, eps)
            emap3 = before.clone()
            rm.error_map_update(emap3, torch.tensor([2], device=gpu), good, probs[1:n2 - 1], lab[1:n2 - 1], w, eps)
            assert torch.equal(emap2, emap3) and not torch.equal(emap3[2], before[2])
            rows = torch.full((n2,), 2, device=gpu); rows[3] = 3; rows[4] = -1                                   # per-ray rows, two outside
            emap4 = before.clone()
            rm.error_map_update(emap4, rows[1:-1], good, probs[1:n2 - 1], lab[1:n2 - 1], w, eps)
            keep = torch.ones(n2 - 2, dtype=torch.bool, device=gpu); keep[2] = False; keep[3] = False
            emap5 = before.clone()
            rm.error_map_update(emap5, torch.tensor([2], device=gpu), good[keep], probs[1:n2 - 1][keep], lab[1:n2 - 1][keep], w, eps)
            assert torch.equal(emap4, emap5)


def _mask_step_setup(gpu, capturable, seed=99):
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf import NeRFNetwork
    from sanerf_hq_amd.optim import Adam
    params = synthetic_params([128, 64, 32], heads=True, seed=1)
    opt = make_opt(with_sam=False, with_mask=True)
    nr, G, ps = 1024, 4, 8
    for k, v in dict(num_rays=nr, ray_pair_rgb_loss_weight=1.0, ray_pair_rgb_num_sample=8, mixed_sampling=True, num_local_sample=G,
                     local_sample_patch_size=ps, ray_pair_rgb_threshold=0.3, ray_pair_rgb_exp_weight=10.0, ray_pair_rgb_iter=-1,
                     ray_pair_rgb_use_pred_logistics=False, label_regularization_weight=0, epsilon=1e-6).items():
        setattr(opt, k, v)
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    model = model.to(gpu).train()
    for n_, p in model.named_parameters():
        p.requires_grad_(n_.startswith("m_grid") or n_.startswith("mask_mlp"))
    H = W = 128
    N = nr + G * ps * ps
    roF, rdF = rm.generate_rays(synth.orbit_pose(1.1, 25.0, 60.0), synth.pinhole_intrinsics(H, W), H, W, device=gpu)
    pix = (synth.hash_u01(nr, seed) * (H * W)).astype(np.int64)
    corner = (synth.hash_u01(2 * G, seed + 5) * (H - ps)).astype(np.int64).reshape(G, 2)
    dy, dx = np.meshgrid(np.arange(ps), np.arange(ps), indexing="ij")
    patch = ((corner[:, 0, None, None] + dy) * W + corner[:, 1, None, None] + dx).reshape(-1)
    pix = torch.from_numpy(np.concatenate([pix, patch])).to(gpu)
    cells, M = 16 * 16, 6
    perm = np.argsort(synth.hash_u01(M * cells, seed + 2))[:nr]                 # distinct (index, inds) targets
    data = dict(masks=torch.from_numpy((synth.hash_u01(N, seed + 1) < 0.5).astype(np.int64)).to(gpu)[:, None],
                index=torch.from_numpy(perm // cells).to(gpu), inds_coarse=torch.from_numpy(perm % cells).to(gpu),
                error_maps=torch.from_numpy(synth.hash_u01(N, seed + 3).astype(np.float32) * 0.5).to(gpu))
    error_map = torch.from_numpy(synth.hash_u01(M * cells, seed + 4).astype(np.float32).reshape(M, cells)).to(gpu)
    uniform = torch.from_numpy(synth.hash_u01(G * ps * ps, seed + 6).astype(np.float32).reshape(G, ps * ps)).to(gpu)
    adam = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, eps=1e-8, capturable=capturable)

    def render():
        o = model.render(roF[pix].contiguous(), rdF[pix].contiguous(), staged=False, bg_color=1, perturb=False, update_proposal=False, return_mask=1)
        assert o["image"].shape == (N, 3), "the mask-mode route must return the colours of all rays"
        o = dict(o)
        o["image"] = (o["image"].detach() * 4).round() / 4      # colour distances 0, 0.25, ...: none within round-off of the threshold 0.3
        return o
    return model, opt, data, error_map, uniform, adam, render


def test_mask_train_loss_equals_the_torch_line_assembly_and_replays_as_a_graph(gpu):
    """mask_train_loss (HIP operators) against trainer.py:412-505 in torch ops on the same render: loss, error map, and every m_grid /
    mask_mlp gradient to the bars of the train_c5 fixture's test (relative L2 1e-3, max 1e-2 of the tensor's max); then the whole step
    (render, loss, backward, Adam) captured once and replayed: parameters, loss and error map equal the eager run's."""
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.graph import GraphedStep
    from sanerf_hq_amd.nerf import mask_train_loss
    model, opt, data, error_map, uniform, _, render = _mask_step_setup(gpu, False)
    nr, G, P, w, eps = opt.num_rays, opt.num_local_sample, opt.local_sample_patch_size ** 2, opt.ray_pair_rgb_exp_weight, opt.epsilon

    # the reference's lines
    o = render()
    gt = data["masks"].reshape(-1)
    inst = torch.softmax(o["instance_mask_logits"], dim=-1)
    pm = torch.clamp(inst, min=eps, max=1 - eps)
    ref_loss = (-torch.log(torch.gather(pm[:nr], -1, gt[:nr, None]))).mean()
    ref_map = error_map.clone()
    err = torch_mask_error(inst[:nr].detach(), gt[:nr], w, eps)
    ref_map[data["index"], data["inds_coarse"]] = 0.1 * ref_map[data["index"], data["inds_coarse"]] + 0.9 * err
    idx = rm.ray_pair_select(data["error_maps"][nr:].view(G, P), opt.ray_pair_rgb_num_sample, uniform)
    assert (idx >= 0).all()
    pair, sim = torch_pair_loss(o["image"][nr:].view(G, P, 3), inst[nr:].view(G, P, -1), idx, opt.ray_pair_rgb_threshold, w, eps, False)
    top = torch.sort(inst[nr:].view(G, P, -1)[torch.arange(G, device=gpu)[:, None], idx], dim=-1).values
    print(f"pair term {pair.item():.6f}, nll {ref_loss.item():.6f}, matches {sim.float().mean().item():.3f}, "
          f"top-2 margin of the sampled pixels {(top[..., -1] - top[..., -2]).min().item():.2e}")
    ref_loss = ref_loss + pair * opt.ray_pair_rgb_loss_weight
    ref_loss.backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}
    model.zero_grad(set_to_none=True)

    # the operators
    o = render()
    got_map = error_map.clone()
    pred, gt_mask, loss = mask_train_loss(o, data, opt, global_step=1, error_map=got_map, uniform=uniform)
    loss.backward()
    assert torch.equal(pred, inst.argmax(-1)) and torch.equal(gt_mask, data["masks"])
    print(f"loss {loss.item():.8f} torch lines {ref_loss.item():.8f}")
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * max(1.0, abs(ref_loss.item()))
    np.testing.assert_allclose(got_map.cpu().numpy(), ref_map.cpu().numpy(), rtol=1e-5)
    for n, p in model.named_parameters():
        if p.requires_grad:
            a, b = p.grad.double(), ref_grads[n].double()
            rel, mx = float((a - b).norm() / b.norm()), float((a - b).abs().max() / b.abs().max())
            print(f"{n}: relative L2 {rel:.2e}, max/max {mx:.2e}")
            assert rel < 1e-3 and mx < 1e-2, (n, rel, mx)
    assert model.grid.embeddings.grad is None
    # before ray_pair_rgb_iter the term is off; without mixed sampling all rays form one group
    opt.ray_pair_rgb_iter = 5
    _, _, plain = mask_train_loss(render(), data, opt, global_step=5)
    assert abs(plain.item() - (ref_loss - pair).item()) <= 1e-5
    opt.ray_pair_rgb_iter, opt.mixed_sampling = -1, False
    _, _, whole = mask_train_loss(render(), data, opt, global_step=1)
    assert np.isfinite(whole.item()) and whole.item() > plain.item()
    opt.mixed_sampling = True
    # mixed sampling without the rays' error-map values (collate_rays without an error map): a clear error, no None.reshape
    with pytest.raises(RuntimeError, match="error_maps"):
        mask_train_loss(render(), {**data, "error_maps": None}, opt, global_step=1)
    # no labelled ray at all (trainer.py:427-432): loss 0 and zero gradients, selected on the device
    opt.ray_pair_rgb_loss_weight = 0.0
    model.zero_grad(set_to_none=True)
    _, _, empty = mask_train_loss(render(), {**data, "masks": torch.full_like(data["masks"], -1)}, opt, global_step=1)
    empty.backward()
    assert empty.item() == 0.0
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())
    # some unlabelled rays: they add nothing, the mean still runs over num_rays (rm.mask_nll's contract)
    some = data["masks"].clone(); some[:nr:2] = -1
    _, _, part = mask_train_loss(render(), {**data, "masks": some}, opt, global_step=1)
    pm_l = -torch.log(torch.gather(pm[:nr], -1, gt[:nr, None]))
    assert abs(part.item() - (pm_l[1::2].sum() / nr).item()) <= 1e-5
    opt.ray_pair_rgb_loss_weight = 1.0

    # eager steps vs one captured graph
    def make_step(capturable):
        model, opt, data, emap, uniform, adam, render = _mask_step_setup(gpu, capturable)

        def step():
            adam.zero_grad(set_to_none=True)
            _, _, loss = mask_train_loss(render(), data, opt, global_step=1, error_map=emap, uniform=uniform)
            loss.backward()
            adam.step()
            return loss.detach()
        return model, emap, step
    steps = 6
    map0 = error_map.clone()
    m_eager, map_eager, step_eager = make_step(False)
    losses_e = [float(step_eager()) for _ in range(2)]
    map_eager.copy_(map0)
    losses_e += [float(step_eager()) for _ in range(steps - 2)]
    m_graph, map_graph, step_graph = make_step(True)
    g = GraphedStep(step_graph, warmup=2)
    map_graph.copy_(map0)            # the warm-up has moved the map already: both sides restart it here, so that only replays can move it
    losses_g = [float(g()) for _ in range(steps - 2)]
    torch.cuda.synchronize()
    print("eager", losses_e, "graph", losses_g)
    assert all(np.isfinite(losses_g)) and abs(losses_g[-1] - losses_e[-1]) <= 1e-4 * max(1.0, abs(losses_e[-1]))
    # the replays carry the two EMA launches: without them the map would still be map0, which lies O(0.1 - 1) from the errors it is pulled
    # to; entries no ray points at keep their bits.  Bound: the parameters may differ as bounded below (relative 1e-3), the error
    # exp(-10 cos) moves by at most ten times the difference of cos
    touched = torch.zeros_like(map0, dtype=torch.bool); touched[data["index"], data["inds_coarse"]] = True
    moved = (map_graph - map0).abs()[touched]
    dmap = float((map_graph - map_eager).abs().max())
    print(f"error map: graph vs eager max|diff| {dmap:.2e}; moved from the start by median {float(moved.median()):.2e}")
    assert float(moved.median()) > 0.05 and torch.equal(map_graph[~touched], map0[~touched])
    assert dmap <= 1e-2
    for (n1, p1), (n2, p2) in zip(m_eager.named_parameters(), m_graph.named_parameters()):
        if p1.requires_grad:        # the bounds of test_mask_training_step_replayed_as_a_hip_graph
            assert float((p1 - p2).abs().max()) <= 5e-3, n1
            assert float((p1 - p2).double().norm() / (p1.double().norm() + 1e-12)) <= 1e-3, n1
