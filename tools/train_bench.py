#!/usr/bin/env python3
"""Timings of the two training steps alone (the same numbers tools/bench_configs.py reports, without its other configurations):
  rgb   RGB-mode step (trainer.py:360-392): 4096 rays, [128,64,32], everything trainable, MSE + proposal loss
  mask  BASELINE configs[4]: mask-field step, 4096 rays, field frozen
  mask_extras  the mask-field step as scripts/train_obj_nerf.sh runs it (ray-pair RGB loss over 4 local 8x8 patches, 8 samples each, per-step
        error-map EMA), two routes in one run: the extras as the reference's torch lines (trainer.py:260-305, 434-464) and as the HIP operators
        (nerf.mask_step.mask_train_loss).  `mask_extras_torch K` / `mask_extras_ops K` run K eager steps of one route and nothing else: for a
        kernel trace of its own (launches per step = the difference of two such runs' dispatch counts / the difference of their K)
  rgb_multi / mask_multi  the same two steps with optim.Adam(multi_tensor=True): one sn_adam_step_multi launch for all parameter tensors
  adam_ab [PAIRS]  both steps "with Adam", eager and as a HIP graph, the per-tensor and the multi-tensor route alternating PAIRS (3) times in
        this one process: the spread between the per-tensor runs is the yardstick for the difference between the routes
  rgb_steps / mask_steps K per_tensor|multi_tensor [capturable]  K eager steps of one route and nothing else, for a kernel trace of its own
        (launches per step = the difference of two such runs' dispatch counts / the difference of their K)
usage: train_bench.py [rgb|mask|both|mask_extras|...]  -> one JSON line.  Eager forward+backward, + single-pass Adam, the step as a HIP graph, and (rgb) the
step without proposal update (4 of 5 steps after step 3000, trainer.py:372-373)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from bench_configs import timeit  # noqa: E402
from helpers import make_opt, synthetic_params  # noqa: E402
from sanerf_hq_amd import ops, raymarching as rm, synth  # noqa: E402
from sanerf_hq_amd.graph import GraphedStep  # noqa: E402
from sanerf_hq_amd.nerf import NeRFNetwork  # noqa: E402
from sanerf_hq_amd.optim import Adam as HipAdam  # noqa: E402

dev = torch.device("cuda:0")
H = W = 512
N = 4096
best = lambda fn, n=3: min(timeit(fn) for _ in range(n))        # noqa: E731


def rays():
    roF, rdF = rm.generate_rays(synth.orbit_pose(1.1, 25.0, 60.0), synth.pinhole_intrinsics(H, W), H, W, device=dev)
    pix = torch.from_numpy((synth.hash_u01(N, 99) * (H * W)).astype(np.int64)).to(dev)
    return roF[pix].contiguous(), rdF[pix].contiguous()


def rgb_setup(multi=False):
    ro, rd = rays()
    opt = make_opt()
    opt.lambda_proposal, opt.lambda_distort = 1.0, 0.0
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params([128, 64, 32], seed=1).items()}, strict=False)
    model = model.to(dev).train()
    gt = torch.from_numpy(synth.hash_uniform((N, 3), 42, 0.0, 1.0)).to(dev)
    new_optim = lambda capturable=False, multi=multi: HipAdam(model.get_params(1e-2), eps=1e-15, capturable=capturable, multi_tensor=multi)   # noqa: E731
    box = {"optim": new_optim(), "upd": True}

    def fwd_bwd():
        box["optim"].zero_grad(set_to_none=True)
        o = model.render(ro, rd, staged=False, bg_color=1, perturb=True, update_proposal=box["upd"])
        loss = torch.nn.functional.mse_loss(o["image"], gt)
        if box["upd"]:
            loss = loss + o["proposal_loss"]
        loss.backward()

    def step():
        fwd_bwd()
        box["optim"].step()
    return box, fwd_bwd, step, new_optim


def rgb(multi=False):
    box, fwd_bwd, step, new_optim = rgb_setup(multi)
    out = {"fwd_bwd_ms": round(best(fwd_bwd) * 1e3, 3), "step_ms": round(best(step) * 1e3, 3)}
    box["upd"] = False
    out["fwd_bwd_without_proposal_update_ms"] = round(best(fwd_bwd) * 1e3, 3)
    out["step_without_proposal_update_ms"] = round(best(step) * 1e3, 3)
    for upd, key in ((True, "step_as_hip_graph_ms"), (False, "step_without_proposal_update_as_hip_graph_ms")):
        box["upd"] = upd
        box["optim"] = new_optim(True)
        try:
            g = GraphedStep(step, warmup=3)
            out[key] = round(best(g) * 1e3, 3)
            del g
        except Exception as e:   # noqa: BLE001
            out[key] = f"failed: {type(e).__name__}: {e}"
    return out


def mask_setup(multi=False):
    ro, rd = rays()
    opt = make_opt(with_mask=True)
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params([128, 64, 32], heads=True, seed=1).items()}, strict=False)
    model = model.to(dev).train()
    for n_, p in model.named_parameters():
        p.requires_grad_(n_.startswith("m_grid") or n_.startswith("mask_mlp"))
    labels = torch.from_numpy((synth.hash_u01(N, 100) < 0.5).astype(np.int64)).to(dev)
    train = [p for p in model.parameters() if p.requires_grad]
    new_optim = lambda capturable=False, multi=multi: HipAdam(train, lr=1e-3, eps=1e-15, capturable=capturable, multi_tensor=multi)   # noqa: E731
    box = {"optim": new_optim()}

    def fwd_bwd():
        box["optim"].zero_grad(set_to_none=True)
        o = model.render(ro, rd, staged=False, bg_color=1, perturb=False, update_proposal=False, return_mask=1)
        rm.mask_nll(o["instance_mask_logits"], labels, 1e-6).mean().backward()

    def step():
        fwd_bwd()
        box["optim"].step()
    return box, fwd_bwd, step, new_optim


def mask(multi=False):
    box, fwd_bwd, step, new_optim = mask_setup(multi)
    ops.WGRAD_SIDE_STREAM = True
    out = {"fwd_bwd_ms": round(best(fwd_bwd) * 1e3, 3), "step_ms": round(best(step) * 1e3, 3)}
    box["optim"] = new_optim(True)
    try:
        g = GraphedStep(step, warmup=3)
        out["step_as_hip_graph_ms"] = round(best(g) * 1e3, 3)
        del g
    except Exception as e:   # noqa: BLE001
        out["step_as_hip_graph_ms"] = f"failed: {type(e).__name__}: {e}"
    ops.WGRAD_SIDE_STREAM = False
    return out


def adam_ab(setup, pairs=3, side_stream=False):
    """The step with Adam, eager and as a HIP graph: per-tensor and multi-tensor route in turn, `pairs` times, same model and process."""
    box, _, step, new_optim = setup()
    ops.WGRAD_SIDE_STREAM = side_stream
    out = {"eager_step_ms": [], "step_as_hip_graph_ms": []}
    for _ in range(pairs):
        eager, graph = {}, {}
        for name, multi in (("per_tensor", False), ("multi_tensor", True)):
            box["optim"] = new_optim(False, multi)
            eager[name] = round(best(step) * 1e3, 3)
            box["optim"] = new_optim(True, multi)
            try:
                g = GraphedStep(step, warmup=3)
                graph[name] = round(best(g) * 1e3, 3)
                del g
            except Exception as e:   # noqa: BLE001
                graph[name] = f"failed: {type(e).__name__}: {e}"
        out["eager_step_ms"].append(eager)
        out["step_as_hip_graph_ms"].append(graph)
    ops.WGRAD_SIDE_STREAM = False
    return out


def eager_steps(setup, k, multi, capturable, side_stream=False):
    box, _, step, new_optim = setup()
    ops.WGRAD_SIDE_STREAM = side_stream
    box["optim"] = new_optim(capturable, multi)
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    ops.WGRAD_SIDE_STREAM = False
    return {"eager_steps_run": k, "multi_tensor": multi, "capturable": capturable}


def torch_extras_loss(o, data, opt, error_map):
    """trainer.py:412-505 (mixed sampling, error map) in the reference's torch ops, torch.multinomial included."""
    F = torch.nn.functional
    nr, G, P, eps, w = opt.num_rays, opt.num_local_sample, opt.local_sample_patch_size ** 2, opt.epsilon, opt.ray_pair_rgb_exp_weight
    gt = data["masks"].to(torch.long).view(-1)
    inst = torch.softmax(o["instance_mask_logits"], dim=-1)
    pm = torch.clamp(inst, min=eps, max=1 - eps)
    loss = (-torch.log(torch.gather(pm[:nr], -1, gt[:nr, None]))).mean()
    onehot = torch.zeros_like(pm[:nr]).scatter_(-1, gt[:nr, None], 1)
    error = torch.exp(-w * F.cosine_similarity(inst[:nr].detach(), onehot, dim=-1) - eps)
    index, inds = data["index"], data["inds_coarse"]
    error_map[index, inds] = 0.1 * error_map[index, inds] + 0.9 * error
    rgb, masks, inc = o["image"][nr:].view(G, P, 3), inst[nr:].view(G, P, -1), data["error_maps"][nr:].view(G, P)
    weights = ((1.0 - inc) > 0.8).to(torch.float32)
    weights = torch.where(weights.sum(-1, keepdim=True) == 0, torch.ones_like(weights), weights)      # (the reference's indexed form reads a count on the host)
    sample_index = torch.multinomial(weights, num_samples=opt.ray_pair_rgb_num_sample, replacement=False)
    col = torch.arange(G, dtype=torch.int64, device=rgb.device)
    rgb_sample = rgb[col[:, None], sample_index][..., None, :]
    sample_mask = masks[col[:, None], sample_index][..., None, :].detach()
    arg = torch.argmax(sample_mask, -1)
    sample_mask = torch.zeros_like(sample_mask).scatter_(-1, arg[..., None], 1)
    sim = torch.norm(rgb[:, None] - rgb_sample, dim=-1) < opt.ray_pair_rgb_threshold
    e = torch.exp(-w * F.cosine_similarity(masks[:, None], sample_mask, dim=-1) - eps)
    pair = ((sim * e).sum(-1) / sim.sum(-1)).mean()
    return loss + pair * opt.ray_pair_rgb_loss_weight


def mask_extras(which="both", eager_steps=0):
    from sanerf_hq_amd.nerf import mask_train_loss
    G, ps = 4, 8
    n_all = N + G * ps * ps
    roF, rdF = rm.generate_rays(synth.orbit_pose(1.1, 25.0, 60.0), synth.pinhole_intrinsics(H, W), H, W, device=dev)
    pix = (synth.hash_u01(N, 99) * (H * W)).astype(np.int64)
    corner = (synth.hash_u01(2 * G, 98) * (H - ps)).astype(np.int64).reshape(G, 2)
    dy, dx = np.meshgrid(np.arange(ps), np.arange(ps), indexing="ij")
    pix = torch.from_numpy(np.concatenate([pix, ((corner[:, 0, None, None] + dy) * W + corner[:, 1, None, None] + dx).reshape(-1)])).to(dev)
    ro, rd = roF[pix].contiguous(), rdF[pix].contiguous()
    opt = make_opt(with_mask=True)
    for k, v in dict(num_rays=N, ray_pair_rgb_loss_weight=1.0, ray_pair_rgb_num_sample=8, mixed_sampling=True, num_local_sample=G,
                     local_sample_patch_size=ps, ray_pair_rgb_threshold=0.3, ray_pair_rgb_exp_weight=10.0, ray_pair_rgb_iter=-1,
                     ray_pair_rgb_use_pred_logistics=False, label_regularization_weight=0, epsilon=1e-6).items():
        setattr(opt, k, v)
    cells, M = 128 * 128, 8
    perm = np.argsort(synth.hash_u01(M * cells, 97))[:N]
    data = dict(masks=torch.from_numpy((synth.hash_u01(n_all, 100) < 0.5).astype(np.int64)).to(dev)[:, None],
                index=torch.from_numpy(perm // cells).to(dev), inds_coarse=torch.from_numpy(perm % cells).to(dev),
                error_maps=torch.from_numpy(synth.hash_u01(n_all, 96).astype(np.float32) * 0.5).to(dev))
    out = {}
    for route in ("torch_lines", "hip_operators"):
        if which not in ("both", route):
            continue
        model = NeRFNetwork(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params([128, 64, 32], heads=True, seed=1).items()}, strict=False)
        model = model.to(dev).train()
        for n_, p in model.named_parameters():
            p.requires_grad_(n_.startswith("m_grid") or n_.startswith("mask_mlp"))
        train = [p for p in model.parameters() if p.requires_grad]
        box = {"optim": HipAdam(train, lr=1e-3, eps=1e-15)}
        emap = torch.from_numpy(synth.hash_u01(M * cells, 95).astype(np.float32).reshape(M, cells)).to(dev)
        ops.WGRAD_SIDE_STREAM = True

        def step():
            box["optim"].zero_grad(set_to_none=True)
            o = model.render(ro, rd, staged=False, bg_color=1, perturb=False, update_proposal=False, return_mask=1)
            if route == "torch_lines":
                loss = torch_extras_loss(o, data, opt, emap)
            else:
                loss = mask_train_loss(o, data, opt, 1, error_map=emap)[2]
            loss.backward()
            box["optim"].step()
        if eager_steps:
            for _ in range(eager_steps):
                step()
            torch.cuda.synchronize()
            out[route] = {"eager_steps_run": eager_steps}
            continue
        res = {"step_ms": round(best(step) * 1e3, 3)}
        box["optim"] = HipAdam(train, lr=1e-3, eps=1e-15, capturable=True)
        try:
            g = GraphedStep(step, warmup=3)
            res["step_as_hip_graph_ms"] = round(best(g) * 1e3, 3)
            del g
        except Exception as e:   # noqa: BLE001
            res["step_as_hip_graph_ms"] = f"failed: {type(e).__name__}: {e}"
        ops.WGRAD_SIDE_STREAM = False
        out[route] = res
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    res = {}
    if which in ("rgb", "both"):
        res["rgb_training_step_4096_rays"] = rgb()
    if which in ("mask", "both"):
        res["c5_mask_training_step_4096_rays"] = mask()
    if which == "rgb_multi":
        res["rgb_training_step_4096_rays_multi_tensor_adam"] = rgb(multi=True)
    if which == "mask_multi":
        res["c5_mask_training_step_4096_rays_multi_tensor_adam"] = mask(multi=True)
    if which == "adam_ab":
        pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
        res["rgb_training_step_4096_rays"] = adam_ab(rgb_setup, pairs)
        res["c5_mask_training_step_4096_rays"] = adam_ab(mask_setup, pairs, side_stream=True)
    if which in ("rgb_steps", "mask_steps"):
        res[which] = eager_steps(rgb_setup if which == "rgb_steps" else mask_setup, int(sys.argv[2]), sys.argv[3] == "multi_tensor",
                                 "capturable" in sys.argv[4:], side_stream=which == "mask_steps")
    if which == "mask_extras":
        res["mask_step_with_ray_pair_loss_and_error_map_4096_plus_256_rays"] = mask_extras()
    if which in ("mask_extras_torch", "mask_extras_ops"):
        res[which] = mask_extras("torch_lines" if which.endswith("torch") else "hip_operators", eager_steps=int(sys.argv[2]))
    print(json.dumps(res))
