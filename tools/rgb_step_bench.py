#!/usr/bin/env python3
"""Time the RGB step's loss tail in HIP (rm.rgb_loss / nerf.rgb_train_step) beside the torch tail it replaces, for the two background
settings of the reference's command line:

  the tail alone   loss + gradients with respect to image and weights_sum at 4096 rays, with the proposal loss folded in:
                     'white'   torch: F.mse_loss(image, gt) + proposal (tools/train_bench.py:56-62)      HIP: rm.rgb_loss(image_has_bg=True)
                     'random'  torch: image + (1 - weights_sum) bg, then the same                        HIP: rm.rgb_loss(bg [N,3], image_has_bg=False)
  the whole step   zero_grad -> render -> tail -> backward -> multi-tensor Adam on the model of tools/train_bench.py (4096 rays, [128,64,32]):
                     'white'   both routes render over 1 on the fused training route; only the tail differs
                     'random'  torch: torch.rand(N,3), model.render(bg_color=<tensor>) -- the operator chain, the fused route refuses a tensor --
                               and the torch tail;  HIP: nerf.rgb_train_step, which renders over 0 on the fused route and adds the term in the tail

Each route runs eager and as a captured graph (graph.GraphedStep).  Per call, HIP events around `--repeats` calls after `--warmup` calls,
the routes alternating within each of `--rounds` rounds; the median and the extremes over the rounds (the extremes are the run-to-run
spread a difference is read against).  Beside the times: the device kernels of one eager call of each route as torch.profiler counts
them (null where the profiler is not usable).

    python tools/rgb_step_bench.py [--out profiles/rgb_step_bench.json]

Nothing is asserted about speed; the numbers of one run are reported."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sanerf_hq_amd import raymarching as rm  # noqa: E402

N, H, W = 4096, 512, 512


def device_kernels(fn):
    """Device kernels of one call of fn as torch.profiler sees them; None without a profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower())
    except Exception as e:                                              # noqa: BLE001  (a missing tracer is not the bench's business)
        print(f"[rgb_step_bench] torch.profiler not usable here: {e}", file=sys.stderr)
        return None


def timed_alternating(fns, warmup, repeats, rounds):
    """ms per call of each route in `fns` (name -> callable): the routes alternate within every round, so that clock and temperature
    drift meets all of them alike; a window is `repeats` calls between two HIP events; the median and the extremes over the rounds."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeats):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / repeats)
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)} for k, v in out.items()}


def graphed(fn):
    from sanerf_hq_amd.graph import GraphedStep
    try:
        return GraphedStep(fn, warmup=3)
    except Exception as e:   # noqa: BLE001
        print(f"[rgb_step_bench] capture failed: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def tail_rows(dev, args):
    from sanerf_hq_amd import synth
    T = lambda shape, seed: torch.from_numpy(synth.hash_uniform(shape, seed, 0.0, 1.0)).to(dev)   # noqa: E731
    image, ws = T((N, 3), 1).requires_grad_(True), T((N,), 2).requires_grad_(True)
    gt, bg = T((N, 3), 3), T((N, 3), 4)
    prop = torch.tensor(0.05, device=dev, requires_grad=True)
    rows = []
    for background in ("white", "random"):
        def torch_route():
            image.grad = ws.grad = prop.grad = None
            pred = image if background == "white" else image + (1 - ws).unsqueeze(-1) * bg
            loss = F.mse_loss(pred, gt) + prop
            loss.backward()
            return loss

        def hip_route():
            image.grad = ws.grad = prop.grad = None
            loss = rm.rgb_loss(image, ws, gt, bg=1.0 if background == "white" else bg, image_has_bg=background == "white",
                               extras=[(prop, 1.0)], want_pred=True)[0]
            loss.backward()
            return loss

        fns = {"torch_eager": torch_route, "hip_eager": hip_route}
        for name, fn in (("torch_graph", torch_route), ("hip_graph", hip_route)):
            g = graphed(fn)
            if g is not None:
                fns[name] = g
        times = timed_alternating(fns, args.warmup, args.repeats, args.rounds)
        lt, lh = float(torch_route().detach()), float(hip_route().detach())
        row = {"what": "tail alone (loss, gradients of image and weights_sum)", "background": background, "rays": N, **times,
               "device_kernels": {"torch": device_kernels(torch_route), "hip": device_kernels(hip_route)},
               "torch_loss": lt, "hip_loss": lh, "repeats": args.repeats, "rounds": args.rounds}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_rows(dev, args):
    from helpers import make_opt, synthetic_params
    from sanerf_hq_amd import synth
    from sanerf_hq_amd.nerf import NeRFNetwork, rgb_train_step
    from sanerf_hq_amd.optim import Adam as HipAdam
    roF, rdF = rm.generate_rays(synth.orbit_pose(1.1, 25.0, 60.0), synth.pinhole_intrinsics(H, W), H, W, device=dev)
    pix = torch.from_numpy((synth.hash_u01(N, 99) * (H * W)).astype(np.int64)).to(dev)
    data = {"rays_o": roF[pix].contiguous(), "rays_d": rdF[pix].contiguous(),
            "images": torch.from_numpy(synth.hash_uniform((N, 3), 42, 0.0, 1.0)).to(dev)}
    rows = []
    for background in ("white", "random"):
        opt = make_opt(background=background, lambda_proposal=1.0, lambda_distort=0.0)
        model = NeRFNetwork(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params([128, 64, 32], seed=1).items()}, strict=False)
        model = model.to(dev).train()
        uniform = torch.empty(N, 3, device=dev)
        box = {}

        def new_optim():
            box["optim"] = HipAdam(model.get_params(1e-2), eps=1e-15, capturable=True, multi_tensor=True)

        def torch_step():
            box["optim"].zero_grad(set_to_none=True)
            bg = torch.rand(N, 3, device=dev) if background == "random" else 1
            o = model.render(data["rays_o"], data["rays_d"], staged=False, bg_color=bg, perturb=True, update_proposal=True)
            loss = F.mse_loss(o["image"], data["images"]) + o["proposal_loss"]
            loss.backward()
            box["optim"].step()
            return loss

        def hip_step():
            box["optim"].zero_grad(set_to_none=True)
            if background == "random":
                uniform.uniform_()
            loss = rgb_train_step(model, data, opt, 10, uniform=uniform)[2]
            loss.backward()
            box["optim"].step()
            return loss

        new_optim()
        fns = {"torch_eager": torch_step, "hip_eager": hip_step}
        for name, fn in (("torch_graph", torch_step), ("hip_graph", hip_step)):
            g = graphed(fn)
            if g is not None:
                fns[name] = g
        warmup, repeats = max(args.warmup // 4, 3), max(args.repeats // 10, 5)
        times = timed_alternating(fns, warmup, repeats, args.rounds)
        row = {"what": "whole step (zero_grad, render, tail, backward, multi-tensor Adam)", "background": background, "rays": N,
               "num_steps": list(opt.num_steps), **times,
               "device_kernels": {"torch": device_kernels(torch_step), "hip": device_kernels(hip_step)},
               "repeats": repeats, "rounds": args.rounds}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgb_step_bench: no GPU visible; a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    rows = tail_rows(dev, args) + step_rows(dev, args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
