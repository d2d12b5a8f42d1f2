#!/usr/bin/env python3
"""Time the perturbed no-grad render (`model.render(staged=True, perturb=True)` under torch.no_grad: the SAM step's ground-truth image and
the viewer's supersampling in the reference) three ways:

  parent        fused_perturb = False, jitter = None: the operator chain with torch.rand jitter (the route before fused_perturb existed);
  fused_rand    the fused render fed with tables from one torch.rand + one rm.jitter launch per stage;
  fused_tables  the fused render fed with rm.jitter_tables (the default route: fused_perturb = True).

Each eager and as a GraphedStep, with HIP events around `--repeats` calls after `--warmup` calls, the routes alternating within each of
`--rounds` rounds; the median and the extremes over the rounds.  Sizes 800x800 and 400x400, schedules [128] and [128, 64, 32], the RGB model
and the mask head (return_mask=1).  Beside the times: the device kernels of one eager call as torch.profiler counts them (null where the
profiler is not usable).  It also times the table launch alone beside a torch.rand of the same size (and beside torch.rand + the rm.jitter
launches that turn it into tables), in GB/s of table written.

    python tools/perturb_bench.py [--out profiles/perturb_bench.json]

Nothing is asserted about speed; the numbers of one run are reported.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sanerf_hq_amd import raymarching as rm, synth  # noqa: E402
from sanerf_hq_amd.graph import GraphedStep  # noqa: E402
from sanerf_hq_amd.nerf import NeRFNetwork  # noqa: E402


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
        print(f"[perturb_bench] torch.profiler not usable here: {e}", file=sys.stderr)
        return None


def timed_alternating(fns, warmup, repeats, rounds):
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in out.items()}


def rand_tables(N, steps, dev):
    """The per-ray tables as the parent's training routes make them: one torch.rand, one rm.jitter launch per stage."""
    rand = torch.rand(N * sum(t + 1 for t in steps), device=dev)
    tabs, at = {}, 0
    for k, t in enumerate(steps):
        tabs[k] = rm.jitter(rand[at:at + N * (t + 1)], N, t + 1, 0 if k == 0 else 1)
        at += N * (t + 1)
    return tabs[0], {k: v for k, v in tabs.items() if k >= 1}


def bench_render(side, steps, mask, dev, args):
    opt = synth.make_opt(num_steps=list(steps), with_mask=mask, max_ray_batch=args.max_ray_batch)
    model = NeRFNetwork(opt)
    params = synth.synthetic_params([128, 64, 32], heads=mask)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    model = model.to(dev).eval()
    H = W = side
    ro, rd = rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(H, W), H, W, device=dev)
    call = dict(staged=True, perturb=True, H=H, W=W, **(dict(return_mask=1) if mask else {}))
    jit = rm.DeviceJitter(dev, seed=1)

    @torch.no_grad()
    def parent():
        model.fused_perturb, model.jitter = False, None
        return model.render(ro, rd, **call)

    @torch.no_grad()
    def fused_tables():
        model.fused_perturb, model.jitter = True, jit
        return model.render(ro, rd, **call)

    class RandJitter:                                                    # DeviceJitter's .tables() out of torch.rand + rm.jitter
        device = torch.device(dev)

        @staticmethod
        def tables(N, steps_, ray_base=0, advance=True):
            return rand_tables(N, steps_, dev)

    @torch.no_grad()
    def fused_rand():
        model.fused_perturb, model.jitter = True, RandJitter
        return model.render(ro, rd, **call)

    routes = {"parent": parent, "fused_rand": fused_rand, "fused_tables": fused_tables}
    kernels = {k: device_kernels(fn) for k, fn in routes.items()}
    eager = timed_alternating(routes, args.warmup, args.repeats, args.rounds)
    graphs = {k: GraphedStep(fn, warmup=2) for k, fn in routes.items()}
    graph = timed_alternating(graphs, args.warmup, args.repeats, args.rounds)
    return {"image": [H, W], "num_steps": list(steps), "head": "mask" if mask else "rgb", "rays": H * W, "chunks": -(-H * W // args.max_ray_batch),
            "routes": {k: {"device_kernels_profiled": kernels[k], "eager": eager[k], "graph": graph[k]} for k in routes}}


def bench_tables(N, steps, dev, args):
    jit = rm.DeviceJitter(dev, seed=1)
    total = N * sum(t + 1 for t in steps)
    out = {k: torch.empty(N, t + 1, device=dev) for k, t in enumerate(steps)}
    fns = {"jitter_tables": lambda: rm.jitter_tables(jit.state, N, steps, out=out),
           "torch_rand": lambda: torch.rand(total, device=dev),
           "torch_rand_plus_jitter": lambda: rand_tables(N, steps, dev)}
    t = timed_alternating(fns, args.warmup, args.repeats, args.rounds)
    for k in t:
        t[k]["table_GB_per_s"] = 4 * total / (t[k]["median_ms"] * 1e-3) / 1e9
        t[k]["launches_from_code"] = {"jitter_tables": 1, "torch_rand": 1, "torch_rand_plus_jitter": 1 + len(steps)}[k]
    return {"rays": N, "num_steps": list(steps), "table_bytes": 4 * total, "routes": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sides", default="800,400")
    ap.add_argument("--heads", default="rgb,mask")
    ap.add_argument("--max-ray-batch", type=int, default=163840, help="opt.max_ray_batch of the staged render (800x800: 4 chunks)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perturb_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    res = {"what": "model.render(staged=True, perturb=True) under no_grad, three routes; and the jitter tables alone", "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds, "max_ray_batch": args.max_ray_batch, "render": [], "tables": []}
    for side in [int(s) for s in args.sides.split(",")]:
        for steps in ([128], [128, 64, 32]):
            res["tables"].append(bench_tables(side * side, steps, dev, args))
            for head in args.heads.split(","):
                res["render"].append(bench_render(side, steps, head == "mask", dev, args))
                print(json.dumps(res["render"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
