#!/usr/bin/env python3
"""Time the parameter average after an optimiser step three ways, for the 13 tensors of the RGB-mode model and for the model with heads:

  hip       optim.ParamEMA.update(): ceil(T / 32) launches of sn_ema_update_multi, the warm-up decay formed in the kernel;
  hip_constant_decay   the same with use_num_updates=False: no device count, no ticket -- what the count costs is the difference;
  torch     torch_ema's statement per tensor, tmp = s - p; tmp.mul_(omd); s.sub_(tmp): 3 T launches, the decay a host number;
  foreach   the same statement as a torch._foreach_sub / _foreach_mul_ / _foreach_sub_ chain over all tensors.

Two modes: eager (the route alone), and inside a captured step behind optim.Adam(capturable=True, multi_tensor=True).step() -- the graph of
"Adam + route" beside the graph of Adam alone; their difference is what the average adds to a replayed step.  (A decay formed on the host
is frozen in such a graph: the torch routes are timed there, not recommended.)

HIP events around `--repeats` calls after `--warmup` calls, the routes alternating within each of `--rounds` rounds; the median and the
extremes over the rounds.  Beside the times: the launches per update (from the code, and as torch.profiler counts the device kernels of
one eager call; null where the profiler is not usable) and the achieved bytes/s -- the algorithm needs 12 B per element (shadow and
parameter read, shadow written), the three-operator statement moves 32 B per element.

    python tools/ema_bench.py [--out profiles/r07/ema_bench.json]

Nothing is asserted about speed; the numbers of one run are reported.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sanerf_hq_amd import _lib, synth  # noqa: E402
from sanerf_hq_amd.optim import Adam, ParamEMA  # noqa: E402

ALGORITHM_BYTES, STATEMENT_BYTES = 12, 32


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
        print(f"[ema_bench] torch.profiler not usable here: {e}", file=sys.stderr)
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


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def bench_model(name, heads, dev, args):
    steps = [128, 64, 32]
    model = synth.product_model(synth.synthetic_params(steps, heads=heads), steps, heads, dev)
    params = list(model.parameters())
    elements = sum(p.numel() for p in params)
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
    opt = Adam(params, lr=1e-4, eps=1e-15, capturable=True, multi_tensor=True)
    ema = ParamEMA(params, 0.95)
    ema_const = ParamEMA(params, 0.95, use_num_updates=False)
    shadows = {k: [p.detach().clone() for p in params] for k in ("torch", "foreach")}
    omd = 1.0 - 0.95

    @torch.no_grad()
    def torch_route():
        for s, p in zip(shadows["torch"], params):
            tmp = s - p
            tmp.mul_(omd)
            s.sub_(tmp)

    @torch.no_grad()
    def foreach_route():
        tmp = torch._foreach_sub(shadows["foreach"], params)
        torch._foreach_mul_(tmp, omd)
        torch._foreach_sub_(shadows["foreach"], tmp)

    routes = {"hip": ema.update, "hip_constant_decay": ema_const.update, "torch": torch_route, "foreach": foreach_route}
    launches_code = {"hip": math.ceil(len(params) / _lib.EMA_MULTI_MAX_TENSORS), "hip_constant_decay": math.ceil(len(params) / _lib.EMA_MULTI_MAX_TENSORS),
                     "torch": 3 * len(params), "foreach": None}
    kernels = {k: device_kernels(fn) for k, fn in routes.items()}
    eager = timed_alternating(routes, args.warmup, args.repeats, args.rounds)

    def behind_adam(fn):
        def step():
            opt.step()
            fn()
        return step
    graphs = {"adam_only": captured(opt.step)}
    graphs.update({k: captured(behind_adam(fn)) for k, fn in routes.items()})
    graph = timed_alternating(graphs, args.warmup, args.repeats, args.rounds)

    def rates(ms, with_statement):
        r = {"achieved_algorithm_bytes_per_s": ALGORITHM_BYTES * elements / (ms * 1e-3)}
        if with_statement:
            r["achieved_statement_bytes_per_s"] = STATEMENT_BYTES * elements / (ms * 1e-3)
        return r
    res = {"model": name, "tensors": len(params), "elements": elements, "algorithm_bytes": ALGORITHM_BYTES * elements,
           "statement_bytes": STATEMENT_BYTES * elements, "num_updates_after": ema.num_updates, "routes": {}}
    for k in routes:
        added = graph[k]["median_ms"] - graph["adam_only"]["median_ms"]
        res["routes"][k] = {"launches_from_code": launches_code[k], "device_kernels_profiled": kernels[k],
                            "eager": {**eager[k], **rates(eager[k]["median_ms"], not k.startswith("hip"))},
                            "captured_behind_adam": {**graph[k], "added_to_adam_only_ms": added, **(rates(added, not k.startswith("hip")) if added > 0 else {})}}
    res["captured_adam_only"] = graph["adam_only"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--models", default="rgb,heads")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    res = {"what": "one update of the parameter average (decay 0.95) over every parameter tensor of the model", "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds, "bytes_per_element": {"algorithm": ALGORITHM_BYTES, "statement": STATEMENT_BYTES},
           "models": [bench_model(m, m == "heads", dev, args) for m in args.models.split(",")]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
