#!/usr/bin/env python3
"""Time the draw of one training batch two ways, with the object-field script's geometry (--error_map --mixed_sampling --num_local_sample 4
--local_sample_patch_size 8 --random_image_batch; 4096 rays, error maps of 128 x 128 cells):

  torch      nerf.utils.collate_rays: randint, multinomial, the patch loop with one get_rays call each, the fancy-index gathers and cats;
  hip        nerf.utils.DeviceCollate.draw(): the random fills, one sn_rm_weighted_draw (the patch centres) and one sn_rm_collate_gather;
  hip_graph  the same draw() captured once and replayed.

HIP events around `--repeats` batches after `--warmup` batches, the routes alternating within each of `--rounds` rounds, the median and the
extremes over the rounds (the extremes are the run-to-run spread the comparison is read against).  Beside the times: the device kernels
and copies of one batch of each eager route as torch.profiler counts them (null where the profiler is not usable).

    python tools/collate_bench.py [--out profiles/r07/collate_bench.json]

Nothing is asserted about speed; the numbers of one run are reported.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sanerf_hq_amd.nerf import DeviceCollate, collate_rays  # noqa: E402


def make_dataset(dev, M, H, W, S, classes=8, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    poses = torch.eye(4, device=dev).repeat(M, 1, 1)
    poses[:, :3, :] = torch.randn(M, 3, 4, device=dev, generator=g)
    intr = torch.tensor([[1.1 * W, 1.1 * W, W / 2, H / 2]], device=dev).repeat(M, 1)
    return dict(poses=poses, intrinsics=intr, images=torch.randint(0, 256, (M, H, W, 3), device=dev, dtype=torch.uint8, generator=g),
                masks=torch.randint(0, classes, (M, H, W, 1), device=dev, generator=g),
                error_map=torch.rand(M, S * S, device=dev, generator=g) + 1e-3,
                cam_near_far=torch.rand(M, 2, device=dev, generator=g))


def device_ops(fn):
    """(kernels, copies) on the device for one call of fn, as torch.profiler sees them; (None, None) without a profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = sum(1 for e in dev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower())
        return len(dev) - copies, copies
    except Exception as e:                                              # noqa: BLE001  (a missing tracer is not the bench's business)
        print(f"[collate_bench] torch.profiler not usable here: {e}", file=sys.stderr)
        return None, None


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--error-map-size", type=int, default=128)
    ap.add_argument("--local", type=int, default=4)
    ap.add_argument("--patch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collate_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    M, H, W, S = args.images, args.size, args.size, args.error_map_size
    d = make_dataset(dev, M, H, W, S)
    geo = dict(random_image_batch=True, use_error_map=True, error_map_size=S, num_local_sample=args.local, local_patch_size=args.patch)
    dc = DeviceCollate(d["poses"], d["intrinsics"], H, W, args.rays, images=d["images"], masks=d["masks"], error_map=d["error_map"],
                       cam_near_far=d["cam_near_far"], **geo)
    fns = {"torch": lambda: collate_rays(d["poses"], d["intrinsics"], H, W, args.rays, images=d["images"], masks=d["masks"], error_map=d["error_map"],
                                         cam_near_far=d["cam_near_far"], **geo),
           "hip": dc.draw}
    # the two routes give batches of the same shapes before anything is timed
    a, b = fns["torch"](), fns["hip"]()
    torch.cuda.synchronize()
    shapes_agree = all(tuple(a[k].shape) == tuple(b[k].shape) for k in ("rays_o", "rays_d", "i", "j", "images", "masks", "error_maps", "cam_near_far"))
    ops = {k: device_ops(fn) for k, fn in fns.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dc.draw()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dc.draw()
    fns["hip_graph"] = graph.replay
    times = timed_alternating(fns, args.warmup, args.repeats, args.rounds)
    library_launches = 1 + int(args.local > 0)
    res = {"what": "one training batch: cameras, pixels, rays and supervision gathers", "images": M, "H": H, "W": W, "rays": args.rays,
           "error_map_size": S, "local_patches": args.local, "patch_size": args.patch, "shapes_agree": bool(shapes_agree),
           "short_draw_status": int(dc.status.item()), "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
           "rounds": args.rounds,
           "routes": {k: {**times[k], "device_kernels_per_batch": ops.get(k, (None, None))[0], "device_copies_per_batch": ops.get(k, (None, None))[1]}
                      for k in fns},
           "library_launches_hip": library_launches, "random_fills_hip": len(dc.randoms)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
