#!/usr/bin/env python3
"""Time the object render (`model.render_object`) beside the plain mask render and a torch-operator route, and its two kernels alone.

  render_object   one fused render + sn_rm_mask_point_labels + sn_rm_object_composite + the per-ray head (the default route);
  mask_render     model.render(..., return_mask=1): the fused render + sn_rm_mask_head (what a mask image costs today);
  torch_labels    render_object with fused_point_labels = False: m_grid.forward_cat -> the matrix-core perceptron -> argmax, which
                  materialises [N*T, 143] and [N*T, K].

Each eager and as a GraphedStep, HIP events around `--repeats` calls after `--warmup` calls, the routes alternating within each of
`--rounds` rounds; median and extremes over the rounds.  Then, on the last-stage samples of the same view:

  mask_head       sn_rm_mask_head alone        (the compositing instantiation of k_mask16);
  point_labels    sn_rm_mask_point_labels alone (the label instantiation: same work minus the compositing);
  composite       sn_rm_object_composite alone, with the GB/s of the N*T*76 bytes it streams (label 1, sigma 4, bin edge 4, 15 geometry
                  channels 60, the weights it may write are not counted; + 7 per-ray outputs).

`--mask-head-only` times sn_rm_mask_head alone and nothing else: with SN_LIB=<a library built from the parent commit> that is the same-box
A/B partner of the label launch (the parent has no label entry).

    python tools/object_render_bench.py [--side 400] [--out profiles/object_render_bench.json]

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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--side", type=int, default=400)
    ap.add_argument("--steps", default="128,64,32")
    ap.add_argument("--n-inst", type=int, default=2)
    ap.add_argument("--mask-head-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("object_render_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [int(s) for s in args.steps.split(",")]
    H = W = args.side
    opt = synth.make_opt(num_steps=steps, with_mask=True, n_inst=args.n_inst, max_ray_batch=1 << 30)
    model = NeRFNetwork(opt)
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    ro, rd = rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(H, W), H, W, device=dev)
    N, T = H * W, steps[-1]
    res = {"what": "render_object beside the mask render and a torch-operator label route; the two kernels alone", "device": torch.cuda.get_device_name(0),
           "library": os.environ.get("SN_LIB") or "product", "image": [H, W], "num_steps": steps, "n_inst": args.n_inst, "rays": N,
           "last_stage_samples": N * T, "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds}

    with torch.no_grad():
        # the last stage's samples of this view, as render_object hands them to its kernels
        out = rm.render_rays(model._get_plan(), ro, rd, want=["xyzs_last", "geo_feat_last", "weights_last", "sigmas_last", "bins_last"])
        k = len(steps) - 1
        xyzs, geo, weights, sig = out["xyzs_last"], out["geo_feat_last"], out["weights_last"], out[f"sigmas{k}"]
        nears, fars = rm.near_far_from_aabb(ro, rd, model.aabb_infer, model.min_near)
        real_bins = rm.sample_positions(ro, rd, nears, fars, out[f"bins{k}"], contract=opt.contract)[0]
        live = (real_bins[:, 1:] - real_bins[:, :-1]) * sig
        live[:, -1] = 1.0
        mlp = model.mask_mlp[0]
        res["live_share"] = {"weights_nonzero": float((weights != 0).float().mean()), "y_nonzero": float((live != 0).float().mean())}
        kernels = {"mask_head": lambda: rm.mask_head(weights, xyzs, geo, model.m_grid, mlp, model.bound),
                   "mask_head_live_as_weights": lambda: rm.mask_head(live, xyzs, geo, model.m_grid, mlp, model.bound)}
        if not args.mask_head_only:
            labels = rm.mask_point_labels(live, xyzs, geo, model.m_grid, mlp, model.bound)
            res["label_histogram"] = {str(int(v)): int(c) for v, c in zip(*labels.unique(return_counts=True))}
            kernels["point_labels"] = lambda: rm.mask_point_labels(live, xyzs, geo, model.m_grid, mlp, model.bound)
            kernels["composite"] = lambda: rm.object_composite(labels, sig, real_bins, geo, rd, 0b10, False, True)
        res["kernels"] = timed_alternating(kernels, args.warmup, args.repeats, args.rounds)
        if not args.mask_head_only:
            nbytes = N * T * 76 + N * (12 + 4 * 33)
            res["kernels"]["composite"]["bytes"] = nbytes
            res["kernels"]["composite"]["GB_per_s"] = nbytes / (res["kernels"]["composite"]["median_ms"] * 1e-3) / 1e9

            def render_object():
                model.fused_point_labels = True
                return model.render_object(ro, rd, [1], H=H, W=W)

            def torch_labels():
                model.fused_point_labels = False
                return model.render_object(ro, rd, [1], H=H, W=W)

            def mask_render():
                return model.render(ro, rd, staged=False, perturb=False, return_mask=1, H=H, W=W)

            routes = {"render_object": render_object, "mask_render": mask_render, "torch_labels": torch_labels}
            eager = timed_alternating(routes, args.warmup, args.repeats, args.rounds)
            graphs = {k_: GraphedStep(fn, warmup=2) for k_, fn in routes.items()}
            graph = timed_alternating(graphs, args.warmup, args.repeats, args.rounds)
            res["routes"] = {k_: {"eager": eager[k_], "graph": graph[k_]} for k_ in routes}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
