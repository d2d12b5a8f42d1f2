#!/usr/bin/env python3
"""Time the mask field's output stage and evaluation meters (rm.mask_output, rm.mask_eval_accumulate) against a torch-operator route
written here for the comparison (softmax, max, table lookup, blend, 8-bit cast; clamp, gather, log, one-hot counts -- no host read
either, so that both routes can be captured), at 400x400 and 800x800, K = 2 and 8:

  eager   the tail alone on given logits, per call, HIP events around `--repeats` calls after `--warmup` calls, the two routes alternating within each of `--rounds`
          rounds, median over the rounds
  graph   a mask-mode model.render followed by the tail, captured as one HIP graph; reported: the graph with each tail minus the
          graph of the render alone

    python tools/mask_output_bench.py [--sizes 400 800] [--ks 2 8] [--no-graph] > profiles/r07/mask_output_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sanerf_hq_amd import raymarching as rm, synth  # noqa: E402
from sanerf_hq_amd.nerf import NeRFNetwork  # noqa: E402


def timed_alternating(fns, warmup, repeats, rounds):
    """ms per call of each route in `fns` (name -> callable): the routes alternate within every round, so that clock and
    temperature drift meets all of them alike; a window is `repeats` calls between two HIP events; the median over the rounds."""
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
    return {k: statistics.median(v) for k, v in out.items()}


def torch_tail(logits, image, cm, labels, acc, alpha=0.7, eps=1e-6):
    """The comparison route: test_step's composition overlay + 8-bit image, eval_step's loss and a mean IoU, as torch operators."""
    K = logits.shape[-1]
    p = torch.softmax(logits, -1)
    conf, ids = p.max(-1)
    rgb = image * alpha + cm[ids] * (1 - alpha)
    rgb8 = (rgb * 255).clamp(0, 255).to(torch.uint8)
    valid = labels >= 0
    py = torch.gather(p.clamp(eps, 1 - eps), -1, labels.clamp(min=0)[:, None])[:, 0]
    nll = torch.where(valid, -torch.log(py), torch.zeros_like(py)).sum() / valid.sum().clamp(min=1)
    a, b = F.one_hot(ids, K).bool(), F.one_hot(labels.clamp(min=0), K).bool() & valid[:, None]
    inter, union = (a & b).sum(0).double(), (a | b).sum(0).double()
    seen = union > 0
    miou = torch.where(seen, inter / union.clamp(min=1), torch.zeros_like(union)).sum() / seen.sum().clamp(min=1)
    acc += torch.stack([nll.double(), miou])
    return rgb, rgb8


def native_tail(logits, image, cm, labels, rec, ws, out):
    o = rm.mask_output(logits, color_map=cm, image=image, mode="composition", want=("probs", "instance_id", "confidence", "rgb", "rgb8"), out=out)
    rm.mask_eval_accumulate(logits, labels, rec, ws)
    return o["rgb"], o["rgb8"]


def mask_model(K, steps, dev):
    params = synth.synthetic_params(steps, heads=True, seed=5)
    torch.manual_seed(K)
    model = NeRFNetwork(synth.make_opt(num_steps=list(steps), with_mask=True, n_inst=K))
    own = model.state_dict()
    sd = {k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}
    model.load_state_dict(sd, strict=False)              # K != 2: the mask MLP's last layer keeps its seeded initialisation
    return model.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[400, 800])
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--graph-repeats", type=int, default=50, help="replays per timing window (a window of a few hundred ms)")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for S in args.sizes:
        for K in args.ks:
            N = S * S
            torch.manual_seed(S + K)
            logits, image = torch.randn(N, K, device=dev) * 2, torch.rand(N, 3, device=dev)
            labels = torch.randint(-1, K, (N,), device=dev)
            cm = torch.rand(100, 3, device=dev)
            rec, ws, out, acc = rm.eval_record(dev), rm.eval_workspace(dev), {}, torch.zeros(2, device=dev, dtype=torch.float64)
            t = timed_alternating({"native": lambda: native_tail(logits, image, cm, labels, rec, ws, out),
                                   "torch": lambda: torch_tail(logits, image, cm, labels, acc)}, args.warmup, args.repeats, args.rounds)
            row = {"size": S, "K": K, "eager_native_ms": t["native"], "eager_torch_ms": t["torch"]}
            if not args.no_graph:
                steps = [128, 64, 32]
                model = mask_model(K, steps, dev)
                ro, rd = rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(S, S), S, S, device=dev)

                def render():
                    with torch.no_grad():
                        return model.render(ro, rd, staged=False, perturb=False, return_mask=1, H=S, W=S, tile_w=S)

                def capture(tail):
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        o = render()
                        tail(o)
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        o = render()
                        tail(o)
                    return g

                graphs = {"render": capture(lambda o: None),
                          "native": capture(lambda o: native_tail(o["instance_mask_logits"], o["image"], cm, labels, rec, ws, out)),
                          "torch": capture(lambda o: torch_tail(o["instance_mask_logits"], o["image"], cm, labels, acc))}
                t = timed_alternating({k: g.replay for k, g in graphs.items()}, 5, args.graph_repeats, args.rounds)
                row.update(graph_render_ms=t["render"], graph_native_tail_ms=t["native"] - t["render"], graph_torch_tail_ms=t["torch"] - t["render"])
            results.append(row)
            print(json.dumps(row), flush=True)
    return results


if __name__ == "__main__":
    main()
