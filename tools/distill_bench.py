#!/usr/bin/env python3
"""Time the fused SAM-feature distillation loss (rm.feature_distill_loss: resize, MSE and gradient in HIP) beside the torch tail it
replaces -- reshape / permute / contiguous / F.interpolate(mode="bilinear") / MSELoss / mean and autograd's mirror image of each, written
here for the comparison (nerf/trainer.py:540-550):

  the operator alone   loss + gradient with respect to the features at 64x64 -> 64x64 and 24x24 -> 32x32, C = 256;
  the whole SAM step   render -> loss -> backward on the model and rays of tests/golden/train_sam.npz, with either tail.

Per call, HIP events around `--repeats` calls after `--warmup` calls, the two routes alternating within each of `--rounds` rounds, the
median and the extremes over the rounds (the extremes are the run-to-run spread the comparison is read against).

    python tools/distill_bench.py [--out profiles/r07/distill_bench.json]

Bytes: the operator's compulsory traffic is the features and the target once in, the gradient once out (3 * 4 * C * 64 * 64 = 12 MB at
the reference's shape)."""
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in out.items()}


def torch_tail(samvit, h, w, gt):
    """The comparison route: trainer.py:540-550 as the reference writes it."""
    C = samvit.shape[-1]
    pred = samvit.reshape(1, h, w, C).permute(0, 3, 1, 2).contiguous()
    pred = F.interpolate(pred, gt.shape[2:], mode="bilinear")
    return torch.nn.MSELoss(reduction="none")(pred, gt).mean()


def operator_rows(dev, args):
    rows = []
    for h, w, Ho, Wo, C in ((64, 64, 64, 64, 256), (24, 24, 32, 32, 256)):
        g = torch.Generator().manual_seed(h + Ho)
        feat = torch.randn(h * w, C, generator=g).to(dev).requires_grad_(True)
        gt = torch.randn(1, C, Ho, Wo, generator=g).to(dev)

        def native():
            feat.grad = None
            rm.feature_distill_loss(feat, h, w, gt).backward()

        def torch_route():
            feat.grad = None
            torch_tail(feat, h, w, gt).backward()

        times = timed_alternating({"native": native, "torch": torch_route}, args.warmup, args.repeats, args.rounds)
        native(); gn = feat.grad.clone(); ln = float(rm.feature_distill_loss(feat, h, w, gt))
        torch_route(); gt_ = feat.grad.clone(); lt = float(torch_tail(feat, h, w, gt))
        row = {"what": "operator", "shape": f"{h}x{w}->{Ho}x{Wo}", "C": C, "native": times["native"], "torch": times["torch"],
               "compulsory_bytes": 4 * (2 * h * w * C + C * Ho * Wo), "native_loss": ln, "torch_loss": lt,
               "max_abs_grad_difference": float((gn - gt_).abs().max()), "repeats": args.repeats, "rounds": args.rounds}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_row(dev, args):
    from helpers import golden, make_opt, params_from_spec, spec_of
    from sanerf_hq_amd import synth
    from sanerf_hq_amd.nerf import NeRFNetwork, sam_train_loss
    g = golden("train_sam")
    opt = make_opt(with_sam=True)
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params_from_spec(spec_of(g)).items()}, strict=False)
    model = model.to(dev).train()
    for n_, p in model.named_parameters():
        p.requires_grad_(n_.startswith("s_grid") or n_.startswith("samvit_mlp"))
    h, w = int(g["h"]), int(g["w"])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ro, rd = T(g["rays_o"]), T(g["rays_d"])
    gt = T(synth.hash_uniform(tuple(int(v) for v in g["gt_shape"]), int(g["gt_seed"]), -1.0, 1.0))
    data = {"h": h, "w": w, "gt_samvit": gt}
    params = [p for p in model.parameters() if p.requires_grad]

    def step(tail):
        for p in params:
            p.grad = None
        out = model.render(ro, rd, staged=False, bg_color=1, perturb=False, return_feats=1, H=h, W=w)
        loss = sam_train_loss(out, data, opt, want_pred=False)[2] if tail == "native" else torch_tail(out["samvit"], h, w, gt)
        loss.backward()
        return loss

    times = timed_alternating({"native": lambda: step("native"), "torch": lambda: step("torch")}, max(args.warmup // 4, 3),
                              max(args.repeats // 10, 5), args.rounds)
    row = {"what": "sam_step (render, loss, backward)", "shape": f"{h}x{w}->{gt.shape[2]}x{gt.shape[3]}", "C": int(gt.shape[1]),
           "native": times["native"], "torch": times["torch"], "native_loss": float(step("native")), "torch_loss": float(step("torch")),
           "repeats": max(args.repeats // 10, 5), "rounds": args.rounds}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench: no GPU visible; a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    rows = operator_rows(dev, args)
    rows.append(step_row(dev, args))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
