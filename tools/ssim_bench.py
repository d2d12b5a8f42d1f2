#!/usr/bin/env python3
"""Time the device-side SSIM meter (rm.image_ssim_accumulate) beside the fp32 torch-operator statement of the same quantity written here
for the comparison (F.conv2d with groups = 3 over the five moment maps, no host read either), on one 800x800 and one 400x400 pair, with a
derived and an explicit data_range:

  per call, HIP events around `--repeats` calls after `--warmup` calls, the two routes alternating within each of `--rounds` rounds, the
  median over the rounds; beside the times, each route's value and its distance from the fp64 statement (tests/ssim_ref64.py, on the CPU).

    python tools/ssim_bench.py [--sizes 800 400] [--out profiles/r07/ssim_bench.json]

Bytes: the kernel's compulsory traffic is the two images once (2 * H * W * 3 * 4 bytes; the derived range reads them a second time)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sanerf_hq_amd import raymarching as rm  # noqa: E402
import ssim_ref64 as ref  # noqa: E402


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


def torch_ssim(pred, truth, window, acc, data_range=None):
    """The comparison route: [H,W,3] float32 -> the valid-window statement in fp32 torch operators, added to `acc` on the device."""
    p, t = pred.permute(2, 0, 1)[None], truth.permute(2, 0, 1)[None]
    dr = torch.maximum(p.max() - p.min(), t.max() - t.min()) if data_range is None else data_range
    c1, c2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    m = F.conv2d(torch.cat([p, t, p * p, t * t, p * t], 1), window, groups=15)[0]
    mu_p, mu_t, e_pp, e_tt, e_pt = m[0:3], m[3:6], m[6:9], m[9:12], m[12:15]
    var_p, var_t = torch.clamp(e_pp - mu_p * mu_p, min=0), torch.clamp(e_tt - mu_t * mu_t, min=0)
    cov = e_pt - mu_p * mu_t
    v = (((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2))).mean()
    acc += v
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 400])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench: no GPU visible; a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    g = ref.gaussian(torch.float32)
    window = (g[:, None] * g[None, :]).expand(15, 1, ref.TAPS, ref.TAPS).contiguous().to(dev)
    rows = []
    for S in args.sizes:
        torch.manual_seed(S)
        yy, xx = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
        truth = torch.stack([0.5 + 0.4 * torch.sin(9 * xx + 5 * yy), 0.5 + 0.4 * torch.cos(7 * yy - 3 * xx), 0.1 + 0.8 * xx * yy], -1).clamp(0, 1)
        pred = (truth + 0.08 * torch.randn(S, S, 3)).clamp(0, 1)
        p, t = pred.to(dev).contiguous(), truth.to(dev).contiguous()
        for dr in (None, 1.0):
            want = ref.ssim_valid(pred, truth, dr)
            rec, ws, acc = rm.ssim_record(dev), rm.ssim_workspace(dev), torch.zeros((), device=dev)
            times = timed_alternating({"native": lambda: rm.image_ssim_accumulate(p, t, rec, ws, data_range=dr),
                                       "torch": lambda: torch_ssim(p, t, window, acc, dr)}, args.warmup, args.repeats, args.rounds)
            native = rm.read_ssim_record(rec)["last"]
            torch_v = float(torch_ssim(p, t, window, acc, dr))
            row = {"size": S, "data_range": "derived" if dr is None else dr, "native": times["native"], "torch": times["torch"],
                   "image_bytes": 2 * S * S * 3 * 4, "fp64": want, "native_value": native, "native_abs_err": abs(native - want),
                   "torch_value": torch_v, "torch_abs_err": abs(torch_v - want), "repeats": args.repeats, "rounds": args.rounds}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
