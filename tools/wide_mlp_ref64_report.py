#!/usr/bin/env python3
"""What the float cases of tests/test_gpu_wide_mlp_ref64.py measure, as a table (profiles/wide_mlp_ref64.txt):

  * the worst |err| / bound per float kind and entry point of the 256-wide split-fp16 perceptron kernels, against tests/wide_ref64.py, with
    the size of the bound relative to the output, and the same for the LayerNorm epilogues behind an exact chain;
  * for the kinds whose inputs sit at a fresh table's +-1e-4 (fresh_field, all_small): the worst error relative to the row's largest output,
    against the unsplit float64 product chain, beside the same figure of torch's fp32 matmul chain on the same data (the baseline).

Usage: python tools/wide_mlp_ref64_report.py > profiles/wide_mlp_ref64.txt
"""
import argparse
import hashlib
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import wide_cases as K  # noqa: E402
import wide_hip as T  # noqa: E402
import wide_ref64 as R  # noqa: E402
from test_wide_ref64 import torch_forward  # noqa: E402


def true_chain(x, ws, bs, skip, leaky):
    """The product chain of the unsplit values in float64."""
    h, xd = x.double(), x.double()
    for l, W in enumerate(ws):
        if l in skip and l > 0:
            h = torch.cat([h, xd], 1)
        h = h @ W.double().t() + (bs[l].double() if bs and bs[l] is not None else 0.0)
        if l + 1 < len(ws):
            h = torch.nn.functional.leaky_relu(h, 0.01) if leaky else torch.relu(h)
    return h


def row_relative(got, ref):
    return float(((got.double() - ref).abs().amax(1) / ref.abs().amax(1).clamp(min=1e-300)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="what to call the tree in the header where it is no git checkout")
    args = ap.parse_args()
    from sanerf_hq_amd import _lib
    dev = torch.device("cuda:0")
    commit = args.commit
    if commit is None:
        try:
            commit = "commit " + subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "an unknown commit"
    with open(_lib.LIB_PATH, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    print(f"wide MLP against tests/wide_ref64.py -- {commit}, library sha256 {digest} ({os.path.getsize(_lib.LIB_PATH)} bytes), "
          f"{torch.cuda.get_device_name(0)}")
    print("\nworst |err| / bound per float kind and entry point (each asserted <= 1), and how much the bound itself says: its median over the")
    print("forward's output elements relative to the largest |output| (a bound near or above 1 pins nothing: deep nets are pinned by the exact data)")
    for c in K.FLOAT_CASES:
        print(f"  {K.case_id(c)}")
        for kind in K.FLOAT_KINDS:
            d = K.float_net(c.net, c.rows, kind)
            fwd = R.chain_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)
            loose = float(fwd["raw_bound"].median() / fwd["raw"].abs().max())
            ratios = T.float_ratios(dev, c, kind)
            print(f"    {kind:12s} bound / max|out| {loose:9.2e}   " + "  ".join(f"{e} {r:.4f}" for e, r in ratios.items()))
    print("\nLayerNorm epilogues behind an exact chain (the bound is the LayerNorm's own rounding count): worst |err| / bound, worst bound / max|out| of a row")
    for c in K.LAYER_NORM_CASES:
        ratio, out, d = T.layer_norm_ratio(dev, c)
        others = torch.arange(c.rows) != d["equal_row"]
        tight = float((d["bound"][others].amax(1) / d["want"][others].abs().amax(1)).max())
        same = bool((out[d["equal_row"]].view(torch.int32) == d["b"].view(torch.int32)).all())
        print(f"  {K.case_id(c):52s} {ratio:.4f}   {tight:.2e}   the row of equal outputs returns ln.bias bit for bit: {same}")
    print("\nworst |error| / (largest |output| of the row), against the float64 chain of the unsplit values: sn_mlp_wide_forward | torch fp32 (the baseline)")
    for kind in ("fresh_field", "all_small", "uniform"):
        for c in K.FLOAT_CASES:
            d = K.float_net(c.net, c.rows, kind)
            ref = true_chain(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)
            hip = T.hip_forward(T.DeviceNet(c.net, d["ws"], d["bs"], dev), d["x"].to(dev)).cpu()
            base = torch_forward(d["x"].to(dev), [w.to(dev) for w in d["ws"]], [b.to(dev) for b in d["bs"]] if d["bs"] else None, c.net.skip, c.net.leaky)["raw"].cpu()
            print(f"  {kind:12s} {K.case_id(c):52s} {row_relative(hip, ref):.3e} | {row_relative(base, ref):.3e}")


if __name__ == "__main__":
    main()
