#!/usr/bin/env python3
"""Time the vertex attributes of an exported mesh on the synthetic head model: the surface probes of NeRFRenderer.vertex_attributes at 256^3,
for the whole scene and for one object (instance_ids=[1]), colours and labels both asked for.

  steps            on all V vertices at once: points (sn_rm_vertex_probe_points), density (the main field at V K positions), labels (the
                   label kernel), composite (sn_rm_vertex_probe_composite), head (view_mlp.forward_sigmoid_bg);
  copy             a device-to-device copy that moves the composite's bytes (read: 64 K + K + 12 per vertex, written: 129), as GB/s of both;
  whole            vertex_attributes() as called (chunks of 2^17) beside extract_mesh() without it (wall clock: it reads totals back);
  torch chain      the composite from torch operators -- where / cumsum in fp64 / exp / weighted sums / scatter_add votes / argmax -- without
                   the SH columns (which favours the chain); its result is compared with the kernel's and the largest differences printed.

The threshold is the 0.99 quantile of the volume's own values, as tools/mesh_bench.py takes it.  HIP events (wall clock around a synchronise
for the rows that contain host reads), `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls, min and max beside them.

    python tools/mesh_attr_bench.py [--size 256] [--samples 8] [--out profiles/mesh_attr_bench.txt]

Nothing is asserted about speed; the numbers of one run are reported.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sanerf_hq_amd import raymarching as rm, synth  # noqa: E402
from sanerf_hq_amd.nerf import NeRFNetwork  # noqa: E402


def timed(fn, warmup, repeats, rounds, wall=False):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        if wall:
            t0 = time.perf_counter()
            for _ in range(repeats):
                fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / repeats)
            continue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / repeats)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def line(name, r, extra=""):
    return f"  {name:<34} median {r['median_ms']:9.3f} ms   min {r['min_ms']:.3f}   max {r['max_ms']:.3f}{extra}"


def torch_composite(sigma, geo, labels, h, keep_mask, invert):
    """Steps 4-8 of the definition from torch operators (no SH): (g [V,15], coverage [V], vertex_label [V] uint8)."""
    lab = labels.long()
    in_set = (lab < 32) & (((torch.tensor(int(keep_mask), dtype=torch.int64, device=lab.device) >> lab.clamp(max=31)) & 1) != 0)
    y = torch.where(in_set != invert, h * sigma, torch.zeros_like(sigma))
    excl = torch.cat([torch.zeros_like(y[:, :1], dtype=torch.float64), torch.cumsum(y.double(), dim=-1)[:, :-1]], dim=-1)
    w = ((1.0 - torch.exp(-y)) * torch.exp(-excl.float())).nan_to_num(0.0)
    W = w.sum(-1)
    G = (w.unsqueeze(-1) * geo).sum(1)
    g = torch.where((W >= 2.0 ** -126).unsqueeze(-1), G / W.unsqueeze(-1), geo.sum(1) * (1.0 / sigma.shape[1]))
    votes = torch.zeros(sigma.shape[0], 33, device=sigma.device).scatter_add_(1, lab.clamp(max=32), w)[:, :32]
    top, arg = votes.max(-1)
    return g, W, torch.where(top > 0, arg, torch.full_like(arg, 255)).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--probe-step", type=float, default=0.5)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_attr_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_attr_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    n, K = args.size, args.samples
    W, R, Q = args.warmup, args.repeats, args.rounds
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    say(f"Vertex attributes: tools/mesh_attr_bench.py, one run on {torch.cuda.get_device_name(0)} (synthetic head model, n_inst 2; {W} warm-up "
        f"calls, {Q} rounds x {R} calls; HIP events, wall clock around a synchronize for the rows marked (wall)).")
    with torch.no_grad():
        vol = model.density_volume(n)
        _, origin, step = model._lattice(n, None)
        total = n ** 3
        iso = float(torch.quantile(vol.reshape(-1)[:: max(total // (1 << 22), 1)], args.quantile))
        del vol
        h = args.probe_step * min(step)
        say(f"{n}^3 lattice on [-1,1]^3, threshold {iso:.4g} (the {args.quantile} quantile of the volume); K = {K} samples, h = {args.probe_step} "
            f"lattice steps = {h:.6g}")
        for name, ids in (("whole scene", None), ("object [1]", [1])):
            mesh = model.extract_mesh(n, threshold=iso, instance_ids=ids)
            v, nr = mesh["vertices"], mesh["normals"]
            V = v.shape[0]
            say(f"\n{name}: V = {V}, T = {mesh['triangles'].shape[0]}; {V * K} probe samples")
            keep = 0xFFFFFFFF if ids is None else rm.keep_mask_of(ids)
            contract = bool(model.opt.contract)
            xyz, dirs = rm.vertex_probe_points(v, nr, K, h, contract=contract)
            flat = xyz.reshape(-1, 3)
            field = model.density(flat)
            sigma, geo = field["sigma"].reshape(V, K).float(), field["geo_feat"].reshape(V, K, -1).contiguous()
            labels = model._point_labels(sigma, xyz, geo)
            f, cov, vl = rm.vertex_probe_composite(sigma, geo, dirs, h, labels, keep, False, want_labels=True)
            ones = torch.ones_like(cov)
            r = {}
            r["points"] = timed(lambda: rm.vertex_probe_points(v, nr, K, h, contract=contract), W, R, Q)
            r["density"] = timed(lambda: model.density(flat), W, R, Q)
            r["labels"] = timed(lambda: model._point_labels(sigma, xyz, geo), W, R, Q)
            r["composite"] = timed(lambda: rm.vertex_probe_composite(sigma, geo, dirs, h, labels, keep, False, want_labels=True), W, R, Q)
            r["head"] = timed(lambda: model.view_mlp.forward_sigmoid_bg(f, ones, 0.0), W, R, Q)
            nbytes = V * (64 * K + K + 12) + V * (31 * 4 + 4 + 1)
            src = torch.empty(nbytes // 2, device=dev, dtype=torch.uint8)
            dst = torch.empty_like(src)
            r["copy"] = timed(lambda: dst.copy_(src), W, R, Q)
            del src, dst
            for k in ("points", "density", "labels", "composite", "head"):
                extra = f"   {nbytes / (r[k]['median_ms'] * 1e-3) / 1e9:.0f} GB/s of its {nbytes} bytes read + written" if k == "composite" else ""
                say(line(k, r[k], extra))
            say(line("copy of the composite's bytes", r["copy"], f"   {nbytes / (r['copy']['median_ms'] * 1e-3) / 1e9:.0f} GB/s read + written; "
                     f"composite / copy = {r['composite']['median_ms'] / r['copy']['median_ms']:.2f}"))
            say(f"  sum of the five medians {sum(r[k]['median_ms'] for k in ('points', 'density', 'labels', 'composite', 'head')):.3f} ms")
            r["attr"] = timed(lambda: model.vertex_attributes(mesh, h, samples=K, instance_ids=ids, labels=True), W, R, Q)
            r["attr_colors"] = timed(lambda: model.vertex_attributes(mesh, h, samples=K), W, R, Q)
            r["extract"] = timed(lambda: model.extract_mesh(n, threshold=iso, instance_ids=ids), 1, 1, 3, wall=True)
            say(line("vertex_attributes(labels=True)", r["attr"]))
            say(line("vertex_attributes(), colours only", r["attr_colors"]))
            say(line("extract_mesh() without (wall)", r["extract"], f"   vertex_attributes / extract_mesh = "
                     f"{r['attr']['median_ms'] / r['extract']['median_ms']:.3f}"))
            r["chain"] = timed(lambda: torch_composite(sigma, geo, labels, h, keep, False), W, R, Q)
            g2, W2, l2 = torch_composite(sigma, geo, labels, h, keep, False)
            say(line("torch chain of the composite", r["chain"], f"   composite / chain = {r['composite']['median_ms'] / r['chain']['median_ms']:.3f}; "
                     f"vertex_attributes with the chain in its place would take {r['attr']['median_ms'] - r['composite']['median_ms'] + r['chain']['median_ms']:.3f} ms"))
            say(f"    chain against kernel: max |g| diff {float((g2 - f[:, :15]).abs().max()):.3e}, max |coverage| diff {float((W2 - cov).abs().max()):.3e}, "
                f"labels differ on {int((l2 != vl).sum())} of {V} vertices")
            del mesh, xyz, flat, field, sigma, geo, labels, f, cov, vl
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
