#!/usr/bin/env python3
"""Time the geometry export on the synthetic head model: the density lattice (whole scene, and one object through the label gate) and the
marching-tetrahedra extraction, at 256^3 and 512^3.

  density_volume   model.density_volume(n) and model.density_volume(n, instance_ids=[1]): chunks of 2^20 lattice vertices through
                   sn_rm_lattice_points -> the field -> (the label kernel);
  count            sn_rm_isosurface_count alone (classify + rank + scan: reads the volume, writes 5 bytes per lattice vertex);
  emit             sn_rm_isosurface_emit alone into exactly sized outputs (reads 1 byte per lattice vertex and the volume on crossing
                   edges, writes 24 bytes per mesh vertex and 12 per triangle);
  copy             a device-to-device copy of the same volume: the measured floor of anything that reads the volume once.

The threshold is a quantile of the volume's own values (`--quantile`, default 0.99: the synthetic field is noise, a trained scene's surface
is far sparser than the median level set of noise).  GB/s of the extraction = (volume read + vertices, normals and triangles written) over
count + emit.  HIP events, `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls.

    python tools/mesh_bench.py [--sizes 256,512] [--out profiles/mesh_bench.json]

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
from sanerf_hq_amd.nerf import NeRFNetwork  # noqa: E402


def timed(fn, warmup, repeats, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / repeats)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def line(name, r, extra=""):
    return f"  {name:<28} median {r['median_ms']:9.3f} ms   min {r['min_ms']:.3f}   max {r['max_ms']:.3f}{extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    res = {"what": "density lattice and marching-tetrahedra extraction on the synthetic head model", "device": torch.cuda.get_device_name(0),
           "quantile": args.quantile, "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds, "sizes": {}}
    print(f"Geometry export: tools/mesh_bench.py, one {res['device']} run (synthetic head model, n_inst 2; {args.warmup} warm-up calls, "
          f"{args.rounds} rounds x {args.repeats} calls; HIP events).")
    with torch.no_grad():
        for n in [int(s) for s in args.sizes.split(",")]:
            r = res["sizes"][str(n)] = {}
            total = n ** 3
            print(f"\n{n}^3 lattice on [-1,1]^3: {total} field queries, volume {total * 4 / 1e6:.1f} MB")
            r["density_scene"] = timed(lambda: model.density_volume(n), 1, 1, 3)
            r["density_object"] = timed(lambda: model.density_volume(n, instance_ids=[1]), 1, 1, 3)
            print(line("density_volume, scene", r["density_scene"], f"   {total / r['density_scene']['median_ms'] / 1e6:.2f} G queries/s"))
            print(line("density_volume, object [1]", r["density_object"], f"   {total / r['density_object']['median_ms'] / 1e6:.2f} G queries/s"))
            vol = model.density_volume(n)
            _, origin, step = model._lattice(n, None)
            sample = vol.reshape(-1)[:: max(total // (1 << 22), 1)]
            iso = float(torch.quantile(sample, args.quantile))
            mesh = rm.isosurface(vol, iso, origin, step)
            V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
            r.update(iso=iso, vertices=V, triangles=T)
            print(f"  threshold {iso:.4g} (the {args.quantile} quantile of the volume): V = {V}, T = {T}")
            ws = rm.isosurface_counts(vol, iso)[1]
            r["count"] = timed(lambda: rm.isosurface_counts(vol, iso), args.warmup, args.repeats, args.rounds)
            rm.isosurface_counts(vol, iso)
            vert, nrm, tri = mesh["vertices"], mesh["normals"], mesh["triangles"]
            r["emit"] = timed(lambda: rm.isosurface_emit(vol, iso, origin, step, ws, vert, nrm, tri), args.warmup, args.repeats, args.rounds)
            r["emit_no_normals"] = timed(lambda: rm.isosurface_emit(vol, iso, origin, step, ws, vert, None, tri), args.warmup, args.repeats, args.rounds)
            dst = torch.empty_like(vol)
            r["copy"] = timed(lambda: dst.copy_(vol), args.warmup, args.repeats, args.rounds)
            del dst
            nbytes = total * 4 + V * 24 + T * 12
            both = r["count"]["median_ms"] + r["emit"]["median_ms"]
            r.update(extraction_bytes=nbytes, extraction_ms=both, extraction_GB_per_s=nbytes / (both * 1e-3) / 1e9,
                     copy_GB_per_s=total * 8 / (r["copy"]["median_ms"] * 1e-3) / 1e9, ratio_to_copy=both / r["copy"]["median_ms"])
            print(line("count", r["count"]))
            print(line("emit", r["emit"]))
            print(line("emit, no normals", r["emit_no_normals"]))
            print(line("copy (device to device)", r["copy"], f"   {r['copy_GB_per_s']:.0f} GB/s read + written"))
            print(f"  extraction (count + emit) {both:.3f} ms for {nbytes} bytes (volume read + outputs written): {r['extraction_GB_per_s']:.0f} GB/s; "
                  f"{r['ratio_to_copy']:.2f} x the copy")
            del vol, mesh, vert, nrm, tri
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
