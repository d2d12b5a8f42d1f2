#!/usr/bin/env python3
"""Time the mesh simplification (uniform vertex clustering) on the meshes of tools/mesh_bench.py: the synthetic head model's density
lattice at 256^3 and 512^3, threshold at a quantile of the volume's own values (default 0.99), cells of 2 and 4 lattice steps aligned with
the extraction's lattice (the lattice NeRFRenderer.extract_mesh(simplify=k) uses).

  count            sn_rm_mesh_simplify_count: two memsets + six launches (keys, insert, keep, rank cells, scan, accumulate);
  emit             sn_rm_mesh_simplify_emit into exactly sized outputs, cluster map included: three launches;
  mesh_simplify    the Python call as users make it: count + one read of {V', T'} + allocation + emit.
Baselines from the same process, on the same mesh:
  (a) isosurface   sn_rm_isosurface_count + _emit on the volume;
  (b) mesh_clean   the Python call, min_triangles = 100;
  (c) torch        the same cluster keys and per-cluster mean positions out of torch operators: the keys in fp32 as the definition has
                   them, torch.unique(keys, return_inverse=True), index_add_ of the positions and of ones, a division.  For scale only: it
                   does none of the triangle work (classes, duplicates, the used cells), and its float sums are not order-independent.
Kernel rows: HIP events, `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls.  Rows that contain host reads
(mesh_simplify, mesh_clean, torch -- torch.unique synchronises): wall clock around a synchronize, the same counts.
`--trace-only` runs mesh_simplify() four times per case (the first also gives the sizes) and nothing else: the run to put under a kernel trace for per-launch times.

    python tools/mesh_simplify_bench.py [--sizes 256,512] [--cells 2,4] [--out profiles/mesh_simplify_bench.json]

Nothing is asserted about speed; the numbers of one run are reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sanerf_hq_amd import _lib, raymarching as rm, synth  # noqa: E402
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


def timed_wall(fn, warmup, repeats, rounds):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / repeats)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def line(name, r, extra=""):
    return f"  {name:<34} median {r['median_ms']:9.3f} ms   min {r['min_ms']:.3f}   max {r['max_ms']:.3f}{extra}"


def aligned_lattice(res, origin, step, k):
    """The cells of extract_mesh(simplify=k): cell = k step, origin = lattice origin - step / 2, dims covering the lattice."""
    return ([float(np.float32(origin[a]) - np.float32(0.5) * np.float32(step[a])) for a in range(3)],
            [float(np.float32(k * step[a])) for a in range(3)], [int((res[a] - 0.5) // k) + 2 for a in range(3)])


def torch_clusters(vertices, origin, cell, dims):
    """Cluster keys and mean positions out of torch operators.  -> (unique keys, mean positions [n,3])."""
    o = torch.tensor(origin, device=vertices.device)
    c = torch.tensor(cell, device=vertices.device)
    i = torch.floor((vertices - o) / c).long()
    keys = (i[:, 0] * dims[1] + i[:, 1]) * dims[2] + i[:, 2]
    uniq, inverse = torch.unique(keys, return_inverse=True)
    sums = torch.zeros(uniq.shape[0], 3, device=vertices.device).index_add_(0, inverse, vertices)
    n = torch.zeros(uniq.shape[0], device=vertices.device).index_add_(0, inverse, torch.ones_like(vertices[:, 0]))
    return uniq, sums / n[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--cells", default="2,4")
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--min-triangles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    w = (args.warmup, args.repeats, args.rounds)
    res = {"what": "mesh simplification on the synthetic head model's isosurface", "device": torch.cuda.get_device_name(0), "quantile": args.quantile,
           "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds, "sizes": {}}
    print(f"Mesh simplification: tools/mesh_simplify_bench.py, one {res['device']} run (synthetic head model, n_inst 2; {args.warmup} warm-up calls, "
          f"{args.rounds} rounds x {args.repeats} calls; HIP events for kernel rows, wall clock for rows with host reads).")
    with torch.no_grad():
        for n in [int(s) for s in args.sizes.split(",")]:
            r = res["sizes"][str(n)] = {"cells": {}}
            total = n ** 3
            vol = model.density_volume(n)
            shape, origin, step = model._lattice(n, None)
            iso = float(torch.quantile(vol.reshape(-1)[:: max(total // (1 << 22), 1)], args.quantile))
            mesh = rm.isosurface(vol, iso, origin, step)
            vert, nrm, tri = mesh["vertices"], mesh["normals"], mesh["triangles"]
            V, T = vert.shape[0], tri.shape[0]
            print(f"\n{n}^3 lattice, threshold {iso:.4g} (the {args.quantile} quantile): V = {V}, T = {T}")
            r.update(iso=iso, vertices=V, triangles=T)
            if not args.trace_only:
                iws = rm.isosurface_counts(vol, iso)[1]
                r["iso_count"] = timed(lambda: rm.isosurface_counts(vol, iso), *w)
                rm.isosurface_counts(vol, iso)
                r["iso_emit"] = timed(lambda: rm.isosurface_emit(vol, iso, origin, step, iws, vert, nrm, tri), *w)
                extraction = r["iso_count"]["median_ms"] + r["iso_emit"]["median_ms"]
                r["mesh_clean"] = timed_wall(lambda: rm.mesh_clean(mesh, min_triangles=args.min_triangles), *w)
                r["extraction_ms"] = extraction
                print(line("(a) isosurface count + emit", {"median_ms": extraction, "min_ms": r["iso_count"]["min_ms"] + r["iso_emit"]["min_ms"],
                                                          "max_ms": r["iso_count"]["max_ms"] + r["iso_emit"]["max_ms"]}))
                print(line(f"(b) mesh_clean() (wall), min {args.min_triangles}", r["mesh_clean"]))
            for k in [float(s) for s in args.cells.split(",")]:
                c = r["cells"][str(k)] = {}
                o, cell, dims = aligned_lattice(shape, origin, step, k)
                out = rm.mesh_simplify(mesh, cell, origin=o, dims=dims, return_cluster=True)
                nv, nt = out["vertices"].shape[0], out["triangles"].shape[0]
                ws_bytes = int(_lib.lib().sn_rm_mesh_simplify_workspace_bytes(V, T, dims[0] * dims[1] * dims[2]))
                c.update(kept_vertices=nv, kept_triangles=nt, dims=dims, workspace_bytes=ws_bytes)
                print(f" cell = {k:g} steps ({dims[0]} x {dims[1]} x {dims[2]} cells): V' = {nv} ({nv / V:.3f} V), T' = {nt} ({nt / T:.3f} T); "
                      f"workspace {ws_bytes / 2 ** 20:.1f} MiB")
                if args.trace_only:
                    for _ in range(3):
                        rm.mesh_simplify(mesh, cell, origin=o, dims=dims, return_cluster=True)
                    torch.cuda.synchronize()
                    continue
                c["count"] = timed(lambda: rm.mesh_simplify_counts(vert, nrm, tri, o, cell, dims), *w)
                _, ws = rm.mesh_simplify_counts(vert, nrm, tri, o, cell, dims)
                ov, on, ot = torch.empty(nv, 3, device=dev), torch.empty(nv, 3, device=dev), torch.empty(nt, 3, device=dev, dtype=torch.int32)
                oc = torch.empty(V, device=dev, dtype=torch.int32)
                c["emit"] = timed(lambda: rm.mesh_simplify_emit(vert, nrm, tri, o, cell, dims, ws, ov, on, ot, oc), *w)
                assert torch.equal(ov, out["vertices"]) and torch.equal(ot, out["triangles"]) and torch.equal(oc, out["vertex_cluster"])
                c["mesh_simplify"] = timed_wall(lambda: rm.mesh_simplify(mesh, cell, origin=o, dims=dims, return_cluster=True), *w)
                uniq, mean = torch_clusters(vert, o, cell, dims)
                c["torch_clusters"] = timed_wall(lambda: torch_clusters(vert, o, cell, dims), *w)
                kernels = c["count"]["median_ms"] + c["emit"]["median_ms"]
                c.update(kernels_ms=kernels, torch_cells=int(uniq.shape[0]), simplify_over_extraction=c["mesh_simplify"]["median_ms"] / extraction,
                         simplify_over_clean=c["mesh_simplify"]["median_ms"] / r["mesh_clean"]["median_ms"],
                         simplify_over_torch=c["mesh_simplify"]["median_ms"] / c["torch_clusters"]["median_ms"])
                print(line("count", c["count"]))
                print(line("emit", c["emit"]))
                print(f"  count + emit, sum of the medians   {kernels:9.3f} ms")
                print(line("mesh_simplify() (wall)", c["mesh_simplify"]))
                print(line("(c) torch keys + unique + index_add", c["torch_clusters"], f"   {int(uniq.shape[0])} occupied cells (all vertices' cells, used or not)"))
                print(f"  mesh_simplify() / (a) = {c['simplify_over_extraction']:.2f}   / (b) = {c['simplify_over_clean']:.2f}   / (c) = {c['simplify_over_torch']:.3f}")
            del vol, mesh, vert, nrm, tri
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
