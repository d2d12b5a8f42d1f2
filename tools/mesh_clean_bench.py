#!/usr/bin/env python3
"""Time the mesh clean-up (connected components, statistics, floater removal) on the meshes of tools/mesh_bench.py: the synthetic head
model's density lattice at 256^3 and 512^3, threshold at a quantile of the volume's own values (default 0.99).

  sweep            sn_rm_mesh_components_init + ONE sn_rm_mesh_components_sweep call of exactly the rounds the mesh needs (what
                   mesh_components() found, the confirming round included): the kernels alone, per round = total / rounds;
  stats            sn_rm_mesh_component_stats;
  filter count     sn_rm_mesh_filter_count (min_triangles = 100);   filter emit: sn_rm_mesh_filter_emit into exactly sized outputs;
  mesh_components  the Python call as users make it: rounds in batches of 4, the 4 flags read back after each batch, then the stats;
  mesh_clean       the Python call: mesh_components + count + one read of {V', T'} + allocation + emit.
Baselines from the same process:
  (a) isosurface   sn_rm_isosurface_count + _emit on the same volume;
  (b) density      model.density_volume(n), the fill the export starts with;
  (c) torch        the same labels by a device torch route: per round two scatter_reduce_("amin") (corner and corner's label) and a
                   gather loop l = l[l], every convergence test a torch.equal (a host read); checked equal to the library's labels.
Kernel-only rows: HIP events, `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls.  Rows that contain host reads
(mesh_components, mesh_clean, torch): wall clock around a synchronize, the same counts.

    python tools/mesh_clean_bench.py [--sizes 256,512] [--out profiles/mesh_clean_bench.json]

Nothing is asserted about speed; the numbers of one run are reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def torch_labels(triangles, V):
    """The hook-and-jump round out of torch operators; every convergence test is a torch.equal.  -> (labels int64, rounds)."""
    tri = triangles.long()
    tri = tri[((tri >= 0) & (tri < V)).all(dim=1)]
    flat = tri.reshape(-1)
    lab = torch.arange(V, device=triangles.device)
    rounds = 0
    while True:
        lt = lab[tri]
        m = lt.amin(dim=1).repeat_interleave(3)
        new = lab.clone()
        new.scatter_reduce_(0, flat, m, "amin")
        new.scatter_reduce_(0, lt.reshape(-1), m, "amin")
        while True:
            nxt = new[new]
            if torch.equal(nxt, new):
                break
            new = nxt
        rounds += 1
        if torch.equal(new, lab):
            return lab, rounds
        lab = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--min-triangles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    L = _lib.lib()
    w = (args.warmup, args.repeats, args.rounds)
    res = {"what": "mesh clean-up on the synthetic head model's isosurface", "device": torch.cuda.get_device_name(0), "quantile": args.quantile,
           "min_triangles": args.min_triangles, "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds, "sizes": {}}
    print(f"Mesh clean-up: tools/mesh_clean_bench.py, one {res['device']} run (synthetic head model, n_inst 2; {args.warmup} warm-up calls, "
          f"{args.rounds} rounds x {args.repeats} calls; HIP events for kernel rows, wall clock for rows with host reads).")
    with torch.no_grad():
        for n in [int(s) for s in args.sizes.split(",")]:
            r = res["sizes"][str(n)] = {}
            total = n ** 3
            r["density"] = timed(lambda: model.density_volume(n), 1, 1, 3)
            vol = model.density_volume(n)
            _, origin, step = model._lattice(n, None)
            iso = float(torch.quantile(vol.reshape(-1)[:: max(total // (1 << 22), 1)], args.quantile))
            mesh = rm.isosurface(vol, iso, origin, step)
            vert, nrm, tri = mesh["vertices"], mesh["normals"], mesh["triangles"]
            V, T = vert.shape[0], tri.shape[0]
            comp = rm.mesh_components(tri, V)
            R = comp["rounds"]
            roots, with_tri = comp["counts"].tolist()
            largest = int(comp["triangle_counts"].max())
            print(f"\n{n}^3 lattice, threshold {iso:.4g} (the {args.quantile} quantile): V = {V}, T = {T}; {with_tri} components, the largest "
                  f"{largest} triangles; rounds {R} (the confirming one included)")
            r.update(iso=iso, vertices=V, triangles=T, components=with_tri, largest=largest, component_rounds=R)
            # ---- kernels alone
            st = _lib.stream()
            labels = torch.empty(V, device=dev, dtype=torch.int32)
            changed = torch.empty(R, device=dev, dtype=torch.int32)

            def sweep():
                _lib.check(L.sn_rm_mesh_components_init(V, labels.data_ptr(), st))
                _lib.check(L.sn_rm_mesh_components_sweep(tri.data_ptr(), T, V, labels.data_ptr(), R, changed.data_ptr(), st))

            r["init"] = timed(lambda: _lib.check(L.sn_rm_mesh_components_init(V, labels.data_ptr(), st)), *w)
            r["sweep"] = timed(sweep, *w)
            assert torch.equal(labels, comp["labels"]) and changed.tolist()[-1] == 0
            tc, vc, cnt = torch.empty_like(labels), torch.empty_like(labels), torch.empty(2, device=dev, dtype=torch.int32)
            r["stats"] = timed(lambda: _lib.check(L.sn_rm_mesh_component_stats(tri.data_ptr(), T, V, labels.data_ptr(), tc.data_ptr(), vc.data_ptr(),
                                                                                cnt.data_ptr(), st)), *w)
            assert torch.equal(tc, comp["triangle_counts"])
            r["filter_count"] = timed(lambda: rm.mesh_filter_counts(tri, V, comp, args.min_triangles), *w)
            counts, ws = rm.mesh_filter_counts(tri, V, comp, args.min_triangles)
            nv, nt = counts.tolist()
            ov, on, ot = torch.empty(nv, 3, device=dev), torch.empty(nv, 3, device=dev), torch.empty(nt, 3, device=dev, dtype=torch.int32)
            r["filter_emit"] = timed(lambda: rm.mesh_filter_emit(tri, vert, nrm, ws, ov, on, ot), *w)
            r.update(kept_vertices=nv, kept_triangles=nt)
            per_round = (r["sweep"]["median_ms"] - r["init"]["median_ms"]) / R
            kernels = r["sweep"]["median_ms"] + r["stats"]["median_ms"] + r["filter_count"]["median_ms"] + r["filter_emit"]["median_ms"]
            r.update(sweep_per_round_ms=per_round, kernels_ms=kernels)
            print(line("init", r["init"]))
            print(line(f"init + sweep, {R} rounds", r["sweep"], f"   {per_round:.3f} ms per round"))
            print(line("stats", r["stats"]))
            print(line(f"filter count (min_triangles {args.min_triangles})", r["filter_count"], f"   keeps V' = {nv}, T' = {nt}"))
            print(line("filter emit", r["filter_emit"]))
            print(f"  kernels, sum of the medians        {kernels:9.3f} ms")
            # ---- the calls as users make them
            r["mesh_components"] = timed_wall(lambda: rm.mesh_components(tri, V), *w)
            r["mesh_clean"] = timed_wall(lambda: rm.mesh_clean(mesh, min_triangles=args.min_triangles), *w)
            print(line("mesh_components() (wall)", r["mesh_components"], f"   {-(-R // 4)} batch(es) of 4 rounds, a flag read after each"))
            print(line("mesh_clean() (wall)", r["mesh_clean"]))
            # ---- baselines
            iws = rm.isosurface_counts(vol, iso)[1]
            r["iso_count"] = timed(lambda: rm.isosurface_counts(vol, iso), *w)
            rm.isosurface_counts(vol, iso)
            r["iso_emit"] = timed(lambda: rm.isosurface_emit(vol, iso, origin, step, iws, vert, nrm, tri), *w)
            extraction = r["iso_count"]["median_ms"] + r["iso_emit"]["median_ms"]
            tl, tr = torch_labels(tri, V)
            assert torch.equal(tl.int(), comp["labels"]), "the torch route's labels differ"
            r["torch_labels"] = timed_wall(lambda: torch_labels(tri, V), *w)
            r.update(extraction_ms=extraction, torch_rounds=tr)
            clean = r["mesh_clean"]["median_ms"]
            r.update(clean_over_density=clean / r["density"]["median_ms"], kernels_over_density=kernels / r["density"]["median_ms"],
                     clean_over_extraction=clean / extraction, components_over_torch=r["mesh_components"]["median_ms"] / r["torch_labels"]["median_ms"],
                     sweep_over_torch=r["sweep"]["median_ms"] / r["torch_labels"]["median_ms"])
            print(line("(a) isosurface count + emit", {"median_ms": extraction, "min_ms": r["iso_count"]["min_ms"] + r["iso_emit"]["min_ms"],
                                                      "max_ms": r["iso_count"]["max_ms"] + r["iso_emit"]["max_ms"]}))
            print(line("(b) density_volume", r["density"]))
            print(line(f"(c) torch labels, {tr} rounds (wall)", r["torch_labels"], "   labels equal to the library's"))
            print(f"  mesh_clean() / (b) = {r['clean_over_density']:.4f}   kernels / (b) = {r['kernels_over_density']:.4f}   mesh_clean() / (a) = "
                  f"{r['clean_over_extraction']:.2f}")
            print(f"  mesh_components() / (c) = {r['components_over_torch']:.3f}   init + sweep kernels / (c) = {r['sweep_over_torch']:.3f}")
            del vol, mesh, vert, nrm, tri, comp, labels, tc, vc, ov, on, ot, tl
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
