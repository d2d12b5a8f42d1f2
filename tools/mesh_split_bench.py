#!/usr/bin/env python3
"""Time the split of a labelled scene mesh into per-instance meshes on the synthetic head model: raymarching.mesh_split at 256^3, on the
mesh as extracted and after simplify=2, labels from vertex_attributes (extract_mesh(vertex_labels=True)).

  count, emit      sn_rm_mesh_split_count (a memset and three launches) and sn_rm_mesh_split_emit (two launches) into buffers of the exact
                   size, sources included;
  mesh_split()     the Python call as a user makes it: count, one read of the two totals, the allocations, emit, one read of the offsets,
                   the views (wall clock: it reads back);
  torch route      the same parts from torch operators: the vote by comparisons and where, then per part that occurs a boolean mask over the
                   triangles, torch.unique of the part's indices (its members, sorted) and torch.searchsorted for the local indices, and
                   the gathers of vertices and normals; its parts are compared with mesh_split's;
  copy             a device-to-device copy that moves the bytes the split has to read and write -- the mesh and its labels in (25 per
                   vertex, 12 per triangle), the packed result and its sources out (28 per vertex row, 16 per triangle row) -- as GB/s;
  per instance     the route the split replaces: one extract_mesh(instance_ids=[k]) per instance id that occurs, each a full pass of the
                   density lattice through the field and the mask head (wall clock), beside the ONE labelled extraction + mesh_split().

The threshold is the 0.99 quantile of the volume's own values, as tools/mesh_bench.py takes it.  HIP events (wall clock around a synchronise
for the rows that contain host reads), `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls, min and max beside them.

    python tools/mesh_split_bench.py [--size 256] [--out profiles/mesh_split_bench.txt]

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

P = rm.MESH_SPLIT_PARTS


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


def torch_split(mesh, labels):
    """{part: mesh} from torch operators.  The triangles are taken as valid (an extracted mesh's are)."""
    tri = mesh["triangles"].long()
    part = labels.long().clamp(max=P - 1)[tri]
    a, b, c = part[:, 0], part[:, 1], part[:, 2]
    tp = torch.where((a == b) | (a == c), a, torch.where(b == c, b, torch.minimum(a, torch.minimum(b, c))))
    parts = {}
    for p in torch.unique(tp).tolist():
        t = tri[tp == p]
        members = torch.unique(t)
        parts[p] = {"vertices": mesh["vertices"][members], "normals": mesh["normals"][members],
                    "triangles": torch.searchsorted(members, t).to(torch.int32)}
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_split_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_split_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    n = args.size
    W, R, Q = args.warmup, args.repeats, args.rounds
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    say(f"Mesh split: tools/mesh_split_bench.py, one run on {torch.cuda.get_device_name(0)} (synthetic head model, n_inst 2; {W} warm-up "
        f"calls, {Q} rounds x {R} calls; HIP events, wall clock around a synchronize for the rows marked (wall)).")
    with torch.no_grad():
        vol = model.density_volume(n)
        total = n ** 3
        iso = float(torch.quantile(vol.reshape(-1)[:: max(total // (1 << 22), 1)], args.quantile))
        del vol
        say(f"{n}^3 lattice on [-1,1]^3, threshold {iso:.4g} (the {args.quantile} quantile of the volume); labels from "
            f"extract_mesh(vertex_labels=True)")
        for name, kw in (("as extracted", {}), ("after simplify=2", {"simplify": 2})):
            mesh = model.extract_mesh(n, threshold=iso, vertex_labels=True, **kw)
            v, nr, tri, lab = mesh["vertices"], mesh["normals"], mesh["triangles"], mesh["labels"]
            V, T = v.shape[0], tri.shape[0]
            full = rm.mesh_split(mesh, return_source=True)
            nv, nt = full["vertices"].shape[0], full["triangles"].shape[0]
            sizes = {p: (m["vertices"].shape[0], m["triangles"].shape[0]) for p, m in full["parts"].items()}
            say(f"\n{name}: V = {V}, T = {T} -> V' = {nv} ({nv - V} seam rows), T' = {nt}; parts (vertices, triangles): {sizes}")
            ov, on, ot = torch.empty_like(full["vertices"]), torch.empty_like(full["normals"]), torch.empty_like(full["triangles"])
            sv, st = torch.empty_like(full["source_vertex"]), torch.empty_like(full["source_triangle"])
            _, _, ws = rm.mesh_split_counts(tri, V, lab)
            r = {}
            r["count"] = timed(lambda: rm.mesh_split_counts(tri, V, lab), W, R, Q)
            r["emit"] = timed(lambda: rm.mesh_split_emit(tri, v, nr, ws, ov, on, ot, sv, st), W, R, Q)
            assert torch.equal(ov, full["vertices"]) and torch.equal(ot, full["triangles"]) and torch.equal(sv, full["source_vertex"])
            r["split"] = timed(lambda: rm.mesh_split(mesh, return_source=True), W, R, Q, wall=True)
            r["torch"] = timed(lambda: torch_split(mesh, lab), W, R, Q, wall=True)
            nbytes = 25 * V + 12 * T + 28 * nv + 16 * nt
            src = torch.empty(nbytes // 2, device=dev, dtype=torch.uint8)
            dst = torch.empty_like(src)
            r["copy"] = timed(lambda: dst.copy_(src), W, R, Q)
            del src, dst
            both = r["count"]["median_ms"] + r["emit"]["median_ms"]
            say(line("count", r["count"]))
            say(line("emit", r["emit"], f"   count + emit = {both:.3f} ms = {nbytes / (both * 1e-3) / 1e9:.0f} GB/s of the {nbytes} bytes in and out"))
            say(line("copy of those bytes", r["copy"], f"   {nbytes / (r['copy']['median_ms'] * 1e-3) / 1e9:.0f} GB/s read + written; "
                     f"(count + emit) / copy = {both / r['copy']['median_ms']:.2f}"))
            say(line("mesh_split() (wall)", r["split"]))
            say(line("torch route (wall)", r["torch"], f"   mesh_split / torch = {r['split']['median_ms'] / r['torch']['median_ms']:.3f}"))
            other = torch_split(mesh, lab)
            same = sorted(other) == sorted(full["parts"]) and all(torch.equal(other[p][k], full["parts"][p][k]) for p in other
                                                                  for k in ("vertices", "normals", "triangles"))
            say(f"    torch route against mesh_split: parts {sorted(other)}, {'equal on every array' if same else 'DIFFERENT'}")
            if not kw:
                ids = [p for p in full["parts"] if p < P - 1]
                r["labelled"] = timed(lambda: model.extract_mesh(n, threshold=iso, vertex_labels=True), 1, 1, 3, wall=True)
                r["per_instance"] = timed(lambda: [model.extract_mesh(n, threshold=iso, instance_ids=[k]) for k in ids], 1, 1, 3, wall=True)
                r["objects"] = timed(lambda: model.extract_object_meshes(resolution=n, threshold=iso), 1, 1, 3, wall=True)
                say(line("extract_mesh(vertex_labels) (wall)", r["labelled"]))
                say(line("extract_object_meshes() (wall)", r["objects"], f"   of which mesh_split() {r['split']['median_ms']:.3f} ms"))
                say(line(f"{len(ids)} x extract_mesh(instance_ids=[k])", r["per_instance"],
                         f"   (wall) = {r['per_instance']['median_ms'] / len(ids):.3f} ms per instance; extract_object_meshes / this = "
                         f"{r['objects']['median_ms'] / r['per_instance']['median_ms']:.3f} at {len(ids)} instances"))
            del mesh, full, ov, on, ot, sv, st
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
