#!/usr/bin/env python3
"""Time the mesh rasteriser (raymarching.mesh_rasterize) on the meshes of the other mesh tools: the synthetic head model's density lattice
at 256^3, threshold at a quantile of the volume's own values (default 0.99) -- the whole scene and the object [1], raw and after
extract_mesh(simplify=2) and (simplify=4) -- from one bench camera (synth.orbit_pose(2.2, 20, 30), 60 degrees), at 800 x 800 and at
1600 x 1600, colours and labels interpolated.

  project, resolve         the two entry points alone, HIP events around each;
  project + draw           the pair -- a draw without the projection's clear before it would append to the queue of the call before;
  k_raster_*               the launches of that pair one by one, from torch.profiler's device times (the draw's entry point issues two);
  queue                    the number of triangles the first draw kernel handed to the second, read from the workspace, and the counts;
  mesh_rasterize()         the Python call, eager and as one captured graph.
Beside them, from the same process:
  (a) copy                 a device-to-device copy of the bytes the four launches must touch at least once: 12V + 16V (rows written) +
                           12T + 16HW (depth buffer cleared and read) + the outputs;
  (b) field                NeRFRenderer.render() and render_object([1]) of the same camera and size (fused routes, unstaged);
  (c) sweep                project + draw at small_max_pixels = 0, 1, 4, 8, 16, 32, 64, 256, 1024, 2^31 - 1: what the Python default is chosen from.
  (d) clipping             the raw scene mesh at 800 x 800 with near-plane clipping (mesh_raster_draw / _resolve with clip=True) beside the
                           unclipped entries of the same build: from the bench camera, where no triangle crosses the near plane, and from
                           cameras INSIDE the mesh (orbit_pose(0.3, 20, 30) and (0.6, 20, 30)), with the counts and clip_counts.
Kernel rows: `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls.

    python tools/mesh_raster_bench.py [--size 256] [--out profiles/mesh_raster_bench.txt]
    python tools/mesh_raster_bench.py --clip             only (d), appended to --out
    python tools/mesh_raster_bench.py --ab PARENT_TREE   the UNCLIPPED entries of the checkout at PARENT_TREE (built) and of this one, three
                                                         fresh processes each, alternating, in one visit to the device; appended to --out
    python tools/mesh_raster_bench.py --unclipped [--tree T]   what --ab starts: one JSON line of the unclipped medians, the package from T

Nothing is asserted about speed; the numbers of one run are reported.  That the thresholds give equal images IS asserted.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[:-1] else ROOT     # the checkout whose package is timed
sys.path.insert(0, TREE)

from sanerf_hq_amd import raymarching as rm, synth  # noqa: E402
from sanerf_hq_amd.graph import GraphedStep  # noqa: E402
from sanerf_hq_amd.nerf import NeRFNetwork  # noqa: E402

SWEEP = (0, 1, 4, 8, 16, 32, 64, 256, 1024, (1 << 31) - 1)


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
    return f"  {name:<40} median {r['median_ms']:9.4f} ms   min {r['min_ms']:.4f}   max {r['max_ms']:.4f}{extra}"


def kernel_times(fn, calls):
    """Mean device microseconds per call of every k_raster_* kernel over `calls` calls of fn, from torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        found = {}
        for e in prof.key_averages():
            if "k_raster_" in e.key:
                name = e.key[e.key.index("k_raster_"):].split("(")[0].split("E")[0]
                total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                found[name] = found.get(name, 0.0) + total / calls
        return found or "no k_raster_ kernel in the profile"
    except Exception as e:                                 # reported, not hidden
        return f"not measured ({type(e).__name__}: {e})"


def bench_mesh(say, name, mesh, pose, intr, H, W, near, w):
    dev = mesh["vertices"].device
    vert, tri = mesh["vertices"], mesh["triangles"]
    V, T = vert.shape[0], tri.shape[0]
    colors, labels = mesh["colors"], mesh["labels"]
    out = rm.mesh_rasterize(mesh, pose, intr, H, W, near=near)
    counts = out["counts"]
    ws = rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts)
    rm.mesh_raster_draw(tri, V, H, W, ws, counts)
    queue = int(ws[:4].view(torch.int32)[0])
    say(f"\n {name} at {W} x {H}: V = {V}, T = {T}; counts (drawn, dropped, degenerate, culled) = {counts.tolist()}; "
        f"covered {float(out['mask'].float().mean()):.3f} of the image; queue at the default threshold ({rm.RASTER_SMALL_MAX_PIXELS}): {queue} triangles")
    say(line("project (+ clear)", timed(lambda: rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts), *w)))

    def pair(small=None):
        rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts)
        rm.mesh_raster_draw(tri, V, H, W, ws, counts, small_max_pixels=small)
    say(line("project + draw (three launches)", timed(pair, *w)))
    k = kernel_times(pair, 10)
    say(f"    of which, per call (profiler): {k if isinstance(k, str) else ', '.join(f'{n} {us:.1f} us' for n, us in sorted(k.items()))}")

    def resolve():
        rm.mesh_raster_resolve(tri, V, H, W, ws, out["triangle_id"], out["depth"], out["mask"], colors, out["image"], None, None, labels, out["label"], 1.0)
    say(line("resolve (colours, labels)", timed(resolve, *w)))
    call = lambda: rm.mesh_rasterize(mesh, pose, intr, H, W, near=near)      # noqa: E731
    eager = timed(call, *w)
    say(line("mesh_rasterize() eager", eager))
    say(line("mesh_rasterize() as a captured graph", timed(GraphedStep(call, warmup=2), *w)))
    nbytes = 12 * V + 16 * V + 12 * T + 16 * H * W + H * W * (4 + 4 + 1 + 12 + 1)
    src, dst = torch.empty(nbytes, device=dev, dtype=torch.uint8), torch.empty(nbytes, device=dev, dtype=torch.uint8)
    copy = timed(lambda: dst.copy_(src), *w)
    say(line(f"(a) copy of {nbytes / 1e6:.1f} MB", copy, f"   eager / copy = {eager['median_ms'] / copy['median_ms']:.1f}"))
    say("  (c) project + draw by small_max_pixels:")
    want = None
    for small in SWEEP:
        pair(small)
        q = int(ws[:4].view(torch.int32)[0])
        img = rm.mesh_rasterize(mesh, pose, intr, H, W, near=near, small_max_pixels=small)
        if want is None:
            want = img
        for key in ("triangle_id", "depth", "mask", "image", "label"):
            assert torch.equal(img[key], want[key]), (small, key)
        say(line(f"    {small:>10}: queue {q:>8}", timed(lambda: pair(small), *w)))
    return eager


def raster_phases(mesh, pose, intr, H, W, near, clip):
    """(pair, resolve, out, counts): project + draw and the resolve as callables on preallocated outputs, clipped or not."""
    vert, tri = mesh["vertices"], mesh["triangles"]
    V, T = vert.shape[0], tri.shape[0]
    out = (rm.mesh_rasterize_clip if clip else rm.mesh_rasterize)(mesh, pose, intr, H, W, near=near)
    counts = out["counts"]
    camera = dict(clip=True, vertices=vert, pose=pose, intrinsics=intr, near=near) if clip else {}
    draw_extra = dict(camera, clip_counts=out["clip_counts"]) if clip else {}
    ws = rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts)

    def pair():
        rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts)
        rm.mesh_raster_draw(tri, V, H, W, ws, counts, **draw_extra)

    def resolve():
        rm.mesh_raster_resolve(tri, V, H, W, ws, out["triangle_id"], out["depth"], out["mask"], mesh["colors"], out["image"], None, None, mesh["labels"],
                               out["label"], 1.0, **camera)
    return pair, resolve, out, counts


def bench_clip(say, mesh, cameras, intr, H, W, near, w):
    """(d): clip off and on, per camera."""
    say(f"\n==== (d) near-plane clipping: scene, raw at {W} x {H}, V = {mesh['vertices'].shape[0]}, T = {mesh['triangles'].shape[0]}, near = {near} ====")
    for name, pose in cameras:
        rows = {}
        for clip in (False, True):
            pair, resolve, out, counts = raster_phases(mesh, pose, intr, H, W, near, clip)
            pair()
            resolve()
            queue = int(_buffers_head(mesh))
            rows[clip] = (timed(pair, *w), timed(resolve, *w), counts.tolist(), out["clip_counts"].tolist() if clip else None,
                          float(out["mask"].float().mean()), queue)
        say(f"\n camera {name}: counts unclipped {rows[False][2]}, covered {rows[False][4]:.3f}, queue {rows[False][5]}; clipped {rows[True][2]}, "
            f"clip_counts (triangles cut, pieces drawn) {rows[True][3]}, covered {rows[True][4]:.3f}, queue {rows[True][5]}")
        for k, what in ((0, "project + draw"), (1, "resolve (colours, labels)")):
            off, on = rows[False][k], rows[True][k]
            say(line(f"{what}, clip off", off))
            say(line(f"{what}, clip on", on, f"   on / off = {on['median_ms'] / off['median_ms']:.3f}"))


def _buffers_head(mesh):
    """The queue's length after the last draw on this device: the first word of the module's "mesh_raster" workspace."""
    from sanerf_hq_amd import _buffers
    return _buffers.scratch("mesh_raster", mesh["vertices"].device, 16)[:4].view(torch.int32)[0]


def unclipped_medians(mesh, pose, intr, H, W, near, w):
    """The entries that exist with and without the clipped ones, through calls both checkouts have."""
    vert, tri = mesh["vertices"], mesh["triangles"]
    V, T = vert.shape[0], tri.shape[0]
    out = rm.mesh_rasterize(mesh, pose, intr, H, W, near=near)
    counts = out["counts"]
    ws = rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts)

    def pair():
        rm.mesh_raster_project(vert, T, pose, intr, H, W, near, counts)
        rm.mesh_raster_draw(tri, V, H, W, ws, counts)

    def resolve():
        rm.mesh_raster_resolve(tri, V, H, W, ws, out["triangle_id"], out["depth"], out["mask"], mesh["colors"], out["image"], None, None, mesh["labels"],
                               out["label"], 1.0)
    pair()
    return {"project_draw_ms": timed(pair, *w)["median_ms"], "resolve_ms": timed(resolve, *w)["median_ms"],
            "mesh_rasterize_ms": timed(lambda: rm.mesh_rasterize(mesh, pose, intr, H, W, near=near), *w)["median_ms"]}


def run_ab(say, parent, args):
    """--ab: three fresh processes per checkout, alternating, each printing one JSON line."""
    import json
    import subprocess
    runs = {"parent": [], "this": []}
    for _ in range(3):
        for name, tree in (("parent", parent), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--unclipped", "--size", str(args.size), "--quantile", str(args.quantile),
                   "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--rounds", str(args.rounds), "--tree", tree]
            text = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            runs[name].append(json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1]))
            print(f"  [{name}] {runs[name][-1]}", flush=True)
    say(f"\n==== the unclipped entries before and after the clipped ones were added: scene, raw at 800 x 800, one visit to the device, three fresh "
        f"processes per checkout, alternating (parent, this, parent, ...); medians of {args.rounds} rounds x {args.repeats} calls, ms ====")
    for key in ("project_draw_ms", "resolve_ms", "mesh_rasterize_ms"):
        a, b = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        med = statistics.median(b)
        verdict = "inside" if min(a) <= med <= max(a) else ("below" if med < min(a) else "ABOVE")
        say(f"  {key:<20} parent {', '.join(f'{x:.4f}' for x in a)}   this {', '.join(f'{x:.4f}' for x in b)}   this median {med:.4f}: {verdict} the "
            f"parent's spread [{min(a):.4f}, {max(a):.4f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", action="store_true", help="only (d), appended to --out")
    ap.add_argument("--ab", metavar="PARENT_TREE", help="time the unclipped entries of that built checkout and of this one; appended to --out")
    ap.add_argument("--unclipped", action="store_true", help="one JSON line of the unclipped entries' medians (what --ab starts)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported (default: this one)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--images", default="800,1600")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_raster_bench.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def write(mode):
        if args.out:
            with open(args.out, mode) as f:
                f.write("\n".join(lines) + "\n")

    if args.ab:                                            # this process starts the timed ones and never opens the device itself
        run_ab(say, os.path.abspath(args.ab), args)
        return write("a")
    if not torch.cuda.is_available():
        raise SystemExit("mesh_raster_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2, max_ray_batch=1 << 30))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    n = args.size
    w = (args.warmup, args.repeats, args.rounds)
    inside = [(f"inside, orbit_pose({r}, 20, 30)", torch.from_numpy(synth.orbit_pose(r, 20.0, 30.0)).to(dev)) for r in (0.3, 0.6)]
    if args.clip or args.unclipped:
        with torch.no_grad():
            vol = model.density_volume(n)
            iso = float(torch.quantile(vol.reshape(-1)[:: max(n ** 3 // (1 << 22), 1)], args.quantile))
            del vol
            scene = model.extract_mesh(n, threshold=iso, vertex_colors=True, vertex_labels=True)
            pose = torch.from_numpy(synth.orbit_pose(2.2, 20.0, 30.0)).to(dev)
            intr = torch.tensor(synth.pinhole_intrinsics(800, 800), device=dev, dtype=torch.float32)
            if args.unclipped:
                import json
                print(json.dumps(unclipped_medians(scene, pose, intr, 800, 800, model.min_near, w)), flush=True)
                return
            say(f"\nNear-plane clipping: tools/mesh_raster_bench.py --clip, one run on {torch.cuda.get_device_name(0)} ({n}^3 lattice, threshold {iso:.4g}; "
                f"{args.warmup} warm-up calls, {args.rounds} rounds x {args.repeats} calls; HIP events).")
            bench_clip(say, scene, [("outside, orbit_pose(2.2, 20, 30)", pose)] + inside, intr, 800, 800, model.min_near, w)
        return write("a")
    say(f"Mesh rasteriser: tools/mesh_raster_bench.py, one run on {torch.cuda.get_device_name(0)} (synthetic head model, n_inst 2; {args.warmup} "
        f"warm-up calls, {args.rounds} rounds x {args.repeats} calls; HIP events; kernel shares from torch.profiler).")
    pose_np = synth.orbit_pose(2.2, 20.0, 30.0)
    pose = torch.from_numpy(pose_np).to(dev)
    with torch.no_grad():
        vol = model.density_volume(n)
        iso = float(torch.quantile(vol.reshape(-1)[:: max(n ** 3 // (1 << 22), 1)], args.quantile))
        del vol
        say(f"{n}^3 lattice on [-1,1]^3, threshold {iso:.4g} (the {args.quantile} quantile of the volume); camera orbit_pose(2.2, 20, 30), fovy 60; "
            f"near = {model.min_near}")
        meshes = []
        for what, ids in (("scene", None), ("object [1]", [1])):
            for simplify in (0, 2, 4):
                m = model.extract_mesh(n, threshold=iso, instance_ids=ids, simplify=simplify, vertex_colors=True, vertex_labels=True)
                meshes.append((f"{what}, {'raw' if not simplify else f'simplify={simplify}'}", m))
        for side in [int(s) for s in args.images.split(",")]:
            H = W = side
            intr_t = synth.pinhole_intrinsics(H, W)
            intr = torch.tensor(intr_t, device=dev, dtype=torch.float32)
            say(f"\n==== {W} x {H} ====")
            for name, m in meshes:
                bench_mesh(say, name, m, pose, intr, H, W, model.min_near, w)
            ro, rd = rm.generate_rays(pose_np, intr_t, H, W, device=dev)
            say(f"\n (b) the field from the same camera at {W} x {H}:")
            say(line("render()", timed(lambda: model.render(ro, rd, staged=False, perturb=False, H=H, W=W), 2, 3, 3)))
            say(line("render_object([1])", timed(lambda: model.render_object(ro, rd, [1], H=H, W=W), 2, 3, 3)))
            del ro, rd
        intr = torch.tensor(synth.pinhole_intrinsics(800, 800), device=dev, dtype=torch.float32)
        bench_clip(say, meshes[0][1], [("outside, orbit_pose(2.2, 20, 30)", pose)] + inside, intr, 800, 800, model.min_near, w)
    write("w")


if __name__ == "__main__":
    main()
