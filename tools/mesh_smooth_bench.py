#!/usr/bin/env python3
"""Time the mesh smoothing (Taubin steps in fixed point, geometric normals) on the meshes of tools/mesh_bench.py: the synthetic head
model's density lattice at 256^3 and 512^3, threshold at a quantile of the volume's own values (default 0.99), raw and after
mesh_simplify with cells of 2 lattice steps; quantised over the lattice's box, as NeRFRenderer.extract_mesh(smooth=N) does.

  build            sn_rm_mesh_smooth_build: a memset + five launches (degree, rank, scan, fill, init);
  half-step        sn_rm_mesh_smooth_steps with 50 Taubin iterations = 100 launches of k_smooth_step back to back, over 100;
  emit             sn_rm_mesh_smooth_emit with normals and flags: one launch;
  mesh_smooth(10)  the Python call as users make it, quantisation given: build + 20 half-steps + emit, nothing read back.
Beside them, from the same process, on the same mesh:
  (a) torch        one half-step out of torch operators that produces the SAME integers: a gather of Q at the placed neighbours,
                   index_add_ into int64 sums, the fp64 arithmetic of the definition, round, clamp, where.  The index lists, the placed
                   filter, n and the free mask are built once outside the timed region (they do not change over the iterations).  Its
                   integers after one half-step are compared with the kernel's at full size.  Launches: counted with torch.profiler.
  (b) copy         a device-to-device copy of 16V + 24T bytes (the Q rows and the pairs a half-step has to read): it reads and writes
                   that many bytes, more than the half-step writes (16V);
  (c) extraction   NeRFRenderer.extract_mesh() without smoothing (wall clock: it reads sizes back), volume evaluation included, and the
                   isosurface count + emit alone.
`--fan N`: instead of the above, a closed double cone with N ring vertices -- two rows of N pairs -- to time a half-step with long rows
(run it under two builds of the library to compare how such rows are summed).
Kernel rows: HIP events, `--warmup` calls first, medians over `--rounds` rounds of `--repeats` calls.  Rows with host reads: wall clock
around a synchronize, the same counts.

    python tools/mesh_smooth_bench.py [--sizes 256,512] [--out profiles/mesh_smooth_bench.json]

Nothing is asserted about speed; the numbers of one run are reported.  The comparison of integers IS asserted.
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

HALF_STEPS = 100


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


def scaled(r, k):
    return {key: v / k for key, v in r.items()}


def line(name, r, extra=""):
    return f"  {name:<36} median {r['median_ms']:9.4f} ms   min {r['min_ms']:.4f}   max {r['max_ms']:.4f}{extra}"


def workspace_q(ws, V, which):
    """The [V,3] integers of buffer `which` (0: qa, 1: qb) of a mesh_smooth workspace (layout: include/sanerf_hip.h), and the flags."""
    q = ws[16 + which * 16 * V: 16 + (which + 1) * 16 * V].view(torch.int32).view(V, 4)
    return q[:, :3], q[:, 3]


class TorchHalfStep:
    """The half-step of the definition out of torch operators, on Q [V,3] int64.  Everything that does not change over the iterations is
    built here, once."""

    def __init__(self, triangles, Q0, flags, pin_open=True):
        V = Q0.shape[0]
        t = triangles.long()
        valid = ((t >= 0) & (t < V)).all(dim=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
        t = t[valid]
        owner = torch.cat([t[:, 0], t[:, 1], t[:, 2]] * 2)
        other = torch.cat([t[:, 1], t[:, 2], t[:, 0], t[:, 2], t[:, 0], t[:, 1]])
        placed = (flags & 1) != 0
        ok = placed[other]
        self.owner, self.other = owner[ok].contiguous(), other[ok].contiguous()
        n = torch.zeros(V, device=Q0.device, dtype=torch.int64).index_add_(0, self.owner, torch.ones_like(self.owner))
        self.free = (placed & (n > 0) & ~(((flags & 2) != 0) & bool(pin_open)))[:, None]
        self.n = n.clamp(min=1).double()[:, None]
        self.V = V

    def __call__(self, Q, f):
        S = torch.zeros(self.V, 3, device=Q.device, dtype=torch.int64).index_add_(0, self.owner, Q[self.other])
        d = S.double() / self.n - Q.double()
        moved = (Q + torch.round(float(np.float32(f)) * d).long()).clamp_(0, (1 << 22) - 1)
        return torch.where(self.free, moved, Q)


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as e:                                 # reported, not hidden
        return f"not counted ({type(e).__name__}: {e})"


def bench_mesh(name, mesh, quant, w, out):
    dev = mesh["vertices"].device
    vert, tri = mesh["vertices"], mesh["triangles"]
    V, T = vert.shape[0], tri.shape[0]
    origin, quantum = quant
    ws_bytes = int(_lib.lib().sn_rm_mesh_smooth_workspace_bytes(V, T))
    ws = rm.mesh_smooth_build(vert, tri, origin, quantum)
    Q0, flags = (x.clone() for x in workspace_q(ws, V, 0))
    deg = torch.bincount(tri.long().clamp(0, V - 1).reshape(-1), minlength=V)
    out.update(vertices=V, triangles=T, workspace_bytes=ws_bytes, open=int(((flags & 2) != 0).sum()), placed=int((flags & 1).sum()), max_pairs=int(deg.max()))
    print(f" {name}: V = {V}, T = {T}; open vertices {out['open']}, placed {out['placed']}, longest row {out['max_pairs']} pairs; "
          f"workspace {ws_bytes / 2 ** 20:.1f} MiB")
    # the torch chain's integers against the kernel's, one half-step from Q0, at full size
    chain = TorchHalfStep(tri, Q0.long(), flags)
    rm.mesh_smooth_steps(V, T, ws, 1, 0.5, 0.0)
    mine = workspace_q(ws, V, 1)[0].long()
    theirs = chain(Q0.long(), 0.5)
    assert torch.equal(mine, theirs), "the torch chain and k_smooth_step disagree"
    out["moved_by_one_half_step"] = int((mine != Q0.long()).any(dim=1).sum())
    out["torch_launches"] = count_launches(lambda: chain(theirs, -0.53))
    print(f"  integers after one half-step: the torch chain's equal the kernel's ({out['moved_by_one_half_step']} vertices moved); "
          f"the chain is {out['torch_launches']} launches a half-step")
    out["build"] = timed(lambda: rm.mesh_smooth_build(vert, tri, origin, quantum), *w)
    rm.mesh_smooth_build(vert, tri, origin, quantum)
    out["half_step"] = scaled(timed(lambda: rm.mesh_smooth_steps(V, T, ws, HALF_STEPS // 2, 0.5, -0.53), *w), HALF_STEPS)
    ov, on, of = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev), torch.empty(V, device=dev, dtype=torch.uint8)
    out["emit"] = timed(lambda: rm.mesh_smooth_emit(vert, T, origin, quantum, ws, ov, on, of), *w)
    out["mesh_smooth_10"] = timed(lambda: rm.mesh_smooth(mesh, 10, origin=origin, quantum=quantum, normals=True), *w)
    out["mesh_smooth_10_wall"] = timed_wall(lambda: rm.mesh_smooth(mesh, 10, origin=origin, quantum=quantum, normals=True), *w)
    state = {"Q": theirs}

    def torch_pair():                                      # two half-steps, so that the integers keep moving as they do in the kernel's run
        state["Q"] = chain(chain(state["Q"], 0.5), -0.53)
    out["torch_half_step"] = scaled(timed(torch_pair, *w), 2)
    nbytes = 16 * V + 24 * T
    src, dst = torch.empty(nbytes, device=dev, dtype=torch.uint8), torch.empty(nbytes, device=dev, dtype=torch.uint8)
    out["copy"] = timed(lambda: dst.copy_(src), *w)
    out["copy_bytes"] = nbytes
    print(line("build", out["build"]))
    print(line(f"half-step (1/{HALF_STEPS} of {HALF_STEPS} launches)", out["half_step"]))
    print(line("emit, normals and flags", out["emit"]))
    print(line("mesh_smooth(10) (events)", out["mesh_smooth_10"]))
    print(line("mesh_smooth(10) (wall)", out["mesh_smooth_10_wall"]))
    print(line("(a) torch chain, one half-step", out["torch_half_step"]))
    print(line(f"(b) copy of {nbytes / 1e6:.1f} MB", out["copy"], f"   {nbytes / out['copy']['median_ms'] / 1e6:.0f} GB/s read + as much written"))
    out["half_step_over_torch"] = out["half_step"]["median_ms"] / out["torch_half_step"]["median_ms"]
    out["half_step_over_copy"] = out["half_step"]["median_ms"] / out["copy"]["median_ms"]
    print(f"  half-step / (a) = {out['half_step_over_torch']:.3f}   half-step / (b) = {out['half_step_over_copy']:.2f}")


def double_cone(n, dev):
    phi = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(phi), np.sin(phi), 0.05 * np.sin(7.0 * phi)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.7], [0.0, 0.0, -0.6]], ring]).astype(np.float32)
    i, j = 2 + np.arange(n), 2 + (np.arange(n) + 1) % n
    t = np.concatenate([np.stack([np.zeros(n, dtype=np.int64), i, j], axis=1), np.stack([np.ones(n, dtype=np.int64), j, i], axis=1)]).astype(np.int32)
    return {"vertices": torch.from_numpy(v).to(dev), "normals": None, "triangles": torch.from_numpy(t).to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fan", default=None, help="comma-separated ring sizes: time only a half-step on double cones")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_smooth_bench: no GPU visible; times are measured on the device or not at all")
    dev = torch.device("cuda:0")
    w = (args.warmup, args.repeats, args.rounds)
    if args.fan:
        print(f"Half-step on a closed double cone (two rows of n pairs), library {_lib.LIB_PATH}:")
        for n in [int(s) for s in args.fan.split(",")]:
            mesh = double_cone(n, dev)
            V, T = n + 2, 2 * n
            origin, quantum = rm.smooth_quantisation([-1, -1, -1], [1, 1, 1])
            ws = rm.mesh_smooth_build(mesh["vertices"], mesh["triangles"], origin, quantum)
            r = scaled(timed(lambda: rm.mesh_smooth_steps(V, T, ws, HALF_STEPS // 2, 0.5, -0.53), *w), HALF_STEPS)
            print(line(f"n = {n}: half-step", r))
        return
    steps = [128, 64, 32]
    model = NeRFNetwork(synth.make_opt(num_steps=steps, with_mask=True, n_inst=2))
    own = model.state_dict()
    params = synth.synthetic_params(steps, heads=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    model = model.to(dev).eval()
    res = {"what": "mesh smoothing on the synthetic head model's isosurface", "device": torch.cuda.get_device_name(0), "quantile": args.quantile,
           "warmup": args.warmup, "repeats": args.repeats, "rounds": args.rounds, "sizes": {}}
    print(f"Mesh smoothing: tools/mesh_smooth_bench.py, one {res['device']} run (synthetic head model, n_inst 2; {args.warmup} warm-up calls, "
          f"{args.rounds} rounds x {args.repeats} calls; HIP events for kernel rows, wall clock for rows with host reads).")
    with torch.no_grad():
        for n in [int(s) for s in args.sizes.split(",")]:
            r = res["sizes"][str(n)] = {}
            total = n ** 3
            vol = model.density_volume(n)
            shape, origin, step = model._lattice(n, None)
            iso = float(torch.quantile(vol.reshape(-1)[:: max(total // (1 << 22), 1)], args.quantile))
            mesh = rm.isosurface(vol, iso, origin, step)
            quant = rm.smooth_quantisation(origin, [origin[a] + (shape[a] - 1) * step[a] for a in range(3)])
            print(f"\n{n}^3 lattice, threshold {iso:.4g} (the {args.quantile} quantile); quantum {quant[1]:.4g}")
            iws = rm.isosurface_counts(vol, iso)[1]
            r["iso_count"] = timed(lambda: rm.isosurface_counts(vol, iso), *w)
            rm.isosurface_counts(vol, iso)
            r["iso_emit"] = timed(lambda: rm.isosurface_emit(vol, iso, origin, step, iws, mesh["vertices"], mesh["normals"], mesh["triangles"]), *w)
            r["extract_mesh"] = timed_wall(lambda: model.extract_mesh(n, threshold=iso), 1, 2, 3)
            r["extract_mesh_smooth_10"] = timed_wall(lambda: model.extract_mesh(n, threshold=iso, smooth=10), 1, 2, 3)
            print(f"  (c) isosurface count + emit          median {r['iso_count']['median_ms'] + r['iso_emit']['median_ms']:9.4f} ms")
            print(line("(c) extract_mesh() (wall)", r["extract_mesh"]))
            print(line("    extract_mesh(smooth=10) (wall)", r["extract_mesh_smooth_10"]))
            r["raw"] = {}
            bench_mesh("raw", mesh, quant, w, r["raw"])
            o = [float(np.float32(origin[a]) - np.float32(0.5) * np.float32(step[a])) for a in range(3)]
            small = rm.mesh_simplify(mesh, [float(np.float32(2.0 * step[a])) for a in range(3)], origin=o, dims=[int((shape[a] - 0.5) // 2.0) + 2 for a in range(3)])
            r["simplify_2"] = {}
            bench_mesh("after simplify=2", small, quant, w, r["simplify_2"])
            del vol, mesh, small
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
