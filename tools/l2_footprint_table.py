#!/usr/bin/env python3
"""Distinct 128-byte table lines behind ONE XCD's L2 per depth step of the bench line's last stage, per tile order (CPU only).

DESIGN.md section 9.4: k_final_stage<lt,K=7> at 800x800 [128] with fp16 tables sends 35 % of its L2 requests on to the fabric -- 18 GB per
frame (TCC_EA0_RDREQ x 128 B).  This model reproduces that figure from the image tiles alone and prices a tile order with it.  An XCD holds
64 workgroups at a time (32 CUs x 2) and, with the XCD-aware remap, they are 64 consecutive tile ids (sn_rm_tile_order_info states which
pixels those are under each tuning.linear_tile_order).  The workgroups march in step, so at one depth index the XCD's L2 sees the corner
fetches of 64 x 256 rays at that depth: levels 5-6 as 16-byte quad rows (densified for this launch), levels 7-15 as 4-byte hashed rows.
The model counts the distinct lines of those fetches, assumes perfect reuse inside a depth step and none across steps, and scales:
    bytes per frame = lines x 128 steps x (2500 / 8 / 64 = 4.88 rounds of 64 workgroups) x 8 XCDs x 128 B.
Nothing is fitted.  Levels 0-4 (1.4 MB of quad rows in all) stay resident and are left out.
usage: python tools/l2_footprint_table.py [--hw 800] [--orders 2,3,4] [--measured 2=18.0,3=17.0]   (GB per frame from the counter, per order)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as orc  # noqa: E402
from helpers import GRIDS, oracle_cfg, synthetic_params  # noqa: E402
from sanerf_hq_amd import raymarching as rm, synth  # noqa: E402
from gather_lines_table import rows_of  # noqa: E402

LEVELS = range(5, 16)
DENSIFIED = (5, 6)            # read as quad rows by the K = 7 instantiation
PLACEMENTS = ((1, 0), (3, 100), (6, 200))      # (XCD, offset of the 64 ids inside its range)
DEPTHS = (9, 27, 45, 63, 81, 99, 117)


def xcd_pixels(W, H, order, xcd, first, n=64):
    """Flat pixel indices of the rays of `n` consecutive tile ids of one XCD's range, from the `first`-th on."""
    nwg = rm.tile_order_info(W, H, 0, order=order)["workgroups"]
    idx = []
    for b in range(xcd + 8 * first, min(xcd + 8 * (first + n), nwg), 8):
        info = rm.tile_order_info(W, H, b, order=order)
        for t in info["tiles"]:
            if t is None:
                continue
            ys, xs = np.meshgrid(t[1] + np.arange(info["tile_h"]), t[0] + np.arange(info["tile_w"]), indexing="ij")
            keep = (ys < H) & (xs < W)
            idx.append((ys[keep] * W + xs[keep]).ravel())
    return np.concatenate(idx)


def lines_per_level(x01, res, offs):
    """x01 [n, 3] sample positions of one depth step -> {level: distinct 128-byte lines over all corner fetches}."""
    out = {}
    for l in LEVELS:
        r = int(res[l]); size = int(offs[l + 1] - offs[l])
        if l in DENSIFIED:    # quad row of vertex (x, y, z) and of (x, y, z + 1): 16 bytes each, 8 to a line
            pos = np.clip(x01.astype(np.float32) * np.float32(r) - np.float32(0.5), 0, r - 1)
            pg = np.floor(pos).astype(np.int64)
            z1 = np.minimum(pg[:, 2] + 1, r - 1)
            base = pg[:, 0] + pg[:, 1] * r
            rows = np.concatenate([base + pg[:, 2] * r * r, base + z1 * r * r])
            out[l] = np.unique(rows // 8).size
        else:                 # 8 corners, 4-byte rows (level_dim 2, fp16), 32 to a line
            rows, _, _ = rows_of(x01[:, None, :], r, size, int(offs[l]))
            out[l] = np.unique(rows.astype(np.int64) // 32).size
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--orders", default="2,3,4")
    ap.add_argument("--measured", default="", help="GB beyond the L2s per frame from TCC_EA0_RDREQ, e.g. 2=18.0,3=16.1")
    a = ap.parse_args()
    orders = [int(o) for o in a.orders.split(",")]
    measured = {int(k): float(v) for k, v in (kv.split("=") for kv in a.measured.split(",") if kv)}
    steps = [128]
    H = W = a.hw
    params = synthetic_params(steps, seed=0)
    cfg = oracle_cfg(orc, params, steps)
    pose = synth.orbit_pose(1.0, 20.0, 30.0)
    fx, fy = synth.pinhole_intrinsics(H, W)[:2]
    ro, rd = orc.generate_rays(pose, fx, fy, W / 2.0, H / 2.0, H, W)
    bound = float(cfg.bound)
    g = GRIDS["grid"]
    offs, pls = orc.grid_layout(3, g["num_levels"], g["level_dim"], 2, 16, g["log2_hashmap_size"], g["desired_resolution"])
    res = orc.level_resolutions(g["num_levels"], float(np.log2(pls)), 16)

    def positions(idx):
        out = orc.render(cfg, ro[idx], rd[idx], debug=True)
        rb = out["real_bins0"].astype(np.float32)
        tmid = (rb[:, 1:] + rb[:, :-1]) / np.float32(2)
        p = ro[idx][:, None, :] + rd[idx][:, None, :] * tmid[..., None]
        z = orc.contract(p.reshape(-1, 3).astype(np.float32)).reshape(p.shape)
        return (z + bound) / (2 * bound)                                  # [n, T, 3]

    nwg = rm.tile_order_info(W, H, 0, order=orders[0])["workgroups"]
    rounds = nwg / 8.0 / 64.0
    table = {o: {l: [] for l in LEVELS} for o in orders}
    for o in orders:
        for xcd, first in PLACEMENTS:
            x = positions(xcd_pixels(W, H, o, xcd, first))
            for t in DEPTHS:
                for l, n in lines_per_level(x[:, t, :], res, offs).items():
                    table[o][l].append(n)
    mean = {o: {l: float(np.mean(v)) for l, v in table[o].items()} for o in orders}
    print(f"bench camera (orbit 1.0 / 20 / 30), {H}x{W} [128], fp16 tables; 64 consecutive tile ids of one XCD, {len(PLACEMENTS)} placements x {len(DEPTHS)} depths; lines = 128 bytes")
    ratios = "".join(f" {'%d / %d' % (o, orders[0]):>8}" for o in orders[1:])
    print(f"{'lvl':>3} {'res':>5} | " + " ".join(f"{'order ' + str(o):>10}" for o in orders) + " |" + ratios)
    for l in LEVELS:
        print(f"{l:>3} {int(res[l]):>5} | " + " ".join(f"{mean[o][l]:>10.0f}" for o in orders) + " |"
              + "".join(f" {mean[o][l] / mean[orders[0]][l]:>8.2f}" for o in orders[1:]))
    tot = {o: sum(mean[o].values()) for o in orders}
    print(f"{'all':>3} {'':>5} | " + " ".join(f"{tot[o]:>10.0f}" for o in orders) + " |" + "".join(f" {tot[o] / tot[orders[0]]:>8.3f}" for o in orders[1:]))
    print(f"\nbytes beyond the L2s per frame = lines x 128 steps x {rounds:.2f} rounds x 8 XCDs x 128 B:")
    for o in orders:
        gb = tot[o] * 128 * rounds * 8 * 128 / 1e9
        m = f"   measured (TCC_EA0_RDREQ x 128 B): {measured[o]:.1f} GB" if o in measured else ""
        print(f"  order {o}: {tot[o]:8.0f} lines per step -> {gb:5.1f} GB predicted{m}")


if __name__ == "__main__":
    main()
