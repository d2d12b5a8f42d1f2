#!/usr/bin/env python3
"""Distinct 128-byte lines per gather instruction of the last stage's HASHED levels when a lane's eight corner requests are grouped by the
PARITY of the corner's absolute y / z instead of by the corner's offset inside the cell (CPU only; round 10).

Canonical order: instruction (dy, dz) of a level fetches the corner (cell.y + dy, cell.z + dz).  Two rays in y-adjacent cells y and y + 1 both need
hash row y + 1, one in its dy = 1 instruction, the other in its dy = 0 instruction: the line is visited twice.  Parity order: every lane puts into
instruction (a, b) the corner whose absolute y has parity a and whose absolute z has parity b (lanes in odd cells trade their two slots of that
axis), so both requests meet in one instruction and the address unit merges them.  The x-corners keep the half-wave exchange of the kernel:
instruction 2q serves both x-corners of lanes 0-31, instruction 2q + 1 those of lanes 32-63.

Per hashed level: mean distinct lines per instruction and the modelled address-unit cycles of the level's 8 instructions (17.5 cycles up to 8
lines, 2.3 per line beyond: tools/ubench/gathers.hip, profiles/r01/ubench_gathers.txt), for the canonical order, y-parity, z-parity and both.
Bench camera, `[128]`, 8x8-pixel wave tiles in row-major lane order, seeded tiles stratified over the image, all samples.
usage: python tools/gather_parity_table.py [--hw 800] [--tiles 16] [--rows-bytes 4|8]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

ORDERS = ("today", "y-parity", "z-parity", "y+z-parity")
BASE_CYCLES, FREE_LINES, CYCLES_PER_LINE = 17.5, 8, 2.3
FIRST_HASHED = 7                                 # the headline kernel reads levels 0-6 as packed dense rows (5 and 6 densified per call)
DENSE_GATHER_CYCLES = 14 * BASE_CYCLES          # those 7 levels: 2 quad-row loads each


def permute_slots(rows, cell, by_y, by_z):
    """rows [..., 8] in corner order c = x + 2 dy + 4 dz, cell [..., 3] -> rows in slot order: slot x + 2 a + 4 b holds the corner whose absolute
    y / z has parity a / b on the axes grouped by parity, the corner with dy = a / dz = b on the others."""
    py = (cell[..., 1] & 1).astype(np.int64) if by_y else np.zeros(cell.shape[:-1], np.int64)
    pz = (cell[..., 2] & 1).astype(np.int64) if by_z else np.zeros(cell.shape[:-1], np.int64)
    slot = np.arange(8)
    src = slot ^ (2 * py[..., None]) ^ (4 * pz[..., None])
    return np.take_along_axis(rows, src, axis=-1)


def half_wave_exchange(v):
    """v [tiles, 64, T, 8] per-lane slots -> [tiles, T, 8, 64]: what the 64 lanes of each of the 8 instructions ask for."""
    ins = []
    for q in range(4):
        ins.append(np.concatenate([v[:, :32, :, 2 * q], v[:, :32, :, 2 * q + 1]], axis=1))
        ins.append(np.concatenate([v[:, 32:, :, 2 * q], v[:, 32:, :, 2 * q + 1]], axis=1))
    return np.stack(ins, axis=-1).transpose(0, 2, 3, 1)


def distinct_lines(ins, row_bytes):
    s = np.sort(ins * row_bytes // 128, axis=-1)
    return 1 + (s[..., 1:] != s[..., :-1]).sum(-1)          # [tiles, T, 8]


def model_cycles(lines):
    return BASE_CYCLES + CYCLES_PER_LINE * np.maximum(lines - FREE_LINES, 0)


def table(hw=800, tiles=16, row_bytes=4, seed=0):
    """-> list of (level, res, {order: (lines per instruction, cycles of the level's 8 instructions)}) for the levels the kernel gathers as hashed."""
    import oracle as orc
    from gather_lines_table import rows_of
    from helpers import GRIDS, oracle_cfg, synthetic_params
    from sanerf_hq_amd import synth
    steps = [128]
    H = W = hw
    cfg = oracle_cfg(orc, synthetic_params(steps, seed=0), steps)
    pose = synth.orbit_pose(1.0, 20.0, 30.0)
    fx, fy = synth.pinhole_intrinsics(H, W)[:2]
    ro, rd = orc.generate_rays(pose, fx, fy, W / 2.0, H / 2.0, H, W)
    rng = np.random.default_rng(seed)
    # stratified: the image is cut into a lattice of g x g cells, `tiles` of them (seeded choice) give one seeded tile each -- the lines per
    # instruction vary with the place in the image, and few purely random tiles scatter by +-10 % around the image's mean
    g = int(np.ceil(np.sqrt(tiles)))
    cells = rng.permutation(g * g)[:tiles]
    nt = H // 8
    ty = (cells // g) * nt // g + rng.integers(0, max(nt // g, 1), tiles); tx = (cells % g) * nt // g + rng.integers(0, max(nt // g, 1), tiles)
    lane = np.arange(64)
    idx = np.concatenate([(y * 8 + (lane >> 3)) * W + (x * 8 + (lane & 7)) for y, x in zip(ty, tx)])
    out = orc.render(cfg, ro[idx], rd[idx], debug=True)
    rb = out["real_bins0"].astype(np.float32)
    tmid = (rb[:, 1:] + rb[:, :-1]) / np.float32(2)
    p = ro[idx][:, None, :] + rd[idx][:, None, :] * tmid[..., None]
    bound = float(cfg.bound)
    x01 = (orc.contract(p.reshape(-1, 3).astype(np.float32)).reshape(p.shape) + bound) / (2 * bound)
    T = x01.shape[1]
    g = GRIDS["grid"]
    offs, pls = orc.grid_layout(3, g["num_levels"], g["level_dim"], 2, 16, g["log2_hashmap_size"], g["desired_resolution"])
    res = orc.level_resolutions(g["num_levels"], float(np.log2(pls)), 16)
    result = []
    for l in range(g["num_levels"]):
        r = int(res[l]); size = int(offs[l + 1] - offs[l])
        rows, cell, dense = rows_of(x01, r, size, int(offs[l]))
        if dense or l < FIRST_HASHED:
            continue
        rows = rows.astype(np.int64).reshape(tiles, 64, T, 8)
        cell = cell.astype(np.int64).reshape(tiles, 64, T, 3)
        per = {}
        for name, by_y, by_z in zip(ORDERS, (False, True, False, True), (False, False, True, True)):
            lines = distinct_lines(half_wave_exchange(permute_slots(rows, cell, by_y, by_z)), row_bytes)
            per[name] = (float(lines.mean()), float(model_cycles(lines).sum(-1).mean()))
        result.append((l, r, per))
    return result


def mean_lines(tab, order="today"):
    """mean distinct lines per hashed-level instruction"""
    return float(np.mean([per[order][0] for _, _, per in tab]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--rows-bytes", type=int, choices=(4, 8), default=4)
    a = ap.parse_args()
    tab = table(a.hw, a.tiles, a.rows_bytes)
    print(f"bench camera (orbit 1.0 / 20 / 30), {a.hw}x{a.hw}, [128], {a.tiles} seeded 8x8 wave tiles, all 128 samples, {a.rows_bytes}-byte rows, "
          f"half-wave x exchange kept; lines = 128 bytes")
    print(f"model: {BASE_CYCLES} cycles per instruction up to {FREE_LINES} lines + {CYCLES_PER_LINE} per line beyond; per level = its 8 instructions")
    print(f"{'lvl':>3} {'res':>5} | " + " | ".join(f"{o:>10}: lines cycles" for o in ORDERS))
    for l, r, per in tab:
        print(f"{l:>3} {r:>5} | " + " | ".join(f"{'':>10}  {per[o][0]:5.1f} {per[o][1]:6.0f}" for o in ORDERS))
    print("all hashed levels, per wave-sample:")
    for o in ORDERS:
        visits = sum(per[o][0] * 8 for _, _, per in tab)
        cyc = sum(per[o][1] for _, _, per in tab)
        print(f"  {o:>10}: {mean_lines(tab, o):5.2f} lines per instruction, {visits:6.0f} line visits, {cyc:6.0f} cycles; with the 14 dense gathers "
              f"({DENSE_GATHER_CYCLES:.0f}) {cyc + DENSE_GATHER_CYCLES:6.0f}")
    for first in (9, 11, 12, 13, 14):
        for o in ("z-parity", "y+z-parity"):
            cyc = sum(per[o if l >= first else "today"][1] for l, _, per in tab)
            print(f"  parity from level {first:>2}, {o:>10}: {cyc:6.0f} cycles on the hashed levels")


if __name__ == "__main__":
    main()
