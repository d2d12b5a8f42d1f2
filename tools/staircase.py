#!/usr/bin/env python3
"""Kernel time of the fused stages as a function of the NUMBER OF WORKGROUPS of a launch (fp16 tables): a 1600-pixel-wide image
of 16*k rows is 100*k workgroups of 16x16 pixels on 512 resident slots (2 per CU).  Shows the round quantisation an 8-way row-band
split of BASELINE configs[3] runs into (200 rows -> 1300 workgroups = 2.54 rounds) and what a tail policy could recover.
usage (GPU box): python tools/staircase.py [W] [--tuning field=value,...] [--schedules 128;128,64,32] [--ks 20,23,24,...] [--rows 200,...]
(--tuning: fields of raymarching.Tuning, e.g. persistent_tiles=1 for the A/B of the persistent tile queue of the last stage)"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import _tuning  # noqa: E402
from helpers import product_model, synthetic_params  # noqa: E402
from sanerf_hq_amd import _lib, raymarching as rm, synth  # noqa: E402

dev = torch.device("cuda:0")
ap = argparse.ArgumentParser()
ap.add_argument("W", type=int, nargs="?", default=1600)
ap.add_argument("--tuning", default="", help="kernel-selection fields of raymarching.Tuning, field=value,...")
ap.add_argument("--schedules", default="128,64,32;128", help="schedules separated by ';'")
ap.add_argument("--ks", default="", help="tile rows (16 image rows each) to time, comma separated; default: the full ladder")
ap.add_argument("--rows", default="", help="image rows to time instead of 16 * ks, comma separated (200: one band of 1600 rows over 8 ranks)")
args = ap.parse_args()
W = args.W
applied = _tuning.apply_default(args.tuning)
H = 1600
lib = _lib.lib()
ro, rd = rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(H, H), H, H, device=dev)
ro = ro.view(H, H, 3)[:, :W].contiguous()
rd = rd.view(H, H, 3)[:, :W].contiguous()
tiles_x = (W + 15) // 16
ks = [int(k) for k in args.ks.split(",")] if args.ks else [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 21, 24, 25, 26, 28, 31, 36, 41, 46, 51, 52]
print(f"library {os.environ.get('SN_LIB', '') or 'HEAD'}, tuning {applied or 'default'}")
for steps in [[int(t) for t in sch.split(",")] for sch in args.schedules.split(";")]:
    model = product_model(synthetic_params(steps, seed=0), steps, False, dev)
    plan = rm.RenderPlan(model, steps, torch.float16)
    print(f"schedule {steps}, W={W}: rows  workgroups  rounds(512)  | pack prop0 prop1 final ms | us per final round-equivalent")
    for rows in ([int(r) for r in args.rows.split(",")] if args.rows else [16 * k for k in ks]):
        if rows > H:
            break
        o = ro[:rows].reshape(-1, 3).contiguous()
        d = rd[:rows].reshape(-1, 3).contiguous()
        for _ in range(3):
            rm.render_rays(plan, o, d, tile_w=W)
        torch.cuda.synchronize()
        lib.sn_rm_profile_enable(1)
        n = 10
        for _ in range(n):
            rm.render_rays(plan, o, d, tile_w=W)
        torch.cuda.synchronize()
        ms = (C.c_float * 8)()
        cnt = (C.c_int32 * 8)()
        _lib.check(lib.sn_rm_profile_read(ms, cnt, 8), "profile_read")
        lib.sn_rm_profile_enable(0)
        nwg = -(-(-(-W // 8) * -(-rows // 8)) // 4)          # ceil(wave tiles / 4)
        per = [ms[i] / n for i in range(6)]
        print(f"  {rows:5d} {nwg:6d} {nwg / 512:6.2f} | {per[0]:.3f} {per[1]:.3f} {per[2]:.3f} {per[4]:.3f} | {per[4] * 1e3 / (nwg / 512):.1f}")
