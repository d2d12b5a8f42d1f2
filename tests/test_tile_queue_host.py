"""CPU: the eight wave-tile queues of the persistent last stage (render_rays.h: tile_queue_range; render.hip: k_final_stage_pt) through
sn_rm_tile_queue_info -- the host twin of the kernel's own arithmetic, no device needed -- and the planner's choice of the launch form
through sn_rm_render_route_info_cus (tests/test_render_route_host.py builds the descriptors).

A launch of `units` 256-ray tile units has 4 * units wave-tile ids (the padding of the last unit included: the kernel takes such an id
from its queue and skips it).  The eight ranges must hold every id exactly once, and queue x must hold exactly the wave tiles of the
workgroup tiles that workgroups x, x + 8, x + 16, ... of the ordinary launch render, in that order (sn_rm_tile_order_info: tile_id of
workgroup b) -- for every linear_tile_order, for widths and heights that are no multiples of 8 or 16, odd wave-tile row counts, the
dist.shard_rows bands of a 1600x1600 image over 8 ranks, a one-tile image, and rays in linear order."""
import ctypes as C

import pytest

from sanerf_hq_amd import _lib, dist
from sanerf_hq_amd import raymarching as rm
from test_render_route_host import make_cfg, make_io

ORDERS = [0, 1, 2, 3, 4]
BANDS_1600 = sorted({e - b for b, e in (dist.shard_rows(1600, 8, r) for r in range(8))})
SHAPES = [(8, 8), (40, 24), (29, 37), (37, 29), (136, 136), (24, 8), (808, 8), (200, 200), (800, 800)] + [(1600, rows) for rows in BANDS_1600]      # W x rows


def units_of(W, rows):
    return -(-(-(-W // 8) * -(-rows // 8)) // 4)


def queues(units, order):
    out = []
    for x in range(8):
        q = rm.tile_queue_info(units, x, order=order)
        assert q["queues"] == 8 and q["wave_tiles"] == 4 * units
        out.append((q["begin"], q["end"]))
    return out


def ordinary_tile_ids(W, rows, order):
    """tile id of every workgroup of the ordinary launch, in dispatch order"""
    info = _lib.TileOrderInfo()
    fn = _lib.lib().sn_rm_tile_order_info
    ids = []
    for b in range(units_of(W, rows)):
        assert fn(W, rows, 0, order, b, C.byref(info)) == 0, _lib.lib().sn_last_error()
        assert info.workgroups == units_of(W, rows)
        ids.append(info.tile_id)
    return ids


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("W,rows", SHAPES)
def test_the_queues_partition_the_wave_tiles_and_are_four_times_the_xcd_ranges(W, rows, order):
    units = units_of(W, rows)
    qs = queues(units, order)
    ids = sorted(g for b, e in qs for g in range(b, e))
    assert ids == list(range(4 * units)), "every wave-tile id in exactly one queue"
    tiles = ordinary_tile_ids(W, rows, order)
    if order == 1:          # no remap: one queue over all ids, in order
        assert qs[0] == (0, 4 * units) and all(b >= e for b, e in qs[1:])
        assert tiles == list(range(units))
        return
    for x, (b, e) in enumerate(qs):
        mine = tiles[x::8]            # what XCD x renders today: workgroups x, x + 8, ...
        assert list(range(b, e)) == [4 * t + w for t in mine for w in range(4)], (x, b, e)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", [1, 64, 1000, 16385])
def test_linear_order_batches(N, order):
    units = -(-N // 256)
    qs = queues(units, order)
    assert sorted(g for b, e in qs for g in range(b, e)) == list(range(4 * units))
    sizes = [e - b for b, e in qs]
    if order != 1:
        assert max(sizes) - min(sizes) <= 4 and all(s % 4 == 0 for s in sizes)


def test_arguments_are_checked():
    info = _lib.TileQueueInfo()
    fn = _lib.lib().sn_rm_tile_queue_info
    assert fn(2500, 0, 0, 8, C.byref(info)) != 0 and b"queue 8" in _lib.lib().sn_last_error()
    assert fn(2500, 0, 6, 0, C.byref(info)) != 0
    assert fn(2500, 0, 0, 0, None) != 0
    assert fn(0, 0, 0, 0, C.byref(info)) == 0 and (info.begin, info.end, info.wave_tiles) == (0, 0, 0)
    assert rm.tile_queue_info(2500, 0) == dict(queues=8, wave_tiles=10000, begin=0, end=1252)      # 2500 = 8 * 312 + 4: the first four ranges hold 313 tiles


# ---- the planner ------------------------------------------------------------------------------------------------------------------
LDS_F16X3 = (8192 + 4 * 2 * 64 * 20) * 4
LDS_F16X3_PT = (8192 + 8 * 2 * 64 * 20 + (32 * 32 + 32 * 32 + 3 * 32)) * 4
CUS = 256


def route(cfg, io, cus):
    info = _lib.LaunchInfo()
    rc = _lib.lib().sn_rm_render_route_info_cus(C.byref(cfg), C.byref(io), cus, C.byref(info))
    assert rc == 0, _lib.lib().sn_last_error()
    return dict(final_kernel=info.final_kernel.decode(), workgroups=info.workgroups, lds_bytes=info.lds_bytes, launches=info.launches,
                persistent_tiles=info.persistent_tiles, grid_workgroups=info.grid_workgroups)


def test_auto_is_on_only_above_the_resident_wave_slots():
    """8 waves per CU are resident: with 256 CUs the rule turns at 2048 wave tiles = 512 tile units."""
    for W, rows, on in ((800, 800, True), (512, 256, False), (512, 264, True), (200, 200, False), (40, 24, False)):
        cfg = make_cfg([128], True)
        r = route(cfg, make_io(cfg, W * rows, W), CUS)
        units = units_of(W, rows)
        assert units * 4 > 8 * CUS if on else units * 4 <= 8 * CUS
        assert r["persistent_tiles"] == int(on) and r["workgroups"] == units, (W, rows, r)
        assert r["grid_workgroups"] == (CUS if on else units) and r["lds_bytes"] == (LDS_F16X3_PT if on else LDS_F16X3)
    # the headline: the name and the unit count the existing tests pin do not change
    cfg = make_cfg([128], True)
    r = route(cfg, make_io(cfg, 800 * 800, 800), CUS)
    assert r == dict(final_kernel="k_final_stage<lt,K=7>", workgroups=2500, lds_bytes=LDS_F16X3_PT, launches=1, persistent_tiles=1, grid_workgroups=256)
    # a device of unknown size (the plain dry run): automatic stays off
    assert route(cfg, make_io(cfg, 800 * 800, 800), 0)["persistent_tiles"] == 0
    info = _lib.LaunchInfo()
    assert _lib.lib().sn_rm_render_route_info(C.byref(cfg), C.byref(make_io(cfg, 800 * 800, 800)), C.byref(info)) == 0
    assert (info.persistent_tiles, info.grid_workgroups, info.workgroups, info.lds_bytes) == (0, 2500, 2500, LDS_F16X3)


def test_two_row_bands_take_the_persistent_launch_from_four_times_the_slot_count():
    """Two bands on two streams: two persistent launches serialise where two ordinary ones overlap their tails (measured: 800x800 loses,
    1600x1600 gains), so the automatic rule asks such a call for more than 4 x 8 x CUs wave tiles per band."""
    cfg = make_cfg([128, 64, 32], True)
    r = route(cfg, make_io(cfg, 800 * 800, 800), CUS)
    assert (r["launches"], r["workgroups"], r["persistent_tiles"], r["grid_workgroups"], r["lds_bytes"]) == (2, 1250, 0, 1250, LDS_F16X3)
    r = route(cfg, make_io(cfg, 1600 * 1600, 1600), CUS)
    assert (r["launches"], r["workgroups"], r["persistent_tiles"], r["grid_workgroups"]) == (2, 5000, 1, CUS)
    cfg = make_cfg([128, 64, 32], True, band_streams=1)
    r = route(cfg, make_io(cfg, 800 * 800, 800), CUS)
    assert (r["launches"], r["workgroups"], r["persistent_tiles"]) == (1, 2500, 1)
    cfg = make_cfg([128, 64, 32], True, persistent_tiles=2)
    assert route(cfg, make_io(cfg, 800 * 800, 800), CUS)["persistent_tiles"] == 1


def test_never_and_always_and_the_workgroup_count():
    cfg = make_cfg([128], True, persistent_tiles=1)
    r = route(cfg, make_io(cfg, 800 * 800, 800), CUS)
    assert (r["persistent_tiles"], r["grid_workgroups"], r["lds_bytes"]) == (0, 2500, LDS_F16X3)
    for f16 in (True, False):
        for densify, name in ((1, "k_final_stage<lt,K=5>"), (2, "k_final_stage<lt,K=7>")):
            cfg = make_cfg([16], f16, persistent_tiles=2, densify=densify)
            r = route(cfg, make_io(cfg, 8 * 8, 8), CUS)
            assert r == dict(final_kernel=name, workgroups=1, lds_bytes=LDS_F16X3_PT, launches=1, persistent_tiles=1, grid_workgroups=CUS)
    cfg = make_cfg([16], True, persistent_tiles=2, persistent_wgs=3)
    assert route(cfg, make_io(cfg, 200 * 200, 200), CUS)["grid_workgroups"] == 3
    # what the persistent form does not cover keeps the ordinary launch even when it is asked for
    cfg = make_cfg([16], True, persistent_tiles=2, exact_early_out=2)
    assert route(cfg, make_io(cfg, 200 * 200, 200), CUS)["persistent_tiles"] == 0
    cfg = make_cfg([64, 32], False, with_feat=True, persistent_tiles=2)
    assert route(cfg, make_io(cfg, 4096, 64), CUS)["persistent_tiles"] == 0
    cfg = make_cfg([64, 32], False, persistent_tiles=2)
    assert route(cfg, make_io(cfg, 64 * 64, 64, debug=("weights",)), CUS)["persistent_tiles"] == 0
    cfg = make_cfg([128], True, persistent_tiles=3)
    info = _lib.LaunchInfo()
    assert _lib.lib().sn_rm_render_route_info(C.byref(cfg), C.byref(make_io(cfg, 4096, 64)), C.byref(info)) == -1
    assert b"persistent_tiles 3" in _lib.lib().sn_last_error()


# (schedule, rays, width, band slots, bytes of the same workspace before the counters existed: packed weights + pair rows + stage scratch)
@pytest.mark.parametrize("steps,N,W,slots,before", [([128], 800 * 800, 800, 1, 77405312), ([128, 64, 32], 800 * 800, 800, 2, 753484976), ([16], 1000, 0, 1, 8557312),
                                                    ([16, 8, 8], 40 * 24, 40, 1, 11257008)])
def test_the_workspace_grows_by_the_counters_only(steps, N, W, slots, before):
    """8 uint32 per band slot behind everything else, whatever the tuning says: the size does not depend on the launch form."""
    l = _lib.lib()
    sizes = [l.sn_rm_render_workspace_bytes(C.byref(make_cfg(steps, True, persistent_tiles=p)), N, W) for p in (0, 1, 2)]
    assert sizes[0] == sizes[1] == sizes[2] == before + 8 * 4 * slots
    cfg = make_cfg(steps, True)
    io = make_io(cfg, N, W)
    io.workspace, io.workspace_bytes = 64, before             # what was enough is too small by the counters, said before any launch
    assert l.sn_rm_render_rays(C.byref(cfg), C.byref(io), None) == -4 and (b"need %d)" % sizes[0]) in l.sn_last_error()
    assert route(cfg, io, CUS)["launches"] == slots
