"""CPU: which part of the image a workgroup of the render stages takes under each tuning.linear_tile_order, through
sn_rm_tile_order_info -- the host twin of the kernels' own arithmetic (render_rays.h: xcd_tile_id, wave_tile_of), no device needed.

Every order is a bijection between the wave-tile slots of the launch's workgroups and the wave tiles of the image, for whole images, odd
wave-tile row counts (the 32x8-pixel workgroups of the last row), widths that are no multiple of 16, the row bands of dist.shard_rows
(1600x200) and both wave-tile shapes in use.  Order 3, the 8x8-block super-tiles, keeps 64 consecutive tile ids of one XCD's range -- the
workgroups an XCD holds at a time (32 CUs x 2) -- inside a bounding box of 16x16 workgroup blocks: that condition is what "compact" means
here, it is not a tuned number (the row-pair order's 64 consecutive ids span the 50 blocks of the image's width).  Order 3 measured slower
than the row pairs and is not the default; the default, order 4, walks 3x3-block super-tiles (its 64 ids: a run of them inside at most two super-tile rows)."""
import ctypes as C

import pytest

from sanerf_hq_amd import _lib
from sanerf_hq_amd import raymarching as rm

SHAPES = [(8, 8), (40, 24), (136, 136), (800, 800), (1600, 200), (24, 8), (808, 8)]      # W x rows
DEFAULT_ORDER = 4             # what linear_tile_order = 0 selects
ORDERS = [0, 1, 2, 3, 4]


def launch_map(W, rows, wave_tile, order):
    """[(tile_id, [(x, y) | None] * 4)] over the launch's workgroups, and the wave tile's size."""
    info = _lib.TileOrderInfo()
    fn = _lib.lib().sn_rm_tile_order_info
    assert fn(W, rows, wave_tile, order, 0, C.byref(info)) == 0, _lib.lib().sn_last_error()
    nwg, tw, th = info.workgroups, info.tile_w, info.tile_h
    out = []
    for b in range(nwg):
        assert fn(W, rows, wave_tile, order, b, C.byref(info)) == 0
        assert (info.workgroups, info.tile_w, info.tile_h) == (nwg, tw, th)
        out.append((info.tile_id, [(info.x[w], info.y[w]) if info.x[w] >= 0 else None for w in range(4)]))
    return out, tw, th


@pytest.mark.parametrize("wave_tile", [0, 4])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("W,rows", SHAPES)
def test_every_order_is_a_bijection_onto_the_wave_tiles(W, rows, wave_tile, order):
    m, tw, th = launch_map(W, rows, wave_tile, order)
    assert (tw, th) == ((8, 8) if wave_tile == 0 else (16, 4))
    tx, ty = -(-W // tw), -(-rows // th)
    assert len(m) == -(-tx * ty // 4), "ceil(wave tiles / 4) workgroups whatever the order"
    assert sorted(t for t, _ in m) == list(range(len(m))), "workgroup -> tile id is a permutation"
    if order == 1:
        assert [t for t, _ in m] == list(range(len(m)))
    tiles = [xy for _, ws in m for xy in ws if xy is not None]
    assert len(tiles) == tx * ty and set(tiles) == {(x * tw, y * th) for x in range(tx) for y in range(ty)}
    # padding only in the LAST tile id, behind its real wave tiles
    for t, ws in m:
        if None in ws:
            assert t == len(m) - 1 and all(w is None for w in ws[ws.index(None):])


@pytest.mark.parametrize("W,rows", SHAPES)
def test_orders_share_tile_ids_where_they_must(W, rows):
    """0 is the default order; 1 and 2 walk the same tiles (2 only deals them to the XCDs in contiguous ranges), 2 and 3 deal the same tile id
    to every workgroup; the odd last wave-tile row keeps its place behind all row pairs in every order."""
    m = {o: launch_map(W, rows, 0, o)[0] for o in ORDERS}
    assert m[0] == m[DEFAULT_ORDER]
    assert [t for t, _ in m[2]] == [t for t, _ in m[3]] == [t for t, _ in m[4]]
    by_tile = {o: dict(m[o]) for o in (1, 2, 3, 4)}
    assert by_tile[1] == by_tile[2]
    ty = -(-rows // 8)
    if ty % 2:
        last_row = {t for t, ws in m[1] if any(xy is not None and xy[1] == (ty - 1) * 8 for xy in ws)}
        for o in (2, 3, 4):
            assert {t for t, ws in m[o] if any(xy is not None and xy[1] == (ty - 1) * 8 for xy in ws)} == last_row


def test_whole_blocks_where_the_image_has_them():
    """800x800: every workgroup of every order is one 16x16-pixel block."""
    for order in (1, 2, 3, 4):
        for _, ws in launch_map(800, 800, 0, order)[0]:
            x0, y0 = min(x for x, _ in ws), min(y for _, y in ws)
            assert x0 % 16 == 0 and y0 % 16 == 0 and set(ws) == {(x0, y0), (x0, y0 + 8), (x0 + 8, y0), (x0 + 8, y0 + 8)}
            assert ws[0][1] == y0 and ws[1] == (ws[0][0], y0 + 8), "a wave-tile column at a time"


def _xcd_ranges(m):
    """tile id -> 16x16 block, and the contiguous tile-id range of each XCD (workgroup b runs on XCD b % 8)."""
    block = {t: (ws[0][0] // 16, ws[0][1] // 16) for t, ws in m}
    ranges = []
    for x in range(8):
        ids = [m[b][0] for b in range(x, len(m), 8)]
        assert ids == list(range(ids[0], ids[0] + len(ids))), "an XCD's workgroups take consecutive tile ids, in dispatch order"
        ranges.append(ids)
    return block, ranges


def _worst_box(block, ids, n=64):
    worst = (0, 0)
    for i in range(len(ids) - n + 1):
        bs = [block[t] for t in ids[i:i + n]]
        w = max(b[0] for b in bs) - min(b[0] for b in bs) + 1
        h = max(b[1] for b in bs) - min(b[1] for b in bs) + 1
        worst = (max(worst[0], w), max(worst[1], h))
    return worst


def test_the_square_super_tiles_keep_an_xcds_co_resident_workgroups_compact():
    m, _, _ = launch_map(800, 800, 0, 3)
    block, ranges = _xcd_ranges(m)
    assert sorted(len(r) for r in ranges) == [312] * 4 + [313] * 4
    for ids in ranges:
        w, h = _worst_box(block, ids)
        assert w <= 16 and h <= 16, f"64 consecutive tile ids of one XCD span {w} x {h} blocks"
    # the previous order for comparison: a strip as wide as the image
    m2, _, _ = launch_map(800, 800, 0, 2)
    block2, ranges2 = _xcd_ranges(m2)
    assert _worst_box(block2, ranges2[0]) == (50, 3)
    # the default: super-tiles of 3 blocks x 3 (one row of them: 2) row pairs = 18 (12) units; 64 ids = 128 units touch at most
    # ceil(127 / 12) + 1 = 12 of them, 3 blocks wide each, in one super-tile row or around the turn into the next
    m4, _, _ = launch_map(800, 800, 0, 4)
    block4, ranges4 = _xcd_ranges(m4)
    for ids in ranges4:
        w, h = _worst_box(block4, ids)
        assert w <= 36 and h <= 6, f"64 consecutive tile ids of one XCD span {w} x {h} blocks"


def test_arguments_are_checked_and_the_python_wrapper_agrees():
    info = _lib.TileOrderInfo()
    fn = _lib.lib().sn_rm_tile_order_info
    assert fn(800, 800, 0, 0, 2500, C.byref(info)) != 0 and b"outside the launch of 2500" in _lib.lib().sn_last_error()
    assert fn(800, 800, 6, 0, 0, C.byref(info)) != 0 and fn(0, 8, 0, 0, 0, C.byref(info)) != 0
    assert fn(800, 800, 0, 0, 0, None) != 0
    got = rm.tile_order_info(40, 24, 3, order=1)
    assert got == dict(workgroups=4, tile_id=3, tile_w=8, tile_h=8, tiles=[(16, 16), (24, 16), (32, 16), None])


def test_pack_valid_sits_in_the_padding_of_the_abi_12_struct():
    assert C.sizeof(_lib.RenderIO) == 312 and _lib.RenderIO.pack_valid.offset == 292 and _lib.RenderIO.workspace.offset == 296
    assert _lib.RenderIO().pack_valid == 0 and _lib.PACK_VALID == 0x50414B31
