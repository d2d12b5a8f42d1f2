"""CPU tests of the parity order of the last stage's hashed-level gathers (render_gather.h: issue_level_lv<..., PY, PZ> / blend_level_par): a numpy
restatement of the slot permutation -- permute by cell parity, trade the x-pairs between the wave's halves, trade back, un-permute -- and the
line model of tools/gather_parity_table.py, which the choice of levels rests on."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gather_parity_table as gpt  # noqa: E402

P1, P2 = np.uint32(2654435761), np.uint32(805459861)


def corner_rows(cell, res, clamp):
    """[64, 8] hash rows of a wave's corners, corner c = x + 2 dy + 4 dz; clamp: the +1 neighbour is held at res - 1 (gridencoder.cu:182)"""
    out = []
    for c in range(8):
        q = cell + np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.uint32)
        if clamp:
            q = np.minimum(q, np.uint32(res - 1))
        out.append(q[:, 0] ^ (q[:, 1] * P1) ^ (q[:, 2] * P2))
    return np.stack(out, axis=-1).astype(np.int64)


def kernel_issue(rows, cell, by_y, by_z):
    """what issue_level_lv does to a wave's [64, 8] requests: lanes with an odd cell coordinate trade their two slots of that axis, then
    the halves of the wave trade the x-pairs (half_wave_swap).  -> the [8, 64] requests of the 8 instructions"""
    s = rows.copy()
    if by_y:
        odd = (cell[:, 1] & 1) == 1
        for i in (0, 1, 4, 5):
            s[odd, i], s[odd, i + 2] = s[odd, i + 2].copy(), s[odd, i].copy()
    if by_z:
        odd = (cell[:, 2] & 1) == 1
        for i in range(4):
            s[odd, i], s[odd, i + 4] = s[odd, i + 4].copy(), s[odd, i].copy()
    return half_swap(s.T.copy())


def half_swap(ins):
    """v_permlane32_swap on each pair (2q, 2q+1): a' = [a.lo | b.lo], b' = [a.hi | b.hi]; its own inverse"""
    out = ins.copy()
    for q in range(4):
        a, b = ins[2 * q], ins[2 * q + 1]
        out[2 * q] = np.concatenate([a[:32], b[:32]])
        out[2 * q + 1] = np.concatenate([a[32:], b[32:]])
    return out


def kernel_blend_order(landed, tag_y, tag_z, by_y, by_z):
    """what blend_level_par does to the landed [8, 64] values: the half-wave exchange back, then the z exchange (i <-> i + 4) and the y exchange
    (i <-> i + 2) for lanes whose carried parity is odd.  -> [64, 8] in corner order"""
    s = half_swap(landed).T.copy()
    if by_z:
        odd = tag_z == 1
        for i in range(4):
            s[odd, i], s[odd, i + 4] = s[odd, i + 4].copy(), s[odd, i].copy()
    if by_y:
        odd = tag_y == 1
        for i in (0, 1, 4, 5):
            s[odd, i], s[odd, i + 2] = s[odd, i + 2].copy(), s[odd, i].copy()
    return s


def wave_cells(parity_y, parity_z, res, border, rng):
    """64 cells around a random place (or against the upper border, where the neighbour is clamped) with the given y / z parities"""
    base = np.full(3, res - 4, np.int64) if border else rng.integers(8, res - 16, 3)
    cell = base + rng.integers(0, 3, (64, 3))
    cell = np.minimum(cell, res - 1)
    for d, par in ((1, parity_y), (2, parity_z)):
        if par is not None:
            cell[:, d] = np.minimum((cell[:, d] & ~1) | par, res - 1 if (res - 1) % 2 == par else res - 2)
    return cell.astype(np.uint32)


@pytest.mark.parametrize("by_y,by_z", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("py", [0, 1, None])
@pytest.mark.parametrize("pz", [0, 1, None])
def test_permutation_round_trip(by_y, by_z, border, py, pz):
    """All four parity combinations (a whole wave of one parity pair) and mixed waves (None), inside the table and against the border where
    the +1 neighbour is clamped: every lane gets its eight rows back in canonical slots, each instruction carries exactly the requests of its
    lanes' corners, and the grouping rule holds -- instruction (a, b) asks only for corners whose absolute y / z has parity a / b."""
    rng = np.random.default_rng(5 + 2 * (py or 0) + (pz or 0))
    res = 1352
    cell = wave_cells(py, pz, res, border, rng)
    rows = corner_rows(cell, res, clamp=border)
    ins = kernel_issue(rows, cell, by_y, by_z)
    assert sorted(ins.ravel().tolist()) == sorted(rows.ravel().tolist()), "the 512 requests are a permutation of the 512 corners"
    # the table: the landed value of a request is a function of its row alone
    landed = (ins * 2654435761 + 12345) % 1000003
    back = kernel_blend_order(landed, cell[:, 1] & 1, cell[:, 2] & 1, by_y, by_z)
    assert np.array_equal(back, (rows * 2654435761 + 12345) % 1000003), "a corner value reached a wrong slot"
    # the same permutation as the tool models
    assert np.array_equal(gpt.half_wave_exchange(gpt.permute_slots(rows, cell.astype(np.int64), by_y, by_z)[None, :, None, :])[0, 0], ins)
    if not border:      # (a clamped neighbour repeats the cell's own coordinate: any slot is right for it)
        own = half_swap(ins).T                                  # each lane's own eight requests, in slot order
        for slot in range(8):
            for lane in range(64):
                cands = [c for c in range(8) if rows[lane, c] == own[lane, slot] and (c & 1) == (slot & 1)]
                assert cands, (lane, slot)
                ok = False
                for c in cands:
                    ay = int(cell[lane, 1]) + ((c >> 1) & 1); az = int(cell[lane, 2]) + ((c >> 2) & 1)
                    wy = (ay & 1) if by_y else ((c >> 1) & 1); wz = (az & 1) if by_z else ((c >> 2) & 1)
                    ok = ok or (wy == ((slot >> 1) & 1) and wz == ((slot >> 2) & 1))
                assert ok, (lane, slot)


def test_adjacent_cells_meet_in_one_instruction():
    """Two lanes in y-adjacent cells ask for the row they share in ONE instruction under the parity order and in two under the canonical one."""
    cell = np.tile(np.array([[500, 600, 700]], np.uint32), (64, 1))          # (the other lanes are elsewhere)
    cell[0] = [100, 200, 300]
    cell[1] = [100, 201, 300]
    rows = corner_rows(cell, 1352, clamp=False)
    shared = rows[0, 2]                     # (x, y + 1, z) of lane 0 = (x, y, z) of lane 1
    assert shared == rows[1, 0]
    for by_y, n in ((False, 2), (True, 1)):
        ins = kernel_issue(rows, cell, by_y, False)
        assert sum(1 for i in range(8) if shared in ins[i].tolist()) == n


def test_model_today_column_stays_where_the_decision_was_taken():
    """With --tiles 4 the canonical order's mean stays within 10 % of the 8.3 lines per hashed-level instruction the counters fit (TA busy 25
    cycles per wave-gather).  (The whole image's mean is 8.9 by this tool's 64-tile run; sets of 4 tiles scatter from 8.3 to 9.6.)"""
    tab = gpt.table(hw=800, tiles=4, row_bytes=4)
    assert len(tab) == 9 and [l for l, _, _ in tab] == list(range(7, 16))
    today = gpt.mean_lines(tab, "today")
    print(f"today: {today:.2f} lines per hashed instruction; y+z parity: {gpt.mean_lines(tab, 'y+z-parity'):.2f}")
    assert abs(today - 8.3) <= 0.1 * 8.3
    for _, _, per in tab:
        assert per["y+z-parity"][0] <= per["z-parity"][0] <= per["today"][0] and per["y+z-parity"][0] <= per["y-parity"][0] <= per["today"][0]
