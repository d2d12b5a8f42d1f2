"""CPU tests of tests/grid_ref64.py, the fp64 reference that the GPU tests of the grid encoder's [L,B,C] layout and of the
>= 2^22-sample scatter compare against (tests/test_gpu_grid_layouts.py).

  * anchored to vectors it did not produce: it reproduces tests/golden/kat_encoders.npz (tools/gen_kat_encoders.py: per-sample Python
    loops, Python integers) for all five grids -- forward within 1e-12, table-gradient rows identical, values within 1e-12;
  * the C oracle (fp32) agrees with it within the derived round-off bounds on what the KAT file lacks: smoothstep, dy_dx, the input
    gradient, max_level < L, D = 4 and 5, fp16 tables.

  * the two regularisers on the table gradient (tv_gradient, weight_decay): a known answer worked out by hand on a 4 x 4 table, the
    oracle (sequential fp32) within tv_bound / weight_decay_bound over every case of tests/test_gpu_grid_regularisers.py, identities.

Worst |err| / bound of the oracle against the reference over the cases below: forward 0.15, dy_dx 0.15, table gradient 0.17,
input gradient 0.05; total variation 0.25 over the 24 (D, C), 0.31 over grid type x align_corners; weight decay 0.23 (a bound of
1.0 is the limit)."""
import os

import numpy as np
import pytest
import torch

import grid_ref64 as R
import grid_reg_cases as K
from helpers import GOLD

KAT = np.load(os.path.join(GOLD, "kat_encoders.npz"))
GRIDS = ["main", "head", "prop1", "tiled_ac", "small_ac"]       # in the order tools/gen_kat_encoders.py draws them
KAT_SEED = 20260929                                             # tools/gen_kat_encoders.py: main()


def _kat_float64_gradients():
    """The KAT file stores the incoming gradient rounded to fp32, but its grad_vals were summed from the unrounded float64 draws, so the
    fp32 copy reproduces them only to 2^-24.  The draws are replayed here (same generator, same sequence of calls as the tool makes:
    sample_points' uniform + integers, then standard_normal); the replay is in step iff its fp32 rounding equals the stored gradient."""
    rng = np.random.default_rng(KAT_SEED)
    out = {}
    for name in GRIDS:
        L = int(KAT[f"{name}.cfg"][1])
        rng.uniform(0, 1, (24 if L == 16 else 40, 3))
        for r in [int(v) for v in KAT[f"{name}.res"]][::3]:
            rng.integers(0, r, (2, 3))
        g = rng.standard_normal(KAT[f"{name}.y"].shape)
        assert np.array_equal(g.astype(np.float32), KAT[f"{name}.grad"]), f"{name}: replay of the generator's draws is out of step"
        out[name] = g
    return out


_G64 = {}


@pytest.mark.parametrize("name", GRIDS)
def test_fp64_reference_reproduces_the_independent_vectors(name):
    from sanerf_hq_amd import synth                              # (table generator only, as in the tool)
    if not _G64:
        _G64.update(_kat_float64_gradients())
    D, L, C, log2T, base, desired, gridtype, ac, seed = [int(v) for v in KAT[f"{name}.cfg"]]
    grid = R.Grid(D, L, C, log2T, base, desired=desired, gridtype=gridtype, align_corners=bool(ac))
    assert grid.offsets == [int(v) for v in KAT[f"{name}.offsets"]] and grid.res == [int(v) for v in KAT[f"{name}.res"]]
    assert abs(grid.scale - float(KAT[f"{name}.scale"][0])) < 1e-15
    table = torch.from_numpy(synth.make_param(dict(name=name, shape=[grid.rows, C], seed=seed, lo=-1.0, hi=1.0)))
    x = torch.from_numpy(KAT[f"{name}.x"])
    y = R.forward(grid, x, table)["y"].reshape(x.shape[0], L * C).numpy()
    assert np.abs(y - KAT[f"{name}.y"]).max() <= 1e-12
    g64 = _G64[name]
    bt = R.backward_table(grid, x, torch.from_numpy(g64).reshape(-1, L, C))
    gt = bt["grad_table"].numpy()
    rows = np.flatnonzero(bt["n"].numpy() > 0)
    assert np.array_equal(rows, KAT[f"{name}.grad_rows"]), "row set differs from the independent index computation"
    assert np.abs(gt[rows] - KAT[f"{name}.grad_vals"]).max() <= 1e-12
    assert not gt[bt["n"].numpy() == 0].any()
    # partition of unity: the weights of a sample sum to 1
    inr = R.in_range(x).numpy()
    want = g64.reshape(-1, L, C)[inr].sum(0)
    for l in range(L):
        assert np.abs(gt[grid.offsets[l]:grid.offsets[l + 1]].sum(0) - want[l]).max() <= 1e-12


def _points(rng, B, D):
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x[0] = 0; x[1] = 1; x[2] = 0.5; x[3, 0] = 1.25; x[4, 1] = -0.01
    return x


CASES = {
    # name: (D, C, L, log2T, base, desired, gridtype, align_corners, interp, max_level, half table)
    "smooth_d3": (3, 2, 3, 11, 4, 40, 0, False, 1, 3, False),
    "smooth_ac_tiled": (3, 4, 3, 9, 4, 24, 1, True, 1, 3, False),
    "max_level": (3, 8, 4, 11, 4, 40, 0, False, 0, 2, False),
    "d2_smooth_half": (2, 16, 3, 8, 4, 40, 0, False, 1, 3, True),
    "d4": (4, 2, 3, 11, 4, 40, 0, False, 0, 3, False),
    "d4_smooth_maxl": (4, 1, 3, 11, 4, 24, 0, True, 1, 2, False),
    "d5": (5, 4, 3, 11, 4, 40, 0, False, 0, 3, True),
    "d5_tiled": (5, 32, 2, 10, 3, 9, 1, False, 1, 2, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_agrees_with_the_fp64_reference_beyond_the_kat_file(orc, name):
    D, C, L, log2T, base, desired, gridtype, ac, interp, max_level, half = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 500)
    grid = R.Grid(D, L, C, log2T, base, desired=desired, gridtype=gridtype, align_corners=ac, interp=interp)
    offs, pls = orc.grid_layout(D, L, C, 2, base, log2T, desired)
    assert [int(v) for v in offs] == grid.offsets and orc.level_resolutions(L, np.log2(pls), base) == grid.res
    emb = rng.uniform(-1, 1, (grid.rows, C)).astype(np.float16 if half else np.float32)
    x = _points(rng, 300, D)
    fw = R.forward(grid, torch.from_numpy(x), torch.from_numpy(emb), want_dy_dx=True, max_level=max_level)
    y, dd = orc.grid_encode_forward(x, emb, offs, pls, base, True, gridtype, ac, interp, max_level)
    ratios = {}
    ratios["forward"], exact = R.worst_ratio(torch.from_numpy(y).reshape(-1, L, C), fw["y"], R.forward_bound(grid, fw["y_mass"]))
    assert exact, "out-of-range samples / levels >= max_level are not exactly zero"
    ratios["dy_dx"], exact = R.worst_ratio(torch.from_numpy(dd).reshape(-1, L, D, C), fw["dy_dx"], R.dy_dx_bound(grid, fw["dy_dx_mass"]))
    assert exact
    g = rng.standard_normal((300, L, C)).astype(np.float32)
    gt = torch.from_numpy(g)
    ge, gi = orc.grid_encode_backward(g.reshape(300, L * C), x, emb, offs, pls, base, dd, gridtype, ac, interp, max_level)
    bt = R.backward_table(grid, torch.from_numpy(x), gt, max_level)
    ratios["table"], exact = R.worst_ratio(torch.from_numpy(ge), bt["grad_table"], R.table_grad_bound(grid, bt["n"], bt["mass"]))
    assert exact, "gradient in rows without contribution"
    assert int(bt["n"][grid.offsets[max_level]:].sum()) == 0 and int(bt["n"].sum()) == int(R.in_range(torch.from_numpy(x)).sum()) * max_level << D
    bi = R.backward_input(grid, gt, fw)
    ratios["input"], exact = R.worst_ratio(torch.from_numpy(gi), bi["grad_inputs"], R.input_grad_bound(grid, bi["mass"]))
    assert exact
    print(name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


# ---- the regularisers: tv_gradient / tv_bound, weight_decay / weight_decay_bound ---------------------------------------------------------
def test_tv_known_answer_written_by_hand(orc):
    """One dense tiled level, D = 2, C = 1, 4 x 4 vertices in 16 rows (row = x + 4 y), the table written out; which neighbours a centre
    has, and what the vertex 4 folds back to, is worked out below by hand -- neither R._rows nor the oracle is asked."""
    T = [[3, -1, 4, 1],          # T[y][x]
         [-5, 9, 2, -6],
         [5, 3, -5, 8],
         [9, -7, 9, 6]]
    table = torch.tensor(T, dtype=torch.float32).reshape(16, 1)
    eps = float(np.float32(1e-9))
    w = 0.5 / (2 * 2)                                              # exact in fp32

    def contribution(centre, neighbours):
        d = [centre - v for v in neighbours]
        return w * sum(d) / np.sqrt(sum(v * v for v in d) + eps), w * sum(abs(v) for v in d) / np.sqrt(sum(v * v for v in d) + eps)

    grid = R.Grid(2, 1, 1, 4, 4, gridtype=1)
    assert grid.res == [4] and grid.offsets == [0, 16] and grid.walk == [2] and grid.hashed == [False]
    # positions x * 4 - 0.5 clamped to [0, 3]: (2.3, 1.1) -> centre (2, 1);  (-0.1 -> 0, -0.5 -> 0) -> (0, 0);  (3.5 -> 3, 3.5 -> 3) -> (3, 3)
    x = torch.tensor([[0.7, 0.4], [0.1, 0.0], [1.0, 1.0]], dtype=torch.float32)
    want = {
        # interior (2, 1): right (3, 1), left (1, 1), above (2, 2), below (2, 0)
        2 + 4 * 1: contribution(T[1][2], [T[1][3], T[1][1], T[2][2], T[0][2]]),
        # (0, 0): no left neighbour in either dimension: (1, 0) and (0, 1) alone
        0: contribution(T[0][0], [T[0][1], T[1][0]]),
        # (3, 3): the right neighbours are the vertices (4, 3) -> 4 + 12 = 16 -> 16 % 16 = row 0 = T[0][0] and (3, 4) -> 3 + 16 = 19 -> row 3 = T[0][3]
        3 + 4 * 3: contribution(T[3][3], [T[0][0], T[3][2], T[0][3], T[2][3]]),
    }
    assert abs(want[6][0] - 0.125 * 6 / np.sqrt(166 + eps)) < 1e-16 and abs(want[0][0] - 0.125 * 12 / np.sqrt(80 + eps)) < 1e-16
    assert abs(want[15][0] - 0.125 * 3 / np.sqrt(47 + eps)) < 1e-16                       # 6-3, 6-9, 6-1, 6-8
    ref = R.tv_gradient(grid, x, table, 0.5)
    g0 = np.zeros((16, 1), np.float32)
    got = orc.grad_total_variation(x.numpy(), table.numpy(), g0, np.asarray(grid.offsets, np.int32), 0.5, grid.scale, 4, 1, False)
    for row in range(16):
        v, m = want.get(row, (0.0, 0.0))
        assert abs(float(ref["grad"][row, 0]) - v) <= 1e-15 and abs(float(ref["mass"][row, 0]) - m) <= 1e-15, row
        assert int(ref["n"][row]) == (row in want)
        assert abs(float(got[row, 0]) - v) <= 1e-6 * abs(v), row
    # align_corners: positions x * 3; (1, 1) -> floor 3 -> min(3, res - 2) = (2, 2), whose right neighbours are the LAST vertices, not past them
    ac = R.Grid(2, 1, 1, 4, 4, gridtype=1, align_corners=True)
    v, _ = contribution(T[2][2], [T[2][3], T[2][1], T[3][2], T[1][2]])
    assert abs(v - 0.125 * -42 / np.sqrt(478 + eps)) < 1e-16
    ref = R.tv_gradient(ac, x[2:], table, 0.5)
    got = orc.grad_total_variation(x[2:].numpy(), table.numpy(), np.zeros((16, 1), np.float32), np.asarray(ac.offsets, np.int32), 0.5, ac.scale, 4, 1, True)
    assert abs(float(ref["grad"][10, 0]) - v) <= 1e-15 and int(ref["n"].sum()) == 1 and abs(float(got[10, 0]) - v) <= 1e-6 * abs(v)
    assert not got[np.arange(16) != 10].any()


def _tv_oracle_case(orc, grid, seed, weight=0.75, B=1029):
    gen = torch.Generator().manual_seed(seed)
    x = K.placed_points(grid, B, gen, "cpu")
    table = torch.rand(grid.rows, grid.C, generator=gen) * 2 - 1
    g0 = torch.randn(grid.rows, grid.C, generator=gen)
    assert orc.level_resolutions(grid.L, np.log2(grid.scale), grid.base) == grid.res
    got = orc.grad_total_variation(x.numpy(), table.numpy(), g0.numpy().copy(), np.asarray(grid.offsets, np.int32), weight, grid.scale, grid.base,
                                   grid.gridtype, grid.align_corners)
    return x, table, g0, torch.from_numpy(got)


@pytest.mark.parametrize("D,C", K.TV_DC)
def test_oracle_tv_within_the_bound_every_instantiation(orc, D, C):
    grid = K.tv_dc_grid(D, C)
    assert not grid.hashed[0] and grid.hashed[2]
    x, table, g0, got = _tv_oracle_case(orc, grid, 100 * D + C)
    K.check_tv_coverage(grid, x)
    ref = R.tv_gradient(grid, x, table, 0.75)
    print(f"oracle tv D={D} C={C}: {K.assert_tv(got, g0, ref, grid, 'oracle'):.3f}")


@pytest.mark.parametrize("D,C,gridtype,ac", K.TV_MODES)
def test_oracle_tv_within_the_bound_grid_types_and_align_corners(orc, D, C, gridtype, ac):
    grid = K.tv_mode_grid(D, C, gridtype, ac)
    K.check_tv_mode_levels(grid)
    x, table, g0, got = _tv_oracle_case(orc, grid, 1000 * D + 10 * C + 2 * gridtype + ac, weight=0.3)
    K.check_tv_coverage(grid, x)
    ref = R.tv_gradient(grid, x, table, 0.3)
    print(f"oracle tv D={D} C={C} gridtype={gridtype} ac={ac}: {K.assert_tv(got, g0, ref, grid, 'oracle'):.3f}")


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_oracle_tv_within_the_bound_batch_edges(orc, B):
    """The CPU counterpart of test_gpu_grid_regularisers.py::test_tv_batch_edges: the same grid, placed samples and batch sizes."""
    grid = K.tv_mode_grid(3, 8, 0, False)
    x, table, g0, got = _tv_oracle_case(orc, grid, 40 + B, B=B)
    ref = R.tv_gradient(grid, x, table, 0.75)
    assert int(ref["n"].sum()) == int(R.in_range(x).sum()) * grid.L
    print(f"oracle tv B={B}: {K.assert_tv(got, g0, ref, grid, 'oracle'):.3f}")


@pytest.mark.parametrize("gridtype,ac", [(0, False), (1, True)])
def test_tv_identities(orc, gridtype, ac):
    grid = K.tv_mode_grid(3, 8, gridtype, ac)
    x, table, g0, got = _tv_oracle_case(orc, grid, 7)
    offs = np.asarray(grid.offsets, np.int32)
    args = (offs, 0.75, grid.scale, grid.base, gridtype, ac)
    # a constant table has no variation: exactly nothing is added (0 / sqrt(eps) = 0, and g0 + 0 = g0)
    const = torch.full_like(table, 0.37)
    assert not bool(R.tv_gradient(grid, x, const, 0.75)["grad"].any())
    assert np.array_equal(orc.grad_total_variation(x.numpy(), const.numpy(), g0.numpy().copy(), *args), g0.numpy())
    # rows that no sample's centre maps to keep g0 bit for bit
    ref = R.tv_gradient(grid, x, table, 0.75)
    untouched = ref["n"] == 0
    assert bool(untouched.any()) and bool((ref["n"] > 0).any()) and torch.equal(got[untouched], g0[untouched])
    assert not bool(ref["grad"][untouched].any()) and not bool(ref["mass"][untouched].any())
    # the samples out of range are skipped: the in-range subset alone gives the same sums, in the oracle's sequential order the same bits
    inr = R.in_range(x)
    assert int((~inr).sum()) == 2
    sub = R.tv_gradient(grid, x[inr], table, 0.75)
    assert torch.equal(sub["grad"], ref["grad"]) and torch.equal(sub["n"], ref["n"]) and int(ref["n"].sum()) == int(inr.sum()) * grid.L
    assert np.array_equal(orc.grad_total_variation(x[inr].numpy(), table.numpy(), g0.numpy().copy(), *args), got.numpy())


def _oracle_weight_decay(orc, grid, seed):
    C = grid.C
    gen = torch.Generator().manual_seed(seed)
    table = torch.rand(grid.rows, C, generator=gen) * 2 - 1
    g0 = torch.randn(grid.rows, C, generator=gen)
    offs = np.asarray(grid.offsets, np.int32)
    got = torch.from_numpy(orc.grad_weight_decay(table.numpy(), g0.numpy().copy(), offs, 0.1))
    term = R.weight_decay(grid, table, 0.1)
    ratio, _ = R.worst_ratio(got, g0.double() + term, R.weight_decay_bound(grid, g0, term))
    print(f"oracle weight decay C={C} L={grid.L} sizes {[grid.size(l) for l in range(grid.L)]}: {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # table = 1, g0 = 0, weight 0.5: every element reads out 1 / size of the level its row was assigned to, exactly
    got = torch.from_numpy(orc.grad_weight_decay(np.ones((grid.rows, C), np.float32), np.zeros((grid.rows, C), np.float32), offs, 0.5))
    assert torch.equal(got, R.weight_decay_exact_levels(grid))
    K.check_wd_level_boundaries(grid)


@pytest.mark.parametrize("C,L", K.WD_CL)
def test_oracle_weight_decay_within_the_bound_and_on_the_right_level(orc, C, L):
    """Level sizes pairwise distinct (asserted in wd_grid): the exact readout tells every level from every other."""
    _oracle_weight_decay(orc, K.wd_grid(C, L), 10 * C + L)


def test_oracle_weight_decay_levels_that_share_the_capped_size(orc):
    _oracle_weight_decay(orc, K.wd_capped_grid(2), 99)
