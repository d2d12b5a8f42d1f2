"""The cases of the regulariser tests -- grids, placed samples and the assertions that the cases hold what they are for -- shared by the
CPU tests (tests/test_grid_ref64.py: the oracle against tests/grid_ref64.py) and the GPU tests (tests/test_gpu_grid_regularisers.py: the
kernels against it).  The operations and their bounds are stated in grid_ref64.py; nothing here computes an expected value."""
import torch

import grid_ref64 as R

TV_DC = [(D, C) for D in (2, 3, 4, 5) for C in (1, 2, 4, 8, 16, 32)]                     # every k_grid_tv<D, C> the library instantiates
TV_MODES = [(D, C, gridtype, ac) for D in (2, 3) for C in (1, 8) for gridtype in (0, 1) for ac in (False, True)]
_TV_SHAPE = {2: (8, 6), 3: (9, 6), 4: (10, 5), 5: (11, 4)}                               # D: (log2T, base); L = 3, scale 2: a dense first level (40, 216, 632, 1024 rows), a hashed last one
WD_CL = [(C, L) for C in (1, 2, 32) for L in (1, 4, 16)]


def tv_dc_grid(D, C):
    log2T, base = _TV_SHAPE[D]
    return R.Grid(D, 3, C, log2T, base, gridtype=0, align_corners=False)


def tv_mode_grid(D, C, gridtype, align_corners):
    """L = 4, base 6, 2^8 rows at most.  D = 2, scale 4 (6, 24, 96, 384): a dense level of 40 rows, then 256 rows each; on the last the dense
    walk stops after one dimension (384 > 256).  D = 3, scale 2 (6, 12, 24, 48): a dense level of 216 rows, then 256 each; from 24 on the
    walk stops after two dimensions."""
    return R.Grid(D, 4, C, 8, 6, desired=384 if D == 2 else 48, gridtype=gridtype, align_corners=align_corners)


def wd_grid(C, L):
    """D = 2, base 4, scale 1.17, 2^11 rows at most: 16, 32, 40, 56, 64, 88, 128, 176, 232, 296, 400, 536, 736, 968, 1376, 1856 rows.  No two
    levels have the same size, so 1.0f / size tells every level from every other."""
    grid = R.Grid(2, L, C, 11, 4, per_level_scale=1.17)
    sizes = [grid.size(l) for l in range(L)]
    assert len(set(sizes)) == L, f"level sizes are not pairwise distinct: {sizes}"
    return grid


def wd_capped_grid(C):
    """D = 2, base 8, scale 1.2, L = 16: 64, 104, ..., 1768 rows, then six levels of the capped size 2048."""
    grid = R.Grid(2, 16, C, 11, 8, per_level_scale=1.2)
    sizes = [grid.size(l) for l in range(16)]
    assert sizes.count(2048) >= 3 and sizes[-1] == 2048, f"no run of levels that share the capped size: {sizes}"
    return grid


def check_wd_level_boundaries(grid):
    """The exact readout's expectation puts offsets[l] on level l and offsets[l] - 1 on level l - 1."""
    lv = R.level_of_rows(grid)
    for l in range(1, grid.L):
        assert int(lv[grid.offsets[l]]) == l and int(lv[grid.offsets[l] - 1]) == l - 1


PILE = 300
ONE_BELOW = 1.0 - 2.0 ** -24
JUST_ABOVE = 1.0 + 2.0 ** -23
JUST_BELOW = -1e-8


def placed_points(grid, B, gen, device):
    """[B, D] fp32: uniform samples with the placed ones written over the first rows -- the domain's corners, 1 - 2^-24, -0.0 (in range),
    one coordinate alone at 1 (the first dimension, then the last: the vertex `res` at the smallest and at the largest stride), every
    level's cell boundaries ((k + 0.5) / res, or k / (res - 1) with align_corners), two samples just outside (1 + 2^-23 and -1e-8), and,
    where B has room for them, PILE copies of one point (PILE atomic additions into one row per level)."""
    D = grid.D
    rows = [[0.0] * D, [1.0] * D, [ONE_BELOW] * D, [-0.0] + [0.5] * (D - 1), [1.0] + [0.25] * (D - 1), [0.25] * (D - 1) + [1.0],
            [JUST_ABOVE] + [0.5] * (D - 1), [0.5] * (D - 1) + [JUST_BELOW]]
    for res in grid.res:
        for k in (1, res // 2, res - 2, res - 1):
            rows.append([k / (res - 1) if grid.align_corners else (k + 0.5) / res] * D)
    placed = torch.tensor(rows, dtype=torch.float32, device=device)
    x = torch.rand(max(B, 1), D, generator=gen, device=device)[:B]
    k = min(B, placed.shape[0])
    x[:k] = placed[:k]
    if B >= placed.shape[0] + PILE:
        x[placed.shape[0]:placed.shape[0] + PILE] = torch.tensor([0.3137] * D, dtype=torch.float32, device=device)
    return x.contiguous()


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def tv_coverage(grid, x):
    """What the samples x reach, read off the reference's own cells: dict of
      skipped       samples out of range
      max_vertex    per level the largest neighbour coordinate asked for (res where a centre sits at res - 1)
      at_zero       per level whether a centre has a coordinate 0 (no left neighbour there)
      on_boundary   per level whether a sample's fp32 position is, in every dimension, within res * 2^-21 of an integer k with 1 <= k <= res - 2:
                    an inner cell boundary.  The domain's corners (k = 0 and k = res - 1, where the samples 0, 1 and 1 - 2^-24 land) do
                    not count, so this holds only through the placed (k + 0.5) / res or k / (res - 1)
      pile          the largest number of contributions to one row
      exact_one, one_below, minus_zero, lone_one, just_above, just_below   whether that placed value is among the samples"""
    ok = R.in_range(x)
    xs = x[ok]
    zeros = torch.zeros(grid.rows, grid.C, device=x.device)
    out = dict(skipped=int((~ok).sum()), max_vertex=[], at_zero=[], on_boundary=[], pile=int(R.tv_gradient(grid, x, zeros, 1.0)["n"].max()))
    for l in range(grid.L):
        cell, frac = R._locate(grid, xs, l)
        out["max_vertex"].append(int(cell.max()) + 1)
        out["at_zero"].append(bool((cell == 0).any()))
        tol = grid.res[l] * 2.0 ** -21                                                   # the two fp32 roundings behind a position < res: 4 ulp of it
        low, high = frac <= tol, frac >= 1 - tol
        k = cell + high.long()                                                           # the integer the position is next to
        inner = (low | high) & (k >= 1) & (k <= grid.res[l] - 2)
        out["on_boundary"].append(bool(inner.all(dim=1).any()))
    is_one = x == 1.0
    out["exact_one"] = bool(is_one.all(dim=1).any())
    out["one_below"] = bool((x == _f32(ONE_BELOW)).all(dim=1).any()) and _f32(ONE_BELOW) < 1.0
    out["minus_zero"] = bool(((x == 0) & torch.signbit(x)).any(dim=1)[ok].any())
    out["lone_one"] = bool((is_one[:, 0] & (is_one.sum(dim=1) == 1)).any()) and bool((is_one[:, -1] & (is_one.sum(dim=1) == 1)).any())
    out["just_above"] = bool(((x == _f32(JUST_ABOVE)).any(dim=1) & ~ok).any()) and _f32(JUST_ABOVE) > 1.0
    out["just_below"] = bool(((x == _f32(JUST_BELOW)).any(dim=1) & ~ok).any()) and _f32(JUST_BELOW) < 0.0
    return out


def check_tv_coverage(grid, x):
    """The placed samples are really there (asserted from the reference's side, so that an edit of placed_points cannot quietly lose one)."""
    cov = tv_coverage(grid, x)
    assert cov["skipped"] == 2 and cov["just_above"] and cov["just_below"], cov
    assert cov["pile"] >= PILE, cov
    assert cov["exact_one"] and cov["one_below"] and cov["minus_zero"] and cov["lone_one"], cov
    assert all(cov["at_zero"]) and all(cov["on_boundary"]), cov
    # without align_corners a centre at res - 1 asks for the vertex res, one past the last; with it the centre stops at res - 2
    assert cov["max_vertex"] == [r - 1 if grid.align_corners else r for r in grid.res], cov
    return cov


def check_tv_mode_levels(grid):
    """The level set of a grid type x align_corners case holds what the case is for."""
    dense = [grid.res[l] ** grid.D <= grid.size(l) for l in range(grid.L)]
    assert any(d and grid.size(l) & (grid.size(l) - 1) for l, d in enumerate(dense)), "no dense level whose size is not a power of two"
    if grid.gridtype == 0:
        assert any(grid.hashed), "no hashed level"
    else:
        assert not any(grid.hashed) and any(grid.walk[l] < grid.D for l in range(grid.L)), "no tiled level whose walk stops early"
        assert any(not d and grid.walk[l] == grid.D for l, d in enumerate(dense)), "no tiled level that wraps after the whole walk"


def assert_tv(got, g0, ref, grid, what):
    """got - g0 within tv_bound of the reference, rows without a contribution bit-equal to g0; returns the worst |err| / bound."""
    ratio, exact = R.worst_ratio(got.double() - g0.double(), ref["grad"], R.tv_bound(grid, ref["n"], ref["mass"], g0))
    untouched = ref["n"] == 0
    assert exact and torch.equal(got[untouched], g0[untouched]), f"{what}: a row that no sample's centre maps to does not keep its gradient bit for bit"
    assert ratio <= 1.0, f"{what}: |err| / bound = {ratio}"
    return ratio
