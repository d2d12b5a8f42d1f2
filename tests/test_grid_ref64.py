"""CPU tests of tests/grid_ref64.py, the fp64 reference that the GPU tests of the grid encoder's [L,B,C] layout and of the
>= 2^22-sample scatter compare against (tests/test_gpu_grid_layouts.py).

  * anchored to vectors it did not produce: it reproduces tests/golden/kat_encoders.npz (tools/gen_kat_encoders.py: per-sample Python
    loops, Python integers) for all five grids -- forward within 1e-12, table-gradient rows identical, values within 1e-12;
  * the C oracle (fp32) agrees with it within the derived round-off bounds on what the KAT file lacks: smoothstep, dy_dx, the input
    gradient, max_level < L, D = 4 and 5, fp16 tables.

Worst |err| / bound of the oracle against the reference over the cases below: forward 0.15, dy_dx 0.15, table gradient 0.17,
input gradient 0.05 (a bound of 1.0 is the limit)."""
import os

import numpy as np
import pytest
import torch

import grid_ref64 as R
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
