"""GPU tests of two routes of the grid encoder that the host code selects and nothing else in the suite runs, through the raw C ABI
(data_ptr()s into sn_grid_encode_forward / _backward / _backward_binned) and against tests/grid_ref64.py, the fp64 reference.

  * SN_LAYOUT_LBC, the reference's own [L,B,C] output / gradient layout: the branch in k_grid_forward,
    k_grid_backward, k_grid_input_backward, k_bin_scatter and k_bin_pull, and the host routing that goes with it (the row-tiled fast forward
    is [B, L*C] only, so D = 3, C in {2, 4, 8} without dy_dx takes the generic kernel here).  Ragged last workgroups, fp32 and fp16
    tables, with and without dy_dx, max_level < L (forward planes / table rows of the levels left out), atomic and binned backward,
    split bins.
  * the "push" form of the binned scatter (k_bin_scatter + k_bin_accum), which the product build takes for C >= 2 only from 2^22
    samples on: C = 2, 4, 8, 16, 32 at B = 2^22, and B = 2^22 - 1, the last batch of the pull form (the 22-bit sample field full).

Every tolerance is the derived round-off bound of grid_ref64 (u = 2^-24, n and the masses from the fp64 side); the tests print
|err| / bound of every comparison (run with -s to see them).
"""
import ctypes

import pytest
import torch

import grid_ref64 as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
DC = [(2, 1), (2, 16), (3, 2), (3, 4), (3, 8), (3, 32), (4, 2), (4, 8), (5, 1), (5, 4)]       # every D, every C; D = 3 x C in {2, 4, 8} switch kernels with the layout
BS = [1, 255, 257, 1029]                                                                        # ragged last workgroup; with [L,B,C] a level's plane starts at an odd multiple of C floats
SHAPE = {2: (16, 256), 3: (4, 40), 4: (4, 40), 5: (3, 27)}                                      # D: (base, desired) -- with L = 3, log2T = 11: one dense and two hashed levels


def _lib():
    from sanerf_hq_amd import _lib as m
    return m


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ok(rc):
    assert rc == 0, _lib().lib().sn_last_error().decode()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _grid(D, C, **kw):
    base, desired = SHAPE[D]
    g = R.Grid(D, 3, C, 11, base, desired=desired, **kw)
    assert g.hashed == [False, True, True]
    return g


def _inputs(grid, B, gen, dev):
    x = torch.rand(B + 5, grid.D, generator=gen, device=dev)
    x[0] = 0; x[1] = 1; x[2] = 0.5; x[3, 0] = 1.25; x[4, 1] = -0.01                            # edges; two out of range
    return x[:B].contiguous()


def _table(grid, gen, dev, half):
    t = torch.rand(grid.rows, grid.C, generator=gen, device=dev) * 2 - 1
    return t.half() if half else t


def hip_forward(grid, x, table, layout, want_dd, max_level=None, fill=0.0):
    m = _lib()
    B, D, L, C = x.shape[0], grid.D, grid.L, grid.C
    out = torch.full((L, B, C) if layout == m.LAYOUT_LBC else (B, L, C), fill, device=x.device)
    dd = torch.full((B, L * D * C), fill, device=x.device) if want_dd else None
    _ok(m.lib().sn_grid_encode_forward(_p(x), _p(table), m.SN_F16 if table.dtype == torch.float16 else m.SN_F32, m.host_i32(grid.offsets), _p(out),
                                       B, D, C, L, L if max_level is None else max_level, grid.S, grid.base, _p(dd),
                                       grid.gridtype, int(grid.align_corners), grid.interp, layout, _stream()))
    return out, dd


def hip_backward(grid, x, table, grad, layout, dd=None, max_level=None):
    """Atomic kernel.  grad in `layout`; returns (grad_table, grad_inputs or None)."""
    m = _lib()
    B, D, L, C = x.shape[0], grid.D, grid.L, grid.C
    assert grad.is_contiguous() and tuple(grad.shape) == ((L, B, C) if layout == m.LAYOUT_LBC else (B, L, C))
    gt = torch.zeros(grid.rows, C, device=x.device)
    gi = torch.full((B, D), SENTINEL, device=x.device) if dd is not None else None
    _ok(m.lib().sn_grid_encode_backward(_p(grad), _p(x), _p(table), m.SN_F16 if table.dtype == torch.float16 else m.SN_F32, m.host_i32(grid.offsets), _p(gt),
                                        B, D, C, L, L if max_level is None else max_level, grid.S, grid.base, _p(dd), _p(gi),
                                        grid.gridtype, int(grid.align_corners), grid.interp, layout, _stream()))
    return gt, gi


def hip_backward_binned(grid, x, grad, layout, max_level=None):
    m = _lib()
    B, D, L, C = x.shape[0], grid.D, grid.L, grid.C
    assert grad.is_contiguous() and tuple(grad.shape) == ((L, B, C) if layout == m.LAYOUT_LBC else (B, L, C))
    ml = L if max_level is None else max_level
    offs = m.host_i32(grid.offsets)
    need = int(m.lib().sn_grid_backward_binned_workspace_bytes(B, D, C, L, ml, offs))
    assert need > 0, "the binned route must take this shape"
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    gt = torch.zeros(grid.rows, C, device=x.device)
    _ok(m.lib().sn_grid_encode_backward_binned(_p(grad), _p(x), offs, _p(gt), B, D, C, L, ml, grid.S, grid.base,
                                               grid.gridtype, int(grid.align_corners), grid.interp, layout, _p(ws), need, _stream()))
    torch.cuda.synchronize()
    return gt


def _within(got, ref, bound, what):
    ratio, exact = R.worst_ratio(got, ref, bound)
    assert exact, f"{what}: an element whose bound is 0 (no contribution / out of range) is not exactly 0"
    assert ratio <= 1.0, f"{what}: |err| / bound = {ratio}"
    return ratio


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("D,C", DC)
def test_lbc_forward_matches_fp64_and_the_blc_call_bit_for_bit(gpu, D, C, B):
    m = _lib()
    gen = torch.Generator(device=gpu).manual_seed(1000 * D + 10 * C + B)
    grid = _grid(D, C)
    x = _inputs(grid, B, gen, gpu)
    ratios = {}
    for half in (False, True):
        table = _table(grid, gen, gpu, half)
        ref = R.forward(grid, x, table, want_dy_dx=True)
        for want_dd in (False, True):
            lbc, dd_l = hip_forward(grid, x, table, m.LAYOUT_LBC, want_dd)
            blc, dd_b = hip_forward(grid, x, table, m.LAYOUT_BLC, want_dd)
            assert lbc.shape == (3, B, C) and torch.equal(lbc.permute(1, 0, 2), blc), "the two layouts claim the same fmaf chain"
            key = ("f16" if half else "f32") + ("+dd" if want_dd else "")
            ratios[key] = _within(lbc.permute(1, 0, 2), ref["y"], R.forward_bound(grid, ref["y_mass"]), f"forward {key}")
            if want_dd:
                assert torch.equal(dd_l, dd_b), "dy_dx is [B, L*D*C] in both layouts"
                ratios[key + " dy_dx"] = _within(dd_l.view(B, 3, D, C), ref["dy_dx"], R.dy_dx_bound(grid, ref["dy_dx_mass"]), f"dy_dx {key}")
    print(f"lbc forward D={D} C={C} B={B}:", {k: round(v, 3) for k, v in ratios.items()})


@pytest.mark.parametrize("B", [257, 1029])
@pytest.mark.parametrize("D,C", DC)
def test_lbc_forward_max_level_leaves_the_last_plane_to_the_caller(gpu, D, C, B):
    """max_level = 2 of 3: the library documents that the caller zeroes the outputs; under [L,B,C] the third level's plane (and its
    part of dy_dx) keep the caller's fill, the first two are what the full call gives."""
    m = _lib()
    gen = torch.Generator(device=gpu).manual_seed(2000 * D + 10 * C + B)
    grid = _grid(D, C)
    x = _inputs(grid, B, gen, gpu)
    table = _table(grid, gen, gpu, False)
    ref = R.forward(grid, x, table, want_dy_dx=True, max_level=2)
    for want_dd in (False, True):
        out, dd = hip_forward(grid, x, table, m.LAYOUT_LBC, want_dd, max_level=2, fill=SENTINEL)
        assert bool((out[2] == SENTINEL).all()), "plane of a level >= max_level was written"
        _within(out[:2].permute(1, 0, 2), ref["y"][:, :2], R.forward_bound(grid, ref["y_mass"][:, :2]), "forward")
        full, _ = hip_forward(grid, x, table, m.LAYOUT_LBC, want_dd)
        assert torch.equal(out[:2], full[:2])
        if want_dd:
            dd = dd.view(B, 3, D, C)
            assert bool((dd[:, 2] == SENTINEL).all()), "dy_dx of a level >= max_level was written"
            _within(dd[:, :2], ref["dy_dx"][:, :2], R.dy_dx_bound(grid, ref["dy_dx_mass"][:, :2]), "dy_dx")


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("D,C", DC)
def test_lbc_atomic_backward_matches_fp64(gpu, D, C, B):
    """Table gradient and input gradient (from an fp32 and an fp16 table's dy_dx) of the atomic kernels reading an [L,B,C] gradient; with
    max_level = 2 the rows of the third level get exactly zero."""
    m = _lib()
    gen = torch.Generator(device=gpu).manual_seed(3000 * D + 10 * C + B)
    grid = _grid(D, C)
    x = _inputs(grid, B, gen, gpu)
    g = torch.randn(3, B, C, generator=gen, device=gpu)
    gv = g.permute(1, 0, 2)                                                                      # the reference's [B, L, C] view of it
    ratios = {}
    for half in (False, True):
        table = _table(grid, gen, gpu, half)
        _, dd = hip_forward(grid, x, table, m.LAYOUT_LBC, True)
        gt, gi = hip_backward(grid, x, table, g, m.LAYOUT_LBC, dd)
        bt = R.backward_table(grid, x, gv)
        key = "f16" if half else "f32"
        ratios["table " + key] = _within(gt, bt["grad_table"], R.table_grad_bound(grid, bt["n"], bt["mass"]), "table gradient")
        bi = R.backward_input(grid, gv, R.forward(grid, x, table, want_dy_dx=True))
        ratios["input " + key] = _within(gi, bi["grad_inputs"], R.input_grad_bound(grid, bi["mass"]), "input gradient " + key)
    gt, _ = hip_backward(grid, x, table, g, m.LAYOUT_LBC, None, max_level=2)
    bt = R.backward_table(grid, x, gv, max_level=2)
    assert int(bt["n"][grid.offsets[2]:].sum()) == 0 and not bool(gt[grid.offsets[2]:].any()), "rows of a level >= max_level got gradient"
    ratios["table max_level"] = _within(gt, bt["grad_table"], R.table_grad_bound(grid, bt["n"], bt["mass"]), "table gradient, max_level 2")
    print(f"lbc atomic backward D={D} C={C} B={B}:", {k: round(v, 3) for k, v in ratios.items()})


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("D,C", [(d, c) for d, c in DC if d <= 3] + [(2, 4), (3, 1)])
def test_lbc_binned_backward_matches_fp64(gpu, D, C, B):
    m = _lib()
    gen = torch.Generator(device=gpu).manual_seed(4000 * D + 10 * C + B)
    grid = _grid(D, C)
    x = _inputs(grid, B, gen, gpu)
    g = torch.randn(3, B, C, generator=gen, device=gpu)
    gv = g.permute(1, 0, 2)
    ratios = {}
    for ml in (3, 2):
        bt = R.backward_table(grid, x, gv, max_level=ml)
        bound = R.table_grad_bound(grid, bt["n"], bt["mass"])
        ratios[f"lbc max_level {ml}"] = _within(hip_backward_binned(grid, x, g, m.LAYOUT_LBC, ml), bt["grad_table"], bound, f"binned, [L,B,C], max_level {ml}")
        ratios[f"blc max_level {ml}"] = _within(hip_backward_binned(grid, x, gv.contiguous(), m.LAYOUT_BLC, ml), bt["grad_table"], bound, f"binned, [B,L*C], max_level {ml}")
    print(f"lbc binned backward D={D} C={C} B={B}:", {k: round(v, 3) for k, v in ratios.items()})


@pytest.mark.parametrize("D,C", [(3, 8), (3, 2), (2, 4), (3, 1)])
def test_lbc_binned_backward_split_bins(gpu, D, C):
    """Half of 70 001 samples piled on one spot: bins far over an item's capacity are split, and every item of a split bin reads the
    [L,B,C] gradient too (references for C >= 2, products for C = 1)."""
    m = _lib()
    B = 70001
    gen = torch.Generator(device=gpu).manual_seed(5000 * D + C)
    grid = _grid(D, C)
    x = _inputs(grid, B, gen, gpu)
    k = B // 2
    x[5:5 + k] = (torch.rand(1, D, generator=gen, device=gpu) * 0.4 + 0.3 + 2e-3 * torch.randn(k, D, generator=gen, device=gpu)).clamp_(0, 1)
    g = torch.randn(3, B, C, generator=gen, device=gpu)
    bt = R.backward_table(grid, x, g.permute(1, 0, 2))
    assert int(bt["n"].max()) > 12096, "one row beyond an item's capacity (12096 / C entries): its bin must split"
    bound = R.table_grad_bound(grid, bt["n"], bt["mass"])
    r_b = _within(hip_backward_binned(grid, x, g, m.LAYOUT_LBC), bt["grad_table"], bound, "binned")
    r_a = _within(hip_backward(grid, x, torch.zeros(1, device=gpu), g, m.LAYOUT_LBC)[0], bt["grad_table"], bound, "atomic")
    print(f"lbc split bins D={D} C={C}: binned {r_b:.4f} atomic {r_a:.4f}")


# ---- the binned scatter at and above 2^22 samples -------------------------------------------------------------------------------------
P22 = 1 << 22
N_MAX = 1024
BIG = {
    # name: (D, C, L, log2T, base, desired, gridtype, align_corners, B, layout is [L,B,C])
    "d3c2_hash_last_pull": (3, 2, 2, 17, 64, 128, 0, False, P22 - 1, False),       # 22-bit sample field full: the last batch of the pull form
    "d3c2_hash": (3, 2, 2, 17, 64, 128, 0, False, P22, False),                     # branch-free row addressing
    "d3c2_hash_last_pull_lbc": (3, 2, 2, 17, 64, 128, 0, False, P22 - 1, True),
    "d3c2_hash_lbc": (3, 2, 2, 17, 64, 128, 0, False, P22, True),
    "d3c4_tiled": (3, 4, 2, 17, 64, 128, 1, False, P22, False),                    # generic addressing
    "d3c8_hash": (3, 8, 1, 17, 64, None, 0, False, P22, False),
    "d2c2_dense": (2, 2, 2, 19, 256, 512, 0, False, P22, False),
    "d2c16": (2, 16, 1, 19, 256, None, 0, False, P22, False),
    "d3c32_hash_ac": (3, 32, 1, 17, 64, None, 0, True, P22, False),
}


def test_push_cases_reach_every_channel_count():
    """k_bin_scatter<D, C> + k_bin_accum<C> run in the product build only where C >= 2 and B >= 2^22 (grid_binned.hip: `pull`)."""
    assert {c[1] for c in BIG.values() if c[8] >= P22} == {2, 4, 8, 16, 32}
    assert any(c[8] == P22 - 1 for c in BIG.values())


def _thinned_uniform(grid, B, gen, dev):
    """Uniform samples, the last three out of range.  A hashed level of 64^3 vertices in 2^17 rows folds up to a dozen vertices into one
    row (1500 contributions where the mean is 256), which would put n beyond N_MAX; the bound stays, the inputs give way: samples
    that touch a row beyond N_MAX are drawn again with probability 1 - 800 / n, until no row is."""
    x = torch.rand(B, grid.D, generator=gen, device=dev)
    x[-3:] = 1.5
    for _ in range(8):
        n = R.contributions(grid, x)
        if int(n.max()) <= N_MAX:
            break
        keep = torch.where(n > N_MAX, 800.0 / n.double().clamp_(min=1.0), torch.ones((), dtype=torch.float64, device=dev))
        again = torch.rand(B, generator=gen, device=dev).double() > R.min_over_rows(grid, x, keep)
        again[-3:] = False
        x[again] = torch.rand(int(again.sum()), grid.D, generator=gen, device=dev)
    return x


@pytest.mark.parametrize("name", list(BIG))
def test_binned_scatter_at_and_above_2p22_samples(gpu, name):
    m = _lib()
    D, C, L, log2T, base, desired, gridtype, ac, B, lbc = BIG[name]
    assert C >= 2 and (B >= P22 or (B == P22 - 1 and C == 2)), "B >= 2^22 with C >= 2 is the push form; 2^22 - 1 the last pull batch"
    gen = torch.Generator(device=gpu).manual_seed(sorted(BIG).index(name) + 77)
    grid = R.Grid(D, L, C, log2T, base, desired=desired, gridtype=gridtype, align_corners=ac)
    x = _thinned_uniform(grid, B, gen, gpu)
    assert not bool(R.in_range(x)[-3:].any()) and int(R.in_range(x).sum()) == B - 3
    g = torch.randn((L, B, C) if lbc else (B, L, C), generator=gen, device=gpu)
    gv = g.permute(1, 0, 2) if lbc else g
    layout = m.LAYOUT_LBC if lbc else m.LAYOUT_BLC
    bt = R.backward_table(grid, x, gv)
    n = bt["n"]
    assert int(n.max()) <= N_MAX, int(n.max())                 # one missing contribution of ~256 stays far above the round-off bound
    bound = R.table_grad_bound(grid, n, bt["mass"])
    got = {"binned": hip_backward_binned(grid, x, g, layout), "atomic": hip_backward(grid, x, torch.zeros(1, device=gpu), g, layout)[0]}
    ratios = {}
    for k, gt in got.items():                                 # both held to the same bound: a failure says which side is wrong
        ratios[k] = _within(gt, bt["grad_table"], bound, k)
    # partition of unity per level and channel: the rows of a level sum to the in-range samples' gradient.  The allowed error is the
    # round-off of the additions behind those rows -- the sum of their bounds; it catches a dropped or doubled block of samples
    # whatever the rows' statistics, and it does not go through the index arithmetic of the reference.
    want = gv[R.in_range(x)].double().sum(0)
    for l in range(L):
        rows = slice(grid.offsets[l], grid.offsets[l + 1])
        allowed = bound[rows].sum(0)
        for k, gt in got.items():
            err = (gt[rows].double().sum(0) - want[l]).abs()
            ratios[f"{k} level {l} sum"] = float((err / allowed).max())
            assert bool((err <= allowed).all()), (k, l, err, allowed)
    print(f"2^22 scatter {name}: n <= {int(n.max())}, mean {float(n.double().mean()):.0f};", {k: round(v, 4) for k, v in ratios.items()})
