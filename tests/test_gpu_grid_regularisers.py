"""GPU tests of the two regularisers of the grid encoder, k_grid_tv<D, C> and k_grid_wd (grid.hip: sn_grad_total_variation,
sn_grad_weight_decay), against the fp64 statement of tests/grid_ref64.py (tv_gradient / tv_bound, weight_decay / weight_decay_bound; the
CPU tests of tests/test_grid_ref64.py anchor that statement to a hand-written answer and hold the sequential oracle to the same bounds).

  * every (D, C) the library instantiates, through the raw C ABI;
  * hash / tiled x align_corners on level sets with a dense level whose size is no power of two, hashed levels, tiled levels that wrap
    after the whole walk and tiled levels whose walk stops early (asserted from Grid.hashed / walk / size);
  * placed samples in every case (grid_reg_cases.placed_points): coordinates 0, 1, 1 - 2^-24, -0.0, cell boundaries, two samples just out of
    range, 300 copies of one point; grid_reg_cases.check_tv_coverage asserts from the reference's side that each kind is present -- in particular
    that without align_corners a centre sits at res - 1 and asks for the vertex res, which only the kernel's forced generic modulo folds
    back into the level;
  * ragged and empty batches; the weight decay's level search read out exactly on every row; the module's copy-back branch
    (non-contiguous and half-precision .grad), inputs=None, bound=2, input_dim = 2; rejections.

Every tolerance is a derived bound with its factor 2.  Worst |err| / bound per family (a measurement against the fp64 statement, not a
threshold).  The oracle column is the sequential fp32 oracle on the CPU (tests/test_grid_ref64.py prints it), the kernel column these
tests on an MI355X (they print every ratio, pytest -s; from a zero gradient the two TV families give 0.13):

  family                                         oracle   kernel
  TV, every (D, C), hash                          0.25    0.22
  TV, hash / tiled x align_corners                0.31    0.30
  TV, batch edges (B = 1, 255, 256, 257)          0.20    0.22
  weight decay (distinct sizes, shared cap)       0.23    0.20
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_ref64 as R
import grid_reg_cases as K

pytestmark = pytest.mark.gpu

ERR_INVALID = -1                                                                                 # include/sanerf_hip.h: SN_ERR_INVALID


def _lib():
    from sanerf_hq_amd import _lib as m
    return m


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def hip_tv_rc(grid, x, table, grad, weight, B=None, D=None, C=None):
    m = _lib()
    rc = m.lib().sn_grad_total_variation(_p(x), _p(table), _p(grad), m.host_i32(grid.offsets), weight, x.shape[0] if B is None else B,
                                         grid.D if D is None else D, grid.C if C is None else C, grid.L, grid.S, grid.base,
                                         grid.gridtype, int(grid.align_corners), _stream())
    torch.cuda.synchronize()
    return rc


def hip_tv(grid, x, table, g0, weight):
    grad = g0.clone()
    assert hip_tv_rc(grid, x, table, grad, weight) == 0, _lib().lib().sn_last_error().decode()
    return grad


def hip_wd_rc(grid, table, grad, weight):
    m = _lib()
    rc = m.lib().sn_grad_weight_decay(_p(table), _p(grad), m.host_i32(grid.offsets), weight, grid.rows, grid.C, grid.L, _stream())
    torch.cuda.synchronize()
    return rc


def _case(grid, seed, dev, B=1029):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = K.placed_points(grid, B, gen, dev)
    table = torch.rand(grid.rows, grid.C, generator=gen, device=dev) * 2 - 1
    g0 = torch.randn(grid.rows, grid.C, generator=gen, device=dev)
    return x, table, g0


@pytest.mark.parametrize("D,C", K.TV_DC)
def test_tv_every_instantiation_matches_fp64(gpu, D, C):
    grid = K.tv_dc_grid(D, C)
    assert not grid.hashed[0] and grid.hashed[2]
    x, table, g0 = _case(grid, 100 * D + C, gpu)
    cov = K.check_tv_coverage(grid, x)
    ref = R.tv_gradient(grid, x, table, 0.75)
    ratio = K.assert_tv(hip_tv(grid, x, table, g0, 0.75), g0, ref, grid, "kernel")
    # from a zero gradient the atomics' round-off is relative to the contributions alone: the tighter statement of the same kernel
    zero = torch.zeros_like(g0)
    ratio0 = K.assert_tv(hip_tv(grid, x, table, zero, 0.75), zero, ref, grid, "kernel, zero gradient")
    print(f"tv D={D} C={C}: {ratio:.3f}, from zero {ratio0:.3f}; n <= {cov['pile']}")


@pytest.mark.parametrize("D,C,gridtype,ac", K.TV_MODES)
def test_tv_grid_types_and_align_corners_match_fp64(gpu, D, C, gridtype, ac):
    grid = K.tv_mode_grid(D, C, gridtype, ac)
    K.check_tv_mode_levels(grid)
    x, table, g0 = _case(grid, 1000 * D + 10 * C + 2 * gridtype + ac, gpu)
    K.check_tv_coverage(grid, x)
    ref = R.tv_gradient(grid, x, table, 0.3)
    ratio = K.assert_tv(hip_tv(grid, x, table, g0, 0.3), g0, ref, grid, "kernel")
    zero = torch.zeros_like(g0)
    ratio0 = K.assert_tv(hip_tv(grid, x, table, zero, 0.3), zero, ref, grid, "kernel, zero gradient")
    print(f"tv D={D} C={C} gridtype={gridtype} ac={ac}: {ratio:.3f}, from zero {ratio0:.3f}")


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_tv_batch_edges(gpu, B):
    grid = K.tv_mode_grid(3, 8, 0, False)
    x, table, g0 = _case(grid, 40 + B, gpu, B=B)
    ref = R.tv_gradient(grid, x, table, 0.75)
    assert int(ref["n"].sum()) == int(R.in_range(x).sum()) * grid.L
    print(f"tv B={B}: {K.assert_tv(hip_tv(grid, x, table, g0, 0.75), g0, ref, grid, 'kernel'):.3f}")


def test_tv_empty_batch_leaves_the_gradient_alone(gpu):
    grid = K.tv_mode_grid(3, 8, 0, False)
    x, table, g0 = _case(grid, 41, gpu, B=16)
    grad = g0.clone()
    assert hip_tv_rc(grid, x, table, grad, 0.75, B=0) == 0 and torch.equal(grad, g0)
    # an empty tensor has a NULL data pointer: still an empty batch, not an invalid argument
    assert hip_tv_rc(grid, torch.empty(0, 3, device=gpu), table, grad, 0.75) == 0 and torch.equal(grad, g0)
    # the grid itself is still checked: an empty batch of a shape that is not built stays a bad argument
    assert hip_tv_rc(grid, x, table, grad, 0.75, B=0, D=6) == ERR_INVALID and hip_tv_rc(grid, x, table, grad, 0.75, B=0, C=3) == ERR_INVALID


def _weight_decay(gpu, grid, seed):
    C = grid.C
    gen = torch.Generator(device=gpu).manual_seed(seed)
    table = torch.rand(grid.rows, C, generator=gen, device=gpu) * 2 - 1
    g0 = torch.randn(grid.rows, C, generator=gen, device=gpu)
    grad = g0.clone()
    assert hip_wd_rc(grid, table, grad, 0.1) == 0, _lib().lib().sn_last_error().decode()
    term = R.weight_decay(grid, table, 0.1)
    ratio, _ = R.worst_ratio(grad, g0.double() + term, R.weight_decay_bound(grid, g0, term))
    print(f"weight decay C={C} L={grid.L}: {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # table = 1, gradient 0, weight 0.5: every element is 1.0f / size of the level the kernel's search assigned to its row, exactly -- rows
    # at offsets[l] and offsets[l] - 1 included
    grad = torch.zeros_like(g0)
    assert hip_wd_rc(grid, torch.ones_like(table), grad, 0.5) == 0
    want = R.weight_decay_exact_levels(grid, gpu)
    K.check_wd_level_boundaries(grid)
    assert torch.equal(grad, want), f"rows on another level: {(grad != want).any(dim=1).nonzero().flatten().tolist()[:8]} (offsets {grid.offsets})"


@pytest.mark.parametrize("C,L", K.WD_CL)
def test_weight_decay_matches_fp64_and_finds_every_rows_level(gpu, C, L):
    """Level sizes pairwise distinct (asserted in wd_grid): the exact readout tells every level from every other."""
    _weight_decay(gpu, K.wd_grid(C, L), 10 * C + L)


def test_weight_decay_levels_that_share_the_capped_size(gpu):
    _weight_decay(gpu, K.wd_capped_grid(2), 99)


# ---- through the module --------------------------------------------------------------------------------------------------------------
def _module(gpu, D, C, seed, half=False):
    from sanerf_hq_amd.gridencoder import GridEncoder
    grid = K.tv_mode_grid(D, C, 0, False)
    enc = GridEncoder(input_dim=D, num_levels=4, level_dim=C, base_resolution=6, log2_hashmap_size=8, desired_resolution=384 if D == 2 else 48).to(gpu)
    assert enc.offsets.tolist() == grid.offsets and float(np.float32(np.log2(enc.per_level_scale))) == grid.S
    gen = torch.Generator(device=gpu).manual_seed(seed)
    enc.embeddings.data.copy_(torch.rand(grid.rows, C, generator=gen, device=gpu) * 2 - 1)
    if half:
        enc = enc.half()
        assert enc.embeddings.dtype == torch.float16
    return enc, grid, gen


def _strided_grad(grid, gen, dev, dtype=torch.float32):
    """A [rows, C] gradient that is every second column of a [rows, 2 C] tensor: not contiguous."""
    wide = torch.randn(grid.rows, 2 * grid.C, generator=gen, device=dev).to(dtype)
    g = wide[:, ::2]
    assert not g.is_contiguous() and tuple(g.shape) == (grid.rows, grid.C)
    return wide, g


def _assert_rounded_once(got, g0, added, bound, what):
    """got is in a narrower dtype than fp32: it must be the rounding of SOME fp32 value within `bound` of g0 + added.  Rounding is monotone,
    so that is  round(centre - b) <= got <= round(centre + b); b carries 2 u |centre| more for the two-step conversion of the fp64 ends."""
    centre = g0.double() + added
    b = bound + 2 * R.U * centre.abs()
    lo, hi = (centre - b).float().to(got.dtype).float(), (centre + b).float().to(got.dtype).float()
    bad = (got.float() < lo) | (got.float() > hi)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are not the fp32 result rounded once to {got.dtype}"


@pytest.mark.parametrize("D,C", [(2, 1), (3, 8)])
def test_module_non_contiguous_gradient_is_updated_in_place(gpu, D, C):
    enc, grid, gen = _module(gpu, D, C, 60 + D)
    table = enc.embeddings.detach()
    for call in (enc.grad_total_variation, enc.grad_weight_decay):
        enc.embeddings.grad = None
        with pytest.raises(ValueError, match="grad is None"):                                    # grid.py:189-190, :202-203
            call(0.1)
    x = K.placed_points(grid, 1029, gen, gpu)
    wide, g = _strided_grad(grid, gen, gpu)
    before, g0 = wide.clone(), g.clone()
    enc.embeddings.grad = g
    inputs = x * 4 - 2                                                                           # [-2, 2]; the module maps it back as grid.py:185 does
    enc.grad_total_variation(0.75, inputs, bound=2)
    x01 = ((inputs + 2) / (2 * 2)).contiguous()
    check = R.tv_gradient(grid, x01, table, 0.75)
    assert enc.embeddings.grad.data_ptr() == g.data_ptr() and not enc.embeddings.grad.is_contiguous()
    assert torch.equal(wide[:, 1::2], before[:, 1::2]), "the copy-back wrote outside the gradient's own elements"
    K.assert_tv(wide[:, ::2], g0, check, grid, "module, strided gradient")
    assert int(check["n"].sum()) == int(R.in_range(x01).sum()) * grid.L > 0
    # weight decay on the same strided gradient
    g1 = wide[:, ::2].clone()
    enc.grad_weight_decay(0.1)
    term = R.weight_decay(grid, table, 0.1)
    ratio, _ = R.worst_ratio(wide[:, ::2], g1.double() + term, R.weight_decay_bound(grid, g1, term))
    assert ratio <= 1.0 and torch.equal(wide[:, 1::2], before[:, 1::2]), ratio


@pytest.mark.parametrize("strided", [False, True])
def test_module_half_precision_gradient_is_the_fp32_result_rounded_once(gpu, strided):
    enc, grid, gen = _module(gpu, 3, 8, 70 + strided, half=True)
    table = enc.embeddings.detach().float()
    x = K.placed_points(grid, 1029, gen, gpu)
    wide, g = _strided_grad(grid, gen, gpu, torch.float16)
    if not strided:
        g = g.contiguous()
    g0 = g.clone()
    enc.embeddings.grad = g
    inputs = x * 2 - 1
    enc.grad_total_variation(0.75, inputs)
    x01 = ((inputs + 1) / (2 * 1)).contiguous()
    ref = R.tv_gradient(grid, x01, table, 0.75)
    got = enc.embeddings.grad
    assert got.dtype == torch.float16 and got.data_ptr() == g.data_ptr()
    _assert_rounded_once(got, g0, ref["grad"], R.tv_bound(grid, ref["n"], ref["mass"], g0.float()), "total variation")
    assert torch.equal(got[ref["n"] == 0], g0[ref["n"] == 0])
    g1 = got.clone()
    enc.grad_weight_decay(0.1)
    term = R.weight_decay(grid, table, 0.1)
    _assert_rounded_once(enc.embeddings.grad, g1, term, R.weight_decay_bound(grid, g1.float(), term), "weight decay")


def test_module_draws_its_own_samples_when_given_none(gpu):
    enc, grid, gen = _module(gpu, 2, 1, 80)
    g0 = torch.randn(grid.rows, 1, generator=gen, device=gpu)
    enc.embeddings.grad = g0.clone()
    torch.manual_seed(1234)
    enc.grad_total_variation(0.75, B=777)                                                        # grid.py:181-183: torch.rand(B, input_dim)
    torch.manual_seed(1234)
    x = torch.rand(777, 2, device=gpu)
    ref = R.tv_gradient(grid, x, enc.embeddings.detach(), 0.75)
    assert int(ref["n"].sum()) == 777 * grid.L
    K.assert_tv(enc.embeddings.grad, g0, ref, grid, "module, inputs=None")


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_and_null_pointers_are_refused_before_any_launch(gpu):
    """D and C outside the 24 instantiations are bad arguments of this ABI (sanerf_hip.h: SN_ERR_INVALID, "unsupported D/C") and the message
    names what is built, in the reference's own words (gridencoder.cu:645, :657); the gradient is not touched."""
    l = _lib().lib()
    grid = K.tv_mode_grid(3, 8, 0, False)
    x, table, g0 = _case(grid, 90, gpu, B=64)
    grad = g0.clone()
    x6 = torch.rand(64, 6, device=gpu)
    assert hip_tv_rc(grid, x6, table, grad, 0.75, D=6) == ERR_INVALID and b"D must be 2, 3, 4 or 5" in l.sn_last_error()
    assert hip_tv_rc(grid, x, table, grad, 0.75, C=3) == ERR_INVALID and b"C must be 1, 2, 4, 8, 16 or 32" in l.sn_last_error()
    for args in ((None, table, grad), (x, None, grad), (x, table, None)):
        assert hip_tv_rc(grid, *args, 0.75, B=64) == ERR_INVALID and b"NULL" in l.sn_last_error()
    for args in ((None, grad), (table, None)):
        assert hip_wd_rc(grid, *args, 0.1) == ERR_INVALID and b"NULL" in l.sn_last_error()
    m = _lib()
    assert l.sn_grad_weight_decay(_p(table), _p(grad), None, 0.1, grid.rows, grid.C, grid.L, _stream()) == ERR_INVALID
    assert l.sn_grad_weight_decay(_p(table), _p(grad), m.host_i32(grid.offsets), 0.1, grid.rows, grid.C, 0, _stream()) == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(grad, g0)
