"""CPU: the fp64 SSIM statement of tests/ssim_ref64.py against answers known without any implementation."""
import numpy as np
import pytest
import torch

import ssim_ref64 as ref


def pair(H, W, seed, noise=0.1):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(5 * xx + 3 * yy), 0.5 + 0.4 * np.cos(4 * yy - xx), xx * yy], -1)
    truth = np.clip(base, 0, 1).astype(np.float32)
    pred = np.clip(base + noise * rng.standard_normal(base.shape), 0, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(truth)


SHAPES = [(11, 11), (12, 75), (37, 45), (70, 133), (64, 64), (23, 11)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_identical_images_give_exactly_one(H, W):
    p, _ = pair(H, W, 1)
    assert ref.ssim_valid(p, p) == 1.0 and ref.ssim_valid(p, p, data_range=1.0) == 1.0


@pytest.mark.parametrize("H,W", SHAPES)
def test_padded_and_cropped_equals_valid_window(H, W):
    p, t = pair(H, W, 2)
    for dr in (None, 1.0):
        a, b = ref.ssim_padded(p, t, dr), ref.ssim_valid(p, t, dr)
        print(f"{H}x{W} data_range={dr}: padded - valid = {a - b:.3e}")
        assert abs(a - b) <= 1e-14


@pytest.mark.parametrize("a,b,dr", [(0.25, 0.75, 1.0), (0.999, 0.998, 1e-3), (0.0, 0.5, 2.0)])
def test_two_constant_images(a, b, dr):
    """Exactly, both variances and the covariance are 0 and the second factor is c2 / c2.  The fp64 statement forms them as
    E[xx] - mu^2 from 121-term sums whose weights do not add up to exactly 1: each is off by up to ~ 16 ulp64 of max(a, b)^2, three of
    them enter a ratio whose scale is c2 -- the bound below; it is 3e-12 at data_range 1 and 6e-6 at data_range 1e-3."""
    p, t = torch.full((17, 19, 3), a, dtype=torch.float64), torch.full((17, 19, 3), b, dtype=torch.float64)
    c1, c2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    got = ref.ssim_valid(p, t, data_range=dr)
    bound = 1e-14 + 3 * 16 * 2.0 ** -53 * max(a, b) ** 2 / c2
    print(f"a={a} b={b} data_range={dr}: got - want = {got - want:.3e} (bound {bound:.1e})")
    assert abs(got - want) <= bound, (got, want)


@pytest.mark.parametrize("H,W", SHAPES)
def test_symmetry(H, W):
    p, t = pair(H, W, 3)
    for dr in (None, 1.0):
        assert abs(ref.ssim_valid(p, t, dr) - ref.ssim_valid(t, p, dr)) <= 1e-15


def test_one_window_equals_the_closed_evaluation():
    p, t = pair(11, 11, 4)
    for dr in (1.0, ref.derived_range(p, t)):
        assert abs(ref.ssim_valid(p, t, dr) - ref.ssim_single_window(p, t, dr)) <= 1e-14


def test_edge_conditions_of_the_statement():
    p, t = pair(16, 16, 5)
    with pytest.raises(ValueError, match="smaller"):
        ref.ssim_valid(p[:10], t[:10])
    q = p.clone()
    q[7, 7, 1] = float("nan")
    assert np.isnan(ref.ssim_valid(q, t)) and np.isnan(ref.ssim_valid(q, t, 1.0))
    # (two constant images with a derived range are 0 / 0 in exact arithmetic; the fp64 sums leave round-off in the variances instead, so
    # that case is asserted on the kernel, whose centred moments are exactly 0 there, not on this statement)


def test_near_constant_fixture_value():
    """The fixture of the GPU test: the fp64 value the issue records (0.88949...), and why fp32 needs centred moments there."""
    t = torch.full((64, 64, 3), 0.999, dtype=torch.float32)
    p = t.clone()
    p[10:20, 10:20] = 0.998
    v = ref.ssim_valid(p, t)
    assert abs(ref.derived_range(p, t) - 1e-3) < 1e-7 and abs(v - 0.8895) < 5e-4, v
    assert abs(ref.ssim_f32_torch(p, t) - v) > 1e-2, "the uncentred fp32 statement is not usable here"
