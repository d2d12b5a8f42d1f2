"""CPU: the numpy restatement of the device-side batch draw (tests/collate_ref.py) is the algorithm it claims to be -- torch.multinomial's
exponential race -- draws with the right frequencies, and its rays are the golden per-ray-camera rays of tests/golden/rays_multi.npz."""
import numpy as np
import torch

import collate_ref as R
from helpers import golden


def test_selected_set_is_the_top_n_of_weights_over_exponentials():
    """multinomial without replacement is topk(weights / exponential): the n smallest expo / weights are the n largest weights / expo."""
    rng = np.random.default_rng(5)
    for C, n in ((25, 1), (25, 24), (256, 128), (576, 100), (1024, 7)):
        w = rng.random((6, C), dtype=np.float32) + np.float32(0.01)
        e = rng.standard_exponential((6, C)).astype(np.float32)
        got, status = R.weighted_draw(w, e, n)
        top = torch.topk(torch.from_numpy(w) / torch.from_numpy(e), n, dim=1).indices.numpy()
        assert status == 0
        for r in range(6):
            assert set(got[r].tolist()) == set(top[r].tolist()), (C, n, r)
            assert (np.diff(got[r]) > 0).all(), "ascending cell order"


def test_single_draws_follow_the_weights():
    """n = 1 over weights [1,2,3,4], 40 000 rows of seeded exponentials: every cell's frequency within 5 binomial standard deviations of w / 10."""
    rows = 40_000
    w = np.tile(np.array([1, 2, 3, 4], dtype=np.float32), (rows, 1))
    e = np.random.default_rng(11).standard_exponential((rows, 4)).astype(np.float32)
    bits = R.key_bits(w, e)
    first = np.argmin(bits, axis=1)                                 # the restatement's rule for n = 1: smallest key, smaller cell on a tie
    check, _ = R.weighted_draw(w[:500], e[:500], 1)
    assert np.array_equal(check[:, 0], first[:500])
    for c in range(4):
        prob = (c + 1) / 10
        sd = np.sqrt(prob * (1 - prob) / rows)
        assert abs((first == c).mean() - prob) <= 5 * sd, (c, (first == c).mean())


def test_unselectable_cells_ties_and_short_rows():
    w = np.array([[1, 0, -1, np.nan, 1, 1, 1, 1]], dtype=np.float32)
    e = np.array([[1, 1, 1, 1, np.inf, 0, 1, np.nan]], dtype=np.float32)
    got, status = R.weighted_draw(w, e, 3)
    assert got.tolist() == [[0, 5, 6]] and status == 0               # key 0 (expo 0) is selectable; inf and NaN keys are not
    got, status = R.weighted_draw(w, e, 5)
    assert got.tolist() == [[0, 5, 6, -1, -1]] and status == 1
    ones = np.ones((1, 9), dtype=np.float32)
    assert R.weighted_draw(ones, ones, 4)[0].tolist() == [[0, 1, 2, 3]]   # all keys tie: the first n cells
    rows, _ = R.weighted_draw(np.arange(1, 7, dtype=np.float32).reshape(3, 2), np.ones((2, 2), dtype=np.float32), 1, row_u=np.array([0.99, 0.4], dtype=np.float32))
    assert rows.tolist() == [[1], [1]]


def test_pick_keeps_the_largest_uniform_inside():
    one_below = np.nextafter(np.float32(1), np.float32(0))
    for n in (1, 5, 48, 64, 800, 12345):
        assert R.pick(np.array([0.0, one_below], dtype=np.float32), n).tolist() == [0, n - 1]
    # a single fp32 product of the largest uniform with n stays below n for every n < 2^24 (n 2^-24 is at least half an ulp below n, and a tie
    # rounds to the even neighbour, which is not n); the min guards the index all the same, and is what is specified
    ns = np.arange(1, 1 << 16, dtype=np.float32)
    assert (one_below * ns < ns).all()
    assert R.pick(np.array([np.nan, -0.5, 2.0], dtype=np.float32), 7).tolist() == [0, 0, 6]


def test_fmaf_rounds_once():
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) for _ in range(3))
    c = (c * np.float32(1e-3)).astype(np.float32)
    from fractions import Fraction
    got = R.fmaf(a, b, c)
    for k in range(0, 20000, 37):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo, hi = np.nextafter(got[k], np.float32(-np.inf)), np.nextafter(got[k], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[k]))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi)))), k


def test_restated_rays_equal_the_golden_per_ray_cameras():
    """tests/golden/rays_multi.npz pins the reference's get_rays with one camera per ray: the restated gather, fed those (camera, pixel)
    pairs, gives its origins, pixel coordinates and coarse cells exactly and its directions within the bound the GPU suite holds
    rays_from_pixels to (the reference multiplies through a matmul, the kernels through an fma chain)."""
    g = golden("rays_multi")
    H, W = (int(v) for v in g["HW"])
    cam, row, col = g["index"].astype(np.int64), g["coords"][:, 0], g["coords"][:, 1]
    ro, rd = R.rays_of_pixels(g["cams"], g["intr"], cam, row, col)
    assert np.array_equal(ro, g["rays_o"])
    np.testing.assert_allclose(rd, g["rays_d"], rtol=0, atol=3e-7)
    assert np.array_equal(R.coarse_index(row, col, H, W, 32), g["inds_coarse"])
    # the same pixels through the uniform mode: u chosen so that pick() lands on them
    M = g["cams"].shape[0]
    u = np.stack([(cam + 0.5) / M, (row + 0.5) / H, (col + 0.5) / W], axis=-1).astype(np.float32)
    res = R.gather({"poses": g["cams"], "intrinsics": g["intr"]}, H, W, len(cam), u=u, S=32)
    assert np.array_equal(res["index"], cam) and np.array_equal(res["i"], g["i"]) and np.array_equal(res["j"], g["j"])
    assert np.array_equal(res["rays_o"], g["rays_o"]) and np.array_equal(res["rays_d"], rd) and np.array_equal(res["inds_coarse"], g["inds_coarse"])


def test_error_map_mode_and_patches_stay_inside_and_in_ij_order():
    H, W, S, M, N, L, p = 48, 64, 16, 5, 40, 3, 4
    rng = np.random.default_rng(9)
    data = {"poses": rng.standard_normal((M, 4, 4)).astype(np.float32), "intrinsics": np.array([[50, 50, 32, 24]], dtype=np.float32),
            "error_map": rng.random((M, S * S), dtype=np.float32)}
    cells = rng.integers(0, S * S, N)
    cells[3] = -1
    u = rng.random((N, 2), dtype=np.float32)
    u[0], u[1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
    res = R.gather(data, H, W, N, mode="error_map", u=u, cells=cells, index=2, S=S, L=L, p=p, ul=np.array([0.0, 0.5, 0.99], dtype=np.float32),
                   centres=np.array([0, S * S - 1, -1]))
    ok = res["valid"][:N]
    ok[1] = False          # the largest uniform: fl(gx sx + fl(u sx)) may round up to the next cell's first pixel, in the reference as here
    assert (res["row"][:N][ok] // (H // S) == cells[ok] // S).all() and (res["col"][:N][ok] // (W // S) == cells[ok] % S).all()
    assert 0 <= res["row"][1] - (cells[1] // S) * (H // S) <= H // S and res["row"][1] <= H - 1 and res["col"][1] <= W - 1
    assert res["row"][0] == (cells[0] // S) * (H // S) and res["col"][0] == (cells[0] % S) * (W // S)
    assert res["i"][3] == -1 and res["inds_coarse"][3] == -1 and np.isnan(res["rays_d"][3]).all() and np.isnan(res["error_maps"][3])
    assert (res["index"][:N] == 2).all() and res["index"][N:].tolist() == [0] * 16 + [2] * 16 + [4] * 16
    first = slice(N, N + 16)
    assert res["row"][first].tolist() == [r for r in range(4) for _ in range(4)] and res["col"][first].tolist() == list(range(4)) * 4
    second = slice(N + 16, N + 32)                                   # the last cell: 15 * 3 - 2 = 43 = H - p - 1 (the clamp's bound), 15 * 4 - 2 = 58
    assert res["row"][second].min() == H - p - 1 and res["col"][second].min() == 58 and res["row"][second].max() == H - 2
    tall = R.gather(data, H, W, 0, u=np.zeros((0, 3), np.float32), S=S, L=1, p=8, ul=np.array([0.3], dtype=np.float32), centres=np.array([S * S - 1]))
    assert tall["row"].min() == H - 8 - 1 and tall["col"].min() == W - 8 - 1 and tall["col"].max() == W - 2      # both clamped
    assert not res["valid"][N + 32:].any() and np.isnan(res["rays_o"][N + 32:]).all()
