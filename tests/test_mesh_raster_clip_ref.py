"""CPU: the numpy restatement of the rasteriser's near-plane clipping (tests/mesh_raster_clip_ref.py) against what can be worked by hand or
stated analytically: two cut triangles whose pixel sets follow from the top-left rule, the weights of a pixel, the unclipped definition
where nothing is cut, the corners that still drop a triangle, a sphere and a ground plane around the camera covered exactly once up to the
cut, and independence of the triangle order.  tests/test_gpu_mesh_raster_clip.py holds the device to the same restatement bit for bit."""
import functools

import numpy as np
import pytest

import mesh_raster_clip_ref as cr
import mesh_raster_ref as ref

F32 = np.float32
SNAP = np.sqrt(2.0) / 512           # a snapped corner moves by at most half a sub-pixel step per axis


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pixels(out):
    jj, ii = np.nonzero(out["mask"])
    return {(int(i), int(j)) for i, j in zip(ii, jj)}


def _attributes(V, seed=5):
    rng = np.random.default_rng(seed)
    return dict(colors=rng.random((V, 3), dtype=np.float32), normals=rng.standard_normal((V, 3)).astype(np.float32),
                labels=rng.integers(0, 7, V).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _sphere():
    case = cr.sphere_case()
    return case, cr.run_case(case, want_coverage=True, **_attributes(len(case["vertices"])))


@functools.lru_cache(maxsize=None)
def _ground():
    case = cr.ground_case()
    return case, cr.run_case(case, want_coverage=True, **_attributes(len(case["vertices"])))


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.hand_cases()))
def test_hand_worked_pixel_sets(name):
    case = cr.hand_cases()[name]
    assert len(case["pixels"]) == {"two_front": 72, "behind_camera": 46}[name]
    out = cr.run_case(case, want_coverage=True)
    assert _pixels(out) == case["pixels"]
    assert out["coverage"].max() == 1                          # the two pieces share their diagonal's pixels out between them
    assert out["counts"].tolist() == [1, 0, 0, 0] and out["clip_counts"].tolist() == [1, 2]
    assert out["depth"][0, 0] == 2.0                           # the centre of pixel (0, 0) is the first corner itself
    assert (out["triangle_id"][out["mask"] == 1] == 0).all()
    # the three rotations of the corners and the reversed winding: the same pixels, the same surface
    for order in ((1, 2, 0), (2, 0, 1), (2, 1, 0), (1, 0, 2), (0, 2, 1)):
        other = cr.run_case(dict(case, triangles=np.array([order], dtype=np.int32)), want_coverage=True)
        assert _pixels(other) == case["pixels"], order
        assert other["coverage"].max() == 1 and other["clip_counts"].tolist() == [1, 2]
        np.testing.assert_allclose(other["depth"], out["depth"], rtol=2.0 ** -22, atol=0)          # (the order of an fp64 sum, then one fp32 rounding)
    # clockwise on the screen, A > 0: culled, both pieces; the reversed winding is kept
    culled = cr.run_case(case, cull=True)
    assert culled["counts"].tolist() == [0, 0, 0, 1] and culled["clip_counts"].tolist() == [1, 0] and not culled["mask"].any()
    kept = cr.run_case(dict(case, triangles=np.array([[2, 1, 0]], dtype=np.int32)), cull=True)
    assert kept["counts"].tolist() == [1, 0, 0, 0] and kept["clip_counts"].tolist() == [1, 2] and _pixels(kept) == case["pixels"]
    # without clipping the triangle is dropped whole
    gone = cr.run_case(case, clip=False)
    assert gone["counts"].tolist() == [0, 1, 0, 0] and not gone["mask"].any() and "clip_counts" not in gone


def test_attributes_on_a_hand_worked_pixel():
    """two_front, pixel (4, 4): its centre (4.5, 4.5) lies on the diagonal from p0 = (0.5, 0.5) (the corner 0, r = 1/2) to p2 = (9, 9) (the
    crossing point of the edge 1 -> 2, r = 1), which the top-left rule gives to the piece (p0, p1, p2): for it the diagonal is a left edge.
    tau = 4 / 8.5 = 8/17 along it: w_0 : w_2 = 9 : 8, w_1 = 0, so p = (9/17 * 1/2, 0, 8/17 * 1) = (9/34, 0, 16/34), rho = 25/34, depth 1.36 and
    mu = (9/25, 0, 16/25).  B[p0] = (1, 0, 0) and B[p2] = (0, 1 - s, s) = (0, 1/2, 1/2): lambda = (9/25, 8/25, 8/25).  Check in space:
    0.36 (1, -1, -2) + 0.32 (17, -1, -2) + 0.32 (1, -17, 0) = (6.12, -6.12, -1.36), the point of the pixel's ray at depth 1.36."""
    case = cr.hand_cases()["two_front"]
    colors = np.eye(3, dtype=F32)
    labels = np.array([3, 5, 6], dtype=np.uint8)
    out = cr.run_case(case, colors=colors, normals=-colors, labels=labels)
    lam = np.array([9 / 25, 8 / 25, 8 / 25])
    # fp64 operations on values below 1, then one rounding to fp32: half a unit of 2^-24 at most, and 2^-50 of noise
    assert np.abs(out["image"][4, 4].astype(np.float64) - lam).max() <= 2.0 ** -25 + 2.0 ** -50
    assert np.abs(out["normal"][4, 4].astype(np.float64) + lam).max() <= 2.0 ** -25 + 2.0 ** -50
    assert abs(float(out["depth"][4, 4]) - 1.36) <= 2.0 ** -24 + 2.0 ** -50           # half a unit in the last place of a number in [1, 2)
    assert out["label"][4, 4] == 3                             # the largest lambda is corner 0's
    # pixel (8, 8), centre (8.5, 8.5): tau = 16/17, p = (1/34, 0, 32/34), mu = (1/33, 0, 32/33), lambda = (1/33, 16/33, 16/33): corners 1 and 2
    # tie and the first of them gives the label
    assert np.abs(out["image"][8, 8].astype(np.float64) - np.array([1 / 33, 16 / 33, 16 / 33])).max() <= 2.0 ** -25 + 2.0 ** -50
    assert out["label"][8, 8] in (5, 6)
    # the first corner's own pixel
    assert out["image"][0, 0].tolist() == [1.0, 0.0, 0.0] and out["label"][0, 0] == 3
    # empty pixels keep the background
    assert (out["image"][11, 11] == 1.0).all() and out["label"][11, 11] == 255 and (out["normal"][11, 11] == 0.0).all()


# ---- against the unclipped definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in ref.hand_cases() if n != "dropped"))
@pytest.mark.parametrize("cull", [False, True])
def test_without_a_behind_corner_nothing_changes(name, cull):
    case = ref.hand_cases()[name]
    attr = _attributes(len(case["vertices"]))
    want = ref.run_case(case, cull=cull, want_coverage=True, bg_color=0.75, **attr)
    out = cr.run_case(case, cull=cull, want_coverage=True, bg_color=0.75, **attr)
    assert out["clip_counts"].tolist() == [0, 0]
    for k in want:
        assert out[k].dtype == want[k].dtype and np.array_equal(_bits(out[k]), _bits(want[k])), k


def test_what_still_drops_a_triangle():
    case = ref.hand_cases()["dropped"]
    plain = ref.run_case(case)
    assert plain["counts"].tolist() == case["counts"] == [1, 5, 1, 0]
    out = cr.run_case(case)
    # (0, 1, 3) has its third corner at z = 0.01 < near: cut now, two pieces.  NaN, the guard band and the bad indices drop theirs as before
    assert out["counts"].tolist() == [2, 4, 1, 0] and out["clip_counts"].tolist() == [1, 2]
    assert (out["mask"] >= plain["mask"]).all()
    status = [cr.run_case(dict(case, triangles=case["triangles"][t:t + 1]))["counts"].tolist().index(1) for t in range(len(case["triangles"]))]
    assert status == [0, 0, 1, 1, 1, 1, 2]
    # wholly behind; one corner behind and one bad; a behind corner that is not finite is bad; a crossing point outside the guard band
    v = np.concatenate([case["vertices"], np.array([(0.0, 0.0, 0.5), (1.0, 0.0, 1.0), (0.0, 1.0, -0.01), (np.inf, 0.0, 1.0), (3000.0, 0.0, -0.04)], dtype=F32)])
    tris = np.array([(6, 7, 8), (0, 6, 4), (0, 6, 5), (0, 1, 9), (0, 1, 10), (0, 1, 6)], dtype=np.int32)
    more = cr.run_case(dict(case, vertices=v, triangles=tris))
    # (0, 1, 10): the edge to (3000, 0) at z = 0.04 crosses the plane 0.05 near x = 3000 * 0.99: 60 000 pixels, far outside 2^14
    assert more["counts"].tolist() == [1, 5, 0, 0] and more["clip_counts"].tolist() == [1, 2]


# ---- analytic scenes ------------------------------------------------------------------------------------------------------------------------------
def test_sphere_around_the_camera_is_covered_once_up_to_the_cut():
    case, out = _sphere()
    v, t = case["vertices"].astype(np.float64), case["triangles"]
    f, c, H, W = 20.0, 32.0, case["H"], case["W"]
    near = float(F32(case["near"]))
    r_hi, r_in = ref.facet_inner_radius(v, t)
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    rad = np.hypot(ii - c, jj - c)
    # the plane z = near cuts the surface between the circles of radius sqrt(R^2 - near^2), R = r_in and r_hi, which project to:
    inner, outer = (f * np.sqrt(R * R - near * near) / near for R in (r_in, r_hi))
    inside, outside = rad < inner - SNAP, rad > outer + SNAP
    print("sphere: counts", out["counts"].tolist(), "clip_counts", out["clip_counts"].tolist(), "inner, outer radius", inner, outer,
          "pixels inside", int(inside.sum()))
    assert inside.sum() > 2000 and outside.sum() > 1000
    assert (out["coverage"][inside] == 1).all(), "a hole or a double cover inside the cut circle"
    assert (out["coverage"][outside] == 0).all() and not out["mask"][outside].any()
    assert out["coverage"].max() == 1
    assert out["clip_counts"][0] == 76 and 76 <= out["clip_counts"][1] <= 152
    assert out["counts"][0] + out["counts"][1] == len(t) and out["counts"][2] == 0
    # depth: a ray (u, v, 1) z meets the surface at |p| = R in [r_in, r_hi], z = R / sqrt(q).  A snapped piece shows at a pixel what the true
    # one shows within SNAP of it, so the bounds move by SNAP times their steepest slope |dz/drad| = R rad / (f^2 q^1.5) <= r_hi rad / f^2
    # over the region; and by the fp32 roundings of r and of the depth, a few units of 2^-24 of it.
    region = rad < 0.9 * inner
    q = 1.0 + ((ii - c) / f) ** 2 + ((jj - c) / f) ** 2
    slack = SNAP * r_hi * (0.9 * inner + 1.0) / (f * f) + 16 * 2.0 ** -24 * r_hi
    depth = out["depth"].astype(np.float64)
    assert region.sum() > 1500
    assert (depth[region] >= r_in / np.sqrt(q[region]) - slack).all() and (depth[region] <= r_hi / np.sqrt(q[region]) + slack).all()
    assert (depth[out["mask"] == 1] >= near * (1 - 2.0 ** -22)).all()
    # without clipping the triangles that cross the plane are gone: holes inside the circle
    plain = cr.run_case(case, clip=False)
    holes = int((plain["mask"][inside] == 0).sum())
    print("sphere without clipping: uncovered pixels inside the cut circle:", holes)
    assert holes > 300
    assert np.array_equal(plain["mask"] & out["mask"], plain["mask"])


def test_ground_plane_under_the_camera_is_covered_once_up_to_the_cut():
    case, out = _ground()
    H, W = case["H"], case["W"]
    near = float(F32(case["near"]))
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = jj - 32.0
    with np.errstate(divide="ignore"):
        z = np.where(d > 0, 8.0 / np.where(d > 0, d, 1.0), np.inf)         # the ray of row j meets y = -0.25 at depth 0.25 * 32 / (j + 1/2 - 32)
    x = (ii - 32.0) / 32.0 * z
    inside = (d > 0) & (z >= near * (1 + 1e-3)) & (z <= 4.03 * 0.99) & (np.abs(x) <= 2.0 * 0.99)
    outside = (d <= 0) | (z < near * (1 - 1e-3)) | (z > 4.03 * 1.01) | (np.abs(x) > 2.0 * 1.01)
    print("ground: counts", out["counts"].tolist(), "clip_counts", out["clip_counts"].tolist(), "pixels inside", int(inside.sum()))
    assert inside.sum() == 864
    assert (out["coverage"][inside] == 1).all(), "a hole or a double cover on the plane"
    assert (out["coverage"][outside] == 0).all()
    assert out["coverage"].max() == 1 and out["clip_counts"][0] == 32
    # depth: the snapped surface shows at row coordinate d what the plane shows within SNAP of it, z = 8 / d; and the fp32 roundings
    bound = z[inside] * SNAP / (d[inside] - SNAP) + 16 * 2.0 ** -24 * z[inside]
    assert (np.abs(out["depth"].astype(np.float64)[inside] - z[inside]) <= bound).all()
    plain = cr.run_case(case, clip=False)
    holes = int((plain["mask"][inside] == 0).sum())
    print("ground without clipping: uncovered pixels on the plane:", holes)
    assert holes > 200


@pytest.mark.parametrize("which", ["sphere", "ground"])
def test_triangle_order_does_not_matter(which):
    case, want = {"sphere": _sphere, "ground": _ground}[which]()
    assert want["ties"].max() == 1                             # no two pieces tie anywhere: the winner is the same triangle in any order
    perm = np.random.default_rng(2).permutation(len(case["triangles"]))
    out = cr.run_case(dict(case, triangles=case["triangles"][perm]), **_attributes(len(case["vertices"])))
    for k in ("mask", "depth", "image", "normal", "label", "counts", "clip_counts"):
        assert np.array_equal(_bits(out[k]), _bits(want[k])), k
    ids = out["triangle_id"]
    assert np.array_equal(np.where(ids >= 0, perm[np.maximum(ids, 0)], -1), want["triangle_id"])
