"""tests/mesh_raster_ref.py -- the numpy restatement of the mesh rasteriser -- pinned by values worked by hand and by what a rasteriser has to
do.  CPU only; the device is compared with the restatement bit for bit in tests/test_gpu_mesh_raster.py."""
import numpy as np
import pytest

import mesh_raster_ref as ref

CASES = ref.hand_cases()


def covered(out):
    jj, ii = np.nonzero(out["mask"])
    return {(int(i), int(j)) for i, j in zip(ii, jj)}


@pytest.mark.parametrize("name", ["centres_cw", "centres_ccw", "centres_right", "corners"])
def test_top_left_rule_by_hand(name):
    case = CASES[name]
    out = ref.run_case(case)
    assert covered(out) == case["pixels"]
    assert out["counts"].tolist() == [1, 0, 0, 0]
    assert np.array_equal(out["triangle_id"] >= 0, out["mask"] == 1)
    # z = 1 at every corner: rho = 1 exactly wherever the triangle is seen
    assert np.array_equal(out["depth"], out["mask"].astype(np.float32))


def test_projection_by_hand():
    """A camera at (1, 2, 3) turned by 90 degrees about y: the world point o + 2 (-z_cam) + 0.5 x_cam - 0.25 y_cam."""
    pose = np.array([[0, 0, 1, 1], [0, 1, 0, 2], [-1, 0, 0, 3], [0, 0, 0, 1]], dtype=np.float32)       # columns: x_cam = (0,0,-1), y_cam = (0,1,0), z_cam = (1,0,0)
    v = np.array([[1.0, 2.0, 3.0]]) + 2.0 * np.array([[-1.0, 0.0, 0.0]]) + 0.5 * np.array([[0.0, 0.0, -1.0]]) - 0.25 * np.array([[0.0, 1.0, 0.0]])
    X, Y, r, placed = ref.project(v, pose, [100.0, 80.0, 32.0, 24.0], 0.05)
    # z = 2, x = 100 * 0.5 / 2 + 32 = 57, y = -80 * (-0.25) / 2 + 24 = 34
    assert placed.tolist() == [True] and X.tolist() == [57 * 256] and Y.tolist() == [34 * 256] and r.tolist() == [0.5]


def quad_inside(case):
    """Pixel centres strictly inside the quad (more than 1e-6 from every edge), in fp64."""
    xy = np.stack([case["vertices"][:4, 0], -case["vertices"][:4, 1]], axis=1).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(case["H"]) + 0.5, np.arange(case["W"]) + 0.5, indexing="ij")
    sign = []
    for k in range(4):
        a, b = xy[k], xy[(k + 1) % 4]
        sign.append(((b[0] - a[0]) * (jj - a[1]) - (b[1] - a[1]) * (ii - a[0])) / np.linalg.norm(b - a))
    sign = np.stack(sign)
    return (sign > 1e-6).all(axis=0) | (sign < -1e-6).all(axis=0), (np.abs(sign) <= 1e-6).any(axis=0)


def test_quad_split_both_ways_covers_once():
    a = ref.run_case(CASES["quad_02"], want_coverage=True)
    b = ref.run_case(CASES["quad_13"], want_coverage=True)
    inside, on_edge = quad_inside(CASES["quad_02"])
    assert inside.sum() > 80 and not on_edge.any()
    for out in (a, b):
        assert np.array_equal(out["coverage"], inside.astype(np.int32))        # all 1 inside, no 0 and no 2; nothing outside
    assert np.array_equal(a["mask"], b["mask"])


def test_fan_covers_once():
    out = ref.run_case(CASES["fan"], want_coverage=True)
    cov = out["coverage"]
    assert cov.max() == 1 and cov[8, 8] == 1                 # the shared vertex sits on the centre of pixel (8, 8)
    jj, ii = np.meshgrid(np.arange(17) + 0.5, np.arange(17) + 0.5, indexing="ij")
    rad = np.hypot(ii - 8.5, jj - 8.5)
    inscribed = (6.3 - 1 / 256) * np.cos(np.pi / 12)
    assert (cov[rad < inscribed] == 1).all() and (cov[rad > 6.3 + 1 / 256] == 0).all()
    assert out["counts"].tolist() == [12, 0, 0, 0]
    # the pixels on the spokes through centres: row 8 has centres on no spoke (the ring is turned by 0.1 rad), the shared vertex on all 12
    assert cov.sum() == (out["mask"] == 1).sum()


def test_nearer_wins_in_both_orders_and_lower_index_on_equal_bits():
    last, first, equal = (ref.run_case(CASES[n]) for n in ("overlap_near_last", "overlap_near_first", "overlap_equal"))
    seen = last["mask"] == 1
    assert seen.sum() > 20
    assert (last["triangle_id"][seen] == 1).all() and (first["triangle_id"][seen] == 0).all()
    assert np.array_equal(last["depth"], first["depth"]) and (last["depth"][seen] == 1.0).all()
    assert (equal["triangle_id"][seen] == 0).all() and np.array_equal(equal["mask"], last["mask"])


def test_dropped_whole_with_exact_counts():
    case = CASES["dropped"]
    out = ref.run_case(case)
    assert out["counts"].tolist() == case["counts"]
    alone = ref.rasterize(case["vertices"], case["triangles"][:1], case["pose"], case["intrinsics"], 8, 8)
    for k in ("triangle_id", "depth", "mask"):
        assert np.array_equal(out[k], alone[k])
    status = ref.triangle_status(case["vertices"], case["triangles"], case["pose"], case["intrinsics"], 8, 8)
    assert status.tolist() == [0, 1, 1, 1, 1, 1, 2]           # near, NaN, guard band, index past the end, negative index; a repeated corner


def front_faces(vertices, triangles, eye):
    """Facing of every triangle for an eye position, in fp64: n . (eye - a) / (|n| |eye - a|) with n = (b - a) x (c - a)."""
    a, b, c = (vertices[triangles[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    return np.einsum("ij,ij->i", n, eye - a) / (np.linalg.norm(n, axis=1) * np.linalg.norm(eye - a, axis=1))


def test_cull_keeps_exactly_the_front_faces():
    v, t = ref.icosphere(2, 1.0)
    eye = np.array([1.3, 0.9, 2.6])
    pose, intr, H, W = ref.look_at(eye), [220.0, 220.0, 48.0, 40.0], 80, 96
    facing = front_faces(v, t, eye)
    assert np.abs(facing).min() > 1e-3                       # no face is seen edge-on: the sign is not a matter of rounding
    status = ref.triangle_status(v, t, pose, intr, H, W, cull=True)
    assert np.array_equal(status == 0, facing > 0) and np.array_equal(status == 3, facing < 0)
    # culling the back of a closed surface changes nothing that is seen
    a, b = ref.rasterize(v, t, pose, intr, H, W, cull=True), ref.rasterize(v, t, pose, intr, H, W, cull=False)
    for k in ("triangle_id", "depth", "mask"):
        assert np.array_equal(a[k], b[k])
    assert a["mask"].sum() > 1000
    # reversed orientation: exactly the back faces stay
    status = ref.triangle_status(v, t[:, ::-1], pose, intr, H, W, cull=True)
    assert np.array_equal(status == 0, facing < 0)
    # from inside every face looks away: none is kept; with the orientation reversed every face in front of the camera is
    inside = ref.look_at([0.05, -0.02, 0.03], target=(1.0, 0.3, -0.2))
    status = ref.triangle_status(v, t, inside, intr, H, W, cull=True)
    assert (status != 0).all() and (status == 3).sum() > 20
    reverse = ref.triangle_status(v, t[:, ::-1], inside, intr, H, W, cull=True)
    assert np.array_equal(reverse == 0, status == 3)


def test_icosphere_silhouette_and_depth():
    v, t = ref.icosphere(3, 0.8)
    distance, H, W = 3.0, 72, 80
    intr = [150.0, 150.0, 40.25, 35.5]
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = distance
    r_hi, r_in = ref.facet_inner_radius(v, t)
    assert abs(r_hi - 0.8) < 1e-12 and 0.79 < r_in < 0.8
    out = ref.rasterize(v, t, pose, intr, H, W)
    bound = ref.check_sphere_image(out, H, W, intr, distance, r_hi, r_in)
    assert bound < 0.02             # the bound that was just checked is the sagitta's size, not a loose one


def test_attributes_interpolate_with_perspective():
    """A triangle with depths 1, 2, 4: at a pixel centre the weights are w_k r_k / sum, worked here in rationals."""
    pose, intr = ref.screen_camera()
    v = ref.screen_vertices([(0.5, 0.5), (8.5, 0.5), (0.5, 8.5)], [1.0, 2.0, 4.0])
    colors = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    out = ref.rasterize(v, [(0, 1, 2)], pose, intr, 10, 10, colors=colors, normals=2 * colors, labels=[7, 8, 9], bg_color=0.25)
    # pixel (2, 2): screen barycentrics (1/2, 1/4, 1/4), over z: (1/2, 1/8, 1/16) / (11/16) = (8, 2, 1) / 11
    assert np.allclose(out["image"][2, 2], np.array([8, 2, 1]) / 11, rtol=0, atol=1e-7)
    assert np.allclose(out["normal"][2, 2], 2 * np.array([8, 2, 1]) / 11, rtol=0, atol=2e-7)
    assert out["depth"][2, 2] == np.float32(16 / 11) and out["label"][2, 2] == 7
    # pixel (6, 1): barycentrics (1/8, 6/8, 1/8), over z (1/8, 3/8, 1/32): the second corner has the largest weight
    # pixel (1, 6): barycentrics (1/8, 1/8, 6/8), over z (1/8, 1/16, 3/16): the third, although it is four times as far away
    # pixel (1, 1): barycentrics (6/8, 1/8, 1/8): the first
    assert out["label"][1, 6] == 8 and out["label"][6, 1] == 9 and out["label"][1, 1] == 7
    assert (out["image"][9, 9] == 0.25).all() and (out["normal"][9, 9] == 0).all() and out["label"][9, 9] == 255 and out["triangle_id"][9, 9] == -1
