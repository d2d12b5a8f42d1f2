"""CPU: the point-prompt step (sn_rm_points_lift, sn_rm_point_store_update, sn_rm_points_project, sn_rm_prompt_overlay) is exported and
declared, validates its arguments before any launch, its Python operators refuse CPU tensors, PointPrompts reads and writes the reference's
points file, and tests/golden/point_prompts.npz (tools/gen_golden_point_prompts.py: the reference's own lines run on the CPU) agrees with
the float64 restatement of tests/prompts_ref64.py -- every integer output and state exactly -- and keeps its recorded margins."""
import ctypes
import os
import re

import numpy as np
import pytest

import prompts_ref64 as R
from helpers import ROOT, golden

NEW = ("sn_rm_points_lift", "sn_rm_point_store_update", "sn_rm_points_project", "sn_rm_prompt_overlay")
INTS = {"coords": slice(0, 2), "labels_out": 2, "kept_index": 3, "sam_coords": slice(4, 6), "overlay_coords": slice(6, 8), "state": 8}
M_PIXEL, M_DEPTH, M_STORE, M_RGB8 = 1e-2, 1e-3, 1e-4, 1e-2


def project_case(g, name):
    """A projection case of the fixture as a dict (see the layout comments of tools/gen_golden_point_prompts.py)."""
    H, W, N, V, n_intr, crucial_count, valid_threshold = (int(v) for v in g[name + ".meta"])
    c = dict(H=H, W=W, N=N, V=V, n_intr=n_intr, crucial_count=crucial_count, valid_threshold=valid_threshold, points=g[name + ".points"],
             labels=np.ascontiguousarray(g[name + ".flags"][:, 0]), crucial=np.ascontiguousarray(g[name + ".flags"][:, 1]), poses=g[name + ".poses"],
             intrinsics=g[name + ".intrinsics"], depth=g[name + ".depth"], counts=g[name + ".counts"], cam=g[name + ".floats"][..., :3],
             uv=g[name + ".floats"][..., 3:], ratio=1024 / W if W > H else 1024 / H)
    for k, sl in INTS.items():
        c[k] = np.ascontiguousarray(g[name + ".ints"][..., sl])
    return c


def overlay_case(g, name):
    H, W, s, radius, sel = (int(v) for v in g[name + ".meta"])
    pts = g[name + ".points"]
    return dict(H=H, W=W, radius=radius, selected=sel, image=g["image"], masks=None if name == "ov_points_only" else g[f"masks{s}"],
                scores=g[name + ".scores"] if name + ".scores" in g.files else None, pixels=np.ascontiguousarray(pts[:, 0:2]),
                coords=np.ascontiguousarray(pts[:, 2:4]), labels=np.ascontiguousarray(pts[:, 4]), rgb8=g[name + ".rgb8"],
                rgb=g[name + ".rgb"] if name + ".rgb" in g.files else None)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_exported_and_declared():
    from sanerf_hq_amd import _lib, nerf, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/sanerf_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.EXPORTED_SYMBOLS
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12, "the additions are additive: the ABI version stays 12"
    assert re.search(r"#define\s+SN_PROMPT_MAX_POINTS\s+%d\b" % _lib.PROMPT_MAX_POINTS, hdr)
    for f in ("points_lift", "point_store", "point_store_update", "points_project", "prompt_overlay"):
        assert callable(getattr(rm, f))
    for f in ("PointPrompts", "decode_prompts", "decode_overlay"):
        assert callable(getattr(nerf, f))
    assert "prompts.hip" in open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    for lines in ("trainer.py:803-809", "trainer.py:812-834", "trainer.py:838-875", "trainer.py:979-991"):
        assert lines in hdr, f"the declarations name the reference lines they replace ({lines})"


def test_entry_points_validate_their_arguments_before_any_launch():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)
    err = l.sn_last_error
    # points_lift(pixels, M, rays_o, rays_d, depth, depth_stride, H, W, point_3d, stream)
    assert l.sn_rm_points_lift(None, 4, d, d, d, 1, 8, 8, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_points_lift(d, 4, d, d, d, 1, 8, 8, None, None) == -1 and b"NULL" in err()
    assert l.sn_rm_points_lift(d, 4, d, d, d, 0, 8, 8, d, None) == -1 and b"stride" in err()
    assert l.sn_rm_points_lift(d, 4, d, d, d, 1, 0, 8, d, None) == -1 and b"0 x 8" in err()
    assert l.sn_rm_points_lift(d, 4, d, d, d, 1, 1 << 16, 1 << 16, d, None) == -2 and b"2^31" in err()
    assert l.sn_rm_points_lift(None, 0, None, None, None, 0, 0, 0, None, None) == 0
    # point_store_update(xyz, labels, crucial, count, cap, point, label, dist_thresh, status, stream)
    assert l.sn_rm_point_store_update(d, d, d, d, 0, d, d, 0.01, d, None) == -1 and b"capacity 0" in err()
    assert l.sn_rm_point_store_update(d, d, d, d, 1025, d, d, 0.01, d, None) == -2 and b"cap=1025" in err()
    assert l.sn_rm_point_store_update(d, d, d, None, 16, d, d, 0.01, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_point_store_update(d, d, d, d, 16, d, d, 0.01, None, None) == -1 and b"NULL" in err()
    assert l.sn_rm_point_store_update(d, d, d, d, 16, d, d, -1.0, d, None) == -1 and b"dist_thresh" in err()
    assert l.sn_rm_point_store_update(d, d, d, d, 16, d, d, float("nan"), d, None) == -1 and b"dist_thresh" in err()
    # points_project(points, labels, crucial, N, n_points, poses, V, intrinsics, n_intr, depth, depth_stride, H, W, depth_tol, crucial_count,
    #                valid_threshold, resize_ratio, coords, labels_out, kept_index, sam_coords, overlay_coords, cam, uv, state, counts, stream)
    def project(points=d, N=8, V=2, n_intr=1, stride=1, H=8, W=8, ratio=2.0, coords=d, sam=d, counts=d):
        return l.sn_rm_points_project(points, d, None, N, None, d, V, d, n_intr, d, stride, H, W, 0.05, 0, 0, ratio, coords, d, d, sam, d, None, None, None, counts, None)
    assert project(points=None) == -1 and b"NULL input" in err()
    assert project(coords=None) == -1 and b"NULL output" in err()
    assert project(counts=None) == -1 and b"NULL output" in err()
    assert project(n_intr=3) == -1 and b"3 intrinsics for 2 views" in err()
    assert project(stride=0) == -1 and b"stride" in err()
    assert project(W=0) == -1 and b"8 x 0" in err()
    assert project(ratio=-1.0) == -1 and b"resize_ratio" in err()
    assert project(ratio=float("nan")) == -1 and b"resize_ratio" in err()
    assert project(sam=None) == -1 and b"sam_coords" in err()
    assert project(H=1 << 16, W=1 << 16) == -2 and b"2^31" in err()
    assert project(N=1 << 20, V=1 << 12) == -2 and b"2^30" in err()
    assert project(points=None, N=0) == 0 and project(points=None, V=0) == 0
    # prompt_overlay(image, image_stride, H, W, masks, M, scores, mask_index, coords, labels, N, count, radius, alpha, rgb, rgb8, pred_mask, selected, stream)
    def overlay(image=d, stride=3, H=8, W=8, masks=d, M=3, scores=d, index=0, coords=d, N=4, radius=2, rgb=d, rgb8=d, selected=d):
        return l.sn_rm_prompt_overlay(image, stride, H, W, masks, M, scores, index, coords, d, N, d, radius, 0.7, rgb, rgb8, None, selected, None)
    assert overlay(image=None) == -1 and b"NULL image" in err()
    assert overlay(stride=2) == -1 and b"stride" in err()
    assert overlay(H=32768) == -2 and b"32767" in err()
    assert overlay(N=1025) == -2 and b"N=1025" in err()
    assert overlay(coords=None) == -1 and b"NULL coords" in err()
    assert overlay(radius=-1) == -1 and b"radius" in err()
    assert overlay(selected=None) == -1 and b"selected" in err()
    assert overlay(rgb=None, rgb8=None) == -1 and b"no output" in err()
    assert overlay(M=0) == -1 and b"M = 0" in err()
    assert overlay(scores=None, index=3) == -1 and b"mask_index 3" in err()
    assert overlay(rgb8=odd) == -1 and b"aligned" in err()
    assert overlay(image=None, H=0) == 0
    assert l.sn_abi_version() == 12


def test_python_operators_refuse_cpu_tensors_and_bad_options():
    import torch
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import PointPrompts
    H, W = 4, 5
    rays, depth = torch.rand(H * W, 3), torch.rand(H, W)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.points_lift(torch.zeros(1, 2, dtype=torch.int32), rays, rays, depth, H, W)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.point_store_update(rm.point_store("cpu", 8), torch.zeros(3), 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.points_project(torch.rand(3, 3), torch.ones(3, dtype=torch.int32), torch.eye(4)[None], torch.rand(4), depth, H, W)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.prompt_overlay(torch.rand(H * W, 3), torch.zeros(2, 2, dtype=torch.int32), torch.ones(2, dtype=torch.int32), H, W)
    with pytest.raises(RuntimeError, match="CUDA"):
        PointPrompts("cpu", 8).click(rays, rays, depth, (1, 2), 1, H, W)
    with pytest.raises(ValueError, match="capacity"):
        rm.point_store("cpu", 2000)
    with pytest.raises(ValueError, match="unknown outputs"):
        rm.points_project(torch.rand(3, 3), torch.ones(3), torch.eye(4)[None], torch.rand(4), depth, H, W, want=("pixels",))
    with pytest.raises(ValueError, match="unknown outputs"):
        rm.prompt_overlay(torch.rand(H * W, 3), torch.zeros(2, 2), torch.ones(2), H, W, want=("mask",))
    assert rm.reference_resize_ratio(37, 53) == 1024 / 53 and rm.reference_resize_ratio(53, 37) == 1024 / 53 and rm.reference_resize_ratio(8, 8) == 128.0


def test_point_prompts_reads_and_writes_the_points_file():
    """trainer.py:88-112 and save_3d_points (:246-258), on a CPU store (the file handling needs no kernel)."""
    from sanerf_hq_amd.nerf import PointPrompts
    pts = [[0.1 * i, -0.2 * i, 0.05 * i * i] for i in range(7)]
    doc = {"points": pts, "negative_labels": [1, 5], "valid_threshold": -1, "crucial_point_index": [0, 3, 6]}
    p = PointPrompts("cpu", capacity=16).from_json(doc)
    assert int(p.store["count"]) == 7 and p.store["xyz"].shape == (16, 3) and p.store["labels"].dtype == p.store["crucial"].dtype
    assert p.store["labels"][:7].tolist() == [1, 0, 1, 1, 1, 0, 1] and p.store["crucial"][:7].tolist() == [1, 0, 0, 1, 0, 0, 1]
    assert p.crucial_count == 3 and p.valid_threshold == int(7 * 0.8) + 1 == 6
    back = p.to_json()
    assert back["negative_labels"] == [1, 5] and back["crucial_point_index"] == [0, 3, 6] and back["valid_threshold"] == -1
    assert np.array_equal(np.array(back["points"], dtype=np.float32), np.array(pts, dtype=np.float32))
    q = PointPrompts("cpu", capacity=16).from_json(back)
    assert q.to_json() == back and q.valid_threshold == 6 and q.crucial_count == 3
    # an explicit threshold is kept; the one-element tuple save_3d_points writes (a JSON list) is read as its value
    assert PointPrompts("cpu", 16).from_json(dict(doc, valid_threshold=4)).valid_threshold == 4
    assert PointPrompts("cpu", 16).from_json(dict(doc, valid_threshold=4)).to_json()["valid_threshold"] == 4
    assert PointPrompts("cpu", 16).from_json(dict(doc, valid_threshold=[-1])).valid_threshold == 6
    empty = PointPrompts("cpu", 16).to_json()
    assert empty == {"points": [], "negative_labels": [], "valid_threshold": -1, "crucial_point_index": []}
    with pytest.raises(ValueError, match="capacity"):
        PointPrompts("cpu", 4).from_json(doc)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases():
    g = golden("point_prompts")
    cases = [project_case(g, n) for n in g["project_cases"]]
    plain = [c for n, c in zip(g["project_cases"], cases) if n.startswith("p")]
    for shape in ((37, 53), (53, 37)):
        assert sorted(c["N"] for c in plain if (c["H"], c["W"]) == shape) == [1, 63, 64, 65, 130]
    for N in (1, 63, 64, 65, 130):
        assert sorted(c["V"] for c in plain if c["N"] == N) == [1, 3]
    assert {c["n_intr"] for c in plain if c["V"] == 3} == {1, 3}
    off, occ, cru = (project_case(g, n) for n in ("offscreen", "occluded", "crucial"))
    assert off["counts"][0, 0] == 0 and (off["state"] == 0).all()
    assert occ["counts"][0, 0] >= occ["N"] // 2 and occ["counts"][0, 1] == 0 and set(occ["state"].ravel()) == {0, 1}
    assert cru["counts"][0, 1] >= cru["valid_threshold"] and cru["counts"][0, 2] < cru["crucial_count"] and cru["counts"][0, 3] == 0
    valid = np.concatenate([c["counts"][:, 3] for c in cases])
    assert valid.any() and not valid.all()
    assert g["store.counts"].tolist() == [1, 2, 3, 4, 3, 4, 3, 2, 0, 1, 0]          # empty store, appends, one of several, two at once, the last one
    ov = {n: overlay_case(g, n) for n in g["overlay_cases"]}
    assert {(c["H"], c["W"]) for c in ov.values()} == {(37, 53), (53, 37)} and {c["radius"] for c in ov.values()} == {2, 3}
    assert [ov[n]["selected"] for n in ("ov_max0", "ov_max1", "ov_max2", "ov_nonpos", "ov_nan", "ov_empty")] == [0, 1, 2, 0, 2, -1]
    assert (ov["ov_nonpos"]["scores"] <= 0).all() and np.isnan(ov["ov_nan"]["scores"]).sum() == 1
    for n, c in ov.items():
        if n == "ov_empty":
            continue
        H, W, r = c["H"], c["W"], c["radius"]
        xs, ys = set(c["coords"][:, 0].tolist()), set(c["coords"][:, 1].tolist())
        assert {0, 1, r} <= xs and {0, 1, r} <= ys and (W - 1 in xs or W - 2 in xs) and (H - 1 in ys or H - 2 in ys), n
        assert (np.abs(c["coords"][16] - c["coords"][17]).max() <= 1) and c["labels"][16] != c["labels"][17], "two overlapping points, two colours"
    assert {W - 1 for W in (37,)} <= set(ov["ov_points_only"]["coords"][:, 0].tolist()) and 52 in ov["ov_points_only"]["coords"][:, 1].tolist()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "point_prompts.npz")) < 200_000


@pytest.mark.parametrize("name", list(golden("point_prompts")["project_cases"]))
def test_projection_fixture_agrees_with_the_float64_restatement(name):
    """Every integer output, state and count exactly; the reference's own fp32 cam / uv inside the bound the GPU test holds the kernel to."""
    g = golden("point_prompts")
    c = project_case(g, name)
    tol = float(g["constants"][0])
    for v in range(c["V"]):
        intr = c["intrinsics"][v % c["n_intr"]]
        want = R.project_view(c["points"], c["labels"], c["crucial"], c["N"], c["poses"][v], intr, c["depth"][v], c["H"], c["W"], tol,
                              c["crucial_count"], c["valid_threshold"], c["ratio"])
        for k in INTS:
            assert np.array_equal(c[k][v], want["labels" if k == "labels_out" else k]), (name, v, k)
        assert np.array_equal(c["counts"][v], want["counts"]), (name, v)
        assert want["margin_pixel"] >= M_PIXEL and want["margin_depth"] >= M_DEPTH, (name, v, want["margin_pixel"], want["margin_depth"])
        e_cam, e_uv = R.cam_uv_bound(c["points"], c["poses"][v], intr, c["W"])
        d_cam, d_uv = np.abs(c["cam"][v] - want["cam"]), np.abs(c["uv"][v] - want["uv"])
        assert (d_cam <= e_cam).all(), (name, v, float((d_cam / e_cam).max()))
        assert (d_uv <= e_uv).all(), (name, v, float((d_uv / e_uv).max()))
        near = (np.abs(want["uv"]) < 200).all(-1)
        if near.any():                                              # the bound is no blank cheque: on and around the screen it stays below the pixel margin
            assert e_uv[near].max() < M_PIXEL, (name, v, float(e_uv[near].max()))


def test_fixture_keeps_its_recorded_margins():
    g = golden("point_prompts")
    m_pixel, m_depth, m_store, m_rgb8, dev_pixel, dev_depth, share = (float(v) for v in g["margins"])
    assert m_pixel >= M_PIXEL and m_depth >= M_DEPTH and m_store >= M_STORE and m_rgb8 >= M_RGB8
    assert dev_pixel <= M_PIXEL / 10 and dev_depth <= M_DEPTH / 10 and share >= 0.9
    # recomputed, not only read back
    tol, worst_p, worst_d = float(g["constants"][0]), np.inf, np.inf
    for name in g["project_cases"]:
        c = project_case(g, name)
        for v in range(c["V"]):
            w = R.project_view(c["points"], c["labels"], c["crucial"], c["N"], c["poses"][v], c["intrinsics"][v % c["n_intr"]], c["depth"][v], c["H"],
                               c["W"], tol, c["crucial_count"], c["valid_threshold"], c["ratio"])
            worst_p, worst_d = min(worst_p, w["margin_pixel"]), min(worst_d, w["margin_depth"])
    assert abs(worst_p - m_pixel) <= 1e-12 and abs(worst_d - m_depth) <= 1e-9
    a, b = np.float32(g["constants"][2]), np.float32(1.0 - g["constants"][2])
    x = g["image"]
    worst = np.inf
    for v in (x, x * a + x * b, x * a + np.float32(1) * b, x * a + np.float32(0) * b):
        t = 255.0 * v.astype(np.float64)
        worst = min(worst, float(np.abs(t - np.rint(t))[(v != 0) & (v != 1)].min()))
    assert worst >= M_RGB8 and abs(worst - m_rgb8) <= 1e-12


def test_lift_and_store_fixture_agree_with_the_float64_restatement():
    g = golden("point_prompts")
    H, W = g["lift.depth"].shape
    want = R.lift(g["lift.pixels"], g["lift.rays"][0], g["lift.rays"][1], g["lift.depth"], H, W)
    assert np.abs(g["lift.point_3d"] - want).max() <= 2 * R.U * np.abs(want).max() + R.U * 4 * np.sqrt(3)      # two roundings: the product and the sum
    cap, thresh = 8, float(g["constants"][1])
    xyz, labels, crucial, count = np.zeros((cap, 3), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), 0
    worst = np.inf
    for i, (p, lb) in enumerate(zip(g["store.clicks"], g["store.click_labels"])):
        xyz, labels, crucial, count, status, margin = R.store_update(xyz, labels, crucial, count, cap, p, lb, thresh)
        worst = min(worst, margin)
        assert count == g["store.counts"][i] and status[3] == 0
        assert np.array_equal(xyz[:count], g["store.xyz"][i][:count]) and np.array_equal(labels[:count], g["store.labels"][i][:count]), i
    assert worst >= M_STORE and abs(worst - float(g["margins"][2])) <= 1e-9
    # a full store: nothing changes, the overflow word is set
    full = R.store_update(np.arange(6, dtype=np.float32).reshape(2, 3), np.ones(2, np.int32), np.zeros(2, np.int32), 2, 2, np.full(3, 9, np.float32), 0, thresh)
    assert full[3] == 2 and full[4] == (3, 2, 2, 1) and np.array_equal(full[0], np.arange(6, dtype=np.float32).reshape(2, 3))


@pytest.mark.parametrize("name", list(golden("point_prompts")["overlay_cases"]))
def test_overlay_fixture_agrees_with_the_float64_restatement(name):
    g = golden("point_prompts")
    c = overlay_case(g, name)
    alpha = float(g["constants"][2])
    rgb64, rgb32, pred, sel = R.overlay(c["image"], c["H"], c["W"], c["coords"], c["labels"], len(c["coords"]), c["radius"], alpha, c["masks"], c["scores"])
    assert sel == c["selected"]
    assert np.array_equal(R.rgb8(rgb64), c["rgb8"]) and np.array_equal(R.rgb8(rgb32), c["rgb8"])
    if c["rgb"] is not None:
        assert np.array_equal(rgb32, c["rgb"]), "the fp32 chain fl(fl(image a) + fl(over b)) is the reference's, bit for bit"
        np.testing.assert_allclose(c["rgb"], rgb64, rtol=1e-6)
    if len(c["coords"]) and c["masks"] is not None:
        # the round trip through SAM's frame (trainer.py:872-875) of the pixels the tail was handed gives the coordinates it drew
        r = 1024 / max(c["H"], c["W"])
        sam = (c["pixels"].astype(np.float32) * np.float32(r)).astype(np.int32)
        assert np.array_equal((sam / r).astype(np.int32), c["coords"]) and (c["pixels"] != c["coords"]).sum() >= len(c["coords"])


def test_restatement_draws_points_with_python_slices():
    """overlay_point's third quirk, on one point at a time: closer than radius to the top or left edge -> not drawn at all; near the bottom
    or right edge -> clipped and drawn; the last of two overlapping points wins."""
    H, W, r = 9, 11, 2
    img = np.full((H * W, 3), 0.5, dtype=np.float32)
    one = lambda x, y, lb=1: R.overlay(img, H, W, np.array([[x, y]]), np.array([lb]), 1, r, 0.7)[0]
    painted = lambda rgb: (rgb != 0.5).any(-1)
    for x, y in ((0, 0), (1, 5), (5, 1), (1, 1), (0, H - 1)):
        assert not painted(one(x, y)).any(), (x, y)
    assert painted(one(r, r)).sum() == 4 * r * r and painted(one(r, r))[:2 * r, :2 * r].all()
    assert painted(one(W - 1, H - 1)).sum() == (r + 1) ** 2 and painted(one(W - 1, H - 1))[H - 1 - r:, W - 1 - r:].all()
    assert painted(one(W - 1, 4)).sum() == 2 * r * (r + 1)
    assert (one(5, 5, 0)[5, 5] == (0, 1, 0)).all() and (one(5, 5, 3)[5, 5] == (1, 0, 0)).all()
    both = R.overlay(img, H, W, np.array([[5, 5], [6, 6]]), np.array([1, 0]), 2, r, 0.7)[0]
    assert (both[5, 5] == (0, 1, 0)).all() and (both[3, 3] == (1, 0, 0)).all() and (both[7, 7] == (0, 1, 0)).all()
    assert not painted(R.overlay(img, H, W, np.array([[5, 5], [6, 6]]), np.array([1, 0]), 0, r, 0.7)[0]).any()
