#!/usr/bin/env python3
"""Generate tests/golden/point_prompts.npz by running the REFERENCE's own code on the CPU:

  * the lift of a click (nerf/trainer.py:803-809), the add-or-remove rule of the remembered points (:812-834), their projection into a
    view with the screen and depth tests as test_step (:839-868) and as decode_step (:932-971) state them, and decode_step's tail
    (:972-991: the round trip through SAM's frame, the score selection, the overlays).  These lines sit inside larger methods, so they are
    read from the reference's source file at run time and executed as they are, on tensors made here, with a stub standing for sam_predict;
  * the reference's own overlay_mask / overlay_point (nerf/utils.py), which those lines call, and overlay_point alone for the overlay
    without a decoder (trainer.py:884).

    python tools/gen_golden_point_prompts.py --reference <checkout of the reference>

Third-party modules the reference imports at module level and that are not installed are replaced by empty stubs (none is used on these
paths).  The fixture holds arrays only.

The outputs have discontinuities: the truncation of the pixel coordinates and the screen test, the depth test, the distance test of the
store, the truncation to 8 bits.  The generator draws three times the points (pixels) it needs and keeps the first ones that stay away
from all of them, builds the depth images from the kept ones, then runs the reference on them, asserts the margins and records them:
  margin_pixel  >= 1e-2   uv, evaluated in float64 with numpy.linalg.inv, from every integer and from -1, W and H;
  margin_depth  >= 1e-3   | |point depth - rendered depth| - 0.05 |;
  margin_store  >= 1e-4   | distance - 0.01 |;
  dev_pixel, dev_depth    what the reference's own fp32 uv and depth differ from the float64 statement by: at most a tenth of the margins;
  share_kept    >= 0.9    the share of a view's drawn points that pass the pixel margin, the lowest over the views (below that the draw is
                          wrong, not the margin);
  margin_rgb8   >= 1e-2   between 255 x and the nearest integer, exact 0 and exact 1 apart, for every image value x and every blend of it
                          (x itself, 0.7 x + 0.3 x, 0.7 x + 0.3, 0.7 x + 0): the rule of tools/gen_golden_mask_output.py.
"""
import argparse
import importlib
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

DEPTH_TOL, DIST_THRESH, ALPHA = 0.05, 0.01, 0.7
M_PIXEL, M_DEPTH, M_STORE, M_RGB8 = 1e-2, 1e-3, 1e-4, 1e-2
FAR = 7.5                                                             # the depth images' background
SHAPES = ((37, 53), (53, 37))
#                name        H   W    N  V  intrinsics  kind
# every N with both shapes, one of them with one view and the other with three; the three-view cases with 1 and with V intrinsics in turn
PROJECT_CASES = [(f"p{H}x{W}_n{N}_v{V}", H, W, N, V, (V if V > 1 and (i + s) % 4 == 1 else 1), "plain")
                 for s, (H, W) in enumerate(SHAPES) for i, N in enumerate((1, 63, 64, 65, 130)) for V in ((1, 3)[(i + s) % 2],)]
PROJECT_CASES += [("offscreen", 37, 53, 65, 1, 1, "offscreen"), ("occluded", 53, 37, 65, 1, 1, "occluded"), ("crucial", 37, 53, 64, 1, 1, "crucial")]


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference(ref):
    sys.path.insert(0, ref)
    for _ in range(32):
        try:
            return importlib.import_module("nerf.trainer"), importlib.import_module("nerf.utils")
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Stub(e.name)
            for k in [k for k in sys.modules if k.startswith("nerf")]:
                del sys.modules[k]
    raise RuntimeError("could not import the reference's nerf package")


_SRC = {}


def source_lines(ref, first, last, must_contain):
    if ref not in _SRC:
        _SRC[ref] = open(os.path.join(ref, "nerf", "trainer.py")).read().splitlines()
    text = textwrap.dedent("\n".join(_SRC[ref][first - 1:last]))
    assert must_contain in text, f"trainer.py:{first}-{last} is not the expected block"
    return text


# ---- cameras, points, depth images --------------------------------------------------------------------------------------------------
def look_at(eye, target, roll):
    """cam2world [4,4] float32 of a camera at `eye` that looks along its -z axis at `target`."""
    back = eye - target
    back /= np.linalg.norm(back)
    up0 = np.array([np.sin(roll), np.cos(roll), 0.0])
    right = np.cross(up0, back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, up, back, eye
    return pose.astype(np.float32)


def uv_f64(points, pose, intr, W):
    w2c = np.linalg.inv(pose.astype(np.float64))
    cam = np.concatenate([points.astype(np.float64), np.ones((len(points), 1))], -1) @ w2c.T
    fx, fy, cx, cy = (float(v) for v in intr)
    with np.errstate(all="ignore"):
        uv = np.stack([W - (fx * cam[:, 0] / cam[:, 2] + cx), fy * cam[:, 1] / cam[:, 2] + cy], -1)
    return cam[:, :3], uv


def pixel_distance(uv, H, W):
    """Distance of every coordinate from the nearest integer (which covers -1, W and H); inf -> 0."""
    d = np.abs(uv - np.rint(uv))
    return np.where(np.isfinite(uv), d, 0.0).min(-1)


def on_screen_f64(uv, H, W):
    return (uv[:, 0] > -1) & (uv[:, 0] < W) & (uv[:, 1] > -1) & (uv[:, 1] < H)


def make_views(rng, H, W, V, n_intr, kind):
    poses, intrs = [], []
    for v in range(V):
        az, el = rng.uniform(0, 2 * np.pi), rng.uniform(-0.5, 0.5)
        eye = rng.uniform(1.6, 2.2) * np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
        target = rng.uniform(-0.15, 0.15, 3)
        if kind == "offscreen":                                       # from twice as far, looking along a tangent: the scene is 64 degrees and more off the axis
            eye = 2.0 * eye
            target = eye + np.cross(eye, np.array([0.3, 1.0, 0.2]))
        poses.append(look_at(eye, target, rng.uniform(-0.3, 0.3)))
    for v in range(n_intr):
        intrs.append(np.array([rng.uniform(45, 57), rng.uniform(45, 57), W / 2 + rng.uniform(-2, 2), H / 2 + rng.uniform(-2, 2)], dtype=np.float32))
    return np.stack(poses), np.stack(intrs)


def make_project_case(rng, H, W, N, V, n_intr, kind):
    poses, intrs = make_views(rng, H, W, V, n_intr, kind)
    cand = rng.uniform(-1.0, 1.0, (3 * max(N, 64), 3)).astype(np.float32)   # three times the points (of at least 64: a share of 3 says nothing)
    ok, share = np.ones(len(cand), bool), 1.0
    taken = [set() for _ in range(V)]
    for v in range(V):
        _, uv = uv_f64(cand, poses[v], intrs[v % n_intr], W)
        fine = pixel_distance(uv, H, W) >= M_PIXEL
        share = min(share, float(fine.mean()))
        ok &= fine
    chosen = []
    for i in np.flatnonzero(ok):                                       # one point per pixel and view: the depth image serves each point alone
        pix = []
        for v in range(V):
            _, uv = uv_f64(cand[i:i + 1], poses[v], intrs[v % n_intr], W)
            pix.append(tuple(np.trunc(uv[0]).astype(int)) if on_screen_f64(uv, H, W)[0] else None)
        if any(p is not None and p in taken[v] for v, p in enumerate(pix)):
            continue
        for v, p in enumerate(pix):
            if p is not None:
                taken[v].add(p)
        chosen.append(i)
        if len(chosen) == N:
            break
    assert len(chosen) == N, (len(chosen), N)
    points = np.ascontiguousarray(cand[chosen])
    labels = (rng.uniform(size=N) < 0.7).astype(np.int32)
    crucial = (rng.uniform(size=N) < 0.15).astype(np.int32)
    depth = np.full((V, H, W), FAR, dtype=np.float32)
    for v in range(V):
        cam, uv = uv_f64(points, poses[v], intrs[v % n_intr], W)
        on = on_screen_f64(uv, H, W)
        for i in np.flatnonzero(on):
            x, y = np.trunc(uv[i]).astype(int)
            seen = kind != "occluded" and rng.uniform() < 0.6
            if kind == "crucial" and crucial[i]:
                seen = False                                           # the crucial points are hidden in this view
            off = rng.uniform(-0.04, 0.04) if seen else rng.choice([-1, 1]) * rng.uniform(0.06, 0.4)
            depth[v, y, x] = np.float32(-cam[i, 2] + off)
    return points, labels, crucial, poses, intrs, depth, share


# ---- the reference's lines ------------------------------------------------------------------------------------------------------------
def run_view(ref, utils, points, labels, crucial, pose, intr, depth, H, W, crucial_count, valid_threshold):
    """trainer.py:839-868 (test_step) and :932-971 + :972-991 (decode_step) for one view."""
    N = len(points)
    me = types.SimpleNamespace(point_3d=torch.from_numpy(points), input_labels=torch.from_numpy(labels), crucial_point_label=torch.from_numpy(crucial),
                               crucial_point_count=crucial_count, valid_threshold=valid_threshold)
    data = {"poses": torch.from_numpy(pose)[None], "intrinsics": torch.from_numpy(intr)[None]}
    base = dict(torch=torch, np=np, self=me, data=data, H=H, W=W, pred_depth=torch.from_numpy(depth))
    ts = dict(base)
    exec(source_lines(ref, 839, 868, "unoccluded_mask"), ts)
    ns = dict(base)
    exec(source_lines(ref, 932, 971, "is_valid"), ns)
    cam = ns["point_3d_cam"][:, :3].numpy().copy()
    fx, fy, cx, cy = (torch.tensor(v) for v in intr)
    c = ns["point_3d_cam"]
    uv = torch.stack([W - (fx * c[:, 0] / c[:, 2] + cx), fy * c[:, 1] / c[:, 2] + cy], -1).numpy()      # the floats behind the block's .long()
    screen = ns["screen_mask"].numpy()
    state = np.zeros(N, dtype=np.int32)
    if screen.any():
        state[np.flatnonzero(screen)] = np.where(ns["unoccluded_mask"].numpy(), 2, 1)
    kept = np.flatnonzero(state == 2)
    out = dict(coords=np.zeros((N, 2), np.int32), labels=np.full(N, -1, np.int32), kept_index=np.full(N, -1, np.int32),
               sam_coords=np.zeros((N, 2), np.int32), overlay_coords=np.zeros((N, 2), np.int32), cam=cam, uv=uv, state=state)
    k = len(kept)
    crucial_kept = 0
    if ns["inputs_point_coords"] is not None:
        assert len(ns["inputs_point_coords"]) == k and np.array_equal(ns["inputs_point_coords"], ts["inputs_point_coords"])
        assert np.array_equal(ns["inputs_point_labels"], ts["inputs_point_labels"]) and np.array_equal(ns["inputs_point_labels"], labels[kept])
        crucial_kept = int(ns["inputs_crucial_point_label"].sum())
        # the tail: a stub decoder with one empty mask; the image does not matter here
        tail = dict(base, inputs_point_coords=ns["inputs_point_coords"], inputs_point_labels=ns["inputs_point_labels"], pred_samvit=None,
                    pred_rgb=torch.zeros(H, W, 3), overlay_mask=utils.overlay_mask, overlay_point=utils.overlay_point)
        me.sam_predict = lambda *a, **kw: (torch.zeros(1, H, W, dtype=torch.bool), np.array([1.0], np.float32), None, None)
        exec(source_lines(ref, 972, 991, "overlay_point"), tail)
        out["coords"][:k] = ns["inputs_point_coords"]
        out["labels"][:k] = ns["inputs_point_labels"]
        out["kept_index"][:k] = kept
        out["sam_coords"][:k] = tail["point_coords"]
        out["overlay_coords"][:k] = tail["original_point_coords"]
        assert abs(tail["resize_ratio"] - 1024 / max(H, W)) == 0
    else:
        assert k == 0 and ts["inputs_point_coords"] is None
    out["counts"] = np.array([int(screen.sum()), k, crucial_kept, int(bool(ns["is_valid"]))], dtype=np.int32)
    return out


def run_decode_tail(ref, utils, image, masks, scores, coords, labels, H, W, radius):
    """trainer.py:972-991 on a decoder's masks and scores; radius: overlay_point's default is 2, another one goes through a wrapper of it."""
    me = types.SimpleNamespace(sam_predict=lambda *a, **kw: (torch.from_numpy(masks), scores, None, None))
    point = utils.overlay_point if radius == 2 else (lambda im, pts, inputs_point_labels=None: utils.overlay_point(im, pts, radius=radius, inputs_point_labels=inputs_point_labels))
    ns = dict(torch=torch, np=np, self=me, H=H, W=W, pred_samvit=None, pred_rgb=torch.from_numpy(image).reshape(H, W, 3).clone(),
              inputs_point_coords=coords if len(coords) else None, inputs_point_labels=labels, overlay_mask=utils.overlay_mask, overlay_point=point)
    exec(source_lines(ref, 972, 991, "overlay_point"), ns)
    if len(coords):
        return ns["pred_rgb"].numpy().copy(), ns["pred_masks"][0].numpy().copy(), int(ns["index"]), ns["original_point_coords"]
    assert float(ns["pred_masks"].abs().max()) == 0.0
    return ns["pred_rgb"].numpy().copy(), np.zeros((H, W), bool), -1, np.zeros((0, 2), np.int32)


def rgb8_distance(x):
    v = 255.0 * x.astype(np.float64)
    d = np.abs(v - np.rint(v))
    return np.where((x == 0.0) | (x == 1.0), np.inf, d)


def blends(x):
    a, b = np.float32(ALPHA), np.float32(1.0 - ALPHA)
    return [x, x * a + x * b, x * a + np.float32(1) * b, x * a + np.float32(0) * b]


def make_image(rng, n):
    cand = rng.uniform(0.02, 0.98, (3 * n, 3)).astype(np.float32)
    d = np.min([rgb8_distance(v).min(-1) for v in blends(cand)], axis=0)
    ok = np.flatnonzero(d >= M_RGB8)
    assert len(ok) >= n
    return np.ascontiguousarray(cand[ok[:n]])


def make_masks(rng, M, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((M, H, W), bool)
    for j in range(M):
        cy, cx, ry, rx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.5) * H, rng.uniform(0.2, 0.5) * W
        out[j] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


def edge_points(H, W, r):
    """x, y in {0, 1, r, W-1, H-1}, and two overlapping points with different labels."""
    xs, ys = [0, 1, r, W - 1], [0, 1, r, H - 1]
    pts = [(x, y) for x in xs for y in ys] + [(W // 2, H // 2), (W // 2 + 1, H // 2 + 1), (W - 1, r), (r, H - 1)]
    labels = [(i * 7 + 3) % 3 != 0 for i in range(len(pts))]
    labels[16], labels[17] = 1, 0                                       # the overlapping pair
    return np.array(pts, dtype=np.int64), np.array(labels, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(GOLD, "point_prompts.npz"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    ref = args.reference
    _, utils = import_reference(ref)
    # constants = depth_tol, dist_thresh, alpha;  margins (below) = pixel, depth, store, rgb8, dev_pixel, dev_depth, share_kept
    arrays = dict(constants=np.array([DEPTH_TOL, DIST_THRESH, ALPHA]), project_cases=np.array([c[0] for c in PROJECT_CASES]))

    # ---- projection ---------------------------------------------------------------------------------------------------------------
    worst = dict(pixel=np.inf, depth=np.inf, dev_pixel=0.0, dev_depth=0.0, share=1.0)
    for n, (name, H, W, N, V, n_intr, kind) in enumerate(PROJECT_CASES):
        rng = np.random.default_rng(500 + n)
        points, labels, crucial, poses, intrs, depth, share = make_project_case(rng, H, W, N, V, n_intr, kind)
        crucial_count = int(crucial.sum()) if kind == "crucial" else min(2, int(crucial.sum()))      # the trainer's count is a free number to the step
        valid_threshold = max(1, N // 4)
        views = []
        for v in range(V):
            o = run_view(ref, utils, points, labels, crucial, poses[v], intrs[v % n_intr], depth[v], H, W, crucial_count, valid_threshold)
            cam64, uv64 = uv_f64(points, poses[v], intrs[v % n_intr], W)
            on = on_screen_f64(uv64, H, W)
            assert np.array_equal(on, o["state"] >= 1), name
            worst["pixel"] = min(worst["pixel"], float(pixel_distance(uv64, H, W).min()))
            fin = (np.abs(uv64) < 200).all(-1)                         # within 200 pixels of the image: far outside, the coordinates' own ulp grows
            worst["dev_pixel"] = max(worst["dev_pixel"], float(np.abs(o["uv"][fin] - uv64[fin]).max()))
            worst["dev_depth"] = max(worst["dev_depth"], float(np.abs(o["cam"][:, 2] - cam64[:, 2]).max()))
            if on.any():
                px = np.trunc(uv64[on]).astype(int)
                gap = np.abs(-cam64[on, 2] - depth[v][px[:, 1], px[:, 0]].astype(np.float64))
                worst["depth"] = min(worst["depth"], float(np.abs(gap - DEPTH_TOL).min()))
                assert np.array_equal(gap <= DEPTH_TOL, o["state"][on] == 2), name
            views.append(o)
        worst["share"] = min(worst["share"], share)
        cnt = np.stack([o["counts"] for o in views])
        if kind == "offscreen":
            assert cnt[0, 0] == 0
        if kind == "occluded":
            assert cnt[0, 0] >= N // 2 and cnt[0, 1] == 0
        if kind == "crucial":
            assert crucial_count >= 2 and cnt[0, 1] >= valid_threshold and cnt[0, 2] < crucial_count and cnt[0, 3] == 0
        st = lambda k: np.stack([o[k] for o in views])
        arrays.update({f"{name}.points": points, f"{name}.flags": np.stack([labels, crucial], -1), f"{name}.poses": poses.reshape(V, 16),
                       f"{name}.intrinsics": intrs, f"{name}.depth": depth,
                       f"{name}.meta": np.array([H, W, N, V, n_intr, crucial_count, valid_threshold], dtype=np.int64),
                       # [V,N,10] int32: coords | labels | kept_index | sam_coords | overlay_coords | state | 0;  [V,N,5] float32: cam | uv
                       f"{name}.ints": np.concatenate([st("coords"), st("labels")[..., None], st("kept_index")[..., None], st("sam_coords"),
                                                       st("overlay_coords"), st("state")[..., None], np.zeros((V, N, 1), np.int32)], -1),
                       f"{name}.floats": np.concatenate([st("cam"), st("uv")], -1), f"{name}.counts": cnt})
        print(f"{name}: on screen / kept / crucial / valid per view {cnt.tolist()}, share {share:.3f}")
    assert worst["pixel"] >= M_PIXEL and worst["depth"] >= M_DEPTH and worst["share"] >= 0.9, worst
    assert worst["dev_pixel"] <= M_PIXEL / 10 and worst["dev_depth"] <= M_DEPTH / 10, worst
    valid = np.concatenate([arrays[c[0] + ".counts"][:, 3] for c in PROJECT_CASES])
    assert valid.any() and not valid.all()
    print("projection margins: pixel %.3e depth %.3e, reference deviation: pixel %.3e depth %.3e, share kept %.3f"
          % (worst["pixel"], worst["depth"], worst["dev_pixel"], worst["dev_depth"], worst["share"]))

    # ---- lift (trainer.py:803-809) -------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(77)
    H, W = 5, 7
    ns = dict(torch=torch, H=H, W=W, rays_o=torch.from_numpy(rng.uniform(-1, 1, (H * W, 3)).astype(np.float32)),
              rays_d=torch.from_numpy(rng.uniform(-1, 1, (H * W, 3)).astype(np.float32)),
              pred_depth=torch.from_numpy(rng.uniform(0.5, 4, (H, W)).astype(np.float32)),
              point_coords=np.array([[0, 0], [6, 4], [3, 2], [6, 0], [0, 4], [2, 3]], dtype=np.int64))
    exec(source_lines(ref, 803, 809, "point_depth.unsqueeze"), ns)
    arrays.update({"lift.rays": np.stack([ns["rays_o"].reshape(-1, 3).numpy(), ns["rays_d"].reshape(-1, 3).numpy()]), "lift.depth": ns["pred_depth"].numpy(),
                   "lift.pixels": ns["point_coords"].astype(np.int32), "lift.point_3d": ns["point_3d"].numpy()})

    # ---- store updates (trainer.py:812-834) ---------------------------------------------------------------------------------------
    rng = np.random.default_rng(78)
    base = rng.uniform(-1, 1, (4, 3)).astype(np.float32)
    unit = lambda: (lambda d: d / np.linalg.norm(d))(rng.standard_normal(3))
    u0 = unit()
    clicks = [base[0], base[1], base[2], base[3],                       # into an empty store, three appends
              base[1] + 0.006 * unit(),                                 # removes one of several
              base[0] + 0.012 * u0,                                     # just outside the threshold: appended
              base[2] + 0.004 * unit(), base[3] + 0.008 * unit(),
              base[0] + 0.005 * u0,                                     # removes two: base[0] and its neighbour
              base[1]]                                                  # the store is empty again: entry 0
    clicks += [clicks[-1] + 0.003 * unit()]                             # removes the last one: the store is empty
    click_labels = [1, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1]
    me = types.SimpleNamespace(point_3d=None, input_labels=None)
    margin_store, states = np.inf, []
    for p, lb in zip(clicks, click_labels):
        p = np.asarray(p, dtype=np.float32)
        if me.point_3d is not None:
            d = np.linalg.norm(me.point_3d.numpy().astype(np.float64) - p.astype(np.float64), axis=-1)
            margin_store = min(margin_store, float(np.abs(d - DIST_THRESH).min()))
        ns = dict(torch=torch, self=me, point_3d=torch.from_numpy(p)[None], point_labels=torch.tensor([lb], dtype=torch.int32))
        exec(source_lines(ref, 812, 834, "keep_mask"), ns)
        n = 0 if me.point_3d is None else len(me.point_3d)
        xyz, labels = np.zeros((8, 3), np.float32), np.full(8, -9, np.int32)
        if n:
            xyz[:n], labels[:n] = me.point_3d.numpy(), me.input_labels.numpy()
        states.append((n, xyz, labels))
    counts = [s[0] for s in states]
    assert counts == [1, 2, 3, 4, 3, 4, 3, 2, 0, 1, 0], counts
    assert margin_store >= M_STORE, margin_store
    arrays.update({"store.clicks": np.stack(clicks).astype(np.float32), "store.click_labels": np.array(click_labels, dtype=np.int32),
                   "store.counts": np.array(counts, dtype=np.int32), "store.xyz": np.stack([s[1] for s in states]),
                   "store.labels": np.stack([s[2] for s in states])})
    print(f"store: counts after each click {counts}, margin {margin_store:.3e}")

    # ---- overlays (trainer.py:972-991, utils.py:23-29, 80-98) -----------------------------------------------------------------------
    nan = np.float32("nan")
    #             name   shape  radius  scores              store the float image
    overlays = [("ov_max0", 0, 2, [0.9, 0.5, 0.2], True), ("ov_max1", 1, 3, [0.1, 0.8, 0.3], False), ("ov_max2", 0, 3, [0.2, 0.2, 0.7], False),
                ("ov_nonpos", 1, 2, [0.0, -0.5, -0.1], False), ("ov_nan", 0, 2, [0.3, nan, 0.5], False), ("ov_empty", 1, 2, [0.9, 0.5, 0.2], False)]
    # one image serves both shapes: 37 x 53 and 53 x 37 have the same number of pixels
    rng = np.random.default_rng(900)
    image = make_image(rng, SHAPES[0][0] * SHAPES[0][1])
    margin_rgb8 = min(float(rgb8_distance(v).min()) for v in blends(image))
    assert margin_rgb8 >= M_RGB8
    arrays.update(image=image, masks0=make_masks(rng, 3, *SHAPES[0]), masks1=make_masks(rng, 3, *SHAPES[1]),
                  overlay_cases=np.array([o[0] for o in overlays] + ["ov_points_only"]),
                  margins=np.array([worst["pixel"], worst["depth"], margin_store, margin_rgb8, worst["dev_pixel"], worst["dev_depth"], worst["share"]]))
    for name, s, radius, scores, keep_float in overlays:
        H, W = SHAPES[s]
        scores = np.array(scores, dtype=np.float32)
        want, labels = edge_points(H, W, radius)
        pts = want.copy()
        if name == "ov_empty":
            pts, labels, want = pts[:0], labels[:0], want[:0]
        else:                                                        # the pixels whose round trip through SAM's frame is the wanted position
            r = 1024 / W if W > H else 1024 / H
            trip = lambda c: int(np.int32(np.int32(np.float32(c) * np.float32(r)) / r))
            for i, j in np.ndindex(*want.shape):                       # (the last pixel of the longer axis is no round trip's result: the one before it)
                while not any(trip(c) == want[i, j] for c in range(want[i, j], want[i, j] + 3)):
                    want[i, j] -= 1
                pts[i, j] = next(c for c in range(want[i, j], want[i, j] + 3) if trip(c) == want[i, j])
        rgb, pred_mask, sel, drawn = run_decode_tail(ref, utils, image, arrays[f"masks{s}"], scores, pts, labels, H, W, radius)
        assert np.array_equal(np.asarray(drawn).reshape(-1, 2), want), name
        assert np.array_equal(pred_mask, arrays[f"masks{s}"][sel] if sel >= 0 else np.zeros((H, W), bool))
        arrays.update({f"{name}.meta": np.array([H, W, s, radius, sel], dtype=np.int64), f"{name}.scores": scores,
                       # [n,5] int32: the pixels handed to the tail | the coordinates it draws | labels
                       f"{name}.points": np.concatenate([pts, want, labels[:, None]], -1).astype(np.int32), f"{name}.rgb8": (rgb * 255).astype(np.uint8)})
        if keep_float:
            arrays[f"{name}.rgb"] = rgb
        print(f"{name}: {H}x{W} radius {radius}, selected {sel}, {len(pts)} points, {int((want != pts).sum())} coordinates moved by the round trip")
    # the points alone, as test_step without a decoder draws them (trainer.py:884)
    H, W = SHAPES[1]
    pts, labels = edge_points(H, W, 2)
    rgb = utils.overlay_point(torch.from_numpy(image).reshape(H, W, 3).clone(), pts, inputs_point_labels=labels).numpy()
    arrays.update({"ov_points_only.meta": np.array([H, W, 1, 2, -1], dtype=np.int64),
                   "ov_points_only.points": np.concatenate([pts, pts, labels[:, None]], -1).astype(np.int32), "ov_points_only.rgb8": (rgb * 255).astype(np.uint8)})
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out} ({size} bytes, {len(arrays)} arrays)")
    assert size < 200_000, "the fixture must stay under 200 KB"


if __name__ == "__main__":
    main()
