"""GPU: the point-prompt step -- rm.points_lift, rm.point_store_update, rm.points_project, rm.prompt_overlay and nerf/prompts.py on top of
them -- against tests/golden/point_prompts.npz (the reference's own lines run on the CPU, tools/gen_golden_point_prompts.py) and the float64
restatement of tests/prompts_ref64.py.  Integer outputs, states, counts, tails and 8-bit images are equal; the camera and pixel coordinates
are within prompts_ref64.cam_uv_bound of float64 (the bound the reference's own fp32 values are held to on the CPU); the float image is
within rtol 1e-5 (tests/test_gpu_mask_output.py's)."""
import ctypes

import numpy as np
import pytest
import torch

import prompts_ref64 as R
from helpers import golden
from test_point_prompts_host import INTS, overlay_case, project_case

pytestmark = pytest.mark.gpu

G = golden("point_prompts")
TOL, THRESH, ALPHA = (float(v) for v in G["constants"])


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def packed_column(values, dev, col=3):
    """`values` [n] as column `col` of a NaN-filled [n,5] render buffer: a view whose elements are 5 floats apart."""
    buf = torch.full((values.numel(), 5), float("nan"), device=dev)
    buf[:, col] = values.reshape(-1)
    return buf[:, col]


def check_projection(c, got, name):
    """got: dict of numpy arrays [V,N,...] against the fixture's integers and the float64 statement's floats."""
    worst = 0.0
    for v in range(c["V"]):
        intr = c["intrinsics"][v % c["n_intr"]]
        for k in INTS:
            assert np.array_equal(got["labels" if k == "labels_out" else k][v], c[k][v]), (name, v, k)
        assert np.array_equal(got["counts"][v], c["counts"][v]), (name, v, got["counts"][v], c["counts"][v])
        cam, uv = R.cam_uv(c["points"], c["poses"][v], intr, c["W"])
        e_cam, e_uv = R.cam_uv_bound(c["points"], c["poses"][v], intr, c["W"])
        d_cam, d_uv = np.abs(got["cam"][v] - cam), np.abs(got["uv"][v] - uv)
        worst = max(worst, float((d_cam / e_cam).max()), float((d_uv / e_uv).max()))
        assert (d_cam <= e_cam).all() and (d_uv <= e_uv).all(), (name, v, worst)
    print(f"{name}: cam / uv at most {worst:.3f} of the derived bound")


@pytest.mark.parametrize("name", list(G["project_cases"]))
def test_projection_equals_the_reference_fixture(gpu, name):
    from sanerf_hq_amd import _lib, raymarching as rm
    from sanerf_hq_amd.nerf import PointPrompts
    c = project_case(G, name)
    H, W, N, V = c["H"], c["W"], c["N"], c["V"]
    pts, lb, cr = T(c["points"], gpu), T(c["labels"], gpu), T(c["crucial"], gpu)
    poses, intr, depth = T(c["poses"], gpu), T(c["intrinsics"], gpu), T(c["depth"], gpu)
    # the raw C ABI
    i32 = dict(device=gpu, dtype=torch.int32)
    o = dict(coords=torch.full((V, N, 2), 77, **i32), labels=torch.full((V, N), 77, **i32), kept_index=torch.full((V, N), 77, **i32),
             sam_coords=torch.full((V, N, 2), 77, **i32), overlay_coords=torch.full((V, N, 2), 77, **i32), state=torch.full((V, N), 77, **i32),
             counts=torch.full((V, 4), 77, **i32), cam=torch.full((V, N, 3), 7.0, device=gpu), uv=torch.full((V, N, 2), 7.0, device=gpu))
    rc = _lib.lib().sn_rm_points_project(P(pts), P(lb), P(cr), N, None, P(poses), V, P(intr), c["n_intr"], P(depth), 1, H, W, TOL, c["crucial_count"],
                                         c["valid_threshold"], c["ratio"], P(o["coords"]), P(o["labels"]), P(o["kept_index"]), P(o["sam_coords"]),
                                         P(o["overlay_coords"]), P(o["cam"]), P(o["uv"]), P(o["state"]), P(o["counts"]), _lib.stream())
    assert rc == 0, _lib.lib().sn_last_error()
    raw = {k: v.cpu().numpy() for k, v in o.items()}
    check_projection(c, raw, name + " (C ABI)")
    # the operator; int64 labels and a bool crucial flag are converted on the device
    got = rm.points_project(pts, lb.long(), poses.view(V, 4, 4), intr, depth, H, W, crucial=cr.bool(), crucial_count=c["crucial_count"],
                            valid_threshold=c["valid_threshold"])
    for k, v in raw.items():
        assert np.array_equal(got[k].cpu().numpy(), v, equal_nan=True), (name, k)
    # without the crucial flags and without a ratio: crucial kept 0, no SAM-frame coordinates
    bare = rm.points_project(pts, lb, poses, intr, depth, H, W, valid_threshold=c["valid_threshold"], resize_ratio=0, want=())
    assert "sam_coords" not in bare and "cam" not in bare and torch.equal(bare["coords"], got["coords"])
    cnt = bare["counts"].cpu().numpy()
    assert np.array_equal(cnt[:, :2], c["counts"][:, :2]) and (cnt[:, 2] == 0).all()
    assert np.array_equal(cnt[:, 3], ((cnt[:, 1] > 0) & (cnt[:, 1] >= c["valid_threshold"])).astype(np.int32))
    if V == 1:
        # the depth column of the packed [H*W,5] render buffer, read in place: equal bits
        col = packed_column(depth, gpu)
        assert col.stride(0) == 5
        pk = rm.points_project(pts, lb, poses, intr, col, H, W, crucial=cr, crucial_count=c["crucial_count"], valid_threshold=c["valid_threshold"])
        for k, v in raw.items():
            assert np.array_equal(pk[k].cpu().numpy(), v, equal_nan=True), (name, "packed", k)
        # through nerf/prompts.py: a store of larger capacity, the count on the device
        pp = PointPrompts(gpu, capacity=N + 7).from_json({"points": c["points"].tolist(), "negative_labels": np.flatnonzero(c["labels"] == 0).tolist(),
                                                          "crucial_point_index": np.flatnonzero(c["crucial"]).tolist(), "valid_threshold": c["valid_threshold"]})
        pp.crucial_count = c["crucial_count"]
        res = pp.project(poses.view(1, 4, 4), intr, depth, H, W, want=("cam", "uv", "state"))
        for k, v in raw.items():
            g_ = res[k].cpu().numpy()
            if k != "counts":
                assert np.array_equal(g_[:, :N], v, equal_nan=True), (name, "store", k)
                assert (g_[:, N:] == (-1 if k in ("labels", "kept_index") else 0)).all(), (name, "store tail", k)
            else:
                assert np.array_equal(g_, v)


def test_device_count_smaller_than_n_and_rejections(gpu):
    """n_points < N: the points behind it are no points.  A point at the camera centre (z = 0: non-finite pixel coordinates) and a NaN depth
    pixel are rejected, and the other points' outputs do not change."""
    from sanerf_hq_amd import raymarching as rm
    c = project_case(G, "p37x53_n130_v1")
    H, W, N = c["H"], c["W"], c["N"]
    pts, lb, cr = T(c["points"], gpu), T(c["labels"], gpu), T(c["crucial"], gpu)
    poses, intr, depth = T(c["poses"], gpu), T(c["intrinsics"], gpu), T(c["depth"], gpu)
    kw = dict(crucial=cr, crucial_count=c["crucial_count"], valid_threshold=c["valid_threshold"])
    for n in (0, 1, 64, 70):
        got = rm.points_project(pts, lb, poses, intr, depth, H, W, n_points=torch.tensor([n], device=gpu, dtype=torch.int32), **kw)
        want = R.project_view(c["points"], c["labels"], c["crucial"], n, c["poses"][0], c["intrinsics"][0], c["depth"][0], H, W, TOL,
                              c["crucial_count"], c["valid_threshold"], c["ratio"])
        for k in ("coords", "labels", "kept_index", "sam_coords", "overlay_coords", "state", "counts"):
            assert np.array_equal(got[k].cpu().numpy()[0], want[k]), (n, k)
    base = rm.points_project(pts, lb, poses, intr, depth, H, W, **kw)
    kept = base["kept_index"][0, :int(base["counts"][0, 1])].cpu().numpy()
    a, b = int(kept[3]), int(kept[len(kept) // 2])
    pts2, depth2 = pts.clone(), depth.clone()
    pts2[a] = poses.view(4, 4)[:3, 3]                                   # the camera centre
    xb, yb = base["coords"][0, len(kept) // 2].cpu().tolist()
    depth2[0, yb, xb] = float("nan")
    got = rm.points_project(pts2, lb, poses, intr, depth2, H, W, **kw)
    st = got["state"][0].cpu().numpy()
    assert st[a] == 0 and st[b] == 1 and not np.isfinite(got["uv"][0, a].cpu().numpy()).all()
    rest = np.setdiff1d(np.arange(N), [a, b])
    assert np.array_equal(st[rest], base["state"][0].cpu().numpy()[rest])
    assert np.array_equal(got["kept_index"][0].cpu().numpy()[:len(kept) - 2], np.setdiff1d(kept, [a, b]))
    assert int(got["counts"][0, 1]) == len(kept) - 2 and int(got["counts"][0, 0]) == int(base["counts"][0, 0]) - 1
    assert torch.equal(got["uv"][0][rest], base["uv"][0][rest]) and (got["labels"][0, len(kept) - 2:] == -1).all()


def test_lift_and_store_equal_the_reference_fixture(gpu):
    from sanerf_hq_amd import raymarching as rm
    H, W = G["lift.depth"].shape
    ro, rd, depth = T(G["lift.rays"][0], gpu), T(G["lift.rays"][1], gpu), T(G["lift.depth"], gpu)
    px = T(G["lift.pixels"], gpu)
    got = rm.points_lift(px, ro, rd, depth, H, W)
    assert np.array_equal(got.cpu().numpy(), G["lift.point_3d"]), "fl(o + fl(d * depth)) is the reference's value bit for bit"
    assert torch.equal(rm.points_lift(px.long(), ro, rd, packed_column(depth, gpu), H, W), got)
    out = rm.points_lift(torch.tensor([[W, 0], [0, H], [-1, 2], [3, -1], [W - 1, H - 1]], device=gpu, dtype=torch.int32), ro, rd, depth, H, W)
    assert torch.isnan(out[:4]).all() and torch.isfinite(out[4]).all()
    # the store, click by click
    cap = 8
    store = rm.point_store(gpu, cap)
    ref = (np.zeros((cap, 3), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), 0)
    for i, (p, lb) in enumerate(zip(G["store.clicks"], G["store.click_labels"])):
        rm.point_store_update(store, T(p, gpu), int(lb) if i % 2 else torch.tensor([lb], device=gpu), THRESH)
        ref = R.store_update(*ref, cap, p, lb, THRESH)[:5]
        n, status = int(store["count"]), ref[4]
        ref = ref[:4]
        assert n == G["store.counts"][i] == ref[3], i
        assert np.array_equal(store["xyz"][:n].cpu().numpy(), G["store.xyz"][i][:n]) and np.array_equal(store["labels"][:n].cpu().numpy(), G["store.labels"][i][:n]), i
        assert store["status"].cpu().tolist() == list(status), (i, store["status"].cpu().tolist(), status)
    # the crucial flags travel with their points (the extension), and a full store changes nothing but the overflow word
    store = rm.point_store(gpu, 4)
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    for p in base:
        rm.point_store_update(store, T(p, gpu), 1)
    store["crucial"].copy_(torch.tensor([1, 0, 1, 1], dtype=torch.int32))
    before = {k: v.clone() for k, v in store.items()}
    rm.point_store_update(store, T(np.array([5, 5, 5], np.float32), gpu), 0)
    assert store["status"].cpu().tolist() == [3, 4, 4, 1]
    assert all(torch.equal(store[k], before[k]) for k in ("xyz", "labels", "crucial", "count"))
    rm.point_store_update(store, T(base[1] + np.float32(0.002), gpu), 0)
    assert store["status"].cpu().tolist() == [2, 4, 3, 1], "the overflow word is only ever set"
    assert store["crucial"][:3].cpu().tolist() == [1, 1, 1] and np.array_equal(store["xyz"][:3].cpu().numpy(), base[[0, 2, 3]])
    # more than one wave of stored points: remove one from each of three waves
    big = rm.point_store(gpu, 200)
    xyz = np.stack([np.arange(150), np.zeros(150), np.zeros(150)], -1).astype(np.float32)
    xyz[[5, 70, 140]] = (500, 0, 0)
    big["xyz"][:150].copy_(T(xyz, gpu)); big["labels"][:150].copy_(torch.arange(150, dtype=torch.int32)); big["count"].fill_(150)
    rm.point_store_update(big, T(np.array([500, 0, 0.001], np.float32), gpu), 1)
    keep = np.setdiff1d(np.arange(150), [5, 70, 140])
    assert big["status"].cpu().tolist() == [2, 150, 147, 0] and big["labels"][:147].cpu().tolist() == keep.tolist()
    assert np.array_equal(big["xyz"][:147].cpu().numpy(), xyz[keep])


def close(got, want, what, rtol=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rel = np.where(got == want, 0.0, np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    print(f"{what}: max rel diff {rel.max():.3e} (bar {rtol:.0e})")
    assert (rel <= rtol).all(), (what, float(rel.max()))


@pytest.mark.parametrize("name", list(G["overlay_cases"]))
def test_overlay_equals_the_reference_fixture(gpu, name):
    from sanerf_hq_amd import _lib, raymarching as rm
    c = overlay_case(G, name)
    H, W, n = c["H"], c["W"], len(c["coords"])
    img = T(c["image"], gpu)
    masks = None if c["masks"] is None else T(c["masks"], gpu)
    scores = None if c["scores"] is None else T(c["scores"], gpu)
    xy, lb = T(c["coords"].reshape(-1, 2), gpu), T(c["labels"], gpu)
    rgb64, rgb32, pred, sel = R.overlay(c["image"], H, W, c["coords"], c["labels"], n, c["radius"], ALPHA, c["masks"], c["scores"])
    # the raw C ABI
    rgb, rgb8 = torch.full((H, W, 3), 7.0, device=gpu), torch.full((H, W, 3), 7, device=gpu, dtype=torch.uint8)
    pm, selected = torch.full((H, W), 7, device=gpu, dtype=torch.uint8), torch.full((1,), 7, device=gpu, dtype=torch.int32)
    cnt = torch.tensor([n], device=gpu, dtype=torch.int32)
    m8 = None if masks is None else masks.view(torch.uint8)
    rc = _lib.lib().sn_rm_prompt_overlay(P(img), 3, H, W, P(m8), 0 if m8 is None else 3, P(scores), 0, P(xy) if n else None, P(lb) if n else None, n, P(cnt),
                                         c["radius"], ALPHA, P(rgb), P(rgb8), P(pm), P(selected), _lib.stream())
    assert rc == 0, _lib.lib().sn_last_error()
    assert int(selected) == c["selected"] == sel
    got8 = rgb8.cpu().numpy()
    print(f"{name} rgb8: {(got8 != c['rgb8']).sum()} of {got8.size} bytes differ")
    assert np.array_equal(got8, c["rgb8"])
    close(rgb.cpu().numpy(), rgb64, name + " rgb")
    print(f"{name} rgb: {(rgb.cpu().numpy() != rgb32).sum()} values differ from the fp32 chain")
    if c["rgb"] is not None:
        close(rgb.cpu().numpy(), c["rgb"], name + " rgb (reference)")
    assert np.array_equal(pm.cpu().numpy().astype(bool), pred)
    # the operator: the image columns of the packed render buffer read in place, more points than the device count says
    buf = torch.full((H * W, 5), float("nan"), device=gpu)
    buf[:, :3] = img
    extra = torch.tensor([[W // 2, H // 2]] * 3, device=gpu, dtype=torch.int32)
    o = rm.prompt_overlay(buf[:, :3], torch.cat([xy, extra]), torch.cat([lb, torch.zeros(3, device=gpu, dtype=torch.int32)]), H, W, count=cnt, masks=masks,
                          scores=scores, radius=c["radius"], alpha=ALPHA, want=("rgb", "rgb8", "pred_mask"))
    assert torch.equal(o["rgb"], rgb) and torch.equal(o["rgb8"], rgb8) and torch.equal(o["pred_mask"].view(torch.uint8), pm) and int(o["selected"]) == sel
    if masks is not None and n:
        # a fixed mask index instead of scores
        o = rm.prompt_overlay(img, xy, lb, H, W, masks=masks, mask_index=1, radius=c["radius"], alpha=ALPHA, want=("rgb8", "pred_mask"))
        want = R.overlay(c["image"], H, W, c["coords"], c["labels"], n, c["radius"], ALPHA, c["masks"], None, 1)
        assert np.array_equal(o["rgb8"].cpu().numpy(), R.rgb8(want[0])) and np.array_equal(o["pred_mask"].cpu().numpy(), want[2]) and int(o["selected"]) == 1


@pytest.mark.parametrize("H,W,radius", [(37, 53, 2), (53, 37, 3)])
def test_overlay_edge_points_against_the_restatement(gpu, H, W, radius):
    """Every combination of x, y in {0, 1, r, W-1, H-1} -- the last pixel of the longer axis is no round trip's result, so the fixture's tail
    cannot draw it -- one point at a time and all together, against numpy's slices."""
    from sanerf_hq_amd import raymarching as rm
    img = G["image"]
    xs, ys = [0, 1, radius, W - 1], [0, 1, radius, H - 1]
    pts = np.array([(x, y) for x in xs for y in ys] + [(W - 2, H - 2), (W - 1, H - 1)], dtype=np.int32)
    labels = (np.arange(len(pts)) % 3 != 0).astype(np.int32)
    masks = G["masks0" if (H, W) == (37, 53) else "masks1"]
    d_img, d_masks = T(img, gpu), T(masks, gpu)
    for sub in [slice(i, i + 1) for i in range(len(pts))] + [slice(0, len(pts))]:
        o = rm.prompt_overlay(d_img, T(pts[sub], gpu), T(labels[sub], gpu), H, W, masks=d_masks, mask_index=2, radius=radius, alpha=ALPHA, want=("rgb", "rgb8"))
        want = R.overlay(img, H, W, pts[sub], labels[sub], len(pts[sub]), radius, ALPHA, masks, None, 2)
        assert np.array_equal(o["rgb8"].cpu().numpy(), R.rgb8(want[0])), (sub, pts[sub])
        assert np.array_equal(o["rgb"].cpu().numpy(), want[1]), (sub, pts[sub])


def test_click_project_overlay_replays_as_one_graph(gpu):
    """PointPrompts.click -> decode_prompts -> decode_overlay on the packed render buffer, captured once with torch.cuda.graph (one stream, no
    parallel branch), replayed after the clicked pixel, the pose, the depth and the image were rewritten in place: every replay equals the eager
    run on the same inputs and the same store bit for bit."""
    from sanerf_hq_amd.nerf import PointPrompts, decode_overlay, decode_prompts
    c = project_case(G, "p37x53_n64_v1")
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(3)
    packed = torch.zeros(H * W, 5, device=gpu)
    ro, rd = T(rng.uniform(-1, 1, (H * W, 3)).astype(np.float32), gpu), T(rng.uniform(-1, 1, (H * W, 3)).astype(np.float32), gpu)
    pose, intr = torch.zeros(1, 4, 4, device=gpu), T(c["intrinsics"][:1], gpu)
    pixel = torch.zeros(1, 2, device=gpu, dtype=torch.int32)
    masks, scores = T(G["masks0"], gpu), T(np.array([0.2, 0.9, 0.4], np.float32), gpu)
    pp = PointPrompts(gpu, capacity=96).from_json({"points": c["points"].tolist(), "negative_labels": np.flatnonzero(c["labels"] == 0).tolist(),
                                                   "crucial_point_index": [], "valid_threshold": 4})
    start = {k: v.clone() for k, v in pp.store.items()}

    def set_inputs(i):
        """View 0 is the fixture's; view i hides every third kept point from the i-th on and moves the camera by 2 i mm."""
        depth_i, pose_i = c["depth"][0].copy(), c["poses"][0].reshape(4, 4).copy()
        if i:
            hide = c["coords"][0][:int(c["counts"][0, 1])][i::3]
            depth_i[hide[:, 1], hide[:, 0]] = 7.5
            pose_i[:3, 3] += np.float32(0.002 * i)
        packed[:, :3] = T(np.roll(G["image"], 17 * i, axis=0), gpu)
        packed[:, 3] = T(depth_i.reshape(-1), gpu)
        pose.copy_(T(pose_i.reshape(1, 4, 4), gpu))
        pixel.copy_(torch.tensor([[5 + 11 * i, 7 + 9 * i]], dtype=torch.int32))
        for k, v in start.items():
            pp.store[k].copy_(v)

    def chain():
        pp.click(ro, rd, packed[:, 3], pixel, 1, H, W)
        proj = decode_prompts({"depth": packed[:, 3]}, {"poses": pose, "intrinsics": intr, "H": H, "W": W}, pp)
        out = decode_overlay({"image": packed[:, :3]}, masks, scores, proj, rgb8=True)
        return {**{k: proj[k] for k in ("coords", "labels", "kept_index", "sam_coords", "overlay_coords", "state", "counts")}, **out}

    def snapshot(o):
        return {**{k: v.clone() for k, v in o.items()}, **{"store." + k: v.clone() for k, v in pp.store.items()}}

    set_inputs(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                         # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = chain()
    replays = []
    for i in range(3):
        set_inputs(i)
        graph.replay()
        replays.append(snapshot(held))
    torch.cuda.synchronize()
    for i in range(3):
        set_inputs(i)
        eager = snapshot(chain())
        for k, v in eager.items():
            assert torch.equal(v, replays[i][k]), (i, k)
        assert int(eager["store.count"]) == c["N"] + 1 and eager["store.status"].cpu().tolist() == [1, 64, 65, 0]
    # the first view is the fixture's: the 64 stored points project as recorded, the clicked one comes behind them
    n_kept = int(c["counts"][0, 1])
    k0 = replays[0]["kept_index"][0].cpu().numpy()
    assert np.array_equal(k0[:n_kept], c["kept_index"][0][:n_kept]) and np.array_equal(replays[0]["coords"][0, :n_kept].cpu().numpy(), c["coords"][0][:n_kept])
    assert int(replays[0]["selected"]) == 1 and replays[0]["pred_masks"].shape == (1, H, W) and replays[0]["rgb8"].dtype == torch.uint8
    kept = [int(r["counts"][0, 1]) for r in replays]
    assert kept[0] >= n_kept and 0 < kept[1] < kept[0] and 0 < kept[2] < kept[0], kept
    assert not torch.equal(replays[0]["pred_rgb"], replays[1]["pred_rgb"]) and not torch.equal(replays[1]["coords"], replays[2]["coords"])
