"""GPU: the mesh rasteriser -- sn_rm_mesh_raster_project / _draw / _resolve against the numpy restatement in tests/mesh_raster_ref.py:
triangle_id, depth, mask, label, image and normal bit for bit and the counts exactly, through both draw kernels (small_max_pixels = 0, the
default, 2^31 - 1); independence of the triangle order and of the run; sentinel margins; the empty cases; an extracted sphere with cull; the
three phases as one captured graph replayed with a new pose; NeRFRenderer.render_mesh."""
import functools

import numpy as np
import pytest
import torch

import mesh_raster_ref as ref
import mesh_ref as mr
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

SMALL = (0, None, (1 << 31) - 1)
IMAGES = ("triangle_id", "depth", "mask", "image", "normal", "label")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _attributes(V, seed=5):
    rng = np.random.default_rng(seed)
    return dict(colors=rng.random((V, 3), dtype=np.float32), normals=rng.standard_normal((V, 3)).astype(np.float32),
                labels=rng.integers(0, 7, V).astype(np.uint8))


def _device(case, gpu, small=None, **kw):
    from sanerf_hq_amd import raymarching as rm
    V = len(case["vertices"])
    attr = {k: torch.from_numpy(v).to(gpu) for k, v in _attributes(V).items()}
    mesh = {"vertices": torch.from_numpy(np.ascontiguousarray(case["vertices"], dtype=np.float32)).reshape(-1, 3).to(gpu),
            "triangles": torch.from_numpy(np.ascontiguousarray(case["triangles"], dtype=np.int32)).reshape(-1, 3).to(gpu)}
    args = dict(near=case.get("near", 0.05), cull=case.get("cull", False), bg_color=0.75, small_max_pixels=small, **attr)
    args.update(kw)
    return rm.mesh_rasterize(mesh, torch.from_numpy(np.asarray(case["pose"], dtype=np.float32)).to(gpu),
                             torch.tensor(np.asarray(case["intrinsics"], dtype=np.float32)).to(gpu), case["H"], case["W"], **args)


def _restated(case, **kw):
    args = dict(near=case.get("near", 0.05), cull=case.get("cull", False), bg_color=0.75, **_attributes(len(case["vertices"])))
    args.update(kw)
    return ref.rasterize(case["vertices"], case["triangles"], case["pose"], case["intrinsics"], case["H"], case["W"], **args)


def _assert_equal(out, want, what=""):
    assert out["counts"].dtype == torch.int32 and _np(out["counts"]).tolist() == want["counts"].tolist(), what
    for k in IMAGES:
        got = _np(out[k])
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k)
        assert np.array_equal(_bits(got), _bits(want[k])), (what, k, int((_bits(got) != _bits(want[k])).sum()))


def _check_all_thresholds(case, gpu, want, what):
    """The device at the three thresholds: each equal to the restatement, hence to one another."""
    for small in SMALL:
        _assert_equal(_device(case, gpu, small), want, f"{what}, small_max_pixels={small}")


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
def _world(pose, intr, xy, z):
    """World points (fp32) that the camera puts near the pixel coordinates xy at depth z."""
    fx, fy, cx, cy = (float(a) for a in intr)
    cam = np.stack([(xy[..., 0] - cx) * z / fx, -(xy[..., 1] - cy) * z / fy, -z], axis=-1)
    m = np.asarray(pose, dtype=np.float64)
    return (cam @ m[:3, :3].T + m[:3, 3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _prefix_case():
    v, t = ref.icosphere(2, 1.0)             # 320 triangles
    return dict(vertices=v.astype(np.float32), triangles=t, pose=ref.look_at([1.1, 0.7, 2.4]), intrinsics=[55.0, 55.0, 26.5, 18.5], H=37, W=53)


@functools.lru_cache(maxsize=None)
def _soup_case():
    rng = np.random.default_rng(11)
    T, H, W = 2000, 48, 64
    pose, intr = ref.look_at([0.4, -1.2, 2.0], target=(0.1, 0.0, -0.3)), [70.0, 64.0, 31.25, 24.5]
    centre = rng.uniform([-8, -8], [W + 8, H + 8], (T, 1, 2))
    size = np.exp(rng.uniform(np.log(0.05), np.log(30.0), (T, 1, 1)))
    xy = centre + rng.standard_normal((T, 3, 2)) * size
    z = rng.uniform(0.5, 4.0, (T, 1)) * np.exp(rng.normal(0.0, 0.2, (T, 3)))
    v = _world(pose, intr, xy, z).reshape(-1, 3)
    tri = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    flip = rng.random(T) < 0.5
    tri[flip] = tri[flip][:, ::-1]
    share = rng.choice(T, 300, replace=False)                   # shared corners: triangles that reach across the screen
    tri[share, 2] = rng.integers(0, 3 * T, 300)
    # corners that are not placed: behind the camera, nearer than near, outside the guard band, NaN, +-Inf
    bad = rng.choice(3 * T, 150, replace=False)
    v[bad[:30]] = _world(pose, intr, rng.uniform(0, 40, (30, 2)), -rng.uniform(0.5, 2.0, 30))
    v[bad[30:60]] = _world(pose, intr, rng.uniform(0, 40, (30, 2)), rng.uniform(0.001, 0.04, 30))
    v[bad[60:90]] = _world(pose, intr, rng.uniform(17000, 90000, (30, 2)) * rng.choice([-1, 1], (30, 2)), rng.uniform(0.5, 2.0, 30))
    v[bad[90:110], rng.integers(0, 3, 20)] = np.nan
    v[bad[110:130], rng.integers(0, 3, 20)] = np.inf
    v[bad[130:150], rng.integers(0, 3, 20)] = -np.inf
    # rows that are not triangles: repeated corners, indices outside [0, V)
    rows = rng.choice(T, 90, replace=False)
    tri[rows[:30], 1] = tri[rows[:30], 0]
    tri[rows[30:50]] = tri[rows[30:50], :1]
    tri[rows[50:60], 0] = 3 * T
    tri[rows[60:70], 1] = -1
    tri[rows[70:80], 2] = (1 << 31) - 1
    tri[rows[80:90], 0] = -(1 << 31)
    return dict(vertices=v, triangles=tri, pose=pose, intrinsics=intr, H=H, W=W)


@functools.lru_cache(maxsize=None)
def _fullscreen_case():
    """One triangle over all of 96 x 80 at depth 2 and 500 sub-pixel ones at depth 1 and 4, every corner on the 1/256 grid of a camera
    that reproduces it exactly: corners and edges through pixel centres happen."""
    rng = np.random.default_rng(3)
    pose, intr = ref.screen_camera()
    H, W, n = 80, 96, 500
    centre = rng.integers(0, [W * 4, H * 4], (n, 1, 2)) / 4.0 + 0.5 * rng.integers(0, 2, (n, 1, 1))
    xy = centre + rng.integers(-160, 161, (n, 3, 2)) / 256.0
    z = np.repeat(np.where(np.arange(n) % 2 == 0, 1.0, 4.0), 3)
    v = np.concatenate([ref.screen_vertices([(-10.0, -10.0), (300.0, -10.0), (-10.0, 300.0)], 2.0), ref.screen_vertices(xy.reshape(-1, 2), z)])
    tri = np.concatenate([np.array([[0, 1, 2]]), 3 + np.arange(3 * n).reshape(n, 3)]).astype(np.int32)
    order = rng.permutation(n + 1)                              # the large one somewhere in the middle
    return dict(vertices=v, triangles=tri[order], pose=pose, intrinsics=intr, H=H, W=W, large=int(np.nonzero(order == 0)[0][0]))


@functools.lru_cache(maxsize=None)
def _want(name):
    case = {"soup": _soup_case, "fullscreen": _fullscreen_case, "prefix": _prefix_case}[name]()
    return case, _restated(case)


# ---- against the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_worked_cases(gpu, name):
    case = ref.hand_cases()[name]
    want = _restated(case)
    if case["pixels"] is not None:
        jj, ii = np.nonzero(want["mask"])
        assert {(int(i), int(j)) for i, j in zip(ii, jj)} == case["pixels"]
    _check_all_thresholds(case, gpu, want, name)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_triangle_counts_around_the_wave(gpu, T):
    case = dict(_prefix_case())
    case["triangles"] = case["triangles"][:T]
    for cull in (False, True):
        c = dict(case, cull=cull)
        want = _restated(c)
        assert want["counts"].sum() == T and (cull or want["mask"].any())        # (the first triangle looks away)
        _check_all_thresholds(c, gpu, want, f"first {T} triangles, cull={cull}")


def test_triangle_soup(gpu):
    case, want = _want("soup")
    counts = want["counts"].tolist()
    print("soup counts (drawn, dropped, degenerate, culled):", counts, "covered:", int(want["mask"].sum()))
    assert counts[0] > 1500 and counts[1] > 150 and counts[2] >= 50 and sum(counts) == 2000
    _check_all_thresholds(case, gpu, want, "soup")
    culled = dict(case, cull=True)
    want_culled = _restated(culled)
    assert want_culled["counts"][3] > 500
    _check_all_thresholds(culled, gpu, want_culled, "soup, cull")


def test_fullscreen_triangle_among_subpixel_ones(gpu):
    case, want = _want("fullscreen")
    assert want["mask"].all() and want["counts"].tolist()[0] + want["counts"].tolist()[2] == 501
    ids = want["triangle_id"]
    front = (ids != case["large"]).sum()
    print("pixels won by a sub-pixel triangle in front:", int(front))
    assert 20 < front < 500 and (want["depth"][ids != case["large"]] == 1.0).all() and (want["depth"][ids == case["large"]] == 2.0).all()
    _check_all_thresholds(case, gpu, want, "fullscreen")


def test_order_and_run_do_not_matter(gpu):
    case, want = _want("soup")
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(case["triangles"]))
    for small in SMALL:
        a = _device(case, gpu, small)
        b = _device(case, gpu, small)
        for k in IMAGES + ("counts",):
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
        p = _device(dict(case, triangles=case["triangles"][perm]), gpu, small)
        assert np.array_equal(_bits(_np(p["depth"])), _bits(want["depth"])) and np.array_equal(_np(p["mask"]), want["mask"])
        assert _np(p["counts"]).tolist() == want["counts"].tolist()
        # the same triangle wherever the winning depth is unique: map the permuted ids back
        ids = _np(p["triangle_id"])
        back = np.where(ids >= 0, perm[np.maximum(ids, 0)], -1)
        same = back == want["triangle_id"]
        unique = _unique_winner(case, want)
        assert same[unique].all() and unique.sum() > 0.9 * (want["mask"] == 1).sum()


def _unique_winner(case, want):
    """Pixels whose winning depth bits exactly one drawn triangle has."""
    return ref.rasterize(case["vertices"], case["triangles"], case["pose"], case["intrinsics"], case["H"], case["W"], want_coverage=True)["ties"] == 1


def test_sentinel_margins(gpu):
    from sanerf_hq_amd import raymarching as rm
    case, want = _want("prefix")
    H, W, V = case["H"], case["W"], len(case["vertices"])
    attr = {k: torch.from_numpy(v).to(gpu) for k, v in _attributes(V).items()}
    vertices, tri = torch.from_numpy(case["vertices"]).to(gpu), torch.from_numpy(case["triangles"]).to(gpu)
    pose, intr = torch.from_numpy(case["pose"]).to(gpu), torch.tensor(case["intrinsics"], device=gpu)
    margin = 67
    spec = {"triangle_id": (torch.int32, 1, -77), "depth": (torch.float32, 1, -5.0), "mask": (torch.uint8, 1, 99), "image": (torch.float32, 3, -5.0),
            "normal": (torch.float32, 3, -5.0), "label": (torch.uint8, 1, 99), "counts": (torch.int32, None, -77)}
    raw, view = {}, {}
    for k, (dtype, ch, fill) in spec.items():
        n = 4 if ch is None else H * W * ch
        raw[k] = torch.full((n + 2 * margin * 4,), fill, device=gpu, dtype=dtype)
        inner = raw[k][margin * 4:margin * 4 + n]
        view[k] = inner if ch is None else inner.view((H, W) if ch == 1 else (H, W, ch))
    ws = rm.mesh_raster_project(vertices, tri.shape[0], pose, intr, H, W, 0.05, view["counts"])
    rm.mesh_raster_draw(tri, V, H, W, ws, view["counts"])
    rm.mesh_raster_resolve(tri, V, H, W, ws, view["triangle_id"], view["depth"], view["mask"], attr["colors"], view["image"], attr["normals"],
                           view["normal"], attr["labels"], view["label"], 0.75)
    _assert_equal(view, want, "phase functions")
    for k, (dtype, ch, fill) in spec.items():
        n = 4 if ch is None else H * W * ch
        assert (raw[k][:margin * 4] == fill).all() and (raw[k][margin * 4 + n:] == fill).all(), k


def test_empty_meshes(gpu):
    from sanerf_hq_amd import raymarching as rm
    pose, intr = torch.eye(4, device=gpu), torch.tensor([10.0, 10.0, 4.0, 3.0], device=gpu)
    tri = torch.tensor([[0, 1, 2]], device=gpu, dtype=torch.int32)
    for v, t, counts in ((torch.zeros(0, 3, device=gpu), tri[:0], [0, 0, 0, 0]), (torch.zeros(0, 3, device=gpu), tri, [0, 1, 0, 0]),
                         (torch.rand(5, 3, device=gpu), tri[:0], [0, 0, 0, 0])):
        V = v.shape[0]
        out = rm.mesh_rasterize({"vertices": v, "triangles": t}, pose, intr, 6, 8, colors=torch.rand(V, 3, device=gpu),
                                labels=torch.zeros(V, device=gpu, dtype=torch.uint8), normals=torch.rand(V, 3, device=gpu), bg_color=0.5)
        assert out["counts"].tolist() == counts
        assert (out["triangle_id"] == -1).all() and (out["depth"] == 0).all() and (out["mask"] == 0).all()
        assert (out["image"] == 0.5).all() and (out["normal"] == 0).all() and (out["label"] == 255).all()
        assert tuple(out["image"].shape) == (6, 8, 3) and tuple(out["label"].shape) == (6, 8)
    plain = rm.mesh_rasterize({"vertices": torch.rand(5, 3, device=gpu), "triangles": tri}, pose, intr, 6, 8)
    assert sorted(plain) == ["counts", "depth", "mask", "triangle_id"]                 # no attribute, no image of it


def test_extracted_sphere_with_cull(gpu):
    """The orientation: isosurface() promises counter-clockwise seen from outside, and cull keeps what faces the camera."""
    from sanerf_hq_amd import raymarching as rm
    n, radius, distance, H, W = 32, 10.0, 3.0, 72, 80
    step = 2.0 / (n - 1)
    vol = torch.from_numpy(mr.sphere_volume(n, (n - 1) / 2.0, radius)).to(gpu)
    mesh = rm.isosurface(vol, 0.0, origin=(-1.0, -1.0, -1.0), step=(step,) * 3)
    intr = [150.0, 150.0, 40.25, 35.5]
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = distance
    v, t = _np(mesh["vertices"]), _np(mesh["triangles"])
    r_hi, r_in = ref.facet_inner_radius(v, t)
    assert abs(r_hi - radius * step) < 0.01 and r_hi - r_in < 0.02
    case = dict(vertices=v, triangles=t, pose=pose, intrinsics=intr, H=H, W=W)
    culled = _device(case, gpu, cull=True)
    both = _device(case, gpu, cull=False)
    counts = culled["counts"].tolist()
    print("sphere counts with cull:", counts, "r_hi, r_in:", r_hi, r_in)
    assert counts[0] > 0.3 * len(t) and counts[3] > 0.3 * len(t) and counts[1] == 0 and sum(counts) == len(t)
    for k in IMAGES:
        assert torch.equal(culled[k], both[k]), k               # culling the back of a closed surface changes nothing that is seen
    _assert_equal(culled, _restated(dict(case, cull=True)), "sphere")
    ref.check_sphere_image({k: _np(culled[k]) for k in ("mask", "depth")}, H, W, intr, distance, r_hi, r_in)
    # seen with the orientation reversed, the front is gone: every pixel shows the far side
    rev = _device(dict(case, triangles=np.ascontiguousarray(t[:, ::-1])), gpu, cull=True)
    seen = culled["mask"] == 1
    assert torch.equal(rev["mask"], culled["mask"]) and (rev["depth"][seen] > culled["depth"][seen]).all()


def test_one_graph_replayed_with_a_new_pose(gpu):
    from sanerf_hq_amd import raymarching as rm
    case, _ = _want("prefix")
    V = len(case["vertices"])
    attr = {k: torch.from_numpy(v).to(gpu) for k, v in _attributes(V).items()}
    mesh = {"vertices": torch.from_numpy(case["vertices"]).to(gpu), "triangles": torch.from_numpy(case["triangles"]).to(gpu)}
    pose, intr = torch.from_numpy(case["pose"]).to(gpu), torch.tensor(case["intrinsics"], device=gpu)
    H, W = case["H"], case["W"]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        rm.mesh_rasterize(mesh, pose, intr, H, W, bg_color=0.75, **attr)               # warm-up: the scratch buffer exists
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = rm.mesh_rasterize(mesh, pose, intr, H, W, bg_color=0.75, **attr)
    for eye in ([1.1, 0.7, 2.4], [-0.9, 1.6, 1.9], [0.2, -2.5, 0.8]):
        new = ref.look_at(eye)
        pose.copy_(torch.from_numpy(new).to(gpu))
        graph.replay()
        torch.cuda.synchronize()
        eager = rm.mesh_rasterize(mesh, pose, intr, H, W, bg_color=0.75, **attr)
        for k in IMAGES + ("counts",):
            assert torch.equal(out[k], eager[k]), (eye, k)
        _assert_equal(out, _restated(dict(case, pose=new)), f"replayed, eye {eye}")


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_mesh_smooth.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


def test_extract_mesh_through_render_mesh(gpu, model):
    res, H, W = 24, 40, 56
    pose = torch.from_numpy(ref.look_at([0.6, 0.9, 2.8])).to(gpu)
    intr = torch.tensor([60.0, 60.0, W / 2, H / 2], device=gpu)
    with torch.no_grad():
        thr = float(model.density_volume(res).median())
        mesh = model.extract_mesh(res, threshold=thr, vertex_colors=True, vertex_labels=True)
        out = model.render_mesh(mesh, pose, intr, H, W, bg_color=0)
    T = mesh["triangles"].shape[0]
    assert sorted(out) == ["counts", "depth", "image", "label", "mask", "triangle_id"]
    want_types = {"triangle_id": (torch.int32, (H, W)), "depth": (torch.float32, (H, W)), "mask": (torch.uint8, (H, W)), "image": (torch.float32, (H, W, 3)),
                  "label": (torch.uint8, (H, W)), "counts": (torch.int32, (4,))}
    for k, (dtype, shape) in want_types.items():
        assert out[k].dtype == dtype and tuple(out[k].shape) == shape, k
    assert int(out["counts"].sum()) == T and int(out["counts"][0]) > 0 and out["mask"].any()
    seen = out["mask"] == 1
    assert (out["triangle_id"][seen] >= 0).all() and (out["triangle_id"][seen] < T).all() and (out["depth"][seen] >= model.min_near).all()
    assert (out["image"][~seen] == 0).all() and (out["label"][~seen] == 255).all()
    want = ref.rasterize(_np(mesh["vertices"]), _np(mesh["triangles"]), _np(pose), _np(intr), H, W, near=model.min_near, colors=_np(mesh["colors"]),
                         labels=_np(mesh["labels"]), bg_color=0.0)
    for k in ("triangle_id", "depth", "mask", "image", "label"):
        assert np.array_equal(_bits(_np(out[k])), _bits(want[k])), k
    with pytest.raises(RuntimeError, match="inference query"):                  # grad mode with parameters that require it
        model.render_mesh(mesh, pose, intr, H, W)
