"""GPU: the rasteriser's near-plane clipping -- sn_rm_mesh_raster_draw_clip / _resolve_clip against the numpy restatement in
tests/mesh_raster_clip_ref.py: triangle_id, depth, mask, image, normal, label bit for bit, counts and clip_counts exactly, through both draw
kernels (small_max_pixels = 0, the default, 2^30), cull off and on, all three attributes at once; clip on a mesh that nothing cuts equals
the unclipped entries; two runs; the three phases as one captured graph replayed with a new camera; NeRFRenderer.render_mesh_clip."""
import functools

import numpy as np
import pytest
import torch

import mesh_raster_clip_ref as cr
import mesh_raster_ref as ref
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

SMALL = (0, None, 1 << 30)
IMAGES = ("triangle_id", "depth", "mask", "image", "normal", "label")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _attributes(V, seed=5):
    rng = np.random.default_rng(seed)
    return dict(colors=rng.random((V, 3), dtype=np.float32), normals=rng.standard_normal((V, 3)).astype(np.float32),
                labels=rng.integers(0, 7, V).astype(np.uint8))


def _device(case, gpu, small=None, clip=True, **kw):
    from sanerf_hq_amd import raymarching as rm
    V = len(case["vertices"])
    attr = {k: torch.from_numpy(v).to(gpu) for k, v in _attributes(V).items()}
    mesh = {"vertices": torch.from_numpy(np.ascontiguousarray(case["vertices"], dtype=np.float32)).reshape(-1, 3).to(gpu),
            "triangles": torch.from_numpy(np.ascontiguousarray(case["triangles"], dtype=np.int32)).reshape(-1, 3).to(gpu)}
    args = dict(near=case.get("near", 0.05), cull=False, bg_color=0.75, small_max_pixels=small, **attr)
    args.update(kw)
    call = rm.mesh_rasterize_clip if clip else rm.mesh_rasterize
    return call(mesh, torch.from_numpy(np.asarray(case["pose"], dtype=np.float32)).to(gpu),
                torch.tensor(np.asarray(case["intrinsics"], dtype=np.float32)).to(gpu), case["H"], case["W"], **args)


def _restated(case, **kw):
    args = dict(bg_color=0.75, **_attributes(len(case["vertices"])))
    args.update(kw)
    return cr.run_case(case, **args)


def _assert_equal(out, want, what=""):
    for k in ("counts", "clip_counts"):
        assert out[k].dtype == torch.int32 and _np(out[k]).tolist() == want[k].tolist(), (what, k, _np(out[k]).tolist(), want[k].tolist())
    for k in IMAGES:
        got = _np(out[k])
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k)
        assert np.array_equal(_bits(got), _bits(want[k])), (what, k, int((_bits(got) != _bits(want[k])).sum()))


def _more_case():
    """The `dropped` case of the unclipped tests and what still drops a triangle under clipping (tests/test_mesh_raster_clip_ref.py)."""
    d = ref.hand_cases()["dropped"]
    v = np.concatenate([d["vertices"], np.array([(0.0, 0.0, 0.5), (1.0, 0.0, 1.0), (0.0, 1.0, -0.01), (np.inf, 0.0, 1.0), (3000.0, 0.0, -0.04)], dtype=np.float32)])
    tris = np.concatenate([d["triangles"], np.array([(6, 7, 8), (0, 6, 4), (0, 6, 5), (0, 1, 9), (0, 1, 10), (0, 1, 6)], dtype=np.int32)])
    return dict(d, vertices=v, triangles=tris)


@functools.lru_cache(maxsize=None)
def _cases():
    cases = dict(cr.hand_cases())
    cases["sphere"], cases["ground"], cases["dropped"] = cr.sphere_case(), cr.ground_case(), _more_case()
    # the camera off the sphere's centre, looking past it: pieces of every size, both windings of the screen
    cases["oblique"] = dict(cr.sphere_case(), pose=ref.look_at([0.3, -0.2, 0.4], target=(1.0, 0.5, -0.2)),
                            intrinsics=np.array([25.0, 22.0, 30.25, 33.5], dtype=np.float32), near=0.35, H=57, W=61)
    return cases


@functools.lru_cache(maxsize=None)
def _want(name, cull):
    return _restated(_cases()[name], cull=cull)


# ---- against the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("name", ["two_front", "behind_camera", "dropped", "sphere", "ground", "oblique"])
def test_device_equals_the_restatement(gpu, name, cull):
    case, want = _cases()[name], _want(name, cull)
    print(name, "cull", cull, "counts", want["counts"].tolist(), "clip_counts", want["clip_counts"].tolist())
    if name not in ("two_front", "behind_camera"):
        assert want["clip_counts"][0] > 0 and (cull or want["clip_counts"][1] > 0)
    for small in SMALL:                        # every drawn triangle through the wave kernel; the default; every one through its lane
        _assert_equal(_device(case, gpu, small, cull=cull), want, f"{name}, cull={cull}, small_max_pixels={small}")


def test_clip_shows_what_the_unclipped_entries_drop(gpu):
    for name in ("sphere", "ground"):
        case = _cases()[name]
        clipped, plain = _device(case, gpu), _device(case, gpu, clip=False)
        assert "clip_counts" not in plain
        more = int(clipped["mask"].sum()) - int(plain["mask"].sum())
        print(name, "pixels that only clipping covers:", more)
        assert more > 300 and bool((clipped["mask"] >= plain["mask"]).all())


@pytest.mark.parametrize("name", ["fan", "quad_02", "overlap_equal"])
def test_clip_of_a_mesh_that_nothing_cuts_is_the_unclipped_image(gpu, name):
    case = ref.hand_cases()[name]
    for small in SMALL:
        for cull in (False, True):
            a, b = _device(case, gpu, small, cull=cull), _device(case, gpu, small, clip=False, cull=cull)
            assert a["clip_counts"].tolist() == [0, 0]
            for k in IMAGES + ("counts",):
                assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), (small, cull, k)


def test_two_runs_give_equal_bits(gpu):
    case = _cases()["oblique"]
    for small in SMALL:
        a, b = _device(case, gpu, small), _device(case, gpu, small)
        for k in IMAGES + ("counts", "clip_counts"):
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


def test_one_graph_replayed_with_a_new_camera(gpu):
    from sanerf_hq_amd import raymarching as rm
    case = _cases()["oblique"]
    V = len(case["vertices"])
    attr = {k: torch.from_numpy(v).to(gpu) for k, v in _attributes(V).items()}
    mesh = {"vertices": torch.from_numpy(case["vertices"]).to(gpu), "triangles": torch.from_numpy(case["triangles"]).to(gpu)}
    pose, intr = torch.from_numpy(case["pose"]).to(gpu), torch.from_numpy(case["intrinsics"]).to(gpu)
    H, W, near = case["H"], case["W"], case["near"]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        rm.mesh_rasterize_clip(mesh, pose, intr, H, W, near=near, bg_color=0.75, **attr)       # warm-up: the scratch buffer exists
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = rm.mesh_rasterize_clip(mesh, pose, intr, H, W, near=near, bg_color=0.75, **attr)
    for eye, target in (([0.3, -0.2, 0.4], (1.0, 0.5, -0.2)), ([-0.5, 0.1, 0.2], (0.0, -1.0, 0.3))):
        new = ref.look_at(eye, target=target)
        pose.copy_(torch.from_numpy(new).to(gpu))
        graph.replay()
        torch.cuda.synchronize()
        eager = rm.mesh_rasterize_clip(mesh, pose, intr, H, W, near=near, bg_color=0.75, **attr)
        for k in IMAGES + ("counts", "clip_counts"):
            assert torch.equal(out[k], eager[k]), (eye, k)
        want = _restated(dict(case, pose=new))
        assert want["clip_counts"][0] > 0
        _assert_equal(out, want, f"replayed, eye {eye}")


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_mesh_raster.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


def test_render_mesh_clip_with_the_camera_inside_the_mesh(gpu, model):
    from sanerf_hq_amd import raymarching as rm
    res, H, W = 24, 40, 56
    intr = torch.tensor([60.0, 60.0, W / 2, H / 2], device=gpu)
    with torch.no_grad():
        thr = float(model.density_volume(res).median())
        mesh = model.extract_mesh(res, threshold=thr, vertex_colors=True, vertex_labels=True)
        lo, hi = mesh["vertices"].min(dim=0).values, mesh["vertices"].max(dim=0).values
        eye = (0.5 * (lo + hi)).tolist()                       # the middle of the mesh's box
        pose = torch.from_numpy(ref.look_at(eye, target=(eye[0] + 1.0, eye[1] + 0.3, eye[2] - 0.2))).to(gpu)
        out = model.render_mesh_clip(mesh, pose, intr, H, W, bg_color=0)
        plain = model.render_mesh(mesh, pose, intr, H, W, bg_color=0)
    T = mesh["triangles"].shape[0]
    assert sorted(out) == ["clip_counts", "counts", "depth", "image", "label", "mask", "triangle_id"]
    assert out["clip_counts"].dtype == torch.int32 and tuple(out["clip_counts"].shape) == (2,)
    print("render_mesh_clip: counts", out["counts"].tolist(), "clip_counts", out["clip_counts"].tolist(), "unclipped counts", plain["counts"].tolist())
    assert int(out["clip_counts"][0]) > 0 and int(out["counts"].sum()) == T
    assert int(out["counts"][1]) + int(out["clip_counts"][0]) <= int(plain["counts"][1])         # every clipped triangle was dropped before
    same = rm.mesh_rasterize_clip(mesh, pose, intr, H, W, near=model.min_near, bg_color=0.0)
    for k in out:
        assert torch.equal(out[k], same[k]), k
    want = cr.rasterize(_np(mesh["vertices"]), _np(mesh["triangles"]), _np(pose), _np(intr), H, W, near=model.min_near, colors=_np(mesh["colors"]),
                        labels=_np(mesh["labels"]), bg_color=0.0)
    for k in ("triangle_id", "depth", "mask", "image", "label", "counts", "clip_counts"):
        assert np.array_equal(_bits(_np(out[k])), _bits(want[k])), k
