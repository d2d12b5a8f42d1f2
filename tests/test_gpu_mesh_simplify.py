"""GPU: mesh simplification -- sn_rm_mesh_simplify_count / _emit against the numpy restatement in tests/mesh_simplify_ref.py: triangles,
cluster map and counts exactly, vertices and normals bit for bit; the properties that need no restatement; independence of the vertex
order and of the run; capacities; NeRFRenderer.extract_mesh(simplify=)."""
import numpy as np
import pytest
import torch

import mesh_ref as mr
import mesh_simplify_ref as ms
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

SHAPE = (24, 24, 24)


def _np(t):
    return t.cpu().numpy()


def _to_device(v, n, t, gpu):
    return {"vertices": torch.from_numpy(np.ascontiguousarray(v)).to(gpu), "normals": None if n is None else torch.from_numpy(np.ascontiguousarray(n)).to(gpu),
            "triangles": torch.from_numpy(np.ascontiguousarray(t)).to(gpu)}


def _host(mesh):
    return _np(mesh["vertices"]), None if mesh["normals"] is None else _np(mesh["normals"]), _np(mesh["triangles"])


def _fill_scratch(gpu):
    from sanerf_hq_amd import _buffers
    ws = _buffers.scratch("mesh_simplify", torch.device(gpu), 8 << 20)
    ws.fill_(0xA5)


def _assert_equal(out, want, what=""):
    """Exact: counts, triangles, cluster map; vertices and normals bit for bit."""
    assert out["vertices"].dtype == torch.float32 and out["triangles"].dtype == torch.int32
    assert [out["vertices"].shape[0], out["triangles"].shape[0]] == want["counts"].tolist(), what
    assert tuple(out["vertices"].shape) == want["vertices"].shape and tuple(out["triangles"].shape) == want["triangles"].shape, what
    assert np.array_equal(_np(out["triangles"]), want["triangles"]), what
    assert np.array_equal(_np(out["vertices"]).view(np.uint32), want["vertices"].view(np.uint32)), what
    if want["normals"] is None:
        assert out["normals"] is None
    else:
        assert np.array_equal(_np(out["normals"]).view(np.uint32), want["normals"].view(np.uint32)), what
    if "vertex_cluster" in out:
        assert out["vertex_cluster"].dtype == torch.int32 and np.array_equal(_np(out["vertex_cluster"]), want["vertex_cluster"]), what


def _run(mesh, lat, what=""):
    """mesh_simplify on the device mesh, equal to the restatement of the same arrays; the properties on the device's own output."""
    from sanerf_hq_amd import raymarching as rm
    origin, cell, dims = lat
    v, n, t = _host(mesh)
    want = ms.simplify(v, n, t, origin, cell, dims)
    out = rm.mesh_simplify(mesh, cell, origin=origin, dims=dims, return_cluster=True)
    print(f"{what}: V={len(v)} T={len(t)} cells={dims} -> V'={out['vertices'].shape[0]} T'={out['triangles'].shape[0]}")
    _assert_equal(out, want, what)
    ms.check_properties({k: _np(out[k]) for k in ("vertices", "triangles", "vertex_cluster")}, v, t, origin, cell, dims)
    return out, want


def _device_isosurface(volume, gpu, want=None):
    from sanerf_hq_amd import raymarching as rm
    mesh = rm.isosurface(torch.from_numpy(volume).to(gpu), 0.0)
    if want is not None:                                   # the fixture the CPU tests looked at
        assert np.array_equal(_np(mesh["triangles"]), want["triangles"])
        assert np.array_equal(_np(mesh["vertices"]).view(np.uint32), want["vertices"].view(np.uint32))
    return mesh


@pytest.mark.parametrize("k", ms.CELLS)
@pytest.mark.parametrize("name", list(ms.VOLUMES))
def test_volumes_equal_the_restatement(gpu, name, k):
    mesh = _device_isosurface(ms.VOLUMES[name](), gpu, ms.volume_mesh(name))
    out, want = _run(mesh, ms.aligned_lattice(SHAPE, k), f"{name} cell {k}")
    assert (want["cls"] != ms.INVALID).all() and out["triangles"].shape[0] > 0


def test_large_sphere_crosses_many_segments(gpu):
    """96^3: tens of thousands of triangles, dozens of segments of 1024, a loaded table, a bitmap of several words per segment."""
    mesh = _device_isosurface(mr.sphere_volume(96, (47.3, 48.1, 46.7), 37.6), gpu)
    T = mesh["triangles"].shape[0]
    assert T > 50 * 1024
    out, want = _run(mesh, ms.aligned_lattice((96, 96, 96), 2.0), "sphere 96^3 cell 2")
    assert 10 * 1024 < out["triangles"].shape[0] < T / 2
    _run(mesh, ms.aligned_lattice((96, 96, 96), 1.0), "sphere 96^3 cell 1")      # 97^3 cells: 28 bitmap segments
    # every triangle a second time, reversed: tens of thousands of key sets that two triangles enter, from lanes far apart
    twice = dict(mesh, triangles=torch.cat([mesh["triangles"], mesh["triangles"].flip(1)]).contiguous())
    again, want2 = _run(twice, ms.aligned_lattice((96, 96, 96), 2.0), "sphere 96^3 twice, cell 2")
    assert (want2["cls"][T:] != ms.KEPT).all() and (want2["cls"] == ms.DUPLICATE).sum() >= out["triangles"].shape[0]
    assert torch.equal(again["triangles"], out["triangles"]) and torch.equal(again["vertices"], out["vertices"])


@pytest.mark.parametrize("T", [1, 1024, 1025, 3 * 1024 + 1])
def test_triangle_counts_at_the_segment_edges(gpu, T):
    mesh = _device_isosurface(ms.VOLUMES["sphere"](), gpu)
    part = dict(mesh, triangles=mesh["triangles"][:T].contiguous())
    _, want = _run(part, ms.aligned_lattice(SHAPE, 1.0), f"first {T} triangles")
    assert (want["counts"][1] > 0) == (T > 1)                                 # (the first triangle alone collapses)


@pytest.mark.parametrize("fixture", ["hand_mesh", "duplicate_mesh", "degenerate_mesh", "terrain"])
def test_hand_built_fixtures(gpu, fixture):
    v, n, t, lat = getattr(ms, fixture)()
    out, want = _run(_to_device(v, n, t, gpu), lat, fixture)
    if fixture == "hand_mesh":
        assert _np(out["vertices"])[2].tolist() == [1.8125, -0.3125, -0.1875] and _np(out["triangles"]).tolist() == [[0, 2, 1], [2, 4, 3]]
    if fixture == "terrain":
        ms.check_fine_cells({k: _np(out[k]) for k in ("vertices", "normals", "triangles", "vertex_cluster")} | {"input_normals": n}, v, t, lat[1])


def test_malformed_mesh(gpu):
    """Indices out of range, NaN and infinite vertices, vertices outside the lattice, non-finite and absurd normals: results, no fault."""
    v, n, t, lat = ms.malformed(ms.volume_mesh("sphere"), SHAPE)
    out, want = _run(_to_device(v, n, t, gpu), lat, "malformed")
    assert (want["cls"] == ms.INVALID).sum() > 4
    assert torch.isfinite(out["vertices"]).all() and torch.isfinite(out["normals"]).all()
    cl = _np(out["vertex_cluster"])
    assert cl[5] == -1 and cl[len(v) // 4] == -1 and cl[len(v) // 2] == -1 and cl[len(v) // 3] == -1


def test_vertex_order_does_not_matter(gpu):
    """Permuted vertices, relabelled triangles in the same order: equal bits -- what the integer sums are for."""
    from sanerf_hq_amd import raymarching as rm
    mesh = _device_isosurface(ms.VOLUMES["two_blobs"](), gpu)
    origin, cell, dims = ms.aligned_lattice(SHAPE, 2.5)
    base = rm.mesh_simplify(mesh, cell, origin=origin, dims=dims, return_cluster=True)
    V = mesh["vertices"].shape[0]
    for seed in (1, 2):
        perm = torch.from_numpy(np.random.default_rng(seed).permutation(V)).to(gpu)        # new row j holds old vertex perm[j]
        inverse = torch.empty_like(perm)
        inverse[perm] = torch.arange(V, device=gpu)
        other = {"vertices": mesh["vertices"][perm].contiguous(), "normals": mesh["normals"][perm].contiguous(),
                 "triangles": inverse[mesh["triangles"].long()].to(torch.int32).contiguous()}
        out = rm.mesh_simplify(other, cell, origin=origin, dims=dims, return_cluster=True)
        for key in ("vertices", "normals", "triangles"):
            assert torch.equal(out[key].view(torch.int32), base[key].view(torch.int32)), key
        assert torch.equal(out["vertex_cluster"], base["vertex_cluster"][perm])


def test_two_calls_give_equal_bits(gpu):
    from sanerf_hq_amd import raymarching as rm
    mesh = _device_isosurface(ms.VOLUMES["sphere"](), gpu)
    origin, cell, dims = ms.aligned_lattice(SHAPE, 2.0)
    first = rm.mesh_simplify(mesh, cell, origin=origin, dims=dims, return_cluster=True)
    again = rm.mesh_simplify(mesh, cell, origin=origin, dims=dims, return_cluster=True)
    _fill_scratch(gpu)                                     # nothing of an earlier call, or of the fill, may show
    poisoned = rm.mesh_simplify(mesh, cell, origin=origin, dims=dims, return_cluster=True)
    for other in (again, poisoned):
        for key in ("vertices", "normals", "triangles", "vertex_cluster"):
            assert torch.equal(first[key].view(torch.int32), other[key].view(torch.int32)), key


def test_everything_in_one_cell_and_empty_meshes(gpu):
    from sanerf_hq_amd import raymarching as rm
    mesh = _device_isosurface(ms.VOLUMES["sphere"](), gpu)
    out = rm.mesh_simplify(mesh, 64.0, origin=(-1.0, -1.0, -1.0), dims=(1, 1, 1), return_cluster=True)
    assert tuple(out["vertices"].shape) == (0, 3) and tuple(out["normals"].shape) == (0, 3) and tuple(out["triangles"].shape) == (0, 3)
    assert (out["vertex_cluster"] == -1).all() and out["vertex_cluster"].shape[0] == mesh["vertices"].shape[0]
    none = torch.zeros(0, 3, device=gpu, dtype=torch.int32)
    for V in (0, 5):
        out = rm.mesh_simplify({"vertices": torch.rand(V, 3, device=gpu), "normals": None, "triangles": none}, 0.25, return_cluster=True)
        assert tuple(out["vertices"].shape) == (0, 3) and tuple(out["triangles"].shape) == (0, 3) and out["normals"] is None
        assert out["vertex_cluster"].tolist() == [-1] * V
    nan = {"vertices": torch.full((3, 3), float("nan"), device=gpu), "normals": None, "triangles": torch.tensor([[0, 1, 2]], device=gpu, dtype=torch.int32)}
    assert rm.mesh_simplify(nan, 1.0)["triangles"].shape[0] == 0             # no finite vertex, no lattice


def test_default_lattice_covers_the_mesh(gpu):
    """origin = dims = None: the bounding box of the finite vertices, pulled back by half a cell; nothing but the non-finite rows is lost."""
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.raymarching import mesh as rm_mesh
    v, n, t, _ = ms.terrain()
    v = v.copy()
    v[4, 0] = np.nan
    mesh = _to_device(v * np.float32(0.37) - np.float32(2.0), n, t, gpu)
    for cell in (0.05, (0.3, 0.2, 0.15)):
        triple = [cell] * 3 if isinstance(cell, float) else list(cell)
        origin, dims = rm_mesh._covering_lattice(mesh["vertices"], triple)
        hv, hn, ht = _host(mesh)
        want = ms.simplify(hv, hn, ht, origin, triple, dims)
        assert (want["key"] >= 0).sum() == len(v) - 1 and want["key"][4] == -1
        lo = np.nanmin(hv, axis=0)
        assert np.allclose(np.asarray(origin), lo - 0.5 * np.asarray(triple), rtol=0, atol=1e-6)
        out = rm.mesh_simplify(mesh, cell, return_cluster=True)
        _assert_equal(out, want, cell)


def test_capacities_truncate_and_guards_stay(gpu):
    """cap_v and cap_t below the counts: the stored prefix is the full result's; the rows behind the capacities keep their fill."""
    from sanerf_hq_amd import raymarching as rm
    mesh = _device_isosurface(ms.VOLUMES["two_blobs"](), gpu)
    origin, cell, dims = ms.aligned_lattice(SHAPE, 2.0)
    full = rm.mesh_simplify(mesh, cell[0], origin=origin, dims=dims, return_cluster=True)
    nv, nt = full["vertices"].shape[0], full["triangles"].shape[0]
    V = mesh["vertices"].shape[0]
    assert 64 < nv < V and 64 < nt
    for cap_v, cap_t in ((nv // 2 + 1, nt // 3 + 1), (1, nt), (nv, 1), (0, 7), (5, 0), (1, 1), (nv + 9, nt + 9)):
        counts, ws = rm.mesh_simplify_counts(mesh["vertices"], mesh["normals"], mesh["triangles"], origin, cell, dims)
        assert counts.tolist() == [nv, nt]
        guard = 64
        ov = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        on = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        ot = torch.full((cap_t + guard, 3), -7, device=gpu, dtype=torch.int32)
        oc = torch.full((V + guard,), -7, device=gpu, dtype=torch.int32)
        rm.mesh_simplify_emit(mesh["vertices"], mesh["normals"], mesh["triangles"], origin, cell, dims, ws, ov, on, ot, oc, cap_v=cap_v, cap_t=cap_t)
        mv, mt = min(cap_v, nv), min(cap_t, nt)
        assert torch.equal(ov[:mv], full["vertices"][:mv]) and torch.equal(on[:mv], full["normals"][:mv]) and torch.equal(ot[:mt], full["triangles"][:mt])
        assert torch.equal(oc[:V], full["vertex_cluster"])
        assert (ov[mv:] == -7.0).all() and (on[mv:] == -7.0).all() and (ot[mt:] == -7).all() and (oc[V:] == -7).all()


def test_without_normals(gpu):
    mesh = _device_isosurface(ms.VOLUMES["sphere"](), gpu)
    out, _ = _run(dict(mesh, normals=None), ms.aligned_lattice(SHAPE, 2.0), "no normals")
    assert out["normals"] is None
    from sanerf_hq_amd import raymarching as rm
    origin, cell, dims = ms.aligned_lattice(SHAPE, 2.0)
    with_normals = rm.mesh_simplify(mesh, cell, origin=origin, dims=dims)
    assert "vertex_cluster" not in with_normals
    assert torch.equal(with_normals["vertices"], out["vertices"]) and torch.equal(with_normals["triangles"], out["triangles"])


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_mesh.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


def test_extract_mesh_simplify(gpu, model):
    from sanerf_hq_amd import raymarching as rm
    res = 24
    with torch.no_grad():
        thr = float(model.density_volume(res).median())
        plain = model.extract_mesh(res, threshold=thr)
        off = model.extract_mesh(res, threshold=thr, simplify=0)                 # today's path, bit for bit
        for k in ("vertices", "normals", "triangles"):
            assert torch.equal(plain[k].view(torch.int32), off[k].view(torch.int32)), k
        _, origin, step = model._lattice(res, None)
        for simplify, clean in ((2, {}), (2.5, {}), (2, dict(keep_largest=1))):
            got = model.extract_mesh(res, threshold=thr, simplify=simplify, **clean)
            lat = ms.aligned_lattice((res,) * 3, simplify, origin, step)
            by_hand = rm.mesh_simplify(rm.mesh_clean(plain, **clean), lat[1], origin=lat[0], dims=lat[2])
            print(f"extract_mesh simplify={simplify} {clean}: T={plain['triangles'].shape[0]} -> T'={got['triangles'].shape[0]}")
            assert 0 < got["triangles"].shape[0] < plain["triangles"].shape[0] / 2
            for k in ("vertices", "normals", "triangles"):
                assert torch.equal(got[k].view(torch.int32), by_hand[k].view(torch.int32)), k
            v, n, t = _host(rm.mesh_clean(plain, **clean))
            _assert_equal(got, ms.simplify(v, n, t, *lat), simplify)
        with pytest.raises(ValueError, match="simplify"):
            model.extract_mesh(res, threshold=thr, simplify=0.5)
