"""GPU: mesh clean-up -- sn_rm_mesh_components_* / sn_rm_mesh_component_stats / sn_rm_mesh_filter_count / _emit against the numpy
restatement in tests/mesh_clean_ref.py, exactly; the round count; triangle soup; capacities; NeRFRenderer.extract_mesh's new options."""
import numpy as np
import pytest
import torch

import mesh_clean_ref as mc
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

FIXTURE_NAMES = list(mc.FIXTURES)


def _np(t):
    return t.cpu().numpy()


def _device_mesh(name, gpu):
    """The isosurface of the fixture's volume by the device, checked equal to the restatement's (so the labels below are comparable)."""
    from sanerf_hq_amd import raymarching as rm
    fx = mc.fixture(name)
    mesh = rm.isosurface(torch.from_numpy(fx["volume"]).to(gpu), fx["iso"])
    assert np.array_equal(_np(mesh["triangles"]), fx["mesh"]["triangles"])
    assert np.array_equal(_np(mesh["vertices"]).view(np.uint32), fx["mesh"]["vertices"].view(np.uint32))
    return fx, mesh


def _assert_components(got, lab, st, what=""):
    assert got["labels"].dtype == torch.int32 and got["triangle_counts"].dtype == torch.int32 and got["vertex_counts"].dtype == torch.int32
    assert np.array_equal(_np(got["labels"]), lab), what
    assert np.array_equal(_np(got["triangle_counts"]), st["triangle_counts"]), what
    assert np.array_equal(_np(got["vertex_counts"]), st["vertex_counts"]), what
    assert got["counts"].is_cuda and got["counts"].tolist() == st["counts"].tolist(), what


def _fill_scratch(gpu):
    from sanerf_hq_amd import _buffers
    ws = _buffers.scratch("mesh_clean", torch.device(gpu), 4 << 20)      # larger than any workspace of this file: the same buffer is used next
    ws.fill_(0xA5)


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_components_equal_the_restatement(gpu, name):
    from sanerf_hq_amd import raymarching as rm
    fx, mesh = _device_mesh(name, gpu)
    V = mesh["vertices"].shape[0]
    got = rm.mesh_components(mesh["triangles"], V)
    print(f"{name}: V={V} T={mesh['triangles'].shape[0]} components {got['counts'].tolist()} rounds {got['rounds']}")
    _assert_components(got, fx["labels"], fx, name)
    again = rm.mesh_components(mesh["triangles"], V)
    _fill_scratch(gpu)
    poisoned = rm.mesh_components(mesh["triangles"], V)
    for other in (again, poisoned):
        for k in ("labels", "triangle_counts", "vertex_counts", "counts"):
            assert torch.equal(got[k], other[k]), k


@pytest.mark.parametrize("name", ["serpentine", "noise_multi"])
def test_rounds_are_logarithmic_not_the_diameter(gpu, name):
    """The synchronous model needs 4 rounds on both and plain propagation 119 / 148: 16 separates the classes of algorithm."""
    from sanerf_hq_amd import raymarching as rm
    fx, mesh = _device_mesh(name, gpu)
    got = rm.mesh_components(mesh["triangles"], mesh["vertices"].shape[0])
    print(f"{name}: device rounds {got['rounds']}, synchronous model {mc.model_rounds(fx['mesh']['triangles'], len(fx['labels']))}")
    assert 1 <= got["rounds"] <= 16


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_triangle_soup(gpu, V):
    from sanerf_hq_amd import raymarching as rm
    rng = np.random.default_rng(V)
    vert = rng.standard_normal((V, 3)).astype(np.float32)
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    for T in (0, 12, max(V // 3, 13), 2 * V + 12):
        t = mc.soup(V, T, seed=V + T)
        lab = mc.components(t, V)
        st = mc.stats(t, V, lab)
        tri = torch.from_numpy(t).to(gpu)
        got = rm.mesh_components(tri, V)
        _assert_components(got, lab, st, (V, T))
        if T:
            assert (~mc.valid_triangles(t, V)).any()
        mesh = {"vertices": torch.from_numpy(vert).to(gpu), "normals": torch.from_numpy(nrm).to(gpu), "triangles": tri}
        for kw in (dict(min_triangles=1), dict(min_triangles=3), dict(keep_largest=1), dict(keep_largest=3, min_triangles=2)):
            keep, _ = mc.select(lab, st["triangle_counts"], **kw)
            want = mc.filter(vert, nrm, t, lab, keep)
            _fill_scratch(gpu)
            out = rm.mesh_clean(mesh, return_source=True, **kw)
            _assert_mesh(out, want, (V, T, kw))


def _assert_mesh(out, want, what=""):
    assert out["vertices"].dtype == torch.float32 and out["triangles"].dtype == torch.int32
    assert tuple(out["vertices"].shape) == want["vertices"].shape and tuple(out["triangles"].shape) == want["triangles"].shape, what
    assert np.array_equal(_np(out["triangles"]), want["triangles"]), what
    assert np.array_equal(_np(out["vertices"]).view(np.uint32), want["vertices"].view(np.uint32)), what
    if want["normals"] is None:
        assert out["normals"] is None
    else:
        assert np.array_equal(_np(out["normals"]).view(np.uint32), want["normals"].view(np.uint32)), what
    if "source_vertex" in out:
        assert out["source_vertex"].dtype == torch.int32 and np.array_equal(_np(out["source_vertex"]), want["source_vertex"]), what


OPTIONS = ([dict(min_triangles=m) for m in (1, 25, 100, 10 ** 9)] + [dict(keep_largest=k) for k in (1, 2, 6, 7, 5000)]
           + [dict(min_triangles=25, keep_largest=6), dict(min_triangles=100, keep_largest=5000), dict(min_triangles=700, keep_largest=6)])


@pytest.mark.parametrize("name", ["two_spheres_speck", "noise_sparse", "special"])
def test_filter_equals_the_restatement(gpu, name):
    from sanerf_hq_amd import raymarching as rm
    fx, mesh = _device_mesh(name, gpu)
    ref = dict(fx["mesh"], normals=_np(mesh["normals"]))       # rows of the INPUT, bit for bit (the device's own normals)
    for kw in OPTIONS:
        keep, _ = mc.select(fx["labels"], fx["triangle_counts"], **kw)
        want = mc.filter(ref["vertices"], ref["normals"], ref["triangles"], fx["labels"], keep)
        out = rm.mesh_clean(mesh, return_source=True, **kw)
        print(f"{name} {kw}: V'={out['vertices'].shape[0]} T'={out['triangles'].shape[0]}")
        _assert_mesh(out, want, (name, kw))
        if kw.get("min_triangles") == 10 ** 9:
            assert tuple(out["vertices"].shape) == (0, 3) and tuple(out["normals"].shape) == (0, 3) and tuple(out["triangles"].shape) == (0, 3)
        rows = out["source_vertex"].long()
        assert torch.equal(out["vertices"], mesh["vertices"][rows]) and torch.equal(out["normals"], mesh["normals"][rows])
    if name == "noise_sparse":
        out = rm.mesh_clean(mesh, min_triangles=100)
        assert (out["vertices"].shape[0], out["triangles"].shape[0]) == (24252, 46894) and "source_vertex" not in out
    # normals=None is carried through
    bare = dict(mesh, normals=None)
    out = rm.mesh_clean(bare, keep_largest=2)
    keep, _ = mc.select(fx["labels"], fx["triangle_counts"], keep_largest=2)
    _assert_mesh(out, mc.filter(ref["vertices"], None, ref["triangles"], fx["labels"], keep))
    assert out["normals"] is None
    assert rm.mesh_clean(mesh) is mesh


@pytest.mark.parametrize("name,kw", [("noise_sparse", dict(min_triangles=100)), ("two_spheres_speck", dict(keep_largest=2))])
def test_capacities_truncate_and_guards_stay(gpu, name, kw):
    """cap_v and cap_t below the counts: the stored prefix is the full result's; the rows behind the capacities keep their fill."""
    from sanerf_hq_amd import raymarching as rm
    _, mesh = _device_mesh(name, gpu)
    V = mesh["vertices"].shape[0]
    full = rm.mesh_clean(mesh, return_source=True, **kw)
    nv, nt = full["vertices"].shape[0], full["triangles"].shape[0]
    assert 0 < nv < V and 0 < nt < mesh["triangles"].shape[0]
    comp = rm.mesh_components(mesh["triangles"], V)
    for cap_v, cap_t in ((nv // 2 + 1, nt // 3 + 1), (1, nt), (nv, 1), (0, 7), (5, 0), (1, 1)):
        counts, ws = rm.mesh_filter_counts(mesh["triangles"], V, comp, **kw)
        assert counts.tolist() == [nv, nt]
        guard = 64
        v = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        n = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        s = torch.full((cap_v + guard,), -7, device=gpu, dtype=torch.int32)
        t = torch.full((cap_t + guard, 3), -7, device=gpu, dtype=torch.int32)
        rm.mesh_filter_emit(mesh["triangles"], mesh["vertices"], mesh["normals"], ws, v, n, t, s, cap_v=cap_v, cap_t=cap_t)
        assert torch.equal(v[:cap_v], full["vertices"][:cap_v]) and torch.equal(n[:cap_v], full["normals"][:cap_v])
        assert torch.equal(s[:cap_v], full["source_vertex"][:cap_v]) and torch.equal(t[:cap_t], full["triangles"][:cap_t])
        assert (v[cap_v:] == -7.0).all() and (n[cap_v:] == -7.0).all() and (s[cap_v:] == -7).all() and (t[cap_t:] == -7).all()


def test_empty_meshes(gpu):
    from sanerf_hq_amd import raymarching as rm
    none = torch.zeros(0, 3, device=gpu, dtype=torch.int32)
    got = rm.mesh_components(none, 0)
    assert got["labels"].shape[0] == 0 and got["counts"].tolist() == [0, 0] and got["rounds"] == 0
    got = rm.mesh_components(none, 5)
    assert got["labels"].tolist() == [0, 1, 2, 3, 4] and got["counts"].tolist() == [5, 0] and got["rounds"] == 1
    for V in (0, 5):
        out = rm.mesh_clean({"vertices": torch.zeros(V, 3, device=gpu), "normals": None, "triangles": none}, min_triangles=1, return_source=True)
        assert tuple(out["vertices"].shape) == (0, 3) and tuple(out["triangles"].shape) == (0, 3) and out["source_vertex"].shape[0] == 0


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


@pytest.mark.parametrize("ids", [None, [1]])
def test_extract_mesh_options(gpu, model, ids):
    from sanerf_hq_amd import raymarching as rm
    with torch.no_grad():
        thr = float(model.density_volume(24).median())
        vol = model.density_volume(24, instance_ids=ids)
        _, origin, step = model._lattice(24, None)
        want = rm.isosurface(vol, thr, origin, step)
        plain = model.extract_mesh(24, threshold=thr, instance_ids=ids)                      # the defaults: today's path
        for k in ("vertices", "normals", "triangles"):
            assert torch.equal(plain[k], want[k]), k
        comp = rm.mesh_components(want["triangles"], want["vertices"].shape[0])
        print(f"extract_mesh 24^3 ids={ids}: V={want['vertices'].shape[0]} T={want['triangles'].shape[0]} components {comp['counts'].tolist()}")
        assert comp["counts"].tolist()[1] > 1, "the test needs a mesh of several components"
        one = model.extract_mesh(24, threshold=thr, instance_ids=ids, keep_largest=1)
        ref = rm.mesh_clean(want, keep_largest=1)
        for k in ("vertices", "normals", "triangles"):
            assert torch.equal(one[k], ref[k]), k
        V1 = one["vertices"].shape[0]
        assert 0 < V1 < want["vertices"].shape[0]
        after = rm.mesh_components(one["triangles"], V1)
        assert after["counts"].tolist() == [1, 1]
        assert int(after["triangle_counts"][0]) == one["triangles"].shape[0] == int(comp["triangle_counts"].max())
        some = model.extract_mesh(24, threshold=thr, instance_ids=ids, min_component_triangles=10, normals=False)
        ref = rm.mesh_clean(rm.isosurface(vol, thr, origin, step, normals=False), min_triangles=10)
        assert some["normals"] is None and torch.equal(some["triangles"], ref["triangles"]) and torch.equal(some["vertices"], ref["vertices"])
