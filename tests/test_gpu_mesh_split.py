"""GPU: mesh split -- sn_rm_mesh_split_count / _emit and raymarching.mesh_split against the numpy restatement in tests/mesh_split_ref.py,
exactly, on every output array; capacities; repeat and poisoned scratch; a marching-tetrahedra mesh cut by a plane;
NeRFRenderer.extract_object_meshes."""
import numpy as np
import pytest
import torch

import mesh_clean_ref as mc
import mesh_split_ref as ms
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

P = ms.P
PACKED = ("vertices", "normals", "triangles", "source_vertex", "source_triangle", "part_triangle_offsets", "part_vertex_offsets")


def _np(t):
    return t.cpu().numpy()


def _rows(V, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.standard_normal((V, 3)).astype(np.float32)


def _device_mesh(vert, nrm, tri, gpu):
    return {"vertices": torch.from_numpy(vert).to(gpu), "normals": None if nrm is None else torch.from_numpy(nrm).to(gpu),
            "triangles": torch.from_numpy(tri).to(gpu)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_split(out, want, what=""):
    """Every array of mesh_split(return_source=True) equals the restatement's, and the parts are its slices."""
    nv, nt = (int(c) for c in want["counts"])
    assert out["vertices"].dtype == torch.float32 and out["triangles"].dtype == torch.int32
    assert tuple(out["vertices"].shape) == (nv, 3) and tuple(out["triangles"].shape) == (nt, 3), what
    for k in ("part_triangle_offsets", "part_vertex_offsets"):
        assert out[k].dtype == torch.int32 and out[k].is_cuda and np.array_equal(_np(out[k]), want[k]), (what, k)
    assert np.array_equal(_np(out["triangles"]), want["triangles"]), what
    assert np.array_equal(_bits(_np(out["vertices"])), _bits(want["vertices"])), what
    if want["normals"] is None:
        assert out["normals"] is None
    else:
        assert np.array_equal(_bits(_np(out["normals"])), _bits(want["normals"])), what
    if "source_vertex" in out:
        for k in ("source_vertex", "source_triangle"):
            assert out[k].dtype == torch.int32 and np.array_equal(_np(out[k]), want[k]), (what, k)
    toff, voff = want["part_triangle_offsets"], want["part_vertex_offsets"]
    assert sorted(out["parts"]) == [p for p in range(P) if toff[p + 1] > toff[p]], what
    for p, part in out["parts"].items():
        assert torch.equal(part["triangles"], out["triangles"][toff[p]:toff[p + 1]]) and torch.equal(part["vertices"], out["vertices"][voff[p]:voff[p + 1]])
        assert (part["normals"] is None) == (want["normals"] is None)
        if part["normals"] is not None:
            assert torch.equal(part["normals"], out["normals"][voff[p]:voff[p + 1]])


def _fill_scratch(gpu):
    from sanerf_hq_amd import _buffers
    ws = _buffers.scratch("mesh_split", torch.device(gpu), 4 << 20)      # larger than any workspace of this file: the same buffer is used next
    ws.fill_(0xA5)


def _equal_outputs(a, b):
    for k in PACKED:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4097]


@pytest.mark.parametrize("V", SIZES)
def test_random_soups_equal_the_restatement(gpu, V):
    """V and T over the wave, segment and workgroup edges; labels from {0, 1, 5, 31, 32, 200, 255}; invalid rows mixed in; with and without
    normals and sources."""
    from sanerf_hq_amd import raymarching as rm
    vert, nrm = _rows(V, V)
    for T in SIZES:
        tri, lab = ms.soup(V, T, seed=1000 * V + T)
        labels = torch.from_numpy(lab).to(gpu)
        with_normals = (V + T) % 2 == 0
        want = ms.split(vert, nrm if with_normals else None, tri, lab)
        mesh = _device_mesh(vert, nrm if with_normals else None, tri, gpu)
        out = rm.mesh_split(mesh, labels, return_source=True)
        _assert_split(out, want, (V, T))
        bare = rm.mesh_split(dict(mesh, labels=labels))                                      # the mesh's own labels, no sources
        assert "source_vertex" not in bare and "source_triangle" not in bare
        _assert_split(bare, want, (V, T, "bare"))
        assert all(torch.equal(part["labels"], labels[out["source_vertex"][want["part_vertex_offsets"][p]:want["part_vertex_offsets"][p + 1]].long()])
                   for p, part in bare["parts"].items())
        if T >= 8 and V > 1:
            assert (ms.triangle_parts(tri, lab) < 0).any()


def test_thirty_three_segments_cross_a_scan_tile(gpu):
    """T = V = 33 000: 33 segments each, so both part-major tables have 33 * 33 = 1089 > 1024 entries and the scan carries into a second
    tile.  Then equal bits on a second call and after the scratch buffer was filled with 0xA5."""
    from sanerf_hq_amd import raymarching as rm
    V = T = 33000
    vert, nrm = _rows(V, 7)
    tri, lab = ms.soup(V, T, seed=33)
    want = ms.split(vert, nrm, tri, lab)
    toff = want["part_triangle_offsets"]
    assert sum(1 for p in range(P) if toff[p + 1] > toff[p]) == 5 and toff[P] > 30000            # parts 0, 1, 5, 31, 32
    mesh = _device_mesh(vert, nrm, tri, gpu)
    labels = torch.from_numpy(lab).to(gpu)
    out = rm.mesh_split(mesh, labels, return_source=True)
    _assert_split(out, want, "33000")
    again = rm.mesh_split(mesh, labels, return_source=True)
    _fill_scratch(gpu)
    poisoned = rm.mesh_split(mesh, labels, return_source=True)
    _equal_outputs(out, again)
    _equal_outputs(out, poisoned)


@pytest.mark.parametrize("case", ["one_part", "three_way_ties", "empty_parts_between", "all_invalid", "all_none"])
def test_special_label_patterns(gpu, case):
    from sanerf_hq_amd import raymarching as rm
    V, T = 1500, 2600
    vert, nrm = _rows(V, 11)
    rng = np.random.default_rng(12)
    tri, lab = ms.soup(V, T, seed=13, invalid=case != "three_way_ties")
    if case == "one_part":
        lab[:] = 5
    elif case == "three_way_ties":                       # corner q of every triangle has label {1, 0, 9}[q]: all go to part 0
        lab = np.array([1, 0, 9], dtype=np.uint8)[np.arange(V) % 3]
        tri = (3 * rng.integers(0, V // 3, size=(T, 3)) + np.arange(3)).astype(np.int32)
    elif case == "empty_parts_between":
        lab = np.array([0, 31, 255], dtype=np.uint8)[rng.integers(0, 3, size=V)]
    elif case == "all_invalid":
        tri[:, 1] = V
    elif case == "all_none":
        lab[:] = 255
    want = ms.split(vert, nrm, tri, lab)
    toff = want["part_triangle_offsets"]
    full = [p for p in range(P) if toff[p + 1] > toff[p]]
    assert full == dict(one_part=[5], three_way_ties=[0], empty_parts_between=[0, 31, 32], all_invalid=[], all_none=[32])[case]
    if case == "three_way_ties":
        assert toff[P] == T and len(set(want["source_vertex"].tolist())) == want["counts"][0]
    _fill_scratch(gpu)
    out = rm.mesh_split(_device_mesh(vert, nrm, tri, gpu), torch.from_numpy(lab).to(gpu), return_source=True)
    _assert_split(out, want, case)


def test_empty_meshes(gpu):
    from sanerf_hq_amd import raymarching as rm
    for V, T in ((0, 0), (5, 0), (0, 3)):
        mesh = {"vertices": torch.zeros(V, 3, device=gpu), "normals": torch.zeros(V, 3, device=gpu),
                "triangles": torch.zeros(T, 3, device=gpu, dtype=torch.int32)}
        labels = torch.zeros(V, device=gpu, dtype=torch.uint8)
        offsets, counts, _ = rm.mesh_split_counts(mesh["triangles"], V, labels)
        assert counts.tolist() == [0, 0] and all(o.tolist() == [0] * (P + 1) for o in offsets.values())
        out = rm.mesh_split(mesh, labels, return_source=True)
        assert out["parts"] == {} and tuple(out["vertices"].shape) == (0, 3) and tuple(out["normals"].shape) == (0, 3)
        assert tuple(out["triangles"].shape) == (0, 3) and out["source_vertex"].shape[0] == 0 and out["source_triangle"].shape[0] == 0
        assert out["part_triangle_offsets"].tolist() == [0] * (P + 1) and out["part_vertex_offsets"].tolist() == [0] * (P + 1)
    # the library's own answer to an empty mesh: the outputs that are given are zeroed
    from sanerf_hq_amd import _lib
    a, b, c = (torch.full((n,), -7, device=gpu, dtype=torch.int32) for n in (P + 1, P + 1, 2))
    _lib.check(_lib.lib().sn_rm_mesh_split_count(None, 0, 9, None, None, 0, a.data_ptr(), b.data_ptr(), c.data_ptr(), _lib.stream()))
    assert not a.any() and not b.any() and not c.any()


def test_capacities_truncate_and_guards_stay(gpu):
    """cap_v and cap_t below the counts: the stored prefix is the full result's; the rows behind the capacities keep their fill."""
    from sanerf_hq_amd import raymarching as rm
    V, T = 3000, 5000
    vert, nrm = _rows(V, 21)
    tri, lab = ms.soup(V, T, seed=22)
    mesh = _device_mesh(vert, nrm, tri, gpu)
    labels = torch.from_numpy(lab).to(gpu)
    full = rm.mesh_split(mesh, labels, return_source=True)
    nv, nt = full["vertices"].shape[0], full["triangles"].shape[0]
    assert nv > V and 0 < nt < T                             # seam vertices are duplicated; invalid triangles are dropped
    for cap_v, cap_t in ((nv // 2 + 1, nt // 3 + 1), (1, nt), (nv, 1), (0, 7), (5, 0), (1, 1), (nv + 9, nt + 9)):
        _, counts, ws = rm.mesh_split_counts(mesh["triangles"], V, labels)
        assert counts.tolist() == [nv, nt]
        guard = 64
        v = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        n = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        sv = torch.full((cap_v + guard,), -7, device=gpu, dtype=torch.int32)
        t = torch.full((cap_t + guard, 3), -7, device=gpu, dtype=torch.int32)
        st = torch.full((cap_t + guard,), -7, device=gpu, dtype=torch.int32)
        rm.mesh_split_emit(mesh["triangles"], mesh["vertices"], mesh["normals"], ws, v, n, t, sv, st, cap_v=cap_v, cap_t=cap_t)
        kv, kt = min(cap_v, nv), min(cap_t, nt)
        assert torch.equal(v[:kv], full["vertices"][:kv]) and torch.equal(n[:kv], full["normals"][:kv]) and torch.equal(sv[:kv], full["source_vertex"][:kv])
        assert torch.equal(t[:kt], full["triangles"][:kt]) and torch.equal(st[:kt], full["source_triangle"][:kt])
        assert (v[kv:] == -7.0).all() and (n[kv:] == -7.0).all() and (sv[kv:] == -7).all() and (t[kt:] == -7).all() and (st[kt:] == -7).all()
    # without normals and without sources
    _, _, ws = rm.mesh_split_counts(mesh["triangles"], V, labels)
    v = torch.full((nv + 8, 3), -7.0, device=gpu)
    t = torch.full((nt + 8, 3), -7, device=gpu, dtype=torch.int32)
    rm.mesh_split_emit(mesh["triangles"], mesh["vertices"], None, ws, v, None, t)
    assert torch.equal(v[:nv], full["vertices"]) and torch.equal(t[:nt], full["triangles"]) and (v[nv:] == -7.0).all() and (t[nt:] == -7).all()


def test_marching_tetrahedra_mesh_cut_by_a_plane(gpu):
    """The two-spheres fixture of the clean-up tests with labels 0 / 1 by the plane x = 11.5, which passes through neither sphere's centre
    but cuts the first: each side is a part, each part has at least one component, and no triangle is lost."""
    from sanerf_hq_amd import raymarching as rm
    fx = mc.fixture("two_spheres_speck")
    ref = fx["mesh"]
    lab = np.where(ref["vertices"][:, 0] < 11.5, 0, 1).astype(np.uint8)
    assert 0 < lab.sum() < len(lab)
    mesh = rm.isosurface(torch.from_numpy(fx["volume"]).to(gpu), fx["iso"])
    assert np.array_equal(_np(mesh["triangles"]), ref["triangles"]) and np.array_equal(_bits(_np(mesh["vertices"])), _bits(ref["vertices"]))
    want = ms.split(ref["vertices"], _np(mesh["normals"]), ref["triangles"], lab)
    out = rm.mesh_split(mesh, torch.from_numpy(lab).to(gpu), return_source=True)
    _assert_split(out, want, "two_spheres_speck")
    assert sorted(out["parts"]) == [0, 1]
    T = mesh["triangles"].shape[0]
    assert sum(part["triangles"].shape[0] for part in out["parts"].values()) == T
    for p, part in out["parts"].items():
        comp = rm.mesh_components(part["triangles"], part["vertices"].shape[0])
        n_roots, n_with_triangles = comp["counts"].tolist()
        print(f"part {p}: V={part['vertices'].shape[0]} T={part['triangles'].shape[0]} components {n_with_triangles}")
        assert n_with_triangles >= 1 and n_roots == n_with_triangles                         # no vertex without a triangle in a part
    seam = out["vertices"].shape[0] - mesh["vertices"].shape[0]
    assert seam > 0                                                                          # the cut duplicates its seam vertices


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]
RES = 24


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_mesh_attr.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


def test_extract_object_meshes(gpu, model):
    from sanerf_hq_amd import raymarching as rm
    keys = ("vertices", "normals", "triangles", "colors", "coverage", "labels")
    with torch.no_grad():
        thr = float(model.density_volume(RES).median())
        kw = dict(resolution=RES, threshold=thr, vertex_colors=True)
        scene = model.extract_mesh(vertex_labels=True, **kw)
        split = rm.mesh_split(scene, return_source=True)
        objects = model.extract_object_meshes(**kw)
        occurring = sorted(set(scene["labels"].tolist()))
        print(f"extract_object_meshes {RES}^3: V={scene['vertices'].shape[0]} T={scene['triangles'].shape[0]}, labels {occurring}, "
              f"parts {[(p, m['triangles'].shape[0]) for p, m in split['parts'].items()]}")
        assert sorted(objects) == [l for l in occurring if l < 32] == [p for p in split["parts"] if p < 32]
        assert len(objects) >= 2, "the test needs a scene of several objects"
        voff = split["part_vertex_offsets"].tolist()
        for p, obj in objects.items():
            assert set(obj) == set(keys)
            rows = split["source_vertex"][voff[p]:voff[p + 1]].long()
            for k in keys:
                assert torch.equal(obj[k], split["parts"][p][k]), (p, k)
            assert torch.equal(obj["colors"], scene["colors"][rows]) and torch.equal(obj["labels"], scene["labels"][rows])
            assert torch.equal(obj["coverage"], scene["coverage"][rows]) and torch.equal(obj["vertices"], scene["vertices"][rows])
        # the selection: an id without triangles is absent, part 32 comes only when asked for
        some = model.extract_object_meshes(instance_ids=[occurring[0], 17, 32], **kw)
        assert sorted(some) == [occurring[0]] + ([32] if 32 in split["parts"] else [])
        for p in some:
            assert torch.equal(some[p]["triangles"], split["parts"][p]["triangles"])
        # the clean-up of every part
        largest = model.extract_object_meshes(part_keep_largest=1, **kw)
        assert sorted(largest) == sorted(objects)
        for p, obj in largest.items():
            ref = rm.mesh_clean(objects[p], keep_largest=1, return_source=True)
            rows = ref["source_vertex"].long()
            for k in ("vertices", "normals", "triangles"):
                assert torch.equal(obj[k], ref[k]), (p, k)
            assert torch.equal(obj["colors"], objects[p]["colors"][rows]) and torch.equal(obj["labels"], objects[p]["labels"][rows])
            assert rm.mesh_components(obj["triangles"], obj["vertices"].shape[0])["counts"].tolist() == [1, 1]
        with pytest.raises(ValueError, match="normals"):
            model.extract_object_meshes(normals=False, **kw)
        with pytest.raises(ValueError, match="instance ids"):
            model.extract_object_meshes(instance_ids=[33], **kw)
    with pytest.raises(RuntimeError, match="no_grad"):
        model.extract_object_meshes(**kw)                                                    # no-grad only, as extract_mesh
