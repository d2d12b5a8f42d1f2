"""CPU: the mesh split restatement (tests/mesh_split_ref.py) pinned by hand-worked values -- every output row of a strip of four triangles,
a three-way tie, an invalid triangle with its vertex, a vertex shared by three parts -- and by the properties of the definition on random
meshes: the stable partition, the order of the vertices, the local indices."""
import numpy as np
import pytest

import mesh_split_ref as ms

P = ms.P


def _mesh(V, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.standard_normal((V, 3)).astype(np.float32)


def _offsets(pairs):
    """[P+1] offsets from {part: size}."""
    out = np.zeros(P + 1, dtype=np.int32)
    for p, n in pairs.items():
        out[p + 1:] += n
    return out


def test_strip_of_four_triangles_every_row():
    """Vertices 0..5 with labels [0,0,1,1,255,0] -> parts [0,0,1,1,32,0]; the strip (0,1,2) (1,3,2) (2,3,4) (3,5,4).
    (0,1,2): parts 0,0,1 -> 0.  (1,3,2): 0,1,1 -> 1.  (2,3,4): 1,1,32 -> 1.  (3,5,4): 1,0,32, all different -> the lowest, 0.
    Part 0 has triangles 0 and 3 and the vertices {0,1,2} + {3,5,4} = 0,1,2,3,4,5; part 1 has triangles 1 and 2 and the vertices 1,2,3,4;
    part 32 has no triangle, so vertex 4 is not a member of it although its label says so."""
    vert, nrm = _mesh(6)
    tri = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]], dtype=np.int32)
    lab = np.array([0, 0, 1, 1, 255, 0], dtype=np.uint8)
    assert ms.triangle_parts(tri, lab).tolist() == [0, 1, 1, 0]
    out = ms.split(vert, nrm, tri, lab)
    assert out["counts"].tolist() == [10, 4]
    assert out["source_triangle"].tolist() == [0, 3, 1, 2]
    assert out["source_vertex"].tolist() == [0, 1, 2, 3, 4, 5, 1, 2, 3, 4]
    assert out["triangles"].tolist() == [[0, 1, 2], [3, 5, 4], [0, 2, 1], [1, 2, 3]]
    assert np.array_equal(out["part_triangle_offsets"], _offsets({0: 2, 1: 2}))
    assert np.array_equal(out["part_vertex_offsets"], _offsets({0: 6, 1: 4}))
    assert out["part_triangle_offsets"].tolist()[:3] == [0, 2, 4] and out["part_vertex_offsets"].tolist()[:3] == [0, 6, 10]
    rows = [0, 1, 2, 3, 4, 5, 1, 2, 3, 4]
    assert np.array_equal(out["vertices"].view(np.uint32), vert[rows].view(np.uint32))
    assert np.array_equal(out["normals"].view(np.uint32), nrm[rows].view(np.uint32))
    assert out["vertices"].dtype == np.float32 and out["triangles"].dtype == np.int32 and out["source_vertex"].dtype == np.int32
    assert ms.split(vert, None, tri, lab)["normals"] is None


def test_three_different_labels_go_to_the_lowest_whatever_the_rotation():
    vert, _ = _mesh(3)
    lab = np.array([7, 3, 200], dtype=np.uint8)
    for tri in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]):
        out = ms.split(vert, None, np.array([tri], dtype=np.int32), lab)
        assert ms.triangle_parts([tri], lab).tolist() == [3]
        assert out["part_triangle_offsets"].tolist() == [0] * 4 + [1] * 30 and out["part_vertex_offsets"].tolist() == [0] * 4 + [3] * 30
        assert out["source_vertex"].tolist() == [0, 1, 2] and out["triangles"].tolist() == [tri]
    # two of three: the pair wins although the third is lower; labels 32 and 255 are the same part
    assert ms.triangle_parts([[0, 1, 2]], np.array([9, 9, 2], dtype=np.uint8)).tolist() == [9]
    assert ms.triangle_parts([[0, 1, 2]], np.array([32, 1, 255], dtype=np.uint8)).tolist() == [32]
    assert ms.triangle_parts([[0, 0, 1]], np.array([4, 2], dtype=np.uint8)).tolist() == [4]              # (a,a,b): a's part, twice


def test_invalid_triangle_is_dropped_with_its_vertex():
    """Vertex 3 is used by the invalid triangle alone: it is in no part.  Vertex 4 is used by nothing."""
    vert, nrm = _mesh(5)
    lab = np.array([1, 1, 1, 1, 1], dtype=np.uint8)
    for bad in (5, -1, 2 ** 31 - 1):
        tri = np.array([[0, 1, 2], [1, 3, bad], [2, 1, 0]], dtype=np.int32)
        out = ms.split(vert, nrm, tri, lab)
        assert ms.triangle_parts(tri, lab).tolist() == [1, -1, 1]
        assert out["counts"].tolist() == [3, 2]
        assert out["source_vertex"].tolist() == [0, 1, 2] and out["source_triangle"].tolist() == [0, 2]
        assert out["triangles"].tolist() == [[0, 1, 2], [2, 1, 0]]


def test_vertex_shared_by_three_parts_appears_three_times():
    """A fan about vertex 0 (label 2): (0,1,2) with labels 2,5,5 -> 5; (0,3,4) with 2,9,9 -> 9; (0,5,6) with 2,2,2 -> 2."""
    vert, _ = _mesh(7)
    lab = np.array([2, 5, 5, 9, 9, 2, 2], dtype=np.uint8)
    tri = np.array([[0, 1, 2], [0, 3, 4], [0, 5, 6]], dtype=np.int32)
    out = ms.split(vert, None, tri, lab)
    assert out["source_triangle"].tolist() == [2, 0, 1]
    assert out["source_vertex"].tolist() == [0, 5, 6, 0, 1, 2, 0, 3, 4]
    assert (out["source_vertex"] == 0).sum() == 3
    assert out["triangles"].tolist() == [[0, 1, 2]] * 3
    assert np.array_equal(out["part_vertex_offsets"], _offsets({2: 3, 5: 3, 9: 3}))


def test_empty_inputs():
    vert, nrm = _mesh(4)
    for v, n, t, l in ((vert[:0], nrm[:0], np.zeros((0, 3), np.int32), np.zeros(0, np.uint8)),
                       (vert, nrm, np.zeros((0, 3), np.int32), np.zeros(4, np.uint8)),
                       (vert[:0], None, np.array([[0, 1, 2]], np.int32), np.zeros(0, np.uint8))):
        out = ms.split(v, n, t, l)
        assert out["counts"].tolist() == [0, 0] and out["triangles"].shape == (0, 3) and out["vertices"].shape == (0, 3)
        assert out["part_triangle_offsets"].tolist() == [0] * (P + 1) and out["part_vertex_offsets"].tolist() == [0] * (P + 1)


@pytest.mark.parametrize("V,T,seed", [(1, 5, 0), (7, 40, 1), (64, 200, 2), (300, 1500, 3), (1025, 700, 4)])
def test_properties_on_random_meshes(V, T, seed):
    vert, nrm = _mesh(V, seed)
    tri, lab = ms.soup(V, T, seed)
    out = ms.split(vert, nrm, tri, lab)
    part = ms.triangle_parts(tri, lab)
    toff, voff = out["part_triangle_offsets"], out["part_vertex_offsets"]
    assert toff[0] == 0 and voff[0] == 0 and (np.diff(toff) >= 0).all() and (np.diff(voff) >= 0).all()
    assert [int(voff[P]), int(toff[P])] == out["counts"].tolist() == [len(out["source_vertex"]), len(out["source_triangle"])]
    # mapped back through source_vertex, the parts in order are the stable sort of the valid input triangles by part
    back = []
    for p in range(P):
        t = out["triangles"][toff[p]:toff[p + 1]]
        nv = voff[p + 1] - voff[p]
        assert t.size == 0 or (t.min() >= 0 and t.max() < nv), p
        src = out["source_vertex"][voff[p]:voff[p + 1]]
        assert (np.diff(src) > 0).all(), p                                               # strictly increasing inside a part
        assert (nv == 0) == (toff[p + 1] == toff[p])
        if t.size:
            assert set(src.tolist()) == set(tri[part == p].reshape(-1).tolist()), p      # the members, no more and no fewer
            back.append(src[t])
    valid = np.flatnonzero(part >= 0)
    order = valid[np.argsort(part[valid], kind="stable")]
    assert np.array_equal(out["source_triangle"], order)
    assert np.array_equal(np.concatenate(back) if back else np.zeros((0, 3), np.int32), tri[order])
    assert np.array_equal(out["vertices"].view(np.uint32), vert[out["source_vertex"]].view(np.uint32))
    assert np.array_equal(out["normals"].view(np.uint32), nrm[out["source_vertex"]].view(np.uint32))
    if T >= 8:
        assert (part < 0).sum() >= 4 and len(set(part[part >= 0].tolist())) > 1
