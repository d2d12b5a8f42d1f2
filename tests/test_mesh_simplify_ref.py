"""CPU: the numpy restatement of the mesh simplification (tests/mesh_simplify_ref.py) against values worked out by hand, the properties
its output must have on every fixture, and the fixtures themselves -- they are what they claim to be, so the GPU tests, which demand
equality with this restatement, inherit the cases."""
import numpy as np
import pytest

import mesh_simplify_ref as ms

SHAPE = (24, 24, 24)


def test_hand_built_mesh():
    """Lattice: origin (-1,-1,-1), cells of 2, dims (3,2,1), so key = 2 ix + iy.  Every number below was worked out on paper."""
    v, n, t, lat = ms.hand_mesh()
    r = ms.simplify(v, n, t, *lat)
    assert r["key"].tolist() == [0, 0, 2, 2, 2, 4, 1, 3, -1, 2]
    # vertex 2 = (1.5, -0.75, -0.5): u = (2.5, 0.25, 0.5), s = (1.25, 0.125, 0.25), i = (1, 0, 0), q = (0.25, 0.125, 0.25) x 65536
    assert r["q"][2].tolist() == [16384, 8192, 16384]
    assert r["q"][4].tolist() == [57344, 49152, 57344] and r["q"][9].tolist() == [0, 0, 0] and r["q"][8].tolist() == [0, 0, 0]
    assert r["cls"].tolist() == [ms.KEPT, ms.DUPLICATE, ms.KEPT, ms.DEGENERATE, ms.DUPLICATE, ms.INVALID, ms.DEGENERATE]
    assert r["used"].tolist() == [0, 1, 2, 3, 4] and r["counts"].tolist() == [5, 2]
    assert r["triangles"].tolist() == [[0, 2, 1], [2, 4, 3]]                   # corner order kept: (v0, v2, v6) -> cells (0, 2, 1)
    assert r["vertex_cluster"].tolist() == [0, 0, 2, 2, 2, 4, 1, 3, -1, 2]
    # cell key 2 = (1,0,0): the vertices 2, 3, 4 and the unreferenced 9.  sum s - i = (0.25 + 0.5 + 0.875 + 0, 0.125 + 0.5 + 0.75 + 0,
    # 0.25 + 0.5 + 0.875 + 0) = (1.625, 1.375, 1.625); mean = (0.40625, 0.34375, 0.40625); position = -1 + 2 (i + mean)
    assert r["n"].tolist() == [2, 1, 4, 1, 1]
    assert r["sum_q"][2].tolist() == [106496, 90112, 106496]
    assert r["vertices"][2].tolist() == [1.8125, -0.3125, -0.1875]
    assert r["vertices"][0].tolist() == [-0.125, 0.0, 0.25] and r["vertices"][4].tolist() == [3.5, 0.0, 0.0]
    # its normals (1,0,0) + (0,1,0) + (0,0,1) + (0.5,0.5,0) = (1.5, 1.5, 1) x 2^20, length sqrt(5.5) x 2^20
    assert r["sum_Q"][2].tolist() == [1572864, 1572864, 1048576]
    want = (np.array([1.5, 1.5, 1.0]) / np.sqrt(5.5)).astype(np.float32)
    assert np.array_equal(r["normals"][2].view(np.uint32), want.view(np.uint32))
    assert r["normals"][0].tolist() == [0.0, 0.0, 1.0]
    assert ms.simplify(v, None, t, *lat)["normals"] is None
    ms.check_properties(r, v, t, *lat)


def test_cells_at_the_edges_of_the_definition():
    o, c, d = [0.0, 0.0, 0.0], [0.5, 1.0, 3.0], [4, 2, 1]
    p = np.array([[0.0, 0.0, 0.0], [1.9999999, 1.9999999, 2.9999998],       # first and last cell
                  [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0],           # on the last face: outside, not clamped
                  [-1e-30, 0.0, 0.0],                                          # floor(-tiny) = -1
                  [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0], [-3e38, 0, 0],
                  [0.74999994, 0.99999994, 0.0]], dtype=np.float32)            # q rounds up to 65536 on axis 1
    key, i, q = ms.cells_of(p, o, c, d)
    assert key.tolist() == [0, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, 2]
    assert i[1].tolist() == [3, 1, 0] and i[11].tolist() == [1, 0, 0]
    assert q[11].tolist() == [32768, 65536, 0] and q.min() >= 0 and q.max() <= 65536
    # the normal quantisation: non-finite and absurd components contribute nothing; ties to even
    Q = ms.normal_q(np.array([[1.0, -1.0, 0.0], [np.nan, np.inf, -np.inf], [2047.9999, 2048.0, -2048.0], [1.5 * 2.0 ** -20, 2.5 * 2.0 ** -20, 3e38]], dtype=np.float32))
    assert Q.tolist() == [[1048576, -1048576, 0], [0, 0, 0], [2147483520, 0, 0], [2, 2, 0]]


def test_duplicate_fixture_has_both_orientations():
    v, n, t, lat = ms.duplicate_mesh()
    r = ms.simplify(v, n, t, *lat)
    cls, tk = ms.classify(t, r["key"])
    assert (cls != ms.INVALID).all() and (cls != ms.DEGENERATE).all()
    dup = np.nonzero(cls == ms.DUPLICATE)[0]
    kept = np.nonzero(cls == ms.KEPT)[0]
    assert len(dup) == len(kept) == 18
    same = opposite = 0
    for j in dup:
        first = next(k for k in kept if sorted(tk[k]) == sorted(tk[j]))
        assert first < j
        rotations = [tuple(np.roll(tk[first], s)) for s in range(3)]
        if tuple(tk[j]) in rotations:
            same += 1
        else:
            assert tuple(tk[j][::-1]) in rotations
            opposite += 1
    assert same >= 1 and opposite >= 1, (same, opposite)
    assert np.array_equal(r["triangles"], ms.simplify(v[:16], n[:16], t[:18], *lat)["triangles"])      # sheet A alone gives the same triangles
    assert (r["n"] == 2).all()
    ms.check_properties(r, v, t, *lat)


def test_degenerate_fixture_has_both_collapses():
    v, n, t, lat = ms.degenerate_mesh()
    r = ms.simplify(v, n, t, *lat)
    cls, tk = ms.classify(t, r["key"])
    distinct = np.array([len(set(row)) for row in tk.tolist()])
    assert ((cls == ms.DEGENERATE) == (distinct < 3)).all()
    assert (distinct == 1).sum() >= 1 and (distinct == 2).sum() >= 1 and (distinct == 3).sum() >= 1
    assert r["counts"].tolist() == [12, 10]
    ms.check_properties(r, v, t, *lat)


@pytest.mark.parametrize("name", list(ms.VOLUMES))
def test_properties_on_the_volumes(name):
    m = ms.volume_mesh(name)
    T = len(m["triangles"])
    before = None
    for k in ms.CELLS:
        lat = ms.aligned_lattice(SHAPE, k)
        r = ms.simplify(m["vertices"], m["normals"], m["triangles"], *lat)
        assert (r["cls"] != ms.INVALID).all(), "the lattice covers the mesh"
        assert r["counts"][1] == len(r["triangles"]) == (r["cls"] == ms.KEPT).sum() and r["counts"][0] == len(r["vertices"])
        ms.check_properties(r, m["vertices"], m["triangles"], *lat)
        length = np.linalg.norm(r["normals"].astype(np.float64), axis=1)
        assert (np.abs(length - 1.0) < 1e-6).all()
        assert before is None or r["counts"][1] < before                     # coarser cells, fewer triangles
        before = r["counts"][1]
        if name == "sphere" and k == 2.0:
            assert 0 < r["counts"][1] < T / 2, "the sphere at 2 steps keeps fewer than half of its triangles"


def test_malformed_fixture_holds_every_case():
    m = ms.volume_mesh("sphere")
    v, n, t, lat = ms.malformed(m, SHAPE)
    V = len(v)
    r = ms.simplify(v, n, t, *lat)
    assert ((t < 0) | (t >= V)).any(axis=1).sum() == 4
    finite = np.isfinite(v).all(axis=1)
    assert (~finite).sum() == 2 and (r["key"][~finite] == -1).all()
    assert (finite & (r["key"] == -1)).sum() == 2                            # finite, outside the lattice
    assert (~np.isfinite(n[finite & (r["key"] >= 0)])).any()                 # a non-finite normal on a vertex with a cell
    assert (r["cls"] == ms.INVALID).sum() > 4                                # the bad rows and the triangles of the cell-less vertices
    assert np.isfinite(r["vertices"]).all() and np.isfinite(r["normals"]).all()
    ms.check_properties(r, v, t, *lat)


def test_fine_cells_reproduce_the_input():
    v, n, t, lat = ms.terrain()
    r = ms.simplify(v, n, t, *lat)
    assert (np.bincount(r["key"][r["key"] >= 0]) <= 1).all() and (r["key"] >= 0).all()      # the fixture: one vertex per cell at most
    assert (r["cls"] == ms.INVALID).sum() == 4 and (r["cls"] == ms.KEPT).sum() == len(t) - 4
    ms.check_fine_cells(dict(r, input_normals=n), v, t, lat[1])
    ms.check_properties(r, v, t, *lat)
