"""CPU: the mesh clean-up restatement (tests/mesh_clean_ref.py) pinned by topology, as tests/test_mesh_ref.py pins the isosurface's: the
components of known shapes, their triangle counts and Euler characteristics, the rounds of the synchronous model, and the filter."""
import numpy as np
import pytest

import mesh_clean_ref as mc
import mesh_ref as mr


def _union_find(triangles, V):
    """A plain union-find of its own (union by smaller root), to check components() against another algorithm."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(triangles, dtype=np.int64).tolist():
        if not (0 <= a < V and 0 <= b < V and 0 <= c < V):
            continue
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    return np.array([find(v) for v in range(V)], dtype=np.int32)


def _sizes(fx):
    tc = fx["triangle_counts"]
    return np.sort(tc[tc > 0])[::-1]


def _component_mesh(fx, root):
    keep = np.zeros(len(fx["labels"]), dtype=bool)
    keep[root] = True
    m = fx["mesh"]
    return mc.filter(m["vertices"], m["normals"], m["triangles"], fx["labels"], keep)


#             fixture             V       T       components  largest triangle counts  model rounds
TABLE = [("two_spheres_speck", 2070, 4128, 3, (2672, 1432, 24), 3),
         ("serpentine", 2606, 5208, 1, (5208,), 4),
         ("torus17", 1688, 3376, 1, (3376,), 3),
         ("noise_multi", 137367, 281530, 19, (281318,), 4),
         ("noise_sparse", 56824, 102778, 1861, (), 4)]


@pytest.mark.parametrize("name,V,T,ncomp,largest,rounds", TABLE)
def test_fixture_table(name, V, T, ncomp, largest, rounds):
    fx = mc.fixture(name)
    m = fx["mesh"]
    assert (len(m["vertices"]), len(m["triangles"])) == (V, T)
    assert fx["counts"].tolist() == [ncomp, ncomp]          # every mesh vertex of an isosurface is in a triangle
    assert tuple(_sizes(fx)[:len(largest)]) == largest
    assert int(fx["triangle_counts"].sum()) == T and int(fx["vertex_counts"].sum()) == V
    assert mc.model_rounds(m["triangles"], V) == rounds
    lab = fx["labels"]
    roots = np.nonzero(lab == np.arange(V))[0]
    assert (lab <= np.arange(V)).all() and (lab[lab] == lab).all()
    assert (fx["triangle_counts"][lab != np.arange(V)] == 0).all() and (fx["vertex_counts"][lab != np.arange(V)] == 0).all()
    assert len(roots) == ncomp
    t = m["triangles"].astype(np.int64)
    assert (lab[t[:, 0]] == lab[t[:, 1]]).all() and (lab[t[:, 0]] == lab[t[:, 2]]).all()


@pytest.mark.parametrize("name", ["two_spheres_speck", "serpentine", "torus17", "noise_sparse", "special", "open_patches"])
def test_components_equal_a_union_find(name):
    fx = mc.fixture(name)
    assert np.array_equal(fx["labels"], _union_find(fx["mesh"]["triangles"], len(fx["labels"])))


def test_component_counts_of_the_remaining_fixtures():
    assert mc.fixture("special")["counts"].tolist() == [29, 29]
    assert mc.fixture("open_patches")["counts"].tolist() == [8, 8]


def test_pure_propagation_needs_the_diameter():
    for name, pure in (("serpentine", 119), ("noise_multi", 148)):
        fx = mc.fixture(name)
        assert mc.pure_propagation_rounds(fx["mesh"]["triangles"], len(fx["labels"])) == pure


@pytest.mark.parametrize("name,chi", [("two_spheres_speck", (2, 2, 2)), ("serpentine", (2,)), ("torus17", (0,))])
def test_one_component_keeps_its_euler_characteristic_and_orientation(name, chi):
    fx = mc.fixture(name)
    roots = np.nonzero(fx["triangle_counts"] > 0)[0]
    assert len(roots) == len(chi)
    for root, want in zip(roots, chi):
        part = _component_mesh(fx, root)
        V, T = len(part["vertices"]), len(part["triangles"])
        assert (V, T) == (fx["vertex_counts"][root], fx["triangle_counts"][root])
        assert mr.euler_characteristic(V, part["triangles"]) == want
        d, u = mr.edge_census(part["triangles"])
        assert set(u.values()) == {2} and set(d.values()) == {1}            # still closed and oriented
        assert mr.signed_volume(part["vertices"], part["triangles"]) > 0
        assert np.array_equal(part["vertices"], fx["mesh"]["vertices"][part["source_vertex"]])
        assert np.array_equal(part["normals"], fx["mesh"]["normals"][part["source_vertex"]])
    assert mr.signed_volume(fx["mesh"]["vertices"], fx["mesh"]["triangles"]) > 0


def test_noise_sparse_selection():
    fx = mc.fixture("noise_sparse")
    m, tc, vc = fx["mesh"], fx["triangle_counts"], fx["vertex_counts"]
    big = tc >= 100
    assert (int(big.sum()), int(vc[big].sum()), int(tc[big].sum())) == (213, 24252, 46894)
    out = mc.clean(m, min_triangles=100)
    assert (len(out["vertices"]), len(out["triangles"])) == (24252, 46894)
    assert out["triangles"].min() == 0 and out["triangles"].max() == 24251
    assert (np.diff(out["source_vertex"]) > 0).all()
    # the 6th and the 7th largest both have 604 triangles: keep_largest = 6 cuts through the tie by root index
    sizes = _sizes(fx)
    assert sizes[5] == sizes[6] == 604 and sizes[4] > 604 > sizes[7]
    tied = np.nonzero(tc == 604)[0]
    assert len(tied) == 2
    keep6, key6 = mc.select(fx["labels"], tc, keep_largest=6)
    assert keep6.sum() == 6 and keep6[tied[0]] and not keep6[tied[1]]
    assert key6 == (604 << 32) | (0xFFFFFFFF - int(tied[0]))
    keep7, _ = mc.select(fx["labels"], tc, keep_largest=7)
    assert keep7.sum() == 7 and keep7[tied[1]]
    both, _ = mc.select(fx["labels"], tc, min_triangles=700, keep_largest=6)
    assert both.sum() == 3
    everything, key = mc.select(fx["labels"], tc, keep_largest=5000)
    assert everything.sum() == 1861 and key == 0
    k = mc.keys(tc)
    assert len(np.unique(k)) == len(k)


def test_soup_follows_the_definition():
    """Invalid rows connect nothing and count nowhere; degenerate and duplicated rows count; unreferenced vertices are their own roots."""
    V = 65
    t = mc.soup(V, 40, 3)
    valid = mc.valid_triangles(t, V)
    assert 0 < (~valid).sum() < len(t) and (t[1] == t[0]).all() and t[2, 0] == t[2, 1] and t[3, 0] == t[3, 1] == t[3, 2]
    lab = mc.components(t, V)
    assert np.array_equal(lab, _union_find(t, V))
    st = mc.stats(t, V, lab)
    assert int(st["triangle_counts"].sum()) == int(valid.sum())
    unreferenced = np.setdiff1d(np.arange(V), t[valid].reshape(-1))
    assert len(unreferenced) >= V // 3 and (lab[unreferenced] == unreferenced).all() and (st["vertex_counts"][unreferenced] == 1).all()
    assert st["counts"][0] > st["counts"][1] > 0
    keep, _ = mc.select(lab, st["triangle_counts"], min_triangles=1)
    out = mc.filter(np.zeros((V, 3), np.float32), None, t, lab, keep)
    assert len(out["triangles"]) == int(valid.sum()) and out["normals"] is None
    assert np.array_equal(out["source_vertex"][out["triangles"]], t[valid])
    # the empty ends
    assert mc.components(np.zeros((0, 3), np.int32), 5).tolist() == [0, 1, 2, 3, 4] and mc.model_rounds(np.zeros((0, 3), np.int32), 5) == 1
    none, _ = mc.select(lab, st["triangle_counts"], min_triangles=10 ** 9)
    assert not none.any()
