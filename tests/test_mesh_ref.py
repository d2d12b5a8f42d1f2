"""CPU: the marching-tetrahedra restatement (tests/mesh_ref.py) checked by topology -- there is no reference mesh anywhere."""
import functools

import numpy as np

import mesh_ref as mr


@functools.lru_cache(maxsize=None)
def _sphere17():
    return mr.isosurface(mr.sphere_volume(17, (8.13, 7.92, 8.30), 5.92), 0.0)


def _closed_and_oriented(mesh):
    """Every undirected edge in exactly two triangles; every directed edge once, with its reverse present."""
    d, u = mr.edge_census(mesh["triangles"])
    assert set(u.values()) == {2}
    assert set(d.values()) == {1}
    assert all((b, a) in d for a, b in d)


def test_table_has_every_case_and_is_oriented():
    assert len(mr.TABLE) == 6 and all(len(row) == 16 for row in mr.TABLE)
    assert mr.PERMUTATIONS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    for row in mr.TABLE:
        assert [len(c) for c in row] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def test_sphere_is_a_closed_oriented_sphere():
    m = _sphere17()
    V, T = len(m["vertices"]), len(m["triangles"])
    print(f"sphere n=17: V={V} T={T}")
    _closed_and_oriented(m)
    assert mr.euler_characteristic(V, m["triangles"]) == 2
    assert mr.signed_volume(m["vertices"], m["triangles"]) > 0
    assert (V, T) == (1950, 3896)
    assert m["triangles"].min() >= 0 and m["triangles"].max() < V


def test_torus_has_genus_one():
    m = mr.isosurface(mr.torus_volume(17, 8.1, 4.7, 2.1), 0.0)
    V, T = len(m["vertices"]), len(m["triangles"])
    print(f"torus n=17: V={V} T={T}")
    _closed_and_oriented(m)
    assert mr.euler_characteristic(V, m["triangles"]) == 0
    assert mr.signed_volume(m["vertices"], m["triangles"]) > 0
    assert (V, T) == (1688, 3376)


def test_values_equal_to_iso_give_degenerate_triangles_and_a_manifold():
    """Radius exactly 3 about a lattice vertex: six lattice values equal iso (outside), mesh vertices sit on lattice vertices."""
    f = mr.sphere_volume(9, (4.0, 4.0, 4.0), 3.0)
    assert int((f == 0).sum()) >= 6
    m = mr.isosurface(f, 0.0)
    v, t = m["vertices"].astype(np.float64), m["triangles"]
    area = np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)
    assert (area == 0).any(), "the case must have zero-area triangles"
    _closed_and_oriented(m)
    assert mr.euler_characteristic(len(v), t) == 2


def test_noise_is_a_manifold_with_boundary_on_the_box_only():
    shape = (7, 6, 5)
    m = mr.isosurface(mr.noise_volume(shape, 3), 0.0)
    d, u = mr.edge_census(m["triangles"])
    assert set(d.values()) == {1}, "no directed edge twice"
    assert max(u.values()) <= 2
    hi = np.array(shape, dtype=np.float32) - 1
    on_box = ((m["vertices"] == 0) | (m["vertices"] == hi[None, :])).any(axis=1)
    lone = [e for e in d if (e[1], e[0]) not in d]
    assert lone, "the noise surface must leave the box"
    for a, b in lone:
        assert on_box[a] and on_box[b]


def test_nonfinite_values_and_ties_follow_the_inside_rule():
    f = np.array([np.nan, np.inf, -np.inf, 0.25, 0.5], dtype=np.float32)
    assert mr.inside_of(f, 0.25).tolist() == [False, True, False, False, True]
    m = mr.isosurface(mr.special_volume((6, 5, 7), 11, 0.25), 0.25)
    assert np.isfinite(m["vertices"]).all() and np.isfinite(m["normals"]).all()
    assert ((m["t"] >= 0) & (m["t"] <= 1)).all()
    d, _ = mr.edge_census(m["triangles"])
    assert set(d.values()) == {1}


def test_volume_converges_from_below():
    """The mesh is inscribed where the field is concave along the edges: below the analytic volume, closer at the finer lattice."""
    rel = []
    for n, s in ((9, 0.5), (17, 1.0)):
        c = np.array((8.13, 7.92, 8.30)) * s
        m = mr.isosurface(mr.sphere_volume(n, c, 5.92 * s), 0.0)
        vol, exact = mr.signed_volume(m["vertices"], m["triangles"]), 4.0 / 3.0 * np.pi * (5.92 * s) ** 3
        print(f"n={n}: volume {vol:.1f} of {exact:.1f}")
        assert 0 < vol < exact
        rel.append((exact - vol) / exact)
    assert rel[1] < rel[0]


def test_origin_and_step_place_the_vertices():
    f = mr.sphere_volume(9, (4.2, 3.9, 4.1), 2.7)
    a = mr.isosurface(f, 0.0)
    b = mr.isosurface(f, 0.0, origin=(-1.0, 0.5, 2.0), step=(0.25, 0.5, 2.0))      # powers of two: exact
    assert np.array_equal(a["triangles"], b["triangles"])
    assert np.array_equal(b["vertices"], a["vertices"] * np.float32([0.25, 0.5, 2.0]) + np.float32([-1.0, 0.5, 2.0]))


def test_fp32_normals_keep_the_derived_bound_and_point_outwards():
    f = mr.sphere_volume(17, (8.13, 7.92, 8.30), 5.92)
    m = _sphere17()
    ref = mr.normals_ref64(f, 0.0, (1.0, 1.0, 1.0), m)
    assert np.isfinite(ref["tol"]).all() and ref["tol"].max() < 1e-4
    assert (np.abs(m["normals"].astype(np.float64) - ref["normals"]) <= ref["tol"]).all()
    radial = m["vertices"].astype(np.float64) - np.array((8.13, 7.92, 8.30))
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert ((ref["normals"] * radial).sum(1) > 0.9).all()
