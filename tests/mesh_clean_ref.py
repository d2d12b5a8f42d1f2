"""Mesh clean-up restated: connected components of an indexed triangle mesh, their statistics, the selection by triangle count and by
key, and the filtered mesh -- numpy, as include/sanerf_hip.h defines the entries of csrc/mesh_clean.hip.

Definition (the header has the same text).  triangles [T,3] int32 over V vertices; any indexed mesh.
  valid       a triangle is valid iff its three indices are in [0, V).  An invalid one connects nothing, is counted nowhere and is never
              emitted.  (a,a,b) and (a,a,a) are valid; duplicates are valid and each counts.
  component   two vertices are connected iff some valid triangle contains both, closed transitively.  label[v] = the smallest vertex index
              of v's component.  A vertex in no valid triangle is its own component with 0 triangles.
  statistics  [V] arrays, nonzero only at roots (label[r] == r): triangle_counts[r] = valid triangles of r's component, vertex_counts[r] =
              its vertices; counts = {roots, roots with at least one triangle}.
  key         key[r] = triangle_counts[r] << 32 | (0xFFFFFFFF - r): unique; larger = more triangles, then the lower root.
  selection   a component is kept iff triangle_counts[r] >= max(min_triangles, 1) and key[r] >= min_key; "keep the largest k" sets min_key
              to the k-th largest key (k beyond the number of components with triangles keeps them all); min_key 0 keeps everything.
  filter      kept vertices keep their relative order and so do kept triangles (valid, and in a kept component); the new index of a vertex
              is its rank among the kept ones; vertex and normal rows are copied bit for bit; source_vertex = the old index of each.

model_rounds() runs the device's round synchronously -- hook from a snapshot, then jump to the fixed point -- and counts the rounds until
one changes nothing (that one included)."""
import numpy as np

import mesh_ref as mr


def valid_triangles(triangles, V):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < V)).all(axis=1)


def _round(lab, tri):
    """One synchronous round: for every valid triangle m = min of its corners' labels, then labels[x] and labels[labels[x]] are lowered to m
    for every corner x (all from the snapshot `lab`); then every vertex jumps to the end of its chain."""
    new = lab.copy()
    if len(tri):
        lt = lab[tri]                                   # [Tv,3]
        m = np.repeat(lt.min(axis=1), 3)
        np.minimum.at(new, tri.reshape(-1), m)
        np.minimum.at(new, lt.reshape(-1), m)
    while True:
        nxt = new[new]
        if np.array_equal(nxt, new):
            return new
        new = nxt


def _propagate(triangles, V):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    tri = t[valid_triangles(t, V)]
    lab = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        new = _round(lab, tri)
        rounds += 1
        if np.array_equal(new, lab):
            return lab, rounds
        lab = new


def components(triangles, V):
    """labels [V] int32."""
    return _propagate(triangles, V)[0].astype(np.int32)


def model_rounds(triangles, V):
    return _propagate(triangles, V)[1]


def pure_propagation_rounds(triangles, V):
    """Rounds of plain min-propagation (every vertex takes the smallest label of its triangles' corners; no hooking of labels, no jumps),
    the confirming round included: the graph's diameter, what the hook-and-jump round is there to avoid."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    tri = t[valid_triangles(t, V)]
    lab = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        new = lab.copy()
        if len(tri):
            np.minimum.at(new, tri.reshape(-1), np.repeat(lab[tri].min(axis=1), 3))
        rounds += 1
        if np.array_equal(new, lab):
            return rounds
        lab = new


def stats(triangles, V, labels):
    """-> dict(triangle_counts [V] int32, vertex_counts [V] int32, counts [2] int32)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    lab = np.asarray(labels, dtype=np.int64)
    tri = t[valid_triangles(t, V)]
    tc = np.bincount(lab[tri[:, 0]], minlength=V).astype(np.int32)
    vc = np.bincount(lab, minlength=V).astype(np.int32)
    roots = lab == np.arange(V)
    return dict(triangle_counts=tc, vertex_counts=vc, counts=np.array([roots.sum(), (roots & (tc > 0)).sum()], dtype=np.int32))


def keys(triangle_counts):
    tc = np.asarray(triangle_counts).astype(np.uint64)
    return (tc << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(len(tc), dtype=np.uint64))


def select(labels, triangle_counts, min_triangles=0, keep_largest=0):
    """-> (keep [V] bool, true at the kept roots only; min_key as a Python int)."""
    lab = np.asarray(labels, dtype=np.int64)
    tc = np.asarray(triangle_counts, dtype=np.int64)
    roots = lab == np.arange(len(lab))
    k = keys(tc)
    min_key = 0
    if keep_largest > 0:
        with_triangles = np.sort(k[roots & (tc > 0)])[::-1]
        if len(with_triangles) >= keep_largest:
            min_key = int(with_triangles[keep_largest - 1])
    keep = roots & (tc >= max(int(min_triangles), 1)) & (k >= np.uint64(min_key))
    return keep, min_key


def filter(vertices, normals, triangles, labels, keep):
    """-> dict(vertices, normals or None, triangles int32, source_vertex int32)."""
    V = len(labels)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    keep_vertex = np.asarray(keep)[np.asarray(labels, dtype=np.int64)] if V else np.zeros(0, dtype=bool)
    new_index = np.cumsum(keep_vertex) - 1
    valid = valid_triangles(t, V)
    kept_t = valid.copy()
    kept_t[valid] = keep_vertex[t[valid, 0]]
    source = np.nonzero(keep_vertex)[0].astype(np.int32)
    return dict(vertices=np.asarray(vertices)[source], normals=None if normals is None else np.asarray(normals)[source],
                triangles=new_index[t[kept_t]].astype(np.int32).reshape(-1, 3), source_vertex=source)


def clean(mesh, min_triangles=0, keep_largest=0):
    """The whole chain on a dict of isosurface()'s keys."""
    V = len(mesh["vertices"])
    lab = components(mesh["triangles"], V)
    st = stats(mesh["triangles"], V, lab)
    keep, _ = select(lab, st["triangle_counts"], min_triangles, keep_largest)
    return filter(mesh["vertices"], mesh["normals"], mesh["triangles"], lab, keep)


# ---- the volumes of the tests ---------------------------------------------------------------------------------------------------------
def two_spheres_speck(n=24):
    """Two separate spheres and one inside lattice vertex far from both: three closed components."""
    f = np.maximum(mr.sphere_volume(n, (7.13, 7.92, 8.30), 4.9).astype(np.float64), mr.sphere_volume(n, (16.4, 15.7, 14.9), 3.6).astype(np.float64))
    f[2, 20, 3] = 0.4
    return f.astype(np.float32)


def serpentine(n=20, nz=9, r=1.3):
    """A tube of radius r about a boustrophedon polyline in the plane z = nz // 2 + 0.13: rows y = 2.1, 6.1, 10.1, 14.1 from x = 2.2 to
    x = n - 3.2, joined alternately at the x ends.  One component whose graph diameter is the tube's length.  f = r - distance in fp64, then
    fp32."""
    x0, x1, zc = 2.2, n - 3.2, nz // 2 + 0.13
    pts = []
    for i, y in enumerate((2.1, 6.1, 10.1, 14.1)):
        pts += [(x0, y), (x1, y)] if i % 2 == 0 else [(x1, y), (x0, y)]
    x, y, z = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), np.arange(nz, dtype=np.float64), indexing="ij")
    p = np.stack([x, y, z], axis=-1)
    dist = np.full(x.shape, np.inf)
    for (ax, ay), (bx, by) in zip(pts[:-1], pts[1:]):
        a, b = np.array([ax, ay, zc]), np.array([bx, by, zc])
        ab = b - a
        s = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
        dist = np.minimum(dist, np.linalg.norm(p - (a + s[..., None] * ab), axis=-1))
    return (r - dist).astype(np.float32)


ISO_SPECIAL = 0.25
FIXTURES = {
    # name: (volume, iso)
    "two_spheres_speck": (two_spheres_speck, 0.0),
    "serpentine": (serpentine, 0.0),
    "torus17": (lambda: mr.torus_volume(17, 8.1, 4.7, 2.1), 0.0),
    "noise_multi": (lambda: mr.noise_volume((33, 18, 70), 5), 0.0),
    "noise_sparse": (lambda: mr.noise_volume((33, 18, 70), 5), 1.2),
    "special": (lambda: mr.special_volume((9, 11, 70), 11, ISO_SPECIAL), ISO_SPECIAL),
    "open_patches": (lambda: mr.sphere_volume(9, (4.0, 4.0, 4.0), 6.0), 0.0),
}

_cache = {}


def fixture(name):
    """-> dict(volume, iso, mesh = mesh_ref.isosurface(volume, iso), labels, triangle_counts, vertex_counts, counts); computed once."""
    if name not in _cache:
        make, iso = FIXTURES[name]
        vol = make()
        mesh = mr.isosurface(vol, iso)
        V = len(mesh["vertices"])
        lab = components(mesh["triangles"], V)
        _cache[name] = dict(volume=vol, iso=iso, mesh=mesh, labels=lab, **stats(mesh["triangles"], V, lab))
    return _cache[name]


def soup(V, T, seed):
    """Random triangles over V vertices with everything the definition names: a third of the vertices unreferenced, duplicated rows,
    (a,a,b) and (a,a,a) rows, and rows that hold -1, V and 2^31 - 1."""
    rng = np.random.default_rng(seed)
    used = np.sort(rng.permutation(V)[: max(V - V // 3, 1)])
    t = used[rng.integers(0, len(used), size=(T, 3))].astype(np.int64)
    if T >= 12:
        t[1] = t[0]                                      # a duplicate
        t[2, 1] = t[2, 0]                                # (a,a,b)
        t[3, :] = t[3, 0]                                # (a,a,a)
        t[4, 0], t[5, 1], t[6, 2] = -1, V, 2 ** 31 - 1
        t[7] = (-1, V, 2 ** 31 - 1)
        t[T - 1, 2] = V
    return t.astype(np.int32)
