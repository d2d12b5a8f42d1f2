"""Mesh simplification restated: uniform vertex clustering of an indexed triangle mesh -- numpy, as include/sanerf_hip.h defines the
entries of csrc/mesh_simplify.hip.  Every quantity is an integer or the correctly rounded result of the stated operations, so the device
has to EQUAL this file: triangles, cluster map and counts exactly, vertices and normals bit for bit.  No tolerance appears anywhere.

Definition (the header has the same text).  vertices [V,3] fp32, normals [V,3] fp32 or None, triangles [T,3] int32; a lattice of cells
origin[3], cell[3] (fp32, cell > 0), dims[3] (each >= 1, product < 2^31).
  cell        per axis u = p - origin and s = u / cell in fp32 (two roundings), i = floor(s).  A vertex with a non-finite coordinate or with
              some i outside [0, dims[a]) has NO cell (nothing is clamped).  key = (ix dims[1] + iy) dims[2] + iz; -1 without a cell.
  offset      q = rint((s - i) 65536) in [0, 65536]: the subtraction and the product are exact in fp32.
  classes     invalid: an index outside [0, V) or a corner without a cell.  degenerate: valid, two corners share a cell.  duplicate: valid,
              not degenerate, and a triangle of LOWER index is valid, not degenerate and has the same SET of three keys.  kept: the rest,
              in their order, corner order unchanged.
  vertices    a cell is used iff it is a corner of a kept triangle; output vertex j = the j-th used cell by key.  Position per axis in fp64,
              every operation rounded on its own, then one rounding to fp32: origin + cell (i + (sum_q / n) / 65536), the sums over ALL
              input vertices of the cell.
  normals     Q = rint(n_a 2^20) (fp32 product) where that is finite and below 2^31 in magnitude, else 0; S = sum Q (int64) over the cell;
              S / sqrt((Sx Sx + Sy Sy) + Sz Sz) in fp64, one rounding to fp32; (0,0,0) when S is zero.
  cluster     vertex_cluster[v] = the output index of v's cell, -1 without a cell or in an unused one."""
import numpy as np

import mesh_ref as mr

INVALID, DEGENERATE, DUPLICATE, KEPT = 0, 1, 2, 3


def lattice(origin, cell, dims):
    cell = [cell] * 3 if np.isscalar(cell) else cell
    return np.asarray(origin, dtype=np.float32), np.asarray(cell, dtype=np.float32), np.asarray(dims, dtype=np.int64)


def cells_of(vertices, origin, cell, dims):
    """-> (key [V] int64, -1 without a cell; i [V,3] int64; q [V,3] int64): i and q are 0 where the vertex has no cell."""
    o, c, d = lattice(origin, cell, dims)
    p = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = p - o                                          # fp32
        s = u / c                                          # fp32, IEEE
        f = np.floor(s)
        ok = ((f >= 0) & (f < d.astype(np.float64))).all(axis=1)          # NaN and the infinities compare false
        frac = np.where(ok[:, None], s - f, np.float32(0))                 # exact
        q = np.rint(frac * np.float32(65536.0)).astype(np.int64)          # exact product; ties to even
    i = np.where(ok[:, None], f, np.float32(0)).astype(np.int64)
    key = np.where(ok, (i[:, 0] * d[1] + i[:, 1]) * d[2] + i[:, 2], -1)
    return key, i, q


def classify(triangles, key):
    """-> (cls [T] of INVALID / DEGENERATE / DUPLICATE / KEPT, tk [T,3] the corners' keys (-1 where the index is out of range))."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = len(key)
    in_range = (t >= 0) & (t < V)
    tk = np.where(in_range, key[np.where(in_range, t, 0)] if V else -1, -1)
    cls = np.full(len(t), INVALID)
    valid = in_range.all(axis=1) & (tk >= 0).all(axis=1)
    degenerate = valid & ((tk[:, 0] == tk[:, 1]) | (tk[:, 1] == tk[:, 2]) | (tk[:, 0] == tk[:, 2]))
    cls[degenerate] = DEGENERATE
    live = np.nonzero(valid & ~degenerate)[0]
    cls[live] = DUPLICATE
    if len(live):
        _, first = np.unique(np.sort(tk[live], axis=1), axis=0, return_index=True)      # the first = the lowest index of each key set
        cls[live[first]] = KEPT
    return cls, tk


def normal_q(normals):
    n = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p = n * np.float32(1048576.0)                      # fp32
        good = np.abs(p) < np.float32(2147483648.0)        # NaN compares false
        return np.rint(np.where(good, p, np.float32(0))).astype(np.int64)


def simplify(vertices, normals, triangles, origin, cell, dims):
    """-> dict(vertices [V',3] f32, normals [V',3] f32 or None, triangles [T',3] int32, vertex_cluster [V] int32, counts [2], and for the
    tests: key, q, cls, used (the used cells' keys, ascending), n, sum_q, sum_Q)."""
    o, c, d = lattice(origin, cell, dims)
    key, _, q = cells_of(vertices, o, c, d)
    cls, tk = classify(triangles, key)
    kept = cls == KEPT
    used = np.unique(tk[kept])                             # ascending
    in_used = (key >= 0) & np.isin(key, used)
    row = np.searchsorted(used, np.where(in_used, key, 0))
    cluster = np.where(in_used, row, -1).astype(np.int32)
    nrow = len(used)
    n = np.bincount(row[in_used], minlength=nrow).astype(np.uint64)
    sum_q = np.zeros((nrow, 3), dtype=np.uint64)
    np.add.at(sum_q, row[in_used], q[in_used].astype(np.uint64))
    iz, iy, ix = used % d[2], (used // d[2]) % d[1], used // (d[1] * d[2])
    i = np.stack([ix, iy, iz], axis=1).astype(np.float64)
    mean = (sum_q.astype(np.float64) / n.astype(np.float64)[:, None]) / 65536.0
    pos = (o.astype(np.float64) + c.astype(np.float64) * (i + mean)).astype(np.float32)
    out_n, sum_Q = None, None
    if normals is not None:
        sum_Q = np.zeros((nrow, 3), dtype=np.int64)
        np.add.at(sum_Q, row[in_used], normal_q(normals)[in_used])
        S = sum_Q.astype(np.float64)                       # one rounding (|S| can pass 2^53)
        with np.errstate(all="ignore"):
            length = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
            out_n = np.where((sum_Q == 0).all(axis=1)[:, None], 0.0, S / length[:, None]).astype(np.float32)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    tri = np.searchsorted(used, tk[kept]).astype(np.int32).reshape(-1, 3)
    assert len(t) == len(cls)
    return dict(vertices=pos.reshape(-1, 3), normals=out_n, triangles=tri, vertex_cluster=cluster,
                counts=np.array([nrow, int(kept.sum())], dtype=np.int64), key=key, q=q, cls=cls, used=used, n=n, sum_q=sum_q, sum_Q=sum_Q)


# ---- the lattices and meshes of the tests ---------------------------------------------------------------------------------------------
def aligned_lattice(shape, k, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0)):
    """The cell lattice NeRFRenderer.extract_mesh(simplify=k) uses for an extraction lattice of `shape` vertices: cell = k step (rounded once to fp32),
    origin = lattice origin - step / 2 (fp32), dims = the cells that cover the vertices 0 .. shape - 1.  -> (origin, cell, dims)."""
    o = np.asarray(origin, dtype=np.float32) - np.float32(0.5) * np.asarray(step, dtype=np.float32)
    c = np.asarray([float(k) * float(np.float32(x)) for x in step], dtype=np.float32)       # the product in fp64, rounded once
    dims = [int(np.floor((n - 0.5) / float(k))) + 2 for n in shape]
    return [float(x) for x in o], [float(x) for x in c], dims


def two_blobs(n=24):
    """Two overlapping spheres of different size: one closed surface with a concave seam."""
    return np.maximum(mr.sphere_volume(n, (8.2, 9.1, 10.3), 5.3).astype(np.float64), mr.sphere_volume(n, (14.6, 13.2, 12.4), 4.4).astype(np.float64)).astype(np.float32)


VOLUMES = {"sphere": lambda: mr.sphere_volume(24, (11.3, 12.1, 10.7), 7.6), "two_blobs": two_blobs}
CELLS = (1.0, 2.0, 2.5, 3.0)
_cache = {}


def volume_mesh(name):
    """mesh_ref.isosurface of the named 24^3 volume at iso 0 (unit lattice at the origin); computed once, never modified."""
    if name not in _cache:
        _cache[name] = mr.isosurface(VOLUMES[name](), 0.0)
    return _cache[name]


def _flat_normals(V):
    return np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), (V, 1))


def hand_mesh():
    """Ten vertices over a 3 x 2 x 1 lattice of 2-wide cells at origin (-1, -1, -1), values that fp32 holds exactly.
    -> (vertices, normals, triangles, (origin, cell, dims)).  Cell (1,0,0) -- key (1 x 2 + 0) x 1 + 0 = 2 -- holds the vertices 2, 3, 4 and 9 (9 is in no
    triangle); vertex 8 lies outside the lattice."""
    v = np.array([[-0.5, -0.5, 0.0],       # 0: cell (0,0,0) key 0
                  [0.25, 0.5, 0.5],        # 1: cell (0,0,0) key 0
                  [1.5, -0.75, -0.5],      # 2: cell (1,0,0) key 2     s = (1.25, 0.125, 0.25)
                  [2.0, 0.0, 0.0],         # 3: cell (1,0,0) key 2     s = (1.5, 0.5, 0.5)
                  [2.75, 0.5, 0.75],       # 4: cell (1,0,0) key 2     s = (1.875, 0.75, 0.875)
                  [3.5, 0.0, 0.0],         # 5: cell (2,0,0) key 4
                  [0.0, 1.5, 0.0],         # 6: cell (0,1,0) key 1
                  [2.0, 2.5, 0.5],         # 7: cell (1,1,0) key 3
                  [5.5, 0.0, 0.0],         # 8: s_x = 3.25 -> outside dims[0] = 3: no cell
                  [1.0, -1.0, -1.0]],      # 9: cell (1,0,0) key 2     s = (1.0, 0.0, 0.0); referenced by no triangle
                 dtype=np.float32)
    n = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0.5, 0.5, 0]], dtype=np.float32)
    t = np.array([[0, 2, 6],               # keys {0,2,1}: kept
                  [1, 3, 6],               # keys {0,2,1} again: duplicate, equal orientation
                  [2, 5, 7],               # keys {2,4,3}: kept
                  [0, 1, 5],               # two corners in cell 0: degenerate
                  [4, 7, 5],               # keys {2,3,4}: duplicate of triangle 2, opposite orientation
                  [5, 8, 7],               # vertex 8 has no cell: invalid
                  [2, 3, 4]],              # all in cell 2: degenerate
                 dtype=np.int32)
    return v, n, t, ([-1.0, -1.0, -1.0], [2.0, 2.0, 2.0], [3, 2, 1])


def duplicate_mesh():
    """Two sheets over one 4 x 4 x 1 lattice of unit cells: every cell of the 4 x 4 grid holds a vertex of sheet A and one of sheet B
    (B a little higher, inside the same cell), and both sheets are triangulated alike -- B's lower triangles with the same orientation as
    A's, B's upper triangles reversed.  Every triangle of B is a duplicate.  -> (vertices, normals, triangles, lattice)."""
    g = 4
    xy = np.stack(np.meshgrid(np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)
    a = np.concatenate([xy + np.float32(0.25), np.full((g * g, 1), 0.25, dtype=np.float32)], axis=1)
    b = np.concatenate([xy + np.float32(0.5), np.full((g * g, 1), 0.75, dtype=np.float32)], axis=1)
    lower = [[x * g + y, (x + 1) * g + y, x * g + y + 1] for x in range(g - 1) for y in range(g - 1)]
    upper = [[(x + 1) * g + y, (x + 1) * g + y + 1, x * g + y + 1] for x in range(g - 1) for y in range(g - 1)]
    ta = np.array(lower + upper, dtype=np.int32)
    tb = np.array(lower + [[u[0], u[2], u[1]] for u in upper], dtype=np.int32) + g * g
    v = np.concatenate([a, b])
    return v, _flat_normals(len(v)), np.concatenate([ta, tb]), ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [g, g, 1])


def degenerate_mesh():
    """A strip of 12 x 3 vertices at spacing 0.5 over unit cells: triangles with all three corners in one cell, with two, and with three
    different cells.  -> (vertices, normals, triangles, lattice)."""
    nx, ny = 12, 3
    xy = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)
    v = np.concatenate([xy * np.float32(0.5) + np.float32(0.125), np.full((nx * ny, 1), 0.5, dtype=np.float32)], axis=1)
    t = []
    for x in range(nx - 1):
        for y in range(ny - 1):
            a, b, c, d = x * ny + y, (x + 1) * ny + y, (x + 1) * ny + y + 1, x * ny + y + 1
            t += [[a, b, c], [a, c, d]]
    return v, _flat_normals(len(v)), np.array(t, dtype=np.int32), ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [6, 2, 1])


def malformed(mesh, shape, k=2.0):
    """A copy of an isosurface mesh with everything the definition names: triangle rows holding -1, V and 2^31 - 1, a NaN vertex, an
    infinite one, a vertex outside the lattice, and NaN / infinite / huge normals on finite vertices.
    -> (vertices, normals, triangles, lattice)."""
    v, t = mesh["vertices"].copy(), mesh["triangles"].copy()
    n = mesh["normals"].copy() if mesh["normals"] is not None else _flat_normals(len(v))
    V, T = len(v), len(t)
    t[3, 0], t[T // 3, 1], t[T // 2, 2], t[T - 1] = -1, V, 2 ** 31 - 1, (-1, V, -2 ** 31)
    v[5, 1] = np.nan
    v[V // 4] = (np.inf, 1.0, 1.0)
    v[V // 2, 2] = np.float32(shape[2] + 40.0)             # finite, beyond the last cell
    v[V // 3, 0] = np.float32(-3.0)                        # below the first
    n[7, 0] = np.nan
    n[V // 5] = (np.inf, 0.0, -np.inf)
    n[V // 6, 2] = np.float32(3.0e38)
    n[V // 7, 1] = np.float32(4096.0)                      # finite, but its product is not below 2^31
    return v, n, t, aligned_lattice(shape, k)


def terrain(nx=15, ny=13, seed=3):
    """A height field over nx x ny vertices at unit spacing, each moved by less than 0.2 per axis: no two vertices are closer than 0.6 in x
    or in y, so cells of 0.5 hold one vertex at most.  Four rows of the triangle list hold an index out of range.  Coordinates stay below
    15, where an fp32 ulp is at most 2^-20.  -> (vertices, normals, triangles, lattice)."""
    rng = np.random.default_rng(seed)
    xy = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    xy += rng.uniform(-0.19, 0.19, size=xy.shape)
    z = 3.0 + 2.0 * np.sin(0.7 * xy[:, :1]) * np.cos(0.5 * xy[:, 1:])
    v = np.concatenate([xy, z], axis=1).astype(np.float32)
    n = rng.standard_normal(v.shape).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = []
    for x in range(nx - 1):
        for y in range(ny - 1):
            a, b, c, d = x * ny + y, (x + 1) * ny + y, (x + 1) * ny + y + 1, x * ny + y + 1
            t += [[a, b, c], [a, c, d]]
    t = np.array(t, dtype=np.int32)
    t[0, 0], t[7, 1], t[100, 2], t[len(t) - 1, 0] = -1, len(v), 2 ** 31 - 1, -5
    return v, n, t, ([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [2 * nx + 2, 2 * ny + 2, 16])


def check_fine_cells(out, vertices, triangles, cell):
    """With at most one vertex per cell: T' = the number of valid triangles, the triangles are the input's under the cluster map, and every
    position is the input's within cell / 65536 per axis plus one fp32 ulp of the coordinate -- the definition's own quantisation step.
    (Why it has to hold here: rint moves q by at most half a step, cell / 131072; the roundings of u, of s and of the result add at most
    1.5 ulp of the largest coordinate, 2^-20 in this fixture, which the other half step, 2^-18 at cell = 0.5, covers.)"""
    V = len(vertices)
    t = np.asarray(triangles, dtype=np.int64)
    valid = ((t >= 0) & (t < V)).all(axis=1)
    cl = out["vertex_cluster"].astype(np.int64)
    assert len(out["triangles"]) == valid.sum()
    assert np.array_equal(out["triangles"], cl[t[valid]])
    ref = cl >= 0
    assert np.array_equal(np.sort(cl[ref]), np.arange(len(out["vertices"])))        # one vertex per cluster
    got = out["vertices"][cl[ref]].astype(np.float64)
    src = np.asarray(vertices)[ref]
    bound = np.asarray(cell, dtype=np.float64) / 65536.0 + np.spacing(np.abs(src)).astype(np.float64)
    assert (np.abs(got - src.astype(np.float64)) <= bound).all()
    if out.get("normals") is not None:                                               # a single unit normal survives to 2^-20 per component
        assert (np.abs(out["normals"][cl[ref]].astype(np.float64) - np.asarray(out["input_normals"])[ref]) <= 2.0 ** -19).all()


# ---- properties that need no restatement ----------------------------------------------------------------------------------------------
def check_properties(out, vertices, triangles, origin, cell, dims):
    """Asserts on a result `out` (dict of numpy arrays: vertices, triangles, vertex_cluster) of the input (vertices, triangles)."""
    o, c, d = lattice(origin, cell, dims)
    ov, ot, cl = out["vertices"], out["triangles"].astype(np.int64), out["vertex_cluster"].astype(np.int64)
    nv = len(ov)
    assert ((ot >= 0) & (ot < nv)).all()
    assert (ot[:, 0] != ot[:, 1]).all() and (ot[:, 1] != ot[:, 2]).all() and (ot[:, 0] != ot[:, 2]).all()
    assert len(np.unique(np.sort(ot, axis=1), axis=0)) == len(ot)                      # no two triangles share a vertex set
    assert np.array_equal(np.unique(ot), np.arange(nv))                                # every output vertex is referenced
    key, i, _ = cells_of(vertices, o, c, d)
    members = cl >= 0
    assert (key[members] >= 0).all()
    if nv:
        assert np.array_equal(np.unique(cl[members]), np.arange(nv))
        cell_of_cluster = np.full(nv, -1)
        cell_of_cluster[cl[members]] = key[members]
        assert np.array_equal(cell_of_cluster[cl[members]], key[members])              # one cluster, one cell
        assert (np.diff(cell_of_cluster) > 0).all()                                    # in key order
        # inside the cell's box: exact in fp64 up to the final rounding to fp32, one ulp of the coordinate
        first = np.zeros(nv, dtype=np.int64)
        first[cl[members][::-1]] = np.nonzero(members)[0][::-1]
        lo = o.astype(np.float64) + c.astype(np.float64) * i[first]
        hi = lo + c.astype(np.float64)
        ulp = np.spacing(np.abs(ov)).astype(np.float64)
        assert (ov >= lo - ulp).all() and (ov <= hi + ulp).all()
