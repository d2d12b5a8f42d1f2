"""Marching tetrahedra on a lattice, restated: numpy fp32, operation for operation as include/sanerf_hip.h defines the isosurface
entries (csrc/mesh.hip), and an fp64 statement of the normals with the bound the fp32 ones have to keep.

The reference project has no geometry export to compare with, and no mesh library is assumed: what pins the definition is this file, and
what pins this file is topology (tests/test_mesh_ref.py): a closed surface has every edge in two triangles, once per direction, and the
Euler characteristic of the shape it encloses.

Definition (the header has the same text).  volume [nx,ny,nz] fp32, z fastest; linear index of a lattice vertex (x ny + y) nz + z.
  inside     f > iso in fp32: NaN is outside, +inf inside, a value equal to iso outside.
  edge slots a lattice vertex owns up to 7 edges: slot e goes to the vertex at offset SLOT_OFFSETS[e], where that vertex is in range.
             An edge carries a mesh vertex iff its two ends differ in inside-ness.
  position   t = (iso - f_a) / (f_b - f_a), fp32, IEEE division, a the owning end; !(t >= 0 && t <= 1) -> t = 0.5.
             Per axis pos = origin + ((float)i + t e) step, every operation rounded on its own (e = the offset's 0 or 1).
  order      mesh vertices by owning lattice vertex's linear index, then slot.
  tetrahedra a cell (its lowest corner names it) splits into the six Kuhn paths v0 -> v0 + e_p1 -> + e_p2 -> (1,1,1), the permutations
             p of the axes in lexicographic order.
  triangles  per tetrahedron, corners in path order: one inside corner I: (I,O0),(I,O1),(I,O2); three: (I0,O),(I1,O),(I2,O); two: the
             quad a=(I0,O0) b=(I0,O1) c=(I1,O1) d=(I1,O0) as (a,b,c),(a,c,d).  Each triangle is flipped (its last two vertices swapped)
             so that its normal points from inside to outside -- decided once, in the 6 x 16 table, from the edge mid-points on the unit
             lattice and the centroids of the inside and outside corners; never from run-time positions.
  order      triangles by cell linear index (x (ny-1) + y)(nz-1) + z, then tetrahedron, then triangle.  Zero-area triangles are kept.
  normals    lattice gradient by central differences (f[i+1] - f[i-1]) / (2 step), one-sided (f[i+1] - f[i]) / step at the faces;
             g = g_a + t (g_b - g_a); n = -g / |g|; a zero or non-finite |g| gives (0,0,0).
"""
import itertools

import numpy as np

SLOT_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMUTATIONS = tuple(itertools.permutations(range(3)))            # lexicographic
U = 2.0 ** -24                                                     # unit round-off of fp32


def _corner(axes):
    c = [0, 0, 0]
    for a in axes:
        c[a] = 1
    return tuple(c)


TET_CORNERS = tuple((_corner(()), _corner(p[:1]), _corner(p[:2]), (1, 1, 1)) for p in PERMUTATIONS)


def _oriented(tri, corners, inside):
    """tri: three (p, q) pairs of local corner numbers.  Flip so that the normal of the mid-point triangle points from the inside corners'
    centroid to the outside corners' (integers throughout: twice the mid-points, n_in n_out times the centroid difference)."""
    m = [np.array(corners[p]) + np.array(corners[q]) for p, q in tri]
    n = np.cross(m[1] - m[0], m[2] - m[0])
    ins = [np.array(corners[i]) for i in range(4) if inside[i]]
    outs = [np.array(corners[i]) for i in range(4) if not inside[i]]
    d = sum(outs) * len(ins) - sum(ins) * len(outs)
    dot = int(np.dot(n, d))
    assert dot != 0, (corners, inside, tri)
    return tri if dot > 0 else (tri[0], tri[2], tri[1])


def _build_table():
    """TABLE[k][case] = list of triangles, each three (p, q) pairs of LOCAL corner numbers of tetrahedron k (p inside, q outside);
    case bit i = path corner i is inside."""
    table = []
    for corners in TET_CORNERS:
        row = []
        for case in range(16):
            inside = [(case >> i) & 1 == 1 for i in range(4)]
            I = [i for i in range(4) if inside[i]]
            O = [i for i in range(4) if not inside[i]]
            if len(I) == 1:
                tris = [((I[0], O[0]), (I[0], O[1]), (I[0], O[2]))]
            elif len(I) == 3:
                tris = [((I[0], O[0]), (I[1], O[0]), (I[2], O[0]))]
            elif len(I) == 2:
                a, b, c, d = (I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])
                tris = [(a, b, c), (a, c, d)]
            else:
                tris = []
            row.append([_oriented(t, corners, inside) for t in tris])
        table.append(row)
    return table


TABLE = _build_table()


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def inside_of(volume, iso):
    with np.errstate(invalid="ignore"):
        return _f32(volume) > np.float32(iso)


def isosurface(volume, iso, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), normals=True):
    """-> dict(vertices [V,3] f32, triangles [T,3] i32, normals [V,3] f32 or None, t [V] f32, owner [V] int64 (linear index), slot [V])."""
    f = np.ascontiguousarray(volume, dtype=np.float32)
    nx, ny, nz = f.shape
    iso = np.float32(iso)
    origin, step = _f32(origin), _f32(step)
    ins = inside_of(f, iso)
    idx = np.arange(nx * ny * nz, dtype=np.int64).reshape(nx, ny, nz)
    # ---- edges: mask[v] bit e
    mask = np.zeros((nx, ny, nz), dtype=np.uint8)
    for e, (dx, dy, dz) in enumerate(SLOT_OFFSETS):
        a = ins[:nx - dx, :ny - dy, :nz - dz]
        b = ins[dx:, dy:, dz:]
        mask[:nx - dx, :ny - dy, :nz - dz] |= ((a != b).astype(np.uint8) << e)
    popcount = np.array([bin(m).count("1") for m in range(128)], dtype=np.int64)
    counts = popcount[mask.reshape(-1)]
    base = np.concatenate([[0], np.cumsum(counts)])[:-1]
    # ---- mesh vertices in (owner, slot) order
    own, slot = np.nonzero(((mask.reshape(-1)[:, None] >> np.arange(7)[None, :]) & 1) == 1)      # row-major: owner, then slot
    off = np.array(SLOT_OFFSETS, dtype=np.int64)[slot]                                            # [V,3]
    ia = np.stack(np.unravel_index(own, (nx, ny, nz)), axis=1).astype(np.int64)                   # [V,3]
    ib = ia + off
    fa = f[ia[:, 0], ia[:, 1], ia[:, 2]]
    fb = f[ib[:, 0], ib[:, 1], ib[:, 2]]
    with np.errstate(all="ignore"):
        t = ((iso - fa).astype(np.float32) / (fb - fa).astype(np.float32)).astype(np.float32)
        ok = (t >= 0) & (t <= 1)
    t = np.where(ok, t, np.float32(0.5)).astype(np.float32)
    te = (t[:, None] * off.astype(np.float32)).astype(np.float32)
    s = (ia.astype(np.float32) + te).astype(np.float32)
    vertices = (origin[None, :] + (s * step[None, :]).astype(np.float32)).astype(np.float32)
    # ---- triangles
    def vid(corner_a, corner_b, cells):
        """Mesh-vertex id of the edge between two corners (offsets) of the given cells [n,3]: the owner is the lower end."""
        lo = np.minimum(corner_a, corner_b)
        d = tuple(int(v) for v in (np.maximum(corner_a, corner_b) - lo))
        e = SLOT_OFFSETS.index(d)
        o = cells + lo[None, :]
        lin = (o[:, 0] * ny + o[:, 1]) * nz + o[:, 2]
        m = mask.reshape(-1)[lin].astype(np.int64)
        assert ((m >> e) & 1).all()
        return base[lin] + counts_below(m, e)

    def counts_below(m, e):
        return popcount[m & ((1 << e) - 1)]

    cells = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"), axis=-1).reshape(-1, 3)
    keys, tris = [], []
    for k, corners in enumerate(TET_CORNERS):
        cs = np.array(corners, dtype=np.int64)
        case = np.zeros(len(cells), dtype=np.int64)
        for i in range(4):
            c = cells + cs[i][None, :]
            case |= ins[c[:, 0], c[:, 1], c[:, 2]].astype(np.int64) << i
        for cv in range(1, 15):
            sel = np.nonzero(case == cv)[0]
            if len(sel) == 0:
                continue
            for j, tri in enumerate(TABLE[k][cv]):
                ids = np.stack([vid(cs[p], cs[q], cells[sel]) for p, q in tri], axis=1)
                tris.append(ids)
                keys.append((sel * 6 + k) * 2 + j)
    if tris:
        keys = np.concatenate(keys)
        order = np.argsort(keys, kind="stable")
        triangles = np.concatenate(tris)[order].astype(np.int32)
    else:
        triangles = np.zeros((0, 3), dtype=np.int32)
    out = dict(vertices=vertices, triangles=triangles, normals=None, t=t, owner=own, slot=slot)
    if normals:
        ga, gb = gradient32(f, ia, step), gradient32(f, ib, step)
        with np.errstate(all="ignore"):
            g = (ga + (t[:, None] * (gb - ga).astype(np.float32)).astype(np.float32)).astype(np.float32)
            ln = np.sqrt(((g[:, 0] * g[:, 0]).astype(np.float32) + (g[:, 1] * g[:, 1]).astype(np.float32)).astype(np.float32)
                         + (g[:, 2] * g[:, 2]).astype(np.float32)).astype(np.float32)
            good = np.isfinite(ln) & (ln > 0)
            n = (-g / ln[:, None]).astype(np.float32)
        out["normals"] = np.where(good[:, None], n, np.float32(0)).astype(np.float32)
    return out


def _gradient(f, at, step, dtype):
    """Central differences (f[i+1] - f[i-1]) / (2 step), one-sided (f[i+1] - f[i]) / step or (f[i] - f[i-1]) / step at the faces."""
    g = np.zeros((len(at), 3), dtype=dtype)
    f = f.astype(dtype)
    step = np.asarray(step, dtype=dtype)
    for a in range(3):
        n = f.shape[a]
        hi, lo = at.copy(), at.copy()
        hi[:, a] = np.minimum(at[:, a] + 1, n - 1)
        lo[:, a] = np.maximum(at[:, a] - 1, 0)
        with np.errstate(all="ignore"):
            d = (f[hi[:, 0], hi[:, 1], hi[:, 2]] - f[lo[:, 0], lo[:, 1], lo[:, 2]]).astype(dtype)
            den = np.where((hi[:, a] - lo[:, a]) == 2, (dtype(2) * step[a]).astype(dtype), step[a]).astype(dtype)
            g[:, a] = (d / den).astype(dtype)
    return g


def gradient32(f, at, step):
    return _gradient(f, at, step, np.float32)


def normals_ref64(volume, iso, step, mesh):
    """The normals of a mesh of isosurface() in fp64, from the fp32 volume, and the bound |n32 - n64| <= tol per component.

    With d = a lattice difference, g_a, g_b the end gradients, t the edge parameter and u = 2^-24, every fp32 operation adds a relative
    error u of its own result:
      g_a, g_b      one subtraction and one division (2 step is exact; the division by the fp32 step is one rounding): 2 u |g|
      t             two subtractions and a division: 3 u |t| (the two differences have one sign and |iso - f_a| <= |f_b - f_a|, so fp32
                    and fp64 agree on 0 <= t <= 1 for finite values)
      g             the difference g_b - g_a: u |g_b - g_a| on top of 2 u (|g_a| + |g_b|); the product with t: u more, and 3 u from t;
                    the sum: u |g|.  Per component
                        e = u (2 |g_a| + t (2 |g_a| + 2 |g_b| + 5 |g_b - g_a|) + |g|)
      n = -g / |g|  three squares, two sums, a root and a division: each component of n moves by at most (e_c + |n_c| |e|_2) / |g| from g's
                    error and by 5 u from its own arithmetic.
    So tol_c = (e_c + |n_c| |e|_2) / |g| + 5 u: the ulp of the inputs over the gradient magnitude.  Where |g| is so small that this
    exceeds 2 the bound says nothing (both are unit vectors or zero); the caller sees it in `tol`."""
    f = np.ascontiguousarray(volume, dtype=np.float32)
    nx, ny, nz = f.shape
    own, slot = mesh["owner"], mesh["slot"]
    off = np.array(SLOT_OFFSETS, dtype=np.int64)[slot]
    ia = np.stack(np.unravel_index(own, (nx, ny, nz)), axis=1).astype(np.int64)
    ib = ia + off
    f64 = f.astype(np.float64)
    fa, fb = f64[ia[:, 0], ia[:, 1], ia[:, 2]], f64[ib[:, 0], ib[:, 1], ib[:, 2]]
    with np.errstate(all="ignore"):
        t = (np.float64(np.float32(iso)) - fa) / (fb - fa)
        t = np.where((t >= 0) & (t <= 1), t, 0.5)
    step64 = np.asarray(np.asarray(step, dtype=np.float32), dtype=np.float64)
    ga, gb = _gradient(f, ia, step64, np.float64), _gradient(f, ib, step64, np.float64)
    with np.errstate(all="ignore"):
        g = ga + t[:, None] * (gb - ga)
        ln = np.sqrt((g * g).sum(1))
        n = np.where((ln > 0)[:, None], -g / ln[:, None], 0.0)
        e = U * (2 * np.abs(ga) + t[:, None] * (2 * np.abs(ga) + 2 * np.abs(gb) + 5 * np.abs(gb - ga)) + np.abs(g))
        tol = (e + np.abs(n) * np.sqrt((e * e).sum(1))[:, None]) / ln[:, None] + 5 * U
    tol = np.where(np.isfinite(tol), tol, np.inf)
    return dict(normals=n, tol=tol, length=ln)


# ---- topology -----------------------------------------------------------------------------------------------------------------------
def directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_census(triangles):
    """-> (directed edge -> count, undirected edge -> count) as dicts keyed by tuples."""
    from collections import Counter
    de = directed_edges(triangles)
    d = Counter(map(tuple, de.tolist()))
    u = Counter(tuple(sorted(e)) for e in de.tolist())
    return d, u


def euler_characteristic(n_vertices, triangles):
    _, u = edge_census(triangles)
    return n_vertices - len(u) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


# ---- the volumes of the tests ---------------------------------------------------------------------------------------------------------
def sphere_volume(n, centre, radius):
    """f = r - dist in fp64, then fp32; inside is f > 0."""
    ax = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    c = np.broadcast_to(np.asarray(centre, dtype=np.float64), (3,))
    return (radius - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def torus_volume(n, centre, R, r):
    ax = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    q = np.sqrt((x - centre) ** 2 + (y - centre) ** 2) - R
    return (r - np.sqrt(q * q + (z - centre) ** 2)).astype(np.float32)


def noise_volume(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def special_volume(shape, seed, iso):
    """Noise seeded with NaN, +-inf and values equal to iso."""
    f = noise_volume(shape, seed)
    r = np.random.default_rng(seed + 1).integers(0, 12, size=shape)
    f[r == 0] = np.nan
    f[r == 1] = np.inf
    f[r == 2] = -np.inf
    f[r == 3] = np.float32(iso)
    return f
