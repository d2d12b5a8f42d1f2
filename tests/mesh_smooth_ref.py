"""Mesh smoothing restated: Taubin / Laplacian smoothing of an indexed triangle mesh on integers, and the geometric normals of the result --
numpy, as include/sanerf_hip.h defines the entries of csrc/mesh_smooth.hip.  Every sum is a sum of integers (int64, wrapping) and every
other quantity is the correctly rounded result of the stated operations (float32 / float64), so the device has to EQUAL this file:
vertices and normals bit for bit, flags exactly.  No tolerance appears anywhere.

Definition (the header has the same text).  vertices [V,3] fp32, triangles [T,3] int32, origin[3] fp32 (finite), ONE quantum fp32 (> 0).
  quantise    per axis u = p - origin and s = u / quantum in fp32 (two roundings), r = rint(s).  PLACED iff all three r are finite and
              0 <= r < 2^22; Q0 = (int)r.  An unplaced vertex never moves, contributes to no sum and to no normal.
  valid       a triangle whose three indices lie in [0, V) and are pairwise distinct; anything else contributes nothing anywhere.
  pairs       a valid triangle (a, b, c) gives a the pair (next = b, prev = c), b the pair (c, a), c the pair (a, b).
  open        mix(i) = the splitmix64 finaliser of i + 1; v is open iff sum mix(next) != sum mix(prev) modulo 2^64 over its pairs.
  half-step   factor f (fp32, promoted to fp64).  S = the int64 sum of Q over the placed next and the placed prev of v's pairs, n the number
              of those terms.  v is free iff placed, n > 0 and not (open and pin_open).  Free: per axis d = S / n - Q (fp64, each
              operation rounded), r = rint(f d) (ties to even), Q' = clamp(Q + r, 0, 2^22 - 1).  Otherwise Q' = Q.  All at once (Jacobi).
  iteration   a half-step with lambda, then one with mu; mu == 0 skips the second.  0 < lambda <= 1; mu == 0 or -1 <= mu < -lambda.
  vertices    final Q == Q0: the input bits.  Otherwise per axis fp32((double)origin + (double)quantum (double)Q).
  normals     S = the int64 sum over v's pairs with all three corners placed of (Q_next - Q_v) x (Q_prev - Q_v), final integers;
              S / sqrt((Sx Sx + Sy Sy) + Sz Sz) in fp64, one rounding to fp32; (0,0,0) when S is zero.
  flags       bit 0 placed, bit 1 open, bit 2 moved (placed and Q != Q0)."""
import numpy as np

import mesh_ref as mr
import mesh_simplify_ref as ms

RANGE = 1 << 22
PLACED, OPEN, MOVED = 1, 2, 4


def quantise(vertices, origin, quantum):
    """-> (Q [V,3] int64, 0 where unplaced; placed [V] bool)."""
    p = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float32)
    with np.errstate(all="ignore"):
        u = p - o                                          # fp32
        s = u / np.float32(quantum)                        # fp32, IEEE
        r = np.rint(s)                                     # ties to even
        placed = ((r >= 0) & (r < np.float32(RANGE))).all(axis=1)          # NaN and the infinities compare false
    return np.where(placed[:, None], r, np.float32(0)).astype(np.int64), placed


def corner_pairs(triangles, V):
    """-> (owner, nxt, prv): one entry per corner of every valid triangle, int64."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    valid = ((t >= 0) & (t < V)).all(axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    t = t[valid]
    owner = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    nxt = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    prv = np.concatenate([t[:, 2], t[:, 0], t[:, 1]])
    return owner, nxt, prv


def mix(i):
    """The finaliser of splitmix64 of i + 1, elementwise, modulo 2^64."""
    with np.errstate(over="ignore"):
        x = np.asarray(i).astype(np.uint64) + np.uint64(1)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def open_vertices(pairs, V):
    owner, nxt, prv = pairs
    a, b = np.zeros(V, dtype=np.uint64), np.zeros(V, dtype=np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(a, owner, mix(nxt))
        np.add.at(b, owner, mix(prv))
    return a != b


def half_step(Q, placed, is_open, pairs, f, pin_open=True):
    """One half-step with factor f on Q [V,3] int64 -> the new Q (the input is not modified)."""
    owner, nxt, prv = pairs
    V = len(Q)
    S, n = np.zeros((V, 3), dtype=np.int64), np.zeros(V, dtype=np.int64)
    for other in (nxt, prv):
        ok = placed[other]
        np.add.at(S, owner[ok], Q[other[ok]])
        np.add.at(n, owner[ok], 1)
    free = placed & (n > 0) & ~(is_open & bool(pin_open))
    out = Q.copy()
    f64 = np.float64(np.float32(f))
    d = S[free].astype(np.float64) / n[free].astype(np.float64)[:, None] - Q[free].astype(np.float64)
    r = np.rint(f64 * d).astype(np.int64)
    out[free] = np.clip(Q[free] + r, 0, RANGE - 1)
    return out


def check_factors(lam, mu):
    lam, mu = np.float32(lam), np.float32(mu)
    return bool(0 < lam <= 1 and (mu == 0 or -1 <= mu < -lam))


def steps(Q, placed, is_open, pairs, iterations, lam=0.5, mu=-0.53, pin_open=True):
    assert check_factors(lam, mu)
    for _ in range(int(iterations)):
        Q = half_step(Q, placed, is_open, pairs, lam, pin_open)
        if np.float32(mu) != 0:
            Q = half_step(Q, placed, is_open, pairs, mu, pin_open)
    return Q


def positions(vertices, Q, Q0, origin, quantum):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    o, q = np.asarray(origin, dtype=np.float32).astype(np.float64), np.float64(np.float32(quantum))
    moved = (Q != Q0).any(axis=1)
    out = v.copy()
    out[moved] = (o + q * Q[moved].astype(np.float64)).astype(np.float32)
    return out, moved


def geometric_normals(Q, placed, pairs):
    owner, nxt, prv = pairs
    ok = placed[owner] & placed[nxt] & placed[prv]
    o, a, b = owner[ok], Q[nxt[ok]] - Q[owner[ok]], Q[prv[ok]] - Q[owner[ok]]
    S = np.zeros((len(Q), 3), dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(S, o, np.cross(a, b))
    s = S.astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        return np.where((S == 0).all(axis=1)[:, None], 0.0, s / length[:, None]).astype(np.float32), S


def smooth(vertices, triangles, origin, quantum, iterations=10, lam=0.5, mu=-0.53, pin_open=True):
    """-> dict(vertices [V,3] f32, normals [V,3] f32, flags [V] uint8, and for the tests: Q, Q0, placed, open, S)."""
    V = len(vertices)
    Q0, placed = quantise(vertices, origin, quantum)
    pairs = corner_pairs(triangles, V)
    is_open = open_vertices(pairs, V)
    Q = steps(Q0, placed, is_open, pairs, iterations, lam, mu, pin_open)
    pos, moved = positions(vertices, Q, Q0, origin, quantum)
    normals, S = geometric_normals(Q, placed, pairs)
    flags = (placed * PLACED + is_open * OPEN + moved * MOVED).astype(np.uint8)
    return dict(vertices=pos, normals=normals, flags=flags, Q=Q, Q0=Q0, placed=placed, open=is_open, S=S)


def quantisation(lo, hi):
    """raymarching.smooth_quantisation restated: E the longest side in fp64, quantum = fp32(E / 2^21), origin = fp32(lo - 524288 quantum)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    quantum = np.float32((hi - lo).max() / 2.0 ** 21)
    return [float(np.float32(x - 524288.0 * np.float64(quantum))) for x in lo], float(quantum)


def bounding_quantisation(vertices):
    v = np.asarray(vertices, dtype=np.float32)
    v = v[np.isfinite(v).all(axis=1)]
    return quantisation(v.min(axis=0), v.max(axis=0))


# ---- measures the properties use ----------------------------------------------------------------------------------------------------------
def boundary_vertices(triangles, V):
    """The endpoints of the undirected edges that exactly one valid triangle uses."""
    owner, nxt, _ = corner_pairs(triangles, V)
    e = np.sort(np.stack([owner, nxt], axis=1), axis=1)
    edges, count = np.unique(e, axis=0, return_counts=True)
    return np.unique(edges[count == 1])


def mean_dihedral_degrees(vertices, triangles):
    """The mean angle between the unit normals of the two triangles at every edge that exactly two triangles share (fp64)."""
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-300)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    face = np.tile(np.arange(len(t)), 3)
    _, inverse, counts = np.unique(e, axis=0, return_inverse=True, return_counts=True)
    by_edge = face[np.argsort(inverse.reshape(-1), kind="stable")]       # the faces, grouped by edge
    first = (np.cumsum(counts) - counts)[counts == 2]
    fa, fb = by_edge[first], by_edge[first + 1]
    cosine = np.clip((fn[fa] * fn[fb]).sum(axis=1), -1.0, 1.0)
    return float(np.degrees(np.arccos(cosine)).mean())


# ---- the meshes of the tests --------------------------------------------------------------------------------------------------------------
SHAPE = (24, 24, 24)
CASES = ((1, 0.5, 0.0, True), (3, 0.5, -0.53, True), (10, 0.63, -0.67, True), (3, 0.5, -0.53, False))       # (N, lambda, mu, pin_open)
_cache = {}


def clipped_sphere():
    return mr.sphere_volume(24, (11.3, 12.1, 3.2), 7.6)


def noisy_sphere():
    rng = np.random.default_rng(5)
    vol = ms.VOLUMES["sphere"]()
    return (vol.astype(np.float64) + rng.normal(0.0, 0.35, size=vol.shape)).astype(np.float32)


VOLUMES = dict(ms.VOLUMES, clipped_sphere=clipped_sphere, noisy_sphere=noisy_sphere)


def volume_mesh(name):
    """mesh_ref.isosurface of the named 24^3 volume at iso 0 (unit lattice at the origin); computed once, never modified."""
    if name in ms.VOLUMES:
        return ms.volume_mesh(name)
    if name not in _cache:
        _cache[name] = mr.isosurface(VOLUMES[name](), 0.0)
    return _cache[name]


def lattice_quantisation(shape=SHAPE, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0)):
    """What NeRFRenderer.extract_mesh(smooth=) uses for an extraction lattice: the quantisation of the lattice's own box."""
    lo = [float(np.float32(o)) for o in origin]
    return quantisation(lo, [lo[a] + (shape[a] - 1) * float(np.float32(step[a])) for a in range(3)])


def double_cone(n=5000):
    """A closed double cone: a ring of n vertices of radius 1 in the plane z = 0, an apex above and one below, oriented outward.  Each
    apex has n pairs -- a row far longer than a mesh's usual valence.  -> (vertices, triangles); vertex 0 and 1 are the apexes."""
    phi = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(phi), np.sin(phi), 0.05 * np.sin(7.0 * phi)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.7], [0.0, 0.0, -0.6]], ring]).astype(np.float32)
    i = 2 + np.arange(n)
    j = 2 + (np.arange(n) + 1) % n
    top = np.stack([np.zeros(n, dtype=np.int64), i, j], axis=1)             # counter-clockwise seen from above
    bottom = np.stack([np.ones(n, dtype=np.int64), j, i], axis=1)
    return v, np.concatenate([top, bottom]).astype(np.int32)


def clamp_fan(upper=False):
    """A fan of six triangles around vertex 0, which sits 3 quanta from the end of the integer range (origin 0, quantum 1) with its rim --
    open, so pinned -- 40 and more quanta further in.  With lambda = 0.2 and mu = -1 an iteration moves the centre by about -0.6 of its
    distance to the rim's mean: out of the range after one iteration, where it is clamped.  -> (vertices, triangles)."""
    rim = np.array([[60, 43, 50], [43, 60, 47], [50, 70, 43], [70, 50, 44], [45, 45, 66], [66, 44, 45]], dtype=np.int64)
    q = np.concatenate([[[3, 3, 3]], rim])
    if upper:
        q = RANGE - 1 - q
    t = np.array([[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)], dtype=np.int32)
    return q.astype(np.float32), t


def tie_tetrahedron(sign=1):
    """Vertex 0 at (100,100,100), the mean of its three neighbours at (100,100,100) + sign (1, 3, -1): with f = +-0.5 the products f d are
    exactly +-0.5 and +-1.5.  -> (vertices, triangles), origin 0 and quantum 1."""
    off = sign * np.array([[6, 0, 0], [-6, 6, 0], [0, -6, 0]]) + sign * np.array([1, 3, -1]) + 100
    return np.concatenate([[[100, 100, 100]], off]).astype(np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)


def terrain():
    v, _, t, _ = ms.terrain()
    return v, t


def malformed():
    """The sphere with everything the definition names, as mesh_simplify_ref.malformed builds its own: triangle rows holding -1, V and
    2^31 - 1, a NaN vertex, an infinite one, a finite vertex beyond the integer range -- and rows that repeat an index.
    -> (vertices, triangles, (origin, quantum)): the quantisation is the 24^3 lattice's."""
    v, _, t, _ = ms.malformed(volume_mesh("sphere"), SHAPE)
    t = t.copy()
    t[11, 1] = t[11, 0]                                    # (a, a, c)
    t[len(t) // 4] = t[len(t) // 4, 0]                     # (a, a, a)
    t[len(t) // 5, 2] = t[len(t) // 5, 0]                  # (a, b, a)
    return v, t, lattice_quantisation()
