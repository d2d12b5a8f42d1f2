"""Mesh split restated: an indexed triangle mesh with a label on every vertex, taken apart into one mesh per part -- numpy and plain loops, as
include/sanerf_hip.h defines the entries of csrc/mesh_split.hip.  Nothing here is shared with the package.

Definition (the header has the same text).  vertices [V,3] f32, normals [V,3] f32 or None, triangles [T,3] int32, labels [V] uint8.
  parts       P = 33.  part(label) = min(label, 32): part p < 32 is instance id p, part 32 collects every label >= 32 (255 = "none" too).
  valid       a triangle is valid iff its three indices are in [0, V).  An invalid one belongs to no part and is dropped.
  vote        the part of a valid triangle is the part that at least two of its corners have; with three different parts, the lowest.
  membership  vertex v belongs to part p iff some valid triangle of part p has v as a corner.  A seam vertex belongs to several parts and is
              duplicated into each; a vertex in no valid triangle belongs to none and is dropped.
  output      packed, parts contiguous and in part order: the triangles of part p in their input order (a stable partition), the member
              vertices of part p in increasing input index; triangle indices local to the part; rows copied bit for bit; source_vertex and
              source_triangle = the input index of every output row; the two offset arrays [P+1]; counts = {V', T'}."""
import numpy as np

P = 33


def part_of(label):
    return min(int(label), P - 1)


def triangle_parts(triangles, labels):
    """[T] int64: the part of every triangle, -1 for an invalid one."""
    V = len(labels)
    out = []
    for row in np.asarray(triangles, dtype=np.int64).reshape(-1, 3):
        a, b, c = (int(x) for x in row)
        if not (0 <= a < V and 0 <= b < V and 0 <= c < V):
            out.append(-1)
            continue
        pa, pb, pc = part_of(labels[a]), part_of(labels[b]), part_of(labels[c])
        if pa == pb or pa == pc:
            out.append(pa)
        elif pb == pc:
            out.append(pb)
        else:
            out.append(min(pa, pb, pc))
    return np.array(out, dtype=np.int64)


def split(vertices, normals, triangles, labels):
    """-> dict(vertices, normals, triangles, source_vertex, source_triangle, part_triangle_offsets, part_vertex_offsets, counts)."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.uint8)
    assert len(labels) == len(vertices)
    part = triangle_parts(tri, labels)
    out_tri, src_v, src_t, toff, voff = [], [], [], [0], [0]
    by_part = [[] for _ in range(P)]
    for t, p in enumerate(part.tolist()):                                   # input order inside every part
        if p >= 0:
            by_part[p].append(t)
    for mine in by_part:
        members = sorted({int(x) for t in mine for x in tri[t]})            # increasing input index
        local = {v: i for i, v in enumerate(members)}
        for t in mine:
            out_tri.append([local[int(x)] for x in tri[t]])
        src_t += mine
        src_v += members
        toff.append(len(src_t))
        voff.append(len(src_v))
    src_v = np.array(src_v, dtype=np.int32)
    return dict(vertices=vertices[src_v], normals=None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)[src_v],
                triangles=np.array(out_tri, dtype=np.int32).reshape(-1, 3), source_vertex=src_v, source_triangle=np.array(src_t, dtype=np.int32),
                part_triangle_offsets=np.array(toff, dtype=np.int32), part_vertex_offsets=np.array(voff, dtype=np.int32),
                counts=np.array([len(src_v), len(src_t)], dtype=np.int64))


LABEL_POOL = (0, 1, 5, 31, 32, 200, 255)


def soup(V, T, seed, invalid=True, pool=LABEL_POOL):
    """Random triangles over V labelled vertices: labels from `pool`, a third of the vertices unreferenced, a duplicated row, (a,a,b) and
    (a,a,a) rows and -- invalid=True, T >= 8 -- rows that hold -1, V and 2^31 - 1.  -> (triangles [T,3] int32, labels [V] uint8)."""
    rng = np.random.default_rng(seed)
    labels = np.array(pool, dtype=np.uint8)[rng.integers(0, len(pool), size=V)]
    used = np.sort(rng.permutation(V)[: max(V - V // 3, 1)])
    t = used[rng.integers(0, len(used), size=(T, 3))].astype(np.int64)
    if T >= 8:
        t[1] = t[0]
        t[2, 1] = t[2, 0]
        t[3, :] = t[3, 0]
        if invalid:
            t[4, 0], t[5, 1], t[6, 2] = -1, V, 2 ** 31 - 1
            t[T - 1] = (-1, V, 2 ** 31 - 1)
    return t.astype(np.int32), labels
