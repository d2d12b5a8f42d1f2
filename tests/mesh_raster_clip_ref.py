"""Near-plane clipping of the mesh rasteriser (include/sanerf_hip.h, "Mesh rasteriser", the paragraphs on clipping) restated in numpy,
operation for operation, on top of tests/mesh_raster_ref.py, which it imports and leaves as it is: the fp32 camera frame recomputed with
the projection's expressions, the corner roles, the fp64 crossing points with their roles taken from the vertices, the polygon walk, the
two pieces set up as triangles are, the parent's key, the counters and the resolve through the parent's corners.  The device must equal
this bit for bit; without a behind corner it equals mesh_raster_ref.rasterize bit for bit."""
import numpy as np

import mesh_raster_ref as ref

F32, F64 = np.float32, np.float64
GUARD = ref.GUARD


def camera_frame(vertices, pose):
    """(c [3] of float32 [V], z float32 [V], finite bool [V]): the projection's own expressions in its order."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    m = np.asarray(pose, dtype=F32).reshape(4, 4)
    with np.errstate(all="ignore"):
        d = [v[:, a] - m[a, 3] for a in range(3)]
        c = [(m[0, j] * d[0] + m[1, j] * d[1]) + m[2, j] * d[2] for j in range(3)]
        return c, -c[2], np.isfinite(v).all(axis=1)


def crossing(P, Q, c, z, intrinsics, near):
    """The point where the edge from the front vertex P to the behind vertex Q meets the near plane: (X, Y, s, ok), fp64 from the fp32
    values, every operation rounded on its own.  ok: inside the guard band (no NaN passes)."""
    k = [F64(a) for a in np.asarray(intrinsics, dtype=F32).reshape(4)]
    near = F64(F32(near))
    with np.errstate(all="ignore"):
        zp, zq = F64(z[P]), F64(z[Q])
        s = (zp - near) / (zp - zq)
        x = F64(c[0][P]) + s * (F64(c[0][Q]) - F64(c[0][P]))
        y = F64(c[1][P]) + s * (F64(c[1][Q]) - F64(c[1][P]))
        px = (k[0] * x) / near + k[2]
        py = -((k[1] * y) / near) + k[3]
        X, Y = np.rint(F64(256.0) * px), np.rint(F64(256.0) * py)
        ok = bool(abs(X) <= GUARD and abs(Y) <= GUARD)
    return (int(X), int(Y), s, True) if ok else (0, 0, s, False)


class _Parent:
    """A triangle as the clipped rasteriser sees it: status (0 drawn, 1 dropped, 2 degenerate, 3 culled), clipped, and its pieces --
    (status, mesh_raster_ref._Tri or None, B [3][3] float64) each, B[k] the weights of the parent's corners at the piece's point k."""


def _piece(points, cull, H, W):
    X = np.array([p[0] for p in points], dtype=np.int32)
    Y = np.array([p[1] for p in points], dtype=np.int32)
    r = np.array([p[2] for p in points], dtype=F32)
    status, s = ref._setup((0, 1, 2), 3, X, Y, r, [True] * 3, cull, H, W)
    return status, s, [p[3] for p in points]


UNIT = [[F64(1.0 if i == k else 0.0) for i in range(3)] for k in range(3)]


def parent(tri, V, X, Y, r, placed, c, z, finite, intrinsics, near, cull, H, W):
    p = _Parent()
    p.clipped, p.pieces = False, []
    idx = [int(i) for i in tri]
    p.idx = idx
    if any(i < 0 or i >= V for i in idx):
        p.status = 1
        return p
    front = [bool(placed[i]) for i in idx]
    if all(front):
        p.status, s = ref._setup(tri, V, X, Y, r, placed, cull, H, W)
        p.pieces = [(p.status, s, UNIT)]
        return p
    behind = [(not front[k]) and bool(finite[idx[k]]) and bool(z[idx[k]] < F32(near)) for k in range(3)]
    if not any(front) or not all(f or b for f, b in zip(front, behind)):
        p.status = 1
        return p
    r_near = F32(1.0) / F32(near)
    points = []
    for k in range(3):
        n = (k + 1) % 3
        if front[k]:
            points.append((int(X[idx[k]]), int(Y[idx[k]]), F32(r[idx[k]]), UNIT[k]))
        if front[k] != front[n]:
            kp, kq = (k, n) if front[k] else (n, k)
            cx, cy, s, ok = crossing(idx[kp], idx[kq], c, z, intrinsics, near)
            if not ok:
                p.status = 1
                return p
            row = [F64(0.0)] * 3
            row[kp], row[kq] = F64(1.0) - s, s
            points.append((cx, cy, r_near, row))
    p.clipped = True
    p.pieces = [_piece([points[0], points[1], points[2]], cull, H, W)]
    if len(points) == 4:
        p.pieces.append(_piece([points[0], points[2], points[3]], cull, H, W))
    statuses = [q[0] for q in p.pieces]
    p.status = 0 if 0 in statuses else (3 if 3 in statuses else 2)
    return p


def _box(s):
    return np.meshgrid(np.arange(s.j0, s.j0 + s.ny), np.arange(s.i0, s.i0 + s.nx), indexing="ij")


def _inside(s, w):
    return (w[0] + s.bias[0] >= 0) & (w[1] + s.bias[1] >= 0) & (w[2] + s.bias[2] >= 0)


def _bits(rho):
    return rho.astype(F32).view(np.uint32).astype(np.uint64)


def rasterize(vertices, triangles, pose, intrinsics, H, W, near=0.05, cull=False, colors=None, normals=None, labels=None, bg_color=1.0,
              want_coverage=False, clip=True):
    """mesh_raster_ref.rasterize with near-plane clipping: its dict, and "clip_counts" int32 [2] = the clipped triangles (one or two corners
    behind the near plane, every crossing point inside the guard band) and the pieces of them that were drawn.  want_coverage: "coverage" is
    the number of drawn PIECES that cover each pixel, "ties" the number of those whose depth bits there are the winner's.  clip=False is
    mesh_raster_ref.rasterize itself."""
    if not clip:
        return ref.rasterize(vertices, triangles, pose, intrinsics, H, W, near=near, cull=cull, colors=colors, normals=normals, labels=labels,
                             bg_color=bg_color, want_coverage=want_coverage)
    vertices = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    V, T = vertices.shape[0], triangles.shape[0]
    X, Y, r, placed = ref.project(vertices, pose, intrinsics, near)
    c, z, finite = camera_frame(vertices, pose)
    zbuf = np.zeros((H, W), dtype=np.uint64)
    coverage = np.zeros((H, W), dtype=np.int32)
    counts, clip_counts = np.zeros(4, dtype=np.int32), np.zeros(2, dtype=np.int32)

    def build(t, cull):
        return parent(triangles[t], V, X, Y, r, placed, c, z, finite, intrinsics, near, cull, H, W)

    def drawn_pieces(p):
        return [(s, B) for status, s, B in p.pieces if status == 0 and s.nx > 0 and s.ny > 0]

    for t in range(T):
        p = build(t, cull)
        counts[p.status] += 1
        if p.clipped:
            clip_counts[0] += 1
            clip_counts[1] += sum(1 for q in p.pieces if q[0] == 0)
        for s, _ in drawn_pieces(p):
            pj, pi = _box(s)
            w = ref._weights(s, pi, pj)
            inside = _inside(s, w)
            key = (_bits(ref._rho(s, w)[2]) << np.uint64(32)) | np.uint64(0xFFFFFFFF - t)
            sub = zbuf[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx]
            np.maximum(sub, np.where(inside, key, np.uint64(0)), out=sub)
            coverage[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx] += inside

    out = {"triangle_id": np.full((H, W), -1, dtype=np.int32), "depth": np.zeros((H, W), dtype=F32), "mask": np.zeros((H, W), dtype=np.uint8),
           "counts": counts, "clip_counts": clip_counts}
    if colors is not None:
        colors = np.asarray(colors, dtype=F32).reshape(V, 3)
        out["image"] = np.full((H, W, 3), F32(bg_color), dtype=F32)
    if normals is not None:
        normals = np.asarray(normals, dtype=F32).reshape(V, 3)
        out["normal"] = np.zeros((H, W, 3), dtype=F32)
    if labels is not None:
        labels = np.asarray(labels, dtype=np.uint8).reshape(V)
        out["label"] = np.full((H, W), 255, dtype=np.uint8)
    if want_coverage:
        out["coverage"] = coverage
        ties = np.zeros((H, W), dtype=np.int32)
        for t in range(T):
            for s, _ in drawn_pieces(build(t, cull)):
                pj, pi = _box(s)
                w = ref._weights(s, pi, pj)
                ties[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx] += _inside(s, w) & (_bits(ref._rho(s, w)[2]) == zbuf[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx] >> np.uint64(32))
        out["ties"] = ties
    winner = (np.uint64(0xFFFFFFFF) - (zbuf & np.uint64(0xFFFFFFFF))).astype(np.int64)
    winner[zbuf == 0] = -1
    for t in np.unique(winner[winner >= 0]):
        p = build(int(t), False)                    # the resolve rebuilds every piece with A != 0
        pj, pi = np.nonzero(winner == t)
        # the piece that covers the pixel centre; of two, the one with the larger fp32 rho bits, then the first
        chosen = np.full(len(pi), -1, dtype=np.int64)
        best = np.zeros(len(pi), dtype=np.uint64)
        per_piece = []
        for n, (status, s, B) in enumerate(p.pieces):
            if status != 0:
                per_piece.append(None)
                continue
            w = ref._weights(s, pi, pj)
            pk, total, rho = ref._rho(s, w)
            per_piece.append((pk, total, rho, B))
            bits = _bits(rho)
            take = _inside(s, w) & ((chosen < 0) | (bits > best))
            chosen[take], best[take] = n, bits[take]
        assert (chosen >= 0).all(), "a winner that no piece covers"
        for n, data in enumerate(per_piece):
            sel = chosen == n
            if data is None or not sel.any():
                continue
            pk, total, rho, B = data
            qj, qi = pj[sel], pi[sel]
            out["triangle_id"][qj, qi] = t
            out["depth"][qj, qi] = (F64(1.0) / rho[sel]).astype(F32)
            out["mask"][qj, qi] = 1
            mu = [pk[k][sel] / total[sel] for k in range(3)]
            if p.clipped:
                lam = []
                for i in range(3):
                    acc = np.zeros(len(qi), dtype=F64)
                    for k in range(3):
                        acc = acc + mu[k] * B[k][i]
                    lam.append(acc)
            else:
                lam = mu
            for name, attr in (("image", colors), ("normal", normals)):
                if attr is not None:
                    a = [attr[p.idx[k]].astype(F64) for k in range(3)]
                    out[name][qj, qi] = ((lam[0][:, None] * a[0] + lam[1][:, None] * a[1]) + lam[2][:, None] * a[2]).astype(F32)
            if labels is not None:
                first = np.zeros(len(qi), dtype=np.int64)
                first[lam[1] > lam[0]] = 1
                first[lam[2] > np.where(first == 1, lam[1], lam[0])] = 2
                out["label"][qj, qi] = labels[np.asarray(p.idx)[first]]
    return out


# ---- the cases the tests share -----------------------------------------------------------------------------------------------------------------
def hand_cases():
    """name -> dict(vertices, triangles, pose, intrinsics, H, W, near, pixels): one triangle each that the plane z = near = 1 cuts, on the
    12 x 12 screen of screen_camera(); "pixels" is the covered (i, j) set worked by hand.

    two_front: (1, -1, -2), (17, -1, -2), (1, -17, 0), i.e. the pixel coordinates (0.5, 0.5) and (8.5, 0.5) at depth 2 and a corner in the
    camera's own plane.  s = (2 - 1) / (2 - 0) = 1/2 on both crossing edges: (17, -1) -> (1, -17) crosses at (9, -9), the pixel coordinates
    (9, 9) at depth 1, and (1, -1) -> (1, -17) at (1, -9), pixel (1, 9).  The polygon (0.5, 0.5), (8.5, 0.5), (9, 9), (1, 9): the top edge
    y = 0.5 holds the centres i = 0 .. 7 (x = 8.5 is its end and belongs to the right edge, which is out); the left edge x = 0.5 + (y - 0.5)
    / 17 passes x = 0.5 only at y = 0.5, so rows 1 .. 8 start at i = 1 (centre 1.5 > 0.5 + 8 / 17); the right edge x = 8.5 + (y - 0.5) / 17
    lies in (8.5, 9), so rows 1 .. 8 end at i = 8; the bottom edge y = 9 is out: 8 + 8 * 8 = 72 pixels.

    behind_camera: the third corner at (1, -17, 2), depth -2, behind the camera.  s = (2 - 1) / (2 + 2) = 1/4: the crossing points are
    (13, -5) and (1, -5), the pixels (13, 5) and (1, 5).  The polygon (0.5, 0.5), (8.5, 0.5), (13, 5), (1, 5): rows 0 .. 4 (the bottom edge
    y = 5 is out); the left edge x = 0.5 + (y - 0.5) / 9 takes i = 0 in row 0 only; the right edge x = 8.5 + (y - 0.5) passes through the
    centre (8.5 + j, j + 0.5) of every row j and is out, so row j ends at i = 7 + j: 8 + 8 + 9 + 10 + 11 = 46 pixels."""
    pose, intr = ref.screen_camera()
    tri = np.array([[0, 1, 2]], dtype=np.int32)

    def case(third, pixels):
        return dict(vertices=np.array([(1, -1, -2), (17, -1, -2), third], dtype=F32), triangles=tri, pose=pose, intrinsics=intr, H=12, W=12, near=1.0,
                    pixels=pixels)
    return {"two_front": case((1, -17, 0), {(i, 0) for i in range(8)} | {(i, j) for j in range(1, 9) for i in range(1, 9)}),
            "behind_camera": case((1, -17, 2), {(i, 0) for i in range(8)} | {(i, j) for j in range(1, 5) for i in range(1, 8 + j)})}


def sphere_case():
    """The camera at the centre of icosphere(3) turned inside out, the near plane cutting it."""
    v, t = ref.icosphere(3, 1.0)
    return dict(vertices=v.astype(F32), triangles=np.ascontiguousarray(t[:, ::-1]), pose=np.eye(4, dtype=F32),
                intrinsics=np.array([20.0, 20.0, 32.0, 32.0], dtype=F32), H=64, W=64, near=0.6)


def ground_case():
    """A 16 x 16 grid of quads, two triangles each, a quarter unit under the camera: x in [-2, 2], z from -4.03 to 0.37."""
    n = 16
    xs, zs = np.linspace(-2.0, 2.0, n + 1), np.linspace(-4.03, 0.37, n + 1)
    gz, gx = np.meshgrid(zs, xs, indexing="ij")
    v = np.stack([gx, np.full_like(gx, -0.25), gz], axis=-1).reshape(-1, 3).astype(F32)
    tris = []
    for a in range(n):
        for b in range(n):
            p00, p01, p10, p11 = a * (n + 1) + b, a * (n + 1) + b + 1, (a + 1) * (n + 1) + b, (a + 1) * (n + 1) + b + 1
            tris += [(p00, p10, p11), (p00, p11, p01)]
    return dict(vertices=v, triangles=np.asarray(tris, dtype=np.int32), pose=np.eye(4, dtype=F32),
                intrinsics=np.array([32.0, 32.0, 32.0, 32.0], dtype=F32), H=64, W=64, near=0.5)


def run_case(case, **kw):
    args = {k: case[k] for k in ("vertices", "triangles", "pose", "intrinsics", "H", "W", "near")}
    args.update(kw)
    return rasterize(**args)
