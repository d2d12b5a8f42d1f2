"""The mesh rasteriser's definition (include/sanerf_hip.h, "Mesh rasteriser") restated in numpy, operation for operation: float32 camera
transform and projection in the stated order, int32 snapping with 8 sub-pixel bits, int64 edge functions with the top-left rule, fp64
interpolation of the inverse depth, the 64-bit key whose maximum is the depth test, and the resolve.  Brute force over each triangle's
bounding box.  The device must equal this bit for bit."""
import numpy as np

GUARD = 1 << 22
F32 = np.float32


def project(vertices, pose, intrinsics, near):
    """rows: X, Y int32 [V]; r float32 [V]; placed bool [V]."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    m = np.asarray(pose, dtype=F32).reshape(4, 4)
    k = np.asarray(intrinsics, dtype=F32).reshape(4)
    near = F32(near)
    with np.errstate(all="ignore"):
        placed = np.isfinite(v).all(axis=1)
        d = [v[:, a] - m[a, 3] for a in range(3)]
        c = [(m[0, j] * d[0] + m[1, j] * d[1]) + m[2, j] * d[2] for j in range(3)]
        z = -c[2]
        placed &= z >= near
        r = (F32(1.0) / z).astype(F32)
        placed &= np.isfinite(r)
        x = (k[0] * c[0]) / z + k[2]
        y = -((k[1] * c[1]) / z) + k[3]
        fx, fy = np.rint(F32(256.0) * x), np.rint(F32(256.0) * y)
        placed &= (np.abs(fx) <= F32(GUARD)) & (np.abs(fy) <= F32(GUARD))        # no NaN passes
        X = np.where(placed, fx, 0).astype(np.int32)
        Y = np.where(placed, fy, 0).astype(np.int32)
    return X, Y, np.where(placed, r, F32(0)).astype(F32), placed


class _Tri:
    pass


def _setup(tri, V, X, Y, r, placed, cull, H, W):
    """(status, _Tri): status 0 drawn, 1 dropped (bad index / unplaced corner), 2 degenerate, 3 culled."""
    idx = [int(i) for i in tri]
    if any(i < 0 or i >= V for i in idx):
        return 1, None
    if not all(placed[i] for i in idx):
        return 1, None
    qx = [int(X[i]) for i in idx]
    qy = [int(Y[i]) for i in idx]
    A = (qx[1] - qx[0]) * (qy[2] - qy[0]) - (qy[1] - qy[0]) * (qx[2] - qx[0])
    if A == 0:
        return 2, None
    if cull and A > 0:          # front faces have A < 0 on a screen whose y points down
        return 3, None
    sg = -1 if A < 0 else 1
    s = _Tri()
    s.A = sg * A
    s.w00, s.sx, s.sy, s.bias = [], [], [], []
    for k in range(3):
        p, n = (k + 1) % 3, (k + 2) % 3
        dx, dy = sg * (qx[n] - qx[p]), sg * (qy[n] - qy[p])
        s.w00.append(dx * (128 - qy[p]) - dy * (128 - qx[p]))
        s.sx.append(-256 * dy)
        s.sy.append(256 * dx)
        s.bias.append(0 if (dy < 0 or (dy == 0 and dx > 0)) else -1)
    s.r = [np.float64(r[i]) for i in idx]
    s.idx = idx
    i0, i1 = max((min(qx) + 127) >> 8, 0), min((max(qx) - 128) >> 8, W - 1)
    j0, j1 = max((min(qy) + 127) >> 8, 0), min((max(qy) - 128) >> 8, H - 1)
    s.i0, s.j0, s.nx, s.ny = i0, j0, max(i1 - i0 + 1, 0), max(j1 - j0 + 1, 0)
    return 0, s


def _weights(s, pi, pj):
    """int64 edge functions at the centres of pixels (pi, pj) (arrays)."""
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    return [np.int64(s.w00[k]) + pi * np.int64(s.sx[k]) + pj * np.int64(s.sy[k]) for k in range(3)]


def _rho(s, w):
    p = [w[k].astype(np.float64) * s.r[k] for k in range(3)]
    total = (p[0] + p[1]) + p[2]
    return p, total, total / np.float64(s.A)


def rasterize(vertices, triangles, pose, intrinsics, H, W, near=0.05, cull=False, colors=None, normals=None, labels=None, bg_color=1.0,
              want_coverage=False):
    """dict of triangle_id int32 [H,W], depth f32 [H,W], mask uint8 [H,W], counts int32 [4] (drawn, dropped, degenerate, culled), and --
    with the attribute given -- image f32 [H,W,3], normal f32 [H,W,3], label uint8 [H,W].  want_coverage: also "coverage" int32 [H,W], the
    number of drawn triangles that cover each pixel, and "ties", the number of those whose depth bits there are the winner's."""
    vertices = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    V, T = vertices.shape[0], triangles.shape[0]
    X, Y, r, placed = project(vertices, pose, intrinsics, near)
    zbuf = np.zeros((H, W), dtype=np.uint64)
    coverage = np.zeros((H, W), dtype=np.int32)
    counts = np.zeros(4, dtype=np.int32)
    setups = {}
    for t in range(T):
        status, s = _setup(triangles[t], V, X, Y, r, placed, cull, H, W)
        counts[status] += 1
        if status != 0 or s.nx == 0 or s.ny == 0:
            continue
        setups[t] = s
        pj, pi = np.meshgrid(np.arange(s.j0, s.j0 + s.ny), np.arange(s.i0, s.i0 + s.nx), indexing="ij")
        w = _weights(s, pi, pj)
        inside = (w[0] + s.bias[0] >= 0) & (w[1] + s.bias[1] >= 0) & (w[2] + s.bias[2] >= 0)
        if not inside.any():
            continue
        _, _, rho = _rho(s, w)
        key = (rho.astype(F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - t)
        sub = zbuf[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx]
        np.maximum(sub, np.where(inside, key, np.uint64(0)), out=sub)
        coverage[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx] += inside

    out = {"triangle_id": np.full((H, W), -1, dtype=np.int32), "depth": np.zeros((H, W), dtype=F32), "mask": np.zeros((H, W), dtype=np.uint8),
           "counts": counts}
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
        ties = np.zeros((H, W), dtype=np.int32)             # drawn triangles whose depth bits at the pixel are the winner's
        for t, s in setups.items():
            pj, pi = np.meshgrid(np.arange(s.j0, s.j0 + s.ny), np.arange(s.i0, s.i0 + s.nx), indexing="ij")
            w = _weights(s, pi, pj)
            inside = (w[0] + s.bias[0] >= 0) & (w[1] + s.bias[1] >= 0) & (w[2] + s.bias[2] >= 0)
            bits = _rho(s, w)[2].astype(F32).view(np.uint32).astype(np.uint64)
            ties[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx] += inside & (bits == zbuf[s.j0:s.j0 + s.ny, s.i0:s.i0 + s.nx] >> np.uint64(32))
        out["ties"] = ties
    winner = (np.uint64(0xFFFFFFFF) - (zbuf & np.uint64(0xFFFFFFFF))).astype(np.int64)
    winner[zbuf == 0] = -1
    for t in np.unique(winner[winner >= 0]):
        s = setups[int(t)]
        pj, pi = np.nonzero(winner == t)
        w = _weights(s, pi, pj)
        p, total, rho = _rho(s, w)
        out["triangle_id"][pj, pi] = t
        out["depth"][pj, pi] = (np.float64(1.0) / rho).astype(F32)
        out["mask"][pj, pi] = 1
        mu = [p[k] / total for k in range(3)]
        for name, attr in (("image", colors), ("normal", normals)):
            if attr is not None:
                a = [attr[s.idx[k]].astype(np.float64) for k in range(3)]
                out[name][pj, pi] = ((mu[0][:, None] * a[0] + mu[1][:, None] * a[1]) + mu[2][:, None] * a[2]).astype(F32)
        if labels is not None:
            best = np.zeros(len(pi), dtype=np.int64)
            best[mu[1] > mu[0]] = 1
            best[mu[2] > np.where(best == 1, mu[1], mu[0])] = 2
            out["label"][pj, pi] = labels[np.asarray(s.idx)[best]]
    return out


# ---- cameras and shapes the tests share ------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """cam2world [4,4] f32 in the convention of get_rays: the camera looks along -z of its frame, x to the right, y up."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = s, u, -f, eye
    return m.astype(F32)


def screen_camera():
    """(pose, intrinsics) of a camera whose screen coordinates are the world's: the world point (px z, -py z, -z) lands on the pixel
    coordinates (px, py) at depth z (fx = fy = 1, cx = cy = 0, identity pose)."""
    return np.eye(4, dtype=F32), np.array([1.0, 1.0, 0.0, 0.0], dtype=F32)


def screen_vertices(xy, z=1.0):
    """World vertices that screen_camera() puts at the pixel coordinates xy [n,2] (exactly, for coordinates that are multiples of 1/256 and
    z a power of two) at depth z."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (xy.shape[0],))
    return np.stack([xy[:, 0] * z, -xy[:, 1] * z, -z], axis=1).astype(F32)


def icosphere(subdivisions=2, radius=1.0):
    """(vertices [V,3] f64, triangles [T,3] int32), counter-clockwise seen from outside."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int32)


def triangle_status(vertices, triangles, pose, intrinsics, H, W, near=0.05, cull=False):
    """int [T]: 0 drawn, 1 dropped, 2 degenerate, 3 culled."""
    vertices = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    X, Y, r, placed = project(vertices, pose, intrinsics, near)
    return np.array([_setup(t, vertices.shape[0], X, Y, r, placed, cull, H, W)[0] for t in triangles], dtype=np.int64)


def sphere_depth_bounds(H, W, intrinsics, distance, r_outer, r_inner):
    """For a camera at (0, 0, distance) with the identity rotation looking at a closed surface that lies between the spheres of radius
    r_inner <= r_outer around the origin: per pixel centre (fp64) the depth at which its ray enters the outer sphere and the inner sphere
    (NaN where it misses), and the radii in pixels of the two silhouettes around (cx, cy).  A ray that hits the inner sphere meets the
    surface between the two depths."""
    fx, fy, cx, cy = (float(a) for a in np.asarray(intrinsics).reshape(4))
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    u, v = (ii - cx) / fx, (jj - cy) / fy
    q = 1.0 + u * u + v * v

    def enter(radius):
        with np.errstate(invalid="ignore"):
            return (distance - np.sqrt(distance * distance - q * (distance * distance - radius * radius))) / q
    silhouette = [min(fx, fy) * radius / np.sqrt(distance * distance - radius * radius) for radius in (r_outer, r_inner)]
    return enter(r_outer), enter(r_inner), silhouette[0], silhouette[1]


def facet_inner_radius(vertices, triangles):
    """(r_hi, r_in): the largest |v|, and a lower bound of |p| over every point p of every facet.  With p = sum l_i v_i,
    |p|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= r_lo^2 - e_max^2 / 3: the sagitta of the facets from the longest edge."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles)
    rad = np.linalg.norm(v, axis=1)
    e = max(np.linalg.norm(v[t[:, a]] - v[t[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    return rad.max(), float(np.sqrt(rad.min() ** 2 - e * e / 3.0))


def check_sphere_image(out, H, W, intr, distance, r_hi, r_in, fraction=0.9):
    """What an image of a closed surface between the spheres r_in and r_hi around the origin must satisfy, seen from (0, 0, distance):
    covered inside the inner silhouette, empty outside the outer one, and inside `fraction` of the inner silhouette a depth between the
    two spheres' -- widened by the snapping term: a snapped triangle shows at a pixel p what the true one shows at some p' within
    sqrt(2) / 512 pixel of it (corners move by at most half a sub-pixel step per axis, and points inside move by a convex combination), so
    the bounds move by that distance times their steepest slope over the region, which for these convex functions of the radius is the
    secant beyond the rim -- and by the fp32 rounding of the camera transform, a few units of 2^-24 of the distance."""
    z_out, z_in, sil_out, sil_in = sphere_depth_bounds(H, W, intr, distance, r_hi, r_in)
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    rad = np.hypot(ii - intr[2], jj - intr[3])
    snap = np.sqrt(2.0) / 512
    mask = out["mask"] == 1
    assert mask[rad < sil_in - snap].all(), "a hole inside the inscribed circle"
    assert not mask[rad > sil_out + snap].any(), "coverage outside the circumscribed circle"
    region = rad < fraction * sil_in
    assert region.sum() > 100

    def depth_at(radius_px, sphere):        # along the ray through a point at that radius from the principal point
        q = 1.0 + (radius_px / intr[0]) ** 2
        return (distance - np.sqrt(distance ** 2 - q * (distance ** 2 - sphere ** 2))) / q
    rim = fraction * sil_in
    slope = max(depth_at(rim + 1.0, s) - depth_at(rim, s) for s in (r_hi, r_in))
    slack = slope * snap + 16 * 2.0 ** -24 * distance
    depth = out["depth"].astype(np.float64)
    assert (depth[region] >= z_out[region] - slack).all() and (depth[region] <= z_in[region] + slack).all()
    return float((z_in - z_out)[region].max() + slack)


# ---- the hand-worked cases (tests/test_mesh_raster_ref.py pins them in numpy, tests/test_gpu_mesh_raster.py runs them on the device) ----------
def hand_cases():
    """name -> dict(vertices, triangles, pose, intrinsics, H, W, near) and, where worked by hand, "pixels": the covered (i, j) set."""
    pose, intr = screen_camera()
    cases = {}

    def add(name, xy, tris, H=8, W=8, z=1.0, pixels=None, **extra):
        cases[name] = dict(vertices=screen_vertices(xy, z), triangles=np.asarray(tris, dtype=np.int32).reshape(-1, 3), pose=pose, intrinsics=intr,
                           H=H, W=W, near=0.05, pixels=pixels, **extra)
    # corners on pixel centres: the top edge y = 0.5 and the left edge x = 0.5 belong to the triangle, the hypotenuse x + y = 5 does not
    lower_left = {(i, j) for j in range(4) for i in range(4 - j)}
    add("centres_cw", [(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)], [(0, 1, 2)], pixels=lower_left)
    add("centres_ccw", [(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)], [(0, 2, 1)], pixels=lower_left)
    # its mirror image: the top edge and the diagonal y = x (a left edge) belong to it, the right edge x = 4.5 does not
    add("centres_right", [(0.5, 0.5), (4.5, 0.5), (4.5, 4.5)], [(0, 1, 2)], pixels={(i, j) for i in range(4) for j in range(i + 1)})
    # corners on pixel corners: centres with x, y > 1 strictly inside or on x + y = 6, which is not a top or left edge
    add("corners", [(1.0, 1.0), (5.0, 1.0), (1.0, 5.0)], [(1, 2, 0)], pixels={(i, j) for i in range(1, 5) for j in range(1, 5) if i + j < 5})
    # a convex quad with generic corners, split along either diagonal
    quad = [(1.30078125, 0.7421875), (13.6171875, 2.1796875), (11.55078125, 12.4140625), (2.26171875, 9.87109375)]
    add("quad_02", quad, [(0, 1, 2), (0, 2, 3)], H=14, W=16)
    add("quad_13", quad, [(0, 1, 3), (1, 2, 3)], H=14, W=16)
    # 12 triangles around a vertex on a pixel centre
    ring = [(8.5 + np.rint(256 * 6.3 * np.cos(a)) / 256, 8.5 + np.rint(256 * 6.3 * np.sin(a)) / 256) for a in np.arange(12) * (np.pi / 6) + 0.1]
    add("fan", [(8.5, 8.5)] + ring, [(0, 1 + k, 1 + (k + 1) % 12) for k in range(12)], H=17, W=17)
    # two overlapping triangles, the second one nearer; and the same triangle twice
    big = [(0.25, 0.25), (7.75, 0.5), (0.5, 7.75)]
    add("overlap_near_last", big + big, [(0, 1, 2), (3, 4, 5)], z=[2.0] * 3 + [1.0] * 3)
    add("overlap_near_first", big + big, [(3, 4, 5), (0, 1, 2)], z=[2.0] * 3 + [1.0] * 3)
    add("overlap_equal", big + big, [(0, 1, 2), (3, 4, 5)], z=1.0)
    # one good triangle and four that are dropped whole
    v = screen_vertices(big + [(1.0, 1.0)] * 3, 1.0)
    v[3] = (0.0, 0.0, -0.01)                   # nearer than near
    v[4] = (np.nan, 0.0, -1.0)
    v[5] = (20000.0, 0.0, -1.0)                # x = 20000 pixels: beyond the guard band of 2^14
    cases["dropped"] = dict(vertices=v, triangles=np.array([(0, 1, 2), (0, 1, 3), (0, 4, 2), (5, 1, 2), (0, 1, 6), (0, -1, 2), (0, 0, 1)], dtype=np.int32),
                            pose=pose, intrinsics=intr, H=8, W=8, near=0.05, pixels=None, counts=[1, 5, 1, 0])
    return cases


def run_case(case, **kw):
    args = {k: case[k] for k in ("vertices", "triangles", "pose", "intrinsics", "H", "W", "near")}
    args.update(kw)
    return rasterize(**args)
