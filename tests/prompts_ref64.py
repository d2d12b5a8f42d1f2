"""A float64 restatement of the point-prompt step (sn_rm_points_lift / _point_store_update / _points_project / _prompt_overlay), written from
the semantics stated in include/sanerf_hip.h, and the error bound the fp32 camera and pixel coordinates are held to.  Used by the CPU test
(the fixture made from the reference's own lines must agree with it) and by the GPU test (the kernels must).

The bound.  u = 2^-24, gamma_k = k u / (1 - k u).  A = the cam2world pose, X = A^-1, p = (x, y, z, 1).  An fp32 evaluation of p @ X^T with an
fp32 inverse -- what the reference does -- has two error sources:
  * the inverse.  LU with partial pivoting, inversion of U, solve against L: each stage perturbs its result by at most gamma_n in the
    componentwise sense (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., sections 9.3, 8.1 and 14.3; n = 4), so to first
    order |X_hat A - I| <= 3 gamma_4 |X| |L| |U| and |X_hat - X| <= 3 gamma_4 |X| |L| |U| |X|.  |L| |U| is formed here from an LU of A
    in float64;
  * the product: a dot product of 4 terms in any order, gamma_4 |X| |p|, and the rounding of the result.
      E_cam = (3 gamma_4 |X| |L| |U| |X| + gamma_4 |X|) |p|.
The kernel inverts and multiplies in fp64 and rounds once: u |cam|, far inside.  The pixel coordinates are then one fp32 chain,
  q = fl(fl(f c) / z), s = fl(q + c0), px = fl(W - s)  (py = s), so with perturbed inputs c +- E_c, z +- E_z:
      E_q  = |f| (E_c / (|z| - E_z) + |c| E_z / (|z| (|z| - E_z))) + gamma_2 |q|
      E_uv = E_q + u (|s| + E_q) + u (|px| + E_q)                              (the last term for px only)
and infinity where |z| <= E_z.
"""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


# ---- lift and store -------------------------------------------------------------------------------------------------------------------
def lift(pixels, rays_o, rays_d, depth, H, W):
    """o + d * depth at the clicked pixels, in float64; NaN for a click outside the image."""
    out = np.full((len(pixels), 3), np.nan)
    for m, (x, y) in enumerate(pixels):
        if 0 <= x < W and 0 <= y < H:
            n = y * W + x
            out[m] = rays_o[n].astype(np.float64) + rays_d[n].astype(np.float64) * float(depth.reshape(-1)[n])
    return out


def store_update(xyz, labels, crucial, count, cap, point, label, thresh):
    """One click on a store of `count` points: returns (xyz, labels, crucial, count, status) with status = (what, before, after, overflow)
    and the smallest | distance - thresh | seen (inf on an empty store)."""
    xyz, labels, crucial = xyz.copy(), labels.copy(), crucial.copy()
    d = np.linalg.norm(xyz[:count].astype(np.float64) - point.astype(np.float64), axis=-1)
    margin = float(np.abs(d - thresh).min()) if count else np.inf
    far = d > thresh
    if far.all():
        if count == cap:
            return xyz, labels, crucial, count, (3, count, count, 1), margin
        xyz[count], labels[count], crucial[count] = point, label, 0
        return xyz, labels, crucial, count + 1, (0 if count == 0 else 1, count, count + 1, 0), margin
    k = int(far.sum())
    xyz[:k], labels[:k], crucial[:k] = xyz[:count][far], labels[:count][far], crucial[:count][far]
    return xyz, labels, crucial, k, (2, count, k, 0), margin


# ---- projection -----------------------------------------------------------------------------------------------------------------------
def cam_uv(points, pose, intr, W):
    """Camera coordinates [N,3] and pixel coordinates [N,2] in float64 (numpy.linalg.inv of the 4 x 4 pose)."""
    X = np.linalg.inv(pose.reshape(4, 4).astype(np.float64))
    p4 = np.concatenate([points.astype(np.float64), np.ones((len(points), 1))], -1)
    cam = p4 @ X.T
    fx, fy, cx, cy = (float(v) for v in intr)
    with np.errstate(all="ignore"):
        uv = np.stack([W - (fx * cam[:, 0] / cam[:, 2] + cx), fy * cam[:, 1] / cam[:, 2] + cy], -1)
    return cam[:, :3], uv


def _abs_lu(A):
    """|L| |U| of an LU factorisation with partial pivoting of A (float64), rows back in A's order."""
    n = len(A)
    U_, L, perm = A.astype(np.float64).copy(), np.eye(n), np.arange(n)
    for k in range(n - 1):
        piv = k + int(np.argmax(np.abs(U_[k:, k])))
        if piv != k:
            U_[[k, piv]] = U_[[piv, k]]
            L[[k, piv], :k] = L[[piv, k], :k]
            perm[[k, piv]] = perm[[piv, k]]
        for i in range(k + 1, n):
            L[i, k] = U_[i, k] / U_[k, k]
            U_[i] -= L[i, k] * U_[k]
    out = np.empty((n, n))
    out[perm] = np.abs(L) @ np.abs(np.triu(U_))
    return out


def cam_uv_bound(points, pose, intr, W):
    """(E_cam [N,3], E_uv [N,2]): the module docstring's bound for an fp32 evaluation."""
    A = pose.reshape(4, 4).astype(np.float64)
    X = np.abs(np.linalg.inv(A))
    EX = 3 * gamma(4) * (X @ _abs_lu(A) @ X) + gamma(4) * X
    p4 = np.concatenate([np.abs(points.astype(np.float64)), np.ones((len(points), 1))], -1)
    e_cam = (p4 @ EX.T)[:, :3]
    cam, uv = cam_uv(points, pose, intr, W)
    fx, fy, cx, cy = (abs(float(v)) for v in intr)
    z, ez = np.abs(cam[:, 2]), e_cam[:, 2]
    e_uv = np.full((len(points), 2), np.inf)
    ok = z > ez
    for j, (f, c0) in enumerate(((fx, cx), (fy, cy))):
        c, ec = np.abs(cam[ok, j]), e_cam[ok, j]
        q = f * c / z[ok]
        eq = f * (ec / (z[ok] - ez[ok]) + c * ez[ok] / (z[ok] * (z[ok] - ez[ok]))) + gamma(2) * q
        s = q + c0                                                         # an upper bound of |s|
        e = eq + U * (s + eq)
        if j == 0:
            e = e + U * (W + s + eq)
        e_uv[ok, j] = e
    return e_cam, e_uv


def pixel_margin(uv):
    """Distance of every coordinate from the nearest integer -- which covers -1, W and H -- the smallest per point."""
    return np.abs(uv - np.rint(uv)).min(-1)


def project_view(points, labels, crucial, n_points, pose, intr, depth, H, W, depth_tol, crucial_count, valid_threshold, ratio):
    """One view of sn_rm_points_project in float64: dict of coords, labels, kept_index, sam_coords, overlay_coords [N,..] (the tail filled),
    state [N], counts [4], cam, uv, and the two margins (pixel, depth) of the points in play."""
    N = len(points)
    cam, uv = cam_uv(points, pose, intr, W)
    live = np.arange(N) < n_points
    on = live & (uv[:, 0] > -1) & (uv[:, 0] < W) & (uv[:, 1] > -1) & (uv[:, 1] < H)      # a NaN fails every comparison
    pix = np.zeros((N, 2), dtype=np.int64)
    pix[on] = np.trunc(uv[on]).astype(np.int64)
    seen = depth.reshape(H, W)[pix[:, 1], pix[:, 0]].astype(np.float64)
    with np.errstate(invalid="ignore"):
        gap = np.abs(-cam[:, 2] - seen)
        kept = on & (gap <= depth_tol)
    state = np.where(kept, 2, np.where(on, 1, 0)).astype(np.int32)
    idx = np.flatnonzero(kept)
    k = len(idx)
    out = dict(coords=np.zeros((N, 2), np.int32), labels=np.full(N, -1, np.int32), kept_index=np.full(N, -1, np.int32),
               sam_coords=np.zeros((N, 2), np.int32), overlay_coords=np.zeros((N, 2), np.int32), state=state, cam=cam, uv=uv)
    out["coords"][:k], out["labels"][:k], out["kept_index"][:k] = pix[idx], labels[idx], idx
    if ratio:
        sam = (pix[idx].astype(np.float32) * np.float32(ratio)).astype(np.int32)              # trainer.py:872-875 as numpy evaluates them
        out["sam_coords"][:k] = sam
        out["overlay_coords"][:k] = (sam / ratio).astype(np.int32)
    ck = int((crucial[idx] != 0).sum()) if crucial is not None else 0
    out["counts"] = np.array([int(on.sum()), k, ck, int(k > 0 and ck >= crucial_count and k >= valid_threshold)], dtype=np.int32)
    out["margin_pixel"] = float(pixel_margin(uv[live]).min()) if live.any() else np.inf
    out["margin_depth"] = float(np.abs(gap[on] - depth_tol).min()) if on.any() else np.inf
    return out


# ---- overlay --------------------------------------------------------------------------------------------------------------------------
def select_mask(scores):
    """trainer.py:979-984: the first score above the running maximum, which starts at 0 with index 0."""
    best, sel = 0.0, 0
    for j, s in enumerate(scores):
        if s > best:
            best, sel = s, j
    return sel


def overlay(image, H, W, coords, labels, count, radius, alpha, masks=None, scores=None, mask_index=0):
    """sn_rm_prompt_overlay: (rgb [H,W,3] float64, rgb as the fp32 chain fl(fl(image a) + fl(over b)) evaluates it, pred_mask [H,W] bool,
    selected).  The rectangles are numpy slices, which are Python's."""
    img = image.reshape(H, W, 3)
    if count == 0:
        return img.astype(np.float64), img.copy(), np.zeros((H, W), bool), -1
    rgb64, rgb32, pred, sel = img.astype(np.float64), img.astype(np.float32).copy(), np.zeros((H, W), bool), -1
    if masks is not None:
        sel = select_mask(scores) if scores is not None else mask_index
        pred = masks[sel].astype(bool)
        a32, b32 = np.float32(alpha), np.float32(1.0 - alpha)
        over64, over32 = rgb64.copy(), rgb32.copy()
        over64[pred], over32[pred] = (1.0, 0.0, 0.0), (1.0, 0.0, 0.0)
        rgb64 = rgb64 * float(a32) + over64 * float(b32)
        rgb32 = rgb32 * a32 + over32 * b32
    for (x, y), lb in zip(coords[:count], labels[:count]):
        colour = (0.0, 1.0, 0.0) if lb == 0 else (1.0, 0.0, 0.0)
        m = np.zeros((H, W), bool)
        m[int(y) - radius:int(y) + radius, int(x) - radius:int(x) + radius] = True
        rgb64[m], rgb32[m] = colour, colour
    return rgb64, rgb32, pred, sel


def rgb8(rgb):
    return np.trunc(np.clip(255.0 * np.asarray(rgb, dtype=np.float64), 0, 255)).astype(np.uint8)
