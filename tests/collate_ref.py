"""A numpy restatement of the device-side batch draw (sn_rm_weighted_draw, sn_rm_collate_gather; include/sanerf_hip.h), with float32
arithmetic exactly as the header specifies it and integer outputs -- what the GPU tests compare the kernels with, bit for bit.

    weighted_draw(weights, expo, n, row_u=None, row_index=None) -> (out [R,n] int64, status)
    gather(data, H, W, ...)                         -> dict of arrays over the N + L p^2 rays
    rays_of_pixels(poses, intrinsics, cam, row, col)-> rays_o, rays_d (the operation sequence of sn_rm_rays_from_pixels, fmaf included)
"""
import numpy as np

F = np.float32
INF_BITS = 0x7F800000


def pick(u, n):
    """min((int)(u * n), n - 1) with the product in fp32; a u outside [0, 1) or a NaN lands inside 0 .. n-1."""
    return trunc_below(np.asarray(u, dtype=F) * F(n), n)


def trunc_below(f, n):
    f = np.asarray(f, dtype=F)
    inside = (f >= 0) & (f < F(n))
    return np.where(inside, np.where(inside, f, 0).astype(np.int64), np.where(f >= F(n), n - 1, 0)).astype(np.int64)


def key_bits(weights, expo):
    """The key expo / weights (fp32, IEEE) as its bit pattern, -0 as 0; 0xffffffff for a cell that is never selected."""
    w, e = np.asarray(weights, dtype=F), np.asarray(expo, dtype=F)
    with np.errstate(all="ignore"):
        key = (e / w).astype(F)
    bits = np.where(key == 0, F(0), key).view(np.uint32).astype(np.int64)
    return np.where((w > 0) & (bits < INF_BITS), bits, 0xFFFFFFFF)


def weighted_draw(weights, expo, n, row_u=None, row_index=None):
    """Per row the n smallest (key, cell), in ascending cell order; -1 behind a row's selectable cells, status 1 if a row fell short."""
    weights, expo = np.asarray(weights, dtype=F), np.asarray(expo, dtype=F)
    R, C = expo.shape
    rows = np.arange(R) if row_u is None else pick(row_u, weights.shape[0])
    if row_index is not None:
        rows = np.clip(np.asarray(row_index, dtype=np.int64).reshape(R), 0, weights.shape[0] - 1)
    out, status = np.full((R, n), -1, dtype=np.int64), 0
    for r in range(R):
        bits = key_bits(weights[rows[r]], expo[r])
        order = np.lexsort((np.arange(C), bits))                     # by key, then by cell
        order = order[bits[order] != 0xFFFFFFFF][:n]
        out[r, :len(order)] = np.sort(order)
        status |= int(len(order) < n)
    return out, status


def fmaf(a, b, c):
    """fl32(a * b + c) with ONE rounding: the product of two floats is exact in float64, the sum is rounded to odd (TwoSum tells on which
    side the exact value lies), and 53 bits rounded to odd round correctly to 24."""
    p, c = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    odd = (s.view(np.int64) & 1) == 1
    fix = (err != 0) & ~odd & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s).astype(F)


def rays_of_pixels(poses, intrinsics, cam, row, col):
    """k_rays_from_pixels' sequence: xs = (i - cx) / fx, ys = -(j - cy) / fy, d_k = fma(-1, m_k2, fma(ys, m_k1, xs * m_k0)), o_k = m_k3."""
    poses, intrinsics = np.asarray(poses, dtype=F).reshape(-1, 4, 4), np.asarray(intrinsics, dtype=F).reshape(-1, 4)
    m = poses[cam]
    k4 = intrinsics[cam] if intrinsics.shape[0] > 1 else np.broadcast_to(intrinsics[0], (len(cam), 4))
    i, j = col.astype(F) + F(0.5), row.astype(F) + F(0.5)
    xs = ((i - k4[:, 2]) / k4[:, 0]).astype(F)
    ys = (-(j - k4[:, 3]) / k4[:, 1]).astype(F)
    d = np.empty((len(cam), 3), dtype=F)
    for k in range(3):
        acc = (xs * m[:, k, 0]).astype(F)
        acc = fmaf(ys, m[:, k, 1], acc)
        d[:, k] = fmaf(F(-1), m[:, k, 2], acc)
    return np.ascontiguousarray(m[:, :3, 3]), d


def coarse_index(row, col, H, W, size):
    """utils.py:294-300: (row * (float)(size / H)).long() * size + (col * (float)(size / W)).long()."""
    return (row.astype(F) * F(size / H)).astype(np.int64) * size + (col.astype(F) * F(size / W)).astype(np.int64)


def gather(data, H, W, N, mode="uniform", u=None, cells=None, index=0, S=1, coarse_size=None, L=0, p=1, ul=None, centres=None):
    """data: dict of the dataset arrays (poses [M,4,4], intrinsics [1|M,4]; images, masks, error_map, cam_near_far optional).
    Returns cam, row, col, valid and every output of sn_rm_collate_gather over the N + L p^2 rays (images over the first N)."""
    poses = np.asarray(data["poses"], dtype=F).reshape(-1, 4, 4)
    M = poses.shape[0]
    coarse_size = S if coarse_size is None else coarse_size
    sx, sy = F(H / S), F(W / S)
    if mode == "uniform":
        u = np.asarray(u, dtype=F).reshape(N, 3)
        cam, row, col = pick(u[:, 0], M), pick(u[:, 1], H), pick(u[:, 2], W)
        valid = np.ones(N, dtype=bool)
        coarse = coarse_index(row, col, H, W, coarse_size)
    else:
        u, cells = np.asarray(u, dtype=F).reshape(N, 2), np.asarray(cells, dtype=np.int64).reshape(N)
        cam = np.full(N, min(max(int(index), 0), M - 1), dtype=np.int64)
        valid = (cells >= 0) & (cells < S * S)
        cl = np.where(valid, cells, 0)
        gx, gy = cl // S, cl % S
        row = trunc_below((gx.astype(F) * sx).astype(F) + (u[:, 0] * sx).astype(F), H)
        col = trunc_below((gy.astype(F) * sy).astype(F) + (u[:, 1] * sy).astype(F), W)
        coarse = cells.copy()
    if L > 0:
        pp = p * p
        lcam = pick(np.asarray(ul, dtype=F).reshape(L), M)
        cen = np.asarray(centres, dtype=np.int64).reshape(L)
        lvalid = (cen >= 0) & (cen < S * S)
        cl = np.where(lvalid, cen, 0)
        cx, cy = cl // S, cl % S
        half = F(p // 2)
        ix = np.minimum(np.maximum((cx.astype(F) * sx).astype(F) - half, F(0)), F(H - p - 1)).astype(np.int64)
        iy = np.minimum(np.maximum((cy.astype(F) * sy).astype(F) - half, F(0)), F(W - p - 1)).astype(np.int64)
        di, dj = np.divmod(np.arange(pp), p)                         # meshgrid(indexing="ij") order
        lrow, lcol = (ix[:, None] + di[None]).reshape(-1), (iy[:, None] + dj[None]).reshape(-1)
        cam, row, col = np.concatenate([cam, np.repeat(lcam, pp)]), np.concatenate([row, lrow]), np.concatenate([col, lcol])
        valid = np.concatenate([valid, np.repeat(lvalid, pp)])
        coarse = np.concatenate([coarse, coarse_index(lrow, lcol, H, W, coarse_size)])
    rays_o, rays_d = rays_of_pixels(poses, data["intrinsics"], cam, row, col)
    bad = ~valid
    rays_o[bad], rays_d[bad] = np.nan, np.nan
    res = {"cam": cam, "row": row, "col": col, "valid": valid, "rays_o": rays_o, "rays_d": rays_d, "index": cam.copy(),
           "i": np.where(valid, col, -1), "j": np.where(valid, row, -1), "inds_coarse": np.where(valid, coarse, -1), "poses": poses[cam].reshape(-1, 16)}
    if data.get("images") is not None:
        img = (np.asarray(data["images"])[cam[:N], row[:N], col[:N]].astype(F) / F(255)).astype(F)
        img[bad[:N]] = np.nan
        res["images"] = img
    if data.get("masks") is not None:
        m = np.asarray(data["masks"])[cam, row, col].copy()
        m[bad] = 0
        res["masks"] = m
    if data.get("error_map") is not None:
        gj = np.minimum((row.astype(F) * F(S / H)).astype(np.int64), S - 1)
        gi = np.minimum((col.astype(F) * F(S / W)).astype(np.int64), S - 1)
        e = np.asarray(data["error_map"], dtype=F).reshape(M, -1)[cam, gj * S + gi].copy()
        e[bad] = np.nan
        res["error_maps"] = e
    if data.get("cam_near_far") is not None:
        res["cam_near_far"] = np.asarray(data["cam_near_far"], dtype=F)[cam]
    return res
