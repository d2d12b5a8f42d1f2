"""3D point prompts: lift, store, projection into views, decode overlays (prompts.hip)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .. import _lib
from ._args import _f32, _i32, _image_rows, _outputs, _pixel_values


def points_lift(pixels, rays_o, rays_d, depth, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Clicked pixels -> 3D points (sn_rm_points_lift; nerf/trainer.py:803-809): pixels [M,2] (x, y) on the device, rays_o / rays_d [H*W,3],
    depth H*W values ([H,W], or the depth column of the packed render buffer read in place) -> [M,3] = o + d * depth.  A click outside
    the image gives NaN."""
    H, W = int(H), int(W)
    px = _i32(pixels.reshape(-1, 2), "pixels")
    M = px.shape[0]
    ro, rd = _f32(rays_o.reshape(-1, 3)), _f32(rays_d.reshape(-1, 3))
    ro_ptr, rd_ptr = _lib.dev(ro, "rays_o"), _lib.dev(rd, "rays_d")
    if ro.shape[0] != H * W or rd.shape[0] != H * W:
        raise RuntimeError(f"points_lift: {ro.shape[0]} / {rd.shape[0]} rays for a {H} x {W} image")
    d, d_ptr, d_stride = _pixel_values(depth, "depth", H * W)
    if out is None:
        out = torch.empty(M, 3, device=px.device, dtype=torch.float32)
    elif tuple(out.shape) != (M, 3):
        raise RuntimeError(f"points_lift: out must be [{M},3], got {tuple(out.shape)}")
    _lib.check(_lib.lib().sn_rm_points_lift(px.data_ptr(), M, ro_ptr, rd_ptr, d_ptr, d_stride, H, W, _lib.dev(out, "out"), _lib.stream()), "points_lift")
    return out


def point_store(device, capacity: int = 256) -> Dict[str, torch.Tensor]:
    """An empty fixed-capacity store of remembered points on the device: 'xyz' [cap,3], 'labels' / 'crucial' [cap] int32, 'count' [1] int32
    and the 'status' [4] int32 record of point_store_update."""
    cap = int(capacity)
    if not 1 <= cap <= _lib.PROMPT_MAX_POINTS:
        raise ValueError(f"point_store: capacity {capacity} outside 1..{_lib.PROMPT_MAX_POINTS}")
    z = lambda *s, dt=torch.int32: torch.zeros(*s, device=device, dtype=dt)
    return {"xyz": z(cap, 3, dt=torch.float32), "labels": z(cap), "crucial": z(cap), "count": z(1), "status": z(4)}


def point_store_update(store: Dict[str, torch.Tensor], point, label, dist_thresh: float = 0.01) -> None:
    """The add-or-remove rule of the remembered points for one new point (sn_rm_point_store_update; trainer.py:812-834), one launch, no
    host read: point [3] (or [1,3]) on the device; label: an int, or a one-element device tensor.  store['status'] = {0 first / 1 appended
    / 2 removed / 3 full, count before, count after, overflow (only ever set)}."""
    xyz = store["xyz"]
    cap = xyz.shape[0]
    p = _f32(point.reshape(-1))
    p_ptr = _lib.dev(p, "point")
    if p.numel() != 3:
        raise RuntimeError(f"point_store_update: one point of 3 coordinates, got {tuple(point.shape)}")
    if torch.is_tensor(label):
        lb = _i32(label.reshape(-1)[:1], "label")
    else:
        lb = torch.empty(1, device=xyz.device, dtype=torch.int32).fill_(int(label))      # a fill, not a copy: it can be captured
    _lib.check(_lib.lib().sn_rm_point_store_update(_lib.dev(xyz, "xyz"), _lib.dev(store["labels"], "labels", torch.int32),
                                                   _lib.dev(store["crucial"], "crucial", torch.int32), _lib.dev(store["count"], "count", torch.int32),
                                                   cap, p_ptr, lb.data_ptr(), float(dist_thresh), _lib.dev(store["status"], "status", torch.int32),
                                                   _lib.stream()), "point_store_update")


def reference_resize_ratio(H: int, W: int) -> float:
    """trainer.py:871 / :973: the factor into SAM's 1024-pixel frame."""
    return 1024 / W if W > H else 1024 / H


def points_project(points, labels, poses, intrinsics, depth, H: int, W: int, crucial=None, n_points=None, depth_tol: float = 0.05,
                   crucial_count: int = 0, valid_threshold: int = 0, resize_ratio: Optional[float] = None,
                   want: Sequence[str] = ("cam", "uv", "state"), out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """The remembered points in V views, one launch and no host read (sn_rm_points_project; trainer.py:838-875, 931-976): points [N,3],
    labels [N], crucial [N] or None, n_points: a one-element int32 device tensor (a store's count) or None; poses [V,4,4] (or [4,4])
    cam2world, intrinsics [4] or [V,4]; depth V*H*W values ([V,H,W], [H,W], or the depth column of the packed render buffer read in place).
    Returns 'coords' [V,N,2] / 'labels' [V,N] / 'kept_index' [V,N] (the kept points first, in their order; behind them 0 / -1 / -1),
    'sam_coords' / 'overlay_coords' [V,N,2] (resize_ratio None: the reference's 1024 / max(H, W); 0: left out), 'counts' [V,4] = {on screen,
    kept, crucial kept, is_valid}, and of `want`: 'cam' [V,N,3], 'uv' [V,N,2], 'state' [V,N] (0 off screen, 1 occluded, 2 kept)."""
    H, W = int(H), int(W)
    unknown = set(want) - {"cam", "uv", "state"}
    if unknown:
        raise ValueError(f"points_project: unknown outputs {sorted(unknown)}")
    pts = _f32(points.reshape(-1, 3))
    pts_ptr = _lib.dev(pts, "points")
    N, dev = pts.shape[0], pts.device
    lb = _i32(labels.reshape(-1), "labels", (N,))
    cr = None if crucial is None else _i32(crucial.reshape(-1), "crucial", (N,))
    npts = None if n_points is None else _i32(n_points.reshape(-1)[:1], "n_points", (1,))
    ps = _f32(poses.reshape(-1, 16))
    ps_ptr = _lib.dev(ps, "poses")
    V = ps.shape[0]
    ks = _f32(intrinsics.reshape(-1, 4))
    ks_ptr = _lib.dev(ks, "intrinsics")
    if ks.shape[0] not in (1, V):
        raise RuntimeError(f"points_project: {ks.shape[0]} intrinsics for {V} views (1 or V)")
    d, d_ptr, d_stride = _pixel_values(depth, "depth", V * H * W)
    ratio = reference_resize_ratio(H, W) if resize_ratio is None else float(resize_ratio)
    names = ["coords", "labels", "kept_index", "counts"] + (["sam_coords", "overlay_coords"] if ratio > 0 else []) + list(want)
    i32, f32 = torch.int32, torch.float32
    specs = {"coords": ((V, N, 2), i32), "labels": ((V, N), i32), "kept_index": ((V, N), i32), "sam_coords": ((V, N, 2), i32),
             "overlay_coords": ((V, N, 2), i32), "cam": ((V, N, 3), f32), "uv": ((V, N, 2), f32), "state": ((V, N), i32), "counts": ((V, 4), i32)}
    res, ptr = _outputs("points_project", specs, names, out, dev)
    _lib.check(_lib.lib().sn_rm_points_project(pts_ptr, lb.data_ptr(), None if cr is None else cr.data_ptr(), N, None if npts is None else npts.data_ptr(),
                                               ps_ptr, V, ks_ptr, ks.shape[0], d_ptr, d_stride, H, W, float(depth_tol), int(crucial_count),
                                               int(valid_threshold), ratio, ptr["coords"], ptr["labels"], ptr["kept_index"], ptr["sam_coords"],
                                               ptr["overlay_coords"], ptr["cam"], ptr["uv"], ptr["state"], ptr["counts"], _lib.stream()), "points_project")
    return res


def prompt_overlay(image, coords, labels, H: int, W: int, count=None, masks=None, scores=None, mask_index: int = 0, radius: int = 2,
                   alpha: float = 0.7, want: Sequence[str] = ("rgb", "pred_mask"), out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """decode_step's tail in one launch (sn_rm_prompt_overlay; trainer.py:979-991, nerf/utils.py:23-29, 80-98): image [H*W,3] / [H,W,3]
    (rows may be strided: the packed render buffer is read in place), coords [N,2] (x, y) and labels [N] int32, count: a one-element int32
    device tensor or None (= N); masks [M,H,W] bool / uint8 or None, scores [M] on the device (the first score above the running maximum,
    which starts at 0) or None with a fixed mask_index.  Returns of `want`: 'rgb' [H,W,3] (the selected mask blended in red at 1 - alpha,
    the points as squares: green for label 0, red otherwise, drawn with the reference's Python-slice bounds, the last point on top),
    'rgb8' [H,W,3] uint8, 'pred_mask' [H,W] bool (the selected mask), and always 'selected' [1] int32.  count == 0: the image unchanged,
    an empty mask, selected -1."""
    H, W = int(H), int(W)
    unknown = set(want) - {"rgb", "rgb8", "pred_mask"}
    if unknown:
        raise ValueError(f"prompt_overlay: unknown outputs {sorted(unknown)}")
    img, img_ptr, img_stride = _image_rows(image, "image", H * W)
    dev = img.device
    xy = _i32(coords.reshape(-1, 2), "coords")
    N = xy.shape[0]
    lb = _i32(labels.reshape(-1), "labels", (N,))
    cnt = None if count is None else _i32(count.reshape(-1)[:1], "count", (1,))
    m, M, sc = None, 0, None
    if masks is not None:
        if not masks.is_cuda:
            raise RuntimeError("masks must be a CUDA tensor")
        m = masks.detach().reshape(-1, H, W).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8)
        M = m.shape[0]
        if scores is not None:
            sc = _f32(scores.reshape(-1))
            if not sc.is_cuda:
                raise RuntimeError("scores must be a CUDA tensor")
            if sc.shape[0] != M:
                raise RuntimeError(f"prompt_overlay: {sc.shape[0]} scores for {M} masks")
    specs = {"rgb": ((H, W, 3), torch.float32), "rgb8": ((H, W, 3), torch.uint8), "pred_mask": ((H, W), torch.bool), "selected": ((1,), torch.int32)}
    res, ptr = _outputs("prompt_overlay", specs, list(want) + ["selected"], out, dev)
    _lib.check(_lib.lib().sn_rm_prompt_overlay(img_ptr, img_stride, H, W, None if m is None else m.data_ptr(), M, None if sc is None else sc.data_ptr(),
                                               int(mask_index), xy.data_ptr(), lb.data_ptr(), N, None if cnt is None else cnt.data_ptr(), int(radius),
                                               float(alpha), ptr["rgb"], ptr["rgb8"], ptr["pred_mask"], ptr["selected"], _lib.stream()), "prompt_overlay")
    return res
