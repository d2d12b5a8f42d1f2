"""A training batch drawn on the device (collate.hip)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from .. import _lib
from ._args import _f32_rows, _row_strided


def weighted_draw(weights, expo, n: int, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                  row_u: Optional[torch.Tensor] = None, row_index: Optional[torch.Tensor] = None):
    """Weighted sampling without replacement from caller-supplied exponential variates (sn_rm_weighted_draw; torch.multinomial's own
    exponential race, utils.py:218, :248): weights [R,C], expo [R,C] (e.g. torch.empty(R, C).exponential_()) -> (out [R,n] int64, status [1]
    int32).  Per row the n cells with the smallest expo / weights, ties to the smaller cell, in ASCENDING CELL ORDER (torch: key order).  A
    cell with weight <= 0 or NaN, or with a key that is not finite, is never drawn; a row with fewer than n such cells gets -1 in its tail
    and sets the sticky status word (torch raises).  row_u [R] in [0,1): row r draws from row min(int(row_u[r] * M), M - 1) of weights [M,C]
    (the cameras of the local patches, chosen on the device by the same formula as collate_gather's); row_index [R] int64 on the device:
    row r draws from that row of weights [M,C] (a single-image batch's image index).  out / status: static tensors to write into.  One launch, nothing read on the host."""
    w, e = _f32_rows(weights, "weights"), _f32_rows(expo, "expo")
    if w.dim() != 2 or e.dim() != 2 or w.shape[1] != e.shape[1]:
        raise RuntimeError(f"weighted_draw: weights {tuple(w.shape)} and expo {tuple(e.shape)} must be [rows, C] with one C")
    R, Cn, n = e.shape[0], e.shape[1], int(n)
    M = w.shape[0]
    ru_ptr = ri_ptr = None
    if row_index is not None:
        if row_u is not None:
            raise RuntimeError("weighted_draw: give row_u or row_index, not both")
        ri = row_index.detach().reshape(-1)
        ri_ptr = _lib.dev(ri, "row_index", torch.int64)
        if ri.numel() != R:
            raise RuntimeError(f"weighted_draw: row_index has {ri.numel()} entries for {R} rows")
    elif row_u is None:
        if M != R:
            raise RuntimeError(f"weighted_draw: {M} rows of weights for {R} rows of expo (give row_u or row_index to draw from chosen rows)")
    else:
        ru = _f32_rows(row_u, "row_u")
        if ru.numel() != R:
            raise RuntimeError(f"weighted_draw: row_u has {ru.numel()} entries for {R} rows")
        ru_ptr = ru.data_ptr()
    if out is None:
        out = torch.empty(R, max(n, 0), device=w.device, dtype=torch.int64)
    elif tuple(out.shape) != (R, n):
        raise RuntimeError(f"weighted_draw: out must be [{R},{n}], got {tuple(out.shape)}")
    if status is None:
        status = torch.zeros(1, device=w.device, dtype=torch.int32)
    _lib.check(_lib.lib().sn_rm_weighted_draw(w.data_ptr(), e.data_ptr(), R, Cn, n, ru_ptr, ri_ptr, M, _lib.dev(out, "out", torch.int64),
                                              _lib.dev(status, "status", torch.int32), _lib.stream()), "weighted_draw")
    return out, status


COLLATE_OUTPUTS = {"rays_o": (3, torch.float32), "rays_d": (3, torch.float32), "index": (1, torch.int64), "i": (1, torch.int64),
                   "j": (1, torch.int64), "inds_coarse": (1, torch.int64), "images": (None, torch.float32), "masks": (None, None),
                   "error_maps": (1, torch.float32), "cam_near_far": (2, torch.float32), "poses": (16, torch.float32),
                   "intrinsics": (4, torch.float32)}


def collate_gather(poses, intrinsics, H: int, W: int, u=None, cells=None, index=0, images=None, masks=None, error_map=None, cam_near_far=None,
                   error_map_size: int = 0, coarse_size: Optional[int] = None, ul=None, centres=None, patch_size: int = 1,
                   out: Optional[Dict[str, torch.Tensor]] = None, want: Optional[Sequence[str]] = None) -> Dict[str, torch.Tensor]:
    """Draw -> rays + supervision in one launch (sn_rm_collate_gather; provider.py:908-1068, utils.py:209-300), the dataset tensors read in
    place: poses [M,4,4], intrinsics [1|M,4], images [M,H,W,3|4] uint8, masks [M,H,W,Cm] (uint8 / float32 / int64 ...: copied as raw
    bytes), error_map [M,S*S] with S = error_map_size, cam_near_far [M,2].
      main part: u [N,3] in [0,1) -> camera, row, column per ray (random_image_batch); or cells [N] (weighted_draw over image `index`'s
      error-map row; index: an int or a one-element int64 device tensor) with u [N,2]: a pixel inside each drawn cell;
      local part: ul [L] and centres [L] (weighted_draw(error_map, expo, 1, row_u=ul)): L patches of patch_size^2 rays behind the main part.
    Outputs (COLLATE_OUTPUTS) over the N + L patch_size^2 rays, 'images' over the first N: those named in `want` are allocated, those given
    in `out` are written in place -- [rows, width] or [rows] tensors that may be columns of a wider buffer (row stride = its width).
    Default: every output the given dataset tensors allow.  inds_coarse: the drawn cell in error-map mode, else the pixel's cell in a map of
    coarse_size (default error_map_size, or H without one, as collate_rays)."""
    H, W = int(H), int(W)
    P = _f32_rows(poses, "poses", 16)
    K = _f32_rows(intrinsics, "intrinsics", 4)
    dev, M = P.device, P.shape[0]
    d = _lib.CollateDesc()
    keep = []
    d.poses, d.intrinsics, d.M, d.n_intrinsics, d.H, d.W = P.data_ptr(), K.data_ptr(), M, K.shape[0], H, W
    S = int(error_map_size)
    d.S, d.coarse_size = S, int(coarse_size) if coarse_size is not None else (S if S > 0 else H)
    avail = {"rays_o", "rays_d", "index", "i", "j", "inds_coarse", "poses", "intrinsics"}
    widths = {k: v[0] for k, v in COLLATE_OUTPUTS.items()}
    dtypes = {k: v[1] for k, v in COLLATE_OUTPUTS.items()}
    if images is not None:
        if images.dim() != 4 or tuple(images.shape[:3]) != (M, H, W):
            raise RuntimeError(f"collate_gather: images must be [{M},{H},{W},3|4], got {tuple(images.shape)}")
        d.images, d.image_channels = _lib.dev(images, "images", torch.uint8), images.shape[3]
        widths["images"] = images.shape[3]
        avail.add("images")
    if masks is not None:
        if masks.dim() != 4 or tuple(masks.shape[:3]) != (M, H, W):
            raise RuntimeError(f"collate_gather: masks must be [{M},{H},{W},C], got {tuple(masks.shape)}")
        d.masks, d.mask_channels, d.mask_elem_bytes = _lib.dev(masks, "masks", None), masks.shape[3], masks.element_size()
        widths["masks"], dtypes["masks"] = masks.shape[3], masks.dtype
        avail.add("masks")
    if error_map is not None:
        if S < 1 or error_map.numel() != M * S * S:
            raise RuntimeError(f"collate_gather: error_map must hold {M} x {S}^2 values (error_map_size), got {tuple(error_map.shape)}")
        d.error_map = _f32_rows(error_map, "error_map").data_ptr()
        avail.add("error_maps")
    if cam_near_far is not None:
        d.cam_near_far = _f32_rows(cam_near_far, "cam_near_far", 2).data_ptr()
        if cam_near_far.numel() != 2 * M:
            raise RuntimeError(f"collate_gather: cam_near_far must be [{M},2], got {tuple(cam_near_far.shape)}")
        avail.add("cam_near_far")
    N = 0
    if u is not None:
        uu = _f32_rows(u, "u")
        if cells is not None:
            cl = cells.detach().reshape(-1)
            N = cl.shape[0]
            d.cells, d.mode = _lib.dev(cl, "cells", torch.int64), _lib.COLLATE_ERROR_MAP
            if torch.is_tensor(index):
                d.index_dev = _lib.dev(index, "index", torch.int64)
            else:
                d.index = int(index)
            cols = 2
        else:
            N, cols = uu.shape[0], 3
        if uu.dim() != 2 or tuple(uu.shape) != (N, cols):
            raise RuntimeError(f"collate_gather: u must be [{N},{cols}], got {tuple(uu.shape)}")
        d.u = uu.data_ptr()
        keep.append(uu)
    elif cells is not None:
        raise RuntimeError("collate_gather: cells without u (the position inside each drawn cell)")
    d.N = N
    L, p = 0, int(patch_size)
    if ul is not None or centres is not None:
        if ul is None or centres is None:
            raise RuntimeError("collate_gather: the local part needs both ul and centres")
        lu, cen = _f32_rows(ul, "ul").reshape(-1), centres.detach().reshape(-1)
        L = lu.shape[0]
        if cen.shape[0] != L:
            raise RuntimeError(f"collate_gather: {cen.shape[0]} centres for {L} patches")
        d.ul, d.centres = lu.data_ptr(), _lib.dev(cen, "centres", torch.int64)
        keep += [lu, cen]
    d.L, d.p = L, p
    total = N + L * p * p
    res = {} if out is None else out
    unknown = (set(res) | set(want or ())) - set(COLLATE_OUTPUTS)
    if unknown:
        raise ValueError(f"collate_gather: unknown outputs {sorted(unknown)}; known: {sorted(COLLATE_OUTPUTS)}")
    names = set(res) | (set(want) if want is not None else (avail if out is None else set()))
    missing = names - avail
    if missing:
        raise RuntimeError(f"collate_gather: outputs {sorted(missing)} need the dataset tensor they are gathered from")
    for name in sorted(names):
        rows = N if name == "images" else total
        t = res.get(name)
        if t is None:
            shape = (rows,) if widths[name] == 1 and name != "masks" else (rows, widths[name])
            t = res[name] = torch.empty(shape, device=dev, dtype=dtypes[name])
        ptr, stride = _row_strided(t, name, rows, widths[name], dtypes[name])
        field = name if name in ("rays_o", "rays_d", "inds_coarse") else name + "_out"
        setattr(d, field, ptr)
        setattr(d, name + "_stride", stride)
    _lib.check(_lib.lib().sn_rm_collate_gather(C.byref(d), _lib.stream()), "collate_gather")
    return res
