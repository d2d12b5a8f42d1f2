"""Render a segmented object alone (object.hip): the gated re-integration of the last stage's samples.

    object_composite     labels, sigmas, real_bins, geo_feat, rays_d -> weights_sum, depth, f_image [, weights] of the samples whose label is
                         in the kept set (or, inverted, is not): include/sanerf_hip.h states the definition, tests/object_ref64.py its fp64 twin
    keep_mask_of         a collection of instance ids -> the 32-bit keep mask
"""
from __future__ import annotations

from typing import Iterable

import torch

from .. import _lib
from ._args import _f32

OBJECT_MAX_IDS = 32        # instance ids of a keep mask: 0 .. 31
OBJECT_GEO = 15            # geometry channels per sample (network.py:94)
LABEL_SKIPPED = 255        # sn_rm_mask_point_labels: the sample's tile was not evaluated (only where delta * sigma == 0)


def keep_mask_of(instance_ids: Iterable[int]) -> int:
    """The 32-bit keep mask of a set of instance ids (each in 0..31)."""
    mask = 0
    for i in instance_ids:
        i = int(i)
        if not 0 <= i < OBJECT_MAX_IDS:
            raise ValueError(f"instance id {i} outside 0..{OBJECT_MAX_IDS - 1}")
        mask |= 1 << i
    return mask


def object_composite(labels: torch.Tensor, sigmas: torch.Tensor, real_bins: torch.Tensor, geo_feat: torch.Tensor, rays_d: torch.Tensor,
                     keep_mask: int, invert: bool = False, last_sample_opaque: bool = False, want_weights: bool = False):
    """One launch: labels [N,T] uint8, sigmas [N,T], real_bins [N,T+1], geo_feat [N,T,15], rays_d [N,3] ->
    (weights_sum [N], depth [N], f_image [N,31]) and, with want_weights, the gated weights w' [N,T] as a fourth value.
    g = (label in keep_mask) xor invert; y = g ? delta * sigma : 0 (last_sample_opaque: the last sample's y = g ? inf : 0);
    w' = (1 - exp(-y)) exp(-sum of the y in front), NaN -> 0.  A label >= 32 (255) is in no set.  No autograd."""
    N, T = sigmas.shape
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (N, T):
        raise RuntimeError(f"object_composite: labels must be uint8 [{N},{T}], got {labels.dtype} {tuple(labels.shape)}")
    if tuple(real_bins.shape) != (N, T + 1) or tuple(geo_feat.shape) != (N, T, OBJECT_GEO) or tuple(rays_d.shape) != (N, 3):
        raise RuntimeError(f"object_composite: real_bins {tuple(real_bins.shape)} / geo_feat {tuple(geo_feat.shape)} / rays_d {tuple(rays_d.shape)} "
                           f"do not match sigmas [{N},{T}] (geo_feat has {OBJECT_GEO} channels)")
    if not 0 <= int(keep_mask) < (1 << 32):
        raise ValueError("object_composite: keep_mask is a 32-bit mask")
    lb, sg, rb, gf, rd = labels.detach().contiguous(), _f32(sigmas), _f32(real_bins), _f32(geo_feat), _f32(rays_d)
    dev = sg.device
    wsum = torch.empty(N, device=dev, dtype=torch.float32)
    depth = torch.empty(N, device=dev, dtype=torch.float32)
    f_image = torch.empty(N, 16 + OBJECT_GEO, device=dev, dtype=torch.float32)
    weights = torch.empty(N, T, device=dev, dtype=torch.float32) if want_weights else None
    _lib.check(_lib.lib().sn_rm_object_composite(_lib.dev(lb, "labels", torch.uint8), _lib.dev(sg, "sigmas"), _lib.dev(rb, "real_bins"),
                                                 _lib.dev(gf, "geo_feat"), _lib.dev(rd, "rays_d"), N, T, int(keep_mask), int(bool(invert)),
                                                 int(bool(last_sample_opaque)), _lib.dev(wsum, "weights_sum"), _lib.dev(depth, "depth"),
                                                 _lib.dev(f_image, "f_image"), _lib.dev(weights, "weights"), _lib.stream()),
               "sn_rm_object_composite")
    return (wsum, depth, f_image, weights) if want_weights else (wsum, depth, f_image)
