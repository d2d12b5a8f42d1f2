"""CPU, through the C ABI: the device-side batch draw (sn_rm_weighted_draw, sn_rm_collate_gather) is exported and declared, validates its
arguments before any launch, and its Python operators refuse CPU tensors and unknown outputs."""
import ctypes
import os
import re

import pytest

from helpers import ROOT

NEW = ("sn_rm_weighted_draw", "sn_rm_collate_gather")


def test_the_two_symbols_are_exported_and_declared():
    from sanerf_hq_amd import _lib, nerf, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/sanerf_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.EXPORTED_SYMBOLS
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12, "the additions are additive: the ABI version stays 12"
    assert re.search(r"#define\s+SN_DRAW_MAX_CELLS\s+%d\b" % _lib.DRAW_MAX_CELLS, hdr)
    assert callable(rm.weighted_draw) and callable(rm.collate_gather) and callable(nerf.DeviceCollate)
    assert "collate.hip" in open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    # the ctypes mirror has the header's fields, in the header's order
    body = re.search(r"typedef struct sn_collate_desc \{(.*?)\} sn_collate_desc;", hdr, re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()))]
    assert names == [f[0] for f in _lib.CollateDesc._fields_]


def desc(**kw):
    from sanerf_hq_amd import _lib
    d = _lib.CollateDesc()
    p = 64
    base = dict(poses=p, intrinsics=p, M=5, n_intrinsics=1, H=48, W=64, N=8, mode=0, u=p, rays_o=p, rays_d=p, rays_o_stride=3, rays_d_stride=3)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_entry_points_validate_their_arguments_before_any_launch():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d = ctypes.c_void_p(64)
    err = l.sn_last_error
    # weighted_draw(weights, expo, R, C, n, row_u, row_index, M, out, status, stream)
    assert l.sn_rm_weighted_draw(None, d, 2, 16, 4, None, None, 2, d, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_weighted_draw(d, None, 2, 16, 4, None, None, 2, d, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 16, 4, None, None, 2, None, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 16, 4, None, None, 2, d, None, None) == -1 and b"NULL" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 16, 0, None, None, 2, d, d, None) == -1 and b"n = 0" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 16, 17, None, None, 2, d, d, None) == -1 and b"n=17" in err() and b"C=16" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 65537, 4, None, None, 2, d, d, None) == -2 and b"C=65537" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 0, 1, None, None, 2, d, d, None) == -1 and b"0 cells" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 16, 4, d, d, 2, d, d, None) == -1 and b"row_index" in err()
    assert l.sn_rm_weighted_draw(d, d, 2, 16, 4, d, None, 0, d, d, None) == -1 and b"M = 0" in err()
    assert l.sn_rm_weighted_draw(None, None, 0, 0, 0, None, None, 0, None, None, None) == 0
    # collate_gather(desc, stream)
    g = lambda **kw: l.sn_rm_collate_gather(ctypes.byref(desc(**kw)), None)
    assert l.sn_rm_collate_gather(None, None) == -1 and b"NULL descriptor" in err()
    assert g(poses=None) == -1 and b"NULL poses" in err()
    assert g(intrinsics=None) == -1 and b"NULL poses" in err()
    assert g(u=None) == -1 and b"NULL u" in err()
    assert g(n_intrinsics=3) == -1 and b"3 intrinsics for 5 images" in err()
    assert g(H=0) == -1 and b"0 x 64" in err()
    assert g(mode=2) == -1 and b"mode 2" in err()
    assert g(mode=1, S=16) == -1 and b"NULL cells" in err()
    assert g(mode=1, S=0, cells=64) == -1 and b"S = 0" in err()
    assert g(mode=1, S=16, cells=64, index=5) == -1 and b"index 5" in err()
    for ch in (0, 1, 2, 5):
        assert g(images=64, images_out=64, images_stride=8, image_channels=ch) == -1 and b"channels (3 or 4)" in err(), ch
    assert g(images_out=64, images_stride=3, image_channels=3) == -1 and b"without the dataset's images" in err()
    assert g(images=64, images_out=64, images_stride=3, image_channels=4) == -1 and b"stride" in err()
    for nb in (0, 2, 3, 16):
        assert g(masks=64, masks_out=64, masks_stride=1, mask_channels=1, mask_elem_bytes=nb) == -1 and b"bytes (1, 4 or 8)" in err(), nb
    assert g(masks=66, masks_out=64, masks_stride=1, mask_channels=1, mask_elem_bytes=8) == -1 and b"aligned" in err()
    assert g(masks=64, masks_out=64, masks_stride=1, mask_channels=2, mask_elem_bytes=4) == -1 and b"stride" in err()
    assert g(error_maps_out=64, error_maps_stride=1, S=16) == -1 and b"error map" in err()
    assert g(cam_near_far_out=64, cam_near_far_stride=2) == -1 and b"cam_near_far" in err()
    assert g(rays_d_stride=2) == -1 and b"stride" in err()
    assert g(L=2, p=4, S=16) == -1 and b"NULL ul" in err()
    assert g(L=2, p=0, S=16, ul=64, centres=64) == -1 and b"0 x 0" in err()
    for p in (48, 49, 100):                                          # p >= H
        assert g(L=2, p=p, S=16, ul=64, centres=64) == -1 and b"does not fit" in err(), p
    assert g(L=2, p=47, S=16, ul=64, centres=64, W=47) == -1 and b"does not fit" in err()
    assert g(H=1 << 24) == -2 and b"2^24" in err()
    assert g(N=0, poses=None) == 0                                   # an empty batch touches nothing
    assert l.sn_abi_version() == 12


def test_python_operators_refuse_cpu_tensors_and_bad_options():
    import torch
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import DeviceCollate
    w = torch.rand(2, 16)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.weighted_draw(w, w, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.collate_gather(torch.eye(4)[None], torch.rand(1, 4), 8, 8, u=torch.rand(4, 3))
    with pytest.raises(RuntimeError, match="error map"):
        DeviceCollate(torch.eye(4)[None], torch.rand(1, 4), 8, 8, 16, num_local_sample=2, local_patch_size=2)
    with pytest.raises(RuntimeError, match="use_error_map"):
        DeviceCollate(torch.eye(4)[None], torch.rand(1, 4), 8, 8, 16, random_image_batch=False)
    assert set(rm.COLLATE_OUTPUTS) >= {"rays_o", "rays_d", "index", "i", "j", "inds_coarse", "images", "masks", "error_maps", "cam_near_far", "poses"}
