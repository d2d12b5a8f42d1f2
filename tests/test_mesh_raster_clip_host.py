"""CPU: the clipped rasteriser's entry points -- declared, exported and bound beside their siblings, the ABI still 12, the workspace the
unclipped one's; arguments refused before any launch; the Python wrappers' host-side refusals."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_mesh_raster_draw_clip", "sn_rm_mesh_raster_resolve_clip")
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
BIG = 1 << 31
SIDE = 8192


def test_symbols_declared_exported_and_bound():
    from sanerf_hq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTED_SYMBOLS
        assert getattr(bound, s).argtypes is not None, s
    assert len(bound.sn_rm_mesh_raster_draw_clip.argtypes) == 16 and len(bound.sn_rm_mesh_raster_resolve_clip.argtypes) == 22
    assert re.search(r"#define SN_ABI_VERSION 12\b", hdr) and _lib.ABI_VERSION == 12 and lib.sn_abi_version() == 12     # additive
    for word in ("Crossing point", "clip_counts", "behind"):
        assert word in hdr, word
    assert "16 + 16V + 8HW + up(4T)" in hdr                    # the workspace does not grow


def test_arguments_are_refused_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the device pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    draw, resolve = l.sn_rm_mesh_raster_draw_clip, l.sn_rm_mesh_raster_resolve_clip
    p, ws, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(8200)
    V, T, H, W = 100, 50, 48, 64
    need = l.sn_rm_mesh_raster_workspace_bytes(V, T, H, W)
    big = 1 << 60

    def d(vertices=p, triangles=p, v=V, t=T, pose=p, intr=p, h=H, w=W, near=0.05, cull=0, small=16, work=ws, size=need, counts=p, clip_counts=p):
        return draw(vertices, triangles, v, t, pose, intr, h, w, near, cull, small, work, size, counts, clip_counts, None)

    def r(vertices=p, triangles=p, v=V, t=T, pose=p, intr=p, h=H, w=W, near=0.05, attrs=(None,) * 3, work=ws, size=need, tid=p, depth=p, mask=p,
          images=(None,) * 3):
        return resolve(vertices, triangles, v, t, pose, intr, h, w, near, attrs[0], attrs[1], attrs[2], 1.0, work, size, tid, depth, mask, images[0],
                       images[1], images[2], None)
    # draw: vertices (NULL only with V == 0), triangles (T == 0), pose, intrinsics, workspace, counts, clip_counts
    for hole in ("vertices", "triangles", "pose", "intr", "work", "counts", "clip_counts"):
        assert d(**{hole: None}) == INVALID and b"NULL" in l.sn_last_error(), hole
    assert d(vertices=None, v=0, size=0) == WORKSPACE and d(triangles=None, t=0, size=0) == WORKSPACE
    for bad in (0.0, -0.0, -1.0, float("inf"), float("nan")):
        assert d(near=bad) == INVALID and b"positive and finite" in l.sn_last_error()
        assert r(near=bad) == INVALID and b"positive and finite" in l.sn_last_error()
    assert d(small=BIG) == INVALID and b"small_max_pixels" in l.sn_last_error()
    assert d(small=BIG - 1, size=need - 1) == WORKSPACE and b"too small" in l.sn_last_error()
    assert d(work=odd) == INVALID and b"aligned" in l.sn_last_error()
    for v, t, h, w in ((BIG, T, H, W), (V, BIG, H, W), (V, T, 0, W), (V, T, H, 0), (V, T, SIDE + 1, W), (V, T, H, SIDE + 1)):
        assert d(v=v, t=t, h=h, w=w, size=big) == UNSUPPORTED and b"not supported" in l.sn_last_error()
        assert r(v=v, t=t, h=h, w=w, size=big) == UNSUPPORTED and b"not supported" in l.sn_last_error()
    # resolve: vertices, triangles, pose, intrinsics, workspace, triangle_id, depth, mask; an attribute and its image come together
    for hole in ("vertices", "triangles", "pose", "intr", "work", "tid", "depth", "mask"):
        assert r(**{hole: None}) == INVALID and b"NULL" in l.sn_last_error(), hole
    for attrs, images in (((p, None, None), (None,) * 3), ((None,) * 3, (p, None, None)), ((None, p, None), (None,) * 3), ((None,) * 3, (None, p, None)),
                          ((None, None, p), (None,) * 3), ((None,) * 3, (None, None, p)), ((p, p, p), (p, p, None))):
        assert r(attrs=attrs, images=images) == INVALID and b"come together" in l.sn_last_error()
    assert r(attrs=(p, p, p), images=(p, p, p), size=need - 1) == WORKSPACE
    assert r(vertices=None, v=0, images=(p, p, p), size=0) == WORKSPACE          # an empty mesh has no attribute to point at
    assert r(work=odd) == INVALID and b"aligned" in l.sn_last_error()
    assert r(triangles=None, t=0, size=0) == WORKSPACE


def test_phase_wrappers_refuse_clip_without_the_mesh_or_the_camera():
    from sanerf_hq_amd import raymarching as rm
    tri = torch.zeros(2, 3, dtype=torch.int32)
    ws, counts, clip_counts = torch.zeros(64, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    camera = dict(vertices=torch.zeros(4, 3), pose=torch.eye(4), intrinsics=torch.ones(4), near=0.05)
    images = (torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8), torch.zeros(8, 8, dtype=torch.uint8))
    for missing in camera:
        given = {k: v for k, v in camera.items() if k != missing}
        with pytest.raises(ValueError, match="clip=True needs"):
            rm.mesh_raster_draw(tri, 4, 8, 8, ws, counts, clip=True, clip_counts=clip_counts, **given)
        with pytest.raises(ValueError, match="clip=True needs"):
            rm.mesh_raster_resolve(tri, 4, 8, 8, ws, *images, clip=True, **given)
    with pytest.raises(ValueError, match="clip_counts"):
        rm.mesh_raster_draw(tri, 4, 8, 8, ws, counts, clip=True, **camera)
    with pytest.raises(ValueError, match=r"vertices are \[4,3\]"):
        rm.mesh_raster_draw(tri, 4, 8, 8, ws, counts, clip=True, clip_counts=clip_counts, **dict(camera, vertices=torch.zeros(5, 3)))
    for near in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="positive and finite"):
            rm.mesh_raster_draw(tri, 4, 8, 8, ws, counts, clip=True, clip_counts=clip_counts, **dict(camera, near=near))
    with pytest.raises(RuntimeError, match="CUDA"):                              # host tensors: refused, no fallback
        rm.mesh_raster_draw(tri, 4, 8, 8, ws, counts, clip=True, clip_counts=clip_counts, **camera)
    for name in ("mesh_raster_draw", "mesh_raster_resolve"):
        sig = inspect.signature(getattr(rm, name)).parameters
        assert sig["clip"].default is False and all(sig[k].default is None for k in ("vertices", "pose", "intrinsics", "near")), name


def test_mesh_rasterize_clip_and_render_mesh_clip_host_side():
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import NeRFNetwork, NeRFRenderer
    from sanerf_hq_amd.synth import make_opt
    assert list(inspect.signature(rm.mesh_rasterize_clip).parameters) == list(inspect.signature(rm.mesh_rasterize).parameters)
    assert list(inspect.signature(NeRFRenderer.render_mesh_clip).parameters) == list(inspect.signature(NeRFRenderer.render_mesh).parameters)
    assert "clip_counts" in rm.mesh_rasterize_clip.__doc__ and "clip_counts" in NeRFRenderer.render_mesh_clip.__doc__
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    pose, intr = torch.eye(4), torch.tensor([10.0, 10.0, 4.0, 4.0])
    with pytest.raises(ValueError, match=r"mesh_rasterize_clip: H = 0"):
        rm.mesh_rasterize_clip(mesh, pose, intr, 0, 8)
    with pytest.raises(ValueError, match="positive and finite"):
        rm.mesh_rasterize_clip(mesh, pose, intr, 8, 8, near=0.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mesh_rasterize_clip(mesh, pose, intr, 8, 8)
    model = NeRFNetwork(make_opt(num_steps=[16, 8, 4]))
    with pytest.raises(RuntimeError, match="inference query"):
        model.render_mesh_clip(mesh, pose, intr, 8, 8)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA"):
            model.render_mesh_clip(mesh, pose, intr, 8, 8)
