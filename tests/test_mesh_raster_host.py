"""CPU: the mesh rasteriser's entry points -- declared, exported and bound; the workspace formula as the header states it; arguments refused
before any launch; the Python operators' host-side behaviour; NeRFRenderer.render_mesh."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_mesh_raster_workspace_bytes", "sn_rm_mesh_raster_project", "sn_rm_mesh_raster_draw", "sn_rm_mesh_raster_resolve")
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
    assert re.search(r"#define SN_ABI_VERSION 12\b", hdr) and _lib.ABI_VERSION == 12 and lib.sn_abi_version() == 12     # additive
    mk = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh_raster\.hip\b", mk, re.M)
    assert re.search(r"^mesh_raster\.o .*: sn_wave\.h", mk, re.M)


def _formula(V, T, H, W):
    """The header's statement: 16 + 16V + 8HW + up(4T)."""
    return 16 + 16 * V + 8 * H * W + (4 * T + 15) // 16 * 16


def test_workspace_formula():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    need = l.sn_rm_mesh_raster_workspace_bytes
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    assert "16 + 16V + 8HW + up(4T)" in hdr
    sizes = (0, 1, 3, 4, 5, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 947638, 1893068, (1 << 30) + 1, BIG - 1)
    sides = (1, 2, 37, 53, 800, 1023, 1024, 1025, SIDE - 1, SIDE)
    for V in sizes:
        for T in sizes:
            for H, W in ((1, 1), (37, 53), (1023, 1025), (800, 800), (SIDE, SIDE), (1, SIDE)):
                assert need(V, T, H, W) == _formula(V, T, H, W), (V, T, H, W)
    for H in sides:
        for W in sides:
            assert need(5, 7, H, W) == _formula(5, 7, H, W), (H, W)
    assert need(0, 0, 1, 1) == 16 + 8
    for V, T, H, W in ((BIG, 0, 8, 8), (0, BIG, 8, 8), (0xFFFFFFFF, 5, 8, 8), (5, 5, 0, 8), (5, 5, 8, 0), (5, 5, SIDE + 1, 8), (5, 5, 8, SIDE + 1),
                       (5, 5, 0xFFFFFFFF, 0xFFFFFFFF)):
        assert need(V, T, H, W) == 0, (V, T, H, W)
        assert b"not supported" in l.sn_last_error()


def test_arguments_are_refused_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the device pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    project, draw, resolve = l.sn_rm_mesh_raster_project, l.sn_rm_mesh_raster_draw, l.sn_rm_mesh_raster_resolve
    p, ws, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(8200)
    V, T, H, W = 100, 50, 48, 64
    need = l.sn_rm_mesh_raster_workspace_bytes(V, T, H, W)
    big = 1 << 60
    # project: vertices (NULL only with V == 0), pose, intrinsics, workspace, counts
    for hole in range(5):
        a = [p, p, p, ws, p]
        a[hole] = None
        assert project(a[0], V, T, a[1], a[2], H, W, 0.05, a[3], need, a[4], None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert project(None, 0, T, p, p, H, W, 0.05, ws, 0, p, None) == WORKSPACE                   # V == 0 without vertices passes the NULL test
    for bad in (0.0, -0.0, -1.0, float("inf"), float("nan")):
        assert project(p, V, T, p, p, H, W, bad, ws, need, p, None) == INVALID and b"positive and finite" in l.sn_last_error()
    assert project(p, V, T, p, p, H, W, 0.05, ws, need - 1, p, None) == WORKSPACE and b"too small" in l.sn_last_error()
    assert project(p, V, T, p, p, H, W, 0.05, odd, need, p, None) == INVALID and b"aligned" in l.sn_last_error()
    for v, t, h, w in ((BIG, T, H, W), (V, BIG, H, W), (V, T, 0, W), (V, T, H, 0), (V, T, SIDE + 1, W), (V, T, H, SIDE + 1)):
        assert project(p, v, t, p, p, h, w, 0.05, ws, big, p, None) == UNSUPPORTED and b"not supported" in l.sn_last_error()
        assert draw(p, v, t, h, w, 0, 16, ws, big, p, None) == UNSUPPORTED
        assert resolve(p, v, t, h, w, None, None, None, 1.0, ws, big, p, p, p, None, None, None, None) == UNSUPPORTED
    # draw: triangles (NULL only with T == 0), workspace, counts; the threshold
    for hole in range(3):
        a = [p, ws, p]
        a[hole] = None
        assert draw(a[0], V, T, H, W, 0, 16, a[1], need, a[2], None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert draw(None, V, 0, H, W, 0, 16, ws, 0, p, None) == WORKSPACE
    assert draw(p, V, T, H, W, 0, BIG, ws, need, p, None) == INVALID and b"small_max_pixels" in l.sn_last_error()
    assert draw(p, V, T, H, W, 1, BIG - 1, ws, need - 1, p, None) == WORKSPACE                 # 2^31 - 1 is accepted
    assert draw(p, V, T, H, W, 1, 0, odd, need, p, None) == INVALID and b"aligned" in l.sn_last_error()
    # resolve: triangles, workspace, triangle_id, depth, mask; an attribute and its image come together
    for hole in range(5):
        a = [p, ws, p, p, p]
        a[hole] = None
        assert resolve(a[0], V, T, H, W, None, None, None, 1.0, a[1], need, a[2], a[3], a[4], None, None, None, None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    for attrs in ((p, None, None, None, None, None), (None, None, None, p, None, None), (None, p, None, None, None, None),
                  (None, None, None, None, p, None), (None, None, p, None, None, None), (None, None, None, None, None, p), (p, p, p, p, p, None)):
        c, n, lb, im, nm, lo = attrs
        assert resolve(p, V, T, H, W, c, n, lb, 1.0, ws, need, p, p, p, im, nm, lo, None) == INVALID and b"come together" in l.sn_last_error()
    assert resolve(p, V, T, H, W, p, p, p, 1.0, ws, need - 1, p, p, p, p, p, p, None) == WORKSPACE
    assert resolve(p, 0, T, H, W, None, None, None, 1.0, ws, 0, p, p, p, p, p, p, None) == WORKSPACE      # an empty mesh has no attribute to point at
    assert resolve(p, V, T, H, W, None, None, None, 1.0, odd, need, p, p, p, None, None, None, None) == INVALID and b"aligned" in l.sn_last_error()
    assert resolve(None, V, 0, H, W, None, None, None, 1.0, ws, 0, p, p, p, None, None, None, None) == WORKSPACE


def test_mesh_rasterize_host_side():
    from sanerf_hq_amd import raymarching as rm
    for name in ("mesh_rasterize", "mesh_raster_project", "mesh_raster_draw", "mesh_raster_resolve"):
        assert callable(getattr(rm, name))
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    pose, intr = torch.eye(4), torch.tensor([10.0, 10.0, 4.0, 4.0])
    for H, W in ((0, 8), (8, 0), (8193, 8), (8, 8193), (-1, 8)):
        with pytest.raises(ValueError, match=r"must be in \[1, 8192\]"):
            rm.mesh_rasterize(mesh, pose, intr, H, W)
    with pytest.raises(ValueError, match="integers"):
        rm.mesh_rasterize(mesh, pose, intr, 8.5, 8)
    for near in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError, match="positive and finite"):
            rm.mesh_rasterize(mesh, pose, intr, 8, 8, near=near)
    for small in (-1, 1 << 31):
        with pytest.raises(ValueError, match="small_max_pixels"):
            rm.mesh_rasterize(mesh, pose, intr, 8, 8, small_max_pixels=small)
    with pytest.raises(RuntimeError, match=r"\[T,3\]"):
        rm.mesh_rasterize(dict(mesh, triangles=torch.zeros(6, dtype=torch.int32)), pose, intr, 8, 8)
    with pytest.raises(RuntimeError, match=r"\[V,3\]"):
        rm.mesh_rasterize(dict(mesh, vertices=torch.zeros(12)), pose, intr, 8, 8)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mesh_rasterize(mesh, pose, intr, 8, 8)                                # a host tensor: refused, no fallback
    sig = inspect.signature(rm.mesh_rasterize).parameters
    assert [k for k in sig] == ["mesh", "pose", "intrinsics", "H", "W", "near", "cull", "colors", "labels", "normals", "bg_color", "small_max_pixels"]
    assert (sig["near"].default, sig["cull"].default, sig["bg_color"].default, sig["small_max_pixels"].default) == (0.05, False, 1.0, None)
    assert sig["colors"].default is None and sig["labels"].default is None and sig["normals"].default is None
    assert 0 <= rm.RASTER_SMALL_MAX_PIXELS < (1 << 31) and rm.RASTER_MAX_SIDE == 8192
    assert "nothing is read back" in rm.mesh_rasterize.__doc__


def test_render_mesh_signature_and_grad_mode():
    from sanerf_hq_amd.nerf import NeRFNetwork, NeRFRenderer
    from sanerf_hq_amd.synth import make_opt
    sig = inspect.signature(NeRFRenderer.render_mesh).parameters
    assert [k for k in sig] == ["self", "mesh", "pose", "intrinsics", "H", "W", "cull", "bg_color"]
    assert (sig["cull"].default, sig["bg_color"].default) == (False, 1)
    doc = NeRFRenderer.render_mesh.__doc__
    assert "weights_sum" in doc and "depth" in doc and "min_near" in doc
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    pose, intr = torch.eye(4), torch.tensor([10.0, 10.0, 4.0, 4.0])
    model = NeRFNetwork(make_opt(num_steps=[16, 8, 4]))
    with pytest.raises(RuntimeError, match="inference query"):                   # as _inference_only refuses density_volume
        model.render_mesh(mesh, pose, intr, 8, 8)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"must be in \[1, 8192\]"):
            model.render_mesh(mesh, pose, intr, 0, 8)
        with pytest.raises(RuntimeError, match="CUDA"):
            model.render_mesh(mesh, pose, intr, 8, 8)
