"""CPU: the mesh clean-up entry points -- declared, exported and bound; the workspace formula; arguments refused before any launch; the
Python operators' host-side behaviour; extract_mesh's new parameters."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_mesh_clean_workspace_bytes", "sn_rm_mesh_components_init", "sn_rm_mesh_components_sweep", "sn_rm_mesh_component_stats",
           "sn_rm_mesh_filter_count", "sn_rm_mesh_filter_emit")
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
BIG = 1 << 31


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
    assert re.search(r"#define SN_ABI_VERSION 12\b", hdr) and _lib.ABI_VERSION == 12 and lib.sn_abi_version() == 12
    mk = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh_clean\.hip\b", mk, re.M) and re.search(r"^SRCS\s*:=.*\bmesh\.hip\b", mk, re.M)


def test_workspace_formula():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    need = l.sn_rm_mesh_clean_workspace_bytes

    def formula(V, T):
        up = lambda n: (n + 15) // 16 * 16
        return up(4 * ((V + 1023) // 1024)) + up(4 * ((T + 1023) // 1024)) + up(4 * V) + up(4 * T)

    sizes = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4097, 137367, 281530, 947638, 1893068, BIG - 1)
    for V in sizes:
        for T in sizes:
            assert need(V, T) == formula(V, T), (V, T)
    assert need(1, 0) > 0
    for a, b in zip(sizes[:-1], sizes[1:]):                  # monotone in each argument
        assert need(a, 7) <= need(b, 7) and need(7, a) <= need(7, b)
    assert need(947638, 1893068) <= 4 * (947638 + 1893068) * 1.01
    for V, T in ((BIG, 0), (0, BIG), (BIG, BIG), (0xFFFFFFFF, 5)):
        assert need(V, T) == 0, (V, T)
        assert b"not supported" in l.sn_last_error()


def test_arguments_are_refused_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    p, ws, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(8200)
    V, T = 100, 50
    need = l.sn_rm_mesh_clean_workspace_bytes(V, T)
    # V == 0: SN_OK, no pointer is looked at
    assert l.sn_rm_mesh_components_init(0, None, None) == OK
    assert l.sn_rm_mesh_components_sweep(None, 5, 0, None, 4, None, None) == OK
    assert l.sn_rm_mesh_components_sweep(None, 5, V, None, 0, None, None) == OK              # no round
    assert l.sn_rm_mesh_component_stats(None, 5, 0, None, None, None, None, None) == OK
    assert l.sn_rm_mesh_filter_count(None, 5, 0, None, None, 0, None, None, 0, None, None) == OK
    assert l.sn_rm_mesh_filter_emit(None, 5, 0, None, None, None, 0, None, None, None, None, 4, 4, None) == OK
    assert l.sn_rm_mesh_filter_emit(None, T, V, None, None, None, 0, None, None, None, None, 0, 0, None) == OK     # nothing can be stored
    # init
    assert l.sn_rm_mesh_components_init(V, None, None) == INVALID and b"NULL" in l.sn_last_error()
    assert l.sn_rm_mesh_components_init(BIG, p, None) == UNSUPPORTED and b"not supported" in l.sn_last_error()
    # sweep
    assert l.sn_rm_mesh_components_sweep(None, T, V, p, 4, p, None) == INVALID and b"NULL" in l.sn_last_error()
    assert l.sn_rm_mesh_components_sweep(p, T, V, None, 4, p, None) == INVALID
    assert l.sn_rm_mesh_components_sweep(p, T, V, p, 4, None, None) == INVALID
    assert l.sn_rm_mesh_components_sweep(p, T, V, p, 4097, p, None) == INVALID and b"rounds" in l.sn_last_error()
    assert l.sn_rm_mesh_components_sweep(p, BIG, V, p, 4, p, None) == UNSUPPORTED
    assert l.sn_rm_mesh_components_sweep(p, T, BIG, p, 4, p, None) == UNSUPPORTED
    # stats
    for hole in range(5):
        a = [p, p, p, p, p]
        a[hole] = None
        assert l.sn_rm_mesh_component_stats(a[0], T, V, a[1], a[2], a[3], a[4], None) == INVALID, hole
    assert l.sn_rm_mesh_component_stats(p, BIG, V, p, p, p, p, None) == UNSUPPORTED
    # count
    for hole in range(6):
        a = [p, p, p, p, ws, p]
        a[hole] = None
        assert l.sn_rm_mesh_filter_count(a[0], T, V, a[1], a[2], 0, a[3], a[4], need, a[5], None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert l.sn_rm_mesh_filter_count(p, T, BIG, p, p, 0, p, ws, 1 << 40, p, None) == UNSUPPORTED
    assert l.sn_rm_mesh_filter_count(p, T, V, p, p, 0, p, ws, need - 1, p, None) == WORKSPACE and b"too small" in l.sn_last_error()
    assert l.sn_rm_mesh_filter_count(p, T, V, p, p, 0, p, odd, need, p, None) == INVALID and b"aligned" in l.sn_last_error()
    # emit
    assert l.sn_rm_mesh_filter_emit(None, T, V, p, None, ws, need, p, None, p, None, 4, 4, None) == INVALID
    assert l.sn_rm_mesh_filter_emit(p, T, V, None, None, ws, need, p, None, p, None, 4, 4, None) == INVALID
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, None, None, need, p, None, p, None, 4, 4, None) == INVALID
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, None, ws, need, None, None, p, None, 4, 4, None) == INVALID
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, None, ws, need, p, None, None, None, 4, 4, None) == INVALID
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, p, ws, need, p, None, p, None, 4, 4, None) == INVALID            # normals in, none out
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, None, ws, need, p, None, p, None, BIG, 4, None) == INVALID
    assert l.sn_rm_mesh_filter_emit(p, BIG, V, p, None, ws, 1 << 40, p, None, p, None, 4, 4, None) == UNSUPPORTED
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, None, ws, need - 1, p, None, p, None, 4, 4, None) == WORKSPACE
    assert l.sn_rm_mesh_filter_emit(p, T, V, p, None, odd, need, p, None, p, None, 4, 4, None) == INVALID and b"aligned" in l.sn_last_error()


def test_mesh_clean_host_side():
    from sanerf_hq_amd import raymarching as rm
    for name in ("mesh_components", "mesh_clean", "mesh_filter_counts", "mesh_filter_emit"):
        assert callable(getattr(rm, name))
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    assert rm.mesh_clean(mesh) is mesh                                       # both options 0: the input object, no launch
    assert rm.mesh_clean(mesh, min_triangles=0, keep_largest=0, return_source=True) is mesh
    for kw in (dict(min_triangles=-1), dict(keep_largest=-1), dict(min_triangles=5, keep_largest=-2)):
        with pytest.raises(ValueError, match="negative"):
            rm.mesh_clean(mesh, **kw)
    with pytest.raises(RuntimeError, match=r"\[T,3\]"):
        rm.mesh_components(torch.zeros(6, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mesh_components(mesh["triangles"], 4)                             # a host tensor: refused, no fallback
    for fn in (rm.mesh_components, rm.mesh_clean):
        assert "graph" in fn.__doc__


def test_extract_mesh_has_the_new_parameters():
    from sanerf_hq_amd.nerf import NeRFRenderer
    sig = inspect.signature(NeRFRenderer.extract_mesh).parameters
    assert sig["min_component_triangles"].default == 0 and sig["keep_largest"].default == 0
    assert [k for k in sig][:7] == ["self", "resolution", "threshold", "aabb", "instance_ids", "invert", "normals"]
