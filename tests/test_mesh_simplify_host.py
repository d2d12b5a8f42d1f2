"""CPU: the mesh simplification entry points -- declared, exported and bound; the workspace formula as the header states it; arguments
refused before any launch; the Python operators' host-side behaviour; extract_mesh's new parameter."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_mesh_simplify_workspace_bytes", "sn_rm_mesh_simplify_count", "sn_rm_mesh_simplify_emit")
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
    assert re.search(r"#define SN_ABI_VERSION 12\b", hdr) and _lib.ABI_VERSION == 12 and lib.sn_abi_version() == 12     # additive
    mk = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh_simplify\.hip\b", mk, re.M)


def _formula(V, T, cells):
    """The header's statement: 16 + up(4V) + 2 up(4T) + up(4 ceil(T/1024)) + up(4C) + 2 up(4W) + up(4 ceil(W/1024)) + 64V."""
    up = lambda n: (n + 15) // 16 * 16
    W = (cells + 31) // 32
    C = 1
    while C < 2 * T:
        C *= 2
    return 16 + up(4 * V) + 2 * up(4 * T) + up(4 * ((T + 1023) // 1024)) + up(4 * C) + 2 * up(4 * W) + up(4 * ((W + 1023) // 1024)) + 64 * V


def test_workspace_formula():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    need = l.sn_rm_mesh_simplify_workspace_bytes
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    assert "16 + up(4V) + 2 up(4T) + up(4 ceil(T / 1024)) + up(4C) + 2 up(4W) + up(4 ceil(W / 1024)) + 64V" in hdr
    sizes = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4097, 32769, 301196, 600294, 947638, 1893068, (1 << 30) + 1, BIG - 1)
    for V in sizes:
        for T in sizes:
            for cells in (1, 31, 32, 33, 32768, 32769, 2197, 1 << 24, BIG - 1):
                assert need(V, T, cells) == _formula(V, T, cells), (V, T, cells)
    assert need(0, 0, 1) > 0
    for a, b in zip(sizes[:-1], sizes[1:]):                  # monotone in each argument
        assert need(a, 7, 9) <= need(b, 7, 9) and need(7, a, 9) <= need(7, b, 9) and need(7, 9, max(a, 1)) <= need(7, 9, b)
    # the figures of the documents: 68 bytes a vertex, at most 24 a triangle, 2 bits a cell
    V, T, cells = 947638, 1893068, 257 ** 3
    assert need(V, T, cells) <= 68 * V + 24 * T + cells // 4 + 1024
    for V, T, cells in ((BIG, 0, 1), (0, BIG, 1), (0, 0, BIG), (BIG, BIG, BIG), (0xFFFFFFFF, 5, 5)):
        assert need(V, T, cells) == 0, (V, T, cells)
        assert b"not supported" in l.sn_last_error()


def _f(*v):
    return (ctypes.c_float * len(v))(*v)


def _u(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_arguments_are_refused_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the device pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    count, emit = l.sn_rm_mesh_simplify_count, l.sn_rm_mesh_simplify_emit
    p, ws, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(8200)
    V, T = 100, 50
    o, c, d = _f(0, 0, 0), _f(1, 2, 3), _u(4, 5, 6)
    need = l.sn_rm_mesh_simplify_workspace_bytes(V, T, 120)
    # V == 0: SN_OK, no pointer is looked at
    assert count(None, None, None, 0, 5, None, None, None, None, 0, None, None) == OK
    assert emit(None, None, None, 0, 5, None, None, None, None, 0, None, None, None, None, 4, 4, None) == OK
    assert emit(None, None, None, V, T, None, None, None, None, 0, None, None, None, None, 0, 0, None) == OK       # nothing can be stored
    # count: every pointer it needs (normals may be NULL; triangles may be NULL only with T == 0)
    for hole in range(7):
        a = [p, p, o, c, d, ws, p]                           # vertices, triangles, origin, cell, dims, workspace, counts
        a[hole] = None
        assert count(a[0], None, a[1], V, T, a[2], a[3], a[4], a[5], need, a[6], None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert count(p, p, None, V, 0, o, c, d, ws, 0, p, None) == WORKSPACE               # T == 0 without triangles passes the NULL test
    assert count(p, None, p, V, T, o, c, d, ws, need - 1, p, None) == WORKSPACE and b"too small" in l.sn_last_error()
    assert count(p, None, p, V, T, o, c, d, ws, 0, p, None) == WORKSPACE
    assert count(p, None, p, V, T, o, c, d, odd, need, p, None) == INVALID and b"aligned" in l.sn_last_error()
    for bad in (_f(0, 2, 3), _f(1, -2, 3), _f(1, 2, float("inf")), _f(float("nan"), 2, 3), _f(1, 2, -0.0)):
        assert count(p, None, p, V, T, o, bad, d, ws, need, p, None) == INVALID and b"positive and finite" in l.sn_last_error()
        assert emit(p, None, p, V, T, o, bad, d, ws, need, p, None, p, None, 4, 4, None) == INVALID and b"positive and finite" in l.sn_last_error()
    assert count(p, None, p, V, T, _f(0, float("nan"), 0), c, d, ws, need, p, None) == INVALID and b"origin" in l.sn_last_error()
    assert count(p, None, p, V, T, o, c, _u(4, 0, 6), ws, need, p, None) == INVALID and b"dims" in l.sn_last_error()
    big = 1 << 60
    assert count(p, None, p, V, T, o, c, _u(BIG, 1, 1), ws, big, p, None) == UNSUPPORTED and b"not supported" in l.sn_last_error()
    assert count(p, None, p, V, T, o, c, _u(1 << 16, 1 << 15, 1), ws, big, p, None) == UNSUPPORTED            # the product reaches 2^31
    assert count(p, None, p, V, T, o, c, _u(1 << 16, 1 << 16, 1 << 16), ws, big, p, None) == UNSUPPORTED      # and does not wrap
    assert count(p, None, p, V, T, o, c, _u((1 << 16) - 1, 1 << 15, 1), ws, 0, p, None) == WORKSPACE          # just below: supported
    assert count(p, None, p, BIG, T, o, c, d, ws, big, p, None) == UNSUPPORTED
    assert count(p, None, p, V, BIG, o, c, d, ws, big, p, None) == UNSUPPORTED
    # emit
    good = lambda: [p, p, o, c, d, ws, p, p]                 # vertices, triangles, origin, cell, dims, workspace, out_vertices, out_triangles
    for hole in (1, 2, 3, 4, 5, 6, 7):                       # (vertices are not read by the emit)
        a = good()
        a[hole] = None
        assert emit(a[0], None, a[1], V, T, a[2], a[3], a[4], a[5], need, a[6], None, a[7], None, 4, 4, None) == INVALID, hole
    assert emit(p, p, p, V, T, o, c, d, ws, need, p, None, p, None, 4, 4, None) == INVALID                    # normals in, none out
    assert emit(p, None, p, V, T, o, c, d, ws, need, p, None, p, None, BIG, 4, None) == INVALID
    assert emit(p, None, p, V, T, o, c, d, ws, need - 1, p, None, p, None, 4, 4, None) == WORKSPACE
    assert emit(p, None, p, V, T, o, c, d, odd, need, p, None, p, None, 4, 4, None) == INVALID and b"aligned" in l.sn_last_error()
    assert emit(p, None, p, V, BIG, o, c, d, ws, big, p, None, p, None, 4, 4, None) == UNSUPPORTED
    assert emit(p, None, p, V, T, o, c, _u(1 << 16, 1 << 15, 1), ws, big, p, None, p, None, 4, 4, None) == UNSUPPORTED
    assert emit(p, None, p, V, T, o, c, d, None, need, None, None, None, p, 0, 0, None) == INVALID           # a cluster map alone still needs the workspace


def test_mesh_simplify_host_side():
    from sanerf_hq_amd import raymarching as rm
    for name in ("mesh_simplify", "mesh_simplify_counts", "mesh_simplify_emit"):
        assert callable(getattr(rm, name))
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    for cell in (0.0, -1.0, float("inf"), float("nan"), (1.0, 0.0, 1.0)):
        with pytest.raises(ValueError, match="positive and finite"):
            rm.mesh_simplify(mesh, cell)
    with pytest.raises(ValueError, match="3 entries"):
        rm.mesh_simplify(mesh, (1.0, 2.0))
    with pytest.raises(ValueError, match="together"):
        rm.mesh_simplify(mesh, 1.0, origin=(0, 0, 0))
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mesh_simplify(mesh, 1.0, origin=(0, 0, 0), dims=(2, 2, 2))        # a host tensor: refused, no fallback
    with pytest.raises(RuntimeError, match=r"\[T,3\]"):
        rm.mesh_simplify(dict(mesh, triangles=torch.zeros(6, dtype=torch.int32)), 1.0)
    sig = inspect.signature(rm.mesh_simplify).parameters
    assert [k for k in sig] == ["mesh", "cell", "origin", "dims", "return_cluster"]
    assert sig["origin"].default is None and sig["dims"].default is None and sig["return_cluster"].default is False
    assert "graph" in rm.mesh_simplify.__doc__ and "read back once" in rm.mesh_simplify.__doc__


def test_extract_mesh_has_the_new_parameter():
    from sanerf_hq_amd.nerf import NeRFRenderer
    sig = inspect.signature(NeRFRenderer.extract_mesh).parameters
    assert sig["simplify"].default == 0
    assert [k for k in sig][:9] == ["self", "resolution", "threshold", "aabb", "instance_ids", "invert", "normals", "min_component_triangles",
                                    "keep_largest"]
