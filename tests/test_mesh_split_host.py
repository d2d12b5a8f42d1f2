"""CPU: the mesh split entry points -- declared, exported and bound; the workspace size; arguments refused before any HIP call; save_meshes;
the Python operators' host-side behaviour."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_mesh_split_workspace_bytes", "sn_rm_mesh_split_count", "sn_rm_mesh_split_emit")
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
    assert re.search(r"#define SN_MESH_SPLIT_PARTS 33\b", hdr)
    mk = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh_split\.hip\b", mk, re.M)
    assert re.search(r"^mesh_split\.o build/exp/mesh_split\.o build/poison/mesh_split\.o: sn_wave\.h mesh_common\.h$", mk, re.M)


def test_workspace_bytes():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    need = l.sn_rm_mesh_split_workspace_bytes

    def formula(V, T):
        up = lambda n: (n + 15) // 16 * 16
        seg = lambda n: (n + 1023) // 1024
        return (up(4 * 33 * seg(T)) + up(4 * 33 * seg(V)) + up(8 * V) + up(4 * V) + up(2 * 33 * ((V + 63) // 64)) + up(4 * T))

    sizes = (0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4097, 33000, 301196, 947638, 1893068, BIG - 1)
    for V in sizes:
        for T in sizes:
            assert need(V, T) == formula(V, T), (V, T)
            assert need(V, T) % 16 == 0
    assert need(1, 1) > 0
    for a, b in zip(sizes[:-1], sizes[1:]):                  # monotone in each argument
        assert need(a, 7) <= need(b, 7) and need(7, a) <= need(7, b)
    assert need(947638, 1893068) <= (13.2 * 947638 + 4.2 * 1893068)
    for V, T in ((BIG, 0), (0, BIG), (BIG, BIG), (0xFFFFFFFF, 5)):
        assert need(V, T) == 0, (V, T)
        assert b"not supported" in l.sn_last_error()


def test_arguments_are_refused_before_any_hip_call():
    """No device is touched: every call below returns from the host-side checks (the pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    p, ws, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(8200)
    V, T = 100, 50
    need = l.sn_rm_mesh_split_workspace_bytes(V, T)
    count, emit = l.sn_rm_mesh_split_count, l.sn_rm_mesh_split_emit
    # the empty mesh: SN_OK; with nothing to store into, no pointer is looked at
    assert count(None, 5, 0, None, None, 0, None, None, None, None) == OK
    assert count(None, 0, 5, None, None, 0, None, None, None, None) == OK
    assert count(None, 0, 0, None, None, 0, None, None, None, None) == OK
    assert emit(None, 5, 0, None, None, None, 0, None, None, None, None, None, 4, 4, None) == OK
    assert emit(None, 0, 5, None, None, None, 0, None, None, None, None, None, 4, 4, None) == OK
    assert emit(None, T, V, None, None, None, 0, None, None, None, None, None, 0, 0, None) == OK          # nothing can be stored
    # count: one hole at a time -- triangles, labels, workspace, the two offset arrays, counts
    for hole in range(6):
        a = [p, p, ws, p, p, p]
        a[hole] = None
        assert count(a[0], T, V, a[1], a[2], need, a[3], a[4], a[5], None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert count(p, T, BIG, p, ws, 1 << 40, p, p, p, None) == UNSUPPORTED and b"not supported" in l.sn_last_error()
    assert count(p, BIG, V, p, ws, 1 << 40, p, p, p, None) == UNSUPPORTED
    assert count(p, T, V, p, ws, need - 1, p, p, p, None) == WORKSPACE and b"too small" in l.sn_last_error()
    assert count(p, T, V, p, odd, need, p, p, p, None) == INVALID and b"aligned" in l.sn_last_error()
    # emit
    assert emit(None, T, V, p, None, ws, need, p, None, p, None, None, 4, 4, None) == INVALID               # triangles
    assert emit(p, T, V, None, None, ws, need, p, None, p, None, None, 4, 4, None) == INVALID               # vertices
    assert emit(p, T, V, p, None, None, need, p, None, p, None, None, 4, 4, None) == INVALID                # workspace
    assert emit(p, T, V, p, None, ws, need, None, None, p, None, None, 4, 4, None) == INVALID               # out_vertices
    assert emit(p, T, V, p, None, ws, need, p, None, None, None, None, 4, 4, None) == INVALID               # out_triangles
    assert emit(p, T, V, p, p, ws, need, p, None, p, None, None, 4, 4, None) == INVALID                     # normals in, none out
    assert emit(p, T, V, p, None, ws, need, p, None, p, None, None, BIG, 4, None) == INVALID
    assert emit(p, BIG, V, p, None, ws, 1 << 40, p, None, p, None, None, 4, 4, None) == UNSUPPORTED
    assert emit(p, T, BIG, p, None, ws, 1 << 40, p, None, p, None, None, 4, 4, None) == UNSUPPORTED
    assert emit(p, T, V, p, None, ws, need - 1, p, None, p, None, None, 4, 4, None) == WORKSPACE
    assert emit(p, T, V, p, None, odd, need, p, None, p, None, None, 4, 4, None) == INVALID and b"aligned" in l.sn_last_error()


def test_save_meshes_writes_what_save_mesh_writes(tmp_path):
    from sanerf_hq_amd.nerf.utils import save_mesh, save_meshes
    rng = np.random.default_rng(3)

    def part(V, T, normals, colors, labels):
        m = {"vertices": torch.from_numpy(rng.standard_normal((V, 3)).astype(np.float32)),
             "triangles": torch.from_numpy(rng.integers(0, V, size=(T, 3)).astype(np.int32)),
             "normals": torch.from_numpy(rng.standard_normal((V, 3)).astype(np.float32)) if normals else None}
        if colors:
            m["colors"], m["coverage"] = torch.from_numpy(rng.random((V, 3)).astype(np.float32)), torch.ones(V)
        if labels:
            m["labels"] = torch.full((V,), labels, dtype=torch.uint8)
        return m

    parts = {7: part(5, 4, True, True, 7), 0: part(9, 11, True, False, 0), 32: part(3, 1, False, False, 255), 12: part(4, 2, False, True, 0)}
    prefix = str(tmp_path / "object")
    paths = save_meshes(prefix, parts)
    assert paths == [f"{prefix}_{i:02d}.ply" for i in (0, 7, 12, 32)]
    for i, path in zip((0, 7, 12, 32), paths):
        m = parts[i]
        alone = save_mesh(str(tmp_path / "alone.ply"), m["vertices"], m["triangles"], m["normals"], m.get("colors"), m.get("labels"))
        assert open(path, "rb").read() == open(alone, "rb").read(), i
    assert save_meshes(prefix, {}) == []


def test_mesh_split_host_side():
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import NeRFRenderer
    for name in ("mesh_split", "mesh_split_counts", "mesh_split_emit"):
        assert callable(getattr(rm, name))
    assert rm.MESH_SPLIT_PARTS == 33
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match=r"uint8 tensor \[4\]"):
        rm.mesh_split(mesh, labels=torch.zeros(5, dtype=torch.uint8))                        # the wrong length
    with pytest.raises(RuntimeError, match=r"uint8 tensor \[4\]"):
        rm.mesh_split(mesh, labels=torch.zeros(4, dtype=torch.int32))                        # the wrong dtype
    with pytest.raises(RuntimeError, match=r"uint8 tensor \[4\]"):
        rm.mesh_split(dict(mesh, labels=torch.zeros(4, 1, dtype=torch.uint8)))               # the mesh's own labels, the wrong shape
    with pytest.raises(RuntimeError, match=r"uint8 tensor \[4\]"):
        rm.mesh_split_counts(mesh["triangles"], 4, torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no labels"):
        rm.mesh_split(mesh)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mesh_split(mesh, labels=torch.zeros(4, dtype=torch.uint8))                        # a host tensor: refused, no fallback
    assert "graph" in rm.mesh_split.__doc__ and "read back" in rm.mesh_split.__doc__
    sig = inspect.signature(NeRFRenderer.extract_object_meshes).parameters
    assert [k for k in sig] == ["self", "instance_ids", "part_min_triangles", "part_keep_largest", "extract_mesh_kwargs"]
    assert sig["instance_ids"].default is None and sig["part_min_triangles"].default == 0 and sig["part_keep_largest"].default == 0
