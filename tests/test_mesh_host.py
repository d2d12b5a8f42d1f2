"""CPU: the geometry-export entry points -- declared, exported and bound; arguments refused before any launch; the PLY writer; the
renderer's methods exist and refuse grad mode."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_lattice_points", "sn_rm_isosurface_workspace_bytes", "sn_rm_isosurface_count", "sn_rm_isosurface_emit")
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


def test_symbols_declared_exported_and_bound():
    from sanerf_hq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define SN_ABI_VERSION 12\b", hdr) and _lib.ABI_VERSION == 12 and lib.sn_abi_version() == 12
    mk = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh\.hip\b", mk, re.M)


def test_workspace_budget_and_unsupported_sizes():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    for shape in ((2, 2, 2), (2, 2, 3), (7, 6, 5), (33, 18, 70), (256, 256, 256), (512, 512, 512), (1290, 1290, 1290)):
        n = shape[0] * shape[1] * shape[2]
        need = l.sn_rm_isosurface_workspace_bytes(*shape)
        assert 5 * n <= need <= 8 * n, (shape, need)
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (1291, 1290, 1290), (2, 1 << 16, 1 << 15), (4, 1 << 31, 1 << 31)):
        assert l.sn_rm_isosurface_workspace_bytes(*shape) == 0, shape
        assert b"not supported" in l.sn_last_error()


def test_arguments_are_refused_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    p, ws = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    o, s = _lib.host_f32([0, 0, 0]), _lib.host_f32([1, 1, 1])
    need = l.sn_rm_isosurface_workspace_bytes(8, 8, 8)
    # lattice_points
    assert l.sn_rm_lattice_points(None, None, 8, 8, 8, 0, 0, 0, None, None) == OK          # count 0: no pointer is looked at
    assert l.sn_rm_lattice_points(o, s, 8, 8, 8, 0, 5, 0, None, None) == INVALID and b"NULL" in l.sn_last_error()
    assert l.sn_rm_lattice_points(None, s, 8, 8, 8, 0, 5, 0, p, None) == INVALID
    assert l.sn_rm_lattice_points(o, s, 8, 8, 8, 510, 3, 0, p, None) == INVALID and b"outside" in l.sn_last_error()
    assert l.sn_rm_lattice_points(o, s, 8, 0, 8, 0, 1, 0, p, None) == INVALID
    assert l.sn_rm_lattice_points(o, s, 1291, 1290, 1290, 0, 1, 0, p, None) == UNSUPPORTED
    # count
    assert l.sn_rm_isosurface_count(None, 8, 8, 8, 0.0, ws, need, p, None) == INVALID and b"NULL" in l.sn_last_error()
    assert l.sn_rm_isosurface_count(p, 8, 8, 8, 0.0, None, need, p, None) == INVALID
    assert l.sn_rm_isosurface_count(p, 8, 8, 8, 0.0, ws, need, None, None) == INVALID
    assert l.sn_rm_isosurface_count(p, 8, 1, 8, 0.0, ws, need, p, None) == UNSUPPORTED and b"not supported" in l.sn_last_error()
    assert l.sn_rm_isosurface_count(p, 1291, 1290, 1290, 0.0, ws, 1 << 40, p, None) == UNSUPPORTED
    assert l.sn_rm_isosurface_count(p, 8, 8, 8, 0.0, ws, need - 1, p, None) == WORKSPACE and b"too small" in l.sn_last_error()
    assert l.sn_rm_isosurface_count(p, 8, 8, 8, 0.0, ctypes.c_void_p(8200), need, p, None) == INVALID and b"aligned" in l.sn_last_error()
    # emit
    assert l.sn_rm_isosurface_emit(None, 8, 8, 8, 0.0, None, None, None, 0, None, None, None, 0, 0, None) == OK     # nothing can be stored
    assert l.sn_rm_isosurface_emit(None, 8, 8, 8, 0.0, o, s, ws, need, p, None, p, 4, 4, None) == INVALID
    assert l.sn_rm_isosurface_emit(p, 8, 8, 8, 0.0, None, s, ws, need, p, None, p, 4, 4, None) == INVALID
    assert l.sn_rm_isosurface_emit(p, 8, 8, 8, 0.0, o, s, None, need, p, None, p, 4, 4, None) == INVALID
    assert l.sn_rm_isosurface_emit(p, 8, 8, 8, 0.0, o, s, ws, need, None, None, p, 4, 4, None) == INVALID
    assert l.sn_rm_isosurface_emit(p, 8, 8, 8, 0.0, o, s, ws, need, p, None, None, 4, 4, None) == INVALID
    assert l.sn_rm_isosurface_emit(p, 1, 8, 8, 0.0, o, s, ws, need, p, None, p, 4, 4, None) == UNSUPPORTED
    assert l.sn_rm_isosurface_emit(p, 8, 8, 8, 0.0, o, s, ws, need - 1, p, None, p, 4, 4, None) == WORKSPACE
    assert l.sn_rm_isosurface_emit(p, 8, 8, 8, 0.0, o, s, ws, need, p, None, p, 1 << 31, 4, None) == INVALID


def _read_ply(path):
    """A parser of its own for the binary little-endian PLY files save_mesh writes."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, current = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            current = dict(name=w[1], count=int(w[2]), props=[])
            elements.append(current)
        elif w[:1] == ["property"]:
            current["props"].append(w[1:])
    pos, out = end, {}
    for el in elements:
        if el["name"] == "vertex":
            assert all(p[0] == "float" for p in el["props"])
            k = len(el["props"])
            out["vertex"] = np.frombuffer(raw, "<f4", el["count"] * k, pos).reshape(el["count"], k)
            out["vertex_names"] = [p[1] for p in el["props"]]
            pos += 4 * k * el["count"]
        else:
            assert el["name"] == "face" and el["props"] == [["list", "uchar", "int", "vertex_indices"]]
            faces = []
            for _ in range(el["count"]):
                n = raw[pos]
                faces.append(np.frombuffer(raw, "<i4", n, pos + 1))
                pos += 1 + 4 * n
            out["face"] = np.array(faces, dtype=np.int32).reshape(el["count"], 3)
    assert pos == len(raw)
    return out


@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_round_trip(tmp_path, with_normals):
    import mesh_ref as mr
    from sanerf_hq_amd.nerf.utils import save_mesh
    m = mr.isosurface(mr.sphere_volume(9, (4.2, 3.9, 4.1), 2.7), 0.0)
    path = str(tmp_path / "m.ply")
    save_mesh(path, torch.from_numpy(m["vertices"]), torch.from_numpy(m["triangles"]), torch.from_numpy(m["normals"]) if with_normals else None)
    got = _read_ply(path)
    assert got["vertex_names"] == (["x", "y", "z", "nx", "ny", "nz"] if with_normals else ["x", "y", "z"])
    assert np.array_equal(got["vertex"][:, :3], m["vertices"]) and np.array_equal(got["face"], m["triangles"])
    if with_normals:
        assert np.array_equal(got["vertex"][:, 3:], m["normals"])
    save_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))               # the empty mesh is a valid file
    got = _read_ply(path)
    assert got["vertex"].shape == (0, 3) and got["face"].shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        save_mesh(path, m["vertices"][:10], m["triangles"])


def test_renderer_methods_exist_and_refuse_grad_mode():
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import NeRFNetwork, NeRFRenderer
    from sanerf_hq_amd.synth import make_opt
    for name in ("lattice_points", "isosurface"):
        assert callable(getattr(rm, name))
    assert callable(NeRFRenderer.density_volume) and callable(NeRFRenderer.extract_mesh)
    model = NeRFNetwork(make_opt(num_steps=[16, 8, 4]))
    assert model.density_thresh == 10
    with pytest.raises(RuntimeError, match="inference query"):
        model.density_volume(8)
    with pytest.raises(RuntimeError, match="inference query"):
        model.extract_mesh(8)
    res, origin, step = model._lattice((5, 3, 9), None)
    assert res == (5, 3, 9) and origin == [-1.0, -1.0, -1.0] and step == [0.5, 1.0, 0.25]
    with pytest.raises(ValueError):
        model._lattice(1, None)
