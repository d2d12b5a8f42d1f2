"""CPU: the mesh smoothing entry points -- declared, exported and bound; the workspace formula as the header states it; arguments refused
before any launch; the Python operators' host-side behaviour; extract_mesh's new parameters."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_mesh_smooth_workspace_bytes", "sn_rm_mesh_smooth_build", "sn_rm_mesh_smooth_steps", "sn_rm_mesh_smooth_emit")
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
    assert re.search(r"^SRCS\s*:=.*\bmesh_smooth\.hip\b", mk, re.M)
    assert re.search(r"^mesh_smooth\.o .*: sn_wave\.h", mk, re.M)


def _formula(V, T):
    """The header's statement: 16 + 32V + up(8V) + 2 up(4V) + up(8 ceil(V / 1024)) + up(24T)."""
    up = lambda n: (n + 15) // 16 * 16
    return 16 + 32 * V + up(8 * V) + 2 * up(4 * V) + up(8 * ((V + 1023) // 1024)) + up(24 * T)


def test_workspace_formula():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    need = l.sn_rm_mesh_smooth_workspace_bytes
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    assert "16 + 32V + up(8V) + 2 up(4V) + up(8 ceil(V / 1024)) + up(24T)" in hdr
    sizes = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4097, 32769, 301196, 600294, 947638, 1893068, (1 << 30) + 1, BIG - 1)
    for V in sizes:
        for T in sizes:
            assert need(V, T) == _formula(V, T), (V, T)
    assert need(0, 0) > 0
    for a, b in zip(sizes[:-1], sizes[1:]):                  # monotone in each argument
        assert need(a, 7) <= need(b, 7) and need(7, a) <= need(7, b)
    V, T = 947638, 1893068                                   # the figures of the documents: 48 bytes a vertex, 24 a triangle
    assert need(V, T) <= 48 * V + 24 * T + 16 * 1024
    for V, T in ((BIG, 0), (0, BIG), (BIG, BIG), (0xFFFFFFFF, 5)):
        assert need(V, T) == 0, (V, T)
        assert b"not supported" in l.sn_last_error()


def _f(*v):
    return (ctypes.c_float * len(v))(*v)


def test_arguments_are_refused_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the device pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    build, steps, emit = l.sn_rm_mesh_smooth_build, l.sn_rm_mesh_smooth_steps, l.sn_rm_mesh_smooth_emit
    p, ws, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(8200)
    V, T = 100, 50
    o, q = _f(0, 0, 0), 0.25
    need = l.sn_rm_mesh_smooth_workspace_bytes(V, T)
    big = 1 << 60
    # V == 0: SN_OK, no pointer is looked at, no argument is judged
    assert build(None, None, 0, 5, None, 0.0, None, 0, None) == OK
    assert steps(0, 5, 3, 7.0, 7.0, 1, None, 0, None) == OK
    assert emit(None, 0, 5, None, 0.0, None, 0, None, None, None, None) == OK
    # build: every pointer it needs (triangles may be NULL only with T == 0)
    for hole in range(4):
        a = [p, p, o, ws]                                    # vertices, triangles, origin, workspace
        a[hole] = None
        assert build(a[0], a[1], V, T, a[2], q, a[3], need, None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert build(p, None, V, 0, o, q, ws, 0, None) == WORKSPACE                        # T == 0 without triangles passes the NULL test
    assert build(p, p, V, T, o, q, ws, need - 1, None) == WORKSPACE and b"too small" in l.sn_last_error()
    assert build(p, p, V, T, o, q, odd, need, None) == INVALID and b"aligned" in l.sn_last_error()
    for bad in (0.0, -0.0, -1.0, float("inf"), float("nan")):
        assert build(p, p, V, T, o, bad, ws, need, None) == INVALID and b"positive and finite" in l.sn_last_error()
        assert emit(p, V, T, o, bad, ws, need, p, None, None, None) == INVALID and b"positive and finite" in l.sn_last_error()
    for bad in (_f(0, float("nan"), 0), _f(float("inf"), 0, 0), _f(0, 0, -float("inf"))):
        assert build(p, p, V, T, bad, q, ws, need, None) == INVALID and b"origin" in l.sn_last_error()
        assert emit(p, V, T, bad, q, ws, need, p, None, None, None) == INVALID and b"origin" in l.sn_last_error()
    assert build(p, p, BIG, T, o, q, ws, big, None) == UNSUPPORTED and b"not supported" in l.sn_last_error()
    assert build(p, p, V, BIG, o, q, ws, big, None) == UNSUPPORTED
    # steps: the factors, then the workspace
    for lam, mu in ((0.0, 0.0), (-0.5, 0.0), (1.5, 0.0), (float("nan"), 0.0), (float("inf"), 0.0)):
        assert steps(V, T, 3, lam, mu, 1, ws, need, None) == INVALID and b"lambda" in l.sn_last_error(), (lam, mu)
    for lam, mu in ((0.5, -0.5), (0.5, -0.25), (0.5, 0.25), (0.5, -1.5), (0.5, float("nan")), (1.0, -1.0), (0.5, -float("inf"))):
        assert steps(V, T, 3, lam, mu, 1, ws, need, None) == INVALID and b"mu" in l.sn_last_error(), (lam, mu)
    assert steps(V, T, 3, 0.5, -0.53, 1, None, need, None) == INVALID and b"NULL" in l.sn_last_error()
    assert steps(V, T, 3, 0.5, -0.53, 1, ws, need - 1, None) == WORKSPACE
    assert steps(V, T, 3, 1.0, 0.0, 0, ws, 0, None) == WORKSPACE                       # lambda = 1 and mu = 0 are accepted
    assert steps(V, T, 3, 0.5, -1.0, 0, ws, 0, None) == WORKSPACE                      # and so is mu = -1
    assert steps(V, T, 3, 0.5, -0.53, 1, odd, need, None) == INVALID and b"aligned" in l.sn_last_error()
    assert steps(BIG, T, 3, 0.5, -0.53, 1, ws, big, None) == UNSUPPORTED
    assert steps(V, BIG, 3, 0.5, -0.53, 1, ws, big, None) == UNSUPPORTED
    assert steps(V, T, 0, 0.5, 0.5, 1, ws, need, None) == INVALID                      # judged even when no iteration is asked for
    # emit: vertices, origin, workspace, out_vertices (normals and flags may be NULL)
    for hole in range(4):
        a = [p, o, ws, p]
        a[hole] = None
        assert emit(a[0], V, T, a[1], q, a[2], need, a[3], None, None, None) == INVALID, hole
        assert b"NULL" in l.sn_last_error()
    assert emit(p, V, T, o, q, ws, need - 1, p, p, p, None) == WORKSPACE
    assert emit(p, V, T, o, q, odd, need, p, p, p, None) == INVALID and b"aligned" in l.sn_last_error()
    assert emit(p, BIG, T, o, q, ws, big, p, p, p, None) == UNSUPPORTED
    assert emit(p, V, BIG, o, q, ws, big, p, p, p, None) == UNSUPPORTED


def test_mesh_smooth_host_side():
    from sanerf_hq_amd import raymarching as rm
    for name in ("mesh_smooth", "mesh_vertex_normals", "mesh_smooth_build", "mesh_smooth_steps", "mesh_smooth_emit", "smooth_quantisation"):
        assert callable(getattr(rm, name))
    mesh = {"vertices": torch.zeros(4, 3), "normals": None, "triangles": torch.zeros(2, 3, dtype=torch.int32)}
    for n in (-1, 2.5, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="non-negative integer"):
            rm.mesh_smooth(mesh, iterations=n)
    for lam in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lambda"):
            rm.mesh_smooth(mesh, lam=lam, mu=0.0)
    for mu in (-0.5, -0.25, 0.25, -1.5, float("nan")):
        with pytest.raises(ValueError, match="mu ="):
            rm.mesh_smooth(mesh, lam=0.5, mu=mu)
    with pytest.raises(ValueError, match="together"):
        rm.mesh_smooth(mesh, origin=(0, 0, 0))
    with pytest.raises(ValueError, match="together"):
        rm.mesh_vertex_normals(mesh, quantum=1.0)
    with pytest.raises(ValueError, match="3 entries"):
        rm.mesh_smooth(mesh, origin=(0, 0), quantum=1.0)
    for quantum in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError, match="positive and finite"):
            rm.mesh_smooth(mesh, origin=(0, 0, 0), quantum=quantum)
    with pytest.raises(ValueError, match="origin"):
        rm.mesh_smooth(mesh, origin=(0, float("inf"), 0), quantum=1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mesh_smooth(mesh, origin=(0, 0, 0), quantum=1.0)                  # a host tensor: refused, no fallback
    with pytest.raises(RuntimeError, match=r"\[T,3\]"):
        rm.mesh_smooth(dict(mesh, triangles=torch.zeros(6, dtype=torch.int32)))
    sig = inspect.signature(rm.mesh_smooth).parameters
    assert [k for k in sig] == ["mesh", "iterations", "lam", "mu", "pin_open", "origin", "quantum", "normals", "return_flags"]
    assert (sig["iterations"].default, sig["lam"].default, sig["mu"].default, sig["pin_open"].default) == (10, 0.5, -0.53, True)
    assert sig["origin"].default is None and sig["quantum"].default is None and sig["normals"].default is None and sig["return_flags"].default is False
    assert [k for k in inspect.signature(rm.mesh_vertex_normals).parameters] == ["mesh", "origin", "quantum"]
    assert "NOTHING is read back" in rm.mesh_smooth.__doc__


def test_extract_mesh_has_the_new_parameters():
    from sanerf_hq_amd.nerf import NeRFRenderer
    sig = inspect.signature(NeRFRenderer.extract_mesh).parameters
    assert (sig["smooth"].default, sig["smooth_lambda"].default, sig["smooth_mu"].default, sig["smooth_pin_open"].default) == (0, 0.5, -0.53, True)
    assert [k for k in sig][:10] == ["self", "resolution", "threshold", "aabb", "instance_ids", "invert", "normals", "min_component_triangles",
                                     "keep_largest", "simplify"]                # the earlier parameters keep their places
    assert [k for k in sig][10:14] == ["vertex_colors", "vertex_labels", "probe_samples", "probe_step"]
    for bad in (-1, 1.5, 2.0, True, "2"):                  # refused before anything is evaluated (self is not touched)
        with pytest.raises(ValueError, match="smooth"):
            NeRFRenderer.extract_mesh(None, 8, smooth=bad)
    for kw in (dict(smooth_lambda=0.0), dict(smooth_lambda=1.5), dict(smooth_mu=-0.5), dict(smooth_mu=0.2)):
        with pytest.raises(ValueError, match="lambda|mu"):
            NeRFRenderer.extract_mesh(None, 8, smooth=2, **kw)
