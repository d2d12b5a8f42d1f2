"""CPU: the two entry points of the object render (sn_rm_mask_point_labels, sn_rm_object_composite) are exported and declared, the ABI
version is unchanged, and they validate their arguments before any launch."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT

NAMES = ("sn_rm_mask_point_labels", "sn_rm_object_composite")
INVALID, UNSUPPORTED = -1, -2


def test_the_symbols_are_exported_and_declared():
    from sanerf_hq_amd import _lib, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/sanerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.EXPORTED_SYMBOLS
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12 == _lib.ABI_VERSION, "the additions are additive: the ABI version stays 12"
    for f in ("mask_point_labels", "mask_point_labels_fusable", "object_composite", "keep_mask_of"):
        assert callable(getattr(rm, f))
    assert "object.hip" in open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    from sanerf_hq_amd.nerf.renderer import NeRFRenderer
    assert callable(NeRFRenderer.render_object)


def _descs(L=16, E=15, K=2, layers=3, bias=False):
    from sanerf_hq_amd import _lib
    g = _lib.GridDesc()
    g.embeddings, g.table_dtype, g.D, g.C, g.L, g.S, g.H = 64, _lib.SN_F32, 3, 8, L, 1.0, 16
    for l in range(L + 1):
        g.offsets[l] = 4096 * l
    m = _lib.MlpDesc()
    m.num_layers, m.activation, m.skip_mask = layers, 1, 0
    dims = [L * 8 + E] + [256] * (layers - 1) + [K]
    for i, d in enumerate(dims):
        m.dims[i] = d
    for l in range(layers):
        m.weight[l] = 64
        m.bias[l] = 64 if bias else None
    return g, m


def test_point_labels_answers_errors_not_launches():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    f, err, d = l.sn_rm_mask_point_labels, l.sn_last_error, ctypes.c_void_p(64)
    g, m = _descs()
    ok_args = lambda T=32, E=15, gg=g, mm=m: (d, d, d, 10, T, E, 1.0, ctypes.byref(gg), ctypes.byref(mm), d, None, d, 1 << 24, None)
    # (xyzs, extra, live, N, T, E, bound, grid, mlp, labels, logits, workspace, workspace_bytes, stream)
    assert f(None, d, d, 10, 32, 15, 1.0, ctypes.byref(g), ctypes.byref(m), d, None, d, 1 << 24, None) == INVALID and b"device pointers" in err()
    assert f(d, d, None, 10, 32, 15, 1.0, ctypes.byref(g), ctypes.byref(m), d, None, d, 1 << 24, None) == INVALID
    assert f(d, d, d, 10, 32, 15, 1.0, ctypes.byref(g), ctypes.byref(m), None, None, d, 1 << 24, None) == INVALID
    assert f(d, d, d, 10, 32, 15, 1.0, None, ctypes.byref(m), d, None, d, 1 << 24, None) == INVALID and b"NULL" in err()
    assert f(d, d, d, 10, 32, 15, 1.0, ctypes.byref(g), None, d, None, d, 1 << 24, None) == INVALID
    assert f(d, d, d, 10, 32, 15, 0.0, ctypes.byref(g), ctypes.byref(m), d, None, d, 1 << 24, None) == INVALID and b"bound" in err()
    for T in (3, 2, 1, 24, 256):
        assert f(*ok_args(T=T)) == UNSUPPORTED and b"power of two" in err(), T
    g17, m17 = _descs(K=17)
    assert f(*ok_args(gg=g17, mm=m17)) == UNSUPPORTED and b"<= 16 outputs" in err()
    gb, mb = _descs(bias=True)
    assert f(*ok_args(gg=gb, mm=mb)) == UNSUPPORTED and b"biases" in err()
    g4, m4 = _descs(layers=4)
    assert f(*ok_args(gg=g4, mm=m4)) == UNSUPPORTED and b"3 bias-free layers" in err()
    g2, m2 = _descs()
    g2.C = 2
    assert f(*ok_args(gg=g2, mm=m2)) == UNSUPPORTED and b"level_dim 8" in err()
    ge, me = _descs(E=17)
    assert f(*ok_args(E=17, gg=ge, mm=me)) == UNSUPPORTED
    gw, mw = _descs()
    mw.dims[0] = 100
    assert f(*ok_args(gg=gw, mm=mw)) == INVALID and b"input width" in err()
    # N = 0: nothing to do, whatever else is passed
    assert f(None, None, None, 0, 32, 15, 1.0, ctypes.byref(g), ctypes.byref(m), None, None, None, 0, None) == 0
    assert l.sn_abi_version() == 12


def test_object_composite_answers_errors_not_launches():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    f, err, d = l.sn_rm_object_composite, l.sn_last_error, ctypes.c_void_p(64)
    # (labels, sigmas, real_bins, geo_feat, rays_d, N, T, keep_mask, invert, last_sample_opaque, weights_sum, depth, f_image, weights, stream)
    for hole in range(5):
        ins = [d] * 5
        ins[hole] = None
        assert f(*ins, 4, 8, 1, 0, 0, d, d, d, None, None) == INVALID and b"NULL" in err(), hole
    for hole in range(3):
        outs = [d] * 3
        outs[hole] = None
        assert f(d, d, d, d, d, 4, 8, 1, 0, 0, *outs, None, None) == INVALID and b"NULL" in err(), hole
    assert f(d, d, d, d, d, 4, 0, 1, 0, 0, d, d, d, None, None) == INVALID and b"T must be" in err()
    assert f(d, d, d, d, d, 1 << 28, 8, 1, 0, 0, d, d, d, None, None) == INVALID and b"rays per call" in err()
    assert f(None, None, None, None, None, 0, 8, 1, 0, 0, None, None, None, None, None) == 0


def test_python_operators_check_their_arguments():
    from sanerf_hq_amd import raymarching as rm
    assert rm.keep_mask_of([]) == 0 and rm.keep_mask_of([0, 3, 3]) == 0b1001 and rm.keep_mask_of(range(32)) == 0xFFFFFFFF
    with pytest.raises(ValueError, match="outside"):
        rm.keep_mask_of([32])
    with pytest.raises(ValueError, match="outside"):
        rm.keep_mask_of([-1])
    N, T = 3, 4
    sg, rb, geo, rd = torch.rand(N, T), torch.rand(N, T + 1), torch.rand(N, T, 15), torch.rand(N, 3)
    with pytest.raises(RuntimeError, match="uint8"):
        rm.object_composite(torch.zeros(N, T, dtype=torch.int64), sg, rb, geo, rd, 1)
    with pytest.raises(RuntimeError, match="do not match"):
        rm.object_composite(torch.zeros(N, T, dtype=torch.uint8), sg, rb[:, :-1], geo, rd, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.object_composite(torch.zeros(N, T, dtype=torch.uint8), sg, rb, geo, rd, 1)


def test_the_mesh_branch_of_run_still_returns_nothing():
    """run() with opt.render_mesh keeps the reference's behaviour (an empty dict); render_object is the working feature beside it."""
    import inspect
    from sanerf_hq_amd.nerf.renderer import NeRFRenderer
    src = inspect.getsource(NeRFRenderer.run)
    assert "if self.opt.render_mesh:\n            return {}" in src
    sig = inspect.signature(NeRFRenderer.render_object)
    assert list(sig.parameters) == ["self", "rays_o", "rays_d", "instance_ids", "invert", "staged", "cam_near_far", "bg_color", "H", "W"]
