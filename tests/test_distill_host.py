"""CPU: the feature-distillation entry points (sn_rm_feature_distill_loss, sn_rm_feature_map) are exported and declared, validate their
arguments before any launch, their Python operators refuse CPU tensors, and the host logic of nerf.sam_step (Cache, use_cache) is the
reference's."""
import ctypes
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

from helpers import ROOT

NAMES = ("sn_rm_feature_distill_workspace_bytes", "sn_rm_feature_distill_loss", "sn_rm_feature_map")


def test_the_symbols_are_exported_and_declared():
    from sanerf_hq_amd import _lib, nerf, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/sanerf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.EXPORTED_SYMBOLS
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12 == _lib.ABI_VERSION, "the addition is additive: the ABI version stays 12"
    assert re.search(r"#define\s+SN_DISTILL_WORKSPACE_FIXED_BYTES\s+%d\b" % _lib.DISTILL_WORKSPACE_FIXED_BYTES, hdr)
    assert "i1 = i0 + (i0 < n_in - 1)" in hdr and "l0 = 1 - l1" in hdr, "the header states the quantity"
    for f in ("feature_distill_loss", "feature_map"):
        assert callable(getattr(rm, f))
    for f in ("sam_train_loss", "sam_eval_loss", "use_cache", "Cache"):
        assert callable(getattr(nerf, f))
    assert "distill.hip" in open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()


def test_workspace_bytes():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    f, fixed = l.sn_rm_feature_distill_workspace_bytes, _lib.DISTILL_WORKSPACE_FIXED_BYTES
    assert f(64, 64, 256, 64, 64) == fixed, "the identity case needs the fixed part alone"
    assert f(24, 24, 256, 32, 32) == fixed + 4 * 256 * 32 * 32
    assert f(11, 13, 3, 5, 7) == fixed + 4 * 3 * 5 * 7
    assert f(0, 64, 256, 64, 64) == 0 and f(1 << 12, 1 << 12, 256, 64, 64) == 0 and f(64, 64, 256, 1 << 12, 1 << 12) == 0
    assert l.sn_debug_set(b"distill_general", 1) == 0
    try:
        assert f(64, 64, 256, 64, 64) == fixed + 4 * 256 * 64 * 64, "the forced general path needs its d buffer"
    finally:
        assert l.sn_debug_set(b"distill_general", 0) == 0
    assert f(64, 64, 256, 64, 64) == fixed


def test_the_entry_points_validate_their_arguments_before_any_launch():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d = ctypes.c_void_p(64)
    err = l.sn_last_error
    f, big = l.sn_rm_feature_distill_loss, 1 << 30
    # (feat, feat_stride, h, w, C, target, Ho, Wo, scale, scale_dev, loss, grad_feat, resized, workspace, workspace_bytes, stream)
    assert f(None, 4, 8, 8, 4, d, 8, 8, 1.0, None, d, d, d, d, big, None) == -1 and b"NULL" in err()
    assert f(d, 4, 8, 8, 4, None, 8, 8, 1.0, None, d, d, d, d, big, None) == -1 and b"NULL" in err()
    assert f(d, 4, 8, 8, 4, d, 8, 8, 1.0, None, None, d, d, d, big, None) == -1 and b"NULL" in err()
    assert f(d, 4, 8, 8, 4, d, 8, 8, 1.0, None, d, d, d, None, big, None) == -1 and b"NULL" in err()
    assert f(d, 3, 8, 8, 4, d, 8, 8, 1.0, None, d, d, d, d, big, None) == -1 and b"feat_stride" in err()
    for sizes in ((0, 8, 4, 8, 8), (8, 0, 4, 8, 8), (8, 8, 0, 8, 8), (8, 8, 4, 0, 8), (8, 8, 4, 8, 0)):
        h, w, C, Ho, Wo = sizes
        assert f(d, 4, h, w, C, d, Ho, Wo, 1.0, None, d, d, d, d, big, None) == -1 and b"at least 1" in err()
    assert f(d, 256, 1 << 12, 1 << 12, 256, d, 8, 8, 1.0, None, d, d, d, d, big, None) == -2 and b"2^31" in err()
    assert f(d, 256, 8, 8, 256, d, 1 << 12, 1 << 12, 1.0, None, d, d, d, d, big, None) == -2 and b"2^31" in err()
    assert f(d, 1, 1 << 16, 1 << 15, 1, d, 8, 8, 1.0, None, d, d, d, d, big, None) == -2 and b"2^31" in err()
    assert f(d, 4, 8, 8, 4, d, 8, 8, 1.0, None, d, d, d, ctypes.c_void_p(68), big, None) == -1 and b"aligned" in err()
    fixed = _lib.DISTILL_WORKSPACE_FIXED_BYTES
    assert f(d, 4, 8, 8, 4, d, 8, 8, 1.0, None, d, d, d, d, fixed - 1, None) == -4 and b"workspace" in err()
    assert f(d, 4, 8, 8, 4, d, 9, 8, 1.0, None, d, d, d, d, fixed, None) == -4, "a resize with a gradient needs the d buffer"
    assert f(d, 4, 8, 8, 4, d, 9, 8, 1.0, None, d, d, d, d, fixed + 4 * 4 * 9 * 8 - 1, None) == -4
    g = l.sn_rm_feature_map
    # (feat, feat_stride, h, w, C, Ho, Wo, out, stream)
    assert g(None, 4, 8, 8, 4, 8, 8, d, None) == -1 and b"NULL" in err()
    assert g(d, 4, 8, 8, 4, 8, 8, None, None) == -1 and b"NULL" in err()
    assert g(d, 3, 8, 8, 4, 8, 8, d, None) == -1 and b"feat_stride" in err()
    assert g(d, 4, 8, 8, 4, 0, 8, d, None) == -1 and b"at least 1" in err()
    assert g(d, 256, 8, 8, 256, 1 << 12, 1 << 12, d, None) == -2 and b"2^31" in err()
    assert l.sn_debug_set(b"no_such_key", 1) != 0
    assert l.sn_abi_version() == 12


def test_python_operators_refuse_cpu_tensors_and_bad_shapes():
    from sanerf_hq_amd import raymarching as rm
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.feature_distill_loss(torch.rand(16, 4), 4, 4, torch.rand(1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.feature_map(torch.rand(16, 4), 4, 4)


def test_sam_cache_semantics_and_use_cache():
    from sanerf_hq_amd.nerf import sam_step
    c = sam_step.Cache(size=3)
    assert not c.full() and c.size == 3 and c.key == 0
    for i in range(3):
        assert not c.full()
        c.insert({"i": i})
    assert c.full() and c.key == 0 and [c.data[k]["i"] for k in range(3)] == [0, 1, 2]
    c.insert({"i": 3})                                                    # a ring: the oldest entry is replaced
    assert c.full() and c.key == 1 and [c.data[k]["i"] for k in range(3)] == [3, 1, 2]
    assert c.get(2)["i"] == 2
    random.seed(4)
    want = [random.randint(0, 2) for _ in range(8)]
    random.seed(4)
    assert [c.get()["i"] for _ in range(8)] == [c.data[k]["i"] for k in want], "get() draws random.randint(0, len - 1) as the reference does"

    opt = SimpleNamespace(with_sam=True, cache_size=3, cache_interval=4)
    assert [sam_step.use_cache(opt, c, s) for s in range(6)] == [False, True, True, True, False, True]
    assert not sam_step.use_cache(opt, sam_step.Cache(size=3), 1), "not before the cache is full"
    assert not sam_step.use_cache(SimpleNamespace(with_sam=False, cache_size=3, cache_interval=4), c, 1)
    assert not sam_step.use_cache(SimpleNamespace(with_sam=True, cache_size=0, cache_interval=4), sam_step.Cache(size=0), 1)
    assert sam_step.use_cache(opt, c, 1) is True
