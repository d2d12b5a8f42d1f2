"""CPU: the device-side SSIM meter (sn_rm_image_ssim_accumulate) is exported and declared, validates its arguments before any launch, its
Python operators refuse CPU tensors, and it leaves the existing meters' surface as it was."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT

NAME = "sn_rm_image_ssim_accumulate"


def test_the_symbol_is_exported_and_declared():
    from sanerf_hq_amd import _lib, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr), f"{NAME} is not declared in include/sanerf_hip.h"
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12 == _lib.ABI_VERSION, "the addition is additive: the ABI version stays 12"
    assert re.search(r"#define\s+SN_SSIM_WORKSPACE_BYTES\s+%d\b" % _lib.SSIM_WORKSPACE_BYTES, hdr)
    assert re.search(r"typedef struct sn_ssim_record \{\s*double ssim_sum;[^}]*double last;[^}]*uint64_t images;[^}]*\} sn_ssim_record;", hdr)
    assert ctypes.sizeof(_lib.SsimRecord) == 24
    assert [f[0] for f in _lib.SsimRecord._fields_] == ["ssim_sum", "last", "images"]
    for f in ("image_ssim_accumulate", "ssim_record", "ssim_workspace", "read_ssim_record"):
        assert callable(getattr(rm, f))
    assert "ssim.hip" in open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()


def test_the_entry_point_validates_its_arguments_before_any_launch():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d = ctypes.c_void_p(64)
    err = l.sn_last_error
    f = l.sn_rm_image_ssim_accumulate
    # (pred, pred_stride, truth, truth_stride, H, W, data_range, record, workspace, stream)
    assert f(None, 3, d, 3, 32, 32, 1.0, d, d, None) == -1 and b"NULL" in err()
    assert f(d, 3, None, 3, 32, 32, 1.0, d, d, None) == -1 and b"NULL" in err()
    assert f(d, 3, d, 3, 32, 32, 1.0, None, d, None) == -1 and b"NULL" in err()
    assert f(d, 3, d, 3, 32, 32, 0.0, d, None, None) == -1 and b"NULL" in err()
    assert f(d, 2, d, 3, 32, 32, 1.0, d, d, None) == -1 and b"stride" in err()
    assert f(d, 5, d, 0, 32, 32, 1.0, d, d, None) == -1 and b"stride" in err()
    assert f(d, 65, d, 3, 32, 32, 1.0, d, d, None) == -2 and b"stride" in err()
    small = f(d, 3, d, 3, 10, 32, 1.0, d, d, None)
    assert small == -5 and b"smaller than the 11 x 11 window" in err(), "a status and a message of its own"
    assert f(d, 3, d, 3, 32, 10, 0.0, d, d, None) == -5 and b"32 x 10" in err()
    assert f(d, 3, d, 3, 0, 0, 1.0, d, d, None) == -5
    assert f(d, 5, d, 3, 1 << 16, 1 << 15, 1.0, d, d, None) == -2 and b"2^31" in err()
    assert f(d, 3, d, 3, 32, 32, 1.0, ctypes.c_void_p(68), d, None) == -1 and b"aligned" in err()
    assert l.sn_abi_version() == 12
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    assert re.search(r"SN_ERR_WINDOW\s*=\s*-5\b", hdr)


def test_python_operators_refuse_cpu_tensors_and_bad_options():
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf.metrics import SSIMMeter
    rec, ws = torch.zeros(3, dtype=torch.int64), torch.zeros(1024, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.image_ssim_accumulate(torch.rand(16, 16, 3), torch.rand(16, 16, 3), rec, ws)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.image_ssim_accumulate(torch.rand(256, 3), torch.rand(256, 3), rec, ws, H=16, W=16, data_range=1.0)
    for name in ("update", "measure", "clear", "report", "write", "prepare_inputs"):
        assert callable(getattr(SSIMMeter, name))
    from sanerf_hq_amd import nerf
    assert nerf.SSIMMeter is SSIMMeter


def test_device_meters_default_surface_is_unchanged():
    """No GPU here: the constructor allocates on the device, so the default's keys are read off measure() on a stand-in record."""
    import inspect
    from sanerf_hq_amd import _lib
    from sanerf_hq_amd.nerf.mask_output import DeviceMeters
    sig = inspect.signature(DeviceMeters.__init__)
    assert list(sig.parameters) == ["self", "device", "num_classes", "eps", "ssim"] and sig.parameters["ssim"].default is False
    assert list(inspect.signature(DeviceMeters.update_rgb).parameters) == ["self", "preds", "truths", "H", "W"]
    m = DeviceMeters.__new__(DeviceMeters)
    m.ssim, m.record = False, torch.zeros(ctypes.sizeof(_lib.EvalRecord) // 8, dtype=torch.int64)
    assert m.measure() == {"mIoU": 0, "loss": 0, "PSNR": 0, "MSE": 0}
    m.ssim, m.ssim_record = True, torch.zeros(3, dtype=torch.int64)
    assert m.measure() == {"mIoU": 0, "loss": 0, "PSNR": 0, "MSE": 0, "SSIM": 0}
    m.clear()
