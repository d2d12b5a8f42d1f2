"""CPU: the RGB step's loss tail (sn_rm_rgb_loss) is exported, declared and bound, validates its arguments before any launch, its Python
operator refuses CPU tensors and bad shapes, and the host logic of nerf.rgb_step (update_proposal_at, adapt_num_rays, step_background)
is the reference's (tests/golden/rgb_step.npz: what its own train_step passed and computed)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import ROOT

NAME = "sn_rm_rgb_loss"
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rgb_step.npz"))


def test_the_symbol_is_exported_declared_and_bound():
    from sanerf_hq_amd import _lib, nerf, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr), f"{NAME} is not declared in include/sanerf_hip.h"
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert NAME in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[NAME][1]) == 23
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12 == _lib.ABI_VERSION, "the addition is additive: the ABI version stays 12"
    assert re.search(r"#define\s+SN_RGB_LOSS_WORKSPACE_BYTES\s+%d\b" % _lib.RGB_LOSS_WORKSPACE_BYTES, hdr)
    assert re.search(r"#define\s+SN_RGB_LOSS_MAX_WORKGROUPS\s+%d\b" % _lib.RGB_LOSS_MAX_WORKGROUPS, hdr), "the header states the cap of the grid"
    assert _lib.RGB_LOSS_WORKSPACE_BYTES == 64 + 2 * 8 * _lib.RGB_LOSS_MAX_WORKGROUPS and _lib.RGB_LOSS_WORKSPACE_BYTES % 8 == 0
    assert re.search(r"typedef struct sn_rgb_loss_record \{ float total, mse, entropy, reserved; \}", hdr)
    assert "gt_c   = truth_c * a + b_c * (1 - a)" in hdr and "(1 - weights_sum) * b_c" in hdr and "log2f(1 - c) - log2f(c)" in hdr, "the header states the quantity"
    assert callable(rm.rgb_loss)
    for f in ("step_background", "update_proposal_at", "rgb_train_loss", "rgb_train_step", "adapt_num_rays", "rgb_eval_loss"):
        assert callable(getattr(nerf, f)), f
    csrc = os.path.join(ROOT, "sanerf-hq_amd", "csrc")
    assert re.search(r"^SRCS\s*:=.*\brgb_loss\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert os.path.exists(os.path.join(csrc, "rgb_loss.hip"))


def test_the_entry_point_validates_its_arguments_before_any_launch():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d, err, f = ctypes.c_void_p(64), l.sn_last_error, l.sn_rm_rgb_loss

    def call(image=d, image_stride=3, ws=d, truth=d, truth_stride=4, ch=4, N=8, bg_value=1.0, bg=None, bg_rows=0, has_bg=1, lam=0.0,
             record=d, workspace=d):
        return f(image, image_stride, ws, truth, truth_stride, ch, N, bg_value, bg, bg_rows, has_bg, lam, None, 0.0, None, 0.0, d, d, record, d, d,
                 workspace, None)

    for kw in (dict(image=None), dict(ws=None), dict(truth=None), dict(record=None), dict(workspace=None)):
        assert call(**kw) == -1 and b"NULL" in err(), kw
    assert call(image_stride=2) == -1 and b"image_stride" in err()
    assert call(truth_stride=3, ch=4) == -1 and b"truth_stride" in err()
    assert call(truth_stride=2, ch=3) == -1 and b"truth_stride" in err()
    for ch in (0, 1, 2, 5):
        assert call(truth_stride=8, ch=ch) == -1 and b"truth_channels" in err()
    for rows in (2, 7, 9):
        assert call(bg=d, bg_rows=rows) == -1 and b"bg_rows" in err()
    assert call(bg=None, bg_rows=1) == -1 and b"NULL bg" in err()
    assert call(bg=None, bg_rows=8) == -1 and b"NULL bg" in err()
    assert call(N=0) == -1 and b"at least 1" in err()
    assert call(workspace=ctypes.c_void_p(68)) == -1 and b"aligned" in err()
    assert call(N=1 << 30) == -2 and b"2^30" in err()
    assert l.sn_abi_version() == 12


def test_the_python_operator_refuses_cpu_tensors_and_bad_shapes():
    from sanerf_hq_amd import raymarching as rm
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.rgb_loss(torch.rand(8, 3), torch.rand(8), torch.rand(8, 4))
    with pytest.raises(RuntimeError, match=r"\[N,3\]"):
        rm.rgb_loss(torch.rand(8, 4), torch.rand(8), torch.rand(8, 4))
    with pytest.raises(RuntimeError, match=r"\[N,3\]"):
        rm.rgb_loss(torch.rand(24), torch.rand(8), torch.rand(8, 4))
    with pytest.raises(RuntimeError, match="at most two"):
        rm.rgb_loss(torch.rand(8, 3), torch.rand(8), torch.rand(8, 4), extras=[(torch.rand(1), 1.0)] * 3)
    with pytest.raises(RuntimeError, match="pairs"):
        rm.rgb_loss(torch.rand(8, 3), torch.rand(8), torch.rand(8, 4), extras=[torch.rand(1)])


def test_update_proposal_and_adaptive_num_rays_equal_the_reference():
    from sanerf_hq_amd.nerf import rgb_step
    for name in (str(c) for c in GOLD["train_cases"]):
        g = lambda k: GOLD[f"{name}.{k}"]   # noqa: E731
        opt = SimpleNamespace(with_sam=False, adaptive_num_rays=True, num_points=int(g("num_points")), num_rays=int(g("num_rays_before")))
        assert rgb_step.update_proposal_at(opt, int(g("global_step"))) is bool(g("update_proposal")), name
        assert rgb_step.adapt_num_rays(opt, {"num_points": int(g("num_points_out"))}) == int(g("num_rays_after")) == opt.num_rays, name
    opt = SimpleNamespace(with_sam=False)
    for step in range(3011):
        assert rgb_step.update_proposal_at(opt, step) is ((not opt.with_sam) and (step <= 3000 or step % 5 == 0))   # trainer.py:372-373
    assert [s for s in range(2998, 3011) if rgb_step.update_proposal_at(opt, s)] == [2998, 2999, 3000, 3005, 3010]
    assert not any(rgb_step.update_proposal_at(SimpleNamespace(with_sam=True), s) for s in (0, 5, 3000, 3005))
    fixed = SimpleNamespace(adaptive_num_rays=False, num_points=1 << 12, num_rays=77)
    assert rgb_step.adapt_num_rays(fixed, {"num_points": 5}) == 77 == fixed.num_rays


def test_step_background():
    from sanerf_hq_amd.nerf import rgb_step
    dev = torch.device("cpu")
    for bg in ("white", "last_sample"):
        got = rgb_step.step_background(SimpleNamespace(background=bg), 16, dev)
        assert got == 1 and not torch.is_tensor(got)
    opt = SimpleNamespace(background="random")
    torch.manual_seed(3)
    want = torch.rand(16, 3)
    torch.manual_seed(3)
    assert torch.equal(rgb_step.step_background(opt, 16, dev), want), "one torch.rand(N, 3), as trainer.py:358 draws it"
    buf = torch.zeros(16, 3)
    assert rgb_step.step_background(opt, 16, dev, uniform=buf) is buf, "the caller's buffer itself, so that a captured step can refill it"
    with pytest.raises(RuntimeError, match="uniform"):
        rgb_step.step_background(opt, 16, dev, uniform=torch.zeros(15, 3))
