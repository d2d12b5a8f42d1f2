"""CPU: the mask field's output stage and the device-side evaluation meters (sn_rm_mask_output, sn_rm_mask_eval_accumulate,
sn_rm_image_sqerr_accumulate) are exported and declared, validate their arguments before any launch, their Python operators refuse CPU
tensors, and tests/golden/mask_output.npz (tools/gen_golden_mask_output.py: the reference's own test_step / eval_step lines, overlays and
meters on the CPU) agrees with a float64 restatement written here and keeps its recorded margins."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT, golden

CASES = ("k1", "k2", "k3", "k8", "k32")
SHAPES = {"k1": (33, 31, 1, 1), "k2": (33, 31, 2, 2), "k3": (33, 31, 3, 3), "k8": (33, 31, 8, 8), "k32": (23, 25, 32, 32)}
VARIANTS = [(m, r) for m in ("heatmap", "composition", "mask") for r in ("all", "one")]
NEW = ("sn_rm_mask_output", "sn_rm_mask_eval_accumulate", "sn_rm_image_sqerr_accumulate")


# ---- the float64 restatement (also what the GPU test uses for inputs the fixture does not hold) ----------------------------------------
def probs_f64(logits):
    x = logits.astype(np.float64)
    if x.shape[-1] == 1:
        return 1.0 / (1.0 + np.exp(-x))
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def overlay_f64(mode, render_id, p, image, color_map, alpha, bg):
    """trainer.py:741-777 + utils.py:49-77 in float64; render_id -1 = all."""
    K = p.shape[-1]
    ids, conf = p.argmax(-1), p.max(-1)
    cm, img = color_map.astype(np.float64), image.astype(np.float64)
    if mode == "heatmap":
        if 0 <= render_id < K:
            return cm[render_id][None, :] * p[:, render_id][:, None]
        return cm[ids] * conf[:, None]
    if mode == "composition":
        over = cm[ids].copy()
        if render_id != -1:
            keep = ids != render_id
            over[keep] = img[keep]
        return img * alpha + over * (1 - alpha)
    if mode == "mask":
        m = (ids == render_id).astype(np.float64)[:, None]
        return img * m + (1 - m) * bg.astype(np.float64)[None, :]
    return img


def eval_f64(logits, labels, C, eps):
    """(mean NLL over the labelled pixels or 0, mIoU, counts [3,32]) of sn_rm_mask_eval_accumulate's contract in float64."""
    p = probs_f64(logits)
    K = p.shape[-1]
    ids = p.argmax(-1)
    valid = (labels >= 0) & (labels < K)
    py = np.where(valid, np.take_along_axis(p, np.clip(labels, 0, K - 1)[:, None], -1)[:, 0], 1.0)
    nll = np.where(valid, -np.log(np.clip(py, eps, 1 - eps)), 0.0)
    labelled = int((labels != -1).sum())
    loss = float(nll.sum() / labelled) if labelled else 0.0
    counts = np.zeros((3, 32), dtype=np.int64)
    ious = []
    for i in range(C):
        counts[0, i] = ((ids == i) & (labels == i)).sum()
        counts[1, i] = (ids == i).sum()
        counts[2, i] = (labels == i).sum()
        union = ((ids == i) | (labels == i)).sum()
        assert union == counts[1, i] + counts[2, i] - counts[0, i]
        if union > 0:
            ious.append(counts[0, i] / union)
    return loss, float(np.mean(ious)), counts


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_declared():
    from sanerf_hq_amd import _lib, raymarching as rm
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/sanerf_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.EXPORTED_SYMBOLS
    assert "#define SN_ABI_VERSION 12" in hdr and lib.sn_abi_version() == 12, "the additions are additive: the ABI version stays 12"
    assert re.search(r"#define\s+SN_MASK_EVAL_WORKSPACE_BYTES\s+%d\b" % _lib.MASK_EVAL_WORKSPACE_BYTES, hdr)
    assert ctypes.sizeof(_lib.EvalRecord) == 4 * 8 + 2 * 8 + 3 * 32 * 8
    for f in ("mask_output", "mask_eval_accumulate", "image_sqerr_accumulate"):
        assert callable(getattr(rm, f))
    src = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert "mask_output.hip" in src


def test_entry_points_validate_their_arguments_before_any_launch():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d = ctypes.c_void_p(64)
    err = l.sn_last_error
    # mask_output(logits, N, K, image, image_stride, color_map, C, mode, render_id, alpha, bg, probs, instance_id, confidence, rgb, rgb8, stream)
    assert l.sn_rm_mask_output(None, 16, 2, d, 3, d, 100, 1, -1, 0.7, d, d, d, d, d, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_mask_output(d, 16, 0, d, 3, d, 100, 1, -1, 0.7, d, d, d, d, d, d, None) == -1 and b"K = 0" in err()
    assert l.sn_rm_mask_output(d, 16, 33, d, 3, d, 100, 1, -1, 0.7, d, d, d, d, d, d, None) == -2 and b"K=33" in err()
    assert l.sn_rm_mask_output(d, 16, 8, d, 3, d, 7, 1, -1, 0.7, d, d, d, d, d, d, None) == -1 and b"C >= K" in err()
    assert l.sn_rm_mask_output(d, 1 << 31, 2, d, 3, d, 100, 1, -1, 0.7, d, d, d, d, d, d, None) == -2 and b"2^31" in err()
    assert l.sn_rm_mask_output(d, 16, 2, d, 3, d, 100, 4, -1, 0.7, d, d, d, d, d, d, None) == -1 and b"mode" in err()
    assert l.sn_rm_mask_output(d, 16, 2, d, 3, d, 100, 1, -1, 0.7, d, None, None, None, None, None, None) == -1 and b"no output" in err()
    assert l.sn_rm_mask_output(d, 16, 2, None, 3, d, 100, 2, -1, 0.7, d, None, None, None, d, None, None) == -1 and b"NULL image" in err()
    assert l.sn_rm_mask_output(d, 16, 2, d, 2, d, 100, 2, -1, 0.7, d, None, None, None, d, None, None) == -1 and b"stride" in err()
    assert l.sn_rm_mask_output(d, 16, 2, d, 3, None, 100, 2, -1, 0.7, d, None, None, None, d, None, None) == -1 and b"color_map" in err()
    assert l.sn_rm_mask_output(d, 16, 2, d, 3, d, 100, 3, 1, 0.7, None, None, None, None, d, None, None) == -1 and b"bg" in err()
    assert l.sn_rm_mask_output(d, 16, 2, d, 3, d, 100, 1, -1, 0.7, d, None, None, None, None, ctypes.c_void_p(66), None) == -1 and b"aligned" in err()
    assert l.sn_rm_mask_output(None, 0, 2, None, 0, None, 0, 1, -1, 0.7, None, None, None, None, None, None, None) == 0
    # mask_eval_accumulate(logits, labels, N, K, C, eps, record, workspace, stream)
    assert l.sn_rm_mask_eval_accumulate(d, None, 16, 2, 2, 1e-6, d, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_mask_eval_accumulate(d, d, 16, 2, 2, 1e-6, None, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_mask_eval_accumulate(d, d, 16, 0, 2, 1e-6, d, d, None) == -1 and b"K = 0" in err()
    assert l.sn_rm_mask_eval_accumulate(d, d, 16, 33, 33, 1e-6, d, d, None) == -2 and b"K=33" in err()
    assert l.sn_rm_mask_eval_accumulate(d, d, 16, 3, 2, 1e-6, d, d, None) == -1 and b"C >= K" in err()
    assert l.sn_rm_mask_eval_accumulate(d, d, 16, 3, 33, 1e-6, d, d, None) == -2 and b"C=33" in err()
    assert l.sn_rm_mask_eval_accumulate(d, d, 1 << 31, 3, 3, 1e-6, d, d, None) == -2 and b"2^31" in err()
    assert l.sn_rm_mask_eval_accumulate(None, None, 0, 3, 3, 1e-6, None, None, None) == 0
    # image_sqerr_accumulate(pred, pred_stride, truth, truth_stride, N, record, workspace, stream)
    assert l.sn_rm_image_sqerr_accumulate(None, 3, d, 3, 16, d, d, None) == -1 and b"NULL" in err()
    assert l.sn_rm_image_sqerr_accumulate(d, 3, d, 3, 16, d, None, None) == -1 and b"NULL" in err()
    assert l.sn_rm_image_sqerr_accumulate(d, 2, d, 3, 16, d, d, None) == -1 and b"stride" in err()
    assert l.sn_rm_image_sqerr_accumulate(d, 5, d, 3, 1 << 31, d, d, None) == -2 and b"2^31" in err()
    assert l.sn_rm_image_sqerr_accumulate(None, 3, None, 3, 0, None, None, None) == 0
    assert l.sn_abi_version() == 12


def test_python_operators_refuse_cpu_tensors_and_bad_options():
    import torch
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.nerf import mask_output as mo
    import types
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mask_output(torch.zeros(8, 2), color_map=torch.rand(100, 3), mode="heatmap")
    rec, ws = torch.zeros(104, dtype=torch.int64), torch.zeros(1024, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mask_eval_accumulate(torch.zeros(8, 2), torch.zeros(8, dtype=torch.long), rec, ws)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.image_sqerr_accumulate(torch.rand(8, 3), torch.rand(8, 3), rec, ws)
    with pytest.raises(ValueError, match="mode"):
        rm.mask_output(torch.zeros(8, 2), mode="overlay")
    opt = types.SimpleNamespace(n_inst=2, epsilon=1e-6, label_regularization_weight=0.1)
    with pytest.raises(NotImplementedError, match="label_regularization"):
        mo.mask_eval_step({"instance_mask_logits": torch.zeros(8, 2)}, {"masks": torch.zeros(8)}, opt, None)
    cm = mo.reference_color_map()                    # matplotlib is a dependency of the reference, present where this suite runs
    g = golden("mask_output")
    assert cm.shape == (100, 3) and cm.dtype == torch.float32 and np.array_equal(cm.numpy(), g["color_map"])


def test_fixture_agrees_with_the_float64_restatement():
    g = golden("mask_output")
    assert list(g["cases"]) == list(CASES) and list(g["strided_cases"]) == ["k3"]
    cm, alpha, bg, eps = g["color_map"], float(g["alpha"]), g["bg"], float(g["epsilon"])
    assert cm.shape == (100, 3) and cm.dtype == np.float32
    for c in CASES:
        H, W, K, C = (int(v) for v in g[c + ".shape"])
        assert (H, W, K, C) == SHAPES[c]
        logits, image, labels = g[c + ".logits"], g[c + ".image"], g[c + ".labels"]
        assert logits.shape == (H * W, K) and image.shape == (H * W, 3) and labels.shape == (H * W,)
        assert (H * W * 3) % 4 != 0 and (H * W) % 256 != 0, "the cases end inside a tile and inside a dword of the 8-bit image"
        p = probs_f64(logits)
        assert np.array_equal(p.argmax(-1), g[c + ".ids"])
        np.testing.assert_allclose(g[c + ".probs"], p, rtol=1e-6)
        np.testing.assert_allclose(g[c + ".conf"], p.max(-1), rtol=1e-6)
        one = int(g[c + ".render_one"])
        assert one == K - 1
        for mode, r in VARIANTS:
            want = overlay_f64(mode, -1 if r == "all" else one, p, image, cm, alpha, bg)
            got = g[f"{c}.{mode}.{r}.rgb"]
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-30)
            assert np.array_equal(g[f"{c}.{mode}.{r}.rgb8"], np.trunc(np.clip(255.0 * want, 0, 255)).astype(np.uint8)), (c, mode, r)
        assert np.array_equal(g[c + ".none.rgb8"], np.trunc(255.0 * image.astype(np.float64)).astype(np.uint8))
        loss, miou, counts = eval_f64(logits, labels, C, eps)
        assert abs(loss - float(g[c + ".eval_loss"])) <= 1e-6 * abs(loss)
        assert abs(miou - float(g[c + ".eval_miou"])) <= 1e-12 * abs(miou)
        assert np.array_equal(counts, g[c + ".eval_counts"])
        assert (labels == -1).any() and labels.max() == C - 1
    # a class that is in neither the predictions nor the labels
    cnt = g["k8.eval_counts"]
    assert cnt[1, 5] == 0 and cnt[2, 5] == 0 and (cnt[1, :8] + cnt[2, :8] > 0).sum() == 7
    # an image without a labelled pixel: loss 0, every predicted class has IoU 0
    none = g["k3_unlabelled.labels"]
    assert (none == -1).all()
    loss, miou, counts = eval_f64(g["k3.logits"], none, 3, eps)
    assert loss == 0.0 == float(g["k3_unlabelled.eval_loss"]) and miou == 0.0 == float(g["k3_unlabelled.eval_miou"])
    assert np.array_equal(counts, g["k3_unlabelled.eval_counts"])
    # the three-image epoch
    ms, ls, ps, es = [], [], [], []
    for i in range(3):
        loss, miou, _ = eval_f64(g[f"meters3.{i}.logits"], g[f"meters3.{i}.labels"], 3, eps)
        d = g[f"meters3.{i}.pred"].astype(np.float64) - g[f"meters3.{i}.truth"].astype(np.float64)
        mse = float((d * d).mean())
        assert abs(mse - float(g[f"meters3.{i}.mse"])) <= 1e-6 * mse and abs(-10 * np.log10(mse) - float(g[f"meters3.{i}.psnr"])) <= 1e-6 * abs(10 * np.log10(mse))
        ms.append(miou); ls.append(loss); ps.append(-10 * np.log10(mse)); es.append(mse)
    want = g["meters3.measure"]
    assert abs(np.mean(ms) - want[0]) <= 1e-12 * want[0]
    np.testing.assert_allclose([np.mean(ls), np.mean(ps), np.mean(es)], want[1:], rtol=1e-6)


def test_fixture_keeps_its_recorded_margins():
    """Recomputed here, not only read back: top-2 probability gap >= 1e-3; every 255 x that feeds an 8-bit value >= 1e-2 from an integer,
    exact zeros (a colour-table channel that is exactly 0) apart -- see tools/gen_golden_mask_output.py."""
    g = golden("mask_output")
    for c in CASES:
        K = int(g[c + ".shape"][2])
        if K > 1:
            ps = np.sort(g[c + ".probs"], axis=-1)
            assert (ps[:, -1] - ps[:, -2]).min() >= 1e-3 and float(g[c + ".margin_top2"]) >= 1e-3
        worst, zeros = np.inf, 0
        for x in [g[c + ".image"]] + [g[f"{c}.{m}.{r}.rgb"] for m, r in VARIANTS]:
            v = 255.0 * x.astype(np.float64)
            d = np.abs(v - np.rint(v))
            worst = min(worst, d[x != 0.0].min())
        for m, r in VARIANTS:
            x = g[f"{c}.{m}.{r}.rgb"]
            zeros += int((x == 0.0).sum())
            if m != "heatmap":
                assert not (x == 0.0).any(), "only a zero colour-table channel makes an exact zero"
        assert worst >= 1e-2 and float(g[c + ".margin_rgb8"]) >= 1e-2, (c, worst)
        assert zeros == int(g[c + ".rgb8_exact_zeros"])
