"""CPU: the object-field loss entry points (ray-pair RGB loss, error measure, error-map EMA) validate their arguments before any launch,
and tests/golden/mask_losses.npz (tools/gen_golden_mask_losses.py: the reference's own Trainer.ray_pair_rgb_loss and error-map lines on the
CPU) agrees with the closed form in float64 and keeps away from the loss's two discontinuities."""
import ctypes

import numpy as np

from helpers import golden

CASES = ("script_k2", "script_k3", "defaults", "odd_p")


def pair_loss_f64(rgb, probs, idx, thr, w, eps, use_pred):
    """nerf/trainer.py:276-303 for given sample indices, float64 (steps 2-5 of the closed form)."""
    rgb, probs = rgb.astype(np.float64), probs.astype(np.float64)
    G, P, K = probs.shape
    pairs = []
    for g in range(G):
        for s in idx[g]:
            if s < 0:
                continue
            q = probs[g, s]
            if not use_pred:
                q = np.eye(K)[np.argmax(q)]
            sim = np.linalg.norm(rgb[g] - rgb[g, s], axis=-1) < thr
            cos = probs[g] @ q / (np.maximum(np.linalg.norm(probs[g], axis=-1), 1e-8) * max(np.linalg.norm(q), 1e-8))
            pairs.append((sim * np.exp(-w * cos - eps)).sum() / sim.sum())
    return float(np.mean(pairs))


def test_mask_loss_entry_points_validate_their_arguments():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    d = ctypes.c_void_p(16)
    # ray_pair_select
    assert l.sn_rm_ray_pair_select(None, d, 4, 64, 8, d, None) == -1 and b"NULL" in l.sn_last_error()
    assert l.sn_rm_ray_pair_select(d, d, 4, 64, 65, d, None) == -2 and b"64 samples" in l.sn_last_error()
    assert l.sn_rm_ray_pair_select(d, d, 1 << 16, 1 << 15, 8, d, None) == -2 and b"2^31" in l.sn_last_error()
    assert l.sn_rm_ray_pair_select(None, None, 0, 64, 8, None, None) == 0
    # ray_pair_rgb_loss(rgb, masks, from_logits, idx, G, P, S, K, thr, w, eps, use_pred, scale, scale_dev, loss_per_pair, pair_count, grad, stream)
    assert l.sn_rm_ray_pair_rgb_loss(None, d, 1, d, 4, 64, 8, 2, 0.1, 10.0, 1e-6, 0, 1.0, None, d, None, d, None) == -1 and b"NULL" in l.sn_last_error()
    assert l.sn_rm_ray_pair_rgb_loss(d, d, 1, d, 4, 64, 8, 2, 0.1, 10.0, 1e-6, 0, 1.0, None, None, None, None, None) == -1 and b"neither" in l.sn_last_error()
    assert l.sn_rm_ray_pair_rgb_loss(d, d, 1, d, 4, 64, 8, 33, 0.1, 10.0, 1e-6, 0, 1.0, None, d, None, d, None) == -2 and b"K=33" in l.sn_last_error()
    assert l.sn_rm_ray_pair_rgb_loss(d, d, 1, d, 4, 64, 65, 2, 0.1, 10.0, 1e-6, 0, 1.0, None, d, None, d, None) == -2 and b"S=65" in l.sn_last_error()
    assert l.sn_rm_ray_pair_rgb_loss(d, d, 1, d, 4, 64, 8, 2, 0.0, 10.0, 1e-6, 0, 1.0, None, d, None, d, None) == -1 and b"threshold" in l.sn_last_error()
    assert l.sn_rm_ray_pair_rgb_loss(d, d, 1, d, 4, 64, 8, 2, -1.0, 10.0, 1e-6, 0, 1.0, None, d, None, d, None) == -1
    assert l.sn_rm_ray_pair_rgb_loss(d, d, 1, d, 1 << 16, 1 << 15, 8, 2, 0.1, 10.0, 1e-6, 0, 1.0, None, d, None, d, None) == -2 and b"2^31" in l.sn_last_error()
    assert l.sn_rm_ray_pair_rgb_loss(None, None, 1, None, 0, 64, 8, 2, 0.1, 10.0, 1e-6, 0, 1.0, None, None, None, None, None) == 0
    # mask_error / error_map_update
    assert l.sn_rm_mask_error(d, 1, None, 4, 2, 10.0, 1e-6, d, None) == -1 and b"NULL" in l.sn_last_error()
    assert l.sn_rm_mask_error(d, 1, d, 4, 0, 10.0, 1e-6, d, None) == -1
    assert l.sn_rm_mask_error(None, 1, None, 0, 2, 10.0, 1e-6, None, None) == 0
    assert l.sn_rm_error_map_update(d, 1, d, d, 1, d, 4, 2, 10.0, 1e-6, 5, 256, d, None, None, None) == -1 and b"NULL" in l.sn_last_error()
    assert l.sn_rm_error_map_update(d, 1, d, d, 3, d, 4, 2, 10.0, 1e-6, 5, 256, d, d, None, None) == -1 and b"1 or N" in l.sn_last_error()
    assert l.sn_rm_error_map_update(d, 1, d, d, 1, d, 4, 2, 10.0, 1e-6, 5, 0, d, d, None, None) == -1 and b"empty" in l.sn_last_error()
    assert l.sn_rm_error_map_update(None, 1, None, None, 1, None, 0, 2, 10.0, 1e-6, 5, 256, None, None, None, None) == 0
    assert l.sn_abi_version() == 12


def test_python_mask_loss_operators_refuse_cpu_tensors():
    import pytest
    import torch
    from sanerf_hq_amd import raymarching as rm
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.ray_pair_select(torch.zeros(2, 8), 2, torch.rand(2, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.ray_pair_rgb_loss(torch.rand(2, 8, 3), torch.rand(2, 8, 2), torch.zeros(2, 2, dtype=torch.long), 0.1, 10.0, 1e-6)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.mask_error(torch.rand(8, 2), torch.zeros(8, dtype=torch.long), 10.0, 1e-6)
    with pytest.raises(RuntimeError, match="CUDA"):
        rm.error_map_update(torch.zeros(2, 16), torch.zeros(1, dtype=torch.long), torch.zeros(8, dtype=torch.long), torch.rand(8, 2),
                            torch.zeros(8, dtype=torch.long), 10.0, 1e-6)


def test_fixture_agrees_with_the_closed_form_in_float64_and_keeps_its_margins():
    g = golden("mask_losses")
    assert list(g["cases"]) == list(CASES)
    thr, w, eps = float(g["thr"]), float(g["exp_weight"]), float(g["epsilon"])
    shapes = {}
    for c in CASES:
        rgb, probs, inc, idx = g[c + ".rgb"], g[c + ".probs"], g[c + ".incoherent"], g[c + ".sample_index"]
        G, P, K = probs.shape
        shapes[c] = (G, P, idx.shape[1], K)
        for name, use_pred in (("onehot", False), ("pred", True)):
            want = float(g[f"{c}.loss_{name}"])
            got = pair_loss_f64(rgb, probs, idx, thr, w, eps, use_pred)
            assert abs(got - want) <= 1e-6 * abs(want), (c, name, got, want)
            assert g[f"{c}.grad_logits_{name}"].shape == probs.shape and np.abs(g[f"{c}.grad_logits_{name}"]).max() > 0
        # the two discontinuities: recomputed here, not only read back
        sel = np.take_along_axis(rgb, idx[:, :, None], axis=1).astype(np.float64)
        dist = np.linalg.norm(rgb[:, None].astype(np.float64) - sel[:, :, None], axis=-1)
        assert np.abs(dist - thr).min() >= 1e-4 and float(g[c + ".margin_thr"]) >= 1e-4
        top = np.sort(np.take_along_axis(probs, idx[:, :, None], axis=1), axis=-1)
        assert (top[..., -1] - top[..., -2]).min() >= 1e-3 and float(g[c + ".margin_top2"]) >= 1e-3
        # the recorded draw: distinct candidates
        cand = (1.0 - inc) > 0.8
        cand[cand.sum(-1) == 0] = True
        assert np.take_along_axis(cand, idx, axis=1).all()
        assert all(len(set(row.tolist())) == idx.shape[1] for row in idx)
    assert shapes == {"script_k2": (4, 64, 8, 2), "script_k3": (4, 64, 8, 3), "defaults": (2, 256, 1, 3), "odd_p": (3, 100, 5, 4)}
    assert any(((1.0 - g[c + ".incoherent"]) > 0.8).sum(-1).min() == 0 for c in CASES), "no group exercises the all-incoherent fallback"
    # EMA: distinct targets; the stored map equals the closed form
    index, inds = g["ema_index"], g["ema_inds"]
    assert len(set(zip(index.tolist(), inds.tolist()))) == len(index)
    p = g["ema_probs"].astype(np.float64)
    err = np.exp(-w * p[np.arange(len(p)), g["ema_labels"]] / np.maximum(np.linalg.norm(p, axis=-1), 1e-8) - eps)
    np.testing.assert_allclose(g["ema_error"], err, rtol=1e-6)
    want = g["ema_map_before"].astype(np.float64).copy()
    want[index, inds] = 0.1 * want[index, inds] + 0.9 * err
    np.testing.assert_allclose(g["ema_map_after"], want, rtol=1e-6)
    untouched = np.ones_like(want, dtype=bool)
    untouched[index, inds] = False
    assert untouched.any() and np.array_equal(g["ema_map_after"][untouched], g["ema_map_before"][untouched])
    # rebuild
    p = g["rebuild_probs"].astype(np.float64).reshape(g["rebuild_labels"].shape + (-1,))
    lab = g["rebuild_labels"]
    py = np.take_along_axis(p, lab[..., None], axis=-1)[..., 0]
    np.testing.assert_allclose(g["rebuild_error_map"], np.exp(-w * py / np.linalg.norm(p, axis=-1) - eps), rtol=1e-6)
