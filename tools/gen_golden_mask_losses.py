#!/usr/bin/env python3
"""Generate tests/golden/mask_losses.npz by running the REFERENCE's own code on the CPU:

  * `Trainer.ray_pair_rgb_loss` (nerf/trainer.py:260-305), called unbound with a SimpleNamespace as `self`; torch.multinomial is wrapped to
    RECORD the indices it returned (not replaced), so that a kernel can be given the same draw;
  * the per-step error-map EMA (trainer.py:457-464) and the whole-map rebuild (trainer.py:1415-1432): these lines sit inside larger methods,
    so they are read from the reference's source file at run time and executed as they are, on tensors made here.

    python tools/gen_golden_mask_losses.py --reference <checkout of the reference>

Third-party modules the reference imports at module level and that are not installed are replaced by empty stubs (none is used on these
paths).  The fixture holds arrays only.  The loss has two discontinuities (the colour threshold, the argmax of the sampled pixel), so the
generator asserts, and records, that no input sits near either: margins `margin_thr` >= 1e-4 and `margin_top2` >= 1e-3 per case, and that
the EMA case has no duplicate (index, inds) target."""
import argparse
import importlib
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

THR, W, EPS = 0.1, 10.0, 1e-6


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_trainer(ref):
    sys.path.insert(0, ref)
    for _ in range(32):
        try:
            return importlib.import_module("nerf.trainer")
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Stub(e.name)
            for k in [k for k in sys.modules if k.startswith("nerf")]:
                del sys.modules[k]
    raise RuntimeError("could not import the reference's nerf.trainer")


def make_case(seed, G, P, S, K, all_incoherent_group=None):
    rng = np.random.default_rng(seed)
    palette = rng.uniform(0.1, 0.9, (4, 3))
    which = rng.integers(0, 4, (G, P))
    rgb = (palette[which] + rng.uniform(-0.02, 0.02, (G, P, 3)) / np.sqrt(3.0)).astype(np.float32)
    logits = (rng.standard_normal((G, P, K)) * 2.0).astype(np.float32)
    inc = rng.uniform(0.0, 0.6, (G, P)).astype(np.float32)          # about two thirds of the pixels are candidates
    if all_incoherent_group is not None:
        inc[all_incoherent_group] = 1.0
    return rgb, logits, inc


def run_case(trainer, seed, G, P, S, K, all_incoherent_group=None):
    rgb, logits, inc = make_case(seed, G, P, S, K, all_incoherent_group)
    recorded = []
    real = torch.multinomial

    def recording(*a, **k):
        out = real(*a, **k)
        recorded.append(out.clone())
        return out

    out = {}
    for name, use_pred in (("onehot", False), ("pred", True)):
        me = types.SimpleNamespace(opt=types.SimpleNamespace(ray_pair_rgb_num_sample=S, ray_pair_rgb_threshold=THR, ray_pair_rgb_exp_weight=W, epsilon=EPS))
        lg = torch.from_numpy(logits).requires_grad_(True)
        probs = torch.softmax(lg, dim=-1)
        probs.retain_grad()
        c = torch.from_numpy(rgb).requires_grad_(True)
        gt = torch.zeros(G, P, 1, dtype=torch.long)
        torch.manual_seed(seed)                                      # the same draw for both settings
        torch.multinomial = recording
        try:
            loss = trainer.Trainer.ray_pair_rgb_loss(me, c, probs, gt, torch.from_numpy(inc)[..., None], use_pred_logistics=use_pred)
        finally:
            torch.multinomial = real
        loss.backward()
        assert c.grad is None, "the reference sends no gradient to rgb"
        out["loss_" + name] = np.float32(loss.item())
        out["grad_logits_" + name] = lg.grad.numpy().copy()
        out["grad_probs_" + name] = probs.grad.numpy().copy()
        out["probs"] = probs.detach().numpy().copy()
    assert len(recorded) == 2 and torch.equal(recorded[0], recorded[1])
    idx = recorded[0].numpy().astype(np.int64)
    # margins
    sel = np.take_along_axis(rgb, idx[:, :, None], axis=1)                                   # [G,S,3]
    dist = np.linalg.norm(rgb[:, None].astype(np.float64) - sel[:, :, None].astype(np.float64), axis=-1)
    margin_thr = float(np.abs(dist - THR).min())
    ps = np.sort(np.take_along_axis(out["probs"], idx[:, :, None], axis=1), axis=-1)
    margin_top2 = float((ps[..., -1] - ps[..., -2]).min())
    cand = (1.0 - inc) > 0.8
    cand[cand.sum(-1) == 0] = True
    assert np.take_along_axis(cand, idx, axis=1).all(), "a recorded index is not a candidate"
    out.update(rgb=rgb, logits=logits, incoherent=inc, sample_index=idx, margin_thr=np.float64(margin_thr), margin_top2=np.float64(margin_top2))
    return out, margin_thr, margin_top2


def source_lines(ref, first, last, must_contain):
    src = open(os.path.join(ref, "nerf", "trainer.py")).read().splitlines()
    text = textwrap.dedent("\n".join(src[first - 1:last]))
    assert must_contain in text, f"trainer.py:{first}-{last} is not the expected block"
    return text


def ema_case(ref, seed, N=512, K=3, M=5, cells=256):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((N, K)) * 2.0).astype(np.float32)
    labels = rng.integers(0, K, N).astype(np.int64)
    flat = rng.permutation(M * cells)[:N]                            # distinct (index, inds) targets
    index, inds = (flat // cells).astype(np.int64), (flat % cells).astype(np.int64)
    assert len(set(zip(index.tolist(), inds.tolist()))) == N
    before = rng.uniform(0.0, 1.0, (M, cells)).astype(np.float32)
    probs = torch.softmax(torch.from_numpy(logits), dim=-1)
    me = types.SimpleNamespace(opt=types.SimpleNamespace(ray_pair_rgb_exp_weight=W, epsilon=EPS, num_rays=N), error_map=torch.from_numpy(before.copy()))
    ns = dict(torch=torch, F=F, self=me, index=torch.from_numpy(index), inds=torch.from_numpy(inds), global_inst_masks=probs,
              global_pred_masks_flattened=probs.clamp(min=EPS, max=1 - EPS), global_gt_masks_flattened=torch.from_numpy(labels))
    exec(source_lines(ref, 457, 464, "ema_error"), ns)
    return dict(ema_logits=logits, ema_probs=probs.numpy().copy(), ema_labels=labels, ema_index=index, ema_inds=inds, ema_map_before=before,
                ema_map_after=me.error_map.numpy().copy(), ema_error=ns["error"].numpy().copy())


def rebuild_case(ref, seed, M=2, H=32, S=8, K=3):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, K, (M, H // 4, H // 4)).repeat(4, axis=1).repeat(4, axis=2)[..., None].astype(np.int64)      # blocky label images
    logits = (rng.standard_normal((M, S, S, K)) * 2.0).astype(np.float32)
    probs = torch.softmax(torch.from_numpy(logits), dim=-1)
    me = types.SimpleNamespace(opt=types.SimpleNamespace(ray_pair_rgb_exp_weight=W, epsilon=EPS, error_map_size=S))
    loader = types.SimpleNamespace(_data=types.SimpleNamespace(masks=torch.from_numpy(gt)))
    ns = dict(torch=torch, F=F, self=me, loader=loader, rendered_masks_softmax=probs)
    exec(source_lines(ref, 1415, 1432, "F.interpolate"), ns)
    return dict(rebuild_probs=probs.numpy().copy(), rebuild_gt_masks=gt, rebuild_labels=ns["gt_masks_flatten"].numpy().copy(),
                rebuild_error_map=ns["error_map"].numpy().copy(), rebuild_size=np.int64(S))


CASES = (("script_k2", dict(G=4, P=64, S=8, K=2, all_incoherent_group=2)),        # scripts/train_obj_nerf.sh
         ("script_k3", dict(G=4, P=64, S=8, K=3, all_incoherent_group=0)),
         ("defaults", dict(G=2, P=256, S=1, K=3)),                               # main.py's defaults
         ("odd_p", dict(G=3, P=100, S=5, K=4)))                                  # P not a multiple of 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(GOLD, "mask_losses.npz"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    trainer = import_trainer(args.reference)
    arrays = dict(thr=np.float32(THR), exp_weight=np.float32(W), epsilon=np.float32(EPS), cases=np.array([c for c, _ in CASES]))
    for n, (name, kw) in enumerate(CASES):
        for seed in range(100 * n + 1, 100 * n + 50):                # the first seed whose inputs keep away from both discontinuities
            out, m_thr, m_top2 = run_case(trainer, seed, **kw)
            if m_thr >= 1e-4 and m_top2 >= 1e-3:
                break
        assert m_thr >= 1e-4 and m_top2 >= 1e-3, (name, m_thr, m_top2)
        print(f"{name}: seed {seed}, loss {out['loss_onehot']:.6f} / {out['loss_pred']:.6f}, margins thr {m_thr:.2e} top2 {m_top2:.2e}")
        arrays.update({f"{name}.{k}": v for k, v in out.items()})
    arrays.update(ema_case(args.reference, 7))
    arrays.update(rebuild_case(args.reference, 11))
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
