#!/usr/bin/env python3
"""Generate tests/golden/rgb_step.npz by running the REFERENCE's own code on the CPU:

  * `Trainer.train_step` (nerf/trainer.py:336-399, its RGB branch) and `Trainer.eval_step` (trainer.py:570-597), called unbound with a
    SimpleNamespace as `self`.  The model is a fake whose `render` returns image0 + (1 - weights_sum)[:, None] * bg_color (renderer.py:353),
    weights_sum, proposal_loss (only when it is asked to update the proposals, as the real renderer does), distort_loss and num_points,
    built from leaf tensors made here, so that the reference's autograd gives its gradients with respect to image0 and weights_sum;
  * torch.rand is wrapped to RECORD the background the reference drew (not replaced).

    python tools/gen_golden_rgb_step.py --reference <checkout of the reference>

Third-party modules the reference imports at module level and that are not installed are replaced by empty stubs, as
tools/gen_golden_mask_losses.py does (none is used on these paths).  The fixture holds arrays only.  The entropy term's gradient jumps at
the two clamp bounds, so the generator asserts, and records as `margin`, that no weights_sum lies within 1e-7 of either."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_mask_losses import import_trainer  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LO, HI = np.float32(1e-5), np.float32(1 - 1e-5)          # what clamp(1e-5, 1 - 1e-5) compares a float tensor with
H, W = 8, 12
N = H * W


def make_inputs(seed, channels):
    rng = np.random.default_rng(seed)
    image0 = rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32)
    ws = rng.uniform(1e-3, 1.0 - 1e-3, N).astype(np.float32)
    # below the clamp range (0 included), above it (1 and slightly above 1 included), just inside either bound, the middle
    special = np.array([0.0, 5e-6, 9e-6, 1.0, 1.0 + 1e-6, 1.0 - 5e-6, 1.0 - 2e-6, 1.2e-5, 1.0 - 1.2e-5, 0.5, 0.5 + 1e-4, 3e-4], dtype=np.float32)
    ws[:special.size] = special
    ws = ws[rng.permutation(N)]
    images = rng.uniform(0.0, 1.0, (N, channels)).astype(np.float32)
    if channels == 4:
        images[:4, 3] = (0.0, 1.0, 0.0, 1.0)
    margin = float(min(np.abs(ws.astype(np.float64) - float(LO)).min(), np.abs(ws.astype(np.float64) - float(HI)).min()))
    assert margin > 1e-7, margin
    return image0, ws, images, margin


class FakeModel:
    def __init__(self, image0, ws, prop, dist, num_points, training):
        self.image0, self.ws, self.prop, self.dist, self.num_points, self.training = image0, ws, prop, dist, num_points, training
        self.calls = []

    def render(self, rays_o, rays_d, staged=False, bg_color=None, update_proposal=True, **kw):
        self.calls.append(dict(staged=staged, bg_color=bg_color, update_proposal=update_proposal, **kw))
        out = {"image": self.image0 + (1 - self.ws).unsqueeze(-1) * bg_color, "weights_sum": self.ws, "depth": torch.zeros(N)}
        if self.training:
            out["num_points"] = self.num_points
            if update_proposal:
                out["proposal_loss"] = self.prop
            out["distort_loss"] = self.dist
        return out


def run_train(trainer, seed, channels, background, lambda_entropy, global_step, lambda_proposal, lambda_distort):
    image0, ws, images, margin = make_inputs(seed, channels)
    rng = np.random.default_rng(seed + 1000)
    prop_v, dist_v = np.float32(rng.uniform(0.01, 0.1)), np.float32(rng.uniform(0.001, 0.01))
    t_image0 = torch.from_numpy(image0).requires_grad_(True)
    t_ws = torch.from_numpy(ws).requires_grad_(True)
    t_prop = torch.tensor(prop_v, requires_grad=True)
    t_dist = torch.tensor(dist_v, requires_grad=True)
    num_points_out = N * (17 + 5 * (seed % 7))                       # what the render says it evaluated: differs from case to case
    model = FakeModel(t_image0, t_ws, t_prop, t_dist, num_points_out, True)
    opt = types.SimpleNamespace(with_sam=False, with_mask=False, cache_size=0, cache_interval=4, background=background,
                                lambda_proposal=lambda_proposal, lambda_distort=lambda_distort, lambda_entropy=lambda_entropy,
                                adaptive_num_rays=True, num_points=2 ** 12, num_rays=N)
    me = types.SimpleNamespace(opt=opt, global_step=global_step, device=torch.device("cpu"), model=model,
                               criterion=torch.nn.MSELoss(reduction="none"), cache=None)
    data = dict(rays_o=torch.zeros(N, 3), rays_d=torch.zeros(N, 3), index=[0], H=H, W=W, images=torch.from_numpy(images))
    recorded = []
    real = torch.rand

    def recording(*a, **k):
        out = real(*a, **k)
        recorded.append(out.clone())
        return out

    torch.manual_seed(seed)
    torch.rand = recording
    try:
        pred_rgb, gt_rgb, loss = trainer.Trainer.train_step(me, data)
    finally:
        torch.rand = real
    loss.backward()
    if background == "random":
        assert len(recorded) == 1 and tuple(recorded[0].shape) == (N, 3)
        bg = recorded[0].numpy().astype(np.float32)
        assert torch.equal(model.calls[0]["bg_color"], recorded[0])
    else:
        assert not recorded and model.calls[0]["bg_color"] == 1
        bg = np.float32(1.0)
    call = model.calls[0]
    assert call["perturb"] is True and call["staged"] is False
    return dict(image0=image0, weights_sum=ws, images=images, bg=bg, proposal_loss=prop_v, distort_loss=dist_v,
                lambda_proposal=np.float32(lambda_proposal), lambda_distort=np.float32(lambda_distort), lambda_entropy=np.float32(lambda_entropy),
                global_step=np.int64(global_step), update_proposal=np.bool_(call["update_proposal"]),
                loss=np.float32(loss.item()), grad_image0=t_image0.grad.numpy().copy(), grad_weights_sum=t_ws.grad.numpy().copy(),
                grad_proposal_loss=np.float32(0.0 if t_prop.grad is None else t_prop.grad.item()),
                grad_distort_loss=np.float32(0.0 if t_dist.grad is None else t_dist.grad.item()),
                pred_rgb=pred_rgb.detach().numpy().copy(), gt_rgb=gt_rgb.detach().numpy().copy(),
                num_rays_before=np.int64(N), num_points=np.int64(opt.num_points), num_points_out=np.int64(num_points_out),
                num_rays_after=np.int64(opt.num_rays), margin=np.float64(margin))


def run_eval(trainer, seed, channels):
    image0, ws, images, margin = make_inputs(seed, channels)
    model = FakeModel(torch.from_numpy(image0), torch.from_numpy(ws), None, None, 0, False)
    opt = types.SimpleNamespace(with_sam=False, with_mask=False)
    me = types.SimpleNamespace(opt=opt, device=torch.device("cpu"), model=model, criterion=torch.nn.MSELoss(reduction="none"))
    data = dict(rays_o=torch.zeros(N, 3), rays_d=torch.zeros(N, 3), index=[0], H=H, W=W, images=torch.from_numpy(images).reshape(H, W, channels))
    with torch.no_grad():
        pred_rgb, pred_depth, _, gt_rgb, loss = trainer.Trainer.eval_step(me, data)
    assert model.calls[0]["bg_color"] == 1 and model.calls[0]["staged"] is True
    return dict(image0=image0, weights_sum=ws, images=images, bg=np.float32(1.0), loss=np.float32(loss.item()),
                pred_rgb=pred_rgb.numpy().copy(), gt_rgb=gt_rgb.numpy().copy(), H=np.int64(H), W=np.int64(W), margin=np.float64(margin))


# (name, channels, background, lambda_entropy, global_step, lambda_proposal, lambda_distort)
TRAIN_CASES = (("rgba_random", 4, "random", 0.0, 10, 1.0, 0.002),
               ("rgba_random_entropy", 4, "random", 1e-3, 3000, 1.0, 0.002),
               ("rgba_white", 4, "white", 0.0, 3001, 1.0, 0.002),          # no proposal update at this step: no proposal_loss in outputs
               ("rgba_white_entropy", 4, "white", 1e-2, 3005, 1.0, 0.0),   # distort_loss in outputs, lambda_distort = 0
               ("rgb_random", 3, "random", 0.0, 3002, 0.5, 0.002),
               ("rgb_random_entropy", 3, "random", 1e-2, 0, 1.0, 0.002),
               ("rgb_white", 3, "white", 0.0, 5, 0.0, 0.0),
               ("rgb_white_entropy", 3, "white", 1e-3, 2999, 1.0, 0.01))
EVAL_CASES = (("eval_rgba", 4), ("eval_rgb", 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(GOLD, "rgb_step.npz"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    trainer = import_trainer(args.reference)
    arrays = dict(train_cases=np.array([c[0] for c in TRAIN_CASES]), eval_cases=np.array([c[0] for c in EVAL_CASES]),
                  clamp_lo=LO, clamp_hi=HI)
    for n, (name, ch, background, lam, gs, lp, ld) in enumerate(TRAIN_CASES):
        out = run_train(trainer, 11 + n, ch, background, lam, gs, lp, ld)
        print(f"{name}: loss {out['loss']:.6f}, update_proposal {bool(out['update_proposal'])}, num_rays {N} -> {int(out['num_rays_after'])}, margin {float(out['margin']):.2e}")
        arrays.update({f"{name}.{k}": v for k, v in out.items()})
    for n, (name, ch) in enumerate(EVAL_CASES):
        out = run_eval(trainer, 51 + n, ch)
        print(f"{name}: loss {out['loss']:.6f}")
        arrays.update({f"{name}.{k}": v for k, v in out.items()})
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
