"""The RGB training step of nerf/trainer.py:355-399 (the first thing scripts/train_rgb_nerf.sh runs) and the RGB branch of eval_step
(trainer.py:586-597), with the loss tail as one HIP launch:

    background of the step           step_background       trainer.py:356-360
    proposal-update schedule         update_proposal_at    trainer.py:372-373
    loss tail of train_step          rm.rgb_loss           trainer.py:364-392 (RGBA blend / MSELoss / mean / extras / entropy)
    adaptive num_rays                adapt_num_rays        trainer.py:395-397 (host arithmetic on host numbers)
    loss tail of eval_step           rm.rgb_loss           trainer.py:586-595

With `--background random` the reference renders over an [N,3] tensor, which the fused training route (NeRFRenderer._run_autograd_unit)
does not take.  The background term is linear -- sigmoid(head) + (1 - weights_sum) bg = [image over bg = 0] + (1 - weights_sum) bg -- so
rgb_train_step renders over 0 and the tail adds the term and its gradient into weights_sum: the step stays on the fused route.
Nothing here reads a device value on the host, so a step built on it can be captured as a HIP graph (sanerf_hq_amd.graph).
"""
from __future__ import annotations

import torch

from .. import raymarching as rm


def step_background(opt, N, device, uniform=None):
    """trainer.py:356-360: an [N,3] uniform tensor with opt.background == 'random', else 1 (white / last_sample).  uniform: the caller's
    [N,3] buffer, returned as it is -- a captured step refills it (uniform_()) before every replay; without it, one torch.rand."""
    if opt.background == "random":
        if uniform is not None:
            if tuple(uniform.shape) != (N, 3):
                raise RuntimeError(f"step_background: uniform must be [{N},3], got {tuple(uniform.shape)}")
            return uniform
        return torch.rand(N, 3, device=device)
    return 1


def update_proposal_at(opt, global_step) -> bool:
    """trainer.py:372-373: the proposal networks train on every step up to 3000, on every fifth after."""
    return bool((not opt.with_sam) and (global_step <= 3000 or global_step % 5 == 0))


def rgb_train_loss(outputs, data, opt, bg_color=1, image_has_bg: bool = True):
    """(pred_rgb, gt_rgb, loss) of trainer.py:364-392 from an RGB-mode render, one launch.

    outputs: `model.render(...)`: 'image' [N,3], 'weights_sum' [N], and 'proposal_loss' / 'distort_loss' where the render made them;
      they enter the loss under the reference's conditions ('proposal_loss' in outputs and opt.lambda_proposal > 0, the same for distort).
    data: 'images' [N,3] or [N,4]; an RGBA truth is blended over bg_color.
    bg_color: the background of the step (step_background).  image_has_bg=False: outputs['image'] was rendered over 0 and the tail adds
      (1 - weights_sum) * bg_color.
    pred_rgb and gt_rgb carry no gradient (the reference's train loop only feeds them to the meters)."""
    extras = []
    if "proposal_loss" in outputs and opt.lambda_proposal > 0:
        extras.append((outputs["proposal_loss"], float(opt.lambda_proposal)))
    if "distort_loss" in outputs and opt.lambda_distort > 0:
        extras.append((outputs["distort_loss"], float(opt.lambda_distort)))
    lam = float(getattr(opt, "lambda_entropy", 0) or 0)
    loss, pred_rgb, gt_rgb = rm.rgb_loss(outputs["image"], outputs["weights_sum"], data["images"], bg=bg_color, image_has_bg=image_has_bg,
                                         lambda_entropy=lam if lam > 0 else 0.0, extras=extras, want_pred=True)
    return pred_rgb, gt_rgb, loss


def adapt_num_rays(opt, outputs) -> int:
    """trainer.py:395-397: with opt.adaptive_num_rays, opt.num_rays follows the number of points the render evaluated (a host number)."""
    if getattr(opt, "adaptive_num_rays", False):
        opt.num_rays = int(round((opt.num_points / outputs["num_points"]) * opt.num_rays))
    return opt.num_rays


def rgb_train_step(model, data, opt, global_step, uniform=None):
    """(pred_rgb, gt_rgb, loss) of trainer.py:355-399: background, render, loss tail, adaptive num_rays.

    A tensor background ('random') is rendered over 0 and added by the tail (image_has_bg=False): the fused training route serves it.
    A scalar background is rendered as before and the tail is told so.  uniform: see step_background."""
    rays_o, rays_d = data["rays_o"], data["rays_d"]
    cam_near_far = data["cam_near_far"] if "cam_near_far" in data else None
    N = rays_o.shape[0]
    bg_color = step_background(opt, N, rays_o.device, uniform)
    per_ray = torch.is_tensor(bg_color)
    outputs = model.render(rays_o, rays_d, staged=False, index=data.get("index"), bg_color=0 if per_ray else bg_color, perturb=True,
                           cam_near_far=cam_near_far, update_proposal=update_proposal_at(opt, global_step), return_feats=0)
    pred_rgb, gt_rgb, loss = rgb_train_loss(outputs, data, opt, bg_color, image_has_bg=not per_ray)
    adapt_num_rays(opt, outputs)
    return pred_rgb, gt_rgb, loss


def rgb_eval_loss(outputs, data):
    """(pred_rgb, gt_rgb, loss) of eval_step's RGB branch (trainer.py:586-597): bg = 1, no gradients; the images are [H,W,3] where data
    carries 'H' and 'W'."""
    with torch.no_grad():
        loss, pred_rgb, gt_rgb = rm.rgb_loss(outputs["image"], outputs["weights_sum"], data["images"], bg=1.0, image_has_bg=True)
    if "H" in data and "W" in data:
        H, W = int(data["H"]), int(data["W"])
        pred_rgb, gt_rgb = pred_rgb.reshape(H, W, 3), gt_rgb.reshape(H, W, 3)
    return pred_rgb, gt_rgb, loss
