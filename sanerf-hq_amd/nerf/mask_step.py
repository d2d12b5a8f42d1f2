"""The mask-mode ("object field") training loss of nerf/trainer.py:401-505 as the reference's own script runs it
(scripts/train_obj_nerf.sh: --ray_pair_rgb_loss_weight 1 --ray_pair_rgb_num_sample 8 --mixed_sampling --num_local_sample 4
--local_sample_patch_size 8 --error_map), assembled from the HIP operators of `raymarching`:

    NLL over the first opt.num_rays rays           rm.mask_nll            trainer.py:419-428
    per-step error-map EMA                         rm.error_map_update    trainer.py:434-464
    ray-pair RGB loss over the local patches       rm.ray_pair_select + rm.ray_pair_rgb_loss    trainer.py:260-305, 480-499
    whole-map rebuild                              rm.mask_error          trainer.py:1406-1434 (build_error_map)

Nothing here reads a device value on the host, so a step built on it can be captured as a HIP graph (sanerf_hq_amd.graph).
`label_regularization` (trainer.py:307-334) reads opt.patch_size, which the reference's main.py never defines: it cannot be reached
from its command line and is not built.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import raymarching as rm


def mask_train_loss(outputs, data, opt, global_step, error_map=None, uniform=None):
    """(pred_masks, gt_mask, loss) of trainer.py:401-505 from a mask-mode render.

    outputs: `model.render(..., return_mask=1)`: 'instance_mask_logits' [N,K] and 'image' [N,3] for all N rays of the step (the first
      opt.num_rays drawn over the images, then -- with opt.mixed_sampling -- opt.num_local_sample patches of opt.local_sample_patch_size^2).
    data: what nerf.utils.collate_rays returns: 'masks' [N,1] labels, 'index', 'inds_coarse', 'error_maps' [N].
    error_map: the dataset's [images, cells] map; when given, the cells of the first num_rays rays get the EMA update in place.
    uniform: optional [G,P] uniform [0,1) tensor for the draw of the compared pixels (one torch.rand here otherwise).

    Differences from the reference, all on paths it cannot run: its `labeled.sum() > 0` host branch is a device-side select; its
    non-mixed call of the ray-pair loss omits an argument and raises TypeError -- here it runs as one group of all rays with
    incoherent = 0 (every pixel a candidate); pred_masks is the argmax of the logits (= of their softmax)."""
    logits = outputs["instance_mask_logits"]
    K = logits.shape[-1]
    lg = logits.reshape(-1, K)
    gt_mask = data["masks"].to(torch.long)
    gt_flat = gt_mask.reshape(-1)
    nr = int(opt.num_rays)
    eps = float(opt.epsilon)
    w = float(getattr(opt, "ray_pair_rgb_exp_weight", 10.0))
    if float(getattr(opt, "label_regularization_weight", 0) or 0) > 0:
        raise NotImplementedError("label_regularization reads opt.patch_size, which the reference's main.py never defines (trainer.py:307-334)")

    nll = rm.mask_nll(lg[:nr], gt_flat[:nr], eps)                                    # [nr, 1]
    loss = torch.where((gt_flat != -1).any(), nll.mean(), nll.new_zeros(()))         # trainer.py:427-432 without the host branch

    if error_map is not None:                                                        # trainer.py:434-464
        rm.error_map_update(error_map, data["index"], data["inds_coarse"].reshape(-1)[:nr], lg[:nr], gt_flat[:nr], w, eps, from_logits=True)

    if float(getattr(opt, "ray_pair_rgb_loss_weight", 0) or 0) > 0 and global_step > int(getattr(opt, "ray_pair_rgb_iter", -1)):
        image = outputs["image"].detach().reshape(-1, 3)
        if getattr(opt, "mixed_sampling", False):                                    # trainer.py:481-495
            G, P = int(opt.num_local_sample), int(opt.local_sample_patch_size) ** 2
            if data.get("error_maps") is None:
                raise RuntimeError("mask_train_loss: mixed sampling draws the compared pixels from data['error_maps'] (trainer.py:491), which is "
                                   "None: collate_rays returns it only when it is given the dataset's error_map")
            pair_logits, rgb = lg[nr:].reshape(G, P, K), image[nr:].reshape(G, P, 3)
            incoherent = data["error_maps"].reshape(-1)[nr:].reshape(G, P)
        else:                                                                        # trainer.py:496-499 (raises in the reference)
            G, P = 1, lg.shape[0]
            pair_logits, rgb = lg.reshape(G, P, K), image.reshape(G, P, 3)
            incoherent = torch.zeros(G, P, device=lg.device, dtype=torch.float32)
        idx = rm.ray_pair_select(incoherent, int(opt.ray_pair_rgb_num_sample), uniform)
        pair = rm.ray_pair_rgb_loss(rgb, pair_logits, idx, float(opt.ray_pair_rgb_threshold), w, eps,
                                    use_pred_logistics=bool(getattr(opt, "ray_pair_rgb_use_pred_logistics", False)), from_logits=True)
        loss = loss + pair * float(opt.ray_pair_rgb_loss_weight)

    pred_masks = logits.detach().argmax(dim=-1)
    return pred_masks, gt_mask, loss


def build_error_map(rendered_probs, gt_masks, opt):
    """The whole-map rebuild of Trainer.update_error_map (trainer.py:1414-1434): rendered_probs [M, S, S, K] or [M, S*S, K], the
    softmax probabilities rendered at the map's resolution S = opt.error_map_size for each of the M training views; gt_masks [M,H,W] or
    [M,H,W,C] (channel 0) -> error map [M, S*S].  Down-scaling and rounding of the labels stay torch (F.interpolate); the measure is
    rm.mask_error."""
    M, K = rendered_probs.shape[0], rendered_probs.shape[-1]
    S = int(opt.error_map_size)
    gt = gt_masks.to(torch.float32)
    if gt.dim() == 4:
        gt = gt[..., 0]
    small = F.interpolate(gt[:, None], (S, S), mode="bilinear").round().to(torch.int64)
    probs = rendered_probs.detach().reshape(M, -1, K)
    labels = small.reshape(M, -1).to(probs.device)
    if probs.shape[1] != labels.shape[1]:
        raise RuntimeError(f"build_error_map: {probs.shape[1]} rendered cells for a {S} x {S} map")
    return rm.mask_error(probs, labels, float(opt.ray_pair_rgb_exp_weight), float(opt.epsilon))
