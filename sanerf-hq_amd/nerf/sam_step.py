"""The SAM-feature distillation step of nerf/trainer.py:507-555 (what scripts/train_sam_nerf.sh runs by default) after its render,
and the host logic around it:

    loss tail of train_step          rm.feature_distill_loss    trainer.py:533-555 (reshape / permute / F.interpolate / MSELoss / mean)
    loss tail of eval_step           rm.feature_distill_loss    trainer.py:657-670
    the cache of encoded views       Cache, use_cache           nerf/utils.py:353-370, trainer.py:339-342

The SAM image encoder that makes `gt_samvit` (trainer.py:512-530) is outside the hot path: the caller encodes the
high-resolution render -- or takes the cached features -- and hands the map in through data['gt_samvit'].  Nothing here reads a device
value on the host, so a step built on it can be captured as a HIP graph (sanerf_hq_amd.graph).
"""
from __future__ import annotations

import random

from .. import raymarching as rm


class Cache:
    """nerf/utils.py:353-370: a ring of the last `size` data dictionaries (each carrying its 'gt_samvit'); host logic only."""

    def __init__(self, size=100):
        self.size = size
        self.data = {}
        self.key = 0

    def full(self):
        return len(self.data) == self.size

    def insert(self, x):
        self.data[self.key] = x
        self.key = (self.key + 1) % self.size

    def get(self, key=None):
        if key is None:
            key = random.randint(0, len(self.data) - 1)
        return self.data[key]


def use_cache(opt, cache, global_step) -> bool:
    """trainer.py:339-342: take a cached view instead of a novel pose on every step that is no multiple of opt.cache_interval, once
    the cache is full."""
    return bool(opt.with_sam and opt.cache_size > 0 and cache.full() and global_step % opt.cache_interval != 0)


def _loss_tail(outputs, data, want_pred):
    gt_samvit = data["gt_samvit"]
    h, w = int(data["h"]), int(data["w"])
    return gt_samvit, rm.feature_distill_loss(outputs["samvit"], h, w, gt_samvit, want_resized=want_pred)


def sam_train_loss(outputs, data, opt, want_pred: bool = True):
    """(pred_samvit, gt_samvit, loss) of trainer.py:533-555 from the low-resolution feature render.

    outputs: `model.render(rays_o_lr, rays_d_lr, staged=False, perturb=False, return_feats=1, H=h, W=w)`: 'samvit' [h*w, C].
    data: 'h', 'w' and 'gt_samvit' [1,C,Ho,Wo] -- the SAM encoder's features of the high-resolution render, or the cached ones.
    want_pred=False skips the resized prediction (None is returned in its place): the reference returns it, its train loop drops it.
    With opt.sam_type == 'sam_hq' the reference returns [gt_samvit, gt_interm_features] as the second value (trainer.py:553-554); so does
    this when data carries 'gt_interm_features'."""
    gt_samvit, res = _loss_tail(outputs, data, want_pred)
    pred, loss = (res[1], res[0]) if want_pred else (None, res)
    if getattr(opt, "sam_type", None) == "sam_hq" and "gt_interm_features" in data:
        gt_samvit = [gt_samvit, data["gt_interm_features"]]
    return pred, gt_samvit, loss


def sam_eval_loss(outputs, data, opt=None):
    """(pred_samvit, loss) of eval_step's feature branch (trainer.py:657-670): the same tail, the resized prediction kept for the
    decoder that follows it."""
    _, (loss, pred) = _loss_tail(outputs, data, True)
    return pred, loss
