"""The SAM-feature distillation loss and the feature map it resizes (distill.hip)."""
from __future__ import annotations

import torch
from torch.autograd import Function

from .. import _buffers, _lib
from ._args import _row_view


def _feature_target(target, C: int):
    """[C,Ho,Wo] or [1,C,Ho,Wo] -> (packed float32 tensor, Ho, Wo)."""
    if not target.is_cuda:
        raise RuntimeError("target must be a CUDA tensor")
    t = target.detach()
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[0] != C:
        raise RuntimeError(f"target must be [C,Ho,Wo] or [1,C,Ho,Wo] with C = {C}, got {tuple(target.shape)}")
    return t.float().contiguous(), int(t.shape[1]), int(t.shape[2])


class _feature_distill_loss(Function):
    """trainer.py:540-550 as one operator (sn_rm_feature_distill_loss): the scalar loss, and the gradient with respect to `samvit` made in
    the same call (`scale` inside it) and kept for backward, which is one multiply."""

    @staticmethod
    def forward(ctx, samvit, h, w, target, scale, want_resized):
        f = _row_view(samvit, "samvit", h * w, f"a {h} x {w} feature render")
        C_ = f.shape[1]
        tgt, Ho, Wo = _feature_target(target, C_)
        l = _lib.lib()
        scale_dev = scale if isinstance(scale, torch.Tensor) else None
        if scale_dev is not None:
            scale_dev = scale_dev.detach().reshape(-1)[:1].float().contiguous()
        nbytes = l.sn_rm_feature_distill_workspace_bytes(h, w, C_, Ho, Wo)
        if nbytes == 0:
            _lib.check(-2, "feature_distill_loss")
        ws = _buffers.zeroed("distill", f.device, _lib.stream(), nbytes)
        loss = torch.empty(1, device=f.device, dtype=torch.float32)
        grad = torch.empty(h * w, C_, device=f.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        resized = torch.empty(1, C_, Ho, Wo, device=f.device, dtype=torch.float32) if want_resized else None
        _lib.check(l.sn_rm_feature_distill_loss(f.data_ptr(), f.stride(0), h, w, C_, _lib.dev(tgt, "target"), Ho, Wo,
                                                1.0 if scale_dev is not None else float(scale), _lib.dev(scale_dev, "scale"), _lib.dev(loss, "loss"),
                                                _lib.dev(grad, "grad_feat"), _lib.dev(resized, "resized"), ws.data_ptr(), ws.numel() * 8, _lib.stream()),
                   "feature_distill_loss")
        ctx.save_for_backward(grad)
        ctx.fshape = samvit.shape
        out = loss[0]
        if scale_dev is not None or float(scale) != 1.0:
            out = out * (scale_dev[0] if scale_dev is not None else float(scale))
        if want_resized:
            ctx.mark_non_differentiable(resized)
            return out, resized
        return out

    @staticmethod
    def backward(ctx, grad_out, *unused):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out).view(ctx.fshape), None, None, None, None, None


def feature_distill_loss(samvit, h: int, w: int, target, scale=1.0, want_resized: bool = False):
    """The SAM-feature distillation loss of nerf/trainer.py:540-550 without the torch tail: samvit [h*w, C] (or [h, w, C]; row-strided views
    are read in place), target [1,C,Ho,Wo] (or [C,Ho,Wo]) -> scale * mean((bilinear_resize(samvit as [C,h,w], (Ho,Wo)) - target)^2), a device
    scalar; nothing reads the host.  scale: a number, or a one-element device tensor read by the kernel (e.g. a loss weight that changes under
    a captured graph).  The gradient reaches `samvit` alone (the reference's target is made under no_grad).  want_resized=True returns
    (loss, pred [1,C,Ho,Wo]) as the reference's train_step returns pred_samvit; pred carries no gradient.  The quantity: include/sanerf_hip.h."""
    return _feature_distill_loss.apply(samvit, int(h), int(w), target, scale, bool(want_resized))


def feature_map(samvit, h: int, w: int, size=None) -> torch.Tensor:
    """The rendered features `samvit` ([h*w, C] or [h, w, C]) as [1, C, Ho, Wo], bilinearly resized to size = (Ho, Wo) when given
    (sn_rm_feature_map: the forward half of feature_distill_loss, one launch, no gradient): what decode_step (trainer.py:928-930) and
    store_sam_feautres feed the SAM decoder / the cache with."""
    h, w = int(h), int(w)
    f = _row_view(samvit, "samvit", h * w, f"a {h} x {w} feature render")
    Ho, Wo = (h, w) if size is None else (int(size[0]), int(size[1]))
    out = torch.empty(1, f.shape[1], Ho, Wo, device=f.device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_feature_map(f.data_ptr(), f.stride(0), h, w, f.shape[1], Ho, Wo, _lib.dev(out, "out"), _lib.stream()), "feature_map")
    return out
