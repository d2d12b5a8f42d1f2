"""The loss tail of the RGB training step (rgb_loss.hip)."""
from __future__ import annotations

import torch
from torch.autograd import Function

from .. import _buffers, _lib
from ._args import _f32, _row_view


class _rgb_loss(Function):
    """trainer.py:364-392 after the render as one operator (sn_rm_rgb_loss): the scalar loss, and the gradients with respect to `image`
    and `weights_sum` made in the same launch and kept for backward, which is one multiply per differentiable input."""

    @staticmethod
    def forward(ctx, image, weights_sum, truth, bg, image_has_bg, lambda_entropy, want_pred, coef0, coef1, extra0, extra1):
        if not torch.is_tensor(image) or image.dim() < 2 or image.shape[-1] != 3:
            raise RuntimeError(f"image must be an [N,3] tensor, got {tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
        if not image.is_cuda:
            raise RuntimeError("image must be a CUDA tensor")
        N = image.numel() // 3
        if N == 0:
            raise RuntimeError("rgb_loss: no rays")
        im = _row_view(image, "image", N, f"{N} rays", (3,))
        tr = _row_view(truth, "truth", N, f"{N} rays", (3, 4))
        if not torch.is_tensor(weights_sum) or not weights_sum.is_cuda:
            raise RuntimeError("weights_sum must be a CUDA tensor")
        if weights_sum.numel() != N:
            raise RuntimeError(f"weights_sum: {weights_sum.numel()} values for {N} rays")
        w = _f32(weights_sum.reshape(-1))
        bg_value, bg_t, bg_rows = 0.0, None, 0
        if torch.is_tensor(bg):
            if not bg.is_cuda:
                raise RuntimeError("bg must be a number or a CUDA tensor")
            if bg.dim() == 1 and bg.numel() == 3:
                bg_rows = 1
            elif bg.dim() >= 2 and bg.shape[-1] == 3 and bg.numel() == 3 * N:
                bg_rows = N
            else:
                raise RuntimeError(f"bg must be a number, a [3] tensor or an [N,3] tensor with N = {N}, got {tuple(bg.shape)}")
            bg_t = _f32(bg.reshape(-1, 3))
        else:
            bg_value = float(bg)
        extras = []
        for e, name in ((extra0, "extras[0]"), (extra1, "extras[1]")):
            if e is None:
                extras.append(None)
                continue
            if not torch.is_tensor(e) or not e.is_cuda or e.numel() != 1:
                raise RuntimeError(f"{name} must be a one-element CUDA tensor")
            extras.append(_f32(e.reshape(1)))
        dev_ = im.device
        new = lambda *shape: torch.empty(*shape, device=dev_, dtype=torch.float32)   # noqa: E731
        record = new(4)
        pred = new(N, 3) if want_pred else None
        gt = new(N, 3) if want_pred else None
        g_im = new(N, 3) if ctx.needs_input_grad[0] else None
        g_ws = new(N) if ctx.needs_input_grad[1] else None
        ws = _buffers.zeroed("rgb_loss", dev_, _lib.stream(), _lib.RGB_LOSS_WORKSPACE_BYTES)
        _lib.check(_lib.lib().sn_rm_rgb_loss(im.data_ptr(), im.stride(0), _lib.dev(w, "weights_sum"), tr.data_ptr(), tr.stride(0), tr.shape[1], N,
                                             bg_value, _lib.dev(bg_t, "bg"), bg_rows, 1 if image_has_bg else 0, float(lambda_entropy),
                                             _lib.dev(extras[0], "extras[0]"), float(coef0), _lib.dev(extras[1], "extras[1]"), float(coef1),
                                             _lib.dev(pred, "pred_rgb"), _lib.dev(gt, "gt_rgb"), _lib.dev(record, "record"),
                                             _lib.dev(g_im, "grad_image"), _lib.dev(g_ws, "grad_weights_sum"), ws.data_ptr(), _lib.stream()),
                   "rgb_loss")
        ctx.save_for_backward(g_im, g_ws)
        ctx.shapes = (image.shape, weights_sum.shape, None if extra0 is None else extra0.shape, None if extra1 is None else extra1.shape)
        ctx.coefs = (float(coef0), float(coef1))
        if want_pred:
            ctx.mark_non_differentiable(pred, gt)
            return record[0], pred, gt
        return record[0]

    @staticmethod
    def backward(ctx, grad_out, *unused):
        g_im, g_ws = ctx.saved_tensors
        s_im, s_ws, s_e0, s_e1 = ctx.shapes
        ge = [None, None]
        for i, s in enumerate((s_e0, s_e1)):
            if s is not None and ctx.needs_input_grad[9 + i]:
                ge[i] = (grad_out * ctx.coefs[i]).reshape(s)
        return ((g_im * grad_out).view(s_im) if g_im is not None else None, (g_ws * grad_out).view(s_ws) if g_ws is not None else None,
                None, None, None, None, None, None, None, ge[0], ge[1])


def rgb_loss(image, weights_sum, truth, bg=1.0, image_has_bg: bool = True, lambda_entropy: float = 0.0, extras=(), want_pred: bool = True):
    """The loss tail of the RGB training step (nerf/trainer.py:364-392) in one launch, nothing read on the host (sn_rm_rgb_loss; the
    quantity: include/sanerf_hip.h): image [N,3] and truth [N,3] or [N,4] (row-strided views, such as the image columns of the packed
    render buffer, are read in place), weights_sum [N]; bg: a number, a [3] tensor or an [N,3] tensor (an RGBA truth is blended over it).
    image_has_bg=False: `image` was rendered over bg = 0 and the background term (1 - weights_sum) * bg of renderer.py:353 is added here,
    with its gradient into weights_sum -- what lets the fused training route serve a per-ray background.  lambda_entropy: the weight of
    the entropy of clamp(weights_sum, 1e-5, 1 - 1e-5) (trainer.py:389-392; 0: not evaluated).  extras: up to two (one-element device
    tensor, coefficient) pairs added to the loss as coefficient * tensor (the proposal and the distortion loss).
    Returns (loss, pred_rgb, gt_rgb); want_pred=False returns (loss, None, None).  The gradient reaches `image`, `weights_sum` and the
    extras (coefficient * grad_out); it is made in the forward launch and backward is one multiply each.  pred_rgb and gt_rgb [N,3] carry
    NO gradient: the reference's train loop only feeds them to the meters.  No gradient goes to truth or bg."""
    extras = list(extras)
    if len(extras) > 2:
        raise RuntimeError(f"rgb_loss: at most two extras, got {len(extras)}")
    for e in extras:
        if not isinstance(e, (tuple, list)) or len(e) != 2:
            raise RuntimeError("rgb_loss: extras are (tensor, coefficient) pairs")
    extras += [(None, 0.0)] * (2 - len(extras))
    res = _rgb_loss.apply(image, weights_sum, truth, bg, bool(image_has_bg), float(lambda_entropy), bool(want_pred), float(extras[0][1]),
                          float(extras[1][1]), extras[0][0], extras[1][0])
    return res if want_pred else (res, None, None)
