"""The mask field's losses and its output stage (mask_losses.hip, mask_output.hip)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
from torch.autograd import Function

from .. import _lib
from ._args import _f32, _i64, _image_rows, _mask_rows, _outputs


class _mask_nll(Function):
    """-log(clamp(softmax(logits)[label], eps, 1 - eps)) per ray, value and gradient in one kernel (sn_rm_mask_nll)."""

    @staticmethod
    def forward(ctx, logits, labels, eps):
        shape = logits.shape[:-1]
        lg, lb = _f32(logits.reshape(-1, logits.shape[-1])), _i64(labels.reshape(-1))
        N, K = lg.shape
        loss = torch.empty(N, device=lg.device, dtype=torch.float32)
        grad = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        _lib.check(_lib.lib().sn_rm_mask_nll(_lib.dev(lg, "logits"), _lib.dev(lb, "labels", torch.int64), N, K, float(eps), _lib.dev(loss, "loss"),
                                             _lib.dev(grad, "grad_logits"), _lib.stream()), "mask_nll")
        ctx.save_for_backward(grad)
        ctx.lshape = logits.shape
        return loss.view(*shape, 1)

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out.reshape(-1, 1)).view(ctx.lshape), None, None


def mask_nll(logits, labels, eps: float = 1e-6):
    """The mask-field training loss of nerf/trainer.py:419-428, per ray: logits [..., n_inst], labels [...] (int) ->
    [..., 1] = -log(gather(clamp(softmax(logits, -1), eps, 1 - eps), -1, labels[..., None])); the trainer takes its .mean()."""
    return _mask_nll.apply(logits, labels, eps)


def ray_pair_select(incoherent, S: int, uniform: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pixels each group of the ray-pair loss compares against (nerf/trainer.py:268-276 without torch.multinomial, sn_rm_ray_pair_select):
    incoherent [G,P] or [G,P,1] (the rays' error-map values), uniform [G,P] in [0,1) (drawn here with one torch.rand when None) -> int64
    [G,S]: among a group's pixels with (1 - incoherent) > 0.8 (all its pixels when there is none) the S with the smallest uniform value, in
    ascending order of it; -1 in the slots a group with fewer than S candidates cannot fill (the reference raises there)."""
    G, P = incoherent.shape[0], incoherent.shape[1]
    inc = _f32(incoherent.reshape(G, P))
    if uniform is None:
        uniform = torch.rand(G, P, device=inc.device, dtype=torch.float32)
    u = _f32(uniform.reshape(G, P))
    out = torch.empty(G, int(S), device=inc.device, dtype=torch.int64)
    _lib.check(_lib.lib().sn_rm_ray_pair_select(_lib.dev(inc, "incoherent"), _lib.dev(u, "uniform"), G, P, int(S), _lib.dev(out, "sample_index", torch.int64),
                                                _lib.stream()), "ray_pair_select")
    return out


class _ray_pair_rgb_loss(Function):
    """nerf/trainer.py:276-303 as one kernel (sn_rm_ray_pair_rgb_loss): the scalar loss, and the gradient with respect to `masks` made in the
    same launch and kept for backward (the mean's 1 / n_pairs inside it)."""

    @staticmethod
    def forward(ctx, rgb, masks, sample_index, threshold, exp_weight, epsilon, use_pred_logistics, from_logits):
        m = _f32(masks)
        G, P, K = m.shape
        c = _f32(rgb.reshape(G, P, 3))
        idx = sample_index.detach().reshape(G, -1).contiguous()
        S = idx.shape[1]
        per_pair = torch.empty(G, S, device=m.device, dtype=torch.float32)
        grad = torch.empty_like(m) if ctx.needs_input_grad[1] else None
        count = torch.empty(1, device=m.device, dtype=torch.float32)
        _lib.check(_lib.lib().sn_rm_ray_pair_rgb_loss(_lib.dev(c, "rgb"), _lib.dev(m, "masks"), int(bool(from_logits)), _lib.dev(idx, "sample_index", torch.int64),
                                                      G, P, S, K, float(threshold), float(exp_weight), float(epsilon), int(bool(use_pred_logistics)),
                                                      1.0, None, _lib.dev(per_pair, "loss_per_pair"), _lib.dev(count, "pair_count"), _lib.dev(grad, "grad_masks"),
                                                      _lib.stream()),
                   "ray_pair_rgb_loss")
        ctx.save_for_backward(grad)
        ctx.mshape = masks.shape
        return per_pair.sum() / count[0]                           # max(pairs, 1) as the kernel counted them; stays on the device

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return None, (grad * grad_out).view(ctx.mshape), None, None, None, None, None, None


def ray_pair_rgb_loss(rgb, masks, sample_index, threshold, exp_weight, epsilon, use_pred_logistics: bool = False, from_logits: bool = False):
    """The ray-pair RGB loss of nerf/trainer.py:260-305 for given sample indices (ray_pair_select): rgb [G,P,3], masks [G,P,K] (softmax
    probabilities, or the logits with from_logits=True: then the gradient reaches the logits without a softmax node), sample_index [G,S]
    int64 (-1 = no pair) -> scalar: the mean over the pairs of sum_i sim exp(-exp_weight cos(masks_i, q) - epsilon) / sum_i sim.  rgb gets no
    gradient (the colour comparison is boolean), nor does the sampled pixel's q (detached in the reference)."""
    return _ray_pair_rgb_loss.apply(rgb, masks, sample_index, threshold, exp_weight, epsilon, use_pred_logistics, from_logits)


def mask_error(masks, labels, exp_weight, epsilon, from_logits: bool = False) -> torch.Tensor:
    """The error measure of the error map (nerf/trainer.py:1426-1432, sn_rm_mask_error): masks [..., K] (probabilities, or logits with
    from_logits=True), labels [...] -> [...] = exp(-exp_weight cos(masks, onehot(labels)) - epsilon).  No gradient."""
    m, lb = _mask_rows(masks, labels)
    N, K = m.shape
    err = torch.empty(N, device=m.device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_mask_error(_lib.dev(m, "masks"), int(bool(from_logits)), _lib.dev(lb, "labels", torch.int64), N, K, float(exp_weight),
                                           float(epsilon), _lib.dev(err, "error"), _lib.stream()), "mask_error")
    return err.view(masks.shape[:-1])


def error_map_update(error_map, index, inds, masks, labels, exp_weight, epsilon, from_logits: bool = False) -> torch.Tensor:
    """The per-step EMA of nerf/trainer.py:457-464, in place (sn_rm_error_map_update): error_map [M, S*S] float32 contiguous, index [1] or
    [N] (the rays' images), inds [N] (their coarse cells), masks [N,K], labels [N]:
    error_map[index, inds] = 0.1 * error_map[index, inds] + 0.9 * mask_error(masks, labels).  Every new value comes from the map as it was
    before the call; rays that share a target leave one of their values.  Returns the rays' error [N].  No gradient."""
    m, lb = _mask_rows(masks, labels)
    N, K = m.shape
    if error_map.dim() != 2:
        raise RuntimeError("error_map must be [images, cells]")
    rows, cols = _i64(torch.as_tensor(index, device=m.device).reshape(-1)), _i64(inds.reshape(-1))
    if cols.shape[0] != N or rows.shape[0] not in (1, N):
        raise RuntimeError(f"error_map_update: {rows.shape[0]} image indices / {cols.shape[0]} cells for {N} rays")
    err = torch.empty(N, device=m.device, dtype=torch.float32)
    stage = torch.empty(N, device=m.device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_error_map_update(_lib.dev(m, "masks"), int(bool(from_logits)), _lib.dev(lb, "labels", torch.int64),
                                                 _lib.dev(rows, "index", torch.int64), rows.shape[0], _lib.dev(cols, "inds", torch.int64), N, K,
                                                 float(exp_weight), float(epsilon), error_map.shape[0], error_map.shape[1],
                                                 _lib.dev(error_map, "error_map"), _lib.dev(stage, "stage"), _lib.dev(err, "error"), _lib.stream()),
               "error_map_update")
    return err


def mask_output(logits, color_map=None, image=None, mode: str = "none", render_id: int = -1, alpha: float = 0.7, bg_color=None,
                want: Sequence[str] = ("probs", "instance_id", "confidence", "rgb", "rgb8"), out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """The mask field's output stage in one launch (sn_rm_mask_output; nerf/trainer.py:730-781 + nerf/utils.py:49-77): logits [..., K],
    K <= 32 (K = 1: sigmoid) -> the tensors named in `want`: probs [..., K], instance_id [...] int64 (argmax, lowest index on a tie),
    confidence [...] (max probability), rgb [..., 3] float32 and rgb8 [..., 3] uint8 = trunc(clamp(255 rgb, 0, 255)).
    mode: 'heatmap' (color_map[id] * confidence, or color_map[render_id] * p[render_id] for 0 <= render_id < K), 'composition'
    (image * alpha + (render_id == -1 or id == render_id ? color_map[id] : image) * (1 - alpha)), 'mask' (image where id == render_id,
    bg_color elsewhere) or 'none' (rgb = image).  image: [..., 3] float32, rows may be strided (a view of the packed [N,5] render buffer);
    color_map [C,3] with C >= K; bg_color: a number or 3 values (tensor: on the device, nothing is read on the host).
    out: a dict of preallocated tensors to write into (a captured graph keeps its outputs); a wanted output that is missing from it is
    allocated and added, one of the wrong shape, dtype or device raises.  No gradient."""
    if mode not in _lib.MASK_OUT_MODES:
        raise ValueError(f"mask_output: mode {mode!r}, one of {sorted(_lib.MASK_OUT_MODES)}")
    unknown = set(want) - {"probs", "instance_id", "confidence", "rgb", "rgb8"}
    if unknown:
        raise ValueError(f"mask_output: unknown outputs {sorted(unknown)}")
    K = logits.shape[-1]
    lead = logits.shape[:-1]
    lg = _f32(logits.reshape(-1, K))
    N = lg.shape[0]
    lg_ptr = _lib.dev(lg, "logits")
    dev = lg.device
    colour = "rgb" in want or "rgb8" in want
    img_ptr, img_stride, cm_ptr, n_colors, bg_ptr, keep = None, 0, None, 0, None, []
    if colour:
        if mode != "heatmap":
            if image is None:
                raise RuntimeError(f"mask_output: mode {mode!r} needs the rendered image")
            img, img_ptr, img_stride = _image_rows(image, "image", N)
            keep.append(img)
        if mode in ("heatmap", "composition"):
            if color_map is None:
                raise RuntimeError(f"mask_output: mode {mode!r} needs a color_map")
            cm = _f32(color_map.reshape(-1, 3))
            cm_ptr, n_colors = _lib.dev(cm, "color_map"), cm.shape[0]
            keep.append(cm)
        if mode == "mask":
            if bg_color is None:
                raise RuntimeError("mask_output: mode 'mask' needs bg_color (trainer.py:777)")
            if torch.is_tensor(bg_color):
                bg = bg_color.detach().to(device=dev, dtype=torch.float32).reshape(-1)
                if bg.numel() not in (1, 3):
                    raise RuntimeError(f"mask_output: bg_color has {bg.numel()} values (1 or 3; a per-ray background is not built)")
                bg = bg.expand(3).contiguous()
            else:
                vals = [float(v) for v in (bg_color if isinstance(bg_color, (list, tuple)) else [bg_color] * 3)]
                if len(vals) != 3:
                    raise RuntimeError(f"mask_output: bg_color has {len(vals)} values (a number or 3)")
                bg = torch.empty(3, device=dev, dtype=torch.float32)
                for j, v in enumerate(vals):                         # fills, not a host-to-device copy: they can be captured
                    bg[j:j + 1].fill_(v)
            bg_ptr = _lib.dev(bg, "bg_color")
            keep.append(bg)
    shapes = {"probs": ((*lead, K), torch.float32), "instance_id": (tuple(lead), torch.int64), "confidence": (tuple(lead), torch.float32),
              "rgb": ((*lead, 3), torch.float32), "rgb8": ((*lead, 3), torch.uint8)}
    res, ptr = _outputs("mask_output", shapes, want, out, dev)
    _lib.check(_lib.lib().sn_rm_mask_output(lg_ptr, N, K, img_ptr, img_stride, cm_ptr, n_colors, _lib.MASK_OUT_MODES[mode], int(render_id), float(alpha), bg_ptr,
                                            ptr["probs"], ptr["instance_id"], ptr["confidence"], ptr["rgb"], ptr["rgb8"], _lib.stream()), "mask_output")
    return res
