"""What nerf/trainer.py does between a mask-mode render's `instance_mask_logits` and what a user sees or scores, assembled from the HIP
operators of `raymarching`:

    test_step's mask branch (trainer.py:730-781)            rm.mask_output             mask_test_outputs
    eval_step's mask branch (trainer.py:599-627)            rm.mask_eval_accumulate    mask_eval_step, DeviceMeters.update_mask
    MeanIoUMeter / loss.item() (metrics.py:165-179, trainer.py:1603-1611)       "
    PSNRMeter / MSEMeter (metrics.py:28-38, 217-221)         rm.image_sqerr_accumulate  DeviceMeters.update_rgb
    SSIMMeter (metrics.py:102-144)                           rm.image_ssim_accumulate   DeviceMeters(ssim=True).update_rgb, nerf.metrics.SSIMMeter

The output stage is one launch per frame, the evaluation of a view one launch (two with the RGB meters; SSIM adds one, or two when it
derives its data range).  Nothing here reads a device value on the host before `DeviceMeters.measure()`, so a render followed by these
calls can be captured as a HIP graph, and a validation epoch synchronises once.  LPIPS needs a third-party network (a VGG) and stays out.
"""
from __future__ import annotations

import torch

from .. import raymarching as rm

MODES = ("heatmap", "composition", "mask")


def reference_color_map(device=None) -> torch.Tensor:
    """The trainer's 100-entry colour table (trainer.py:129-133: gist_ncar resampled to 100 entries, entry (7 i + 5) mod 100 for id i), built
    through matplotlib at run time; it is never embedded in the package."""
    try:
        import matplotlib
    except ImportError as e:
        raise RuntimeError("reference_color_map: the reference builds its colour table with matplotlib ('gist_ncar'), which is not installed; "
                           "pass a [C,3] color_map tensor of your own") from e
    import numpy as np
    cmap = matplotlib.colormaps["gist_ncar"].resampled(100) if hasattr(matplotlib, "colormaps") else matplotlib.cm.get_cmap("gist_ncar", 100)
    table = np.array([cmap((i * 7 + 5) % 100)[:3] for i in range(100)])
    t = torch.from_numpy(table).to(torch.float)
    return t.to(device) if device is not None else t


def _render_id(opt) -> int:
    rid = int(getattr(opt, "render_mask_instance_id", -1))
    return rid if 0 <= rid < int(opt.n_inst) else -1                   # trainer.py:742, 756-759, 767-770


def _check_opt(opt) -> None:
    if float(getattr(opt, "label_regularization_weight", 0) or 0) > 0:
        raise NotImplementedError("label_regularization reads opt.patch_size, which the reference's main.py never defines (trainer.py:307-334)")


def mask_test_outputs(outputs, opt, color_map, bg_color=None, H=None, W=None, rgb8: bool = False, alpha: float = 0.7, out=None) -> dict:
    """test_step's mask branch (trainer.py:730-781) on what `model.render(..., return_mask=1)` returned -- 'instance_mask_logits' [N,K] and
    'image' [N,3], which may be a strided view of the packed [N,5] render buffer (the `packed=` route): it is read in place.

    Returns 'pred_rgb' (the overlay opt.render_mask_type selects: 'heatmap', 'composition' or 'mask'; anything else leaves the rendered image,
    as the reference does), 'pred_mask' (the softmax / sigmoid probabilities; in 'mask' mode the 0/1 mask `instance_id == render_id`, as the
    reference rebinds it), 'instance_id', 'confidence', and with rgb8=True 'rgb8' = the (pred_rgb * 255).astype(uint8) the reference makes on
    the host.  With H and W the per-pixel tensors are viewed [H,W,...].  One launch ('mask' mode: two more torch launches for its 0/1 mask).
    out: dict that keeps the output tensors between calls."""
    logits = outputs["instance_mask_logits"]
    K = logits.shape[-1]
    if K != int(opt.n_inst):
        raise RuntimeError(f"mask_test_outputs: {K} logits per pixel for opt.n_inst = {opt.n_inst}")
    kind = getattr(opt, "render_mask_type", None)
    mode = kind if kind in MODES else "none"
    want = ["probs", "instance_id", "confidence", "rgb"] + (["rgb8"] if rgb8 else [])
    res = rm.mask_output(logits.reshape(-1, K), color_map=color_map, image=outputs["image"], mode=mode, render_id=_render_id(opt), alpha=alpha,
                         bg_color=bg_color, want=want, out=out)
    pred_mask = res["probs"]
    if mode == "mask":
        pred_mask = (res["instance_id"] == _render_id(opt)).to(torch.float32)            # trainer.py:773-774
    ret = {"pred_rgb": res["rgb"], "pred_mask": pred_mask, "instance_id": res["instance_id"], "confidence": res["confidence"]}
    if rgb8:
        ret["rgb8"] = res["rgb8"]
    if H is not None and W is not None:
        ret = {k: v.view(H, W, *v.shape[1:]) for k, v in ret.items()}
    return ret


class DeviceMeters:
    """The reference's MeanIoUMeter, PSNRMeter, MSEMeter and the running loss of evaluate_one_epoch as one record on the device:
    update_mask / update_rgb add an image without a host read, measure() does the only one.  ssim=True: a second record beside it holds
    the SSIMMeter, fed by update_rgb too."""

    def __init__(self, device, num_classes=None, eps: float = 1e-6, ssim: bool = False):
        self.device = torch.device(device)
        self.num_classes = num_classes
        self.eps = float(eps)
        self.record = rm.eval_record(self.device)
        self.workspace = rm.eval_workspace(self.device)
        self.ssim = bool(ssim)
        if self.ssim:
            self.ssim_record = rm.ssim_record(self.device)
            self.ssim_workspace = rm.ssim_workspace(self.device)

    def clear(self) -> None:
        self.record.zero_()
        if self.ssim:
            self.ssim_record.zero_()

    def update_mask(self, logits, labels, eps=None) -> None:
        """One image's logits [..., K] and labels [...] (-1: unlabelled): eval_step's loss and MeanIoUMeter.update(argmax id, label).
        eps: the clamp of the loss for this image (default: the constructor's)."""
        rm.mask_eval_accumulate(logits, labels, self.record, self.workspace, self.eps if eps is None else float(eps), self.num_classes)

    def update_rgb(self, preds, truths, H=None, W=None) -> None:
        """One image's prediction and ground truth [..., 3]: MSEMeter.update and PSNRMeter.update; with ssim=True also SSIMMeter.update,
        which needs the image's shape: [H,W,3] inputs, or H and W beside [N,3] rows."""
        rm.image_sqerr_accumulate(preds, truths, self.record, self.workspace)
        if self.ssim:
            rm.image_ssim_accumulate(preds, truths, self.ssim_record, self.ssim_workspace, H=H, W=W)

    def read(self) -> dict:
        """The raw record (sums, image counts, the last image's class counts) on the host."""
        return rm.read_eval_record(self.record)

    def measure(self) -> dict:
        """{'mIoU', 'loss', 'PSNR', 'MSE'} (and 'SSIM' with ssim=True): means over the images seen, 0 for a meter that saw none (as the
        reference's meters)."""
        r = self.read()
        n, m = r["images"], r["rgb_images"]
        res = {"mIoU": r["miou_sum"] / n if n else 0, "loss": r["nll_mean_sum"] / n if n else 0,
               "PSNR": r["psnr_sum"] / m if m else 0, "MSE": r["mse_sum"] / m if m else 0}
        if self.ssim:
            s = rm.read_ssim_record(self.ssim_record)
            res["SSIM"] = s["ssim_sum"] / s["images"] if s["images"] else 0
        return res


def mask_eval_step(outputs, data, opt, meters: DeviceMeters):
    """eval_step's mask branch (trainer.py:599-646) on a mask-mode render of one view: adds the view's loss and mIoU to `meters` and returns
    (pred_rgb, pred_depth, gt_mask) as views of what it was given.  The loss is not returned: it exists on the device only, inside the
    record, until meters.measure().  (The probabilities the reference also returns are mask_test_outputs' 'pred_mask'.)"""
    _check_opt(opt)
    if data.get("use_default_intrinsics"):
        raise RuntimeError("mask_eval_step: a view with use_default_intrinsics has no ground truth to score (trainer.py:620, 632-633)")
    logits = outputs["instance_mask_logits"]
    K = logits.shape[-1]
    if K != int(opt.n_inst):
        raise RuntimeError(f"mask_eval_step: {K} logits per pixel for opt.n_inst = {opt.n_inst}")
    gt_mask = data["masks"].to(torch.long)
    meters.update_mask(logits.reshape(-1, K), gt_mask.reshape(-1), eps=float(opt.epsilon))
    return outputs["image"], outputs["depth"], gt_mask
