"""The device-side evaluation meters: records, workspaces, accumulate operators and readers (mask_output.hip, ssim.hip)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._args import _image_rows, _mask_rows, _record_ptrs

EVAL_RECORD_BYTES, SSIM_RECORD_BYTES = C.sizeof(_lib.EvalRecord), C.sizeof(_lib.SsimRecord)


def eval_record(device) -> torch.Tensor:
    """A zeroed sn_eval_record on the device (as int64 words; read it with `read_eval_record`)."""
    return torch.zeros(EVAL_RECORD_BYTES // 8, device=device, dtype=torch.int64)


def eval_workspace(device) -> torch.Tensor:
    """The zero-at-rest scratch of mask_eval_accumulate / image_sqerr_accumulate (one per stream)."""
    return torch.zeros(_lib.MASK_EVAL_WORKSPACE_BYTES // 8, device=device, dtype=torch.int64)


def read_eval_record(record: torch.Tensor) -> dict:
    """The record's fields on the host (this is the host read: it synchronises)."""
    r = _lib.EvalRecord.from_buffer_copy(record.detach().cpu().numpy().tobytes())
    return {"nll_mean_sum": r.nll_mean_sum, "miou_sum": r.miou_sum, "mse_sum": r.mse_sum, "psnr_sum": r.psnr_sum, "images": int(r.images),
            "rgb_images": int(r.rgb_images), "inter": np.array(r.inter[:], dtype=np.uint64), "pred": np.array(r.pred[:], dtype=np.uint64),
            "truth": np.array(r.truth[:], dtype=np.uint64)}


def mask_eval_accumulate(logits, labels, record: torch.Tensor, workspace: torch.Tensor, eps: float = 1e-6, num_classes: Optional[int] = None) -> None:
    """eval_step's mask branch + the loss and mIoU meters for one image, in one launch and without a host read (sn_rm_mask_eval_accumulate;
    nerf/trainer.py:599-627, 1603-1604, nerf/metrics.py:165-179): logits [..., K], labels [...] (-1: unlabelled) -> `record` gets the image's
    mean NLL over its labelled pixels (0 when there is none) and its mean IoU of (argmax id, label) over num_classes >= K classes
    (default K) added, and its class counts stored."""
    m, lb = _mask_rows(logits, labels)
    N, K = m.shape
    m_ptr, lb_ptr = _lib.dev(m, "logits"), _lib.dev(lb, "labels", torch.int64)
    rec, ws = _record_ptrs(record, workspace, EVAL_RECORD_BYTES, _lib.MASK_EVAL_WORKSPACE_BYTES, "eval")
    _lib.check(_lib.lib().sn_rm_mask_eval_accumulate(m_ptr, lb_ptr, N, K, int(K if num_classes is None else num_classes), float(eps), rec, ws, _lib.stream()),
               "mask_eval_accumulate")


def image_sqerr_accumulate(pred, truth, record: torch.Tensor, workspace: torch.Tensor) -> None:
    """MSEMeter.update and PSNRMeter.update for one image without a host read (sn_rm_image_sqerr_accumulate; nerf/metrics.py:28-38, 217-221):
    pred, truth [..., 3] float32 (rows may be strided) -> `record` gets mean((pred - truth)^2) and -10 log10 of it added."""
    if not pred.is_cuda or not truth.is_cuda:
        raise RuntimeError("pred / truth must be a CUDA tensor")
    N = pred.numel() // pred.shape[-1] if pred.dim() != 2 else pred.shape[0]
    p, p_ptr, p_stride = _image_rows(pred, "pred", N)
    t, t_ptr, t_stride = _image_rows(truth, "truth", N)
    rec, ws = _record_ptrs(record, workspace, EVAL_RECORD_BYTES, _lib.MASK_EVAL_WORKSPACE_BYTES, "eval")
    _lib.check(_lib.lib().sn_rm_image_sqerr_accumulate(p_ptr, p_stride, t_ptr, t_stride, N, rec, ws, _lib.stream()), "image_sqerr_accumulate")


def ssim_record(device) -> torch.Tensor:
    """A zeroed sn_ssim_record on the device (as int64 words; read it with `read_ssim_record`)."""
    return torch.zeros(SSIM_RECORD_BYTES // 8, device=device, dtype=torch.int64)


def ssim_workspace(device) -> torch.Tensor:
    """The zero-at-rest scratch of image_ssim_accumulate (one per stream)."""
    return torch.zeros(_lib.SSIM_WORKSPACE_BYTES // 8, device=device, dtype=torch.int64)


def read_ssim_record(record: torch.Tensor) -> dict:
    """The record's fields on the host (this is the host read: it synchronises)."""
    r = _lib.SsimRecord.from_buffer_copy(record.detach().cpu().numpy().tobytes())
    return {"ssim_sum": r.ssim_sum, "last": r.last, "images": int(r.images)}


def image_ssim_accumulate(pred, truth, record: torch.Tensor, workspace: torch.Tensor, H: Optional[int] = None, W: Optional[int] = None,
                          data_range: Optional[float] = None) -> None:
    """SSIMMeter.update for one image pair without a host read (sn_rm_image_ssim_accumulate; nerf/metrics.py:124-131, torchmetrics'
    structural_similarity_index_measure at its defaults: 11 x 11 Gaussian window of sigma 1.5, mean over channels and the pixels a whole
    window fits around): pred, truth [H,W,3] float32, or [N,3] / row-strided views (the image columns of the packed [N,5] render buffer are
    read in place) with explicit H and W -> `record` gets the image's value added.  data_range: a positive number, or None as the reference
    calls it: max(pred.max() - pred.min(), truth.max() - truth.min()), found on the device by one more launch."""
    if not pred.is_cuda or not truth.is_cuda:
        raise RuntimeError("pred / truth must be a CUDA tensor")
    if H is None or W is None:
        if pred.dim() != 3:
            raise RuntimeError(f"image_ssim_accumulate: H and W are needed for a pred of shape {tuple(pred.shape)} (only [H,W,3] carries them)")
        H, W = pred.shape[0], pred.shape[1]
    H, W = int(H), int(W)
    if data_range is not None and not float(data_range) > 0:
        raise ValueError(f"image_ssim_accumulate: data_range {data_range!r} must be positive (None: derived from the images)")
    rows = []
    for t, name in ((pred, "pred"), (truth, "truth")):
        t, _, stride = _image_rows(t, name, H * W)
        if stride > _lib.SSIM_MAX_STRIDE:                            # the kernel reads a tile's rows whole: a sparser image is packed first
            t = t.contiguous()
        rows.append(t)
    rec, ws = _record_ptrs(record, workspace, SSIM_RECORD_BYTES, _lib.SSIM_WORKSPACE_BYTES, "ssim")
    _lib.check(_lib.lib().sn_rm_image_ssim_accumulate(rows[0].data_ptr(), rows[0].stride(0), rows[1].data_ptr(), rows[1].stride(0), H, W,
                                                      0.0 if data_range is None else float(data_range), rec, ws, _lib.stream()),
               "image_ssim_accumulate")
