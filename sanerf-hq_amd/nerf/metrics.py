"""The reference's SSIMMeter (nerf/metrics.py:102-144) on the device-side SSIM operator: `update` enqueues one image pair and reads
nothing on the host, `measure()` is the host read.  The quantity is torchmetrics' structural_similarity_index_measure at its defaults as
include/sanerf_hip.h states it (sn_rm_image_ssim_accumulate).  The other RGB meters are `nerf.mask_output.DeviceMeters`; LPIPS needs a VGG
and is not built."""
from __future__ import annotations

import os

import torch

from .. import raymarching as rm


class SSIMMeter:
    """V and N of the reference's meter live in one record on the device.  data_range: None as the reference calls the package (derived
    from each pair), or a positive number."""

    def __init__(self, device=None, data_range=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.data_range = data_range
        self.record = rm.ssim_record(self.device)
        self.workspace = rm.ssim_workspace(self.device)

    def clear(self) -> None:
        self.record.zero_()

    def prepare_inputs(self, *inputs):
        """[H,W,3] or [1,H,W,3] -> [H,W,3] on the meter's device (the reference's loaders yield one view per batch)."""
        outputs = []
        for inp in inputs:
            if inp.dim() == 4:
                if inp.shape[0] != 1:
                    raise RuntimeError(f"SSIMMeter: a batch of {inp.shape[0]} images; update() takes one view, [H,W,3] or [1,H,W,3]")
                inp = inp[0]
            if inp.dim() != 3 or inp.shape[-1] != 3:
                raise RuntimeError(f"SSIMMeter: an input of shape {tuple(inp.shape)}; [H,W,3] or [1,H,W,3]")
            outputs.append(inp.to(self.device))
        return outputs

    def update(self, preds, truths) -> None:
        preds, truths = self.prepare_inputs(preds, truths)
        rm.image_ssim_accumulate(preds, truths, self.record, self.workspace, data_range=self.data_range)

    def measure(self):
        r = rm.read_ssim_record(self.record)
        return r["ssim_sum"] / r["images"] if r["images"] > 0 else 0

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, "SSIM"), self.measure(), global_step)

    def report(self):
        return f"SSIM = {self.measure():.6f}"
