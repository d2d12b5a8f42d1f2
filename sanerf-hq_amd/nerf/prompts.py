"""The propagation of 3D point prompts across views, assembled from the HIP operators of `raymarching` (prompts.hip):

    test_step's "remember new point_3d" (trainer.py:802-834)      rm.points_lift + rm.point_store_update    PointPrompts.click
    the points file (trainer.py:88-112, save_3d_points :246-258)                                            PointPrompts.from_json / to_json
    projection, screen and depth test (trainer.py:838-875, 931-976)   rm.points_project                     PointPrompts.project, decode_prompts
    score selection, overlay_mask, overlay_point (trainer.py:979-991) rm.prompt_overlay                     decode_overlay

A click on one view becomes a 3D point; the point is projected into every other view and tested against that view's rendered depth; only
the surviving pixels prompt the SAM decoder.  The decoder call itself stays the caller's: `decode_prompts` hands it a fixed-shape prompt
(the kept points first, SAM's padding label -1 behind them) and `decode_overlay` takes its masks and scores.  Nothing here reads a device
value on the host -- `to_json` apart, which is the host read -- so click -> project -> overlay can be captured as one HIP graph.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import raymarching as rm


class PointPrompts:
    """The trainer's point_3d / input_labels / crucial_point_label / crucial_point_count / valid_threshold as a fixed-capacity store on the
    device.  Stated difference: the reference leaves crucial_point_label behind when a click adds or removes a point; here the flags are
    compacted with their points and a clicked point is not crucial."""

    def __init__(self, device, capacity: int = 256, dist_thresh: float = 0.01, depth_tol: float = 0.05):
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self.dist_thresh, self.depth_tol = float(dist_thresh), float(depth_tol)
        self.store = rm.point_store(self.device, self.capacity)
        self.crucial_count = 0
        self.valid_threshold = 0
        self._json_threshold = -1
        self._pixel = torch.zeros(1, 2, device=self.device, dtype=torch.int32)
        self._point = torch.zeros(1, 3, device=self.device, dtype=torch.float32)

    # -- the points file ------------------------------------------------------------------------------------------------------------
    def from_json(self, point_json: dict) -> "PointPrompts":
        """trainer.py:88-112: 'points' [n,3]; every label 1 but those listed in 'negative_labels'; 'crucial_point_index' sets the crucial
        flags and their number is the crucial count; 'valid_threshold' -1 becomes int(n * 0.8) + 1."""
        pts = torch.tensor(point_json["points"], dtype=torch.float32).reshape(-1, 3)
        n = pts.shape[0]
        if n > self.capacity:
            raise ValueError(f"PointPrompts.from_json: {n} points for a store of capacity {self.capacity}")
        labels = torch.ones(n, dtype=torch.int32)
        for i in point_json.get("negative_labels", []):
            labels[i] = 0
        crucial = torch.zeros(n, dtype=torch.int32)
        idx = list(point_json.get("crucial_point_index", []))
        for i in idx:
            crucial[i] = 1
        thr = point_json.get("valid_threshold", -1)
        if isinstance(thr, (list, tuple)):                              # save_3d_points writes a one-element tuple (trainer.py:253)
            thr = thr[0]
        self._json_threshold = int(thr)
        self.crucial_count = len(idx)
        self.valid_threshold = int(n * 0.8) + 1 if int(thr) == -1 else int(thr)
        st = self.store
        for k in ("xyz", "labels", "crucial", "status"):
            st[k].zero_()
        st["xyz"][:n].copy_(pts)
        st["labels"][:n].copy_(labels)
        st["crucial"][:n].copy_(crucial)
        st["count"].fill_(n)
        return self

    def to_json(self) -> dict:
        """save_3d_points (trainer.py:246-258).  This is the one place that reads the store on the host.  The reference always writes
        valid_threshold -1 and no crucial index; here the threshold is the one from_json was given (-1 otherwise) and the store's crucial
        flags are listed."""
        n = int(self.store["count"].item())
        labels = self.store["labels"][:n].cpu().tolist()
        crucial = self.store["crucial"][:n].cpu().tolist()
        return {"points": self.store["xyz"][:n].cpu().numpy().tolist(),
                "negative_labels": [i for i, v in enumerate(labels) if v == 0],
                "valid_threshold": self._json_threshold,
                "crucial_point_index": [i for i, v in enumerate(crucial) if v != 0]}

    # -- the device side ------------------------------------------------------------------------------------------------------------
    def click(self, rays_o, rays_d, depth, pixel, label, H: int, W: int) -> None:
        """trainer.py:802-834 for one click: pixel (x, y) -- two ints, or a [2] / [1,2] device tensor that a captured graph can rewrite --
        is lifted to o + d * depth and added to the store, or removes the stored points within dist_thresh of it.  Two launches."""
        if torch.is_tensor(pixel):
            px = pixel.reshape(1, 2)
        else:
            px = self._pixel
            px[:, 0:1].fill_(int(pixel[0]))
            px[:, 1:2].fill_(int(pixel[1]))
        rm.points_lift(px, rays_o, rays_d, depth, H, W, out=self._point)
        rm.point_store_update(self.store, self._point, label, self.dist_thresh)

    def project(self, poses, intrinsics, depth, H: int, W: int, want=("state",), out: Optional[dict] = None) -> dict:
        """The stored points in the V views of poses [V,4,4] against depth [V,H,W] (V = 1: one rendered view; V > 1: the depth stack of
        update_depth): rm.points_project's dict, with the store's count, crucial flags, crucial count and valid threshold.  One launch."""
        st = self.store
        return rm.points_project(st["xyz"], st["labels"], poses, intrinsics, depth, H, W, crucial=st["crucial"], n_points=st["count"],
                                 depth_tol=self.depth_tol, crucial_count=self.crucial_count, valid_threshold=self.valid_threshold,
                                 want=want, out=out)


def decode_prompts(outputs, data, prompts: PointPrompts, out: Optional[dict] = None) -> dict:
    """The first half of decode_step (trainer.py:931-976) on a full-resolution render of one view: outputs['depth'] (H*W values, may be the
    depth column of the packed render buffer), data['poses'] [1,4,4], data['intrinsics'] [1,4] or [4], data['H'], data['W'].
    Returns rm.points_project's dict for V = 1 and beside it what a decoder call needs, as views of it: 'point_coords' [cap,2] int32 (the
    pixels the reference hands sam_predict), 'point_labels' [cap] (-1 behind the kept ones), 'sam_point_coords' [cap,2] (the same in SAM's
    1024 frame), 'count' [1], 'is_valid' [1] (trainer.py:969-971), 'H', 'W'."""
    H, W = int(data["H"]), int(data["W"])
    intr = data["intrinsics"]
    res = prompts.project(data["poses"][:1] if data["poses"].dim() == 3 else data["poses"], intr[:1] if intr.dim() == 2 else intr,
                          outputs["depth"], H, W, out=out)
    res.update(point_coords=res["coords"][0], point_labels=res["labels"][0], sam_point_coords=res["sam_coords"][0],
               count=res["counts"][0, 1:2], is_valid=res["counts"][0, 3:4], H=H, W=W)
    return res


def decode_overlay(outputs, masks, scores, projected: dict, rgb8: bool = False, radius: int = 2, alpha: float = 0.7, out: Optional[dict] = None) -> dict:
    """The second half of decode_step (trainer.py:977-994) on the decoder's masks [M,H,W] (bool) and scores [M] (device tensors) and
    decode_prompts' dict: 'pred_rgb' [H,W,3] (the best-scoring mask in red at 1 - alpha, the prompts as squares), 'pred_masks' [1,H,W] bool
    (that mask), 'selected' [1] int32, 'is_valid' [1] int32, with rgb8=True also 'rgb8' [H,W,3] uint8.  In a view that keeps no point the
    image is returned unchanged with an empty mask and selected -1 (the reference's else branch returns zeros shaped like the image).
    outputs['image']: [H*W,3], may be the image columns of the packed render buffer.  One launch.  masks None: the points alone
    (test_step without a decoder, trainer.py:884)."""
    H, W = projected["H"], projected["W"]
    want = ["rgb", "pred_mask"] + (["rgb8"] if rgb8 else [])
    res = rm.prompt_overlay(outputs["image"], projected["overlay_coords"][0], projected["point_labels"], H, W, count=projected["count"], masks=masks,
                            scores=scores, radius=radius, alpha=alpha, want=want, out=out)
    ret = {"pred_rgb": res["rgb"], "pred_masks": res["pred_mask"].view(1, H, W), "selected": res["selected"], "is_valid": projected["is_valid"]}
    if rgb8:
        ret["rgb8"] = res["rgb8"]
    return ret
