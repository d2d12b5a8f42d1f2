"""Volume renderer with the reference's `NeRFRenderer` contract (nerf/renderer.py:142-385):
`render(rays_o, rays_d, staged=False, cam_near_far=None, **kw)` / `run(...)` returning the
same result keys (`image`, `depth`, `weights_sum`, `samvit`, `instance_mask_logits`,
`weights`, `num_points`, `proposal_loss`, `distort_loss`), same buffers (`aabb_train`,
`aabb_infer`) and the same `opt` fields.

Two execution paths:
  * fused (default whenever no gradient has to reach the radiance field): one
    `raymarching.render_rays` call = sn_rm_render_rays, which runs proposal resampling, the
    hash-grid field, the MLPs and compositing on the GPU without materialising per-sample
    tensors; the SAM-feature and mask heads then consume its last-stage samples.  perturb=True
    without a field gradient (the SAM step's ground-truth image, the viewer's supersampling) is
    the same call fed with per-ray jitter tables from `model.jitter`, a Philox counter on the
    device (`raymarching.DeviceJitter`; `fused_perturb = False`: the stage loop below).
  * differentiable (RGB training): the stage loop in torch autograd with the
    HIP encoders / `sample_pdf` / `composite` as building blocks; its jitter is `torch.rand`
    unless the caller has set `model.jitter`.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import raymarching as rm


def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.05):
    return rm.near_far_from_aabb(rays_o, rays_d, aabb, min_near)


def contract(x):
    return rm.contract(x)


def sample_pdf(bins, weights, T, perturb=False):
    return rm.sample_pdf(bins, weights, T, perturb)


def proposal_loss(all_bins, all_weights):
    """Inter-level proposal loss (nerf/renderer.py:30-57)."""
    if (len(all_bins) > 1 and all(w.is_cuda and w.dim() == 2 and w.shape[-1] <= rm.PROPOSAL_LOSS_MAX_T for w in all_weights)):
        return rm.proposal_loss_all(all_bins, all_weights)       # one autograd node, one kernel per stage and direction
    ref_bins = all_bins[-1].detach()
    ref_w = all_weights[-1].detach()
    total = 0
    for bins, w in zip(all_bins[:-1], all_weights[:-1]):
        if w.is_cuda and max(w.shape[-1], ref_w.shape[-1]) <= rm.PROPOSAL_LOSS_MAX_T and w.dim() == 2:
            total = total + rm.proposal_loss_stage(bins, w, ref_bins, ref_w)      # one kernel forward, one backward
            continue
        cum = torch.cat([torch.zeros_like(w[..., :1]), torch.cumsum(w, dim=-1)], dim=-1)
        last = w.shape[-1] - 1
        lo = (torch.searchsorted(bins[..., :-1].contiguous(), ref_bins[..., :-1].contiguous(), right=True) - 1).clamp(0, last)
        hi = torch.searchsorted(bins[..., 1:].contiguous(), ref_bins[..., 1:].contiguous(), right=True).clamp(0, last)
        bound = torch.take_along_dim(cum[..., 1:], hi, dim=-1) - torch.take_along_dim(cum[..., :-1], lo, dim=-1)
        total = total + ((ref_w - bound).clamp(min=0) ** 2 / (ref_w + 1e-8)).mean()
    return total


def distort_loss(bins, weights):
    """Mip-NeRF-360 distortion loss, O(T) per ray (what the reference gets from the third-party
    `eff_distloss`, nerf/renderer.py:17-27): sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i, mean over rays."""
    if weights.is_cuda and weights.dim() == 2 and weights.shape[-1] <= rm.DISTORT_LOSS_MAX_T:
        return rm.distort_loss(bins, weights)              # value and gradient from one kernel
    d = bins[..., 1:] - bins[..., :-1]
    m = bins[..., :-1] + d / 2
    wm = weights * m
    cw = torch.cumsum(weights, dim=-1) - weights          # exclusive prefix
    cwm = torch.cumsum(wm, dim=-1) - wm
    inter = 2 * (wm * cw - weights * cwm).sum(-1)
    intra = (weights * weights * d).sum(-1) / 3
    return (inter + intra).mean()


class NeRFRenderer(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.real_bound = opt.bound                         # world-space marching bound
        self.bound = 2 if opt.contract else opt.bound       # grid-query bound (renderer.py:152-155)
        self.cascade = 1 + math.ceil(math.log2(self.bound))
        self.min_near = opt.min_near
        self.density_thresh = opt.density_thresh
        b = float(self.real_bound)
        aabb = torch.FloatTensor([-b, -b, -b, b, b, b])
        self.register_buffer("aabb_train", aabb)
        self.register_buffer("aabb_infer", aabb.clone())
        self._plan = None
        self._plan_key = None
        self.render_table_dtype = torch.float32             # torch.float16: render from half-precision table copies
        self.render_tables_static = False                   # True: skip the per-call refresh of those copies (frozen field)
        self.render_keep_packs = False                      # True (frozen field, eval mode): the fused render keeps its packed weights / pair rows
                                                            # between calls (RenderPlan.keep_packs; invalidate_render_plan() after a write through .data)
        self.unstaged_cam_near_far = False                  # True: honour cam_near_far when staged=False (the reference ignores it)

    def forward(self, x, d, **kwargs):
        raise NotImplementedError()

    def density(self, x, **kwargs):
        raise NotImplementedError()

    def update_aabb(self, aabb):
        if not torch.is_tensor(aabb):
            aabb = torch.as_tensor(aabb).float()
        self.aabb_train = aabb.clamp(-self.real_bound, self.real_bound).to(self.aabb_train.device)
        self.aabb_infer = self.aabb_train.clone()
        self._plan = None
        print(f"[INFO] update_aabb: {self.aabb_train.cpu().numpy().tolist()}")

    # ---------------------------------------------------------------------------------------
    def render(self, rays_o, rays_d, staged=False, cam_near_far=None, **kwargs):
        if not staged:
            # the reference drops cam_near_far here (renderer.py:187-188: `self.run(rays_o, rays_d, **kwargs)`), so every
            # un-staged call -- all of its training steps -- marches the full aabb interval; same here unless opted in
            if getattr(self, "unstaged_cam_near_far", False):
                return self.run(rays_o, rays_d, cam_near_far=cam_near_far, **kwargs)
            return self.run(rays_o, rays_d, **kwargs)
        # staged inference (renderer.py:185-219): chunks of max_ray_batch, results scattered into place
        N = rays_o.shape[0]
        results: Dict[str, torch.Tensor] = {}
        step = self.opt.max_ray_batch
        for head in range(0, N, step):
            tail = min(head + step, N)
            cnf = cam_near_far if cam_near_far is None or cam_near_far.shape[0] == 1 else cam_near_far[head:tail]
            # (one route for every chunk of the image; a perturbed image is one draw of the jitter tables whatever max_ray_batch is)
            part = self.run(rays_o[head:tail], rays_d[head:tail], cam_near_far=cnf, _image_rays=N, _ray_base=head, _advance=tail == N, **kwargs)
            for k, v in part.items():
                if v is None:
                    continue
                if torch.is_tensor(v):
                    if k not in results:
                        results[k] = torch.empty(N, *v.shape[1:], device=rays_o.device)
                    results[k][head:tail] = v
                else:
                    results[k] = v
        return results

    # ---------------------------------------------------------------------------------------
    def _core_parameters(self):
        for name, p in self.named_parameters():
            if name.startswith(("grid", "view_mlp", "prop_")):
                yield p

    def _needs_field_grad(self, update_proposal: bool) -> bool:
        if not torch.is_grad_enabled():
            return False
        return any(p.requires_grad for p in self._core_parameters())

    def _load_from_state_dict(self, *args, **kwargs):
        # a checkpoint load rewrites tables / aabb in place (same data_ptr): never reuse a plan across it
        self._plan = None
        return super()._load_from_state_dict(*args, **kwargs)

    def invalidate_render_plan(self):
        """Drop the cached fused-render plan (call after writing parameters through `.data`, e.g. an EMA copy_to)."""
        self._plan = None

    def _plan_tensors(self, with_feat: bool):
        encs = [self.grid] + list(getattr(self, "prop_encoders", [])) + ([self.s_grid] if with_feat else [])
        mlps = [self.grid_mlp, self.view_mlp] + list(getattr(self, "prop_mlp", []))
        return [e.embeddings for e in encs] + [lin.weight for m in mlps for lin in m.net]

    def _get_plan(self, with_feat: bool = False):
        """The cached RenderPlan.  The plan holds device pointers into the module's own fp32 tensors (in-place updates
        by an optimiser step / load_state_dict are seen as they are), so it is rebuilt only when a tensor moved
        (data_ptr / device / dtype) or the schedule changed.  What the plan COPIES is refreshed on every call: the aabb
        (host values, memoised on the buffer's version counter) and, with render_table_dtype=float16, the
        half-precision table copies (one conversion pass per render, ~20 us for the main grid; writes through `.data`
        do not bump version counters, so nothing cheaper is safe -- set `render_tables_static = True` for a frozen
        field to skip it)."""
        tensors = self._plan_tensors(with_feat)
        key = (tuple((t.data_ptr(), t.dtype, t.device) for t in tensors), tuple(self.opt.num_steps), self.render_table_dtype,
               with_feat, float(getattr(self.opt, "early_stop_eps", 0.0) or 0.0), bool(getattr(self.opt, "compact_live", False)))
        if self._plan is None or self._plan_key != key:
            self._plan = rm.RenderPlan(self, self.opt.num_steps, self.render_table_dtype,
                                       feat_encoder=self.s_grid if with_feat else None,
                                       early_stop_eps=float(getattr(self.opt, "early_stop_eps", 0.0) or 0.0),
                                       compact_live=bool(getattr(self.opt, "compact_live", False)) and self._fused_kind() == "main")
            self._plan_key = key
        elif not getattr(self, "render_tables_static", False):
            self._plan.refresh_tables()        # (the fp16 range guard is re-checked by render_rays before a final-stage launch)
        self._plan.keep_packs = bool(getattr(self, "render_keep_packs", False)) and not self.training
        ab = rm._host_values(self.aabb_train if self.training else self.aabb_infer)
        for i in range(6):
            self._plan.cfg.aabb[i] = ab[i]
        return self._plan

    # A subclass whose forward() is NOT "grid -> grid_mlp -> [trunc_exp(sigma) | geo_feat], colour = view_mlp(cat(geo_feat, SH(d)))"
    # (network.py:146-186) sets this to False: the fused kernels restate that structure, they do not call forward().
    standard_field = True
    fused_mask_head = True        # inference: sn_rm_mask_head (one kernel); False = the three-kernel route (A/B, tests)
    fused_proposals = True        # training calls whose proposal networks get no gradient run those stages in the fused kernels
    fused_perturb = True          # perturbed calls that need no field gradient take the fused render (False: the operator chain, as before)
    jitter = None                 # Optional[rm.DeviceJitter]: the Philox state of those calls, created on the rays' device at first need.
                                  # Set by the caller, it also feeds the autograd routes (one jitter.tables() call instead of torch.rand)
    fused_min_rays = 16384        # fields of other sizes than the reference network's: batches below this take the operator chain (see run())

    def _fused_shape(self) -> bool:
        """Can sn_rm_render_rays take this field?  Two kernels serve the last stage: the one instantiated for the reference
        network's own sizes (nerf/network.py:93-98, 131-143: L=16 F=2 grid, 32-64-64-16 and 31-32-32-3 bias-free ReLU MLPs) on the
        matrix cores, and a size-agnostic one (k_final_stage_any) for any other field of the same structure -- level_dim 2,
        up to 32 levels' worth of 64 features, bias-free ReLU MLPs of <= 4 layers and <= 64 neurons, <= 31 geometry channels;
        BASELINE configs[0] (L=8 grid, 16-32-16 / 31-32-3 MLPs) is one.  Proposal stages must be the reference's (L=5 F=2 grids,
        10-16-1 MLPs).  Anything else renders through the stage loop over the stand-alone HIP operators (grid_encode, SH,
        sample_pdf, weights, composite); the library itself would answer SN_ERR_UNSUPPORTED."""
        return self._fused_kind() is not None

    def _fused_kind(self):
        def dims(mlp):
            net = list(getattr(mlp, "net", []))
            return [net[0].weight.shape[1]] + [l.weight.shape[0] for l in net] if net and all(l.bias is None for l in net) else None
        try:
            if not self.standard_field:
                return None
            g = self.grid
            if not (g.input_dim == 3 and g.level_dim == 2 and getattr(self.view_encoder, "degree", 0) == 4):
                return None
            n_prop = len(self.opt.num_steps) - 1
            if n_prop > 0:
                encs, mlps = list(self.prop_encoders), list(self.prop_mlp)
                if not (len(encs) >= n_prop and all(
                        e.input_dim == 3 and e.num_levels == 5 and e.level_dim == 2 and e.gridtype_id == 0 and not e.align_corners
                        and e.interp_id == 0 and dims(m) == [10, 16, 1] for e, m in zip(encs[:n_prop], mlps[:n_prop]))):
                    return None
            dg, dv = dims(self.grid_mlp), dims(self.view_mlp)
            if (g.num_levels == 16 and g.gridtype_id == 0 and not g.align_corners and g.interp_id == 0
                    and dg == [32, 64, 64, 16] and dv == [31, 32, 32, 3]):
                return "main"
            from .network import MLP                                                            # network.py:9-29: ReLU between the layers
            relu = all(type(m) is MLP for m in (self.grid_mlp, self.view_mlp))                  # (a subclass may change forward(): exact type)
            if (dg is not None and dv is not None and relu and g.num_levels * 2 <= 64 and len(dg) <= 5 and len(dv) <= 5
                    and max(dg) <= 64 and max(dv) <= 64 and dg[0] == g.num_levels * 2 and 2 <= dg[-1] <= 32
                    and dv[0] == dg[-1] - 1 + 16 and dv[-1] == 3 and getattr(self, "geom_feat_dim", dg[-1] - 1) == dg[-1] - 1):
                return "any"
            return None
        except AttributeError:
            return None

    def _sam_fusable(self) -> bool:
        """f_sam can be accumulated inside the fused render (no graph through s_grid wanted, standard hash grid)."""
        if not self.opt.with_sam or not self.opt.sam_use_view_direction:
            return False
        if torch.is_grad_enabled() and self.s_grid.embeddings.requires_grad:
            return False
        if self._fused_kind() != "main":                    # the in-render feature stage is instantiated next to the reference network's last stage only
            return False
        g = self.s_grid
        return g.gridtype_id == 0 and not g.align_corners and g.interp_id == 0 and g.level_dim in (2, 4, 8)

    def run(self, rays_o, rays_d, bg_color=None, perturb=False, cam_near_far=None, update_proposal=True,
            return_feats=0, return_mask=0, H=None, W=None, tile_w=0, **kwargs):
        if self.opt.render_mesh:
            return {}                                       # the reference's mesh branch is commented out (renderer.py:257,386)
        if bg_color is None:
            bg_color = 1
        kind = self._fused_kind()
        # the size-agnostic last stage gives a ray to one lane for all its samples: below ~16 k rays the chip is mostly idle and the operator
        # chain, which spreads the SAMPLES over the lanes, is faster (configs[0], 4096 rays: 0.63 vs 0.44 ms; 160 000 rays: 1.9 vs 3.2 ms)
        # (single-stage fields only: with proposal stages in front, the chain would also leave THEIR fused kernels)
        if kind == "any" and len(self.opt.num_steps) == 1 and int(kwargs.get("_image_rays", rays_o.shape[0])) < self.fused_min_rays:
            kind = None
        # staged render: chunk [head, tail) of an image draws its jitter rows with ray_base = head and only the last chunk advances the draw
        ray_base, advance = int(kwargs.get("_ray_base", 0)), bool(kwargs.get("_advance", True))
        needs_grad = self._needs_field_grad(update_proposal)
        if perturb and not needs_grad and kind is not None and self.fused_perturb and rays_o.is_cuda:
            # a perturbed render that differentiates nothing in the field (the SAM step's ground-truth image, trainer.py:513; the viewer's
            # supersampling, trainer.py:1308: perturb = spp) is the fused render fed with per-ray jitter tables
            return self._run_fused(rays_o, rays_d, bg_color, cam_near_far, return_feats, return_mask, H, W, tile_w, packed=kwargs.get("packed"),
                                   jitter=self._device_jitter(rays_o.device), ray_base=ray_base, advance=advance)
        if perturb or needs_grad or kind is None:
            return self._run_autograd(rays_o, rays_d, bg_color, perturb, cam_near_far, update_proposal,
                                      return_feats, return_mask, H, W, ray_base=ray_base, advance=advance)
        return self._run_fused(rays_o, rays_d, bg_color, cam_near_far, return_feats, return_mask, H, W, tile_w, packed=kwargs.get("packed"))

    def _device_jitter(self, device, explicit_only: bool = False):
        """The DeviceJitter of this model on `device`.  One that the renderer made itself (seeded from torch's default CPU generator) serves
        the fused perturbed render only: the autograd routes (explicit_only) keep torch.rand unless the caller has set `model.jitter`."""
        j = self.jitter
        if j is not None and j is not getattr(self, "_own_jitter", None):      # the caller's
            if j.device != device:
                raise RuntimeError(f"model.jitter lives on {j.device}, the rays on {device}")
            return j
        if explicit_only:
            return None
        if j is None or j.device != device:
            self.jitter = self._own_jitter = rm.DeviceJitter(device)
        return self.jitter

    # ---------------------------------------------------------------------------------------
    @staticmethod
    def _head_mlp(seq, x):
        """nn.Sequential(SkipConnMLP[, LayerNorm]) of a feature head.  Without autograd (inference) the whole stack is
        one matrix-core kernel (rm.mlp_forward); with autograd it is the torch module."""
        mlp = seq[0]
        ln = seq[1] if len(seq) > 1 else None
        fusable = (not torch.is_grad_enabled() and x.is_cuda and mlp.dim_hidden == 256 and mlp.dim_out <= 256
                   and len(mlp.net) <= 8 and (ln is None or isinstance(ln, torch.nn.LayerNorm)))
        if not fusable:
            return seq(x)
        lead = x.shape[:-1]
        return rm.mlp_forward(x.reshape(-1, x.shape[-1]), mlp, ln).reshape(*lead, -1)

    def _heads(self, results, weights, xyzs, geo_feat, f_image, image, depth, return_feats, return_mask, H, W,
               tile_w=0, f_sam=None, head_input=None):
        opt = self.opt
        if opt.with_sam:                                    # renderer.py:301-302, 359-374
            if head_input is not None:
                pass                                        # cat([f_sam, f_image, image, depth]) was written in place by the fused render
            elif f_sam is not None:
                pass                                        # accumulated inside the fused render (feature stage)
            elif torch.is_grad_enabled() and any(t.requires_grad for t in (self.s_grid.embeddings, weights, xyzs)):
                features = self.s_grid(xyzs, bound=self.bound)
                f_sam = rm.composite(weights, features)
            else:   # inference: one kernel, no [N*T, 128] intermediate
                f_sam = rm.grid_composite(weights, xyzs, self.s_grid, self.bound, tile_w=tile_w)
            if head_input is not None:
                f = head_input
            elif opt.sam_use_view_direction:
                f = torch.cat([f_sam, f_image, image, depth.unsqueeze(-1)], dim=-1)
            else:
                f = torch.cat([f_sam, rm.composite(weights, geo_feat), image, depth.unsqueeze(-1)], dim=-1)
            samvit = self._head_mlp(self.samvit_mlp, f)
            if return_feats > 0:
                results["samvit"] = samvit.view(H, W, -1)
        if return_mask > 0:                                 # renderer.py:304-305, 376-385
            if opt.mask_mlp_type == "default":
                mlp = self.mask_mlp[0]
                if (not torch.is_grad_enabled() and weights.is_cuda and len(self.mask_mlp) == 1
                        and rm.mask_head_fusable(self.m_grid, mlp, weights.shape[1], geo_feat.shape[-1])
                        and self.fused_mask_head):
                    # inference: grid gather -> matrix-core MLP -> compositing in one kernel, nothing per-sample written
                    results["instance_mask_logits"] = rm.mask_head(weights, xyzs, geo_feat, self.m_grid, mlp, self.bound)
                    return
                # features and (detached) geometry channels land in one [.., 143] buffer in a single pass; in training the table gets its gradient
                # through ops._grid_encode_cat (the reference: torch.cat([m_grid(xyzs), geo_feat.detach()]), renderer.py:380)
                mlp_in = self.m_grid.forward_cat(xyzs.detach(), geo_feat, bound=self.bound)
                point_masks = self._head_mlp(self.mask_mlp, mlp_in)
            else:
                raise RuntimeError("mask_mlp_type='lightweight_mask' is dimensionally inconsistent in the reference "
                                   "(renderer.py:381 feeds 63 features into a 35-input MLP, network.py:128)")
            results["instance_mask_logits"] = rm.composite(weights.detach(), point_masks)

    def _run_fused(self, rays_o, rays_d, bg_color, cam_near_far, return_feats, return_mask, H, W, tile_w, packed=None,
                   jitter=None, ray_base=0, advance=True):
        """packed: optional [N, >=5] buffer that receives rgb | depth | weights_sum in place (rm.render_rays; the all-gather payload of dist.py);
        only with a scalar background (a tensor background is added after the kernel, renderer.py:353).
        jitter: a DeviceJitter = perturb: every stage samples at per-ray jittered positions (renderer.py:262-270, 97-102), the tables of rays
        ray_base .. ray_base + N - 1 written by one launch."""
        opt = self.opt
        need_heads = opt.with_sam or return_mask > 0
        fused_sam = self._sam_fusable()
        need_samples = return_mask > 0 or (opt.with_sam and not fused_sam)      # per-sample tensors for the torch heads
        want = []
        if opt.with_sam:
            want.append("f_image")
        if need_samples:
            want += ["weights_last", "xyzs_last"]
        if return_mask > 0 or (opt.with_sam and not opt.sam_use_view_direction):
            want.append("geo_feat_last")                    # [N,T,15] per-sample features
        plan = self._get_plan(with_feat=fused_sam)
        bg = float(bg_color) if not torch.is_tensor(bg_color) else 0.0
        # the SAM head's MLP input [N, 163] = f_sam | f_image | image | depth written in place by the kernels (no torch.cat, renderer.py:366);
        # a tensor background is blended after the kernel, so the image columns would be stale: that case keeps the concatenation
        head_in = fused_sam and opt.sam_use_view_direction and not torch.is_tensor(bg_color)
        with torch.no_grad():
            b0 = u_tabs = None
            if jitter is not None:
                b0, u_tabs = jitter.tables(rays_o.reshape(-1, 3).shape[0], list(opt.num_steps), ray_base=ray_base, advance=advance)
            out = rm.render_rays(plan, rays_o, rays_d, cam_near_far=cam_near_far, bg_color=bg, tile_w=tile_w, want=want,
                                 packed=None if torch.is_tensor(bg_color) else packed, head_input=head_in, bins0_table=b0, u_tables=u_tabs)
            image = out["image"]
            if torch.is_tensor(bg_color):                   # per-ray / rgb background (renderer.py:353)
                image = image + (1 - out["weights_sum"]).unsqueeze(-1) * bg_color
        results = {"weights_sum": out["weights_sum"], "depth": out["depth"], "image": image}
        if need_heads:
            self._heads(results, out.get("weights_last"), out.get("xyzs_last"), out.get("geo_feat_last"), out.get("f_image"),
                        image, out["depth"], return_feats, return_mask, H, W, tile_w=tile_w or 0, f_sam=out.get("f_feat"),
                        head_input=out.get("head_input") if head_in else None)
        return results

    # ---------------------------------------------------------------------------------------
    fused_point_labels = True     # render_object: per-sample labels from sn_rm_mask_point_labels (False: the operator chain, A/B and tests)

    def render_object(self, rays_o, rays_d, instance_ids, invert=False, staged=False, cam_near_far=None, bg_color=None, H=None, W=None):
        """Render the object that the mask field assigns to `instance_ids` alone -- or, with invert=True, the scene without it.
        (The reference names this, main.py:183-185 --render_mesh / --render_mask_instance_id and trainer.py:711-713 outputs['mesh_image'],
        and leaves it commented out; the definition is this project's: include/sanerf_hip.h, tests/object_ref64.py.)

        Only the LAST stage is gated: the samples are exactly those of render(..., return_mask=1).  Each gets the label argmax_k
        mask_mlp(cat[m_grid(x), geo_feat]) (lowest index on a tie); the samples whose label is in `instance_ids` (xor invert) keep their
        density, the others get none, and the ray is integrated again.  Returns image / depth / weights_sum of the full scene (free, from the
        same call) and object_image / object_depth / object_weights_sum; mesh_image is object_image.  No-grad only; nothing is read back
        to the host, so a warmed-up call can be captured as a HIP graph.  staged=True: chunks of opt.max_ray_batch, same bits."""
        if self._needs_field_grad(True) or (torch.is_grad_enabled() and any(p.requires_grad for m in (self.m_grid, self.mask_mlp) for p in m.parameters())):
            raise RuntimeError("render_object is an inference render: call it under torch.no_grad() (or on a frozen field)")
        keep = rm.keep_mask_of(instance_ids)
        rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
        N = rays_o.shape[0]
        bg_color = 1 if bg_color is None else bg_color
        per_ray_bg = torch.is_tensor(bg_color) and bg_color.dim() == 2 and bg_color.shape[0] == N and N > 1
        with torch.no_grad():
            if not staged:
                cnf = cam_near_far if getattr(self, "unstaged_cam_near_far", False) else None     # (as render(): the reference drops it here)
                res = self._run_object(rays_o, rays_d, keep, bool(invert), cnf, bg_color)
            else:
                res: Dict[str, torch.Tensor] = {}
                step = self.opt.max_ray_batch
                for head in range(0, N, step):
                    tail = min(head + step, N)
                    cnf = cam_near_far if cam_near_far is None or cam_near_far.shape[0] == 1 else cam_near_far[head:tail]
                    part = self._run_object(rays_o[head:tail], rays_d[head:tail], keep, bool(invert), cnf,
                                            bg_color[head:tail] if per_ray_bg else bg_color)
                    for k, v in part.items():
                        if k not in res:
                            res[k] = torch.empty(N, *v.shape[1:], device=v.device, dtype=v.dtype)
                        res[k][head:tail] = v
        res["mesh_image"] = res["object_image"]             # the key the reference's test_step reads (trainer.py:711-713)
        return res

    def _point_labels(self, live, xyzs, geo_feat, want_logits=False):
        """label = argmax_k mask_mlp(cat[m_grid(x), geo_feat]) per sample, uint8 [N,T]: one kernel where sn_rm_mask_point_labels takes the head
        (255 on the tiles it skips, where live == 0 throughout), else m_grid.forward_cat -> the matrix-core MLP -> argmax."""
        if self.opt.mask_mlp_type != "default":
            raise RuntimeError("render_object needs mask_mlp_type='default' (see _heads)")
        mlp = self.mask_mlp[0]
        if (self.fused_point_labels and live.is_cuda and len(self.mask_mlp) == 1
                and rm.mask_point_labels_fusable(self.m_grid, mlp, live.shape[1], geo_feat.shape[-1])):
            return rm.mask_point_labels(live, xyzs, geo_feat, self.m_grid, mlp, self.bound, want_logits=want_logits)
        logits = self._head_mlp(self.mask_mlp, self.m_grid.forward_cat(xyzs, geo_feat, bound=self.bound))
        if logits.shape[-1] > 32:
            raise RuntimeError(f"render_object: at most 32 instances (the mask field has {logits.shape[-1]})")
        labels = torch.argmax(logits, dim=-1).to(torch.uint8)
        return (labels, logits) if want_logits else labels

    def _object_samples(self, rays_o, rays_d, cam_near_far, bg_color):
        """The full-scene render and the last stage's samples: (results, sigmas [N,T], real_bins [N,T+1], xyzs [N,T,3], geo_feat [N,T,15])."""
        opt = self.opt
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        if self._fused_kind() is not None and rays_o.is_cuda:
            bg = float(bg_color) if not torch.is_tensor(bg_color) else 0.0
            out = rm.render_rays(self._get_plan(), rays_o, rays_d, cam_near_far=cam_near_far, bg_color=bg,
                                 want=["xyzs_last", "geo_feat_last", "sigmas_last", "bins_last"])
            last = len(opt.num_steps) - 1
            image = out["image"]
            if torch.is_tensor(bg_color):                   # per-ray / rgb background (renderer.py:353)
                image = image + (1 - out["weights_sum"]).unsqueeze(-1) * bg_color
            results = {"image": image, "depth": out["depth"], "weights_sum": out["weights_sum"]}
            # real bin edges from the existing sample_positions arithmetic (the fused render's own real_bin)
            nears, fars = rm.near_far_from_aabb(rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer, self.min_near)
            if cam_near_far is not None:
                nears = torch.maximum(nears, cam_near_far[:, [0]])
                fars = torch.minimum(fars, cam_near_far[:, [1]])
            real_bins = rm.sample_positions(rays_o, rays_d, nears, fars, out[f"bins{last}"], contract=opt.contract)[0]
            return results, out[f"sigmas{last}"], real_bins, out["xyzs_last"], out["geo_feat_last"]
        samples: dict = {}
        results = self._run_autograd(rays_o, rays_d, bg_color, False, cam_near_far, False, 0, 0, None, None, samples=samples)
        return ({k: results[k] for k in ("image", "depth", "weights_sum")}, samples["sigmas"], samples["real_bins"], samples["xyzs"],
                samples["geo_feat"])

    def _run_object(self, rays_o, rays_d, keep_mask, invert, cam_near_far, bg_color):
        last_opaque = self.opt.background == "last_sample"
        results, sigmas, real_bins, xyzs, geo_feat = self._object_samples(rays_o, rays_d, cam_near_far, bg_color)
        # which samples can matter at all: y = delta * sigma != 0 (not "weight != 0": a sample behind a gated-away occluder has weight 0)
        live = (real_bins[:, 1:] - real_bins[:, :-1]) * sigmas
        if last_opaque:
            live[:, -1] = 1.0                               # the last sample is opaque whenever it is kept, whatever its density
        labels = self._point_labels(live, xyzs, geo_feat)
        wsum, depth, f_image = rm.object_composite(labels, sigmas, real_bins, geo_feat, rays_d, keep_mask, invert, last_opaque)
        image = self.view_mlp.forward_sigmoid_bg(f_image, wsum, float(bg_color) if not torch.is_tensor(bg_color) else 0.0)
        if torch.is_tensor(bg_color):
            image = image + (1 - wsum).unsqueeze(-1) * bg_color
        results.update(object_image=image, object_depth=depth, object_weights_sum=wsum)
        return results

    # ---------------------------------------------------------------------------------------
    # Geometry export: the density of the main field on a world-space lattice, and its isosurface as a triangle mesh.  (The reference offers
    # --render_mesh / --density_thresh, imports mcubes and trimesh, and calls neither; this is the project's own definition:
    # include/sanerf_hip.h, tests/mesh_ref.py.)
    def _inference_only(self, what: str):
        if self._needs_field_grad(True) or (torch.is_grad_enabled() and self.opt.with_mask
                                            and any(p.requires_grad for m in (self.m_grid, self.mask_mlp) for p in m.parameters())):
            raise RuntimeError(f"{what} is an inference query: call it under torch.no_grad() (or on a frozen field)")

    @staticmethod
    def _lattice(resolution, aabb):
        """((nx, ny, nz), origin, step) of a lattice with its first and last vertices on the faces of aabb; origin and step as the fp32
        values the kernels receive."""
        import numpy as np
        res = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
        if len(res) != 3 or min(res) < 2:
            raise ValueError(f"resolution must be an int or a triple, every entry >= 2 (got {resolution})")
        box = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0] if aabb is None else [float(v) for v in (aabb.tolist() if torch.is_tensor(aabb) else aabb)]
        if len(box) != 6:
            raise ValueError("aabb must be [xmin, ymin, zmin, xmax, ymax, zmax]")
        origin = [float(np.float32(box[a])) for a in range(3)]
        step = [float(np.float32((box[3 + a] - box[a]) / (res[a] - 1))) for a in range(3)]
        return res, origin, step

    def density_volume(self, resolution, aabb=None, instance_ids=None, invert=False, chunk=1 << 20):
        """sigma of the main field on a world-space lattice: [nx,ny,nz] fp32 (z fastest), vertex i at aabb_min + i * step per axis.
        resolution: an int or a triple; aabb: default [-1,1]^3, the region the contraction leaves alone (positions outside it are contracted
        when opt.contract is set).  With instance_ids, sigma is kept where the mask field's label -- _point_labels, the kernels of
        render_object -- is in the set, xor invert, and is 0 elsewhere.  Works in chunks of `chunk` lattice vertices (positions from
        raymarching.lattice_points, no meshgrid); the result does not depend on chunk.  No-grad only."""
        self._inference_only("density_volume")
        res, origin, step = self._lattice(resolution, aabb)
        total = res[0] * res[1] * res[2]
        chunk = max(int(chunk), 1)
        device = self.aabb_train.device
        lut = None
        if instance_ids is not None:
            if not self.opt.with_mask:
                raise RuntimeError("density_volume: instance_ids need the mask field (opt.with_mask)")
            keep = rm.keep_mask_of(instance_ids)
            lut = torch.tensor([i < 32 and bool((keep >> i) & 1) for i in range(256)], device=device) ^ bool(invert)
        volume = torch.empty(total, device=device, dtype=torch.float32)
        with torch.no_grad():
            for first in range(0, total, chunk):
                count = min(chunk, total - first)
                xyz = rm.lattice_points(origin, step, res, first, count, contract=bool(self.opt.contract), device=device)
                out = self.density(xyz)
                sigma = out["sigma"].reshape(-1).float()
                if lut is not None:
                    # the label kernel takes [rays, samples] with at least 4 samples a ray: rows of 4 lattice vertices, the last one padded
                    pad = (-count) % 4
                    geo = out["geo_feat"]
                    if pad:
                        xyz = torch.cat([xyz, xyz.new_zeros(pad, 3)])
                        geo = torch.cat([geo, geo.new_zeros(pad, geo.shape[-1])])
                    live = torch.cat([sigma, sigma.new_zeros(pad)]) if pad else sigma
                    labels = self._point_labels(live.reshape(-1, 4), xyz.reshape(-1, 4, 3), geo.reshape(-1, 4, geo.shape[-1]).contiguous())
                    sigma = torch.where(lut[labels.reshape(-1)[:count].long()], sigma, torch.zeros_like(sigma))
                volume[first:first + count] = sigma
        return volume.reshape(res)

    def vertex_attributes(self, mesh, probe_step, samples=8, instance_ids=None, invert=False, labels=False, chunk=1 << 17):
        """Colour, coverage and instance label of every vertex of a mesh (the keys of extract_mesh; needs mesh["normals"]): each vertex is
        shaded the way a pixel is, by a short ray of `samples` = K in {4, 8, 16, 32} samples, `probe_step` = h apart, that enters the
        surface head-on (d = -normal) and is composited and normalised -- include/sanerf_hip.h states the definition,
        tests/mesh_attr_ref64.py its fp64 twin.  With instance_ids only the samples whose mask-field label is in the set (xor invert) are
        integrated; with labels=True each vertex also gets the id that holds most of its weight (255: none).

        Returns {"colors" [V,3] f32 in [0,1], "coverage" [V] f32 (the probe's alpha: near 0 where nothing kept was hit, and the colour is
        then that of the plain mean of the probe's geometry), "labels" [V] uint8 or None}.  Works in chunks of `chunk` vertices -- probe
        points -> density -> _point_labels (when asked for) -> composite -> colour head; the result does not depend on chunk.  No-grad
        only; nothing is read back to the host."""
        self._inference_only("vertex_attributes")
        if mesh.get("normals") is None:
            raise ValueError("vertex_attributes: the probes need mesh['normals'] (extract_mesh(normals=True))")
        K = int(samples)
        h = float(probe_step)
        if K not in rm.PROBE_SAMPLES:
            raise ValueError(f"vertex_attributes: samples = {K} must be one of {rm.PROBE_SAMPLES}")
        if not (0.0 < h < float("inf")):
            raise ValueError(f"vertex_attributes: probe_step = {h} must be positive and finite")
        gated = instance_ids is not None
        if (gated or labels) and not self.opt.with_mask:
            raise RuntimeError("vertex_attributes: labels and instance_ids need the mask field (opt.with_mask)")
        keep = rm.keep_mask_of(instance_ids) if gated else 0xFFFFFFFF
        vertices, normals = mesh["vertices"], mesh["normals"]
        V, device = vertices.shape[0], vertices.device
        chunk = max(int(chunk), 1)
        colors = torch.empty(V, 3, device=device, dtype=torch.float32)
        coverage = torch.empty(V, device=device, dtype=torch.float32)
        vlabels = torch.empty(V, device=device, dtype=torch.uint8) if labels else None
        with torch.no_grad():
            for first in range(0, V, chunk):
                count = min(chunk, V - first)
                xyz, dirs = rm.vertex_probe_points(vertices, normals, K, h, first, count, contract=bool(self.opt.contract))
                out = self.density(xyz.reshape(-1, 3))
                sigma = out["sigma"].reshape(count, K).float()
                geo = out["geo_feat"].reshape(count, K, -1).contiguous()
                lab = self._point_labels(sigma, xyz, geo) if (gated or labels) else None
                f, cov, vl = rm.vertex_probe_composite(sigma, geo, dirs, h, lab, keep, gated and bool(invert), want_labels=bool(labels))
                colors[first:first + count] = self.view_mlp.forward_sigmoid_bg(f, torch.ones_like(cov), 0.0)
                coverage[first:first + count] = cov
                if labels:
                    vlabels[first:first + count] = vl
        return {"colors": colors, "coverage": coverage, "labels": vlabels}

    def extract_mesh(self, resolution=256, threshold=None, aabb=None, instance_ids=None, invert=False, normals=True,
                     min_component_triangles=0, keep_largest=0, simplify=0, vertex_colors=False, vertex_labels=False, probe_samples=8,
                     probe_step=0.5, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53, smooth_pin_open=True):
        """The surface sigma = threshold (default self.density_thresh) of density_volume(resolution, aabb, instance_ids, invert) by marching
        tetrahedra on the device: {"vertices" [V,3] f32, "normals" [V,3] f32 or None, "triangles" [T,3] int32} in world coordinates -- the
        whole scene, or with instance_ids the object alone (invert: the scene without it).  The size of the result depends on the data
        (raymarching.isosurface reads two totals back once).  nerf.utils.save_mesh writes it as a PLY file.

        min_component_triangles, keep_largest (both 0: everything above the threshold, floaters included): the mesh then goes through
        raymarching.mesh_clean, which keeps the connected components of at least that many triangles and / or the k largest.

        simplify = k >= 1 (fractional allowed; 0: off, and nothing is launched for it): after the clean-up the mesh goes through
        raymarching.mesh_simplify -- uniform vertex clustering -- with cells of k lattice steps that are aligned with the extraction's own
        lattice (cell = k step, origin = lattice origin - step / 2, dims covering the lattice), so the result does not depend on where
        the object sits in its bounding box.  Clustering does not preserve manifoldness.

        smooth = N >= 1 iterations (0: off, nothing is launched for it, and the result is the same bits as without the parameter): after
        clean-up and simplification the mesh goes through raymarching.mesh_smooth -- Taubin smoothing in fixed point with smooth_lambda and
        smooth_mu (mu = 0: plain Laplacian), vertices on open edges pinned with smooth_pin_open -- quantised over the extraction lattice's
        own box (raymarching.smooth_quantisation), so the result does not depend on where the object sits and nothing is read back.  With
        normals=True the result's normals are then the geometric ones of the smoothed triangles, and the probes below enter along them.

        vertex_colors, vertex_labels (both False: nothing is launched for them and the dict has the three keys above; either needs
        normals=True): the FINAL mesh -- after clean-up, simplification and smoothing -- goes through vertex_attributes with probe_samples samples
        probe_step lattice steps apart (h = probe_step min(step)) and the same instance_ids / invert, and the dict gains "colors" [V,3]
        and "coverage" [V] (vertex_colors) and "labels" [V] uint8 (vertex_labels).  save_mesh writes both."""
        simplify = float(simplify)
        if simplify != 0.0 and not (1.0 <= simplify < float("inf")):
            raise ValueError(f"extract_mesh: simplify = {simplify} must be 0 (off) or at least 1 lattice step")
        smooth = rm.mesh._smooth_iterations(smooth, "extract_mesh: smooth")
        if smooth:
            rm.mesh._smooth_factors(smooth_lambda, smooth_mu, "extract_mesh")
        res, origin, step = self._lattice(resolution, aabb)
        attributes = bool(vertex_colors) or bool(vertex_labels)
        if attributes:
            if not normals:
                raise ValueError("extract_mesh: vertex_colors / vertex_labels need normals=True (the probes enter along the normal)")
            if int(probe_samples) not in rm.PROBE_SAMPLES:
                raise ValueError(f"extract_mesh: probe_samples = {probe_samples} must be one of {rm.PROBE_SAMPLES}")
            probe_h = float(probe_step) * min(abs(v) for v in step)
            if not (0.0 < probe_h < float("inf")):
                raise ValueError(f"extract_mesh: probe_step = {probe_step} must be positive and finite")
            if vertex_labels and not self.opt.with_mask:
                raise RuntimeError("extract_mesh: vertex_labels need the mask field (opt.with_mask)")
        volume = self.density_volume(res, aabb, instance_ids, invert)
        iso = float(self.density_thresh if threshold is None else threshold)
        mesh = rm.isosurface(volume, iso, origin, step, normals=normals)
        if min_component_triangles or keep_largest:
            mesh = rm.mesh_clean(mesh, min_triangles=min_component_triangles, keep_largest=keep_largest)
        if simplify:
            import numpy as np
            mesh = rm.mesh_simplify(mesh, cell=[float(np.float32(simplify * step[a])) for a in range(3)],
                                    origin=[float(np.float32(origin[a]) - np.float32(0.5) * np.float32(step[a])) for a in range(3)],
                                    dims=[int((res[a] - 0.5) // simplify) + 2 for a in range(3)])     # one spare cell for the rounding of the last vertex
        if smooth:
            quant = rm.smooth_quantisation(origin, [origin[a] + (res[a] - 1) * step[a] for a in range(3)])       # the lattice's box, in fp64
            if quant is None:
                raise ValueError("extract_mesh: smooth needs a lattice box of positive, finite extent")
            mesh = rm.mesh_smooth(mesh, smooth, smooth_lambda, smooth_mu, smooth_pin_open, origin=quant[0], quantum=quant[1], normals=bool(normals))
        if attributes:
            attr = self.vertex_attributes(mesh, probe_h, samples=int(probe_samples), instance_ids=instance_ids, invert=invert,
                                          labels=bool(vertex_labels))
            mesh = dict(mesh)
            if vertex_colors:
                mesh["colors"], mesh["coverage"] = attr["colors"], attr["coverage"]
            if vertex_labels:
                mesh["labels"] = attr["labels"]
        return mesh

    def extract_object_meshes(self, instance_ids=None, part_min_triangles=0, part_keep_largest=0, **extract_mesh_kwargs):
        """Every segmented object as a mesh of its own, {instance id: mesh}, from ONE pass of the density lattice: one
        extract_mesh(vertex_labels=True, **extract_mesh_kwargs) of the scene, then raymarching.mesh_split by the vertex labels -- instead of
        one extract_mesh(instance_ids=[k]) per object, each of which sends the whole lattice through the field and the mask head.  Each
        mesh has the keys of extract_mesh, "labels" included and "colors" / "coverage" with vertex_colors=True, gathered from the scene
        mesh; indices are local, so each goes to nerf.utils.save_mesh as it is (save_meshes writes them all).

        instance_ids: which parts to return (default: every non-empty part below 32).  Part 32 -- the vertices whose label is no
        instance, 255 = "none" among them -- is returned only when 32 is asked for; an id that has no triangle is absent from the result.
        part_min_triangles, part_keep_largest (both 0: off): each part then goes through raymarching.mesh_clean with these, which drops
        the specks that label noise leaves in a part; a part that is emptied is still returned, with 0 triangles.

        The split sends a seam triangle whole to one part, so objects are open shells where they met a neighbour, unlike the closed
        surface that extract_mesh(instance_ids=[k]) cuts from the gated density.  Needs opt.with_mask and normals=True.  No-grad only."""
        self._inference_only("extract_object_meshes")
        if "vertex_labels" in extract_mesh_kwargs:
            raise ValueError("extract_object_meshes: vertex_labels is always on")
        if not extract_mesh_kwargs.get("normals", True):
            raise ValueError("extract_object_meshes: the vertex labels need normals=True (the probes enter along the normal)")
        if not self.opt.with_mask:
            raise RuntimeError("extract_object_meshes: the vertex labels need the mask field (opt.with_mask)")
        part_min_triangles, part_keep_largest = int(part_min_triangles), int(part_keep_largest)
        if part_min_triangles < 0 or part_keep_largest < 0:
            raise ValueError("extract_object_meshes: part_min_triangles and part_keep_largest must not be negative")
        if instance_ids is not None:
            instance_ids = sorted({int(i) for i in instance_ids})
            if any(i < 0 or i >= rm.MESH_SPLIT_PARTS for i in instance_ids):
                raise ValueError(f"extract_object_meshes: instance ids are 0 .. {rm.MESH_SPLIT_PARTS - 1}, got {instance_ids}")
        with torch.no_grad():
            scene = self.extract_mesh(vertex_labels=True, **extract_mesh_kwargs)
            parts = rm.mesh_split(scene)["parts"]
            wanted = [p for p in parts if p < rm.MESH_SPLIT_PARTS - 1] if instance_ids is None else [p for p in instance_ids if p in parts]
            out = {}
            for p in wanted:
                part = parts[p]
                if part_min_triangles or part_keep_largest:
                    kept = rm.mesh_clean(part, min_triangles=part_min_triangles, keep_largest=part_keep_largest, return_source=True)
                    rows = kept.pop("source_vertex").long()
                    kept.update({k: part[k][rows] for k in rm.mesh._CARRIED if k in part})
                    part = kept
                out[p] = part
        return out

    def render_mesh(self, mesh, pose, intrinsics, H, W, cull=False, bg_color=1):
        """The image of an extracted mesh from one camera: raymarching.mesh_rasterize of `mesh` (what extract_mesh returns, with its "colors" and
        "labels" where it has them) for pose [4,4] and intrinsics [4] in get_rays' convention, with near = opt.min_near -- the plane at which
        the field's rays start.  Returns "triangle_id", "depth", "mask" [H,W], "counts" [4] and, with the attribute, "image" [H,W,3] and
        "label" [H,W].  (The geometry image that the reference's commented-out --render_mesh branch announced.)  No-grad only; nothing is
        read back, and with pose and intrinsics as fp32 device tensors a warmed-up call can be captured as a HIP graph and replayed with a
        new camera written into them.

        Beside the field's renders of the same camera (rays from get_rays(pose, intrinsics, H, W), results reshaped to [H,W]):
        "depth" is the camera-space -z of the surface and so is render()'s "depth" (get_rays' directions are not normalised; their -z
        component is 1): where the surface is opaque and "mask" is 1 the two agree to the lattice step of the extraction, and "depth" is 0
        where the mesh is not seen.  "mask" is the silhouette: set it beside render()'s or render_object()'s "weights_sum" /
        "object_weights_sum" > 0.5 -- of the object's mesh (instance_ids) beside render_object() with the same ids."""
        self._inference_only("render_mesh")
        with torch.no_grad():
            return rm.mesh_rasterize(mesh, pose, intrinsics, H, W, near=self.min_near, cull=cull, bg_color=float(bg_color))

    def render_mesh_clip(self, mesh, pose, intrinsics, H, W, cull=False, bg_color=1):
        """render_mesh() for a camera inside the mesh -- a training view of a scene mesh: raymarching.mesh_rasterize_clip, which cuts the
        triangles that cross the plane z = opt.min_near there instead of dropping them, so a floor or a wall that passes the camera ends
        where the field's render() of that camera starts.  The same arguments and outputs, and "clip_counts" [2]: the triangles that were
        cut and their drawn pieces.  A mesh wholly in front of the plane gives render_mesh()'s bits."""
        self._inference_only("render_mesh_clip")
        with torch.no_grad():
            return rm.mesh_rasterize_clip(mesh, pose, intrinsics, H, W, near=self.min_near, cull=cull, bg_color=float(bg_color))

    # ---------------------------------------------------------------------------------------
    fused_training_ops = True    # RGB-mode training: unit-cube positions, fused small MLPs, one-kernel per-ray head (False: the operator chain)

    def _unit_path_ok(self, rays_o, bg_color, return_mask) -> bool:
        """The training route built from the fused training operators (_run_autograd_unit): the reference network's own field
        (raw = [sigma_raw | 15 geometry channels], degree-4 SH, scalar background) without feature heads."""
        opt = self.opt
        return (self.fused_training_ops and rays_o.is_cuda and not torch.is_tensor(bg_color) and not opt.with_sam and not return_mask > 0
                and self._fused_kind() == "main" and hasattr(self, "field_unit") and hasattr(self, "density_unit")
                and max(opt.num_steps) <= rm.WEIGHTS_BACKWARD_MAX_T and not torch.is_autocast_enabled())

    def _run_autograd_unit(self, rays_o, rays_d, bg_color, perturb, cam_near_far, update_proposal, ray_base=0, advance=True):
        """renderer.py:261-357 for RGB-mode training out of the fused training operators: per stage one geometry kernel that emits the grid
        encoder's unit-cube coordinates, grid_encode, ONE kernel for the stage's perceptron (trunc_exp folded in), one for sigma -> weights;
        then one kernel for weights_sum / depth / f_image (SH once per ray) and one for view_mlp + sigmoid + background.  All jitter comes from
        ONE torch.rand call.  Same results as _run_autograd up to fp32 round-off (tests/test_gpu_train_ops.py)."""
        opt = self.opt
        rays_o = rays_o.contiguous()
        rays_d = rays_d.contiguous()
        N = rays_o.shape[0]
        device = rays_o.device
        steps = list(opt.num_steps)
        nears, fars = rm.near_far_from_aabb(rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer, self.min_near)
        if cam_near_far is not None:
            nears = torch.maximum(nears, cam_near_far[:, [0]])
            fars = torch.minimum(fars, cam_near_far[:, [1]])
        jit = self._device_jitter(device, explicit_only=True) if perturb else None      # the caller's model.jitter, if set
        rand = torch.rand(N * sum(T + 1 for T in steps), device=device) if perturb and jit is None else None
        cursor = [0]

        def draw(T1):                                       # the next N*T1 uniform numbers (contiguous), or None
            if rand is None:
                return None
            r = rand[cursor[0]:cursor[0] + N * T1]
            cursor[0] += N * T1
            return r

        if jit is not None:                                 # every stage's table from one launch instead of torch.rand + a jitter launch per stage
            jb0, ju = jit.tables(N, steps, ray_base=ray_base, advance=advance)

        def table(k):                                       # stage k's perturbed bins (k = 0) / sample_pdf u (k >= 1); the plain bins without perturb
            if jit is not None:
                return jb0 if k == 0 else ju[k]
            return rm.jitter(draw(steps[k] + 1), N, steps[k] + 1, 0 if k == 0 else 1, device=device)

        prop_needs_grad = update_proposal and torch.is_grad_enabled() and any(
            p.requires_grad for m in (list(self.prop_encoders) + list(self.prop_mlp)) for p in m.parameters())
        wants_prop_loss = self.training and opt.lambda_proposal > 0 and update_proposal
        all_bins, all_weights = [], []
        bins = weights = None
        first_stage = 0
        if len(steps) > 1 and not prop_needs_grad and not wants_prop_loss and self.fused_proposals:
            # proposal stages that receive no gradient: the fused inference kernels on the same jitter (see _run_autograd)
            if perturb:
                b0 = table(0)
                u_tabs = {k: table(k) for k in range(1, len(steps))}
            else:
                b0, u_tabs = torch.linspace(0, 1, steps[0] + 1, device=device), None
            with torch.no_grad():
                got = rm.render_rays(self._get_plan(), rays_o, rays_d, cam_near_far=cam_near_far, bins0_table=b0, u_tables=u_tabs,
                                     skip_final=True, out={})
            bins = got[f"bins{len(steps) - 1}"]
            first_stage = len(steps) - 1
        last = len(steps) - 1
        raw = rays_t = None
        for k, T in enumerate(steps):
            if k < first_stage:
                continue
            if k == first_stage and first_stage > 0:
                pass
            elif k == 0:
                bins = table(0)
            elif perturb:
                bins = rm.sample_pdf(bins, weights, T + 1, False, u=table(k))
            else:
                bins = rm.sample_pdf(bins, weights, T + 1, False)
            real_bins, rays_t, x01 = rm.sample_positions(rays_o, rays_d, nears, fars, bins, contract=opt.contract, grid_bound=float(self.bound))
            if k != last:
                with torch.set_grad_enabled(update_proposal and torch.is_grad_enabled()):
                    sigmas = self.density_unit(x01, k)
            else:
                sigmas, raw = self.field_unit(x01)
            weights = rm.weights_from_sigma(real_bins, sigmas, opt.background == "last_sample")
            if self.training:
                all_bins.append(bins)
                all_weights.append(weights)
        weights_sum, depth, f_image = rm.ray_composite(weights, rays_t, raw, rays_d)
        image = self.view_mlp.forward_sigmoid_bg(f_image, weights_sum, float(bg_color))
        results = {}
        if self.training and not opt.with_mask:
            results["num_points"] = N * steps[-1]
            results["weights"] = weights
            if opt.lambda_proposal > 0 and update_proposal:
                results["proposal_loss"] = proposal_loss(all_bins, all_weights)
            if opt.lambda_distort > 0:
                results["distort_loss"] = distort_loss(bins, weights)
        results["weights_sum"] = weights_sum
        results["depth"] = depth
        results["image"] = image
        return results

    def _run_autograd(self, rays_o, rays_d, bg_color, perturb, cam_near_far, update_proposal,
                      return_feats, return_mask, H, W, ray_base=0, advance=True, samples=None):
        """The stage loop of renderer.py:261-357 in torch autograd over the HIP encoders.
        samples: a dict that receives the last stage's sigmas, real_bins, xyzs and geo_feat (render_object on a field the fused render does not take)."""
        if samples is None and self._unit_path_ok(rays_o, bg_color, return_mask):
            return self._run_autograd_unit(rays_o, rays_d, bg_color, perturb, cam_near_far, update_proposal, ray_base=ray_base, advance=advance)
        opt = self.opt
        rays_o = rays_o.contiguous()
        rays_d = rays_d.contiguous()
        N = rays_o.shape[0]
        device = rays_o.device
        nears, fars = rm.near_far_from_aabb(rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer, self.min_near)
        if cam_near_far is not None:
            nears = torch.maximum(nears, cam_near_far[:, [0]])
            fars = torch.minimum(fars, cam_near_far[:, [1]])

        all_bins, all_weights = [], []
        steps = opt.num_steps
        bins = weights = None
        # Proposal networks that receive no gradient in this call (trainer.py:372-373: after step 3000 they are updated on every
        # 5th step only; mask / SAM training never updates them) are pure inference: their stages run in the fused kernels --
        # per-ray perturbed bins and u as inputs, exactly the reference's jitter (renderer.py:101-102, 267-270) -- and only the
        # last stage, which carries the gradients, goes through the autograd operators below.
        prop_needs_grad = update_proposal and torch.is_grad_enabled() and any(
            p.requires_grad for m in (list(getattr(self, "prop_encoders", [])) + list(getattr(self, "prop_mlp", []))) for p in m.parameters())
        wants_prop_loss = self.training and not opt.with_mask and not opt.with_sam and opt.lambda_proposal > 0 and update_proposal
        first_stage = 0
        # the caller's model.jitter, if set: every stage's table from one launch (the same tables as the fused perturbed render draws)
        jit = self._device_jitter(device, explicit_only=True) if perturb and rays_o.is_cuda else None
        if jit is not None:
            jb0, ju = jit.tables(N, list(steps), ray_base=ray_base, advance=advance)
        if (len(steps) > 1 and not prop_needs_grad and not wants_prop_loss and rays_o.is_cuda and self._fused_shape()
                and self.fused_proposals):
            b0 = torch.linspace(0, 1, steps[0] + 1, device=device)
            u_tabs = None
            if jit is not None:
                b0, u_tabs = jb0, ju
            elif perturb:
                b0 = (b0.unsqueeze(0).expand(N, -1) + (torch.rand(N, steps[0] + 1, device=device) - 0.5) / steps[0]).clamp(0, 1)
                u_tabs = {}
                for k in range(1, len(steps)):
                    Tq = steps[k] + 1
                    base = torch.linspace(0.5 / Tq, 1 - 0.5 / Tq, steps=Tq, device=device)
                    u_tabs[k] = base.unsqueeze(0).expand(N, -1) + (torch.rand(N, Tq, device=device) - 0.5) / Tq
            with torch.no_grad():
                got = rm.render_rays(self._get_plan(), rays_o, rays_d, cam_near_far=cam_near_far, bins0_table=b0, u_tables=u_tabs,
                                     skip_final=True, out={})
            bins = got[f"bins{len(steps) - 1}"]
            first_stage = len(steps) - 1
        for k, T in enumerate(steps):
            if k < first_stage:
                continue
            if k == first_stage and first_stage > 0:
                pass                                            # bins of the last stage came from the fused proposal stages
            elif k == 0:
                # (the same stage-0 edges as the fused kernels and the fused training route: aten's scalar linspace recipe, sn_rm_jitter)
                if jit is not None:
                    bins = jb0
                else:
                    bins = rm.jitter(torch.rand(N, T + 1, device=device) if perturb else None, N, T + 1, 0, device=device) if rays_o.is_cuda else None
                if bins is None:
                    bins = torch.linspace(0, 1, T + 1, device=device).unsqueeze(0).expand(N, -1)
                    if perturb:
                        bins = (bins + (torch.rand_like(bins) - 0.5) / T).clamp(0, 1)
            elif jit is not None:
                bins = rm.sample_pdf(bins, weights, T + 1, False, u=ju[k])
            else:
                bins = rm.sample_pdf(bins, weights, T + 1, perturb)
            # bins -> distances, mid-points, (contracted) positions: nothing on this chain is differentiated
            # (sample_pdf's output carries no gradient, the encoders have no input gradient), so it is one kernel
            real_bins, rays_t, xyzs = rm.sample_positions(rays_o, rays_d, nears, fars, bins, contract=opt.contract)
            if k != len(steps) - 1:
                with torch.set_grad_enabled(update_proposal and torch.is_grad_enabled()):
                    sigmas = self.density(xyzs, proposal=k)["sigma"]
            else:
                dirs = rays_d.view(-1, 1, 3).expand_as(xyzs)
                dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
                field = self(xyzs, dirs)
                sigmas, colors, geo_feat = field["sigma"], field["color"], field["geo_feat"]
            # renderer.py:308-325 (delta*sigma -> alpha, transmittance, weights) forward and backward in one kernel each
            weights = rm.weights_from_sigma(real_bins, sigmas, opt.background == "last_sample")
            if self.training:
                all_bins.append(bins)
                all_weights.append(weights)

        weights_sum = weights.sum(dim=-1)
        depth = (weights * rays_t).sum(dim=-1)
        f_image = rm.composite(weights, colors)
        image = torch.sigmoid(self.view_mlp(f_image))
        results = {}
        if self.training and not opt.with_mask and not opt.with_sam:
            results["num_points"] = xyzs.shape[0] * xyzs.shape[1]
            results["weights"] = weights
            if opt.lambda_proposal > 0 and update_proposal:
                results["proposal_loss"] = proposal_loss(all_bins, all_weights)
            if opt.lambda_distort > 0:
                results["distort_loss"] = distort_loss(bins, weights)
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        results["weights_sum"] = weights_sum
        results["depth"] = depth
        results["image"] = image
        if samples is not None:
            samples.update(sigmas=sigmas, real_bins=real_bins, xyzs=xyzs, geo_feat=geo_feat)
            return results
        if opt.with_sam or return_mask > 0:
            self._heads(results, weights, xyzs, geo_feat, f_image, image, depth, return_feats, return_mask, H, W)
        return results
