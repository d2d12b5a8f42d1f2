"""The fused renderer (render.hip: sn_rm_render_rays; its front part lives in csrc/render_*.h):

    render_rays          nerf/renderer.py:221-357 + nerf/network.py:146-186, fused
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ._args import _f32, _flat3


class Tuning:
    """Kernel selection of the fused render (sn_render_tuning in include/sanerf_hip.h): plain attributes, copied into the call's
    config right before every launch.  `raymarching.tuning` is the process default; `RenderPlan(..., tuning=Tuning(...))` /
    `render_rays(..., tuning=...)` override it per plan / per call (two threads or two plans may differ -- rounds 1-3 read
    environment variables inside the library instead).  Every field 0 / False = the shipped default; none changes WHAT is
    computed beyond fp32 round-off.
        mlp_mode           _lib.MLP_AUTO | MLP_F16X3 (forces split-fp16 past the range guard) | MLP_MFMA32 (exact fp32) | MLP_VALU
        per_sample_form    the last stage evaluates the third MLP layer per sample everywhere (bit-identical to the compacting and
                           several-lanes-per-ray kernels; the default "linear tail" differs by fp32 round-off)
        densify            0 automatic, 1 never, 2 whenever the kernel exists (levels 5-6 of the main grid re-laid out per call)
        linear_tile_order  workgroup -> image tile (bit-neutral): 1 linear ids, 2 one contiguous id range per XCD over whole row pairs, 3 / 4 the same
                           ranges over 128x128- / 48x48-pixel super-tiles, 0 the default (4); tile_order_info() states each on the host
        prop_sp_max_rays / final_sp_max_rays   ray-count thresholds of the several-lanes-per-ray kernels (0 default, < 0 never)
        feat_levels        levels per pass of the feature stage (0 default)
        wave_tile          image mode: a wave covers 2^w x 2^(6-w) pixels (0 default = 8x8; 1..5)
        prop_sp_lanes      small linear-order batches: lanes sharing a ray in the proposal stages (0 automatic; 8 / 16 / 32; bit-neutral)
        feat_patch         feature stage: 1 = per-wave LDS patch of the dense levels (bit-neutral; measured 3-9 % slower, so 0 = off is the default)
        prop_pair          proposal stages: a lane evaluates two consecutive samples at once (bit-neutral): 0 automatic, 1 never, 2 always
        experiment         _lib.EXP_*: measured-and-rejected variants, experiments builds only (SN_LIB=.../libsanerf_hip_exp.so)
        persistent_tiles   last stage, plain linear-tail launch: one resident 8-wave workgroup per CU whose waves pull 64-ray wave tiles from eight
                           queues (bit-neutral): 0 automatic (more wave tiles than 8 x CUs), 1 never, 2 always; tile_queue_info() states the queues
        persistent_wgs     workgroups of that launch: 0 one per CU, n exactly n"""
    FIELDS = ("mlp_mode", "per_sample_form", "densify", "linear_tile_order", "prop_sp_max_rays", "final_sp_max_rays", "feat_levels", "band_streams", "exact_early_out", "wave_tile", "prop_sp_lanes", "feat_patch", "prop_pair", "experiment",
              "persistent_tiles", "persistent_wgs")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, 0)
        for k, v in kw.items():
            if k not in self.FIELDS:
                raise TypeError(f"Tuning: unknown field {k!r} (fields: {', '.join(self.FIELDS)})")
            setattr(self, k, int(v))

    def write(self, ct) -> None:
        for f in self.FIELDS:
            setattr(ct, f, int(getattr(self, f)))

    def __repr__(self):
        return "Tuning(" + ", ".join(f"{f}={getattr(self, f)}" for f in self.FIELDS if getattr(self, f)) + ")"


tuning = Tuning()          # process default; tests and A/B tools set attributes on it (monkeypatch.setattr(rm.tuning, "per_sample_form", 1))
FP16_SPLIT_LIMIT = 65504.0 * 0.5      # split-fp16 operands must stay below the fp16 range; half of it as the guard band


def last_launch_info() -> dict:
    """What the last render_rays call of this thread launched as its last stage (kernel variant, workgroups, LDS bytes, gather
    instructions per wave-sample): sn_rm_last_launch_info."""
    info = _lib.LaunchInfo()
    _lib.check(_lib.lib().sn_rm_last_launch_info(C.byref(info)), "last_launch_info")
    return _launch_info_dict(info)


def _launch_info_dict(info) -> dict:
    """sn_launch_info as a dict.  workgroups counts 256-ray tile units whichever launch form ran; grid_workgroups is the real grid."""
    return dict(final_kernel=info.final_kernel.decode(), workgroups=int(info.workgroups), lds_bytes=int(info.lds_bytes),
                dense_levels=int(info.dense_levels), gathers_per_wave_sample=int(info.gathers_per_wave_sample), launches=int(info.launches),
                persistent_tiles=int(info.persistent_tiles), grid_workgroups=int(info.grid_workgroups))


def tile_queue_info(units: int, queue: int, order: int = 0, wave_tile: int = 0) -> dict:
    """Queue `queue` (0..7) of the persistent last stage for a launch of `units` 256-ray tile units under Tuning.linear_tile_order = order
    (sn_rm_tile_queue_info: host arithmetic only): queues, wave_tiles = 4 * units, and the wave-tile ids [begin, end) the queue holds."""
    info = _lib.TileQueueInfo()
    _lib.check(_lib.lib().sn_rm_tile_queue_info(int(units), int(order), int(wave_tile), int(queue), C.byref(info)), "tile_queue_info")
    return dict(queues=int(info.queues), wave_tiles=int(info.wave_tiles), begin=int(info.begin), end=int(info.end))


def tile_order_info(W: int, rows: int, workgroup: int, wave_tile: int = 0, order: int = 0) -> dict:
    """The part of a W x rows image that workgroup `workgroup` of the render stages takes under Tuning.wave_tile / linear_tile_order = order
    (sn_rm_tile_order_info: host arithmetic only, no device needed): workgroups of the launch, tile_id, the wave tile's size and the pixel
    origins [(x, y)] * 4 of its four wave tiles (None: padding of the last workgroup)."""
    info = _lib.TileOrderInfo()
    _lib.check(_lib.lib().sn_rm_tile_order_info(int(W), int(rows), int(wave_tile), int(order), int(workgroup), C.byref(info)), "tile_order_info")
    return dict(workgroups=int(info.workgroups), tile_id=int(info.tile_id), tile_w=int(info.tile_w), tile_h=int(info.tile_h),
                tiles=[(int(info.x[w]), int(info.y[w])) if info.x[w] >= 0 else None for w in range(4)])


def _fill_grid(desc: _lib.GridDesc, enc, table: torch.Tensor) -> None:
    from ..gridencoder.grid import _host_offsets
    offs = _host_offsets(enc.offsets)
    desc.embeddings = table.data_ptr()
    desc.table_dtype = _lib.SN_F16 if table.dtype == torch.float16 else _lib.SN_F32
    for i, o in enumerate(offs):
        desc.offsets[i] = o
    desc.D, desc.C, desc.L = enc.input_dim, enc.level_dim, enc.num_levels
    desc.S = float(np.float32(np.log2(enc.per_level_scale)))
    desc.H = int(enc.base_resolution)
    desc.gridtype, desc.align_corners, desc.interp = enc.gridtype_id, int(enc.align_corners), enc.interp_id


def _fill_mlp(desc: _lib.MlpDesc, layers: Sequence[torch.nn.Linear], dim_in: int, keep: list) -> None:
    desc.num_layers = len(layers)
    desc.activation = 0
    desc.skip_mask = 0
    desc.dims[0] = dim_in
    for l, lin in enumerate(layers):
        w = _f32(lin.weight)
        keep.append(w)
        desc.weight[l] = w.data_ptr()
        desc.dims[l + 1] = w.shape[0]
        if lin.bias is not None:
            b = _f32(lin.bias)
            keep.append(b)
            desc.bias[l] = b.data_ptr()
        else:
            desc.bias[l] = None


class RenderPlan:
    """Everything sn_rm_render_rays needs from a NeRFNetwork-shaped module, built once and reused:
    the config struct (device pointers of tables / MLP weights) and a cached workspace.

    table_dtype=torch.float16 renders from half-precision copies of the hash tables (made here,
    the module keeps its fp32 parameters); arithmetic stays fp32 either way."""

    def __init__(self, model, num_steps: Sequence[int], table_dtype=torch.float32, feat_encoder=None,
                 early_stop_eps: float = 0.0, compact_live: bool = False, tuning: Optional["Tuning"] = None, keep_packs: bool = False):
        self.keep: list = []
        # opt-in for a FROZEN field (inference, evaluation of many views): the packed MLP weights and pair / quad rows that a call leaves in the
        # plan's workspace are read again by the next call instead of being re-made (sn_render_io.pack_valid), as long as the call is the
        # same in everything the packs depend on (_pack_key).  A writer that changes tables or weights without moving their version counters
        # (`.data.copy_()`, raw pointers) must call invalidate_packs() / invalidate_range(), as for the range guard.  May be set at any time.
        self.keep_packs = bool(keep_packs)
        self._pack_key = None            # what the packs in self._ws were made from; None: nothing to reuse
        self.pack_reuses = 0             # calls that ran on kept packs (tests, measurements)
        self.tuning = tuning            # None: the module default `raymarching.tuning` at call time
        cfg = _lib.RenderCfg()
        S = len(num_steps)
        if not 1 <= S <= _lib.MAX_STAGES:
            raise RuntimeError(f"num_steps must have 1..{_lib.MAX_STAGES} entries")
        cfg.num_stages = S
        for k, t in enumerate(num_steps):
            cfg.num_steps[k] = int(t)

        self.copies: list = []       # (source parameter, converted copy) pairs: see refresh_tables()

        def table_of(enc):
            src = enc.embeddings.detach()
            t = src
            if src.dtype != table_dtype or not src.is_contiguous():
                t = src.to(table_dtype).contiguous()
                self.copies.append((enc.embeddings, t))
            self.keep.append(t)
            return t

        for k in range(S - 1):
            enc = model.prop_encoders[k]
            _fill_grid(cfg.prop_grid[k], enc, table_of(enc))
            _fill_mlp(cfg.prop_mlp[k], list(model.prop_mlp[k].net), model.prop_mlp[k].dim_in, self.keep)
        _fill_grid(cfg.grid, model.grid, table_of(model.grid))
        _fill_mlp(cfg.grid_mlp, list(model.grid_mlp.net), model.grid_mlp.dim_in, self.keep)
        _fill_mlp(cfg.view_mlp, list(model.view_mlp.net), model.view_mlp.dim_in, self.keep)
        cfg.sh_degree = model.view_encoder.degree
        ab = model.aabb_infer.detach().cpu().tolist()
        for i in range(6):
            cfg.aabb[i] = ab[i]
        cfg.min_near = float(model.min_near)
        cfg.bound = float(model.bound)
        cfg.contract = int(bool(model.opt.contract))
        cfg.last_sample_opaque = int(model.opt.background == "last_sample")
        cfg.bg_color = 1.0
        self.feat_dim = 0
        if feat_encoder is not None:                    # s_grid (network.py:103): f_sam accumulated inside the render
            _fill_grid(cfg.feat_grid, feat_encoder, table_of(feat_encoder))
            cfg.with_feat = 1
            self.feat_dim = feat_encoder.output_dim
        cfg.early_stop_eps = float(early_stop_eps)      # opt-in transmittance early-out of the last stage (0 = reference behaviour)
        cfg.compact_live = int(bool(compact_live))      # opt-in per-ray termination + live-sample compaction (k_final_stage_cmp)
        self.cfg = cfg
        self._range_model = model
        self._range_versions = None
        self.activation_bound = 0.0
        self.check_range()
        self.num_steps = [int(t) for t in num_steps]
        self.geo = int(getattr(model, "geom_feat_dim", list(model.grid_mlp.net)[-1].weight.shape[0] - 1))
        self.ncol = self.geo + model.view_encoder.output_dim
        self._ws: Optional[torch.Tensor] = None

    @torch.no_grad()
    def check_range(self) -> None:
        """Static range guard of the split-fp16 MLP of the final stage.  Hash-grid features are convex combinations of
        table values, so |feature| <= max|table|; a ReLU layer's outputs are bounded by the largest row L1 norm of its
        weight times the bound of its inputs.  If features, hidden activations or weights could reach the fp16 range the
        plan switches the kernel to the exact fp32 matrix-core path (cfg.mlp_exact_fp32, ~2.2x slower final stage) instead
        of risking inf / NaN.  Re-evaluated when a parameter's version counter moved (device reductions + ONE sync); called by
        render_rays right before a launch that runs the final stage -- never for skip_final calls, whose proposal stages use
        fp32 vector arithmetic only (a training step that takes its sample positions from the fused proposal stages stays free
        of host synchronisation).  sanerf_hq_amd.optim.Adam bumps the version counters of the tensors it updates."""
        m = self._range_model
        tensors = [m.grid.embeddings] + [lin.weight for lin in m.grid_mlp.net]
        versions = tuple((t.data_ptr(), t._version) for t in tensors)
        if versions == self._range_versions:
            return
        self._range_versions = versions
        layers = list(m.grid_mlp.net)
        # every reduction stays on the device; ONE host transfer (= one sync) fetches them all
        stats = [m.grid.embeddings.detach().abs().max().float()]
        stats += [lin.weight.detach().float().abs().sum(dim=1).max() for lin in layers[:-1]]   # the last layer's outputs stay fp32 accumulators
        stats += [lin.weight.detach().abs().max().float() for lin in layers]
        vals = torch.stack(stats).tolist()
        bound = worst = vals[0]
        for row_l1 in vals[1:len(layers)]:
            bound = row_l1 * bound
            worst = max(worst, bound)
        wmax = max(vals[len(layers):]) if layers else 0.0
        if any(v != v for v in vals):
            worst = float("nan")
        self.activation_bound = max(worst, wmax)
        exact = not (self.activation_bound < FP16_SPLIT_LIMIT)          # also catches NaN
        if exact and not self.cfg.mlp_exact_fp32:
            warnings.warn(f"fused render: activations of the 32-64-64-16 MLP are only bounded by {self.activation_bound:.3g} "
                          f"(>= {FP16_SPLIT_LIMIT:.0f}): using the exact fp32 matrix-core path instead of split-fp16")
        self.cfg.mlp_exact_fp32 = int(exact)

    def invalidate_range(self) -> None:
        """Forget the cached range-guard decision: the next render re-evaluates it.  For writers that change the field's parameters WITHOUT
        moving their version counters -- `param.data.copy_()` (torch_ema's copy_to / restore around an evaluation, as the reference's trainer
        uses it), raw-pointer writers, a load_state_dict into .data -- which check_range's (data_ptr, _version) key cannot see."""
        self._range_versions = None
        self._pack_key = None

    def invalidate_packs(self) -> None:
        """Forget the packs kept in the workspace (keep_packs): the next render makes them again."""
        self._pack_key = None

    def _pack_key_of(self, io, stream: int):
        """Everything the pack kernels' output and its place in the workspace depend on: the whole config (table / weight pointers, dtypes,
        level offsets, tuning: densify; mlp_exact_fp32), the versions of the tensors it points to, and what decides the call's route (N,
        tile_w, which optional inputs / outputs are present), the workspace and the stream the packs were ordered on."""
        present = tuple(bool(v) for v in (io.cam_near_far, io.bins0_table, *io.u_table, io.image, *io.bins, *io.weights, *io.sigmas, *io.inds,
                                          io.xyzs_last, io.geo_feat_last, io.f_image, io.f_feat))
        shape = (io.N, io.tile_w, io.bins0_ray_stride, tuple(io.u_ray_stride), io.skip_final, io.out_stride, io.head_stride, present)
        return (bytes(self.cfg), tuple((t.data_ptr(), t._version) for t in self.keep), shape, io.workspace, io.workspace_bytes, stream)

    @torch.no_grad()
    def refresh_tables(self) -> None:
        """Re-convert the table copies (render_table_dtype != the parameters' dtype) from the live parameters, in place:
        the plan's device pointers stay valid.  A plan over fp32 tables holds no copies and this is a no-op.  (The fp16 range
        guard is evaluated by render_rays, see check_range.)"""
        for src, copy in self.copies:
            copy.copy_(src.detach())

    def workspace(self, N: int, tile_w: int, device) -> torch.Tensor:
        (self.tuning or tuning).write(self.cfg.tuning)
        need = int(_lib.lib().sn_rm_render_workspace_bytes(C.byref(self.cfg), N, tile_w))
        if self._ws is None or self._ws.numel() < need or self._ws.device != torch.device(device):
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
            self._pack_key = None
        return self._ws


def _fill_io(plan: RenderPlan, io, N: int, tile_w: int, want, u_tables, bins0_table, skip_final: bool, packed, head_input: bool, tuning, buf, table):
    """What render_rays and route_info share: the call's sn_render_io (but for the rays and the workspace) and the tuning written into the
    plan's config.  buf(name, shape, dtype) -> the device pointer of that output; table(t) -> (tensor as the call reads it, its pointer)."""
    io.N, io.tile_w = N, int(tile_w)
    if bins0_table is not None:      # [T0+1]: one table for all rays; [N, T0+1]: per ray (a training step's perturbed bins)
        b0, io.bins0_table = table(bins0_table)
        if b0.dim() == 2:
            if b0.shape != (N, plan.num_steps[0] + 1):
                raise RuntimeError(f"bins0_table: expected [{N}, {plan.num_steps[0] + 1}] per-ray bins, got {tuple(b0.shape)}")
            io.bins0_ray_stride = b0.shape[1]
    if u_tables:
        for k, u in u_tables.items():
            u, io.u_table[k] = table(u)
            if u.dim() == 2:
                if u.shape != (N, plan.num_steps[k] + 1):
                    raise RuntimeError(f"u_tables[{k}]: expected [{N}, {plan.num_steps[k] + 1}] per-ray values, got {tuple(u.shape)}")
                io.u_ray_stride[k] = u.shape[1]
    S = plan.cfg.num_stages
    want = set(want)
    if skip_final:                   # proposal stages only: the last stage's resampled bins [N, T_last+1] are the result
        if S < 2:
            raise RuntimeError("render_rays(skip_final=True) needs a schedule with proposal stages")
        io.skip_final = 1
        want = set()
        io.bins[S - 1] = buf(f"bins{S - 1}", (N, plan.num_steps[S - 1] + 1))
    else:
        plan.check_range()           # fp16 range guard of the final stage's MLP: a no-op unless a parameter version moved
        if packed is not None:
            base = packed.data_ptr()
            io.image, io.depth, io.weights_sum, io.out_stride = base, base + 12, base + 16, packed.shape[1]
        else:
            io.image = buf("image", (N, 3))
            io.depth = buf("depth", (N,))
            io.weights_sum = buf("weights_sum", (N,))
    for k in range(S):
        T = plan.num_steps[k]
        if "bins" in want or (k == S - 1 and "bins_last" in want):
            io.bins[k] = buf(f"bins{k}", (N, T + 1))
        if "weights" in want or (k == S - 1 and "weights_last" in want):
            io.weights[k] = buf(f"weights{k}", (N, T))
        if "sigmas" in want or (k == S - 1 and "sigmas_last" in want):
            io.sigmas[k] = buf(f"sigmas{k}", (N, T))
        if "inds" in want and k >= 1:
            io.inds[k] = buf(f"inds{k}", (N, T + 1), torch.int32)
    Tl = plan.num_steps[S - 1]
    if "xyzs_last" in want:
        io.xyzs_last = buf("xyzs_last", (N, Tl, 3))
    if "geo_feat_last" in want:
        io.geo_feat_last = buf("geo_feat_last", (N, Tl, plan.geo))
    if head_input and plan.cfg.with_feat and not skip_final:
        io.f_feat = buf("head_input", (N, plan.feat_dim + plan.ncol + 4))
        io.f_image, io.head_stride = io.f_feat + 4 * plan.feat_dim, plan.feat_dim + plan.ncol + 4
    else:
        if "f_image" in want:
            io.f_image = buf("f_image", (N, plan.ncol))
        if plan.cfg.with_feat and not skip_final:
            io.f_feat = buf("f_feat", (N, plan.feat_dim))
    eff = tuning or plan.tuning or globals()["tuning"]           # per call > per plan > process default
    eff.write(plan.cfg.tuning)
    return eff


def route_info(plan: RenderPlan, N: int, tile_w: int = 0, want: Sequence[str] = (), u_tables: Optional[Dict[int, torch.Tensor]] = None,
               bins0_table: Optional[torch.Tensor] = None, skip_final: bool = False, tuning: Optional["Tuning"] = None,
               packed: Optional[torch.Tensor] = None, head_input: bool = False, compute_units: Optional[int] = None) -> dict:
    """What last_launch_info() would report after render_rays(plan, <N rays>, ...) with the same arguments, without rendering
    (sn_rm_render_route_info: the same validation and route planning on the host; no render kernel is launched and no output is
    allocated).  Like render_rays it writes the effective tuning into plan.cfg.tuning and, unless skip_final, consults the plan's fp16
    range guard (plan.check_range(): device reductions and one sync when a parameter version moved) -- the guard decides the route.
    compute_units: CUs of the device to plan for (None: the device of the plan's tables; 0: not known)."""
    io = _lib.RenderIO()
    stand_in = 64                                                  # an aligned non-NULL address: the dry run dereferences nothing
    io.rays_o = io.rays_d = stand_in
    _fill_io(plan, io, int(N), tile_w, want, u_tables, bins0_table, skip_final, packed, head_input, tuning,
             lambda name, shape, dtype=torch.float32: stand_in, lambda t: (t, stand_in))
    info = _lib.LaunchInfo()
    if compute_units is None:      # the device the plan's tables live on: what sn_rm_render_rays asks its device (the automatic rule of persistent_tiles)
        t0 = plan.keep[0] if plan.keep else None
        compute_units = torch.cuda.get_device_properties(t0.device).multi_processor_count if t0 is not None and t0.is_cuda else 0
    _lib.check(_lib.lib().sn_rm_render_route_info_cus(C.byref(plan.cfg), C.byref(io), int(compute_units), C.byref(info)), "route_info")
    return _launch_info_dict(info)


def render_rays(plan: RenderPlan, rays_o, rays_d, cam_near_far=None, bg_color: float = 1.0, tile_w: int = 0,
                want: Sequence[str] = (), u_tables: Optional[Dict[int, torch.Tensor]] = None,
                bins0_table: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None,
                skip_final: bool = False, tuning: Optional["Tuning"] = None, packed: Optional[torch.Tensor] = None,
                head_input: bool = False):
    """Fused render of N rays.  Returns dict(image [N,3], depth [N], weights_sum [N]) plus the
    per-stage tensors named in `want`: 'bins', 'weights', 'sigmas', 'inds' (all stages),
    'weights_last', 'xyzs_last', 'geo_feat_last', 'f_image'; a plan built with `feat_encoder` also
    returns 'f_feat' [N, L*C] = composite(weights_last, feat_encoder(xyzs_last)).
    packed: a contiguous fp32 [N, K >= 5] buffer -- the kernels write rgb | depth | weights_sum into its first five columns (sn_render_io.out_stride)
    and the returned image / depth / weights_sum are views of it: the payload of the image all-gather without a concatenation (dist.py).
    head_input (plans with `feat_encoder`): also return 'head_input' [N, L*C + ncol + 4] = cat([f_feat, f_image, image, depth]) -- the SAM head's
    MLP input of renderer.py:366 -- written in place by the kernels (sn_render_io.head_stride); 'f_feat' / 'f_image' are then views of it."""
    rays_o, rays_d = _flat3(rays_o), _flat3(rays_d)
    N = rays_o.shape[0]
    device = rays_o.device
    io = _lib.RenderIO()
    res: Dict[str, torch.Tensor] = {} if out is None else out
    keep: List[torch.Tensor] = []

    def buf(name, shape, dtype=torch.float32):
        t = res.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
            t = torch.empty(shape, device=device, dtype=dtype)     # (a strided view left by an earlier packed= call is not reused)
            res[name] = t
        return _lib.dev(t, name, dtype)

    def table(t):
        t = t.to(device).contiguous().float()
        keep.append(t)
        return t, t.data_ptr()

    io.rays_o, io.rays_d = _lib.dev(rays_o, "rays_o"), _lib.dev(rays_d, "rays_d")
    if cam_near_far is not None:
        cnf = cam_near_far.float()
        if cnf.shape[0] == 1:
            cnf = cnf.expand(N, 2)
        cnf = cnf.contiguous()
        keep.append(cnf)
        io.cam_near_far = _lib.dev(cnf, "cam_near_far")
    if packed is not None and not skip_final:
        if not (packed.is_cuda and packed.dtype == torch.float32 and packed.dim() == 2 and packed.shape[0] == N and packed.shape[1] >= 5
                and packed.is_contiguous() and packed.device == device):
            raise RuntimeError(f"render_rays: packed must be a contiguous fp32 [{N}, >=5] tensor on {device}, got {tuple(packed.shape)} {packed.dtype}")
        res["image"], res["depth"], res["weights_sum"] = packed[:, :3], packed[:, 3], packed[:, 4]
    eff = _fill_io(plan, io, N, tile_w, want, u_tables, bins0_table, skip_final, packed, head_input, tuning, buf, table)
    S = plan.cfg.num_stages
    if io.head_stride:
        hb = res["head_input"]
        res["f_feat"], res["f_image"] = hb[:, :plan.feat_dim], hb[:, plan.feat_dim:plan.feat_dim + plan.ncol]
    need = int(_lib.lib().sn_rm_render_workspace_bytes(C.byref(plan.cfg), N, int(tile_w)))
    ws = plan.workspace(N, int(tile_w), device)
    if ws.numel() < need:                                          # (a per-call tuning that needs more than the plan's own)
        plan._ws = ws = torch.empty(need, dtype=torch.uint8, device=device)
        plan._pack_key = None
    eff.write(plan.cfg.tuning)
    io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
    plan.cfg.bg_color = float(bg_color)
    stream = _lib.stream()
    key = plan._pack_key_of(io, stream) if plan.keep_packs else None
    reuse = key is not None and key == plan._pack_key
    io.pack_valid = _lib.PACK_VALID if reuse else 0
    plan._pack_key = None                                          # (a call that fails leaves nothing to vouch for)
    _lib.check(_lib.lib().sn_rm_render_rays(C.byref(plan.cfg), C.byref(io), stream), "render_rays")
    plan._pack_key = key
    plan.pack_reuses += int(reuse)
    if "weights_last" in set(want) and not skip_final:
        res["weights_last"] = res[f"weights{S - 1}"]
    return res
