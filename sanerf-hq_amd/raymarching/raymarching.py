"""`raymarching` operators on MI355X.

The reference's README (README.md:32-34) mentions a `raymarching` extension that is not in
its tree; the ray-marching maths lives as torch code in nerf/utils.py and nerf/renderer.py.
This module is that operator surface, implemented over libsanerf_hip.so:

    generate_rays        nerf/utils.py:182-304 (full image branch)
    near_far_from_aabb   nerf/renderer.py:122-139
    contract             nerf/renderer.py:60-69
    sample_pdf           nerf/renderer.py:84-119   (+ the integer searchsorted result)
    weights_from_sigma   nerf/renderer.py:308-325
    composite            nerf/renderer.py:333-338, 361, 384  (autograd w.r.t. both operands)
    grid_composite       nerf/renderer.py:301-302 + 361: composite(weights, s_grid(xyzs)) fused (inference)
    mlp_forward          nerf/network.py:31-66 (+ LayerNorm :115): the 256-wide head MLPs on the matrix cores (inference)
    render_rays          nerf/renderer.py:221-357 + nerf/network.py:146-186, fused
    jitter               nerf/renderer.py:262-270, 97-102: one stage's perturbed bins / u from caller-supplied uniforms
    jitter_tables        the same tables for every stage in one launch, uniforms from a Philox counter on the device (DeviceJitter)
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch.autograd import Function

from .. import _lib


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
        experiment         _lib.EXP_*: measured-and-rejected variants, experiments builds only (SN_LIB=.../libsanerf_hip_exp.so)"""
    FIELDS = ("mlp_mode", "per_sample_form", "densify", "linear_tile_order", "prop_sp_max_rays", "final_sp_max_rays", "feat_levels", "band_streams", "exact_early_out", "wave_tile", "prop_sp_lanes", "feat_patch", "prop_pair", "experiment")

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
check_range_default = False   # mlp_forward(check_range=None): read the overflow flag after every call (one device sync each)


def last_launch_info() -> dict:
    """What the last render_rays call of this thread launched as its last stage (kernel variant, workgroups, LDS bytes, gather
    instructions per wave-sample): sn_rm_last_launch_info."""
    info = _lib.LaunchInfo()
    _lib.check(_lib.lib().sn_rm_last_launch_info(C.byref(info)), "last_launch_info")
    return dict(final_kernel=info.final_kernel.decode(), workgroups=int(info.workgroups), lds_bytes=int(info.lds_bytes),
                dense_levels=int(info.dense_levels), gathers_per_wave_sample=int(info.gathers_per_wave_sample), launches=int(info.launches))


def tile_order_info(W: int, rows: int, workgroup: int, wave_tile: int = 0, order: int = 0) -> dict:
    """The part of a W x rows image that workgroup `workgroup` of the render stages takes under Tuning.wave_tile / linear_tile_order = order
    (sn_rm_tile_order_info: host arithmetic only, no device needed): workgroups of the launch, tile_id, the wave tile's size and the pixel
    origins [(x, y)] * 4 of its four wave tiles (None: padding of the last workgroup)."""
    info = _lib.TileOrderInfo()
    _lib.check(_lib.lib().sn_rm_tile_order_info(int(W), int(rows), int(wave_tile), int(order), int(workgroup), C.byref(info)), "tile_order_info")
    return dict(workgroups=int(info.workgroups), tile_id=int(info.tile_id), tile_w=int(info.tile_w), tile_h=int(info.tile_h),
                tiles=[(int(info.x[w]), int(info.y[w])) if info.x[w] >= 0 else None for w in range(4)])


def _flat3(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1, 3).contiguous().float()


def generate_rays(pose, intrinsics, H: int, W: int, device="cuda", row_begin: int = 0, row_end: Optional[int] = None):
    """Rays of image rows [row_begin, row_end): rays_o, rays_d of shape [(rows)*W, 3].
    pose: 4x4 cam2world (array-like / tensor), intrinsics: (fx, fy, cx, cy)."""
    row_end = H if row_end is None else row_end
    pose = np.asarray(pose.detach().cpu() if torch.is_tensor(pose) else pose, dtype=np.float32).reshape(4, 4)
    fx, fy, cx, cy = [float(v) for v in (intrinsics.tolist() if hasattr(intrinsics, "tolist") else intrinsics)]
    n = (row_end - row_begin) * W
    rays_o = torch.empty(n, 3, device=device, dtype=torch.float32)
    rays_d = torch.empty(n, 3, device=device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_generate_rays(_lib.host_f32(pose.reshape(-1)), fx, fy, cx, cy, H, W, row_begin, row_end,
                                              _lib.dev(rays_o, "rays_o"), _lib.dev(rays_d, "rays_d"), _lib.stream()),
               "generate_rays")
    return rays_o, rays_d


def rays_from_pixels(poses: torch.Tensor, intrinsics: torch.Tensor, inds: torch.Tensor, W: int):
    """Rays through the flat pixel indices `inds` [N] (row-major, width W): poses [1 or N, 4, 4] and intrinsics
    [1 or N, 4] on the device, one camera for all rays or one per ray (nerf/utils.py:209-287 with the per-ray cameras of
    provider.py:908-913).  Everything stays on the device."""
    inds = inds.reshape(-1).contiguous().long()
    N = inds.shape[0]
    poses = poses.reshape(-1, 16).contiguous().float()
    intrinsics = intrinsics.reshape(-1, 4).contiguous().float()
    rays_o = torch.empty(N, 3, device=inds.device, dtype=torch.float32)
    rays_d = torch.empty(N, 3, device=inds.device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_rays_from_pixels(_lib.dev(poses, "poses"), poses.shape[0], _lib.dev(intrinsics, "intrinsics"),
                                                 intrinsics.shape[0], _lib.dev(inds, "inds", torch.int64), int(W), N,
                                                 _lib.dev(rays_o, "rays_o"), _lib.dev(rays_d, "rays_d"), _lib.stream()),
               "rays_from_pixels")
    return rays_o, rays_d


def _host_values(t) -> list:
    """Host copy of a small device tensor, memoised on the tensor object (keyed by its in-place version counter): a
    device->host read per call would put a synchronisation into every training step and forbids graph capture."""
    if not torch.is_tensor(t):
        return list(t)
    cached = getattr(t, "_sn_host_values", None)
    if cached is None or cached[0] != t._version:
        cached = (t._version, t.detach().cpu().tolist())
        try:
            t._sn_host_values = cached
        except AttributeError:
            pass
    return cached[1]


def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.05):
    rays_o, rays_d = _flat3(rays_o), _flat3(rays_d)
    N = rays_o.shape[0]
    nears = torch.empty(N, 1, device=rays_o.device, dtype=torch.float32)
    fars = torch.empty(N, 1, device=rays_o.device, dtype=torch.float32)
    ab = _host_values(aabb)
    _lib.check(_lib.lib().sn_rm_near_far_from_aabb(_lib.dev(rays_o, "rays_o"), _lib.dev(rays_d, "rays_d"), _lib.host_f32(ab),
                                                   float(min_near), N, _lib.dev(nears, "nears"), _lib.dev(fars, "fars"),
                                                   _lib.stream()), "near_far_from_aabb")
    return nears, fars


def contract(x):
    shape = x.shape
    flat = _flat3(x)
    z = torch.empty_like(flat)
    _lib.check(_lib.lib().sn_rm_contract(_lib.dev(flat, "x"), flat.shape[0], _lib.dev(z, "z"), _lib.stream()), "contract")
    return z.view(shape)


def sample_pdf(bins, weights, T: int, perturb: bool = False, return_inds: bool = False, u: Optional[torch.Tensor] = None):
    """bins [N,T0+1], weights [N,T0] -> [N,T] (no gradient, like the `.detach()` at renderer.py:274)."""
    bins = bins.detach().contiguous().float()
    weights = weights.detach().contiguous().float()
    N, T0 = weights.shape
    out = torch.empty(N, T, device=bins.device, dtype=torch.float32)
    inds = torch.empty(N, T, device=bins.device, dtype=torch.int32) if return_inds else None
    u_stride = 0
    if perturb:   # renderer.py:98-102
        base = torch.linspace(0.5 / T, 1 - 0.5 / T, steps=T, device=bins.device)
        u = (base.expand(N, T) + (torch.rand(N, T, device=bins.device) - 0.5) / T).contiguous()
    if u is not None:
        u = u.contiguous().float()
        u_stride = 0 if u.dim() == 1 else T
    _lib.check(_lib.lib().sn_rm_sample_pdf(_lib.dev(bins, "bins"), _lib.dev(weights, "weights"), N, T0, T,
                                           _lib.dev(u, "u"), u_stride, _lib.dev(out, "out_bins"),
                                           _lib.dev(inds, "inds", torch.int32), _lib.stream()), "sample_pdf")
    return (out, inds) if return_inds else out


class _weights_from_sigma(Function):
    """weights [N,T] of renderer.py:308-325 from real_bins [N,T+1] and sigmas [N,T]; differentiable w.r.t. sigmas (the
    bin edges carry no gradient on this path: sample_pdf's output is not differentiated)."""

    @staticmethod
    def forward(ctx, real_bins, sigmas, last_sample_opaque):
        real_bins = real_bins.detach().contiguous().float()
        sig = sigmas.detach().contiguous().float()
        N, T = sig.shape
        w = torch.empty(N, T, device=sig.device, dtype=torch.float32)
        _lib.check(_lib.lib().sn_rm_weights_from_sigma(_lib.dev(real_bins, "real_bins"), _lib.dev(sig, "sigmas"), N, T,
                                                       int(last_sample_opaque), _lib.dev(w, "weights"), _lib.stream()),
                   "weights_from_sigma")
        ctx.save_for_backward(real_bins, sig)
        ctx.last = int(last_sample_opaque)
        return w

    @staticmethod
    def backward(ctx, gw):
        real_bins, sig = ctx.saved_tensors
        N, T = sig.shape
        gw = gw.contiguous().float()
        gs = torch.empty_like(sig)
        _lib.check(_lib.lib().sn_rm_weights_from_sigma_backward(_lib.dev(real_bins, "real_bins"), _lib.dev(sig, "sigmas"),
                                                                _lib.dev(gw, "grad_weights"), N, T, ctx.last,
                                                                _lib.dev(gs, "grad_sigmas"), _lib.stream()), "weights_from_sigma_backward")
        return None, gs, None


WEIGHTS_BACKWARD_MAX_T = 131072   # sn_rm_weights_from_sigma_backward: any ray the product meets (up to 256 samples in one wave's registers, beyond that the
                                  # segment prefixes in LDS); the torch statement below is what the tests compare the kernel with (they lower this constant)


def weights_from_sigma(real_bins, sigmas, last_sample_opaque: bool = True):
    """real_bins [N,T+1], sigmas [N,T] -> weights [N,T]; under autograd the gradient reaches `sigmas`."""
    if torch.is_grad_enabled() and sigmas.requires_grad:
        if sigmas.shape[-1] > WEIGHTS_BACKWARD_MAX_T:       # (renderer.py:308-325 as torch states it: the tests' comparison route)
            ds = (real_bins[..., 1:] - real_bins[..., :-1]).detach() * sigmas
            if last_sample_opaque:
                ds = torch.cat([ds[..., :-1], torch.full_like(ds[..., -1:], torch.inf)], dim=-1)
            trans = torch.cumsum(ds[..., :-1], dim=-1)
            trans = torch.exp(-torch.cat([torch.zeros_like(ds[..., :1]), trans], dim=-1))
            return ((1 - torch.exp(-ds)) * trans).nan_to_num(0)
        return _weights_from_sigma.apply(real_bins, sigmas, bool(last_sample_opaque))
    return _weights_from_sigma.forward(_NoCtx(), real_bins, sigmas, bool(last_sample_opaque))


class _NoCtx:
    def save_for_backward(self, *a):
        pass


def sample_positions(rays_o, rays_d, nears, fars, bins, contract: bool = True, grid_bound: float = 0.0):
    """One stage's geometry (renderer.py:277-285), no autograd: bins [N,T+1] -> (real_bins [N,T+1], rays_t [N,T],
    xyzs [N,T,3]); positions are contracted into [-2,2]^3 when `contract`.  grid_bound > 0: the positions come back as the
    grid encoder's unit-cube coordinates (x + grid_bound) / (2 grid_bound) (gridencoder/grid.py:156) -- for `grid_encode` itself."""
    rays_o, rays_d = rays_o.detach().contiguous().float(), rays_d.detach().contiguous().float()
    bins = bins.detach().contiguous().float()
    N, T = bins.shape[0], bins.shape[1] - 1
    nears = nears.detach().reshape(-1).contiguous().float()
    fars = fars.detach().reshape(-1).contiguous().float()
    assert nears.numel() == N and fars.numel() == N and rays_o.shape == (N, 3)
    dev = bins.device
    real_bins = torch.empty(N, T + 1, device=dev, dtype=torch.float32)
    rays_t = torch.empty(N, T, device=dev, dtype=torch.float32)
    xyzs = torch.empty(N, T, 3, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_sample_positions_ex(_lib.dev(rays_o, "rays_o"), _lib.dev(rays_d, "rays_d"), _lib.dev(nears, "nears"),
                                                    _lib.dev(fars, "fars"), _lib.dev(bins, "bins"), N, T, int(contract), float(grid_bound),
                                                    _lib.dev(real_bins, "real_bins"), _lib.dev(rays_t, "rays_t"), _lib.dev(xyzs, "xyzs"),
                                                    _lib.stream()), "sample_positions")
    return real_bins, rays_t, xyzs


def jitter(uniform: Optional[torch.Tensor], N: int, T: int, kind: int, device=None) -> torch.Tensor:
    """Sampling positions of a training stage from one uniform [0,1) tensor (sn_rm_jitter): kind 0 = the stage-0 bins of renderer.py:262-270
    (T = num_steps[0] + 1 edges, clamped to [0,1]), kind 1 = sample_pdf's u of renderer.py:97-102.  uniform: [N,T] (contiguous) or None."""
    if uniform is not None:
        uniform = uniform.reshape(N, T)
        device = uniform.device
    out = torch.empty(N, T, device=device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_jitter(_lib.dev(uniform, "uniform"), N, T, int(kind), _lib.dev(out, "out"), _lib.stream()), "jitter")
    return out


def jitter_tables(state: torch.Tensor, N: int, steps: Sequence[int], ray_base: int = 0, advance: bool = True,
                  want: Optional[Sequence[int]] = None, out: Optional[Dict[int, torch.Tensor]] = None):
    """The per-ray jitter tables of every stage of the schedule `steps` in one launch (sn_rm_jitter_tables; advance adds a one-thread launch), from the counter-based
    generator whose state is `state` (int64 [4] on the device: seed, draw, ticket, reserved -- DeviceJitter holds one):
    -> (bins0 [N, steps[0]+1], {k: u_k [N, steps[k]+1] for k >= 1}), what render_rays takes as bins0_table / u_tables.
    Row n belongs to ray ray_base + n: a value depends on (seed, draw, stage, ray, column) only, so the chunks of an image, each drawn with
    its own ray_base, make the image's table.  advance: the launch ends with draw + 1 (on the device: a captured call draws fresh
    jitter on every replay); False leaves the state as it was.  want: the stages to write (0 = bins0; None = all): the others come
    back as None / are missing.  out: {stage: contiguous fp32 [N, steps[k]+1] tensor} to write into."""
    if not (torch.is_tensor(state) and state.is_cuda and state.dtype == torch.int64 and state.numel() == 4 and state.is_contiguous()):
        raise RuntimeError("jitter_tables: state must be a contiguous int64 [4] CUDA tensor (seed, draw, ticket, reserved)")
    N, S = int(N), len(steps)
    stages = set(range(S)) if want is None else {int(k) for k in want}
    if not stages <= set(range(S)):
        raise RuntimeError(f"jitter_tables: want={sorted(stages)} names stages outside 0..{S - 1}")
    tabs: Dict[int, torch.Tensor] = {}
    for k in sorted(stages):
        shape = (N, int(steps[k]) + 1)
        t = out.get(k) if out else None
        if t is None:
            t = torch.empty(shape, device=state.device, dtype=torch.float32)
        elif tuple(t.shape) != shape or t.device != state.device:
            raise RuntimeError(f"jitter_tables: out[{k}] must be {list(shape)} on {state.device}, got {list(t.shape)} on {t.device}")
        tabs[k] = t
    u_ptrs = (C.c_void_p * max(S, 1))(*[_lib.dev(tabs[k], f"out[{k}]") if k in tabs and k >= 1 else None for k in range(S)])
    _lib.check(_lib.lib().sn_rm_jitter_tables(state.data_ptr(), N, int(ray_base), S, (C.c_uint32 * max(S, 1))(*[int(t) for t in steps]),
                                              _lib.dev(tabs.get(0), "out[0]"), u_ptrs, 1 if advance else 0, _lib.stream()), "jitter_tables")
    return tabs.get(0), {k: t for k, t in tabs.items() if k >= 1}


class DeviceJitter:
    """The state of sn_rm_jitter_tables' generator on `device`: an int64 [4] tensor (seed, draw, ticket, reserved).  seed=None takes
    64 bits from torch's default CPU generator, so torch.manual_seed still reproduces a run.  `draw` counts the tables drawn: every
    tables(advance=True) call -- on the device, also under graph replay -- moves it by one; (seed, draw) names a table."""

    def __init__(self, device, seed: Optional[int] = None):
        self.state = torch.zeros(4, dtype=torch.int64, device=device)
        if self.state.data_ptr() % 16:
            raise RuntimeError("DeviceJitter: the allocator returned a state that is not 16-byte aligned")
        self.set(seed=self._fresh_seed() if seed is None else seed, draw=0)

    @staticmethod
    def _fresh_seed() -> int:
        lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
        return (hi << 32) | lo

    @staticmethod
    def _i64(v: int) -> int:                                # a uint64 as the int64 with the same bits
        v = int(v) & 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v

    @property
    def device(self):
        return self.state.device

    def set(self, seed: Optional[int] = None, draw: Optional[int] = None) -> "DeviceJitter":
        """Overwrite the seed and / or the draw counter (unsigned 64-bit values; a host write, not for a captured step)."""
        if seed is not None:
            self.state[0:1].copy_(torch.tensor([self._i64(seed)], dtype=torch.int64))
        if draw is not None:
            self.state[1:2].copy_(torch.tensor([self._i64(draw)], dtype=torch.int64))
        return self

    def tables(self, N: int, steps: Sequence[int], ray_base: int = 0, advance: bool = True):
        """(bins0, {k: u_k}) for rays ray_base .. ray_base + N - 1 at the current draw (jitter_tables)."""
        return jitter_tables(self.state, N, steps, ray_base=ray_base, advance=advance)

    def advance(self) -> None:
        """draw + 1 without drawing a table (one one-thread launch)."""
        jitter_tables(self.state, 1, [1], advance=True, want=())

    def state_dict(self) -> Dict[str, int]:
        seed, draw = self.state[:2].tolist()                # (reads the device: one synchronisation)
        return {"seed": seed & 0xFFFFFFFFFFFFFFFF, "draw": draw & 0xFFFFFFFFFFFFFFFF}

    def load_state_dict(self, sd: Dict[str, int]) -> None:
        self.set(seed=sd["seed"], draw=sd["draw"])


class _ray_composite(Function):
    """weights [N,T], rays_t [N,T], raw [N,T,16] (grid_mlp's output), rays_d [N,3] -> (weights_sum [N], depth [N], f_image [N,31]) in one
    kernel (sn_rm_ray_composite; renderer.py:327-347 with colour = cat([geo_feat, SH(d)]), network.py:164-170); differentiable w.r.t.
    weights and raw."""

    @staticmethod
    def forward(ctx, weights, rays_t, raw, rays_d):
        w = weights.detach().contiguous().float()
        tm = rays_t.detach().contiguous().float()
        r = raw.detach().contiguous().float()
        d = rays_d.detach().contiguous().float()
        N, T = w.shape
        assert r.shape == (N, T, 16) and d.shape == (N, 3)
        ws = torch.empty(N, device=w.device, dtype=torch.float32)
        depth = torch.empty(N, device=w.device, dtype=torch.float32)
        f = torch.empty(N, 31, device=w.device, dtype=torch.float32)
        _lib.check(_lib.lib().sn_rm_ray_composite(_lib.dev(w, "weights"), _lib.dev(tm, "rays_t"), _lib.dev(r, "raw"), _lib.dev(d, "rays_d"), N, T,
                                                  _lib.dev(ws, "weights_sum"), _lib.dev(depth, "depth"), _lib.dev(f, "f_image"), _lib.stream()),
                   "ray_composite")
        ctx.save_for_backward(w, tm, r, d)
        ctx.set_materialize_grads(False)
        return ws, depth, f

    @staticmethod
    def backward(ctx, g_ws, g_depth, g_f):
        w, tm, r, d = ctx.saved_tensors
        if g_ws is None and g_depth is None and g_f is None:
            return None, None, None, None
        N, T = w.shape
        c = lambda t: t.contiguous().float() if t is not None else None        # noqa: E731
        g_ws, g_depth, g_f = c(g_ws), c(g_depth), c(g_f)
        gw = torch.empty_like(w)
        gr = torch.empty_like(r)
        _lib.check(_lib.lib().sn_rm_ray_composite_backward(_lib.dev(w, "weights"), _lib.dev(tm, "rays_t"), _lib.dev(r, "raw"), _lib.dev(d, "rays_d"),
                                                           _lib.dev(g_ws, "grad_weights_sum"), _lib.dev(g_depth, "grad_depth"), _lib.dev(g_f, "grad_f_image"),
                                                           N, T, _lib.dev(gw, "grad_weights"), _lib.dev(gr, "grad_raw"), _lib.stream()),
                   "ray_composite_backward")
        return gw, None, gr, None


def ray_composite(weights, rays_t, raw, rays_d):
    return _ray_composite.apply(weights, rays_t, raw, rays_d)


def _proposal_loss_launch(bins, w, ref_bins, ref_w, scale, scale_dev, per_ray_ptr, grad_ptr, what):
    """One stage, one direction (sn_rm_proposal_loss_long): up to 512 samples per ray the arrays of a ray sit in LDS; longer rays get a
    workspace (at most 64 MiB) -- the same kernel arithmetic either way, nothing falls back to torch."""
    N, T, Tr = w.shape[0], w.shape[1], ref_w.shape[1]
    lib = _lib.lib()
    nbytes = 0 if max(T, Tr) <= 512 else int(lib.sn_rm_proposal_loss_workspace_bytes(N, T, Tr, 0 if grad_ptr is None else 1))
    ws = torch.empty((nbytes + 7) // 8, device=w.device, dtype=torch.float64) if nbytes else None
    _lib.check(lib.sn_rm_proposal_loss_long(_lib.dev(bins, "bins"), _lib.dev(w, "weights"), _lib.dev(ref_bins, "ref_bins"), _lib.dev(ref_w, "ref_weights"),
                                            N, T, Tr, float(scale), scale_dev, per_ray_ptr, grad_ptr, ws.data_ptr() if ws is not None else None,
                                            nbytes, _lib.stream()), what)
    if ws is not None:
        ws.record_stream(torch.cuda.current_stream(w.device))


class _proposal_loss_all(Function):
    """The whole inter-level proposal loss (nerf/renderer.py:30-57) as one autograd node: one kernel per proposal stage forward and backward,
    the mean's 1 / (N Tr) and the incoming gradient scalar applied inside the kernels (sn_rm_proposal_loss_scaled)."""

    @staticmethod
    def forward(ctx, ref_bins, ref_weights, *bw):
        ref_bins, ref_w = ref_bins.detach().contiguous().float(), ref_weights.detach().contiguous().float()
        N, Tr = ref_w.shape
        S = len(bw) // 2
        bins = [b.detach().contiguous().float() for b in bw[:S]]
        ws = [w.detach().contiguous().float() for w in bw[S:]]
        per_ray = torch.empty(S, N, device=ref_w.device, dtype=torch.float32)
        scale = 1.0 / float(N * Tr)
        for k in range(S):
            _proposal_loss_launch(bins[k], ws[k], ref_bins, ref_w, scale, None, per_ray[k].data_ptr(), None, "proposal_loss")
        ctx.save_for_backward(ref_bins, ref_w, *bins, *ws)
        ctx.S = S
        return per_ray.sum()

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        ref_bins, ref_w = saved[0], saved[1]
        S = ctx.S
        bins, ws = saved[2:2 + S], saved[2 + S:]
        N, Tr = ref_w.shape
        scale = 1.0 / float(N * Tr)
        g = grad_out.detach().reshape(1).contiguous().float()         # stays on the device: no host sync
        out = []
        for k in range(S):
            gw = torch.empty_like(ws[k])
            _proposal_loss_launch(bins[k], ws[k], ref_bins, ref_w, scale, _lib.dev(g, "grad_out"), None, _lib.dev(gw, "grad_weights"), "proposal_loss_backward")
            out.append(gw)
        return (None, None) + (None,) * S + tuple(out)


def proposal_loss_all(all_bins, all_weights):
    """sum over the proposal stages of proposal_loss_stage(...) against the last entry (renderer.py:30-57), one autograd node."""
    return _proposal_loss_all.apply(all_bins[-1], all_weights[-1], *all_bins[:-1], *all_weights[:-1])


def zeros_f32(shape, device) -> torch.Tensor:
    """torch.zeros(shape) whose fill is a library kernel on the current stream (sn_zero; capturable)."""
    t = torch.empty(shape, device=device, dtype=torch.float32)
    nbytes = t.numel() * 4
    if nbytes % 16 == 0 and t.data_ptr() % 16 == 0 and nbytes > 0:
        _lib.check(_lib.lib().sn_zero(t.data_ptr(), nbytes, _lib.stream()), "zero")
    else:
        t.zero_()
    return t


class _proposal_loss_stage(Function):
    """One proposal stage's term of the inter-level loss (nerf/renderer.py:30-57): mean over rays and final-stage
    intervals of max(w_ref - bound, 0)^2 / (w_ref + 1e-8); differentiable w.r.t. the proposal weights only (bins come
    from sample_pdf, the final stage's bins and weights are detached in the reference)."""

    @staticmethod
    def forward(ctx, bins, weights, ref_bins, ref_weights):
        bins, ref_bins = bins.detach().contiguous().float(), ref_bins.detach().contiguous().float()
        w, ref_w = weights.detach().contiguous().float(), ref_weights.detach().contiguous().float()
        N, T = w.shape
        Tr = ref_w.shape[1]
        per_ray = torch.empty(N, device=w.device, dtype=torch.float32)
        _proposal_loss_launch(bins, w, ref_bins, ref_w, 1.0, None, _lib.dev(per_ray, "loss_per_ray"), None, "proposal_loss")
        ctx.save_for_backward(bins, w, ref_bins, ref_w)
        return per_ray.sum() / float(N * Tr)

    @staticmethod
    def backward(ctx, grad_out):
        bins, w, ref_bins, ref_w = ctx.saved_tensors
        N, T = w.shape
        Tr = ref_w.shape[1]
        gw = torch.empty_like(w)
        _proposal_loss_launch(bins, w, ref_bins, ref_w, 1.0, None, None, _lib.dev(gw, "grad_weights"), "proposal_loss_backward")
        return None, gw * (grad_out / float(N * Tr)), None, None      # no host sync: the scale stays a device scalar


PROPOSAL_LOSS_MAX_T = 1 << 24       # the kernels take any ray (up to 512 samples in LDS, beyond that in a workspace); nerf/renderer.py keeps the torch statement
                                    # for CPU tensors and the tests' comparison (they lower this constant)


def proposal_loss_stage(bins, weights, ref_bins, ref_weights):
    """bins [N,T+1], weights [N,T] of a proposal stage; ref_* of the final stage -> scalar (renderer.py:37-56, one stage)."""
    return _proposal_loss_stage.apply(bins, weights, ref_bins, ref_weights)


class _distort_loss(Function):
    """Mip-NeRF-360 distortion loss of nerf/renderer.py:17-27 (the reference delegates to the third-party
    torch_efficient_distloss.eff_distloss): mean over rays of (1/3) sum w_i^2 d_i + sum_ij w_i w_j |m_i - m_j|;
    value and d/dw from one kernel, the gradient is kept for backward (bins carry no gradient)."""

    @staticmethod
    def forward(ctx, bins, weights):
        bins = bins.detach().contiguous().float()
        w = weights.detach().contiguous().float()
        N, T = w.shape
        per_ray = torch.empty(N, device=w.device, dtype=torch.float32)
        gw = torch.empty_like(w)
        _lib.check(_lib.lib().sn_rm_distort_loss(_lib.dev(bins, "bins"), _lib.dev(w, "weights"), N, T, _lib.dev(per_ray, "loss_per_ray"),
                                                 _lib.dev(gw, "grad_weights"), _lib.stream()), "distort_loss")
        ctx.save_for_backward(gw)
        ctx.n = N
        return per_ray.sum() / float(N)

    @staticmethod
    def backward(ctx, grad_out):
        (gw,) = ctx.saved_tensors
        return None, gw * (grad_out / float(ctx.n))


DISTORT_LOSS_MAX_T = 1 << 24        # any ray (up to 2048 samples in LDS, beyond that read in place); as above


def distort_loss(bins, weights):
    """bins [N,T+1], weights [N,T] -> scalar (renderer.py:17-27)."""
    return _distort_loss.apply(bins, weights)


class _mask_nll(Function):
    """-log(clamp(softmax(logits)[label], eps, 1 - eps)) per ray, value and gradient in one kernel (sn_rm_mask_nll)."""

    @staticmethod
    def forward(ctx, logits, labels, eps):
        shape = logits.shape[:-1]
        lg = logits.reshape(-1, logits.shape[-1]).contiguous().float()
        lb = labels.reshape(-1).contiguous().long()
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
    inc = incoherent.detach().reshape(G, P).contiguous().float()
    if uniform is None:
        uniform = torch.rand(G, P, device=inc.device, dtype=torch.float32)
    u = uniform.detach().reshape(G, P).contiguous().float()
    out = torch.empty(G, int(S), device=inc.device, dtype=torch.int64)
    _lib.check(_lib.lib().sn_rm_ray_pair_select(_lib.dev(inc, "incoherent"), _lib.dev(u, "uniform"), G, P, int(S), _lib.dev(out, "sample_index", torch.int64),
                                                _lib.stream()), "ray_pair_select")
    return out


class _ray_pair_rgb_loss(Function):
    """nerf/trainer.py:276-303 as one kernel (sn_rm_ray_pair_rgb_loss): the scalar loss, and the gradient with respect to `masks` made in the
    same launch and kept for backward (the mean's 1 / n_pairs inside it)."""

    @staticmethod
    def forward(ctx, rgb, masks, sample_index, threshold, exp_weight, epsilon, use_pred_logistics, from_logits):
        m = masks.detach().contiguous().float()
        G, P, K = m.shape
        c = rgb.detach().reshape(G, P, 3).contiguous().float()
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


def _mask_rows(masks, labels):
    m = masks.detach().reshape(-1, masks.shape[-1]).contiguous().float()
    lb = labels.detach().reshape(-1).contiguous().long()
    if lb.shape[0] != m.shape[0]:
        raise RuntimeError(f"{lb.shape[0]} labels for {m.shape[0]} mask rows")
    return m, lb


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
    rows = torch.as_tensor(index, device=m.device).detach().reshape(-1).contiguous().long()
    cols = inds.detach().reshape(-1).contiguous().long()
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


def _image_rows(t, name, N):
    """An [N, >=3] float32 image whose rows are `stride` floats apart (the packed [N,5] render buffer's image columns are read in place)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if t.dim() != 2:
        t = t.reshape(-1, t.shape[-1])
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < 3 or t.shape[1] < 3:
        t = t[:, :3].float().contiguous()
    if t.shape[0] != N:
        raise RuntimeError(f"{name}: {t.shape[0]} rows for {N} pixels")
    return t, t.data_ptr(), t.stride(0)


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
    lg = logits.detach().reshape(-1, K).contiguous().float()
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
            cm = color_map.detach().reshape(-1, 3).contiguous().float()
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
    res, ptr = {} if out is None else out, {}
    for name, (shape, dtype) in shapes.items():
        if name not in want:
            ptr[name] = None
            continue
        t = res.get(name)
        if t is None:
            t = torch.empty(shape, device=dev, dtype=dtype)
            res[name] = t
        elif tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"mask_output: out[{name!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, "
                               f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        ptr[name] = _lib.dev(t, name, dtype)
    _lib.check(_lib.lib().sn_rm_mask_output(lg_ptr, N, K, img_ptr, img_stride, cm_ptr, n_colors, _lib.MASK_OUT_MODES[mode], int(render_id), float(alpha), bg_ptr,
                                            ptr["probs"], ptr["instance_id"], ptr["confidence"], ptr["rgb"], ptr["rgb8"], _lib.stream()), "mask_output")
    return res


EVAL_RECORD_BYTES = C.sizeof(_lib.EvalRecord)


def eval_record(device) -> torch.Tensor:
    """A zeroed sn_eval_record on the device (as int64 words; read it with `read_eval_record`)."""
    return torch.zeros(EVAL_RECORD_BYTES // 8, device=device, dtype=torch.int64)


def eval_workspace(device) -> torch.Tensor:
    """The zero-at-rest scratch of mask_eval_accumulate / image_sqerr_accumulate (one per stream)."""
    return torch.zeros(_lib.MASK_EVAL_WORKSPACE_BYTES // 8, device=device, dtype=torch.int64)


def read_eval_record(record: torch.Tensor) -> dict:
    """The record's fields on the host (this is the host read: it synchronises)."""
    raw = record.detach().cpu().numpy().tobytes()
    r = _lib.EvalRecord.from_buffer_copy(raw)
    return {"nll_mean_sum": r.nll_mean_sum, "miou_sum": r.miou_sum, "mse_sum": r.mse_sum, "psnr_sum": r.psnr_sum, "images": int(r.images),
            "rgb_images": int(r.rgb_images), "inter": np.array(r.inter[:], dtype=np.uint64), "pred": np.array(r.pred[:], dtype=np.uint64),
            "truth": np.array(r.truth[:], dtype=np.uint64)}


def _record_ptrs(record, workspace):
    if record.dtype != torch.int64 or record.numel() * 8 < EVAL_RECORD_BYTES:
        raise RuntimeError("record must come from raymarching.eval_record()")
    if workspace.dtype != torch.int64 or workspace.numel() * 8 < _lib.MASK_EVAL_WORKSPACE_BYTES:
        raise RuntimeError("workspace must come from raymarching.eval_workspace()")
    return _lib.dev(record, "record", torch.int64), _lib.dev(workspace, "workspace", torch.int64)


def mask_eval_accumulate(logits, labels, record: torch.Tensor, workspace: torch.Tensor, eps: float = 1e-6, num_classes: Optional[int] = None) -> None:
    """eval_step's mask branch + the loss and mIoU meters for one image, in one launch and without a host read (sn_rm_mask_eval_accumulate;
    nerf/trainer.py:599-627, 1603-1604, nerf/metrics.py:165-179): logits [..., K], labels [...] (-1: unlabelled) -> `record` gets the image's
    mean NLL over its labelled pixels (0 when there is none) and its mean IoU of (argmax id, label) over num_classes >= K classes
    (default K) added, and its class counts stored."""
    m, lb = _mask_rows(logits, labels)
    N, K = m.shape
    m_ptr, lb_ptr = _lib.dev(m, "logits"), _lib.dev(lb, "labels", torch.int64)
    rec, ws = _record_ptrs(record, workspace)
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
    rec, ws = _record_ptrs(record, workspace)
    _lib.check(_lib.lib().sn_rm_image_sqerr_accumulate(p_ptr, p_stride, t_ptr, t_stride, N, rec, ws, _lib.stream()), "image_sqerr_accumulate")


SSIM_RECORD_BYTES = C.sizeof(_lib.SsimRecord)


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
    if record.dtype != torch.int64 or record.numel() * 8 < SSIM_RECORD_BYTES:
        raise RuntimeError("record must come from raymarching.ssim_record()")
    if workspace.dtype != torch.int64 or workspace.numel() * 8 < _lib.SSIM_WORKSPACE_BYTES:
        raise RuntimeError("workspace must come from raymarching.ssim_workspace()")
    rec, ws = _lib.dev(record, "record", torch.int64), _lib.dev(workspace, "workspace", torch.int64)
    _lib.check(_lib.lib().sn_rm_image_ssim_accumulate(rows[0].data_ptr(), rows[0].stride(0), rows[1].data_ptr(), rows[1].stride(0), H, W,
                                                      0.0 if data_range is None else float(data_range), rec, ws, _lib.stream()),
               "image_ssim_accumulate")


def _feature_rows(samvit, h: int, w: int):
    """The render's `samvit` ([h*w, C] or [h, w, C]) as h*w rows of C float32, read in place where its rows are contiguous."""
    if not samvit.is_cuda:
        raise RuntimeError("samvit must be a CUDA tensor")
    t = samvit.detach()
    if t.dim() != 2:
        t = t.reshape(-1, t.shape[-1])
    if t.shape[0] != h * w:
        raise RuntimeError(f"samvit: {t.shape[0]} rows for a {h} x {w} feature render")
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.float().contiguous()
    return t


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


_distill_workspaces: Dict[tuple, torch.Tensor] = {}


def _distill_workspace(device, stream: int, nbytes: int) -> torch.Tensor:
    """The operator's workspace, one per (device, stream): zeroed when it is made (the kernels leave its fixed part zeroed) and grown on demand."""
    key = (device.index, stream)
    ws = _distill_workspaces.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _distill_workspaces[key] = torch.zeros((nbytes + 7) // 8, device=device, dtype=torch.int64)
    return ws


class _feature_distill_loss(Function):
    """trainer.py:540-550 as one operator (sn_rm_feature_distill_loss): the scalar loss, and the gradient with respect to `samvit` made in
    the same call (`scale` inside it) and kept for backward, which is one multiply."""

    @staticmethod
    def forward(ctx, samvit, h, w, target, scale, want_resized):
        f = _feature_rows(samvit, h, w)
        C_ = f.shape[1]
        tgt, Ho, Wo = _feature_target(target, C_)
        l = _lib.lib()
        scale_dev = scale if isinstance(scale, torch.Tensor) else None
        if scale_dev is not None:
            scale_dev = scale_dev.detach().reshape(-1)[:1].float().contiguous()
        nbytes = l.sn_rm_feature_distill_workspace_bytes(h, w, C_, Ho, Wo)
        if nbytes == 0:
            _lib.check(-2, "feature_distill_loss")
        ws = _distill_workspace(f.device, _lib.stream(), nbytes)
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
    f = _feature_rows(samvit, h, w)
    Ho, Wo = (h, w) if size is None else (int(size[0]), int(size[1]))
    out = torch.empty(1, f.shape[1], Ho, Wo, device=f.device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_feature_map(f.data_ptr(), f.stride(0), h, w, f.shape[1], Ho, Wo, _lib.dev(out, "out"), _lib.stream()), "feature_map")
    return out


# ---- the loss tail of the RGB training step (rgb_loss.hip) ------------------------------------------------------------------------------
_rgb_loss_workspaces: Dict[tuple, torch.Tensor] = {}


def _rgb_loss_workspace(device, stream: int) -> torch.Tensor:
    """The operator's workspace, one per (device, stream): zeroed when it is made, left zeroed by every launch."""
    key = (device.index, stream)
    ws = _rgb_loss_workspaces.get(key)
    if ws is None:
        ws = _rgb_loss_workspaces[key] = torch.zeros(_lib.RGB_LOSS_WORKSPACE_BYTES // 8, device=device, dtype=torch.int64)
    return ws


def _rgb_rows(t, name, N, channels):
    """An [N, >= channels] float32 tensor whose rows are read in place where they are contiguous (a column slice of a wider buffer)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if t.dim() < 2 or t.shape[-1] not in channels:
        raise RuntimeError(f"{name} must be [N,{' or '.join(str(c) for c in channels)}], got {tuple(t.shape)}")
    if t.dim() != 2:
        t = t.reshape(-1, t.shape[-1])
    if t.shape[0] != N:
        raise RuntimeError(f"{name}: {t.shape[0]} rows for {N} rays")
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.float().contiguous()
    return t


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
        im = _rgb_rows(image, "image", N, (3,))
        tr = _rgb_rows(truth, "truth", N, (3, 4))
        if not torch.is_tensor(weights_sum) or not weights_sum.is_cuda:
            raise RuntimeError("weights_sum must be a CUDA tensor")
        if weights_sum.numel() != N:
            raise RuntimeError(f"weights_sum: {weights_sum.numel()} values for {N} rays")
        w = weights_sum.detach().reshape(-1).float().contiguous()
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
            bg_t = bg.detach().reshape(-1, 3).float().contiguous()
        else:
            bg_value = float(bg)
        extras = []
        for e, name in ((extra0, "extras[0]"), (extra1, "extras[1]")):
            if e is None:
                extras.append(None)
                continue
            if not torch.is_tensor(e) or not e.is_cuda or e.numel() != 1:
                raise RuntimeError(f"{name} must be a one-element CUDA tensor")
            extras.append(e.detach().reshape(1).float().contiguous())
        dev_ = im.device
        new = lambda *shape: torch.empty(*shape, device=dev_, dtype=torch.float32)   # noqa: E731
        record = new(4)
        pred = new(N, 3) if want_pred else None
        gt = new(N, 3) if want_pred else None
        g_im = new(N, 3) if ctx.needs_input_grad[0] else None
        g_ws = new(N) if ctx.needs_input_grad[1] else None
        ws = _rgb_loss_workspace(dev_, _lib.stream())
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


# ---- 3D point prompts: lift, store, projection into views, decode overlays (prompts.hip) -----------------------------------------------
def _pixel_values(t, name, n):
    """n float32 values a constant number of floats apart, read in place: a contiguous tensor (1), or a column of the packed [N,5] render
    buffer such as buf[:, 3] or buf[:, 3].view(H, W) (5).  Anything else is packed first."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if t.numel() != n:
        raise RuntimeError(f"{name}: {t.numel()} values for {n} pixels")
    uniform = t.dim() >= 1 and t.stride(-1) >= 1 and all(t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 1))
    if not uniform:
        t = t.contiguous().reshape(-1)
    return t, t.data_ptr(), t.stride(-1)


def _i32(t, name, shape=None):
    """A contiguous int32 tensor on the device (labels, flags, coordinates; bool and int64 are converted by a device-side copy)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _outputs(op, specs, want, out, dev):
    """The `out=` idiom of mask_output: name -> (shape, dtype); returns (dict of tensors, dict of pointers, None for an unwanted one)."""
    res, ptr = {} if out is None else out, {}
    for name, (shape, dtype) in specs.items():
        if name not in want:
            ptr[name] = None
            continue
        t = res.get(name)
        if t is None:
            t = res[name] = torch.empty(shape, device=dev, dtype=dtype)
        elif tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"{op}: out[{name!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, "
                               f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        ptr[name] = _lib.dev(t, name, dtype)
    return res, ptr


def points_lift(pixels, rays_o, rays_d, depth, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Clicked pixels -> 3D points (sn_rm_points_lift; nerf/trainer.py:803-809): pixels [M,2] (x, y) on the device, rays_o / rays_d [H*W,3],
    depth H*W values ([H,W], or the depth column of the packed render buffer read in place) -> [M,3] = o + d * depth.  A click outside
    the image gives NaN."""
    H, W = int(H), int(W)
    px = _i32(pixels.reshape(-1, 2), "pixels")
    M = px.shape[0]
    ro, rd = rays_o.detach().reshape(-1, 3).contiguous().float(), rays_d.detach().reshape(-1, 3).contiguous().float()
    ro_ptr, rd_ptr = _lib.dev(ro, "rays_o"), _lib.dev(rd, "rays_d")
    if ro.shape[0] != H * W or rd.shape[0] != H * W:
        raise RuntimeError(f"points_lift: {ro.shape[0]} / {rd.shape[0]} rays for a {H} x {W} image")
    d, d_ptr, d_stride = _pixel_values(depth, "depth", H * W)
    if out is None:
        out = torch.empty(M, 3, device=px.device, dtype=torch.float32)
    elif tuple(out.shape) != (M, 3):
        raise RuntimeError(f"points_lift: out must be [{M},3], got {tuple(out.shape)}")
    _lib.check(_lib.lib().sn_rm_points_lift(px.data_ptr(), M, ro_ptr, rd_ptr, d_ptr, d_stride, H, W, _lib.dev(out, "out"), _lib.stream()), "points_lift")
    return out


def point_store(device, capacity: int = 256) -> Dict[str, torch.Tensor]:
    """An empty fixed-capacity store of remembered points on the device: 'xyz' [cap,3], 'labels' / 'crucial' [cap] int32, 'count' [1] int32
    and the 'status' [4] int32 record of point_store_update."""
    cap = int(capacity)
    if not 1 <= cap <= _lib.PROMPT_MAX_POINTS:
        raise ValueError(f"point_store: capacity {capacity} outside 1..{_lib.PROMPT_MAX_POINTS}")
    z = lambda *s, dt=torch.int32: torch.zeros(*s, device=device, dtype=dt)
    return {"xyz": z(cap, 3, dt=torch.float32), "labels": z(cap), "crucial": z(cap), "count": z(1), "status": z(4)}


def point_store_update(store: Dict[str, torch.Tensor], point, label, dist_thresh: float = 0.01) -> None:
    """The add-or-remove rule of the remembered points for one new point (sn_rm_point_store_update; trainer.py:812-834), one launch, no
    host read: point [3] (or [1,3]) on the device; label: an int, or a one-element device tensor.  store['status'] = {0 first / 1 appended
    / 2 removed / 3 full, count before, count after, overflow (only ever set)}."""
    xyz = store["xyz"]
    cap = xyz.shape[0]
    p = point.detach().reshape(-1).contiguous().float()
    p_ptr = _lib.dev(p, "point")
    if p.numel() != 3:
        raise RuntimeError(f"point_store_update: one point of 3 coordinates, got {tuple(point.shape)}")
    if torch.is_tensor(label):
        lb = _i32(label.reshape(-1)[:1], "label")
    else:
        lb = torch.empty(1, device=xyz.device, dtype=torch.int32).fill_(int(label))      # a fill, not a copy: it can be captured
    _lib.check(_lib.lib().sn_rm_point_store_update(_lib.dev(xyz, "xyz"), _lib.dev(store["labels"], "labels", torch.int32),
                                                   _lib.dev(store["crucial"], "crucial", torch.int32), _lib.dev(store["count"], "count", torch.int32),
                                                   cap, p_ptr, lb.data_ptr(), float(dist_thresh), _lib.dev(store["status"], "status", torch.int32),
                                                   _lib.stream()), "point_store_update")


def reference_resize_ratio(H: int, W: int) -> float:
    """trainer.py:871 / :973: the factor into SAM's 1024-pixel frame."""
    return 1024 / W if W > H else 1024 / H


def points_project(points, labels, poses, intrinsics, depth, H: int, W: int, crucial=None, n_points=None, depth_tol: float = 0.05,
                   crucial_count: int = 0, valid_threshold: int = 0, resize_ratio: Optional[float] = None,
                   want: Sequence[str] = ("cam", "uv", "state"), out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """The remembered points in V views, one launch and no host read (sn_rm_points_project; trainer.py:838-875, 931-976): points [N,3],
    labels [N], crucial [N] or None, n_points: a one-element int32 device tensor (a store's count) or None; poses [V,4,4] (or [4,4])
    cam2world, intrinsics [4] or [V,4]; depth V*H*W values ([V,H,W], [H,W], or the depth column of the packed render buffer read in place).
    Returns 'coords' [V,N,2] / 'labels' [V,N] / 'kept_index' [V,N] (the kept points first, in their order; behind them 0 / -1 / -1),
    'sam_coords' / 'overlay_coords' [V,N,2] (resize_ratio None: the reference's 1024 / max(H, W); 0: left out), 'counts' [V,4] = {on screen,
    kept, crucial kept, is_valid}, and of `want`: 'cam' [V,N,3], 'uv' [V,N,2], 'state' [V,N] (0 off screen, 1 occluded, 2 kept)."""
    H, W = int(H), int(W)
    unknown = set(want) - {"cam", "uv", "state"}
    if unknown:
        raise ValueError(f"points_project: unknown outputs {sorted(unknown)}")
    pts = points.detach().reshape(-1, 3).contiguous().float()
    pts_ptr = _lib.dev(pts, "points")
    N, dev = pts.shape[0], pts.device
    lb = _i32(labels.reshape(-1), "labels", (N,))
    cr = None if crucial is None else _i32(crucial.reshape(-1), "crucial", (N,))
    npts = None if n_points is None else _i32(n_points.reshape(-1)[:1], "n_points", (1,))
    ps = poses.detach().reshape(-1, 16).contiguous().float()
    ps_ptr = _lib.dev(ps, "poses")
    V = ps.shape[0]
    ks = intrinsics.detach().reshape(-1, 4).contiguous().float()
    ks_ptr = _lib.dev(ks, "intrinsics")
    if ks.shape[0] not in (1, V):
        raise RuntimeError(f"points_project: {ks.shape[0]} intrinsics for {V} views (1 or V)")
    d, d_ptr, d_stride = _pixel_values(depth, "depth", V * H * W)
    ratio = reference_resize_ratio(H, W) if resize_ratio is None else float(resize_ratio)
    names = ["coords", "labels", "kept_index", "counts"] + (["sam_coords", "overlay_coords"] if ratio > 0 else []) + list(want)
    i32, f32 = torch.int32, torch.float32
    specs = {"coords": ((V, N, 2), i32), "labels": ((V, N), i32), "kept_index": ((V, N), i32), "sam_coords": ((V, N, 2), i32),
             "overlay_coords": ((V, N, 2), i32), "cam": ((V, N, 3), f32), "uv": ((V, N, 2), f32), "state": ((V, N), i32), "counts": ((V, 4), i32)}
    res, ptr = _outputs("points_project", specs, names, out, dev)
    _lib.check(_lib.lib().sn_rm_points_project(pts_ptr, lb.data_ptr(), None if cr is None else cr.data_ptr(), N, None if npts is None else npts.data_ptr(),
                                               ps_ptr, V, ks_ptr, ks.shape[0], d_ptr, d_stride, H, W, float(depth_tol), int(crucial_count),
                                               int(valid_threshold), ratio, ptr["coords"], ptr["labels"], ptr["kept_index"], ptr["sam_coords"],
                                               ptr["overlay_coords"], ptr["cam"], ptr["uv"], ptr["state"], ptr["counts"], _lib.stream()), "points_project")
    return res


def prompt_overlay(image, coords, labels, H: int, W: int, count=None, masks=None, scores=None, mask_index: int = 0, radius: int = 2,
                   alpha: float = 0.7, want: Sequence[str] = ("rgb", "pred_mask"), out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """decode_step's tail in one launch (sn_rm_prompt_overlay; trainer.py:979-991, nerf/utils.py:23-29, 80-98): image [H*W,3] / [H,W,3]
    (rows may be strided: the packed render buffer is read in place), coords [N,2] (x, y) and labels [N] int32, count: a one-element int32
    device tensor or None (= N); masks [M,H,W] bool / uint8 or None, scores [M] on the device (the first score above the running maximum,
    which starts at 0) or None with a fixed mask_index.  Returns of `want`: 'rgb' [H,W,3] (the selected mask blended in red at 1 - alpha,
    the points as squares: green for label 0, red otherwise, drawn with the reference's Python-slice bounds, the last point on top),
    'rgb8' [H,W,3] uint8, 'pred_mask' [H,W] bool (the selected mask), and always 'selected' [1] int32.  count == 0: the image unchanged,
    an empty mask, selected -1."""
    H, W = int(H), int(W)
    unknown = set(want) - {"rgb", "rgb8", "pred_mask"}
    if unknown:
        raise ValueError(f"prompt_overlay: unknown outputs {sorted(unknown)}")
    img, img_ptr, img_stride = _image_rows(image, "image", H * W)
    dev = img.device
    xy = _i32(coords.reshape(-1, 2), "coords")
    N = xy.shape[0]
    lb = _i32(labels.reshape(-1), "labels", (N,))
    cnt = None if count is None else _i32(count.reshape(-1)[:1], "count", (1,))
    m, M, sc = None, 0, None
    if masks is not None:
        if not masks.is_cuda:
            raise RuntimeError("masks must be a CUDA tensor")
        m = masks.detach().reshape(-1, H, W).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8)
        M = m.shape[0]
        if scores is not None:
            sc = scores.detach().reshape(-1).contiguous().float()
            if not sc.is_cuda:
                raise RuntimeError("scores must be a CUDA tensor")
            if sc.shape[0] != M:
                raise RuntimeError(f"prompt_overlay: {sc.shape[0]} scores for {M} masks")
    specs = {"rgb": ((H, W, 3), torch.float32), "rgb8": ((H, W, 3), torch.uint8), "pred_mask": ((H, W), torch.bool), "selected": ((1,), torch.int32)}
    res, ptr = _outputs("prompt_overlay", specs, list(want) + ["selected"], out, dev)
    _lib.check(_lib.lib().sn_rm_prompt_overlay(img_ptr, img_stride, H, W, None if m is None else m.data_ptr(), M, None if sc is None else sc.data_ptr(),
                                               int(mask_index), xy.data_ptr(), lb.data_ptr(), N, None if cnt is None else cnt.data_ptr(), int(radius),
                                               float(alpha), ptr["rgb"], ptr["rgb8"], ptr["pred_mask"], ptr["selected"], _lib.stream()), "prompt_overlay")
    return res


class _composite(Function):
    """out[n,k] = sum_t w[n,t] * v[n,t,k]."""

    @staticmethod
    def forward(ctx, weights, values):
        weights = weights.contiguous().float()
        values = values.contiguous().float()
        N, T = weights.shape
        K = values.shape[-1]
        out = torch.empty(N, K, device=values.device, dtype=torch.float32)
        _lib.check(_lib.lib().sn_rm_composite(_lib.dev(weights, "weights"), _lib.dev(values, "values"), N, T, K,
                                              _lib.dev(out, "out"), _lib.stream()), "composite")
        ctx.save_for_backward(weights, values)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        weights, values = ctx.saved_tensors
        N, T = weights.shape
        K = values.shape[-1]
        grad_out = grad_out.contiguous().float()
        gv = gw = None
        if ctx.needs_input_grad[1]:
            gv = torch.empty_like(values)
            _lib.check(_lib.lib().sn_rm_composite_backward(_lib.dev(weights, "weights"), _lib.dev(grad_out, "grad_out"), N, T, K,
                                                           _lib.dev(gv, "grad_values"), _lib.stream()), "composite_backward")
        if ctx.needs_input_grad[0]:
            gw = (values * grad_out.unsqueeze(1)).sum(-1)
        return gw, gv


# ---- a training batch drawn on the device (collate.hip) ---------------------------------------------------------------------------------
def _f32_rows(t, name, cols=None):
    """A contiguous float32 [rows, cols] tensor on the device, read in place (nothing is copied: these are dataset or static tensors)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 tensor, got {t.dtype}{'' if t.is_contiguous() else ' (not contiguous)'}")
    t = t.detach().reshape(-1, cols) if cols is not None else t.detach()
    return t


def weighted_draw(weights, expo, n: int, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                  row_u: Optional[torch.Tensor] = None, row_index: Optional[torch.Tensor] = None):
    """Weighted sampling without replacement from caller-supplied exponential variates (sn_rm_weighted_draw; torch.multinomial's own
    exponential race, utils.py:218, :248): weights [R,C], expo [R,C] (e.g. torch.empty(R, C).exponential_()) -> (out [R,n] int64, status [1]
    int32).  Per row the n cells with the smallest expo / weights, ties to the smaller cell, in ASCENDING CELL ORDER (torch: key order).  A
    cell with weight <= 0 or NaN, or with a key that is not finite, is never drawn; a row with fewer than n such cells gets -1 in its tail
    and sets the sticky status word (torch raises).  row_u [R] in [0,1): row r draws from row min(int(row_u[r] * M), M - 1) of weights [M,C]
    (the cameras of the local patches, chosen on the device by the same formula as collate_gather's); row_index [R] int64 on the device:
    row r draws from that row of weights [M,C] (a single-image batch's image index).  out / status: static tensors to write into.  One launch, nothing read on the host."""
    w, e = _f32_rows(weights, "weights"), _f32_rows(expo, "expo")
    if w.dim() != 2 or e.dim() != 2 or w.shape[1] != e.shape[1]:
        raise RuntimeError(f"weighted_draw: weights {tuple(w.shape)} and expo {tuple(e.shape)} must be [rows, C] with one C")
    R, Cn, n = e.shape[0], e.shape[1], int(n)
    M = w.shape[0]
    ru_ptr = ri_ptr = None
    if row_index is not None:
        if row_u is not None:
            raise RuntimeError("weighted_draw: give row_u or row_index, not both")
        ri = row_index.detach().reshape(-1)
        ri_ptr = _lib.dev(ri, "row_index", torch.int64)
        if ri.numel() != R:
            raise RuntimeError(f"weighted_draw: row_index has {ri.numel()} entries for {R} rows")
    elif row_u is None:
        if M != R:
            raise RuntimeError(f"weighted_draw: {M} rows of weights for {R} rows of expo (give row_u or row_index to draw from chosen rows)")
    else:
        ru = _f32_rows(row_u, "row_u")
        if ru.numel() != R:
            raise RuntimeError(f"weighted_draw: row_u has {ru.numel()} entries for {R} rows")
        ru_ptr = ru.data_ptr()
    if out is None:
        out = torch.empty(R, max(n, 0), device=w.device, dtype=torch.int64)
    elif tuple(out.shape) != (R, n):
        raise RuntimeError(f"weighted_draw: out must be [{R},{n}], got {tuple(out.shape)}")
    if status is None:
        status = torch.zeros(1, device=w.device, dtype=torch.int32)
    _lib.check(_lib.lib().sn_rm_weighted_draw(w.data_ptr(), e.data_ptr(), R, Cn, n, ru_ptr, ri_ptr, M, _lib.dev(out, "out", torch.int64),
                                              _lib.dev(status, "status", torch.int32), _lib.stream()), "weighted_draw")
    return out, status


COLLATE_OUTPUTS = {"rays_o": (3, torch.float32), "rays_d": (3, torch.float32), "index": (1, torch.int64), "i": (1, torch.int64),
                   "j": (1, torch.int64), "inds_coarse": (1, torch.int64), "images": (None, torch.float32), "masks": (None, None),
                   "error_maps": (1, torch.float32), "cam_near_far": (2, torch.float32), "poses": (16, torch.float32),
                   "intrinsics": (4, torch.float32)}


def _row_strided(t, name, rows, width, dtype):
    """(pointer, row stride in elements) of an output written in place: [rows] or [rows, >= width] with unit column stride -- a contiguous
    tensor or columns of a wider buffer (buf[:, 3:6], buf[:, 7])."""
    if not t.is_cuda:
        raise RuntimeError(f"out[{name!r}] must be a CUDA tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"out[{name!r}] must be a {dtype} tensor, got {t.dtype}")
    if t.dim() == 1 and width == 1:
        ok, stride = t.shape[0] == rows, t.stride(0)
    else:
        ok = t.dim() == 2 and t.shape[0] == rows and t.shape[1] == width and (t.stride(1) == 1 or width == 1)
        stride = t.stride(0) if t.dim() == 2 else 0
    if not ok or (rows > 1 and stride < width):
        raise RuntimeError(f"out[{name!r}] must be [{rows},{width}] with unit column stride and rows that do not overlap, got {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), max(int(stride), width)


def collate_gather(poses, intrinsics, H: int, W: int, u=None, cells=None, index=0, images=None, masks=None, error_map=None, cam_near_far=None,
                   error_map_size: int = 0, coarse_size: Optional[int] = None, ul=None, centres=None, patch_size: int = 1,
                   out: Optional[Dict[str, torch.Tensor]] = None, want: Optional[Sequence[str]] = None) -> Dict[str, torch.Tensor]:
    """Draw -> rays + supervision in one launch (sn_rm_collate_gather; provider.py:908-1068, utils.py:209-300), the dataset tensors read in
    place: poses [M,4,4], intrinsics [1|M,4], images [M,H,W,3|4] uint8, masks [M,H,W,Cm] (uint8 / float32 / int64 ...: copied as raw
    bytes), error_map [M,S*S] with S = error_map_size, cam_near_far [M,2].
      main part: u [N,3] in [0,1) -> camera, row, column per ray (random_image_batch); or cells [N] (weighted_draw over image `index`'s
      error-map row; index: an int or a one-element int64 device tensor) with u [N,2]: a pixel inside each drawn cell;
      local part: ul [L] and centres [L] (weighted_draw(error_map, expo, 1, row_u=ul)): L patches of patch_size^2 rays behind the main part.
    Outputs (COLLATE_OUTPUTS) over the N + L patch_size^2 rays, 'images' over the first N: those named in `want` are allocated, those given
    in `out` are written in place -- [rows, width] or [rows] tensors that may be columns of a wider buffer (row stride = its width).
    Default: every output the given dataset tensors allow.  inds_coarse: the drawn cell in error-map mode, else the pixel's cell in a map of
    coarse_size (default error_map_size, or H without one, as collate_rays)."""
    H, W = int(H), int(W)
    P = _f32_rows(poses, "poses", 16)
    K = _f32_rows(intrinsics, "intrinsics", 4)
    dev, M = P.device, P.shape[0]
    d = _lib.CollateDesc()
    keep = []
    d.poses, d.intrinsics, d.M, d.n_intrinsics, d.H, d.W = P.data_ptr(), K.data_ptr(), M, K.shape[0], H, W
    S = int(error_map_size)
    d.S, d.coarse_size = S, int(coarse_size) if coarse_size is not None else (S if S > 0 else H)
    avail = {"rays_o", "rays_d", "index", "i", "j", "inds_coarse", "poses", "intrinsics"}
    widths = {k: v[0] for k, v in COLLATE_OUTPUTS.items()}
    dtypes = {k: v[1] for k, v in COLLATE_OUTPUTS.items()}
    if images is not None:
        if images.dim() != 4 or tuple(images.shape[:3]) != (M, H, W):
            raise RuntimeError(f"collate_gather: images must be [{M},{H},{W},3|4], got {tuple(images.shape)}")
        d.images, d.image_channels = _lib.dev(images, "images", torch.uint8), images.shape[3]
        widths["images"] = images.shape[3]
        avail.add("images")
    if masks is not None:
        if masks.dim() != 4 or tuple(masks.shape[:3]) != (M, H, W):
            raise RuntimeError(f"collate_gather: masks must be [{M},{H},{W},C], got {tuple(masks.shape)}")
        d.masks, d.mask_channels, d.mask_elem_bytes = _lib.dev(masks, "masks", None), masks.shape[3], masks.element_size()
        widths["masks"], dtypes["masks"] = masks.shape[3], masks.dtype
        avail.add("masks")
    if error_map is not None:
        if S < 1 or error_map.numel() != M * S * S:
            raise RuntimeError(f"collate_gather: error_map must hold {M} x {S}^2 values (error_map_size), got {tuple(error_map.shape)}")
        d.error_map = _f32_rows(error_map, "error_map").data_ptr()
        avail.add("error_maps")
    if cam_near_far is not None:
        d.cam_near_far = _f32_rows(cam_near_far, "cam_near_far", 2).data_ptr()
        if cam_near_far.numel() != 2 * M:
            raise RuntimeError(f"collate_gather: cam_near_far must be [{M},2], got {tuple(cam_near_far.shape)}")
        avail.add("cam_near_far")
    N = 0
    if u is not None:
        uu = _f32_rows(u, "u")
        if cells is not None:
            cl = cells.detach().reshape(-1)
            N = cl.shape[0]
            d.cells, d.mode = _lib.dev(cl, "cells", torch.int64), _lib.COLLATE_ERROR_MAP
            if torch.is_tensor(index):
                d.index_dev = _lib.dev(index, "index", torch.int64)
            else:
                d.index = int(index)
            cols = 2
        else:
            N, cols = uu.shape[0], 3
        if uu.dim() != 2 or tuple(uu.shape) != (N, cols):
            raise RuntimeError(f"collate_gather: u must be [{N},{cols}], got {tuple(uu.shape)}")
        d.u = uu.data_ptr()
        keep.append(uu)
    elif cells is not None:
        raise RuntimeError("collate_gather: cells without u (the position inside each drawn cell)")
    d.N = N
    L, p = 0, int(patch_size)
    if ul is not None or centres is not None:
        if ul is None or centres is None:
            raise RuntimeError("collate_gather: the local part needs both ul and centres")
        lu, cen = _f32_rows(ul, "ul").reshape(-1), centres.detach().reshape(-1)
        L = lu.shape[0]
        if cen.shape[0] != L:
            raise RuntimeError(f"collate_gather: {cen.shape[0]} centres for {L} patches")
        d.ul, d.centres = lu.data_ptr(), _lib.dev(cen, "centres", torch.int64)
        keep += [lu, cen]
    d.L, d.p = L, p
    total = N + L * p * p
    res = {} if out is None else out
    unknown = (set(res) | set(want or ())) - set(COLLATE_OUTPUTS)
    if unknown:
        raise ValueError(f"collate_gather: unknown outputs {sorted(unknown)}; known: {sorted(COLLATE_OUTPUTS)}")
    names = set(res) | (set(want) if want is not None else (avail if out is None else set()))
    missing = names - avail
    if missing:
        raise RuntimeError(f"collate_gather: outputs {sorted(missing)} need the dataset tensor they are gathered from")
    for name in sorted(names):
        rows = N if name == "images" else total
        t = res.get(name)
        if t is None:
            shape = (rows,) if widths[name] == 1 and name != "masks" else (rows, widths[name])
            t = res[name] = torch.empty(shape, device=dev, dtype=dtypes[name])
        ptr, stride = _row_strided(t, name, rows, widths[name], dtypes[name])
        field = name if name in ("rays_o", "rays_d", "inds_coarse") else name + "_out"
        setattr(d, field, ptr)
        setattr(d, name + "_stride", stride)
    _lib.check(_lib.lib().sn_rm_collate_gather(C.byref(d), _lib.stream()), "collate_gather")
    return res


def composite(weights, values):
    """weights [N,T], values [N,T,K] or [N,T] -> [N,K] or [N]."""
    if values.dim() == 2:
        return _composite.apply(weights, values.unsqueeze(-1)).squeeze(-1)
    return _composite.apply(weights, values)


# --------------------------------------------------------------------------------------------
# fused renderer
# --------------------------------------------------------------------------------------------
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


def grid_composite(weights: torch.Tensor, xyzs: torch.Tensor, encoder, bound: float = 1.0, tile_w: int = 0,
                   table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """composite(weights, encoder(xyzs, bound)) in one kernel (renderer.py:301-302 + 361): [N,T], [N,T,3] -> [N, L*C].
    Inference only: no autograd graph is recorded (training uses encoder(...) + composite(...))."""
    N, T = weights.shape
    assert xyzs.shape == (N, T, 3), f"xyzs {tuple(xyzs.shape)} does not match weights {tuple(weights.shape)}"
    L = _lib.lib()
    emb = (encoder.embeddings if table is None else table).detach()
    w = weights.detach().contiguous().float()
    x = xyzs.detach().contiguous().float()
    out = torch.empty(N, encoder.output_dim, device=w.device, dtype=torch.float32)
    desc = _lib.GridDesc()
    _fill_grid(desc, encoder, emb.contiguous())
    _lib.check(L.sn_rm_grid_composite(_lib.dev(x, "xyzs"), _lib.dev(w, "weights"), N, T, float(bound), C.byref(desc),
                                      int(tile_w), _lib.dev(out, "out"), _lib.stream()), "sn_rm_grid_composite")
    return out


FP16_SPLIT_LIMIT = 65504.0 * 0.5      # split-fp16 operands must stay below the fp16 range; half of it as the guard band


def mlp_wide_overflow() -> bool:
    """True if a matrix-core head MLP call since the last query produced a non-finite output row, i.e. an activation
    left the fp16 range of its split-fp16 arithmetic.  Reads and clears the device flag; synchronises."""
    flag = C.c_int32(0)
    _lib.check(_lib.lib().sn_mlp_wide_overflow(C.byref(flag)), "sn_mlp_wide_overflow")
    return bool(flag.value)


def mlp_forward(x: torch.Tensor, mlp, layer_norm: Optional[torch.nn.LayerNorm] = None, check_range: Optional[bool] = None) -> torch.Tensor:
    """SkipConnMLP / MLP forward [+ LayerNorm] in one matrix-core kernel (network.py:9-66, 115; the feature heads
    of renderer.py:359-385).  x [N, dim_in] -> [N, dim_out].  Inference only (no autograd graph); hidden width 256.
    check_range (default: environment SN_CHECK_RANGE=1): query the overflow flag after the call (one synchronisation) and
    raise if an activation left the fp16 range -- the inputs are run-time data, so no static bound exists for this kernel."""
    L = _lib.lib()
    x = x.detach().contiguous().float()
    layers = list(mlp.net)
    desc = _lib.MlpDesc()
    keep: list = []
    _fill_mlp(desc, layers, x.shape[-1], keep)
    leaky = getattr(mlp, "skip_layers", None) is not None        # SkipConnMLP uses LeakyReLU(0.01), MLP uses ReLU
    desc.activation = 1 if leaky else 0
    desc.skip_mask = sum(1 << int(i) for i in (getattr(mlp, "skip_layers", None) or []))
    need = int(L.sn_mlp_wide_workspace_bytes(C.byref(desc)))
    if need == 0:
        raise RuntimeError("mlp_forward: " + L.sn_last_error().decode())
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = torch.empty(x.shape[0], desc.dims[desc.num_layers], device=x.device, dtype=torch.float32)
    lw = lb = None
    eps = 0.0
    if layer_norm is not None:
        lw = layer_norm.weight.detach().contiguous().float()
        lb = layer_norm.bias.detach().contiguous().float()
        eps = float(layer_norm.eps)
    _lib.check(L.sn_mlp_wide_forward(C.byref(desc), _lib.dev(lw, "ln.weight"), _lib.dev(lb, "ln.bias"), eps,
                                     _lib.dev(x, "x"), x.shape[0], _lib.dev(out, "out"), ws.data_ptr(), ws.numel(),
                                     _lib.stream()), "sn_mlp_wide_forward")
    if check_range if check_range is not None else check_range_default:
        if mlp_wide_overflow():
            raise RuntimeError("mlp_forward: an activation left the fp16 range of the split-fp16 matrix-core arithmetic "
                               "(|v| >= 65504): outputs are not finite; run this head through the torch module instead")
    return out


def mask_head_fusable(encoder, mlp, T: int, E: int) -> bool:
    """Can sn_rm_mask_head take this head (renderer.py:376-385)?  fp32 3-D grid with level_dim 8, 256-wide MLP without skip
    layers and at most 32 outputs, a power-of-two number of samples per ray <= 128, at most 16 appended channels."""
    return (encoder.input_dim == 3 and encoder.level_dim == 8 and encoder.embeddings.dtype == torch.float32
            and (encoder.num_levels % 2 == 0 or E == 0) and E <= 16 and 1 <= T <= 128 and (T & (T - 1)) == 0
            and getattr(mlp, "dim_hidden", 0) == 256 and mlp.dim_out <= 32 and not (getattr(mlp, "skip_layers", None) or [])
            and mlp.dim_in == encoder.output_dim + E)


def mask_head(weights: torch.Tensor, xyzs: torch.Tensor, extra: torch.Tensor, encoder, mlp, bound: float) -> torch.Tensor:
    """composite(weights, mlp(cat([encoder(xyzs, bound), extra], -1))) in ONE kernel (renderer.py:304-305, 376-385):
    weights [N,T], xyzs [N,T,3], extra [N,T,E] -> [N, mlp.dim_out].  Inference only; see mask_head_fusable()."""
    N, T = weights.shape
    E = int(extra.shape[-1]) if extra is not None else 0
    assert xyzs.shape == (N, T, 3)
    L = _lib.lib()
    w = weights.detach().contiguous().float()
    x = xyzs.detach().contiguous().float()
    e = extra.detach().contiguous().float() if E else None
    gdesc = _lib.GridDesc()
    _fill_grid(gdesc, encoder, encoder.embeddings.detach().contiguous())
    mdesc = _lib.MlpDesc()
    keep: list = []
    _fill_mlp(mdesc, list(mlp.net), mlp.dim_in, keep)
    mdesc.activation = 1 if getattr(mlp, "skip_layers", None) is not None else 0      # SkipConnMLP: LeakyReLU(0.01)
    need = int(L.sn_rm_mask_head_workspace_bytes(C.byref(mdesc)))
    if need == 0:
        raise RuntimeError("mask_head: " + L.sn_last_error().decode())
    ws = torch.empty(need, dtype=torch.uint8, device=w.device)
    out = torch.empty(N, mdesc.dims[mdesc.num_layers], device=w.device, dtype=torch.float32)
    _lib.check(L.sn_rm_mask_head(_lib.dev(x, "xyzs"), _lib.dev(e, "extra"), _lib.dev(w, "weights"), N, T, E, float(bound),
                                 C.byref(gdesc), C.byref(mdesc), _lib.dev(out, "out"), ws.data_ptr(), ws.numel(), _lib.stream()),
               "sn_rm_mask_head")
    return out


def _fill_mlp(desc: _lib.MlpDesc, layers: Sequence[torch.nn.Linear], dim_in: int, keep: list) -> None:
    desc.num_layers = len(layers)
    desc.activation = 0
    desc.skip_mask = 0
    desc.dims[0] = dim_in
    for l, lin in enumerate(layers):
        w = lin.weight.detach().contiguous().float()
        keep.append(w)
        desc.weight[l] = w.data_ptr()
        desc.dims[l + 1] = w.shape[0]
        if lin.bias is not None:
            b = lin.bias.detach().contiguous().float()
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
        if "bins" in want:
            io.bins[k] = buf(f"bins{k}", (N, T + 1))
        if "weights" in want or (k == S - 1 and "weights_last" in want):
            io.weights[k] = buf(f"weights{k}", (N, T))
        if "sigmas" in want:
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
               packed: Optional[torch.Tensor] = None, head_input: bool = False) -> dict:
    """What last_launch_info() would report after render_rays(plan, <N rays>, ...) with the same arguments, without rendering
    (sn_rm_render_route_info: the same validation and route planning on the host; no render kernel is launched and no output is
    allocated).  Like render_rays it writes the effective tuning into plan.cfg.tuning and, unless skip_final, consults the plan's fp16
    range guard (plan.check_range(): device reductions and one sync when a parameter version moved) -- the guard decides the route."""
    io = _lib.RenderIO()
    stand_in = 64                                                  # an aligned non-NULL address: the dry run dereferences nothing
    io.rays_o = io.rays_d = stand_in
    _fill_io(plan, io, int(N), tile_w, want, u_tables, bins0_table, skip_final, packed, head_input, tuning,
             lambda name, shape, dtype=torch.float32: stand_in, lambda t: (t, stand_in))
    info = _lib.LaunchInfo()
    _lib.check(_lib.lib().sn_rm_render_route_info(C.byref(plan.cfg), C.byref(io), C.byref(info)), "route_info")
    return dict(final_kernel=info.final_kernel.decode(), workgroups=int(info.workgroups), lds_bytes=int(info.lds_bytes),
                dense_levels=int(info.dense_levels), gathers_per_wave_sample=int(info.gathers_per_wave_sample), launches=int(info.launches))


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
