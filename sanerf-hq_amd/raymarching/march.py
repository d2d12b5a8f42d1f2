"""Ray geometry, sampling and the per-ray losses (raymarch.hip):

    generate_rays        nerf/utils.py:182-304 (full image branch)
    near_far_from_aabb   nerf/renderer.py:122-139
    contract             nerf/renderer.py:60-69
    sample_pdf           nerf/renderer.py:84-119   (+ the integer searchsorted result)
    weights_from_sigma   nerf/renderer.py:308-325
    composite            nerf/renderer.py:333-338, 361, 384  (autograd w.r.t. both operands)
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch.autograd import Function

from .. import _lib
from ._args import _f32, _flat3, _i64

WEIGHTS_BACKWARD_MAX_T = 131072   # sn_rm_weights_from_sigma_backward: any ray the product meets (up to 256 samples in one wave's registers, beyond that the
                                  # segment prefixes in LDS); the torch statement in weights_from_sigma is what the tests compare the kernel with (they lower this constant)
PROPOSAL_LOSS_MAX_T = 1 << 24       # the kernels take any ray (up to 512 samples in LDS, beyond that in a workspace); nerf/renderer.py keeps the torch statement
                                    # for CPU tensors and the tests' comparison (they lower this constant)
DISTORT_LOSS_MAX_T = 1 << 24        # any ray (up to 2048 samples in LDS, beyond that read in place); as above


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
    inds = _i64(inds.reshape(-1))
    N = inds.shape[0]
    poses, intrinsics = _f32(poses.reshape(-1, 16)), _f32(intrinsics.reshape(-1, 4))
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
    bins, weights = _f32(bins), _f32(weights)
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
        real_bins, sig = _f32(real_bins), _f32(sigmas)
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
    rays_o, rays_d, bins = _f32(rays_o), _f32(rays_d), _f32(bins)
    N, T = bins.shape[0], bins.shape[1] - 1
    nears, fars = _f32(nears.reshape(-1)), _f32(fars.reshape(-1))
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


class _ray_composite(Function):
    """weights [N,T], rays_t [N,T], raw [N,T,16] (grid_mlp's output), rays_d [N,3] -> (weights_sum [N], depth [N], f_image [N,31]) in one
    kernel (sn_rm_ray_composite; renderer.py:327-347 with colour = cat([geo_feat, SH(d)]), network.py:164-170); differentiable w.r.t.
    weights and raw."""

    @staticmethod
    def forward(ctx, weights, rays_t, raw, rays_d):
        w, tm, r, d = _f32(weights), _f32(rays_t), _f32(raw), _f32(rays_d)
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
        ref_bins, ref_w = _f32(ref_bins), _f32(ref_weights)
        N, Tr = ref_w.shape
        S = len(bw) // 2
        bins = [_f32(b) for b in bw[:S]]
        ws = [_f32(w) for w in bw[S:]]
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
        g = _f32(grad_out.reshape(1))         # stays on the device: no host sync
        out = []
        for k in range(S):
            gw = torch.empty_like(ws[k])
            _proposal_loss_launch(bins[k], ws[k], ref_bins, ref_w, scale, _lib.dev(g, "grad_out"), None, _lib.dev(gw, "grad_weights"), "proposal_loss_backward")
            out.append(gw)
        return (None, None) + (None,) * S + tuple(out)


def proposal_loss_all(all_bins, all_weights):
    """sum over the proposal stages of proposal_loss_stage(...) against the last entry (renderer.py:30-57), one autograd node."""
    return _proposal_loss_all.apply(all_bins[-1], all_weights[-1], *all_bins[:-1], *all_weights[:-1])


class _proposal_loss_stage(Function):
    """One proposal stage's term of the inter-level loss (nerf/renderer.py:30-57): mean over rays and final-stage
    intervals of max(w_ref - bound, 0)^2 / (w_ref + 1e-8); differentiable w.r.t. the proposal weights only (bins come
    from sample_pdf, the final stage's bins and weights are detached in the reference)."""

    @staticmethod
    def forward(ctx, bins, weights, ref_bins, ref_weights):
        bins, ref_bins, w, ref_w = _f32(bins), _f32(ref_bins), _f32(weights), _f32(ref_weights)
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


def proposal_loss_stage(bins, weights, ref_bins, ref_weights):
    """bins [N,T+1], weights [N,T] of a proposal stage; ref_* of the final stage -> scalar (renderer.py:37-56, one stage)."""
    return _proposal_loss_stage.apply(bins, weights, ref_bins, ref_weights)


class _distort_loss(Function):
    """Mip-NeRF-360 distortion loss of nerf/renderer.py:17-27 (the reference delegates to the third-party
    torch_efficient_distloss.eff_distloss): mean over rays of (1/3) sum w_i^2 d_i + sum_ij w_i w_j |m_i - m_j|;
    value and d/dw from one kernel, the gradient is kept for backward (bins carry no gradient)."""

    @staticmethod
    def forward(ctx, bins, weights):
        bins, w = _f32(bins), _f32(weights)
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


def distort_loss(bins, weights):
    """bins [N,T+1], weights [N,T] -> scalar (renderer.py:17-27)."""
    return _distort_loss.apply(bins, weights)


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


def composite(weights, values):
    """weights [N,T], values [N,T,K] or [N,T] -> [N,K] or [N]."""
    if values.dim() == 2:
        return _composite.apply(weights, values.unsqueeze(-1)).squeeze(-1)
    return _composite.apply(weights, values)
