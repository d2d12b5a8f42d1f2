"""Encoder operators of the hot path on MI355X: multiresolution hash / tiled grid, real spherical
harmonics (degree <= 8) and NeRF frequency encoding, each as a `torch.autograd.Function` over the C ABI
of libsanerf_hip.so plus the `nn.Module` the reference's `get_encoder` hands out.

The reference keeps these in three packages (gridencoder/grid.py, shencoder/sphere_harmonics.py,
freqencoder/freq.py), each bound to its own pybind/CUDA extension; those module paths still exist here
and re-export the classes below, so `from gridencoder import GridEncoder` etc. keep working.

Observable differences from the reference (all neutral for callers):
  * the grid kernel writes [B, L*C] directly, so the permute copy of grid.py:63 is gone;
  * the per-level table (resolution, size, dense/hash) is computed once on the host from the offsets
    instead of per thread on the device (gridencoder.cu:132-133);
  * kernels run on torch's current stream, not the legacy default stream;
  * there is no CPU path: a CPU tensor raises "... must be a CUDA tensor" (gridencoder.cu:15).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _buffers, _lib

# =============================================================================================
# hash / tiled grid
# =============================================================================================
_gridtype_to_id = {"hash": 0, "tiled": 1}
_interp_to_id = {"linear": 0, "smoothstep": 1}

def _host_offsets(offsets: torch.Tensor) -> Tuple[int, ...]:
    """Offsets as host ints.  The copy is memoised ON the tensor object (with its version counter),
    so a device-resident buffer costs one device->host sync, once; a memo keyed by address would be
    unsafe because the allocator recycles addresses."""
    memo = getattr(offsets, "_sn_host_offsets", None)
    if memo is not None and memo[0] == offsets._version:
        return memo[1]
    if offsets.dtype != torch.int32:
        raise RuntimeError("offsets must be an int tensor")               # gridencoder.cu:17
    host = tuple(int(v) for v in offsets.detach().cpu().tolist())
    try:
        offsets._sn_host_offsets = (offsets._version, host)
    except AttributeError:
        pass
    return host


def _table_dtype(embeddings: torch.Tensor) -> int:
    if embeddings.dtype == torch.float32:
        return _lib.SN_F32
    if embeddings.dtype == torch.float16:
        return _lib.SN_F16
    raise RuntimeError("embeddings must be a floating tensor (float32 or float16)")


# Gradient scatter strategy of the grid encoder: "auto" uses the binned kernels (one partition pass + LDS accumulation, no atomics
# per corner: grid_binned.hip) once the scatter is large enough to amortise their five launches, "atomic" / "binned" force one path
# ("sorted", the name of the rounds 1-3 implementation, is accepted as an alias of "binned").
GRID_BACKWARD_MODE = "auto"
_BINNED_MIN_CONTRIBUTIONS = 1 << 19


def _binned_workspace_bytes(B: int, D: int, Cc: int, L: int, max_level: int, offs, dy_dx) -> int:
    """Device bytes the binned backward needs, or 0 when this call takes the atomic kernel."""
    if GRID_BACKWARD_MODE == "atomic" or dy_dx is not None or D not in (2, 3) or B >= (1 << 24):
        return 0
    n = B * max_level * (1 << D)
    if n == 0 or n >= (1 << 31):
        return 0
    if GRID_BACKWARD_MODE not in ("binned", "sorted") and n < _BINNED_MIN_CONTRIBUTIONS:
        return 0
    return int(_lib.lib().sn_grid_backward_binned_workspace_bytes(B, D, Cc, L, max_level, _lib.host_i32(offs)))   # 0: shape outside the kernels' limits


class _grid_encode(Function):
    """forward/backward contract of gridencoder/grid.py:24-95."""

    @staticmethod
    def forward(ctx, inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs=False,
                gridtype=0, align_corners=False, interpolation=0, max_level=None):
        inputs = inputs.contiguous()
        if inputs.dtype != torch.float32:
            inputs = inputs.float()
        B, D = inputs.shape
        L = offsets.shape[0] - 1
        Cc = embeddings.shape[1]
        S = float(np.float32(np.log2(per_level_scale)))
        H = int(base_resolution)
        max_level = L if max_level is None else min(max_level, L)
        table = embeddings
        if torch.is_autocast_enabled() and Cc % 2 == 0:        # grid.py:43-46
            table = embeddings.to(torch.half)
        table = table.contiguous()
        offs = _host_offsets(offsets)
        if offs[-1] != embeddings.shape[0]:
            raise RuntimeError(f"offsets end at row {offs[-1]} but embeddings has {embeddings.shape[0]} rows")
        out = torch.empty(B, L * Cc, device=inputs.device, dtype=torch.float32)
        if max_level < L:
            out.zero_()
        dy_dx = None
        if calc_grad_inputs:
            dy_dx = torch.empty(B, L * D * Cc, device=inputs.device, dtype=torch.float32)
            if max_level < L:
                dy_dx.zero_()
        lib = _lib.lib()
        _lib.check(lib.sn_grid_encode_forward(
            _lib.dev(inputs, "inputs"), _lib.dev(table, "embeddings", None), _table_dtype(table), _lib.host_i32(offs),
            _lib.dev(out, "outputs"), B, D, Cc, L, max_level, S, H, _lib.dev(dy_dx, "dy_dx"),
            gridtype, int(align_corners), interpolation, _lib.LAYOUT_BLC, _lib.stream()), "grid_encode_forward")
        ctx.save_for_backward(inputs, table, dy_dx)
        ctx.meta = (offs, B, D, Cc, L, S, H, gridtype, interpolation, max_level, bool(align_corners), embeddings.dtype)
        return out if table.dtype == torch.float32 else out.to(table.dtype)

    @staticmethod
    def backward(ctx, grad):
        inputs, table, dy_dx = ctx.saved_tensors
        offs, B, D, Cc, L, S, H, gridtype, interpolation, max_level, align_corners, emb_dtype = ctx.meta
        grad = grad.contiguous().float()
        grad_embeddings = _buffers.zeros_f32(table.shape, table.device)                                # grid.py:83
        grad_inputs = torch.zeros_like(inputs) if dy_dx is not None else None
        lib = _lib.lib()
        need = _binned_workspace_bytes(B, D, Cc, L, max_level, offs, dy_dx)
        if need:
            ws = _buffers.scratch("grid_binned", table.device, need)
            _lib.check(lib.sn_grid_encode_backward_binned(
                _lib.dev(grad, "grad"), _lib.dev(inputs, "inputs"), _lib.host_i32(offs), _lib.dev(grad_embeddings, "grad_embeddings"),
                B, D, Cc, L, max_level, S, H, gridtype, int(align_corners), interpolation, _lib.LAYOUT_BLC,
                ws.data_ptr(), ws.numel(), _lib.stream()), "grid_encode_backward_binned")
            return None, grad_embeddings.to(emb_dtype), None, None, None, None, None, None, None, None
        _lib.check(lib.sn_grid_encode_backward(
            _lib.dev(grad, "grad"), _lib.dev(inputs, "inputs"), _lib.dev(table, "embeddings", None), _table_dtype(table),
            _lib.host_i32(offs), _lib.dev(grad_embeddings, "grad_embeddings"), B, D, Cc, L, max_level, S, H,
            _lib.dev(dy_dx, "dy_dx"), _lib.dev(grad_inputs, "grad_inputs"),
            gridtype, int(align_corners), interpolation, _lib.LAYOUT_BLC, _lib.stream()), "grid_encode_backward")
        return grad_inputs, grad_embeddings.to(emb_dtype), None, None, None, None, None, None, None, None


grid_encode = _grid_encode.apply


class _grid_encode_cat(Function):
    """cat([grid_encode(inputs, embeddings), extra.detach()], -1) under autograd in ONE forward pass (sn_grid_encode_forward_cat): the mask
    head's MLP input in training (renderer.py:380: grid features next to the detached geometry channels).  Gradient: to the embeddings only
    (the first L*C columns of the incoming gradient, through the same binned / atomic scatter as _grid_encode); inputs and extra get none."""

    @staticmethod
    def forward(ctx, inputs, embeddings, offsets, extra, per_level_scale, base_resolution, gridtype, align_corners, interpolation):
        inputs = inputs.contiguous().float()
        extra = extra.contiguous().float()
        B, D = inputs.shape
        L, Cc, E = offsets.shape[0] - 1, embeddings.shape[1], extra.shape[1]
        S, H = float(np.float32(np.log2(per_level_scale))), int(base_resolution)
        table = embeddings.contiguous()
        offs = _host_offsets(offsets)
        if offs[-1] != embeddings.shape[0]:
            raise RuntimeError(f"offsets end at row {offs[-1]} but embeddings has {embeddings.shape[0]} rows")
        out = torch.empty(B, L * Cc + E, device=inputs.device, dtype=torch.float32)
        _lib.check(_lib.lib().sn_grid_encode_forward_cat(
            _lib.dev(inputs, "inputs"), _lib.dev(table, "embeddings", None), _table_dtype(table), _lib.host_i32(offs),
            _lib.dev(extra, "extra"), E, _lib.dev(out, "outputs"), B, Cc, L, S, H, gridtype, int(align_corners), interpolation, _lib.stream()),
            "grid_encode_forward_cat")
        ctx.save_for_backward(inputs, table)
        ctx.meta = (offs, B, D, Cc, L, S, H, gridtype, interpolation, bool(align_corners), embeddings.dtype)
        return out

    @staticmethod
    def backward(ctx, grad):
        inputs, table = ctx.saved_tensors
        offs, B, D, Cc, L, S, H, gridtype, interpolation, align_corners, emb_dtype = ctx.meta
        grad_embeddings = _buffers.zeros_f32(table.shape, table.device)                                # grid.py:83
        lib = _lib.lib()
        need = _binned_workspace_bytes(B, D, Cc, L, L, offs, None)
        if need and grad.is_contiguous() and grad.dtype == torch.float32 and grad.data_ptr() % 16 == 0:
            # the binned scatter reads the first L*C columns of the [B, L*C + E] gradient in place (no slice copy)
            ws = _buffers.scratch("grid_binned", table.device, need)
            _lib.check(lib.sn_grid_encode_backward_binned_rows(
                _lib.dev(grad, "grad"), grad.shape[1], _lib.dev(inputs, "inputs"), _lib.host_i32(offs), _lib.dev(grad_embeddings, "grad_embeddings"),
                B, D, Cc, L, L, S, H, gridtype, int(align_corners), interpolation, _lib.LAYOUT_BLC,
                ws.data_ptr(), ws.numel(), _lib.stream()), "grid_encode_backward_binned_rows")
            return None, grad_embeddings.to(emb_dtype), None, None, None, None, None, None, None
        g = grad[:, :L * Cc].contiguous().float()
        if need:
            ws = _buffers.scratch("grid_binned", table.device, need)
            _lib.check(lib.sn_grid_encode_backward_binned(
                _lib.dev(g, "grad"), _lib.dev(inputs, "inputs"), _lib.host_i32(offs), _lib.dev(grad_embeddings, "grad_embeddings"),
                B, D, Cc, L, L, S, H, gridtype, int(align_corners), interpolation, _lib.LAYOUT_BLC,
                ws.data_ptr(), ws.numel(), _lib.stream()), "grid_encode_backward_binned")
        else:
            _lib.check(lib.sn_grid_encode_backward(
                _lib.dev(g, "grad"), _lib.dev(inputs, "inputs"), _lib.dev(table, "embeddings", None), _table_dtype(table),
                _lib.host_i32(offs), _lib.dev(grad_embeddings, "grad_embeddings"), B, D, Cc, L, L, S, H,
                _lib.dev(None, "dy_dx"), _lib.dev(None, "grad_inputs"),
                gridtype, int(align_corners), interpolation, _lib.LAYOUT_BLC, _lib.stream()), "grid_encode_backward")
        return None, grad_embeddings.to(emb_dtype), None, None, None, None, None, None, None


def grid_level_offsets(input_dim: int, num_levels: int, per_level_scale: float, base_resolution: int,
                       log2_hashmap_size: int) -> np.ndarray:
    """First row of every level (+ the total), int32 [L+1]: rows per level = min(2^log2T, res^D) rounded up to a
    multiple of 8 with res = ceil(base * scale^level) in float64 (grid.py:121-136)."""
    sizes = []
    for level in range(num_levels):
        res = int(np.ceil(base_resolution * per_level_scale ** level))
        rows = min(2 ** log2_hashmap_size, res ** input_dim)
        sizes.append(int(np.ceil(rows / 8) * 8))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


class GridEncoder(nn.Module):
    """Same constructor, attributes and state_dict keys as gridencoder/grid.py:102-204."""

    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16,
                 log2_hashmap_size=19, desired_resolution=None, gridtype="hash", align_corners=False,
                 interpolation="linear"):
        super().__init__()
        if desired_resolution is not None:   # grid.py:107-108
            per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1))
        self.input_dim = input_dim
        self.num_levels = num_levels
        self.level_dim = level_dim
        self.per_level_scale = per_level_scale
        self.log2_hashmap_size = log2_hashmap_size
        self.base_resolution = base_resolution
        self.output_dim = num_levels * level_dim
        self.gridtype = gridtype
        self.gridtype_id = _gridtype_to_id[gridtype]
        self.interpolation = interpolation
        self.interp_id = _interp_to_id[interpolation]
        self.align_corners = align_corners

        self.max_params = 2 ** log2_hashmap_size
        starts = grid_level_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size)
        self.register_buffer("offsets", torch.from_numpy(starts))
        self.n_params = int(starts[-1]) * level_dim
        self.embeddings = nn.Parameter(torch.empty(int(starts[-1]), level_dim))
        self.reset_parameters()

    def reset_parameters(self):
        self.embeddings.data.uniform_(-1e-4, 1e-4)   # grid.py:144-146

    def __repr__(self):
        top = int(round(self.base_resolution * self.per_level_scale ** (self.num_levels - 1)))
        return (f"GridEncoder: input_dim={self.input_dim} num_levels={self.num_levels} level_dim={self.level_dim} "
                f"resolution={self.base_resolution} -> {top} per_level_scale={self.per_level_scale:.4f} "
                f"params={tuple(self.embeddings.shape)} gridtype={self.gridtype} align_corners={self.align_corners} "
                f"interpolation={self.interpolation}")

    def forward(self, inputs, bound=1, max_level=None):
        inputs = (inputs + bound) / (2 * bound)   # [-bound, bound] -> [0, 1] (grid.py:156)
        lead = list(inputs.shape[:-1])
        flat = inputs.view(-1, self.input_dim)
        out = grid_encode(flat, self.embeddings, self.offsets, self.per_level_scale, self.base_resolution,
                          flat.requires_grad, self.gridtype_id, self.align_corners, self.interp_id, max_level)
        return out.view(lead + [self.output_dim])

    def forward_unit(self, x01, max_level=None):
        """forward() for inputs that are already the unit-cube coordinates (inputs + bound) / (2 bound) of grid.py:156
        (raymarching.sample_positions(grid_bound=...) produces them in the same kernel as the positions)."""
        lead = list(x01.shape[:-1])
        flat = x01.reshape(-1, self.input_dim)
        out = grid_encode(flat, self.embeddings, self.offsets, self.per_level_scale, self.base_resolution,
                          flat.requires_grad, self.gridtype_id, self.align_corners, self.interp_id, max_level)
        return out.view(lead + [self.output_dim])

    def forward_cat(self, inputs, extra, bound=1):
        """cat([self(inputs, bound), extra.detach()], -1) in one pass (the mask head's MLP input, renderer.py:380: no [B, L*C] intermediate
        and no concatenation pass).  inputs [..., 3], extra [..., E] -> [..., L*C + E].  With autograd on and a trainable fp32 table the
        embeddings receive their gradient (ops._grid_encode_cat); inputs and extra never do."""
        with torch.no_grad():
            x = ((inputs + bound) / (2 * bound)).reshape(-1, self.input_dim).contiguous().float()
            ex = extra.reshape(-1, extra.shape[-1]).contiguous().float()
        lead = list(inputs.shape[:-1])
        B, E = x.shape[0], ex.shape[1]
        if ex.shape[0] != B or self.input_dim != 3:
            raise ValueError(f"forward_cat: inputs {tuple(inputs.shape)} / extra {tuple(extra.shape)} do not match (3-D inputs only)")
        if torch.is_grad_enabled() and self.embeddings.requires_grad:
            if self.embeddings.dtype == torch.float32 and x.is_cuda and not torch.is_autocast_enabled():
                out = _grid_encode_cat.apply(x, self.embeddings, self.offsets, ex, self.per_level_scale, self.base_resolution,
                                             self.gridtype_id, self.align_corners, self.interp_id)
                return out.view(lead + [self.output_dim + E])
            # a half table / autocast (grid.py:43-46) keeps the encoder's own autograd path and a concatenation, as the reference writes it
            return torch.cat([self(inputs, bound=bound), extra.detach()], dim=-1)
        return self._forward_cat_nograd(x, ex, lead)

    @torch.no_grad()
    def _forward_cat_nograd(self, x, ex, lead):
        B, E = x.shape[0], ex.shape[1]
        table = self.embeddings.detach().contiguous()
        out = torch.empty(B, self.output_dim + E, device=x.device, dtype=torch.float32)
        S = float(np.float32(np.log2(self.per_level_scale)))
        _lib.check(_lib.lib().sn_grid_encode_forward_cat(
            _lib.dev(x, "inputs"), _lib.dev(table, "embeddings", None), _table_dtype(table), _lib.host_i32(_host_offsets(self.offsets)),
            _lib.dev(ex, "extra"), E, _lib.dev(out, "outputs"), B, self.level_dim, self.num_levels, S, int(self.base_resolution),
            self.gridtype_id, int(self.align_corners), self.interp_id, _lib.stream()), "grid_encode_forward_cat")
        return out.view(lead + [self.output_dim + E])

    @torch.no_grad()
    def grad_total_variation(self, weight=1e-7, inputs=None, bound=1, B=1000000):
        """In-place TV-regulariser gradient on .embeddings.grad (grid.py:170-191)."""
        if self.embeddings.grad is None:
            raise ValueError("grad is None, should be called after loss.backward() and before optimizer.step()!")
        if inputs is None:
            inputs = torch.rand(B, self.input_dim, device=self.embeddings.device)
        else:
            inputs = ((inputs + bound) / (2 * bound)).view(-1, self.input_dim)
            B = inputs.shape[0]
        inputs = inputs.contiguous().float()
        S = float(np.float32(np.log2(self.per_level_scale)))
        emb = self.embeddings.detach().float().contiguous()
        grad = self.embeddings.grad
        g32 = grad if grad.dtype == torch.float32 and grad.is_contiguous() else grad.float().contiguous()
        _lib.check(_lib.lib().sn_grad_total_variation(
            _lib.dev(inputs, "inputs"), _lib.dev(emb, "embeddings"), _lib.dev(g32, "grad"),
            _lib.host_i32(_host_offsets(self.offsets)), float(weight), B, self.input_dim, self.level_dim,
            self.num_levels, S, int(self.base_resolution), self.gridtype_id, int(self.align_corners), _lib.stream()),
            "grad_total_variation")
        if g32 is not grad:
            grad.copy_(g32)

    @torch.no_grad()
    def grad_weight_decay(self, weight=0.1):
        """Level-wise mean weight decay added to .embeddings.grad (grid.py:193-204)."""
        if self.embeddings.grad is None:
            raise ValueError("grad is None, should be called after loss.backward() and before optimizer.step()!")
        emb = self.embeddings.detach().float().contiguous()
        grad = self.embeddings.grad
        g32 = grad if grad.dtype == torch.float32 and grad.is_contiguous() else grad.float().contiguous()
        _lib.check(_lib.lib().sn_grad_weight_decay(
            _lib.dev(emb, "embeddings"), _lib.dev(g32, "grad"), _lib.host_i32(_host_offsets(self.offsets)),
            float(weight), emb.shape[0], emb.shape[1], self.num_levels, _lib.stream()), "grad_weight_decay")
        if g32 is not grad:
            grad.copy_(g32)


# =============================================================================================
# spherical harmonics
# =============================================================================================
class _sh_encoder(Function):
    @staticmethod
    def forward(ctx, inputs, degree, calc_grad_inputs=False):
        inputs = inputs.float().contiguous()          # forced fp32 (sphere_harmonics.py:16)
        B, input_dim = inputs.shape
        out_dim = degree ** 2
        outputs = torch.empty(B, out_dim, dtype=torch.float32, device=inputs.device)
        dy_dx = torch.empty(B, input_dim * out_dim, dtype=torch.float32, device=inputs.device) if calc_grad_inputs else None
        _lib.check(_lib.lib().sn_sh_encode_forward(_lib.dev(inputs, "inputs"), _lib.dev(outputs, "outputs"), B, input_dim,
                                                   degree, _lib.dev(dy_dx, "dy_dx"), _lib.stream()), "sh_encode_forward")
        ctx.save_for_backward(inputs, dy_dx)
        ctx.dims = (B, input_dim, degree)
        return outputs

    @staticmethod
    def backward(ctx, grad):
        inputs, dy_dx = ctx.saved_tensors
        if dy_dx is None:
            return None, None, None
        B, input_dim, degree = ctx.dims
        grad = grad.contiguous().float()
        grad_inputs = torch.zeros_like(inputs)
        _lib.check(_lib.lib().sn_sh_encode_backward(_lib.dev(grad, "grad"), _lib.dev(inputs, "inputs"), B, input_dim, degree,
                                                    _lib.dev(dy_dx, "dy_dx"), _lib.dev(grad_inputs, "grad_inputs"),
                                                    _lib.stream()), "sh_encode_backward")
        return grad_inputs, None, None


sh_encode = _sh_encoder.apply


class SHEncoder(nn.Module):
    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = degree ** 2
        assert self.input_dim == 3, "SH encoder only support input dim == 3"
        assert 0 < self.degree <= 8, "SH encoder only supports degree in [1, 8]"

    def __repr__(self):
        return f"SHEncoder: input_dim={self.input_dim} degree={self.degree}"

    def forward(self, inputs, size=1):
        inputs = inputs / size
        inputs = inputs / torch.norm(inputs, dim=-1, keepdim=True)   # sphere_harmonics.py:82
        lead = list(inputs.shape[:-1])
        flat = inputs.reshape(-1, self.input_dim)
        out = sh_encode(flat, self.degree, flat.requires_grad)
        return out.reshape(lead + [self.output_dim])


# =============================================================================================
# frequency encoding
# =============================================================================================
class _freq_encoder(Function):
    @staticmethod
    def forward(ctx, inputs, degree, output_dim):
        inputs = inputs.float().contiguous()
        B, input_dim = inputs.shape
        outputs = torch.empty(B, output_dim, dtype=torch.float32, device=inputs.device)
        _lib.check(_lib.lib().sn_freq_encode_forward(_lib.dev(inputs, "inputs"), B, input_dim, degree, output_dim,
                                                     _lib.dev(outputs, "outputs"), _lib.stream()), "freq_encode_forward")
        ctx.save_for_backward(outputs)
        ctx.dims = (B, input_dim, degree, output_dim)
        return outputs

    @staticmethod
    def backward(ctx, grad):
        (outputs,) = ctx.saved_tensors
        B, input_dim, degree, output_dim = ctx.dims
        grad = grad.contiguous().float()
        grad_inputs = torch.zeros(B, input_dim, dtype=torch.float32, device=grad.device)
        _lib.check(_lib.lib().sn_freq_encode_backward(_lib.dev(grad, "grad"), _lib.dev(outputs, "outputs"), B, input_dim,
                                                      degree, output_dim, _lib.dev(grad_inputs, "grad_inputs"),
                                                      _lib.stream()), "freq_encode_backward")
        return grad_inputs, None, None


freq_encode = _freq_encoder.apply


class FreqEncoder(nn.Module):
    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = input_dim + input_dim * 2 * degree

    def __repr__(self):
        return f"FreqEncoder: input_dim={self.input_dim} degree={self.degree} output_dim={self.output_dim}"

    def forward(self, inputs, **kwargs):
        lead = list(inputs.shape[:-1])
        flat = inputs.reshape(-1, self.input_dim)
        out = freq_encode(flat, self.degree, self.output_dim)
        return out.reshape(lead + [self.output_dim])


# ---------------------------------------------------------------------------------------------
# small linear layers under autograd: weight gradient through sn_linear_wgrad
# ---------------------------------------------------------------------------------------------
LINEAR_WGRAD_MIN_ROWS = 16384      # below this the BLAS call is as fast
LINEAR_WGRAD_MAX_OUT = 256         # sn_linear_wgrad's output rows (any fan-in)

# Weight gradients beside the rest of the backward pass (round 4).  A layer's weight gradient is a leaf of the backward graph: nothing
# downstream of it runs before the optimiser.  sn_linear_wgrad is matrix-core work, the gradient scatter of the grid encoder that follows it
# in a mask-field / RGB step is memory and LDS work -- on ONE stream they run one after the other.  With WGRAD_SIDE_STREAM the weight
# gradients of a backward call go to a second stream (forked after everything they read exists) and the backward pass joins it in an engine
# callback at its very end (torch.autograd queue_callback), so the two kinds of kernel overlap.  Only when no gradient tensor can be touched
# before that join: every parameter's .grad is None (AccumulateGrad then stores the tensor, no kernel) -- otherwise the launch stays inline.
# Tensors the side stream reads or writes are recorded with the caching allocator (record_stream).  Capturable (fork and join are events).
#
# OPT-IN (round 5, advisor): the caller states, by setting the flag, what this module cannot see from a parameter -- that nothing consumes
# a weight gradient on the main stream before the backward pass ends.  That is false under DistributedDataParallel (the reducer's hooks sit
# on the AccumulateGrad node in C++ and all-reduce the bucket while the side stream may still be writing it) and when one MLP is applied
# twice inside one graph (the engine's input buffer adds the two gradients on the main stream).  What CAN be seen is checked per call
# (_beside_ok): a leaf that requires grad, .grad is None, no tensor hooks, no post-accumulate-grad hooks; the shared-weight case is caught by
# counting the live autograd nodes that hold the weight (_wide_uses).  bench.py / tools/train_*.py set the flag for their single-process steps.
WGRAD_SIDE_STREAM = False
_side_streams: dict = {}


def _wgrad_side_stream(device):
    s = _side_streams.get(device)
    if s is None:
        s = _side_streams[device] = torch.cuda.Stream(device=device)
    return s


class _UseToken:
    __slots__ = ("__weakref__",)


_wide_uses: dict = {}      # id(weight) -> WeakSet of tokens, one per live _wide_mlp_train node that holds the weight and has not been differentiated
                           # (a weight used twice in one graph must not take the side stream; a node dropped without backward() frees its token)


_shared_now: set = set()   # weights seen with two live nodes during the running backward pass (cleared by an engine callback at its end)


def _beside_ok(params) -> bool:
    for p in params:
        if not (p.is_leaf and p.requires_grad) or p.grad is not None or p._backward_hooks:
            return False
        if getattr(p, "_post_accumulate_grad_hooks", None):
            return False
        if len(_wide_uses.get(id(p), ())) > 1 or id(p) in _shared_now:
            return False
    return True


def _run_beside_backward(params, tensors, launch) -> bool:
    """launch() on the side stream if that is safe (see above); returns whether it did."""
    if not WGRAD_SIDE_STREAM or not _beside_ok(params):
        return False
    dev = tensors[0].device
    main, side = torch.cuda.current_stream(dev), _wgrad_side_stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        launch()
    for t in tensors:
        t.record_stream(side)
    ev = side.record_event()
    try:
        torch.autograd.Variable._execution_engine.queue_callback(lambda: torch.cuda.current_stream(dev).wait_event(ev))
    except RuntimeError:            # not inside an engine-driven backward pass (backward() called by hand): join right away
        main.wait_event(ev)
    return True


COLD_GEMM_NATIVE = True            # nn.Linear layers the specialised kernels do not cover: True = the library's own fp32 matrix product (sn_gemm_f32: true fp32 on
                                   # the matrix cores, one k-ascending chain per output, deterministic); False = torch.nn.functional.linear / `@` (rocBLAS: faster on
                                   # large shapes, summation order its own) -- a plain library GEMM, for A/B and for users who prefer it
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def _gemm(a, a_row, a_col, b, b_row, b_col, bias, act, M, N, K, out):
    _lib.check(_lib.lib().sn_gemm_f32(_lib.dev(a, "a"), int(a_row), int(a_col), _lib.dev(b, "b"), int(b_row), int(b_col),
                                      _lib.dev(bias, "bias") if bias is not None else None, int(act), int(M), int(N), int(K),
                                      _lib.dev(out, "out"), int(N), _lib.stream()), "sn_gemm_f32")          # (outputs are contiguous [M, N])
    return out


def gemm_ok(x: torch.Tensor, weight: torch.Tensor, bias=None) -> bool:
    """Can sn_gemm_f32 take this nn.Linear?  fp32 CUDA tensors, no autocast."""
    return (COLD_GEMM_NATIVE and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.is_cuda
            and (bias is None or (bias.dtype == torch.float32 and bias.is_cuda)) and not torch.is_autocast_enabled() and weight.dim() == 2)


def linear_forward(x: torch.Tensor, weight: torch.Tensor, bias=None, act: int = ACT_NONE) -> torch.Tensor:
    """act(x W^T + b) through sn_gemm_f32 (no autograd): x [..., K], weight [N, K] -> [..., N]."""
    K, N = weight.shape[1], weight.shape[0]
    rows = 1
    for d in x.shape[:-1]:
        rows *= int(d)
    x2 = x.detach().reshape(rows, K).contiguous()
    w = weight.detach().contiguous()
    out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)          # (returned as it is: not a view, callers apply in-place activations)
    _gemm(x2, K, 1, w, 1, K, bias.detach().contiguous() if bias is not None else None, act, rows, N, K, out.view(rows, N))
    return out


def linear_backward_input(gy2: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """dx [M, K] = dy [M, N] W [N, K] through sn_gemm_f32."""
    M, N = gy2.shape
    K = weight.shape[1]
    out = torch.empty(M, K, device=gy2.device, dtype=torch.float32)
    return _gemm(gy2, N, 1, weight.detach().contiguous(), K, 1, None, ACT_NONE, M, K, N, out)


def linear_wgrad_general(x2: torch.Tensor, gy2: torch.Tensor, gw: torch.Tensor) -> torch.Tensor:
    """dw [N, K] = dy [M, N]^T x [M, K] through sn_gemm_f32 (layers wider than sn_linear_wgrad takes: one workgroup per 64 x 64 tile walks all M rows)."""
    M, K, N = x2.shape[0], x2.shape[1], gy2.shape[1]
    return _gemm(gy2, 1, N, x2, K, 1, None, ACT_NONE, N, K, M, gw)


class _small_linear(Function):
    """y = x W^T (+ b) for a layer applied to many rows, any width (the layers of nerf/network.py:9-66 that the fused kernels of this file do not
    cover).  Forward and input gradient: sn_gemm_f32 (COLD_GEMM_NATIVE; else torch / rocBLAS); the weight gradient -- a small result of a
    1e5-long reduction, for which BLAS heuristics pick slow kernels -- is one call of sn_linear_wgrad (deterministic summation order), or of
    sn_gemm_f32 for more than 256 outputs."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if gemm_ok(x, weight, bias):
            return linear_forward(x, weight, bias)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = gw = gb = None
        gy2 = gy.reshape(-1, gy.shape[-1]).contiguous()
        if ctx.needs_input_grad[0]:
            gy2f = gy2 if gy2.dtype == torch.float32 else gy2.float()
            gx = (linear_backward_input(gy2f, weight) if gemm_ok(gy2f, weight) else gy2 @ weight).reshape(x.shape)
        if ctx.needs_input_grad[1]:
            x2 = x.reshape(-1, x.shape[-1]).contiguous()
            M, K, N = x2.shape[0], x2.shape[1], gy2.shape[1]
            gw = torch.empty(N, K, device=x2.device, dtype=torch.float32)
            if N > LINEAR_WGRAD_MAX_OUT and M > 0:
                linear_wgrad_general(x2, gy2, gw)
            else:                      # (an empty batch: _wgrad_into zeroes gw)
                # (inline: on the side stream the ~10 small launches of an RGB step cost more in forks than they hide -- step as a graph 2.24 -> 2.45 ms)
                _wgrad_into(x2, gy2, gw, "linear_wgrad")
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy2.sum(0)
        return gx, gw, gb


# ---------------------------------------------------------------------------------------------
# the reference's small ReLU perceptrons under autograd: one kernel per direction (csrc/mlp_small.hip)
# ---------------------------------------------------------------------------------------------
SMALL_MLP_FUSED = True              # False: nn.Linear layers through torch / rocBLAS (A/B, tests)
SMALL_ACT_NONE, SMALL_ACT_TRUNC_EXP0, SMALL_ACT_SIGMOID_BG = 0, 1, 2


def _small_desc(weights):
    desc = _lib.MlpDesc()
    desc.num_layers = len(weights)
    desc.activation = 0
    desc.skip_mask = 0
    desc.dims[0] = weights[0].shape[1]
    for i, w in enumerate(weights):
        desc.weight[i] = w.data_ptr()
        desc.bias[i] = None
        desc.dims[i + 1] = w.shape[0]
    return desc


def _wgrad_into(x2, gy2, gw, tag="small_mlp_wgrad"):
    """gw[N,K] = gy2[M,N]^T x2[M,K] through sn_linear_wgrad (fixed summation order); tag: the caller's workspace (_buffers.scratch)."""
    lib = _lib.lib()
    M, K, N = x2.shape[0], x2.shape[1], gy2.shape[1]
    if M == 0:                      # an empty batch: the sum over no rows
        gw.zero_()
        return
    need = int(lib.sn_linear_wgrad_workspace_bytes(M, K, N))
    if need == 0:
        raise RuntimeError("sn_linear_wgrad: " + lib.sn_last_error().decode())
    ws = _buffers.scratch(tag, x2.device, need, floor=1 << 20)
    _lib.check(lib.sn_linear_wgrad(_lib.dev(x2, "x"), _lib.dev(gy2, "grad_output"), M, K, N, _lib.dev(gw, "grad_weight"),
                                   ws.data_ptr(), ws.numel(), _lib.stream()), "sn_linear_wgrad")


def _packed16(t):
    """t as contiguous fp32 whose first element is 16-byte aligned, which sn_mlp_small_* require of x and grad_out whatever the width.
    A contiguous row slice such as x[1:] of a 10- or 31-wide tensor starts 40 or 124 bytes into its allocation: such a view is repacked
    (one copy), anything else is passed as it is.  Not needed for aux_in and grad_aux: the kernels read those with scalar loads and the
    library does not check their alignment; grad_in, out and the hidden buffers are fresh allocations."""
    t = t.contiguous().float()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _small_mlp_train(Function):
    """A bias-free ReLU `MLP` (network.py:9-29) of the reference network's sizes under autograd, with what follows it on the training path
    folded in: act = SMALL_ACT_TRUNC_EXP0 also returns trunc_exp(out[..., 0]) (network.py:155,179; activation.py:5-17), act =
    SMALL_ACT_SIGMOID_BG also returns sigmoid(out) + (1 - aux_in) * bg (renderer.py:349-353).  Forward: ONE kernel (sn_mlp_small_forward_train,
    true fp32 on the matrix cores, hidden outputs saved).  Backward: ONE kernel for the data path (sn_mlp_small_backward) + sn_linear_wgrad per
    layer.  Returns (raw output, activated output or None)."""

    @staticmethod
    def forward(ctx, x, act, aux_in, bg, *weights):
        lib = _lib.lib()
        lead = x.shape[:-1]
        rows = x.numel() // x.shape[-1]
        x2 = _packed16(x.detach().reshape(rows, x.shape[-1]))
        ws = [w.detach().contiguous() for w in weights]
        desc = _small_desc(ws)
        nl = len(ws)
        dev = x.device
        hs = [torch.empty(rows, w.shape[0], device=dev, dtype=torch.float32) for w in ws[:-1]]
        dout = ws[-1].shape[0]
        out = torch.empty(rows, dout, device=dev, dtype=torch.float32)
        aux = None
        if act == SMALL_ACT_TRUNC_EXP0:
            aux = torch.empty(rows, device=dev, dtype=torch.float32)
        elif act == SMALL_ACT_SIGMOID_BG:
            aux = torch.empty(rows, dout, device=dev, dtype=torch.float32)
        ai = aux_in.detach().reshape(rows).contiguous().float() if aux_in is not None else None
        hid = (C.c_void_p * max(nl - 1, 1))(*[t.data_ptr() for t in hs])
        _lib.check(lib.sn_mlp_small_forward_train(C.byref(desc), _lib.dev(x2, "x"), rows, hid, _lib.dev(out, "out"), int(act),
                                                  _lib.dev(ai, "aux_in"), float(bg), _lib.dev(aux, "aux_out"), _lib.stream()),
                   "sn_mlp_small_forward_train")
        ctx.save_for_backward(x2, out, *hs, *ws)
        ctx.meta = (nl, int(act), float(bg), tuple(x.shape), aux_in is not None)
        ctx.set_materialize_grads(False)
        out_v = out.view(*lead, dout)
        if aux is None:
            ctx.mark_non_differentiable()
            return out_v, None
        return out_v, (aux.view(*lead) if act == SMALL_ACT_TRUNC_EXP0 else aux.view(*lead, dout))

    @staticmethod
    def backward(ctx, g_out, g_aux):
        nl, act, bg, xshape, has_aux_in = ctx.meta
        saved = ctx.saved_tensors
        x2, out = saved[0], saved[1]
        hs, ws = saved[2:1 + nl], saved[1 + nl:]
        n_w = len(ws)
        if g_out is None and g_aux is None:
            return (None,) * (4 + n_w)
        lib = _lib.lib()
        rows, dev = x2.shape[0], x2.device
        dout = ws[-1].shape[0]
        go = _packed16(g_out.reshape(rows, dout)) if g_out is not None else None
        ga = g_aux.reshape(rows, 1 if act == SMALL_ACT_TRUNC_EXP0 else dout).contiguous().float() if g_aux is not None else None
        desc = _small_desc(ws)
        need_x = ctx.needs_input_grad[0]
        gx = torch.empty(rows, x2.shape[1], device=dev, dtype=torch.float32) if need_x else None
        ghs = [torch.empty_like(h) for h in hs]
        glast = torch.empty(rows, dout, device=dev, dtype=torch.float32)
        g_aux_in = torch.empty(rows, device=dev, dtype=torch.float32) if (has_aux_in and ctx.needs_input_grad[2] and ga is not None) else None
        hid = (C.c_void_p * max(nl - 1, 1))(*[t.data_ptr() for t in hs])
        ghp = (C.c_void_p * max(nl - 1, 1))(*[t.data_ptr() for t in ghs])
        _lib.check(lib.sn_mlp_small_backward(C.byref(desc), _lib.dev(go, "grad_out"), _lib.dev(ga, "grad_aux"), act, _lib.dev(out, "out_raw"), bg,
                                             hid, rows, _lib.dev(gx, "grad_in"), ghp, _lib.dev(glast, "grad_last"), _lib.dev(g_aux_in, "grad_aux_in"),
                                             _lib.stream()), "sn_mlp_small_backward")
        ins = [x2] + list(hs)
        gys = ghs + [glast]
        gws = []
        for i in range(nl):
            if not ctx.needs_input_grad[4 + i]:
                gws.append(None)
                continue
            gw = torch.empty(ws[i].shape, device=dev, dtype=torch.float32)
            _wgrad_into(ins[i], gys[i], gw)
            gws.append(gw)
        g_ai = None
        if g_aux_in is not None:
            g_ai = g_aux_in
        return (gx.view(xshape) if need_x else None), None, g_ai, None, *gws


def small_mlp_fusable(x: torch.Tensor, layers) -> bool:
    """Training-time route of an `MLP` through _small_mlp_train: CUDA fp32, autograd on, bias-free, widths this build instantiates."""
    if not (SMALL_MLP_FUSED and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()):
        return False
    if not (1 <= len(layers) <= 4) or any(l.bias is not None or l.weight.dtype != torch.float32 for l in layers):
        return False
    if not (x.requires_grad or any(l.weight.requires_grad for l in layers)):
        return False
    key = (x.shape[-1],) + tuple(l.weight.shape[0] for l in layers)
    ok = _small_supported.get(key)
    if ok is None:
        if x.shape[-1] != layers[0].weight.shape[1] or any(a.weight.shape[0] != b.weight.shape[1] for a, b in zip(layers[:-1], layers[1:])):
            return False
        ok = _small_supported[key] = bool(_lib.lib().sn_mlp_small_supported(C.byref(_small_desc([l.weight for l in layers]))))
    return ok


_small_supported: dict = {}


def small_mlp_train(x: torch.Tensor, layers, act: int = SMALL_ACT_NONE, aux_in=None, bg: float = 0.0):
    """(raw, activated) of the fused small perceptron; see _small_mlp_train."""
    return _small_mlp_train.apply(x, act, aux_in, bg, *[l.weight for l in layers])


WIDE_MLP_BACKWARD_MIN_ROWS = 16384
WIDE_MLP_BACKWARD_FUSED = True      # False: the wide training MLP differentiates through torch (A/B, tests)
WIDE_MLP_FORWARD_F16X3 = True       # the wide training MLP's forward as ONE kernel on the inference path's matrix-core kernel (split-fp16 x3 products, ~2^-22 per
                                    # product, fp32 accumulation; sn_mlp_wide_forward_train_f16x3) with the hidden outputs saved: 0.38 -> 0.2 ms for the mask head.
                                    # Against the reference's gradients (train_c5.npz) it gives the same errors as the BLAS forward to three digits
                                    # (tools/train_fwd_modes_err.py).  Activations must stay inside the fp16 range (raymarching.mlp_wide_overflow()).  False: BLAS fp32
WIDE_MLP_RANGE_CHECK_EVERY = 64    # with the split-fp16 forward: every this many training forwards the library's sticky overflow flag is read (one device
                                    # synchronisation; skipped while a HIP graph is being captured) and a RuntimeError names the cause -- an activation or
                                    # input at or beyond 65504 makes the logits, the loss and every gradient non-finite.  0: never check
_wide_fwd_calls = [0]
WIDE_MLP_SIGN_BITS = True           # the split-fp16 training forward also writes one sign bit per hidden unit and the backward data path reads those (A/B, tests: False)
WIDE_MLP_FORWARD_NATIVE = False     # True: the wide training MLP's forward as ONE kernel (sn_mlp_wide_forward_train: fp32 MFMA, fused activations).  Measured slower
                                    # than the BLAS GEMMs + activation kernels (0.555 vs 0.377 ms for the mask head, csrc/mlp_f32.inc), so opt-in


class _wide_mlp_train(Function):
    """A bias-free 256-wide perceptron without skip layers under autograd (the per-sample mask head in training,
    network.py:118-123 / trainer.py:401-428).  Forward: one matrix-core kernel (split-fp16 x3 products, WIDE_MLP_FORWARD_F16X3) with every
    hidden output saved; or the usual BLAS fp32 GEMMs; or, with WIDE_MLP_FORWARD_NATIVE, one fp32-MFMA kernel (sn_mlp_wide_forward_train).
    (Rounds 2-4 kept the BLAS forward for fear that differently rounded pre-activations flip LeakyReLU branches and spend the 1e-3 gradient
    budget; measured in round 5, the error against the reference's gradients is the same to three digits for all three forwards.)  Backward: ONE kernel for the whole data path (sn_mlp_wide_backward: grad of the
    input and of every hidden pre-activation, masks from the saved outputs) + sn_linear_wgrad per layer."""

    @staticmethod
    def forward(ctx, x, leaky, *weights):
        hs = []
        if WIDE_MLP_FORWARD_F16X3 and not WIDE_MLP_FORWARD_NATIVE:
            # one kernel for all layers on the inference path's matrix-core kernel (split-fp16 x3 products, fp32 accumulation), hidden outputs saved
            nl = len(weights)
            rows = x.numel() // x.shape[-1]
            x2 = x.reshape(rows, x.shape[-1]).contiguous()
            ws = [w.contiguous() for w in weights]
            desc = _small_desc(ws)
            desc.activation = 1 if leaky else 0
            lib = _lib.lib()
            need = int(lib.sn_mlp_wide_workspace_bytes(C.byref(desc)))
            if need == 0:
                raise RuntimeError("wide MLP forward: " + lib.sn_last_error().decode())
            wsb = _buffers.scratch("wide_mlp_forward", x.device, need)
            hs = [torch.empty(*x.shape[:-1], 256, device=x.device, dtype=torch.float32) for _ in range(nl - 1)]
            h = torch.empty(*x.shape[:-1], ws[-1].shape[0], device=x.device, dtype=torch.float32)
            hid = (C.c_void_p * max(nl - 1, 1))(*[t.data_ptr() for t in hs])
            # one bit per hidden unit (set = output > 0): all the backward DATA path needs of the saved outputs (32 bytes per row and layer
            # instead of 1 KiB; the weight gradients still read the outputs themselves)
            bits = [torch.empty(rows, 8, device=x.device, dtype=torch.int32) for _ in range(nl - 1)] if WIDE_MLP_SIGN_BITS else []
            bid = (C.c_void_p * max(nl - 1, 1))(*[t.data_ptr() for t in bits]) if bits else None
            _lib.check(lib.sn_mlp_wide_forward_train_f16x3(C.byref(desc), _lib.dev(x2, "x"), rows, hid, bid, _lib.dev(h, "out"),
                                                           wsb.data_ptr(), wsb.numel(), _lib.stream()), "sn_mlp_wide_forward_train_f16x3")
            ctx.sign_bits = bits
            _wide_fwd_calls[0] += 1
            if (WIDE_MLP_RANGE_CHECK_EVERY and _wide_fwd_calls[0] % WIDE_MLP_RANGE_CHECK_EVERY == 0
                    and not torch.cuda.is_current_stream_capturing()):
                flag = C.c_int32(0)
                _lib.check(lib.sn_mlp_wide_overflow(C.byref(flag)), "sn_mlp_wide_overflow")
                # the flag is process-wide and sticky: an inference call of the head kernels may have raised it since the last read.  It only
                # counts here when THIS call's own output is not finite (a training run that left the range stays outside it)
                if flag.value and not bool(torch.isfinite(h).all()):
                    raise RuntimeError(
                        "wide MLP training forward: an activation or input left the fp16 range (|v| >= 65504) of the split-fp16 matrix-core "
                        "forward (checked every %d calls); logits, loss and gradients of this step are not finite.  Set "
                        "sanerf_hq_amd.ops.WIDE_MLP_FORWARD_F16X3 = False (fp32 BLAS forward, no range limit) or rescale the inputs."
                        % WIDE_MLP_RANGE_CHECK_EVERY)
        elif WIDE_MLP_FORWARD_NATIVE and x.shape[-1] <= 256 and weights[-1].shape[0] <= 256:
            # one kernel for all layers: true fp32 on the matrix cores, activation fused, hidden outputs saved (sn_mlp_wide_forward_train)
            nl = len(weights)
            rows = x.numel() // x.shape[-1]
            x2 = x.reshape(rows, x.shape[-1]).contiguous()
            ws = [w.contiguous() for w in weights]
            desc = _small_desc(ws)
            desc.activation = 1 if leaky else 0
            hs = [torch.empty(*x.shape[:-1], 256, device=x.device, dtype=torch.float32) for _ in range(nl - 1)]
            h = torch.empty(*x.shape[:-1], ws[-1].shape[0], device=x.device, dtype=torch.float32)
            hid = (C.c_void_p * max(nl - 1, 1))(*[t.data_ptr() for t in hs])
            _lib.check(_lib.lib().sn_mlp_wide_forward_train(C.byref(desc), _lib.dev(x2, "x"), rows, hid, _lib.dev(h, "out"), _lib.stream()),
                       "sn_mlp_wide_forward_train")
        else:
            h = x                        # (WIDE_MLP_FORWARD_F16X3 = WIDE_MLP_FORWARD_NATIVE = False: the BLAS forward, an explicit A/B switch)
            for i, w in enumerate(weights):
                h = torch.nn.functional.linear(h, w)
                if i + 1 < len(weights):
                    h = torch.nn.functional.leaky_relu(h, inplace=True) if leaky else torch.relu_(h)
                    hs.append(h)
        ctx.save_for_backward(x, *hs, *weights)
        ctx.nl, ctx.leaky = len(weights), bool(leaky)
        if WGRAD_SIDE_STREAM:
            ctx.use_token = _UseToken()
            for w in weights:
                _wide_uses.setdefault(id(w), weakref.WeakSet()).add(ctx.use_token)
        return h

    @staticmethod
    def backward(ctx, gy):
        nl = ctx.nl
        saved = ctx.saved_tensors
        x, hs, ws = saved[0], saved[1:nl], saved[nl:]
        lib = _lib.lib()
        gy2 = gy.reshape(-1, gy.shape[-1]).contiguous().float()
        N = gy2.shape[0]
        x2 = x.reshape(N, -1)
        desc = _small_desc(ws)
        desc.activation = 1 if ctx.leaky else 0
        need = int(lib.sn_mlp_wide_backward_workspace_bytes(C.byref(desc)))
        if need == 0:
            raise RuntimeError("wide MLP backward: " + lib.sn_last_error().decode())
        ws_buf = _buffers.scratch("wide_mlp_backward", x.device, need)
        gx = torch.empty(N, x2.shape[1], device=x.device, dtype=torch.float32)
        gh = [torch.empty(N, 256, device=x.device, dtype=torch.float32) for _ in range(nl - 1)]
        hid = (C.c_void_p * (nl - 1))(*[h.reshape(N, 256).data_ptr() for h in hs])
        ghp = (C.c_void_p * (nl - 1))(*[g.data_ptr() for g in gh])
        bits = getattr(ctx, "sign_bits", None)
        if bits:
            bid = (C.c_void_p * (nl - 1))(*[t.data_ptr() for t in bits])
            _lib.check(lib.sn_mlp_wide_backward_bits(C.byref(desc), _lib.dev(gy2, "grad_output"), bid, N, _lib.dev(gx, "grad_input"), ghp,
                                                     ws_buf.data_ptr(), ws_buf.numel(), _lib.stream()), "sn_mlp_wide_backward_bits")
        else:
            _lib.check(lib.sn_mlp_wide_backward(C.byref(desc), _lib.dev(gy2, "grad_output"), hid, N, _lib.dev(gx, "grad_input"), ghp,
                                                ws_buf.data_ptr(), ws_buf.numel(), _lib.stream()), "sn_mlp_wide_backward")
        grads_w = []
        inputs = [x2.contiguous()] + [h.reshape(N, 256) for h in hs]
        outs = gh + [gy2]
        todo = [i for i in range(nl) if ctx.needs_input_grad[2 + i]]
        gws = {i: torch.empty(outs[i].shape[1], inputs[i].shape[1], device=x.device, dtype=torch.float32) for i in todo}
        wneed = max([int(lib.sn_linear_wgrad_workspace_bytes(N, inputs[i].shape[1], outs[i].shape[1])) for i in todo], default=0)
        # (its own workspace: these launches may run beside _linear's on the main stream)
        wsb = _buffers.scratch("wide_mlp_wgrad", x.device, wneed, floor=1 << 20) if todo else None

        def launch_wgrads():
            for i in todo:
                K, Nn = inputs[i].shape[1], outs[i].shape[1]
                _lib.check(lib.sn_linear_wgrad(_lib.dev(inputs[i], "x"), _lib.dev(outs[i], "grad_output"), N, K, Nn, _lib.dev(gws[i], "grad_weight"),
                                               wsb.data_ptr(), wsb.numel(), _lib.stream()), "sn_linear_wgrad")
        if any(len(_wide_uses.get(id(w), ())) > 1 for w in ws):          # a weight shared by two nodes of this graph: both stay inline
            _shared_now.update(id(w) for w in ws)
            try:
                torch.autograd.Variable._execution_engine.queue_callback(_shared_now.clear)
            except RuntimeError:
                pass
        if todo and not _run_beside_backward([ws[i] for i in todo], [inputs[i] for i in todo] + [outs[i] for i in todo] + list(gws.values()) + [wsb], launch_wgrads):
            launch_wgrads()
        ctx.use_token = None
        grads_w = [gws.get(i) for i in range(nl)]
        return (gx.reshape(x.shape) if ctx.needs_input_grad[0] else None), None, *grads_w


def wide_mlp_fusable(x: torch.Tensor, layers, skip_layers) -> bool:
    """Training-time route of a SkipConnMLP / MLP through _wide_mlp_train: CUDA fp32, autograd on, many rows, no bias, no
    skip layers, hidden width 256, at most 256 inputs and at most 256 outputs (wider inputs take the torch layers)."""
    rows = x.numel() // max(x.shape[-1], 1)
    return (torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and rows >= WIDE_MLP_BACKWARD_MIN_ROWS
            and not skip_layers and len(layers) >= 2 and all(l.bias is None and l.weight.dtype == torch.float32 for l in layers)
            and all(l.weight.shape[0] == 256 for l in layers[:-1]) and layers[-1].weight.shape[0] <= 256
            and all(l.weight.shape[1] == 256 for l in layers[1:]) and layers[0].weight.shape[1] <= 256   # the backward plans the transposed MLP: its last width is dim_in
            and any(l.weight.requires_grad for l in layers)
            and WIDE_MLP_BACKWARD_FUSED)


def wide_mlp_train(x: torch.Tensor, layers, leaky: bool) -> torch.Tensor:
    return _wide_mlp_train.apply(x, leaky, *[l.weight for l in layers])


def _act_torch(h: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.nn.functional.relu(h, inplace=True)
    if act == ACT_LEAKY:
        return torch.nn.functional.leaky_relu(h, inplace=True)
    return h


def small_linear(x: torch.Tensor, layer: torch.nn.Linear, act: int = ACT_NONE) -> torch.Tensor:
    """act(layer(x)) for the layers no fused kernel covers.  fp32 CUDA tensors run the library's own matrix product (sn_gemm_f32) in both
    directions and the deterministic weight-gradient kernel -- without autograd the activation (ACT_RELU / ACT_LEAKY) rides in the product's
    epilogue; other tensors (CPU twins of the tests, autocast) run the torch layer."""
    w = layer.weight
    rows = x.numel() // max(x.shape[-1], 1)
    needs_grad = torch.is_grad_enabled() and (w.requires_grad or x.requires_grad or (layer.bias is not None and layer.bias.requires_grad))
    if gemm_ok(x, w, layer.bias) and rows > 0:
        if needs_grad:
            return _act_torch(_small_linear.apply(x, w, layer.bias), act)
        return linear_forward(x, w, layer.bias, act)
    if (torch.is_grad_enabled() and w.requires_grad and x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32
            and w.shape[0] <= LINEAR_WGRAD_MAX_OUT and rows >= LINEAR_WGRAD_MIN_ROWS):
        return _act_torch(_small_linear.apply(x, w, layer.bias), act)
    return _act_torch(layer(x), act)
