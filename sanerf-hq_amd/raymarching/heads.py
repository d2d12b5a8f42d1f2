"""The 256-wide head MLPs and the heads fused with the compositing (heads.hip, mlp.hip):

    grid_composite       nerf/renderer.py:301-302 + 361: composite(weights, s_grid(xyzs)) fused (inference)
    mlp_forward          nerf/network.py:31-66 (+ LayerNorm :115): the 256-wide head MLPs on the matrix cores (inference)
    mask_head            nerf/renderer.py:304-305, 376-385: grid gather -> mask MLP -> compositing in one kernel (inference)
    mask_point_labels    the same kernel with a label epilogue: per-sample argmax of the mask field (render_object; raymarching/object.py)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._args import _f32
from .render import _fill_grid, _fill_mlp

check_range_default = False   # mlp_forward(check_range=None): read the overflow flag after every call (one device sync each)


def grid_composite(weights: torch.Tensor, xyzs: torch.Tensor, encoder, bound: float = 1.0, tile_w: int = 0,
                   table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """composite(weights, encoder(xyzs, bound)) in one kernel (renderer.py:301-302 + 361): [N,T], [N,T,3] -> [N, L*C].
    Inference only: no autograd graph is recorded (training uses encoder(...) + composite(...))."""
    N, T = weights.shape
    assert xyzs.shape == (N, T, 3), f"xyzs {tuple(xyzs.shape)} does not match weights {tuple(weights.shape)}"
    L = _lib.lib()
    emb = (encoder.embeddings if table is None else table).detach()
    w, x = _f32(weights), _f32(xyzs)
    out = torch.empty(N, encoder.output_dim, device=w.device, dtype=torch.float32)
    desc = _lib.GridDesc()
    _fill_grid(desc, encoder, emb.contiguous())
    _lib.check(L.sn_rm_grid_composite(_lib.dev(x, "xyzs"), _lib.dev(w, "weights"), N, T, float(bound), C.byref(desc),
                                      int(tile_w), _lib.dev(out, "out"), _lib.stream()), "sn_rm_grid_composite")
    return out


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
    raise if an activation left the fp16 range -- the inputs are run-time data, so no static bound exists for this kernel.
    Rows are not rescaled: an input or weight v is held to within max(2^-23 |v|, 2^-25), an ABSOLUTE floor below |v| = 1/4."""
    L = _lib.lib()
    x = _f32(x)
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
        lw, lb = _f32(layer_norm.weight), _f32(layer_norm.bias)
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
    w, x = _f32(weights), _f32(xyzs)
    e = _f32(extra) if E else None
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


def mask_point_labels_fusable(encoder, mlp, T: int, E: int) -> bool:
    """Can sn_rm_mask_point_labels take this head?  What sn_rm_mask_head's 16-row kernel takes: a 3-D fp32 grid with level_dim 8 and at most
    16 levels of the fast-path shape (hash / tiled levels, linear interpolation, no align_corners), a 256-wide perceptron of three bias-free
    layers without skip connections and at most 16 outputs, at most 16 appended channels, a power-of-two number of samples per ray in 4..128."""
    net = list(getattr(mlp, "net", []))
    return (mask_head_fusable(encoder, mlp, T, E) and T >= 4 and len(net) == 3 and all(l.bias is None for l in net) and mlp.dim_out <= 16
            and encoder.num_levels <= 16 and getattr(encoder, "gridtype_id", 0) == 0 and not getattr(encoder, "align_corners", False)
            and getattr(encoder, "interp_id", 0) == 0)


def mask_point_labels(live: torch.Tensor, xyzs: torch.Tensor, extra: torch.Tensor, encoder, mlp, bound: float, want_logits: bool = False):
    """Per-sample labels of the mask field in ONE kernel: labels[n,t] = the lowest index attaining max_k mlp(cat([encoder(xyzs[n,t], bound),
    extra[n,t]]))_k, uint8 [N,T].  live [N,T] (y = delta * sigma): a 128-sample tile (32 consecutive rays x 4 consecutive depth indices) whose
    live values are all exactly 0 is skipped and gets label 255.  want_logits: returns (labels, logits [N,T,K] fp32, 0 on skipped tiles) --
    for tests and tools.  Inference only; raises where mask_point_labels_fusable() is False (there is no second route)."""
    N, T = live.shape
    E = int(extra.shape[-1]) if extra is not None else 0
    assert xyzs.shape == (N, T, 3)
    L = _lib.lib()
    lv, x = _f32(live), _f32(xyzs)
    e = _f32(extra) if E else None
    gdesc = _lib.GridDesc()
    _fill_grid(gdesc, encoder, encoder.embeddings.detach().contiguous())
    mdesc = _lib.MlpDesc()
    keep: list = []
    _fill_mlp(mdesc, list(mlp.net), mlp.dim_in, keep)
    mdesc.activation = 1 if getattr(mlp, "skip_layers", None) is not None else 0      # SkipConnMLP: LeakyReLU(0.01)
    need = int(L.sn_rm_mask_head_workspace_bytes(C.byref(mdesc)))
    if need == 0:
        raise RuntimeError("mask_point_labels: " + L.sn_last_error().decode())
    ws = torch.empty(need, dtype=torch.uint8, device=lv.device)
    labels = torch.empty(N, T, device=lv.device, dtype=torch.uint8)
    logits = torch.empty(N, T, mdesc.dims[mdesc.num_layers], device=lv.device, dtype=torch.float32) if want_logits else None
    _lib.check(L.sn_rm_mask_point_labels(_lib.dev(x, "xyzs"), _lib.dev(e, "extra"), _lib.dev(lv, "live"), N, T, E, float(bound),
                                         C.byref(gdesc), C.byref(mdesc), _lib.dev(labels, "labels", torch.uint8), _lib.dev(logits, "logits"),
                                         ws.data_ptr(), ws.numel(), _lib.stream()), "sn_rm_mask_point_labels")
    return (labels, logits) if want_logits else labels
