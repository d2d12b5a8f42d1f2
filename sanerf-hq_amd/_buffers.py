"""Device buffers the operator modules keep between calls (ops.py and raymarching/ both import this; it imports _lib and torch only).
Every call site owns a tag of its own: two operators may run beside each other on two streams (ops._run_beside_backward), so none shares a buffer."""
from __future__ import annotations

import torch

from . import _lib

_scratch: dict = {}     # (tag, device) -> uint8 tensor
_zeroed: dict = {}      # (tag, device.index, stream) -> int64 tensor


def zeros_f32(shape, device) -> torch.Tensor:
    """torch.zeros(shape) whose fill is a library kernel on the current stream (sn_zero; capturable)."""
    t = torch.empty(shape, device=device, dtype=torch.float32)
    nbytes = t.numel() * 4
    if nbytes % 16 == 0 and t.data_ptr() % 16 == 0 and nbytes > 0:
        _lib.check(_lib.lib().sn_zero(t.data_ptr(), nbytes, _lib.stream()), "zero")
    else:
        t.zero_()
    return t


def scratch(tag: str, device, nbytes: int, floor: int = 0) -> torch.Tensor:
    """An uninitialised uint8 workspace of at least nbytes, one per (tag, device): kept while it is large enough, else replaced by a fresh
    allocation of max(nbytes, floor)."""
    ws = _scratch.get((tag, device))
    if ws is None or ws.numel() < nbytes:
        ws = _scratch[(tag, device)] = torch.empty(max(nbytes, floor), dtype=torch.uint8, device=device)
    return ws


def zeroed(tag: str, device, stream: int, nbytes: int) -> torch.Tensor:
    """An int64 workspace of at least nbytes, one per (tag, device.index, stream), for kernels that rely on zero-at-rest: zeroed when it is
    made (its kernels leave it zeroed) and replaced by a new zeroed one when too small."""
    key = (tag, device.index, stream)
    ws = _zeroed.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _zeroed[key] = torch.zeros((nbytes + 7) // 8, device=device, dtype=torch.int64)
    return ws
