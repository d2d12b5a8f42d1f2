"""Jitter of a perturbed render (jitter.hip):

    jitter               nerf/renderer.py:262-270, 97-102: one stage's perturbed bins / u from caller-supplied uniforms
    jitter_tables        the same tables for every stage in one launch, uniforms from a Philox counter on the device (DeviceJitter)

`jitter_tables(state, N, steps, ...)` / `DeviceJitter(device, seed)` write their tables in one capturable launch from a Philox4x32-10 counter
on the device -- (seed, draw, stage, ray, column) name a value, `draw` advances once per image."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from .. import _lib


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
