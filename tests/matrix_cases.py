"""Shapes, data makers and the two assertions shared by tests/test_matrix_ref64.py (CPU) and tests/test_gpu_matrix_fp32.py (GPU).

The main instrument is EXACT data: small integers stored as float32.  Every product and every partial sum, in any order, slab split or k
permutation, is then an integer below 2^24, which fp32 holds exactly; so is every float64 sum (below 2^53): the float64 statement of
matrix_ref64.py IS the int64 result, and a kernel must reproduce it bit for bit.  Magnitudes:
  chains   x, grad_out in -2..2, weights in {-1, 0, 1}: worst case 32-64-64-16 forward 2*32 = 64 -> 64*64 = 4096 -> 4096*64 = 262 144, backward
           2*16 = 32 -> 2048 -> 131 072.  int_chain() asserts the actual maximum < 2^24 and that a quarter of every hidden layer is positive.
  wgrad    x, dy in -2..2: |sum| <= 4 M, exact up to M = 4 194 304.
  gemm     operands in -3..3, integer bias in -5..5, K <= 300: |sum| <= 2705.
Selection matrices: every weight row is one-hot 1.0 (a different permutation per layer, repeated where a layer widens) and the inputs are the
distinct positive values 1 + row / 2^10 + column / 2^4 (exact): every forward output is bit-equal to one named input element.

Float data only feeds the bound tests: uniform inputs in +-1 and weights uniform in +-1.5 / sqrt(fan_in) as in the older operator tests, inputs
whose magnitudes spread over 2^-20 .. 2^6 (a tensor-wide tolerance hides the small elements), and a whole input row of zeros.
"""
import torch

import matrix_ref64 as R

SHAPES = [(10, 16, 1), (32, 64, 64, 16), (31, 32, 32, 3), (16, 32, 16), (31, 32, 3)]          # SN_SMALL_SHAPES of csrc/mlp_small.hip
SECOND_PASS = 131072                                                                            # 512 workgroups x 4 waves x 64 rows
ROWS = [1, 63, 64, 65, 129, SECOND_PASS, SECOND_PASS + 65]                                       # the last: two tiles into the second pass
FLOAT_KINDS = ("uniform", "spread", "zero_row")
EXACT_LIMIT = float(1 << 24)


def shape_id(shape):
    return "-".join(str(d) for d in shape)


# ---- the two assertions ---------------------------------------------------------------------------------------------------------------
def assert_bits(got, want64, what):
    """got (fp32) must hold exactly the values want64 (float64, each exactly representable in fp32), +0.0 for zero."""
    want = (want64 + 0.0).to(torch.float32)                               # (the statement's products leave -0.0 where a sum from +0.0 never does)
    assert bool((want.double() == want64).all()), f"{what}: the expected values are not exact in fp32 (a mistake of the test)"
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
    if not bool(same.all()):
        bad = (~same).nonzero()
        first = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {same.numel()} elements differ, first at {first}: got {float(got[first])!r}, expected {float(want[first])!r}")


def assert_bound(got, ref, bound, what):
    """`exact and ratio <= 1` against the statement; returns the ratio."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    ratio, exact = R.worst_ratio(got, ref, bound)
    assert exact and ratio <= 1.0, f"{what}: worst |err| / bound {ratio:.3f}, zero-bound elements exact: {exact}"
    return ratio


def plant_zeros(h):
    """A copy of the hidden output h with exact 0.0 at a fixed scatter of places (gates that must close whatever the statement had there)."""
    r = torch.arange(h.shape[0], device=h.device)[:, None]
    c = torch.arange(h.shape[1], device=h.device)[None, :]
    return torch.where((3 * r + c) % 11 == 0, torch.zeros_like(h), h)


def live_share(hidden):
    """Smallest share of positive units over the hidden layers."""
    return min(float((h > 0).double().mean()) for h in hidden) if hidden else 1.0


# ---- exact data -----------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


def int_chain(shape, M):
    """Integer case of one chain on the CPU: x [M, d0], ws, grad_out [M, dL], hidden_in (the fp32 hidden outputs with zeros planted, what the
    backward is given) and the statement's results fwd / bwd (float64 holding integers).  The seed is searched here, deterministically, until
    a quarter of every hidden layer is positive for this row count (one row of a 16-wide layer needs 4 of 16)."""
    for seed in range(64):
        gen = torch.Generator().manual_seed(1000 * len(shape) + 64 * shape[0] + seed)
        ws = [_ints(gen, (b, a), -1, 1) for a, b in zip(shape[:-1], shape[1:])]
        x = _ints(gen, (M, shape[0]), -2, 2)
        fwd = R.chain_forward(x, ws)
        if live_share(fwd["hidden"]) >= 0.25:
            break
    else:
        raise AssertionError(f"no seed gives a live net for {shape} at {M} rows")
    grad_out = _ints(gen, (M, shape[-1]), -2, 2)
    hidden_in = [plant_zeros(h.float()) for h in fwd["hidden"]]
    bwd = R.chain_backward(grad_out, ws, hidden_in)
    peak = max([float(fwd["raw"].abs().max()), float(bwd["grad_in"].abs().max())] + [float(t.abs().max()) for t in fwd["hidden"] + bwd["grad_hidden"]])
    assert peak < EXACT_LIMIT, f"{shape} at {M} rows: |value| reaches {peak}, not exact in fp32"
    for t in [fwd["raw"], bwd["grad_in"]] + fwd["hidden"] + bwd["grad_hidden"]:
        assert bool((t == t.round()).all())
    return dict(x=x, ws=ws, grad_out=grad_out, hidden_in=hidden_in, fwd=fwd, bwd=bwd, live=live_share(fwd["hidden"]), peak=peak)


def selection_chain(shape, M):
    """One-hot weights and distinct positive inputs: x, ws, src (per layer, the input column that each output feature carries), grad_out (distinct
    positive values too) and hidden_in for the backward (the forward's hidden outputs with zeros planted)."""
    gen = torch.Generator().manual_seed(77 + shape[0] + len(shape))
    r = torch.arange(M, dtype=torch.float64)[:, None]
    x = (1.0 + r / 1024.0 + torch.arange(shape[0], dtype=torch.float64)[None, :] / 16.0).float()
    grad_out = (1.0 + r / 1024.0 + torch.arange(shape[-1], dtype=torch.float64)[None, :] / 16.0).float()
    ws, srcs = [], []
    src = torch.arange(shape[0])
    for a, b in zip(shape[:-1], shape[1:]):
        pick = torch.randperm(a, generator=gen)[torch.arange(b) % a]
        W = torch.zeros(b, a)
        W[torch.arange(b), pick] = 1.0
        ws.append(W)
        src = src[pick]
        srcs.append(src)
    hidden_in = [plant_zeros(x[:, s]) for s in srcs[:-1]]
    return dict(x=x, ws=ws, src=srcs, grad_out=grad_out, hidden_in=hidden_in)


def assert_selected(got, x, src, layer, what):
    """got [M, width] must be x[:, src] bit for bit; the message names the (layer, feature) that went to the wrong place."""
    want = x[:, src.to(x.device)]
    same = (got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32))
    if not bool(same.all()):
        bad = (~same).nonzero()
        row, f = int(bad[0][0]), int(bad[0][1])
        wrong = sorted(set(int(v) for v in bad[:, 1].tolist()))
        raise AssertionError(f"{what}: layer {layer} feature {f} (row {row}) should carry input column {int(src[f])} = {float(want[row, f])!r}, "
                             f"got {float(got[row, f])!r}; features off in this layer: {wrong[:16]}")


def int_wgrad(M, K, N, seed=0):
    gen = torch.Generator().manual_seed(31 * M + 7 * K + N + seed)
    return _ints(gen, (M, K), -2, 2), _ints(gen, (M, N), -2, 2)


def int_gemm(M, N, K, seed=0):
    gen = torch.Generator().manual_seed(5 * M + 3 * N + K + seed)
    return _ints(gen, (M, K), -3, 3), _ints(gen, (K, N), -3, 3), _ints(gen, (N,), -5, 5)


# ---- float data -----------------------------------------------------------------------------------------------------------------------
def _uniform(gen, shape):
    return torch.rand(shape, generator=gen) * 2.0 - 1.0


def _spread(gen, shape):
    """Random signs, magnitudes 2^e with e uniform in [-20, 6]."""
    e = torch.rand(shape, generator=gen) * 26.0 - 20.0
    return torch.exp2(e) * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)


def float_rows(kind, M, width, gen):
    if kind == "spread":
        return _spread(gen, (M, width)).float()
    v = _uniform(gen, (M, width)).float()
    if kind == "zero_row":
        v[M // 2] = 0.0
    return v


def float_weights(shape, gen):
    return [(_uniform(gen, (b, a)) * 1.5 / a ** 0.5).float() for a, b in zip(shape[:-1], shape[1:])]


def float_chain(shape, M, kind):
    """x, ws, grad_out of one float case on the CPU (the statement is evaluated by the caller, on its device)."""
    gen = torch.Generator().manual_seed(len(kind) * 100003 + 17 * shape[0] + len(shape) + M)
    ws = float_weights(shape, gen)
    return dict(x=float_rows(kind, M, shape[0], gen), ws=ws, grad_out=float_rows(kind, M, shape[-1], gen))


def placed_raw(M, C, gen):
    """Raw outputs in +-4 with the clamp's edges placed first: +-15 (the clamp itself), +-15.5 (beyond it) and 0."""
    raw = (_uniform(gen, (M, C)) * 4.0).float()
    edges = torch.tensor([15.0, -15.0, 15.5, -15.5, 0.0])
    n = min(M, edges.numel())
    for c in range(C):
        raw[:n, c] = edges.roll(c)[:n]
    return raw
