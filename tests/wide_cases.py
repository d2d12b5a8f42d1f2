"""Nets, data makers and the host's dispatch rule shared by tests/test_wide_ref64.py (CPU) and tests/test_gpu_wide_mlp_ref64.py (GPU); the two
assertions are matrix_cases.assert_bits / assert_bound.

The decisive instrument is EXACT data: every product the split-fp16 scheme keeps and every partial sum, in any k order, is exact in fp32, so
the float64 statement of wide_ref64.py IS the answer and a kernel must reproduce it bit for bit.
  three-product   for the layer that consumes external input (forward layer 0 and the x part of skip layers; the last forward layer in the
                  backward): weights p (1 + q 2^-12), p, q in {-1, 0, 1}; inputs r + s 2^-12, |r| in {1, 2}, s in {-1, 0, 1}, about one in
                  five zero.  Both halves of both operands are then non-zero, hi*hi is an integer, the cross terms live at 2^-12 and the
                  lo*lo terms, at 2^-24, are what the scheme drops.  All other layers are sparse ternary.  With every value a multiple of
                  2^-12 and every absolute mass (which bounds every partial sum) below 2^10, a sum needs at most 22 bits -- and so does the
                  hidden value that is split again: 11 bits in hi, the rest, signed, in lo.  exact_forward() / exact_backward() assert all of
                  that from the statement, with the share of non-zero lo halves and of positive units, and search their seed deterministically.
                  scale = 2^-10 multiplies inputs and biases: lo halves are then fp16 SUBNORMALS (2^-22), which the forward does not scale away.
  leaky           0.01f t rounds, so only the exact part is asserted: negative first-layer pre-activations as fl(0.01f t) in hidden[0]
                  (the float64 product of two fp32 values, rounded once) and the first backward layer's dump.
  selection       one-hot weight rows, another permutation per layer and over cat([h, x]) in skip layers; inputs are distinct values with 22
                  significant bits in [128, 32768) (lo normal and non-zero); integer bias on the last layer only (a sum would not split
                  exactly again).  Every output is one named input element (+ its bias); every unit is positive, so leaky nets are exact too.
  range edge      selection data with one input element of 65519 (hi 65504, lo 15: exact, flag clear) or 65520 (hi rounds to inf).

Float data feeds the bounds: uniform (inputs +-1, weights +-1.5 / sqrt(fan_in)), spread (magnitudes 2^-20 .. 2^6 per element), zero_row,
fresh_field (128 columns at +-1e-4 and 15 to 35 columns of N(0, 1): the heads' input at a new table) and all_small (every input +-1e-4).
"""
from collections import namedtuple

import torch

import wide_ref64 as R
from matrix_cases import _spread, _uniform, assert_bits, live_share

WIDE = R.WIDE
MAX_LAYERS = 8                                                           # SN_MAX_LAYERS
FLOAT_KINDS = ("uniform", "spread", "zero_row", "fresh_field", "all_small")
SMALL = 2.0 ** -10

Net = namedtuple("Net", "din dout layers skip bias leaky")


def net_id(n):
    return (f"{n.din}-{n.layers}x-{n.dout}" + ("-skip" + ".".join(str(s) for s in n.skip) if n.skip else "") + ("-bias" if n.bias else "")
            + ("-leaky" if n.leaky else "-relu"))


def weight_shapes(n):
    dims = [n.din] + [WIDE] * (n.layers - 1) + [n.dout]
    return [(dims[l + 1], dims[l] + (n.din if l in n.skip else 0)) for l in range(n.layers)]


def input_mode(rows, din):
    """The input mode wide_forward_impl (csrc/mlp.hip) takes: 2 = the tile's inputs copied verbatim into LDS by DMA, 1 = copied into padded LDS
    rows with ordinary loads, 0 = too wide for LDS, read per k-step."""
    xs = (din + 3) & ~3
    if ((xs >> 2) & 1) == 0:
        xs += 4
    fixed = 4 * 1024 * 16 + MAX_LAYERS * WIDE * 4
    x1 = (128 * xs + 32) * 4
    x2 = 128 * din * 4 + 1024
    cap = 160 * 1024
    dma_ok = (din & 1) == 1 and fixed + x2 <= cap and rows * din >= 4 and ((rows * din) % 4 == 0 or rows % 128 == 0)
    return 2 if dma_ok else (1 if fixed + x1 <= cap else 0)


FIRST_EVEN_PAST_LDS = next(d for d in range(2, 1025, 2) if input_mode(1, d) == 0)


# ---- exact data: three products ---------------------------------------------------------------------------------------------------------
def _pick(gen, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs, dtype=torch.float64), int(torch.tensor(shape).prod()), replacement=True, generator=gen)
    return torch.tensor(values, dtype=torch.float64)[idx].reshape(shape)


def _three_weights(gen, shape, fan):
    """p (1 + q 2^-12); the share of non-zero p falls with the fan-in so that the absolute mass stays below 2^10."""
    d = min(2.0 / 3.0, 96.0 / fan)
    p = _pick(gen, shape, [-1.0, 0.0, 1.0], [d / 2, 1 - d, d / 2])
    q = _pick(gen, shape, [-1.0, 0.0, 1.0], [1 / 3, 1 / 3, 1 / 3])
    return (p * (1.0 + q * 2.0 ** -12)).float()


def _three_values(gen, shape):
    r = _pick(gen, shape, [-2.0, -1.0, 0.0, 1.0, 2.0], [0.2, 0.2, 0.2, 0.2, 0.2])
    s = _pick(gen, shape, [-1.0, 0.0, 1.0], [1 / 3, 1 / 3, 1 / 3])
    return torch.where(r == 0, r, r + s * 2.0 ** -12).float()


def _ternary(gen, shape, per_row):
    """Sparse {-1, 0, 1}: about per_row non-zeros in every row of 256, three in five of them +1 (a net of these stays alive and bounded)."""
    d = per_row / WIDE
    return _pick(gen, shape, [-1.0, 0.0, 1.0], [0.4 * d, 1 - d, 0.6 * d]).float()


def _assert_exact(values, masses, unit, what):
    for i, v in enumerate(values):
        assert bool(((v / unit) == (v / unit).round()).all()), f"{what}: value {i} is no multiple of the unit"
        hi, lo = R.split(v)
        assert bool((hi + lo == v).all()), f"{what}: value {i} does not split exactly"
    peak = max(float(m.max()) for m in masses)
    assert peak / unit < 2.0 ** 22, f"{what}: absolute mass {peak} needs more than 22 bits at unit {unit}"
    return peak


def exact_forward(net, M, scale=1.0):
    """Three-product case of a ReLU net (leaky: only hidden[0] is exact, see above) on the CPU: x, ws, bs and fwd = the statement."""
    unit = scale * 2.0 ** -12
    shapes = weight_shapes(net)
    per_row = 4 if net.layers <= 3 else 3
    for seed in range(64):
        gen = torch.Generator().manual_seed(7919 * net.layers + 31 * net.din + net.dout + 1000003 * seed)
        ws = []
        for l, (o, i) in enumerate(shapes):
            if l == 0:
                ws.append(_three_weights(gen, (o, i), i))
            else:
                parts = [_ternary(gen, (o, WIDE), per_row)]
                if l in net.skip:
                    parts.append(_three_weights(gen, (o, net.din), 2 * net.din))
                ws.append(torch.cat(parts, 1))
        bs = [(_pick(gen, (o,), [-2.0, -1.0, 0.0, 1.0, 2.0], [0.2] * 5) * scale).float() for o, _ in shapes] if net.bias else None
        x = _three_values(gen, (M, net.din)) * scale
        fwd = R.chain_forward(x, ws, bs, net.skip, net.leaky)
        if net.layers == 1 or (live_share(fwd["hidden"]) >= 0.25 and max(float(m.max()) for m in fwd["mass"]) / unit < 2.0 ** 22):
            break
    else:
        raise AssertionError(f"no seed gives a live, exact net for {net_id(net)} at {M} rows")
    if net.leaky:                                                         # only layer 0 is exact: its pre-activations are hidden[0] before 0.01f t
        peak = _assert_exact([], fwd["mass"][:1], unit, net_id(net))
    else:
        peak = _assert_exact(fwd["hidden"] + [fwd["raw"]], fwd["mass"], unit, net_id(net))
    maxima = [float(t.abs().max()) for t in fwd["hidden"] + [fwd["raw"]]]
    assert max(maxima) < 65504.0
    if net.layers > 1:
        lo = R.split(fwd["hidden"][0])[1]
        assert float((lo != 0).double().mean()) >= 0.25, "the first hidden layer carries too few non-zero lo halves"
    if scale != 1.0:
        assert float(R.split(x)[1].abs().max()) < R.F16_MIN_NORMAL, "the scaled inputs' lo halves are meant to be fp16 subnormals"
    return dict(x=x, ws=ws, bs=bs, fwd=fwd, peak=peak, maxima=maxima)


def fixed_gates(M, layers):
    """Gates of the hidden layers that no forward produced: a fixed scatter with row 0 all set and row 1 all clear."""
    r = torch.arange(M)[:, None]
    c = torch.arange(WIDE)[None, :]
    gates = []
    for l in range(layers - 1):
        g = (3 * r + 5 * c + 7 * l) % 11 < 6
        g[0] = True
        if M > 1:
            g[1] = False
        gates.append(g)
    return gates


ROW_EXPONENTS = [0, -60, 40, -23, 5, -1]


def exact_backward(net, M):
    """Three-product case of the backward: the LAST forward layer's weights are p (1 + q 2^-12), all others sparse ternary; grad_out rows are
    r + s 2^-12 times a power of two 2^-60 .. 2^40 per row, one row all zero; gates from fixed_gates() -> ws, grad_out, gates, bwd."""
    assert not net.skip and net.layers >= 2
    shapes = weight_shapes(net)
    for seed in range(64):
        gen = torch.Generator().manual_seed(104729 * net.layers + 17 * net.din + net.dout + 1000003 * seed)
        ws = [_ternary(gen, s, 4) for s in shapes[:-1]] + [_three_weights(gen, shapes[-1], 2 * net.dout)]
        g = _three_values(gen, (M, net.dout)).double()
        e = torch.tensor([ROW_EXPONENTS[i % len(ROW_EXPONENTS)] for i in range(M)], dtype=torch.float64)[:, None]
        grad_out = (g * torch.exp2(e)).float()
        if M > 2:
            grad_out[2] = 0.0
        gates = fixed_gates(M, net.layers)
        bwd = R.chain_backward(grad_out, ws, gates, net.leaky)
        if max(float(m.max()) for m in bwd["mass"]) < 2.0 ** 9:
            break
    else:
        raise AssertionError(f"no seed gives an exact backward for {net_id(net)} at {M} rows")
    s = bwd["scale"]
    unit = 2.0 ** -13                                                     # the scaled rows: (r + s 2^-12) / 2 where the largest entry is 2 or more
    scaled = [] if net.leaky else [t * s for t in bwd["grad_hidden"]] + [bwd["scaled_in"]]      # (leaky: the first dump is fl(0.01f t), one rounding)
    _assert_exact(scaled, bwd["mass"][-1:] if net.leaky else bwd["mass"], unit, net_id(net) + " backward")
    return dict(ws=ws, grad_out=grad_out, gates=gates, bwd=bwd)


# ---- exact data: selection --------------------------------------------------------------------------------------------------------------
def selection_inputs(M, din):
    """Distinct values 2^e (1 + m 2^-21), m odd, e in 7 .. 14: 22 significant bits, hi and lo non-zero, lo normal."""
    assert M <= 1024 and din <= 1024
    r = torch.arange(M, dtype=torch.float64)[:, None]
    c = torch.arange(din, dtype=torch.float64)[None, :]
    m = 2.0 * (r * 1024.0 + c) + 1.0
    x = torch.exp2(7.0 + (c % 8)) * (1.0 + m * 2.0 ** -21)
    hi, lo = R.split(x)
    assert bool((x.float().double() == x).all()) and bool((lo != 0).all()) and bool((lo.abs() >= R.F16_MIN_NORMAL).all()) and bool((hi + lo == x).all())
    return x.float()


def selection_forward(net, M, x=None):
    """x, ws, bs, src (per layer, the input column each output carries) and fwd = the statement, which is asserted to equal the named elements."""
    gen = torch.Generator().manual_seed(77 + net.din + 13 * net.layers + net.dout)
    x = selection_inputs(M, net.din) if x is None else x
    ws, srcs = [], []
    src = torch.arange(net.din)
    for l, (o, i) in enumerate(weight_shapes(net)):
        pick = torch.randperm(i, generator=gen)[torch.arange(o) % i]
        W = torch.zeros(o, i)
        W[torch.arange(o), pick] = 1.0
        ws.append(W)
        if l == 0:
            src = pick
        else:
            src = torch.where(pick < WIDE, src[pick.clamp(max=WIDE - 1)], pick - WIDE)
        srcs.append(src)
    bs = None
    if net.bias:
        bs = [None] * (net.layers - 1) + [torch.randint(-3, 4, (net.dout,), generator=gen).float()]
    fwd = R.chain_forward(x, ws, bs, net.skip, net.leaky)
    named = x.double()[:, srcs[-1]] + (bs[-1].double() if bs else 0.0)
    finite = torch.isfinite(fwd["raw"])                                   # (a range-edge row beyond fp16 is not finite in the statement)
    assert bool((fwd["raw"][finite] == named[finite]).all()), "the statement does not select the named elements (a mistake of the test)"
    return dict(x=x, ws=ws, bs=bs, src=srcs, fwd=fwd, named=named)


# ---- float data -------------------------------------------------------------------------------------------------------------------------
def float_rows(kind, M, width, gen):
    if kind == "spread":
        return _spread(gen, (M, width)).float()
    if kind == "all_small":
        return (_uniform(gen, (M, width)) * 1e-4).float()
    if kind == "fresh_field":
        v = (_uniform(gen, (M, width)) * 1e-4).float()
        wide = min(width, max(15, min(35, width - 128)))                  # 15 .. 35 columns of N(0, 1), the rest (128 in the heads) a fresh table's +-1e-4
        v[:, width - wide:] = torch.randn((M, wide), generator=gen)
        return v
    v = _uniform(gen, (M, width)).float()
    if kind == "zero_row":
        v[M // 2] = 0.0
    return v


def float_net(net, M, kind):
    """x, ws, bs, grad_out of one float case on the CPU."""
    gen = torch.Generator().manual_seed(len(kind) * 100003 + 17 * net.din + net.layers + M + net.dout)
    ws = [(_uniform(gen, s) * 1.5 / s[1] ** 0.5).float() for s in weight_shapes(net)]
    bs = [(_uniform(gen, (s[0],)) * 0.1).float() for s in weight_shapes(net)] if net.bias else None
    grad_kind = kind if kind in ("uniform", "spread", "zero_row") else "uniform"
    return dict(x=float_rows(kind, M, net.din, gen), ws=ws, bs=bs, grad_out=float_rows(grad_kind, M, net.dout, gen))


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "net rows data")                                # data: "three", "small" (three-product data times 2^-10) or "select"
_N = Net
FORWARD_CASES = [
    Case(_N(1, 1, 2, (), False, False), 1, "three"),
    Case(_N(15, 2, 2, (), True, False), 31, "three"),
    Case(_N(16, 5, 3, (), False, False), 33, "three"),
    Case(_N(17, 33, 2, (), True, False), 127, "three"),                  # narrow last layer, two tiles
    Case(_N(17, 256, 1, (), True, False), 33, "three"),                  # a single layer, the LDS output path
    Case(_N(64, 64, 2, (), False, False), 129, "three"),                 # even width: the padded LDS tile
    Case(_N(64, 5, 1, (), True, False), 31, "select"),
    Case(_N(143, 5, 3, (), False, False), 261, "three"),                 # the mask head; 261 * 143 % 4 != 0
    Case(_N(143, 5, 3, (), False, False), 260, "small"),                 # 260 * 143 % 4 == 0: the DMA tile, partial last tile
    Case(_N(143, 2, 3, (), False, False), 4, "three"),
    Case(_N(143, 5, 3, (2,), True, True), 33, "select"),                 # a skip into the last layer
    Case(_N(143, 65, 3, (1,), False, True), 261, "select"),              # three output tiles, scalar stores
    Case(_N(143, 40, 5, (), True, False), 129, "three"),
    Case(_N(163, 256, 5, (2,), True, False), 129, "three"),              # the SAM head's shape
    Case(_N(163, 256, 5, (2,), True, False), 36, "small"),
    Case(_N(163, 256, 5, (2,), True, True), 33, "select"),
    Case(_N(163, 200, 2, (), False, False), 1, "three"),                 # out & 3 == 0, partial tile
    Case(_N(FIRST_EVEN_PAST_LDS, 65, 2, (), False, False), 31, "three"),
    Case(_N(700, 200, 3, (1,), True, True), 33, "select"),
    Case(_N(700, 5, 2, (), False, False), 127, "small"),
    Case(_N(1024, 255, 2, (), False, False), 127, "three"),              # the documented maximum
    Case(_N(1024, 1, 3, (1, 2), True, True), 31, "select"),              # two skip layers
    Case(_N(64, 256, MAX_LAYERS, (3, 6), True, True), 129, "select"),
    Case(_N(64, 33, 5, (), True, False), 261, "small"),
    Case(_N(16, 64, MAX_LAYERS, (), False, False), 33, "select"),
]
BACKWARD_CASES = [
    Case(_N(143, 2, 3, (), False, False), 33, "three"),
    Case(_N(64, 5, 2, (), False, False), 129, "three"),                  # narrow last backward layer
    Case(_N(256, 40, 3, (), False, False), 261, "three"),
    Case(_N(1, 256, 5, (), False, False), 31, "three"),
    Case(_N(64, 2, 2, (), False, False), 1, "three"),
    Case(_N(143, 5, 3, (), False, True), 127, "three"),                  # leaky: the first dump only
]
FLOAT_CASES = [
    Case(_N(143, 5, 3, (), False, False), 129, "float"),
    Case(_N(163, 256, 5, (2,), True, True), 33, "float"),
    Case(_N(64, 200, 2, (), True, False), 31, "float"),
    Case(_N(700, 33, 3, (1,), False, True), 33, "float"),
    Case(_N(64, 5, 3, (), False, True), 33, "float"),                    # leaky without a skip layer: the saved hidden outputs and the backward beyond its first dump
]
LAYER_NORM_CASES = [                                                     # over 256: the LDS epilogue; over 200 and 2: the register epilogue
    Case(_N(163, 256, 5, (2,), False, True), 33, "select"),
    Case(_N(64, 200, 2, (), False, False), 31, "select"),
    Case(_N(17, 2, 2, (), False, False), 33, "select"),
]


def case_id(c):
    return f"{net_id(c.net)}-{c.rows}rows-{c.data}-mode{input_mode(c.rows, c.net.din)}"


def make_forward(c, x=None):
    """x, ws, bs and fwd (the statement) of an exact forward case on the CPU."""
    if c.data == "select":
        return selection_forward(c.net, c.rows, x)
    return exact_forward(c.net, c.rows, SMALL if c.data == "small" else 1.0)


def layer_norm_case(c):
    """A LayerNorm case: selection data, so the chain's raw output is EXACT (E = 0) and the bound is the LayerNorm's own rounding count; row
    `equal_row` of x is all 3.0, so its outputs are all equal.  Asserts that the bound is finite and a small fraction of the output, and
    that it tells the biased variance from the unbiased one -> x, ws, bs, w, b, eps, want, bound, equal_row."""
    x = selection_inputs(c.rows, c.net.din)
    equal_row = c.rows // 2
    x[equal_row] = 3.0
    d = selection_forward(c.net, c.rows, x)
    y = d["fwd"]["raw"]
    assert bool((y[equal_row] == 3.0).all()) and bool((y.float().double() == y).all())
    gen = torch.Generator().manual_seed(11 + c.net.dout)
    w, b, eps = torch.rand(c.net.dout, generator=gen) + 0.5, torch.rand(c.net.dout, generator=gen) - 0.5, 1e-5
    want, bound = R.layer_norm(y, w, b, eps)
    others = torch.arange(c.rows) != equal_row
    assert bool(torch.isfinite(bound).all()), "the LayerNorm bound must be finite"
    assert float((bound[others].amax(1) / want[others].abs().amax(1)).max()) < 1e-4, "the LayerNorm bound must be a small fraction of the output"
    n = c.net.dout
    unbiased = (y - y.mean(1, keepdim=True)) * (y.var(1, unbiased=True, keepdim=True) + eps).rsqrt() * w.double() + b.double()
    assert bool((((unbiased - want).abs() > bound)[others]).any()), f"the bound over {n} outputs does not tell var / n from var / (n - 1)"
    return dict(x=x, ws=d["ws"], bs=d["bs"], w=w, b=b, eps=eps, want=want, bound=bound, equal_row=equal_row)


LEAKY_THREE = Case(_N(64, 2, 2, (), False, True), 33, "three")            # a leaky net on three-product data: hidden[0] is the exact part


# ---- what is asserted bit for bit of an exact case ----------------------------------------------------------------------------------------
def round32(t):
    """The float64 value rounded once to fp32: fl(0.01f t) of an exact t."""
    return t.float().double()


def check_forward_bits(c, got, fwd, what):
    """assert_bits on what is exact of a forward case: everything of a ReLU or selection case, hidden[0] as fl(0.01f t) of a leaky three-product one."""
    if c.net.leaky and c.data != "select":
        if fwd["hidden"]:
            assert_bits(got["hidden"][0], round32(fwd["hidden"][0]), f"{what} hidden[0]")
        return
    for l, (g, w) in enumerate(zip(got["hidden"], fwd["hidden"])):
        assert_bits(g, w, f"{what} hidden[{l}]")
    assert_bits(got["raw"], fwd["raw"], f"{what} output")


def check_backward_bits(c, got, bwd, what):
    L = c.net.layers
    if c.net.leaky:
        assert_bits(got["grad_hidden"][L - 2], round32(bwd["grad_hidden"][L - 2]), f"{what} grad_hidden[{L - 2}]")
        return
    for l in range(L - 1):
        assert_bits(got["grad_hidden"][l], bwd["grad_hidden"][l], f"{what} grad_hidden[{l}]")
    assert_bits(got["grad_in"], bwd["grad_in"], f"{what} grad_in")
