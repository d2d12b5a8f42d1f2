"""CPU anchor of tests/wide_ref64.py, the statement the GPU tests of the 256-wide split-fp16 perceptron kernels compare with
(tests/test_gpu_wide_mlp_ref64.py).

An fp32 emulation of the kernels' scheme -- fp16 casts, three products per k-step of 16 in the order k_pack_mlp_wide packs, fp32 accumulation
from the bias -- must equal the statement bit for bit on every exact case and stay inside its bounds on every float kind; so must torch's own
fp32 matmul chain (a bound tighter than fp32 itself would be a mistake).  A table of MUTATED emulations shows that the exact data can tell:
each of them fails assert_bits on at least one exact case.
"""
import pytest
import torch

import wide_cases as K
import wide_ref64 as R
from matrix_cases import assert_bound
from wide_cases import check_backward_bits, check_forward_bits

MUTATIONS = ("drop Wl*hh", "drop Wh*hl", "add Wl*hl", "swap two k columns in a k-step", "swap across the h|x boundary", "ignore the skip part",
             "drop the bias", "slope 0.01 as a double", "flush lo")


def _halves(v, mut):
    hi = v.half()
    lo = (v - hi.float()).half()
    if mut == "flush lo":
        lo = torch.where(lo.float().abs() < R.F16_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi.float(), lo.float()


def _h_order():
    """The k order of a hidden layer's 256 outputs: k-step ks, half-wave half, slot i <-> register r = 8 (ks & 1) + i of tile ks >> 1."""
    cols = []
    for ks in range(16):
        for half in range(2):
            for i in range(8):
                r = 8 * (ks & 1) + i
                cols.append(32 * (ks >> 1) + (r & 3) + 8 * (r >> 2) + 4 * half)
    return cols


def _emulate_layer(h, x, W, bias, mut, skip, layer):
    """One layer in fp32: h [M, 256] or None, x [M, din] or None (layer 0 and skip layers), W [out, 256? + din?]."""
    M = (h if h is not None else x).shape[0]
    op = torch.cat([t for t in (h, x) if t is not None], 1)
    pairs = []                                                            # (operand column, weight column) in packed order, padded to k-steps of 16
    if h is not None:
        pairs += [(c, c) for c in _h_order()]
    if x is not None and not (mut == "ignore the skip part" and h is not None):
        base = K.WIDE if h is not None else 0
        pairs += [(base + c, base + c) for c in range(x.shape[1])]
        pairs += [None] * (-x.shape[1] % 16)
    if mut == "swap two k columns in a k-step" and layer == 0 and x.shape[1] >= 3:
        (o1, w1), (o2, w2) = pairs[1], pairs[2]
        pairs[1], pairs[2] = (o1, w2), (o2, w1)
    if mut == "swap across the h|x boundary" and skip:
        (o1, w1), (o2, w2) = pairs[K.WIDE - 1], pairs[K.WIDE]
        pairs[K.WIDE - 1], pairs[K.WIDE] = (o1, w2), (o2, w1)
    acc = torch.zeros(M, W.shape[0]) if bias is None or mut == "drop the bias" else bias.float().expand(M, -1).clone()
    zero_op, zero_w = torch.zeros(M, 1), torch.zeros(W.shape[0], 1)
    opz, Wz = torch.cat([op, zero_op], 1), torch.cat([W, zero_w], 1)
    for k0 in range(0, len(pairs), 16):
        step = pairs[k0:k0 + 16]
        oc = [p[0] if p else opz.shape[1] - 1 for p in step]
        wc = [p[1] if p else Wz.shape[1] - 1 for p in step]
        Bh, Bl = _halves(opz[:, oc], mut)
        Ah, Al = _halves(Wz[:, wc], mut)
        if mut != "drop Wl*hh":
            acc = acc + Bh @ Al.t()                                       # small terms first, as the kernels issue them
        if mut != "drop Wh*hl":
            acc = acc + Bl @ Ah.t()
        if mut == "add Wl*hl":
            acc = acc + Bl @ Al.t()
        acc = acc + Bh @ Ah.t()
    return acc


def _slope(t, leaky, mut):
    if not leaky:
        return torch.zeros_like(t)
    return (t.double() * 0.01).float() if mut == "slope 0.01 as a double" else torch.tensor(0.01, dtype=torch.float32) * t


def emulate_forward(x, ws, bs, skip, leaky, mut=None):
    x = x.float()
    h, hs = None, []
    for l, W in enumerate(ws):
        acc = _emulate_layer(h, x if (l == 0 or l in skip) else None, W.float(), bs[l] if bs else None, mut, l in skip, l)
        if l + 1 == len(ws):
            return dict(hidden=hs, raw=acc)
        h = torch.maximum(acc, _slope(acc, leaky, mut))
        hs.append(h)


def emulate_backward(grad_out, ws, gates, leaky, mut=None):
    s = R.row_scale(grad_out).float()
    g = grad_out.float() * s
    L = len(ws)
    dumps = [None] * (L - 1)
    for l in range(L - 1, -1, -1):
        acc = _emulate_layer(g if l < L - 1 else None, g if l == L - 1 else None, ws[l].float().t().contiguous(), None, mut, False, L - 1 - l)
        if l == 0:
            return dict(grad_hidden=dumps, grad_in=acc / s)
        g = torch.where(gates[l - 1], acc, _slope(acc, leaky, mut) if leaky else torch.zeros_like(acc))
        dumps[l - 1] = g / s


def torch_forward(x, ws, bs, skip, leaky):
    """The torch module's arithmetic: fp32 matmuls (nerf/network.py:31-66)."""
    h, hs = x.float(), []
    for l, W in enumerate(ws):
        if l in skip and l > 0:
            h = torch.cat([h, x.float()], 1)
        h = torch.nn.functional.linear(h, W.float(), bs[l].float() if bs and bs[l] is not None else None)
        if l + 1 < len(ws):
            h = torch.nn.functional.leaky_relu(h, 0.01) if leaky else torch.relu(h)
            hs.append(h)
    return dict(hidden=hs, raw=h)


# ---- the statement on exact data --------------------------------------------------------------------------------------------------------
LEAKY_THREE = K.LEAKY_THREE


@pytest.mark.parametrize("c", K.FORWARD_CASES + [LEAKY_THREE], ids=K.case_id)
def test_emulation_equals_the_statement_forward(c):
    d = K.make_forward(c)
    got = emulate_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)
    check_forward_bits(c, got, d["fwd"], K.case_id(c))
    if c.data == "small":                                                 # and the flushed statement is another one: the data can tell them apart
        flushed = R.chain_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky, keep_subnormals=False)
        assert not bool((flushed["raw"] == d["fwd"]["raw"]).all())


@pytest.mark.parametrize("c", K.BACKWARD_CASES, ids=K.case_id)
def test_emulation_equals_the_statement_backward(c):
    d = K.exact_backward(c.net, c.rows)
    got = emulate_backward(d["grad_out"], d["ws"], d["gates"], c.net.leaky)
    check_backward_bits(c, got, d["bwd"], K.case_id(c))
    if c.rows > 2:                                                         # row 2 of grad_out is all zero: exact zeros everywhere
        assert bool((got["grad_in"][2] == 0).all()) and bool((d["bwd"]["grad_in"][2] == 0).all())
        assert all(bool((t[2] == 0).all()) for t in got["grad_hidden"])


def test_backward_rows_scale_exactly():
    """The statement times a power of two per row IS the statement of the scaled rows (2^-60 .. 2^40)."""
    c = K.BACKWARD_CASES[0]
    d = K.exact_backward(c.net, c.rows)
    e = torch.tensor([K.ROW_EXPONENTS[i % len(K.ROW_EXPONENTS)] for i in range(c.rows)], dtype=torch.float64)[:, None]
    base = R.chain_backward((d["grad_out"].double() * torch.exp2(-e)).float(), d["ws"], d["gates"], False)
    assert bool((base["grad_in"] * torch.exp2(e) == d["bwd"]["grad_in"]).all())
    for a, b in zip(base["grad_hidden"], d["bwd"]["grad_hidden"]):
        assert bool((a * torch.exp2(e) == b).all())


# ---- mutations --------------------------------------------------------------------------------------------------------------------------
MUTATION_CASES = [K.Case(K.Net(143, 5, 3, (), False, False), 33, "three"), K.Case(K.Net(143, 5, 3, (), False, False), 33, "small"),
                  K.Case(K.Net(17, 33, 2, (), True, False), 33, "three"), K.Case(K.Net(20, 256, 3, (1,), True, True), 33, "select"),
                  K.Case(K.Net(143, 5, 3, (1,), True, False), 33, "three"), LEAKY_THREE]


@pytest.fixture(scope="module")
def mutation_data():
    return [(c, K.make_forward(c)) for c in MUTATION_CASES]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_every_mutation_is_caught(mut, mutation_data):
    caught = []
    for c, d in mutation_data:
        got = emulate_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky, mut)
        try:
            check_forward_bits(c, got, d["fwd"], K.case_id(c))
        except AssertionError:
            caught.append(K.case_id(c))
    print(f"{mut}: caught by {caught}")
    assert caught, f"no exact case tells the emulation with '{mut}' from the statement"


def test_backward_mutations_are_caught():
    c = K.BACKWARD_CASES[2]
    d = K.exact_backward(c.net, c.rows)
    for mut in MUTATIONS[:4]:
        got = emulate_backward(d["grad_out"], d["ws"], d["gates"], False, mut)
        with pytest.raises(AssertionError):
            check_backward_bits(c, got, d["bwd"], mut)


# ---- float data -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.FLOAT_KINDS)
@pytest.mark.parametrize("c", K.FLOAT_CASES, ids=K.case_id)
def test_emulation_and_plain_fp32_meet_the_bounds(c, kind):
    d = K.float_net(c.net, c.rows, kind)
    fwd = R.chain_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)
    for name, got in (("emulation", emulate_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)),
                      ("plain fp32", torch_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky))):
        worst = [assert_bound(g, w, b, f"{name} hidden[{l}]") for l, (g, w, b) in enumerate(zip(got["hidden"], fwd["hidden"], fwd["hidden_bound"]))]
        worst.append(assert_bound(got["raw"], fwd["raw"], fwd["raw_bound"], f"{name} output"))
        print(f"{K.case_id(c)} {kind} {name}: worst |err| / bound {max(worst):.4f}")
    if not c.net.skip and c.net.din <= K.WIDE:
        gates = [h > 0 for h in fwd["hidden"]]
        bwd = R.chain_backward(d["grad_out"], d["ws"], gates, c.net.leaky)
        got = emulate_backward(d["grad_out"], d["ws"], gates, c.net.leaky)
        for l in range(c.net.layers - 1):
            assert_bound(got["grad_hidden"][l], bwd["grad_hidden"][l], bwd["grad_hidden_bound"][l], f"emulation grad_hidden[{l}]")
        assert_bound(got["grad_in"], bwd["grad_in"], bwd["grad_in_bound"], "emulation grad_in")


@pytest.mark.parametrize("c", K.LAYER_NORM_CASES, ids=K.case_id)
def test_layer_norm_bound_holds_for_fp32_and_is_tight(c):
    """torch's own fp32 LayerNorm of the exact raw output stays inside the bound, which layer_norm_case() has shown to be finite, below 1e-4 of
    the output and tight enough to tell the biased variance from the unbiased one; the statement equals torch's float64 LayerNorm."""
    d = K.layer_norm_case(c)
    raw = R.chain_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)["raw"]
    got = torch.nn.functional.layer_norm(raw.float(), (c.net.dout,), d["w"], d["b"], d["eps"])
    print(f"{K.case_id(c)}: torch fp32 LayerNorm at {assert_bound(got, d['want'], d['bound'], 'LayerNorm of the exact chain'):.4f} of the bound")
    assert bool((got[d["equal_row"]] == d["b"]).all())
    ref = torch.nn.functional.layer_norm(raw, (c.net.dout,), d["w"].double(), d["b"].double(), d["eps"])
    assert float(((d["want"] - ref).abs() / (ref.abs() + 1.0)).max()) < 1e-12


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def test_sign_bits_round_trip():
    gen = torch.Generator().manual_seed(3)
    pos = torch.rand(37, K.WIDE, generator=gen) < 0.5
    pos[0], pos[1] = True, False
    words = R.pack_sign_bits(pos)
    assert words.dtype == torch.int32 and tuple(words.shape) == (37, 8)
    assert bool((words[0] == -1).all()) and bool((words[1] == 0).all())
    assert bool((R.unpack_sign_bits(words) == pos).all())
    one = torch.zeros(1, K.WIDE, dtype=torch.bool)
    one[0, 32 * 3 + 2 + 8 * 1 + 4 * 1] = True                              # tile 3, register r = 4 * 1 + 2 = 6, half-wave 1: word 4 + 1, bit 16 + 6
    assert R.pack_sign_bits(one)[0].tolist() == [0, 0, 0, 0, 0, 1 << 22, 0, 0]


def test_split_keeps_or_flushes_subnormals():
    v = torch.tensor([1.0 + 2.0 ** -12, 2.0 ** -10 + 2.0 ** -22, 2.0 ** -15, 65519.0])
    hi, lo = R.split(v)
    assert hi.tolist() == [1.0, 2.0 ** -10, 2.0 ** -15, 65504.0] and lo.tolist() == [2.0 ** -12, 2.0 ** -22, 0.0, 15.0]
    hi, lo = R.split(v, keep_subnormals=False)
    assert hi.tolist() == [1.0, 2.0 ** -10, 0.0, 65504.0] and lo.tolist() == [2.0 ** -12, 0.0, 0.0, 15.0]


def test_the_cases_reach_every_input_mode():
    assert {K.input_mode(c.rows, c.net.din) for c in K.FORWARD_CASES} == {0, 1, 2}
    assert K.input_mode(1, K.FIRST_EVEN_PAST_LDS - 2) == 1 and K.input_mode(4, 143) == 2 and K.input_mode(33, 143) == 1
