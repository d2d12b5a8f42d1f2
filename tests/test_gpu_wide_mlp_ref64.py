"""GPU tests of the 256-wide split-fp16 perceptron kernels of csrc/mlp.hip against tests/wide_ref64.py, per element, in the product library:
k_pack_mlp_wide and k_mlp_wide_j<0|1|2> (sn_mlp_wide_forward through raymarching.mlp_forward), its SAVE = 1 instantiation
(sn_mlp_wide_forward_train_f16x3) and the backward kernels k_mlp_wide<4> (sn_mlp_wide_backward) and k_mlp_wide<5> (sn_mlp_wide_backward_bits).

The training entries go through the raw C ABI, so that hidden, sign_bits and grad_hidden are the test's own buffers (filled with a sentinel
first).  Exact data (wide_cases.py) is asserted bit for bit -- no tolerance anywhere in those tests; float data per element against the derived
bounds of wide_ref64.py, zero-bound elements exact.  The 2^-10-scaled exact cases assert the statement with fp16 SUBNORMALS KEPT: the forward
does not scale its rows, so the lo halves of small inputs are subnormal fp16 values and the matrix cores must honour them.

The id of every forward case ends in the input mode the host's dispatch takes for it (wide_cases.input_mode: 2 = DMA tile, 1 = padded LDS
tile, 0 = read from memory per k-step); the backward tests name their kernel.  Run with -s to see |err| / bound of the float comparisons.
"""
import pytest
import torch

import wide_cases as K
import wide_ref64 as R
from matrix_cases import assert_bits

pytestmark = pytest.mark.gpu

from wide_hip import BACKWARD_ENTRIES, DeviceNet, float_ratios, hip_backward, hip_forward, hip_forward_train, layer_norm_ratio, overflow_flag
from wide_hip import _cpu  # noqa: I001


def test_the_cases_reach_every_input_mode():
    assert {K.input_mode(c.rows, c.net.din) for c in K.FORWARD_CASES} == {0, 1, 2}


# ---- exact data -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.FORWARD_CASES, ids=K.case_id)
def test_forward_is_the_statement_bit_for_bit(gpu, c):
    d = K.make_forward(c)
    dn = DeviceNet(c.net, d["ws"], d["bs"], gpu)
    out = hip_forward(dn, d["x"].to(gpu)).cpu()
    try:
        assert_bits(out, d["fwd"]["raw"], K.case_id(c))
    except AssertionError as e:
        if c.data != "small":
            raise
        flushed = R.chain_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky, keep_subnormals=False)["raw"]
        verdict = "IS met bit for bit" if bool((out.double() == flushed).all()) else "is not met either"
        raise AssertionError(f"{e}; the statement with fp16 subnormals FLUSHED {verdict}") from None
    if c.data == "select":
        assert_bits(out, d["named"], K.case_id(c) + " (the named input elements)")


TRAIN_CASES = [c for c in K.FORWARD_CASES if not c.net.skip] + [K.LEAKY_THREE]


@pytest.mark.parametrize("c", TRAIN_CASES, ids=K.case_id)
def test_training_forward_saves_exact_hidden_outputs_and_their_sign_bits(gpu, c):
    d = K.make_forward(c)
    dn = DeviceNet(c.net, d["ws"], d["bs"], gpu)
    x = d["x"].to(gpu)
    got = _cpu(hip_forward_train(dn, x))
    K.check_forward_bits(c, got, d["fwd"], K.case_id(c))
    exact_layers = 1 if (c.net.leaky and c.data != "select") else c.net.layers - 1
    for l, (h, words) in enumerate(zip(got["hidden"], got["bits"])):
        assert bool((words == R.pack_sign_bits(h > 0)).all()), f"sign_bits[{l}] are not the signs of hidden[{l}]"
        if l < exact_layers:
            assert bool((words == R.pack_sign_bits(d["fwd"]["hidden"][l] > 0)).all()), f"sign_bits[{l}] are not the statement's"
    plain = hip_forward(dn, x).cpu()
    assert bool((plain.view(torch.int32) == got["raw"].view(torch.int32)).all()), "the training forward's output differs from sn_mlp_wide_forward's"


@pytest.mark.parametrize("entry", BACKWARD_ENTRIES)
@pytest.mark.parametrize("c", K.BACKWARD_CASES, ids=K.case_id)
def test_backward_is_the_statement_bit_for_bit(gpu, c, entry):
    d = K.exact_backward(c.net, c.rows)
    dn = DeviceNet(c.net, d["ws"], None, gpu)
    got = _cpu(hip_backward(dn, d["grad_out"].to(gpu), entry, d["gates"]))
    K.check_backward_bits(c, got, d["bwd"], f"{K.case_id(c)} {entry}")
    if c.rows > 2:                                                         # the all-zero row of grad_out
        assert all(bool((t[2].view(torch.int32) == 0).all()) for t in got["grad_hidden"] + [got["grad_in"]]), "an all-zero row must give exact +0.0"


@pytest.mark.parametrize("c", K.BACKWARD_CASES, ids=K.case_id)
def test_backward_entries_agree_bit_for_bit(gpu, c):
    """With the bits of hidden > 0 the two entries are the same function (float data here: every element is live)."""
    d = K.float_net(c.net, c.rows, "spread")
    dn = DeviceNet(c.net, d["ws"], None, gpu)
    gates = K.fixed_gates(c.rows, c.net.layers)
    g = d["grad_out"].to(gpu)
    a, b = (_cpu(hip_backward(dn, g, e, gates)) for e in BACKWARD_ENTRIES)
    for ta, tb in zip(a["grad_hidden"] + [a["grad_in"]], b["grad_hidden"] + [b["grad_in"]]):
        assert bool((ta.view(torch.int32) == tb.view(torch.int32)).all())


# ---- the range edge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [65519.0, 65520.0], ids=["65519-exact", "65520-overflows"])
def test_range_edge_of_the_hi_half(gpu, value):
    c = K.Case(K.Net(64, 256, 3, (), False, False), 129, "select")
    row, col = 40, 7
    x = K.selection_inputs(c.rows, c.net.din)
    x[row, col] = value
    d = K.make_forward(c, x)
    dn = DeviceNet(c.net, d["ws"], d["bs"], gpu)
    overflow_flag()                                                        # (sticky: cleared by the read)
    got = _cpu(hip_forward_train(dn, x.to(gpu)))
    out = hip_forward(dn, x.to(gpu)).cpu()
    flag = overflow_flag()
    others = torch.arange(c.rows) != row
    if value == 65519.0:                                                   # hi 65504, lo 15: inside the range, exact
        assert float(d["fwd"]["hidden"][0].max()) == value and flag == 0
        K.check_forward_bits(c, got, d["fwd"], "65519")
        assert_bits(out, d["fwd"]["raw"], "65519")
    else:                                                                  # hi rounds to inf: the row is lost and the flag says so
        assert flag == 1, "sn_mlp_wide_overflow must report the hidden unit of 65520"
        assert not bool(torch.isfinite(out[row]).any()) and not bool(torch.isfinite(got["raw"][row]).any())
        assert_bits(out[others], d["fwd"]["raw"][others], "the neighbouring rows of the tile")
        for l, h in enumerate(got["hidden"]):
            assert_bits(h[others], d["fwd"]["hidden"][l][others], f"the neighbouring rows of hidden[{l}]")


# ---- float data -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.FLOAT_KINDS)
@pytest.mark.parametrize("c", K.FLOAT_CASES, ids=K.case_id)
def test_float_data_stays_inside_the_bounds(gpu, c, kind):
    for entry, ratio in float_ratios(gpu, c, kind).items():
        print(f"{K.case_id(c)} {kind} {entry}: worst |err| / bound {ratio:.4f}")


@pytest.mark.parametrize("c", K.LAYER_NORM_CASES, ids=K.case_id)
def test_layer_norm_epilogues(gpu, c):
    """Over 256 outputs (the LDS epilogue), over 200 and 2 (the register epilogue), behind a chain whose raw output is EXACT (selection data):
    the bound is the LayerNorm's own rounding count.  A row whose outputs are all equal returns ln.bias itself."""
    ratio, out, d = layer_norm_ratio(gpu, c)
    print(f"{K.case_id(c)} LayerNorm: worst |err| / bound {ratio:.4f}")
    assert bool((out[d["equal_row"]].view(torch.int32) == d["b"].view(torch.int32)).all()), "a row of equal outputs must return ln.bias bit for bit"
