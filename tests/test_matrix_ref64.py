"""CPU anchors of tests/matrix_ref64.py and tests/matrix_cases.py (no GPU): what the GPU tests of tests/test_gpu_matrix_fp32.py rest on.

  * the statement against independent ones: a per-row Python loop in float64, torch autograd in float64, an int64 matrix product;
  * an fp32 emulation of every operator (numpy float32, one fma chain per output, k ascending and k shuffled) stays inside every bound;
    the worst ratios are printed (pytest -s) and recorded in the table of test_gpu_matrix_fp32.py;
  * sensitivity: the bound assertion FAILS for (a) operands cut to 10 mantissa bits before the products, (b) two hidden features swapped in one
    layer, (c) the gate taken from the wrong layer, (d) the 1 - s factor dropped from the sigmoid's backward; the exact assertion FAILS for
    (e) one row of M dropped, (f) one row counted twice, (g) k and k + 1 swapped in one layer's permuted order;
  * the integer cases satisfy their own two conditions for every shape and row count the GPU tests use.
"""
import numpy as np
import pytest
import torch

import matrix_cases as K
import matrix_ref64 as R

F32, F64 = np.float32, np.float64


# ---- fp32 emulation -------------------------------------------------------------------------------------------------------------------
def cut10(a):
    """fp32 values with the mantissa cut to 10 bits (what a reduced-precision matrix path would multiply)."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFFE000)).view(F32)


def fma_rows(h, W, order=None, trunc=False):
    """h [M, K] fp32, W [N, K] fp32 -> [M, N] fp32: per output one chain acc = fma(h[k], W[k], acc) over k in `order` (ascending by default).
    The float64 product of two fp32 values is exact, so each step rounds once."""
    h, W = np.asarray(h, F32), np.asarray(W, F32)
    if trunc:
        h, W = cut10(h), cut10(W)
    acc = np.zeros((h.shape[0], W.shape[0]), F32)
    for k in (range(h.shape[1]) if order is None else order):
        acc = (h[:, k, None].astype(F64) * W[None, :, k].astype(F64) + acc.astype(F64)).astype(F32)
    return acc


def _order(K_, rng):
    return None if rng is None else rng.permutation(K_)


def emu_forward(x, ws, rng=None, trunc=False, swap_layer=None, kswap=None):
    """The chain in fp32.  Faults: trunc (a), swap_layer: features 0 and 1 of that hidden layer exchanged (b), kswap = (layer, k): that layer
    reads weight columns k and k + 1 in each other's place (g)."""
    h = x.numpy()
    hs = []
    for l, W in enumerate(ws):
        Wn = W.numpy()
        if kswap is not None and kswap[0] == l:
            k = kswap[1]
            Wn = Wn.copy()
            Wn[:, [k, k + 1]] = Wn[:, [k + 1, k]]
        a = fma_rows(h, Wn, _order(Wn.shape[1], rng), trunc)
        if l + 1 < len(ws):
            h = np.maximum(a, F32(0))
            if swap_layer == l:
                h = h.copy()
                h[:, [0, 1]] = h[:, [1, 0]]
            hs.append(torch.from_numpy(h))
    return hs, torch.from_numpy(a)


def emu_backward(g_last, ws, hidden_in, rng=None, wrong_gate=False):
    """The backward data path in fp32 with the hidden outputs given.  Fault (c): every gate taken from the neighbouring hidden layer."""
    g = g_last.numpy()
    L = len(ws)
    gh = [None] * (L - 1)
    for l in range(L - 1, 0, -1):
        t = fma_rows(g, ws[l].numpy().T, _order(ws[l].shape[0], rng))
        src = l - 1
        if wrong_gate:
            src = l - 2 if l >= 2 else l                     # (the caller picks a shape whose neighbouring hidden layers have one width)
        g = np.where(hidden_in[src].numpy() > 0, t, F32(0)).astype(F32)
        gh[l - 1] = torch.from_numpy(g)
    return gh, torch.from_numpy(fma_rows(g, ws[0].numpy().T, _order(ws[0].shape[0], rng)))


def emu_sigmoid(x):
    return (F32(1) / (F32(1) + np.exp(-x).astype(F32))).astype(F32)


def emu_act_forward(act, raw, aux_in, bg):
    raw = raw.numpy()
    if act == R.ACT_TRUNC_EXP0:
        return torch.from_numpy(np.exp(raw[:, 0]).astype(F32))
    t = ((F32(1) - aux_in.numpy()) * F32(bg)).astype(F32)
    return torch.from_numpy((emu_sigmoid(raw) + t[:, None]).astype(F32))


def emu_act_backward(act, raw, g_raw, g_aux, bg, drop_one_minus_s=False):
    raw = raw.numpy()
    g0 = np.zeros_like(raw) if g_raw is None else g_raw.numpy().copy()
    if act == R.ACT_TRUNC_EXP0:
        e = np.exp(np.clip(raw[:, 0], F32(-15), F32(15))).astype(F32)
        g0[:, 0] = (g_aux.numpy().reshape(-1).astype(F64) * e.astype(F64) + g0[:, 0].astype(F64)).astype(F32)
        return torch.from_numpy(g0), None
    s = emu_sigmoid(raw)
    d = s if drop_one_minus_s else (s * (F32(1) - s)).astype(F32)
    ga = g_aux.numpy()
    out = (ga.astype(F64) * d.astype(F64) + g0.astype(F64)).astype(F32)
    gsum = np.zeros(raw.shape[0], F32)
    for c in range(raw.shape[1]):
        gsum = (gsum + ga[:, c]).astype(F32)
    return torch.from_numpy(out), torch.from_numpy((-F32(bg) * gsum).astype(F32))


M_EMU = 48


def _float_case(shape, kind):
    c = K.float_chain(shape, M_EMU, kind)
    fwd = R.chain_forward(c["x"], c["ws"])
    c["fwd"] = fwd
    c["hidden_in"] = [K.plant_zeros(h.float()) for h in fwd["hidden"]]
    c["bwd"] = R.chain_backward(c["grad_out"], c["ws"], c["hidden_in"])
    return c


def check_forward(c, hs, raw, what):
    r = 0.0
    for l, h in enumerate(hs):
        r = max(r, K.assert_bound(h, c["fwd"]["hidden"][l], c["fwd"]["hidden_bound"][l], f"{what} hidden[{l}]"))
    return max(r, K.assert_bound(raw, c["fwd"]["raw"], c["fwd"]["raw_bound"], f"{what} raw"))


def check_backward(c, gh, gi, what, ref=None):
    ref = c["bwd"] if ref is None else ref
    r = 0.0
    for l, g in enumerate(gh):
        r = max(r, K.assert_bound(g, ref["grad_hidden"][l], ref["grad_hidden_bound"][l], f"{what} grad_hidden[{l}]"))
    return max(r, K.assert_bound(gi, ref["grad_in"], ref["grad_in_bound"], f"{what} grad_in"))


# ---- the statement against independent ones -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(10, 16, 1), (31, 32, 32, 3)], ids=K.shape_id)
def test_statement_equals_a_per_row_loop(shape):
    c = K.float_chain(shape, 5, "uniform")
    fwd = R.chain_forward(c["x"], c["ws"])
    hidden_in = [K.plant_zeros(h.float()) for h in fwd["hidden"]]
    bwd = R.chain_backward(c["grad_out"], c["ws"], hidden_in)
    ws = [[[float(v) for v in row] for row in W.tolist()] for W in c["ws"]]
    for m in range(5):
        h = [float(v) for v in c["x"][m].tolist()]
        for l, W in enumerate(ws):
            a = [sum(wv * hv for wv, hv in zip(row, h)) for row in W]
            if l + 1 < len(ws):
                h = [max(v, 0.0) for v in a]
                assert np.allclose(h, fwd["hidden"][l][m].numpy(), rtol=1e-13, atol=1e-15)
        assert np.allclose(a, fwd["raw"][m].numpy(), rtol=1e-13, atol=1e-15)
        g = [float(v) for v in c["grad_out"][m].tolist()]
        for l in range(len(ws) - 1, -1, -1):
            g = [sum(ws[l][i][k] * g[i] for i in range(len(g))) for k in range(len(ws[l][0]))]
            if l > 0:
                g = [gv if float(hidden_in[l - 1][m, k]) > 0 else 0.0 for k, gv in enumerate(g)]
                assert np.allclose(g, bwd["grad_hidden"][l - 1][m].numpy(), rtol=1e-13, atol=1e-15)
        assert np.allclose(g, bwd["grad_in"][m].numpy(), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("shape,act", [(s, a) for s in K.SHAPES for a in (R.ACT_NONE, R.ACT_TRUNC_EXP0, R.ACT_SIGMOID_BG) if a != R.ACT_SIGMOID_BG or s[-1] <= 4],
                         ids=lambda v: K.shape_id(v) if isinstance(v, tuple) else f"act{v}")
def test_statement_backward_equals_autograd(shape, act):
    """The whole statement (chain, activation, both gradient arrivals) against torch autograd in float64, on the rows where no pre-activation
    is 0 (there the subgradient is a convention); the hidden outputs given to the statement are the float64 ones, so the gates agree."""
    M, bg = 33, 1.0
    c = K.float_chain(shape, M, "zero_row")
    gen = torch.Generator().manual_seed(5)
    x = c["x"].double().requires_grad_(True)
    ws = [W.double() for W in c["ws"]]
    ws_in = torch.rand(M, generator=gen, dtype=torch.float64).requires_grad_(True)
    h, pre = x, []
    for l, W in enumerate(ws):
        a = h @ W.t()
        if l + 1 < len(ws):
            pre.append(a)
            h = torch.relu(a)
    g_raw = c["grad_out"].double()
    loss = (a * g_raw).sum()
    g_aux = None
    if act == R.ACT_TRUNC_EXP0:
        g_aux = torch.rand(M, generator=gen, dtype=torch.float64) - 0.5
        loss = loss + (torch.exp(a[:, 0]) * g_aux).sum()                     # (|raw| < 15 here: the clamp of the backward is the identity)
    elif act == R.ACT_SIGMOID_BG:
        g_aux = torch.rand(M, shape[-1], generator=gen, dtype=torch.float64) - 0.5
        loss = loss + ((torch.sigmoid(a) + (1 - ws_in)[:, None] * bg) * g_aux).sum()
    pre_grads = torch.autograd.grad(loss, [x, ws_in] + pre, allow_unused=True)
    fwd = R.chain_forward(c["x"], c["ws"])
    ab = R.act_backward(act, fwd["raw"], g_raw, g_aux, bg)
    bwd = R.chain_backward(ab["grad_last"], c["ws"], fwd["hidden"])
    rows = torch.ones(M, dtype=torch.bool)
    for p in pre:
        rows &= (p != 0).all(1)
    assert int(rows.sum()) >= M - 1 and not bool(rows[M // 2])               # (the row of zeros is the excluded one)
    assert torch.allclose(bwd["grad_in"][rows], pre_grads[0][rows], rtol=1e-12, atol=1e-14)
    for l in range(len(pre)):
        assert torch.allclose(bwd["grad_hidden"][l][rows], pre_grads[2 + l][rows], rtol=1e-12, atol=1e-14)
    if act == R.ACT_SIGMOID_BG:
        assert torch.allclose(ab["grad_aux_in"], pre_grads[1], rtol=1e-12, atol=1e-14)
        y, _ = R.act_forward(act, fwd["raw"], fwd["raw_bound"], ws_in.detach(), bg)
        assert torch.allclose(y, (torch.sigmoid(a) + (1 - ws_in)[:, None] * bg).detach(), rtol=1e-13)


def test_float64_products_of_integer_data_are_the_int64_results():
    x, dy = K.int_wgrad(4099, 31, 32)
    assert torch.equal(R.wgrad(x, dy)[0].long(), dy.long().t() @ x.long())
    a, b, bias = K.int_gemm(65, 63, 33)
    assert torch.equal(R.gemm(a, b, bias, 0)[0].long(), a.long() @ b.long() + bias.long())
    c = K.int_chain((31, 32, 3), 65)
    h = c["x"].long()
    for W in c["ws"][:-1]:
        h = torch.relu(h @ W.long().t())
    assert torch.equal(c["fwd"]["raw"].long(), h @ c["ws"][-1].long().t())


# ---- fp32 stays inside every bound ----------------------------------------------------------------------------------------------------
def test_fp32_emulation_is_inside_every_bound():
    worst = dict(fwd=0.0, bwd=0.0, exp_f=0.0, exp_b=0.0, sig_f=0.0, sig_b=0.0, sig_ws=0.0, wgrad=0.0, gemm=0.0)
    for shape in K.SHAPES:
        for kind in K.FLOAT_KINDS:
            c = _float_case(shape, kind)
            for rng in (None, np.random.default_rng(3)):
                hs, raw = emu_forward(c["x"], c["ws"], rng)
                worst["fwd"] = max(worst["fwd"], check_forward(c, hs, raw, f"{shape} {kind}"))
                gh, gi = emu_backward(c["grad_out"], c["ws"], c["hidden_in"], rng)
                worst["bwd"] = max(worst["bwd"], check_backward(c, gh, gi, f"{shape} {kind}"))
            if kind == "spread":                                         # (raw outputs in the hundreds: exp leaves the fp32 range)
                continue
            # the activations on the emulated raw output (forward) and on placed raw values (backward)
            gen = torch.Generator().manual_seed(9)
            acts = ([R.ACT_TRUNC_EXP0] if shape[-1] > 4 else [R.ACT_TRUNC_EXP0, R.ACT_SIGMOID_BG])
            for act in acts:
                C = shape[-1]
                ws_in = torch.rand(M_EMU, generator=gen)
                raw_p = K.placed_raw(M_EMU, C, gen)
                g_aux = K.float_rows(kind, M_EMU, 1 if act == R.ACT_TRUNC_EXP0 else C, gen)
                for bg in (0.0, 1.0):
                    y, yb = R.act_forward(act, c["fwd"]["raw"], c["fwd"]["raw_bound"], ws_in, bg)
                    r = K.assert_bound(emu_act_forward(act, raw, ws_in, bg), y, yb, f"act {act} forward")
                    for g_raw in (c["grad_out"], None):
                        ab = R.act_backward(act, raw_p, g_raw, g_aux, bg)
                        gl, gws = emu_act_backward(act, raw_p, g_raw, g_aux, bg)
                        rb = K.assert_bound(gl, ab["grad_last"], ab["grad_last_bound"], f"act {act} grad_last")
                        ref = R.chain_backward(ab["grad_last"], c["ws"], c["hidden_in"], ab["grad_last_bound"])
                        gh, gi = emu_backward(gl, c["ws"], c["hidden_in"])
                        check_backward(c, gh, gi, f"act {act} chain", ref)
                        if act == R.ACT_TRUNC_EXP0:
                            worst["exp_f"], worst["exp_b"] = max(worst["exp_f"], r), max(worst["exp_b"], rb)
                        else:
                            worst["sig_f"], worst["sig_b"] = max(worst["sig_f"], r), max(worst["sig_b"], rb)
                            worst["sig_ws"] = max(worst["sig_ws"], K.assert_bound(gws, ab["grad_aux_in"], ab["grad_aux_in_bound"], "grad of weights_sum"))
    gen = torch.Generator().manual_seed(4)
    for M, Kw, N in ((1, 10, 16), (129, 31, 32), (4096, 16, 1), (65, 77, 100)):
        for kind in K.FLOAT_KINDS:
            x, dy = K.float_rows(kind, M, Kw, gen), K.float_rows(kind, M, N, gen)
            ref, bound = R.wgrad(x, dy)
            for rng in (None, np.random.default_rng(5)):
                got = torch.from_numpy(fma_rows(dy.numpy().T, x.numpy().T, _order(M, rng)))
                worst["wgrad"] = max(worst["wgrad"], K.assert_bound(got, ref, bound, f"wgrad {M} {Kw} {N} {kind}"))
    for M, N, Kw in ((63, 65, 31), (65, 63, 33), (30, 57, 129)):
        a, b, bias = K.float_rows("spread", M, Kw, gen), K.float_rows("uniform", Kw, N, gen), K.float_rows("uniform", 1, N, gen)[0]
        for act in (0, 1, 2):
            ref, bound = R.gemm(a, b, bias, act)
            v = (torch.from_numpy(fma_rows(a.numpy(), b.numpy().T)) + bias).numpy()
            v = np.maximum(v, F32(0)) if act == 1 else (np.maximum(v, (F32(0.01) * v).astype(F32)) if act == 2 else v)
            worst["gemm"] = max(worst["gemm"], K.assert_bound(torch.from_numpy(v), ref, bound, f"gemm act {act}"))
    print("fp32 emulation, worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- sensitivity: each planted fault fails its assertion ------------------------------------------------------------------------------
def test_bound_assertions_fail_for_the_planted_faults():
    shape = (32, 64, 64, 16)
    c = _float_case(shape, "uniform")
    check_forward(c, *emu_forward(c["x"], c["ws"]), "clean")
    check_backward(c, *emu_backward(c["grad_out"], c["ws"], c["hidden_in"]), "clean")
    with pytest.raises(AssertionError, match="hidden\\[0\\]"):           # (a) a reduced-precision matrix path
        check_forward(c, *emu_forward(c["x"], c["ws"], trunc=True), "10-bit operands")
    with pytest.raises(AssertionError, match="hidden\\[1\\]"):           # (b) two hidden features exchanged
        check_forward(c, *emu_forward(c["x"], c["ws"], swap_layer=1), "swapped features")
    with pytest.raises(AssertionError, match="grad_hidden"):             # (c) the gate of another layer
        check_backward(c, *emu_backward(c["grad_out"], c["ws"], c["hidden_in"], wrong_gate=True), "wrong gate")
    gen = torch.Generator().manual_seed(2)                               # (d) s in place of s (1 - s)
    raw, g_aux, g_raw = K.placed_raw(M_EMU, 3, gen), K.float_rows("uniform", M_EMU, 3, gen), K.float_rows("uniform", M_EMU, 3, gen)
    ab = R.act_backward(R.ACT_SIGMOID_BG, raw, g_raw, g_aux, 1.0)
    K.assert_bound(emu_act_backward(R.ACT_SIGMOID_BG, raw, g_raw, g_aux, 1.0)[0], ab["grad_last"], ab["grad_last_bound"], "clean")
    with pytest.raises(AssertionError, match="dropped"):
        K.assert_bound(emu_act_backward(R.ACT_SIGMOID_BG, raw, g_raw, g_aux, 1.0, drop_one_minus_s=True)[0], ab["grad_last"], ab["grad_last_bound"], "1 - s dropped")


def test_exact_assertions_fail_for_the_planted_faults():
    M = 131072 + 130
    x, dy = K.int_wgrad(M, 32, 3)
    ref = R.wgrad(x, dy)[0]
    K.assert_bits((dy.double().t() @ x.double()).float(), ref, "clean")
    live = int(((dy[:, 0] != 0) & (x[:, 0] != 0)).nonzero()[-1])       # a row whose product is not 0 in element (0, 0)
    with pytest.raises(AssertionError, match="elements differ"):        # (e) one row of M dropped
        keep = torch.arange(M) != live
        K.assert_bits((dy[keep].double().t() @ x[keep].double()).float(), ref, "a row dropped")
    with pytest.raises(AssertionError, match="elements differ"):        # (f) one row counted twice
        twice = torch.cat([torch.arange(M), torch.tensor([live])])
        K.assert_bits((dy[twice].double().t() @ x[twice].double()).float(), ref, "a row twice")
    for shape in K.SHAPES:                                              # (g) k and k + 1 exchanged in one layer's order
        c = K.int_chain(shape, 65)
        hs, raw = emu_forward(c["x"], c["ws"], np.random.default_rng(1))
        for l, h in enumerate(hs):
            K.assert_bits(h, c["fwd"]["hidden"][l], "clean, shuffled k order")
        K.assert_bits(raw, c["fwd"]["raw"], "clean, shuffled k order")
        W1 = c["ws"][1]
        k = int((W1[:, :-1] != W1[:, 1:]).any(0).nonzero()[0])          # two neighbouring columns that differ
        with pytest.raises(AssertionError, match="elements differ"):
            hs, raw = emu_forward(c["x"], c["ws"], kswap=(1, k))
            K.assert_bits((hs + [raw])[1], (c["fwd"]["hidden"] + [c["fwd"]["raw"]])[1], "k order")
        s = K.selection_chain(shape, 65)
        hs, raw = emu_forward(s["x"], s["ws"])
        for l, out in enumerate(hs + [raw]):
            K.assert_selected(out, s["x"], s["src"][l], l, "clean")
        k = min(int(s["ws"][1][0].argmax()), s["ws"][1].shape[1] - 2)     # the column that feature 0 of layer 1 selects
        with pytest.raises(AssertionError, match="layer 1 feature"):
            hs, raw = emu_forward(s["x"], s["ws"], kswap=(1, k))
            K.assert_selected((hs + [raw])[1], s["x"], s["src"][1], 1, "k order")


# ---- the integer cases themselves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_integer_cases_are_exact_and_live(shape):
    for M in K.ROWS:
        c = K.int_chain(shape, M)                                        # (asserts |value| < 2^24 and integrality itself)
        assert c["peak"] < K.EXACT_LIMIT and c["live"] >= 0.25, (shape, M, c["peak"], c["live"])
        for h in c["hidden_in"]:
            assert bool((h == 0).any())
    x, dy = K.int_wgrad(4, 3, 2)
    assert 4 * 4194304 <= K.EXACT_LIMIT and float(x.abs().max()) <= 2 and float(dy.abs().max()) <= 2
    a, b, bias = K.int_gemm(130, 257, 129)
    assert float((a.abs() @ b.abs()).max()) + 5 < K.EXACT_LIMIT
