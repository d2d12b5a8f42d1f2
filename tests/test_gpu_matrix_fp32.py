"""GPU tests of the fp32 matrix-core kernels against the fp64 statement of tests/matrix_ref64.py and the exact integer data of
tests/matrix_cases.py: sn_mlp_small_forward_train / sn_mlp_small_backward (csrc/mlp_small.hip), sn_linear_wgrad with all its routes
(csrc/mlp.hip) and sn_gemm_f32 (csrc/linear.hip).  tests/test_matrix_ref64.py anchors the statement on the CPU, holds an fp32 emulation to
the same bounds and shows that every planted fault (reduced-precision products, swapped features, a wrong gate, a dropped 1 - s, a lost or
doubled row, two exchanged k) fails the assertions used here.

  * through the raw C ABI into NaN-filled buffers with a guard past the end, and once per family through the autograd wrapper;
  * integer data: every output bit-equal to the int64 result, whatever the summation order, slab split or k permutation; selection matrices:
    every output bit-equal to one named input element; float data: every element within its derived bound (`exact and ratio <= 1`);
  * mlp_small: all five SN_SMALL_SHAPES at 1, 63, 64, 65, 129, 131 072 and 131 072 + 65 rows -- from 131 073 rows on a wave of the persistent
    grid (512 workgroups x 4 waves x 64 rows) walks a second tile; the backward with `hidden` supplied by the test (zeros planted), with
    and without grad_in (same bits); both output activations with every gradient arrival, raw values at the clamp's edges, bg 0 and 1;
  * the wrappers: ops.small_mlp_train on integer data, ops.small_linear (sn_gemm_f32 both ways + sn_linear_wgrad) on integer data, and
    ops.small_mlp_train / nerf.network.MLP on row-slice views that start 40 / 124 / 4 / 12 bytes into their allocation (see below).

Which id selects which sn_linear_wgrad instantiation (re-derived from the dispatch at the bottom of csrc/mlp.hip; `route` is in the id):
  small layers, K, N <= 64     rows<10,16> / rows<16,1>    (10,16), (16,1) with x and dy 16-byte aligned, every M (rpw > 128 from 131 073 rows on)
                               valu-partial                every other shape below 16 384 rows, and (10,16), (16,1) with x or dy offset by a float
                               mfma<2,msplit>              from 16 384 rows on (both sides: 16 383 / 16 384 / 16 385); 131 072 + 130 rows: rpw = 130
  wide, K > 64 or N > 64       mfma<2>   (50,100) (64,65)      mfma<4>   (77,100)              mfma<5>   (129,66) (160,71), (160,70) dy+4 bytes
                               mfma<6>   (161,70) (192,65)     mfma<8>   (193,65), (257,33) with two y-blocks
                               mfma<4,vec> (68,66) (128,128)   mfma<8,vec> (132,66) (160,70), (260,66) with two y-blocks
                               mfma<2,flat> (66,30) (65,1), (300,32) with two y-blocks
                               (128,128) dy+4 bytes: mfma<4> by the alignment of dy;  (128,128) dw+4 bytes: sum<16> in place of sum4
  (160,70) with aligned operands is vectorisable (K % 4 == 0, N even) and so takes mfma<8,vec>, not mfma<5>: the K == 160 upper edge of
  mfma<5> is reached by an odd N, (160,71), and by (160,70) with dy offset by one float.
  Every offset pointer here is one the dispatch answers with a scalar-loading instantiation by its own alignment test.

A wrapper defect these tests found: ops._small_mlp_train passed x and grad_out to the library as they came, and the library requires 16-byte
alignment of both for every width; x_wide[1:] of a 10- or 31-wide tensor (40 / 124 bytes in) and an upstream gradient that is such a view of
a 1- or 3-column tensor raised "must be 16-byte aligned".  ops._packed16 now repacks such a view; the library's rejection stays as it was.

Worst |err| / bound per family (a measurement against the fp64 statement, not a threshold; the threshold is always 1).  First column: the fp32
emulation on the CPU (printed by tests/test_matrix_ref64.py), second: the kernels on an MI355X (these tests print every ratio, pytest -s):

  family                                              fp32 emulation        kernel, float data    kernel, integer / selection data
  chain forward, hidden and raw                       0.19                  0.30                  exact
  chain backward, grad_hidden and grad_in             0.28                  0.36                  exact
  trunc_exp forward / grad_last                       0.03 / 0.42           0.02 / 0.47           -
  sigmoid + bg forward / grad_last / to weights_sum   0.05 / 0.44 / 0.00    0.02 / 0.47 / 0.13    -
  wgrad (float data: M <= 4096)                       0.23                  0.25                  exact
  gemm                                                0.09                  -                     exact
The GPU gemm tests use integer data only: the bound of matrix_ref64.gemm is exercised by the CPU emulation alone.
No family came near 1, so no rounding was recounted.  (The emulation's 0.00 for weights_sum: its 48 rows of uniform gradients, multiples of
2^-23, happen to sum without rounding.)  Integer data through the wrapper: `aux` is bit-equal between two calls and within its bound of
the statement -- exp and sigmoid of an integer are not integers.
"""
import ctypes

import numpy as np
import pytest
import torch

import matrix_cases as K
import matrix_ref64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64


def _m():
    from sanerf_hq_amd import _lib as m
    return m


def _l():
    return _m().lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    torch.cuda.synchronize()
    assert rc == 0, _l().sn_last_error().decode()


def _nan(n, dev):
    """A flat NaN-filled buffer of n elements with GUARD more past the end."""
    return torch.full((n + GUARD,), NAN, device=dev)


def _untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all()) and not bool(torch.isnan(buf[:n]).any())


def _take(buf, rows, width, what):
    assert _untouched(buf, rows * width), f"{what}: a write past {rows} x {width} elements, or an element left unwritten"
    return buf[:rows * width].view(rows, width)


def _desc(ws):
    d = _m().MlpDesc()
    d.num_layers, d.activation, d.skip_mask = len(ws), 0, 0
    d.dims[0] = ws[0].shape[1]
    for i, w in enumerate(ws):
        assert w.is_contiguous() and w.dtype == torch.float32
        d.weight[i], d.bias[i], d.dims[i + 1] = w.data_ptr(), None, w.shape[0]
    return d


def _ptrs(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


def hip_forward(x, ws, act=R.ACT_NONE, aux_in=None, bg=0.0):
    """-> (hidden list, raw, activated output or None) through sn_mlp_small_forward_train."""
    M, dev = x.shape[0], x.device
    hb = [_nan(M * w.shape[0], dev) for w in ws[:-1]]
    C = ws[-1].shape[0]
    ob = _nan(M * C, dev)
    aw = 1 if act == R.ACT_TRUNC_EXP0 else C
    ab = _nan(M * aw, dev) if act != R.ACT_NONE else None
    d = _desc(ws)
    _ok(_l().sn_mlp_small_forward_train(ctypes.byref(d), _p(x), M, _ptrs(hb), _p(ob), act, _p(aux_in), float(bg), _p(ab), _s()))
    hidden = [_take(b, M, w.shape[0], f"hidden[{l}]") for l, (b, w) in enumerate(zip(hb, ws[:-1]))]
    return hidden, _take(ob, M, C, "out"), (None if ab is None else _take(ab, M, aw, "aux_out"))


def hip_backward(ws, hidden, grad_out, grad_aux=None, act=R.ACT_NONE, raw=None, bg=0.0, want_in=True, want_aux_in=False):
    """-> dict(grad_in or None, grad_hidden list, grad_last, grad_aux_in or None) through sn_mlp_small_backward."""
    M, dev = hidden[0].shape[0] if hidden else (grad_out if grad_out is not None else grad_aux).shape[0], ws[0].device
    C, d0 = ws[-1].shape[0], ws[0].shape[1]
    gb = [_nan(M * w.shape[0], dev) for w in ws[:-1]]
    lb, ib = _nan(M * C, dev), (_nan(M * d0, dev) if want_in else None)
    wb = _nan(M, dev) if want_aux_in else None
    d = _desc(ws)
    _ok(_l().sn_mlp_small_backward(ctypes.byref(d), _p(grad_out), _p(grad_aux), act, _p(raw), float(bg), _ptrs(hidden), M, _p(ib), _ptrs(gb), _p(lb),
                                   _p(wb), _s()))
    return dict(grad_hidden=[_take(b, M, w.shape[0], f"grad_hidden[{l}]") for l, (b, w) in enumerate(zip(gb, ws[:-1]))],
                grad_last=_take(lb, M, C, "grad_last"), grad_in=(_take(ib, M, d0, "grad_in") if want_in else None),
                grad_aux_in=(_take(wb, M, 1, "grad_aux_in")[:, 0] if want_aux_in else None))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _without_grad_in_same_bits(ws, hidden, full, **kw):
    """The call that does not want grad_in skips the last chain layer at run time: grad_hidden and grad_last must not change by a bit."""
    part = hip_backward(ws, hidden, want_in=False, **kw)
    assert part["grad_in"] is None
    assert _same_bits(part["grad_last"], full["grad_last"]), "grad_in == NULL changes grad_last"
    for l, (a, b) in enumerate(zip(part["grad_hidden"], full["grad_hidden"])):
        assert _same_bits(a, b), f"grad_in == NULL changes grad_hidden[{l}]"
    return part


def _dev(c, gpu, keys=("x", "grad_out")):
    return {**c, **{k: c[k].to(gpu) for k in keys}, "ws": [w.to(gpu) for w in c["ws"]], "hidden_in": [h.to(gpu) for h in c.get("hidden_in", [])]}


SHAPE_ROWS = [pytest.param(s, M, id=f"{K.shape_id(s)}-M{M}" + ("-second-pass" if M > K.SECOND_PASS else "")) for s in K.SHAPES for M in K.ROWS]


# ---- mlp_small: exact data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M", SHAPE_ROWS)
def test_small_chain_integer_data_is_exact(gpu, shape, M):
    c = _dev(K.int_chain(shape, M), gpu)
    hidden, raw, _ = hip_forward(c["x"], c["ws"])
    for l, h in enumerate(hidden):
        K.assert_bits(h, c["fwd"]["hidden"][l].to(gpu), f"forward hidden[{l}]")
    K.assert_bits(raw, c["fwd"]["raw"].to(gpu), "forward out")
    full = hip_backward(c["ws"], c["hidden_in"], c["grad_out"])
    K.assert_bits(full["grad_last"], c["grad_out"].double(), "grad_last")
    for l, g in enumerate(full["grad_hidden"]):
        K.assert_bits(g, c["bwd"]["grad_hidden"][l].to(gpu), f"grad_hidden[{l}]")
    K.assert_bits(full["grad_in"], c["bwd"]["grad_in"].to(gpu), "grad_in")
    _without_grad_in_same_bits(c["ws"], c["hidden_in"], full, grad_out=c["grad_out"])


@pytest.mark.parametrize("shape,M", SHAPE_ROWS)
def test_small_chain_selection_matrices_name_every_feature(gpu, shape, M):
    c = _dev(K.selection_chain(shape, M), gpu)
    hidden, raw, _ = hip_forward(c["x"], c["ws"])
    for l, out in enumerate(hidden + [raw]):
        K.assert_selected(out, c["x"], c["src"][l], l, "forward")
    ref = R.chain_backward(c["grad_out"], c["ws"], c["hidden_in"])                       # sums of at most a few exact values: exact
    full = hip_backward(c["ws"], c["hidden_in"], c["grad_out"])
    for l, g in enumerate(full["grad_hidden"]):
        K.assert_bits(g, ref["grad_hidden"][l], f"backward, gradient of layer {l}'s pre-activation")
    K.assert_bits(full["grad_in"], ref["grad_in"], "backward, grad_in")
    _without_grad_in_same_bits(c["ws"], c["hidden_in"], full, grad_out=c["grad_out"])


# ---- mlp_small: float data within the bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.FLOAT_KINDS)
@pytest.mark.parametrize("shape,M", SHAPE_ROWS)
def test_small_chain_float_data_within_bounds(gpu, shape, M, kind):
    c = _dev(K.float_chain(shape, M, kind), gpu)
    fwd = R.chain_forward(c["x"], c["ws"])
    hidden, raw, _ = hip_forward(c["x"], c["ws"])
    rf = K.assert_bound(raw, fwd["raw"], fwd["raw_bound"], "forward out")
    for l, h in enumerate(hidden):
        rf = max(rf, K.assert_bound(h, fwd["hidden"][l], fwd["hidden_bound"][l], f"forward hidden[{l}]"))
    hidden_in = [K.plant_zeros(h.float()) for h in fwd["hidden"]]
    ref = R.chain_backward(c["grad_out"], c["ws"], hidden_in)
    full = hip_backward(c["ws"], hidden_in, c["grad_out"])
    assert _same_bits(full["grad_last"], c["grad_out"]), "grad_last is not grad_out's bits"
    rb = K.assert_bound(full["grad_in"], ref["grad_in"], ref["grad_in_bound"], "grad_in")
    for l, g in enumerate(full["grad_hidden"]):
        rb = max(rb, K.assert_bound(g, ref["grad_hidden"][l], ref["grad_hidden_bound"][l], f"grad_hidden[{l}]"))
    _without_grad_in_same_bits(c["ws"], hidden_in, full, grad_out=c["grad_out"])
    print(f"chain {K.shape_id(shape)} M={M} {kind}: forward {rf:.3f} backward {rb:.3f}")


# ---- mlp_small: the output activations ------------------------------------------------------------------------------------------------
ACT_CASES = [(R.ACT_TRUNC_EXP0, (10, 16, 1)), (R.ACT_TRUNC_EXP0, (32, 64, 64, 16)), (R.ACT_SIGMOID_BG, (31, 32, 32, 3)), (R.ACT_SIGMOID_BG, (31, 32, 3))]


@pytest.mark.parametrize("M", [1, 65, 4097])
@pytest.mark.parametrize("act,shape", ACT_CASES, ids=[("trunc_exp-" if a == 1 else "sigmoid_bg-") + K.shape_id(s) for a, s in ACT_CASES])
def test_small_output_activations_match_fp64(gpu, act, shape, M):
    """Forward: the activated output from the kernel's own raw output.  Backward: raw values given by the test with the clamp's edges placed
    (+-15, +-15.5, 0); the gradient arriving through the raw output only, through the activated output only (grad_out == NULL) and through both;
    grad_aux_in wanted and NULL (same bits elsewhere); bg 0 and 1; each with and without grad_in."""
    c = _dev(K.float_chain(shape, M, "uniform"), gpu)
    gen = torch.Generator().manual_seed(M + act)
    C = shape[-1]
    ws_in = torch.rand(M, generator=gen).to(gpu)
    raw_p = K.placed_raw(M, C, gen).to(gpu)
    g_aux = K.float_rows("uniform", M, 1 if act == R.ACT_TRUNC_EXP0 else C, gen).to(gpu)
    fwd = R.chain_forward(c["x"], c["ws"])
    hidden_in = [K.plant_zeros(h.float()) for h in fwd["hidden"]]
    rf = rl = rc = rw = 0.0
    for bg in ((0.0,) if act == R.ACT_TRUNC_EXP0 else (0.0, 1.0)):
        hidden, raw, aux = hip_forward(c["x"], c["ws"], act, ws_in if act == R.ACT_SIGMOID_BG else None, bg)
        K.assert_bound(raw, fwd["raw"], fwd["raw_bound"], "forward out")
        y, yb = R.act_forward(act, fwd["raw"], fwd["raw_bound"], ws_in, bg)
        rf = max(rf, K.assert_bound(aux.view(y.shape), y, yb, f"activated output, bg {bg}"))
        for arrival, (g_raw, ga) in dict(raw_only=(c["grad_out"], None), aux_only=(None, g_aux), both=(c["grad_out"], g_aux)).items():
            ab = R.act_backward(act, raw_p, g_raw, ga, bg)
            ref = R.chain_backward(ab["grad_last"], c["ws"], hidden_in, ab["grad_last_bound"])
            kw = dict(grad_out=g_raw, grad_aux=ga, act=act, raw=raw_p, bg=bg)
            wants = (False, True) if (act == R.ACT_SIGMOID_BG and ga is not None) else (False,)
            first = None
            for want_aux_in in wants:
                full = hip_backward(c["ws"], hidden_in, want_aux_in=want_aux_in, **kw)
                what = f"{arrival}, bg {bg}, grad_aux_in {'wanted' if want_aux_in else 'NULL'}"
                rl = max(rl, K.assert_bound(full["grad_last"], ab["grad_last"], ab["grad_last_bound"], f"grad_last ({what})"))
                rc = max(rc, K.assert_bound(full["grad_in"], ref["grad_in"], ref["grad_in_bound"], f"grad_in ({what})"))
                for l, g in enumerate(full["grad_hidden"]):
                    rc = max(rc, K.assert_bound(g, ref["grad_hidden"][l], ref["grad_hidden_bound"][l], f"grad_hidden[{l}] ({what})"))
                if want_aux_in:
                    rw = max(rw, K.assert_bound(full["grad_aux_in"], ab["grad_aux_in"], ab["grad_aux_in_bound"], f"grad_aux_in ({what})"))
                _without_grad_in_same_bits(c["ws"], hidden_in, full, want_aux_in=want_aux_in, **kw)
                if first is not None:
                    assert _same_bits(first["grad_last"], full["grad_last"]) and _same_bits(first["grad_in"], full["grad_in"]), "grad_aux_in == NULL changes other outputs"
                first = full
    print(f"act {act} {K.shape_id(shape)} M={M}: activated output {rf:.3f}, grad_last {rl:.3f}, chain behind it {rc:.3f}, to weights_sum {rw:.3f}")


# ---- mlp_small: the autograd wrapper --------------------------------------------------------------------------------------------------
def _layers(ws):
    layers = [torch.nn.Linear(w.shape[1], w.shape[0], bias=False).to(w.device) for w in ws]
    for l, w in zip(layers, ws):
        l.weight.data = w.clone()
    return layers


def _wrapper_run(x, layers, act, aux_in, bg, g_out, g_aux):
    from sanerf_hq_amd import ops
    for l in layers:
        l.weight.grad = None
    xt = x.detach().requires_grad_(True)                    # (detach() of a view keeps its storage offset)
    out, aux = ops.small_mlp_train(xt, layers, act, aux_in, bg)
    outs, grads = ([out], [g_out]) if g_aux is None else ([out, aux], [g_out, g_aux])
    torch.autograd.backward(outs, grads)
    return [out.detach(), None if aux is None else aux.detach(), xt.grad] + [l.weight.grad.clone() for l in layers]


WRAP_ACT = {(10, 16, 1): R.ACT_TRUNC_EXP0, (32, 64, 64, 16): R.ACT_TRUNC_EXP0, (31, 32, 32, 3): R.ACT_SIGMOID_BG, (16, 32, 16): R.ACT_NONE, (31, 32, 3): R.ACT_SIGMOID_BG}


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_small_mlp_train_wrapper_integer_data(gpu, shape):
    """ops.small_mlp_train on integer data, the gradient arriving through the raw output: out and x.grad bit-equal to the int64 results, the
    activated output within its bound, every weight gradient within the wgrad bound of the exact integer operands (the kernel's own hidden
    outputs and pre-activation gradients ARE those operands, by the equalities above); two calls give the same bits."""
    from sanerf_hq_amd import ops
    M, act, bg = 4097, WRAP_ACT[shape], 1.0
    c = K.int_chain(shape, M)
    d = _dev(c, gpu)
    layers = _layers(d["ws"])
    assert ops.small_mlp_fusable(d["x"].requires_grad_(True), layers)
    aux_in = torch.rand(M, generator=torch.Generator().manual_seed(1)).to(gpu) if act == R.ACT_SIGMOID_BG else None
    a = _wrapper_run(d["x"], layers, act, aux_in, bg, d["grad_out"], None)
    b = _wrapper_run(d["x"], layers, act, aux_in, bg, d["grad_out"], None)
    for u, v in zip(a, b):
        assert (u is None and v is None) or _same_bits(u, v), "two calls differ"
    K.assert_bits(a[0], c["fwd"]["raw"].to(gpu), "out")
    if act != R.ACT_NONE:
        raw = c["fwd"]["raw"].to(gpu)
        ok = (raw[:, 0].abs() <= 80.0) if act == R.ACT_TRUNC_EXP0 else torch.ones(M, dtype=torch.bool, device=gpu)    # (exp of a larger integer leaves fp32)
        y, yb = R.act_forward(act, raw[ok], torch.zeros_like(raw[ok]), None if aux_in is None else aux_in[ok], bg)
        K.assert_bound(a[1][ok].view(y.shape), y, yb, "activated output")
    # the wrapper's backward gates on the forward's own hidden outputs: no zeros planted here
    ref = R.chain_backward(c["grad_out"], c["ws"], c["fwd"]["hidden"])
    K.assert_bits(a[2], ref["grad_in"].to(gpu), "x.grad")
    ins, gys = [c["x"]] + c["fwd"]["hidden"], ref["grad_hidden"] + [c["grad_out"]]
    for l in range(len(shape) - 1):
        dw, bound = R.wgrad(ins[l], gys[l])
        K.assert_bound(a[3 + l], dw.to(gpu), bound.to(gpu), f"weight gradient of layer {l}")


@pytest.mark.parametrize("shape", [(10, 16, 1), (31, 32, 3)], ids=K.shape_id)
def test_small_mlp_train_wrapper_takes_views_that_are_not_16_byte_aligned(gpu, shape):
    """x_wide[1:] of a 10- / 31-wide tensor starts 40 / 124 bytes into its allocation, an upstream gradient that is such a view of a 1- / 3-column
    tensor 4 / 12 bytes: each must compute, and give the same bits as a packed clone."""
    M = 321
    act = WRAP_ACT[shape]
    d = _dev(K.float_chain(shape, M + 1, "uniform"), gpu)
    layers = _layers(d["ws"])
    aux_in = torch.rand(M, generator=torch.Generator().manual_seed(2)).to(gpu) if act == R.ACT_SIGMOID_BG else None
    gen = torch.Generator().manual_seed(3)
    ga_wide = K.float_rows("uniform", M + 1, 1 if act == R.ACT_TRUNC_EXP0 else shape[-1], gen).to(gpu)
    xv, gv = d["x"][1:], d["grad_out"][1:]
    gav = ga_wide[1:, 0] if act == R.ACT_TRUNC_EXP0 else ga_wide[1:]
    assert xv.is_contiguous() and xv.data_ptr() % 16 != 0 and gv.data_ptr() % 16 != 0
    packed = _wrapper_run(xv.clone(), layers, act, aux_in, 1.0, gv.clone(), gav.clone())
    for what, args in dict(x=(xv, gv.clone(), gav.clone()), grad_out=(xv.clone(), gv, gav.clone()), all=(xv, gv, gav)).items():
        got = _wrapper_run(args[0], layers, act, aux_in, 1.0, args[1], args[2])
        for i, (u, v) in enumerate(zip(got, packed)):
            assert _same_bits(u, v), f"a view as {what}: result {i} differs from the packed clone's"
    # nerf.network.MLP, the module the training code calls, on the same view
    from sanerf_hq_amd.nerf.network import MLP
    mlp = MLP(shape[0], shape[-1], shape[1], len(shape) - 1, bias=False).to(gpu)
    for l, w in zip(mlp.net, d["ws"]):
        l.weight.data = w.clone()
    assert _same_bits(mlp(xv.detach().requires_grad_(True)).detach(), packed[0]), "MLP on the view differs from the packed clone's output"
    # and the library itself still rejects the pointer (the wrapper repacks, the check stays)
    hb = [_nan(M * w.shape[0], gpu) for w in d["ws"][:-1]]
    ob = _nan(M * shape[-1], gpu)
    desc = _desc(d["ws"])
    rc = _l().sn_mlp_small_forward_train(ctypes.byref(desc), _p(xv), M, _ptrs(hb), _p(ob), 0, None, 0.0, None, _s())
    torch.cuda.synchronize()
    assert rc == -1 and b"16-byte aligned" in _l().sn_last_error() and bool(torch.isnan(ob).all())


def test_small_linear_wrapper_integer_data(gpu):
    """ops.small_linear under autograd on a 40 -> 70 layer with a bias, integer data: the forward and the input gradient (sn_gemm_f32) and the
    weight gradient (sn_linear_wgrad, mfma<4,vec>) bit-equal to the integer results; two calls give the same bits."""
    from sanerf_hq_amd import ops
    M, N, Kw = 321, 70, 40
    a, b, bias = K.int_gemm(M, N, Kw)
    gy = K.int_wgrad(M, Kw, N)[1].to(gpu)
    lin = torch.nn.Linear(Kw, N, bias=True).to(gpu)
    lin.weight.data, lin.bias.data = b.t().contiguous().to(gpu), bias.to(gpu)
    runs = []
    for _ in range(2):
        lin.zero_grad()
        x = a.to(gpu).requires_grad_(True)
        y = ops.small_linear(x, lin)
        y.backward(gy)
        runs.append([y.detach(), x.grad, lin.weight.grad.clone(), lin.bias.grad.clone()])
    for u, v in zip(*runs):
        assert _same_bits(u, v), "two calls differ"
    y, gx, gw, gb = runs[0]
    K.assert_bits(y, (a.double() @ b.double() + bias.double()).to(gpu), "layer output")
    K.assert_bits(gx, gy.double() @ b.double().t().to(gpu), "input gradient")
    K.assert_bits(gw, R.wgrad(a.to(gpu), gy)[0], "weight gradient")
    K.assert_bits(gb, gy.double().sum(0), "bias gradient")


# ---- sn_linear_wgrad ------------------------------------------------------------------------------------------------------------------
def _offset(t):
    """The same values one float into a fresh allocation."""
    return torch.empty(t.numel() + 1, device=t.device)[1:].view(t.shape).copy_(t)


def hip_wgrad(x, dy, offset_dw=False):
    M, Kw, N = x.shape[0], x.shape[1], dy.shape[1]
    need = int(_l().sn_linear_wgrad_workspace_bytes(M, Kw, N))
    assert need > 0 and need % 4 == 0
    ws = _nan(need // 4, x.device)                                                       # a workspace of exactly the bytes asked for, a guard behind it
    buf = _nan(N * Kw + 1, x.device)
    dw = buf[1:] if offset_dw else buf
    assert dw.data_ptr() % 16 == (4 if offset_dw else 0)
    _ok(_l().sn_linear_wgrad(_p(x), _p(dy), M, Kw, N, _p(dw), _p(ws), need, _s()))
    assert bool(torch.isnan(ws[need // 4:]).all()), "a write past the workspace size the library asked for"
    assert bool(torch.isnan(buf[:1]).all()) or not offset_dw
    assert _untouched(dw, N * Kw), "dw: a write past N x K elements, or an element left unwritten"
    return dw[:N * Kw].view(N, Kw)


def _wgrad_case(gpu, M, Kw, N, off=None):
    x, dy = (t.to(gpu) for t in K.int_wgrad(M, Kw, N))
    ref = R.wgrad(x, dy)[0]
    assert float(ref.abs().max()) < K.EXACT_LIMIT
    xs, ds = (_offset(x) if off == "x" else x), (_offset(dy) if off == "dy" else dy)
    got = hip_wgrad(xs, ds, offset_dw=off == "dw")
    K.assert_bits(got, ref, f"dw of {M} rows, {Kw} -> {N}" + (f", {off} offset by one float" if off else ""))
    assert _same_bits(got, hip_wgrad(xs, ds, offset_dw=off == "dw")), "two calls differ"
    if M <= 4096:
        gen = torch.Generator().manual_seed(M + Kw + N)
        ratio = 0.0
        for kind in K.FLOAT_KINDS:
            xf, df = K.float_rows(kind, M, Kw, gen).to(gpu), K.float_rows(kind, M, N, gen).to(gpu)
            want, bound = R.wgrad(xf, df)
            xs, ds = (_offset(xf) if off == "x" else xf), (_offset(df) if off == "dy" else df)
            ratio = max(ratio, K.assert_bound(hip_wgrad(xs, ds, offset_dw=off == "dw"), want, bound, f"dw of {M} rows, {Kw} -> {N}, {kind}"))
        print(f"wgrad M={M} {Kw}->{N}{' ' + off + '+4' if off else ''}: {ratio:.3f}")


def _small_route(Kw, N, M, off=None):
    if (Kw, N) in ((10, 16), (16, 1)) and off is None:
        return f"rows<{Kw},{N}>"
    return "mfma<2,msplit>" if M >= 16384 else "valu-partial"


WG_SMALL_M = [1, 127, 128, 129, 16383, 16384, 16385, 131072 + 130]
WG_SMALL = [pytest.param(M, Kw, N, None, id=f"{Kw}x{N}-M{M}-{_small_route(Kw, N, M)}")
            for (Kw, N) in ((32, 64), (64, 64), (64, 16), (31, 32), (32, 3), (16, 32), (10, 16), (16, 1)) for M in WG_SMALL_M]
WG_SMALL += [pytest.param(M, Kw, N, off, id=f"{Kw}x{N}-M{M}-{off}+4-{_small_route(Kw, N, M, off)}")
             for (Kw, N) in ((10, 16), (16, 1)) for off in ("x", "dy") for M in WG_SMALL_M]


@pytest.mark.parametrize("M,Kw,N,off", WG_SMALL)
def test_linear_wgrad_small_layers_exact(gpu, M, Kw, N, off):
    _wgrad_case(gpu, M, Kw, N, off)


WG_WIDE_SHAPES = [(50, 100, "mfma<2>"), (64, 65, "mfma<2>"), (77, 100, "mfma<4>"), (129, 66, "mfma<5>"), (160, 71, "mfma<5>"), (160, 70, "mfma<8,vec>"), (161, 70, "mfma<6>"),
                  (192, 65, "mfma<6>"), (193, 65, "mfma<8>"), (257, 33, "mfma<8>-2y"), (68, 66, "mfma<4,vec>"), (128, 128, "mfma<4,vec>"),
                  (132, 66, "mfma<8,vec>"), (260, 66, "mfma<8,vec>-2y"), (66, 30, "mfma<2,flat>"), (300, 32, "mfma<2,flat>-2y"), (65, 1, "mfma<2,flat>")]
WG_WIDE_M = [1, 65, 129, 16385]
WG_WIDE = [pytest.param(M, Kw, N, None, id=f"{Kw}x{N}-M{M}-{route}") for (Kw, N, route) in WG_WIDE_SHAPES for M in WG_WIDE_M]
WG_WIDE += [pytest.param(M, 128, 128, "dy", id=f"128x128-M{M}-dy+4-mfma<4>") for M in WG_WIDE_M]
WG_WIDE += [pytest.param(M, 160, 70, "dy", id=f"160x70-M{M}-dy+4-mfma<5>") for M in WG_WIDE_M]
WG_WIDE += [pytest.param(M, 128, 128, "dw", id=f"128x128-M{M}-dw+4-mfma<4,vec>-sum<16>") for M in WG_WIDE_M]


@pytest.mark.parametrize("M,Kw,N,off", WG_WIDE)
def test_linear_wgrad_wide_branch_exact(gpu, M, Kw, N, off):
    _wgrad_case(gpu, M, Kw, N, off)


# ---- sn_gemm_f32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kw", [(1, 1, 1), (63, 65, 31), (64, 64, 32), (65, 63, 33), (130, 257, 129)])
def test_gemm_f32_integer_data_is_exact(gpu, M, N, Kw):
    """All four operand layouts, bias on and off, the three activations: the whole output bit-equal to the integer result (leaky ReLU: to the
    one fp32 product 0.01f * v of a negative v)."""
    a, b, bias = K.int_gemm(M, N, Kw)
    v = (a.double() @ b.double())
    bias_dev = bias.to(gpu)
    for use_bias in (False, True):
        vb = ((v + bias.double()) if use_bias else v).float().numpy() + np.float32(0)     # (+0.0 for zero)
        assert float(np.abs(vb).max()) < K.EXACT_LIMIT
        for act in (0, 1, 2):
            want = vb if act == 0 else (np.maximum(vb, np.float32(0)) if act == 1 else np.maximum(vb, (np.float32(0.01) * vb).astype(np.float32)))
            want = torch.from_numpy(np.ascontiguousarray(want)).to(gpu)
            for ta in (False, True):
                for tb in (False, True):
                    at = (a.t().contiguous() if ta else a).to(gpu)                       # stored [K, M] when transposed
                    bt = (b.t().contiguous() if tb else b).to(gpu)                       # stored [N, K] when transposed
                    buf = _nan(M * N, gpu)
                    _ok(_l().sn_gemm_f32(_p(at), 1 if ta else Kw, M if ta else 1, _p(bt), 1 if tb else N, Kw if tb else 1,
                                         _p(bias_dev) if use_bias else None, act, M, N, Kw, _p(buf), N, _s()))
                    got = _take(buf, M, N, "c")
                    assert _same_bits(got, want), f"layouts a^T={ta} b^T={tb}, bias {use_bias}, act {act}: {int((got != want).sum())} of {M * N} elements differ"
