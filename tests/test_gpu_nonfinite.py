"""NaN and +-inf planted in values (inputs, weights, biases, gradients) against torch's expressions in fp64 ("Non-finite
values"): every route must give torch's NaN pattern and torch's infinities, sign included, keep its usual tolerance on the finite entries,
and leave the rows that hold no planted value bit-identical to a clean run.  Non-finite values never go into anything that becomes an
index (ray geometry, grid coordinates, near / far)."""
import numpy as np
import pytest
import torch

from helpers import camera_rays, oracle_cfg, product_model, synthetic_params

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def assert_nonfinite_like(got, ref, tol, what=""):
    """Same NaN mask, same infinities (sign included), finite entries within tol * max(1, max |ref|) of the reference."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, what
    assert torch.equal(got.isnan(), ref.isnan()), f"{what}: NaN masks differ at {int((got.isnan() != ref.isnan()).sum())} entries"
    inf = ref.isinf()
    assert torch.equal(got.isinf(), inf) and torch.equal(got[inf], ref[inf]), f"{what}: infinities differ"
    fin = torch.isfinite(ref)
    if fin.any():
        err = float((got[fin] - ref[fin]).abs().max())
        assert err <= tol * max(1.0, float(ref[fin].abs().max())), f"{what}: finite entries off by {err}"


def plant_rows(x, cols=(0, 1, 2)):
    """NaN, +inf, -inf in three rows of a copy of x (rows 3, 10, 20 or the last rows of a short batch); returns (copy, planted row indices)."""
    x = x.clone()
    n = x.shape[0]
    rows = [r % n for r in (3, 10, 20)]
    for r, c, v in zip(rows, cols, (NAN, INF, -INF)):
        x[r, c % x.shape[1]] = v
    return x, sorted(set(rows))


def others(n, rows):
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(rows)] = False
    return keep


# ---------------------------------------------------------------------------------------------------------------------------- sn_gemm_f32

@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_f32_nonfinite_inputs_weights_and_bias(gpu, act):
    """sn_gemm_f32 through ops.linear_forward: a NaN / +inf / -inf in three input rows, one NaN weight (a whole output column goes NaN), a
    +inf and a -inf bias; ReLU must keep NaN and map -inf to 0, leaky ReLU must keep -inf.  ops._gemm with the input column-major gives the
    same result bit for bit (NaN where NaN)."""
    from sanerf_hq_amd import ops
    M, N, K = 300, 70, 45
    rng = np.random.default_rng(71 + act)
    x = T(rng.standard_normal((M, K)).astype(np.float32), gpu)
    w = T((rng.standard_normal((N, K)) / K ** 0.5).astype(np.float32), gpu)
    b = T(rng.standard_normal(N).astype(np.float32), gpu)
    w[9, 11] = NAN
    b[4], b[6] = INF, -INF
    clean = ops.linear_forward(x, w, b, act)
    xp, rows = plant_rows(x, (5, 7, 2))
    y = ops.linear_forward(xp, w, b, act)
    ref = xp.double() @ w.double().t() + b.double()
    ref = torch.relu(ref) if act == 1 else (torch.nn.functional.leaky_relu(ref, 0.01) if act == 2 else ref)
    assert_nonfinite_like(y, ref, 2e-6, f"act {act}")
    keep = others(M, rows)
    assert bool(y[:, 9].isnan().all())
    if act == 1:
        assert bool((y[keep, 6] == 0).all()), "relu(-inf) = 0"
    elif act == 2:
        assert bool((y[keep, 6] == -INF).all())
    assert torch.equal(y[keep].nan_to_num(), clean[keep].nan_to_num()) and torch.equal(y[keep].isnan(), clean[keep].isnan())
    out = torch.empty(M, N, device=gpu)
    xt = xp.t().contiguous()
    ops._gemm(xt, 1, M, w, 1, K, b, act, M, N, K, out)
    assert torch.equal(out.isnan(), y.isnan()) and torch.equal(out.nan_to_num(), y.nan_to_num())


@pytest.mark.parametrize("act", [1, 2])
def test_small_linear_same_nan_mask_with_and_without_autograd(gpu, act):
    """ops.small_linear runs the activation in the product's epilogue without autograd and in torch under it: both routes must return
    torch's NaN pattern for the same layer and input."""
    from sanerf_hq_amd import ops
    torch.manual_seed(5)
    layer = torch.nn.Linear(40, 128).to(gpu)
    x = torch.randn(500, 40, device=gpu)
    with torch.no_grad():
        layer.weight[17, 3] = NAN
    xp, _ = plant_rows(x)
    with torch.no_grad():
        y0 = ops.small_linear(xp, layer, act)
    y1 = ops.small_linear(xp, layer, act)
    assert y1.requires_grad
    ref = torch.nn.functional.linear(xp.double(), layer.weight.double(), layer.bias.double())
    ref = torch.relu(ref) if act == ops.ACT_RELU else torch.nn.functional.leaky_relu(ref, 0.01)
    assert_nonfinite_like(y0, ref, 2e-6, "no grad")
    assert_nonfinite_like(y1, ref, 2e-6, "autograd")
    assert torch.equal(y0.isnan(), y1.detach().isnan())


# ---------------------------------------------------------------------------------------------------------------------------- small MLPs

SHAPES = [(10, 16, 1), (32, 64, 64, 16), (31, 32, 32, 3), (16, 32, 16), (31, 32, 3)]


def _small_layers(dims, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    layers = [torch.nn.Linear(a, b, bias=False) for a, b in zip(dims[:-1], dims[1:])]
    for l in layers:
        l.weight.data = (torch.rand(l.weight.shape, generator=g) * 2 - 1) * (1.5 / np.sqrt(l.weight.shape[1]))
    return [l.to(dev) for l in layers]


def _torch_mlp(x, ws):
    h = x
    for w in ws[:-1]:
        h = torch.relu(torch.nn.functional.linear(h, w))
    return torch.nn.functional.linear(h, ws[-1])


@pytest.mark.parametrize("dims", SHAPES)
def test_small_mlp_nonfinite_rows_forward(gpu, dims):
    """sn_mlp_small_forward_train on every instantiated shape with NaN, +inf and -inf in three input rows against torch in fp64: ReLU keeps
    NaN and maps -inf to 0.  The other rows' outputs are bit-identical to a clean run."""
    from sanerf_hq_amd import ops
    rows = 1000
    layers = _small_layers(dims, gpu, 40 + len(dims))
    g = torch.Generator(device=gpu).manual_seed(3)
    x0 = torch.rand(rows, dims[0], device=gpu, generator=g) * 2 - 1

    def run(xin):
        xs = xin.clone().requires_grad_(True)
        assert ops.small_mlp_fusable(xs, layers)
        return ops.small_mlp_train(xs, layers)[0].detach()

    clean = run(x0)
    xp, planted = plant_rows(x0)
    out = run(xp)
    ref = _torch_mlp(xp.double(), [l.weight.detach().double() for l in layers])
    assert_nonfinite_like(out, ref, 2e-6, "forward")
    keep = others(rows, planted)
    assert torch.equal(out[keep], clean[keep])


@pytest.mark.xfail(strict=True, reason="known divergence (DESIGN.md 4.1): the fused small-MLP backward's input gradient of a row with a "
                                       "non-finite input differs from torch autograd; open")
@pytest.mark.parametrize("dims", [(10, 16, 1), (32, 64, 64, 16)])
def test_small_mlp_backward_input_gradient_of_nonfinite_rows(gpu, dims):
    """sn_mlp_small_backward with NaN / +inf / -inf in three input rows: the input gradient against torch autograd in fp64 (threshold_backward:
    a NaN or zero activation passes no gradient)."""
    from sanerf_hq_amd import ops
    rows = 1000
    layers = _small_layers(dims, gpu, 40 + len(dims))
    g = torch.Generator(device=gpu).manual_seed(3)
    x0 = torch.rand(rows, dims[0], device=gpu, generator=g) * 2 - 1
    gy = torch.randn(rows, dims[-1], device=gpu, generator=g)
    xp, _ = plant_rows(x0)
    xs = xp.clone().requires_grad_(True)
    ops.small_mlp_train(xs, layers)[0].backward(gy)
    x64 = xp.double().requires_grad_(True)
    _torch_mlp(x64, [l.weight.detach().double() for l in layers]).backward(gy.double())
    assert_nonfinite_like(xs.grad, x64.grad, 2e-5, "input gradient")


def test_small_mlp_nan_weight_reaches_the_loss(gpu):
    """A NaN in one hidden weight of a small MLP: ReLU keeps it, so every output is NaN as in torch (the unit is not silently zeroed, so the
    loss cannot stay finite while the weight is NaN)."""
    from sanerf_hq_amd import ops
    layers = _small_layers((32, 64, 64, 16), gpu, 9)
    with torch.no_grad():
        layers[1].weight[5, 7] = NAN
    x = (torch.rand(777, 32, device=gpu) * 2 - 1).requires_grad_(True)
    out, _ = ops.small_mlp_train(x, layers)
    ref = _torch_mlp(x.detach().double(), [l.weight.detach().double() for l in layers])
    assert_nonfinite_like(out, ref, 2e-6, "forward")
    assert bool(out.isnan().all())


def test_small_mlp_trunc_exp_and_sigmoid_outputs_keep_nan(gpu):
    """The trunc_exp density output and the sigmoid + background image output of a row whose input holds a NaN are NaN (torch), the other rows
    are finite and as in torch."""
    from sanerf_hq_amd import ops
    from sanerf_hq_amd.activation import trunc_exp
    layers = _small_layers((32, 64, 64, 16), gpu, 3)
    x = torch.rand(3000, 32, device=gpu) * 4 - 2
    x[100, 4] = NAN
    xs = x.clone().requires_grad_(True)
    raw, sig = ops.small_mlp_train(xs, layers, ops.SMALL_ACT_TRUNC_EXP0)
    raw64 = _torch_mlp(x.double(), [l.weight.detach().double() for l in layers])
    assert_nonfinite_like(raw, raw64, 2e-6, "raw")
    assert_nonfinite_like(sig, trunc_exp(raw64[:, 0]), 5e-6, "sigma")
    assert bool(sig[100].isnan()) and int(sig.isnan().sum()) == 1
    vl = _small_layers((31, 32, 32, 3), gpu, 5)
    xv = torch.rand(4096, 31, device=gpu) * 2 - 1
    xv[7, 0] = NAN
    ws = torch.rand(4096, device=gpu)
    _, img = ops.small_mlp_train(xv, vl, ops.SMALL_ACT_SIGMOID_BG, ws, 1.0)
    img64 = torch.sigmoid(_torch_mlp(xv.double(), [l.weight.detach().double() for l in vl])) + (1 - ws.double()).unsqueeze(-1)
    assert_nonfinite_like(img, img64, 2e-6, "image")
    assert bool(img[7].isnan().all()) and int(img.isnan().sum()) == 3


# ---------------------------------------------------------------------------------------------------------------------------- wide MLP

@pytest.mark.parametrize("n_out", [4, 256])
def test_wide_mlp_relu_of_minus_inf_is_zero(gpu, n_out):
    """The inference wide MLP (sn_mlp_wide_forward, split-fp16 products) of a ReLU perceptron whose hidden biases hold -inf: relu(-inf) = 0,
    so every output is finite and as torch's, and the range flag stays down (it looks only at the last layer's outputs, not at the hidden
    pre-activations left in the other accumulator tiles).  max(t, t * 0) made the unit NaN here.  A narrow (4) and a full-width last layer."""
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf.network import MLP
    mlp = MLP(143, n_out, 256, 3, bias=True).to(gpu)
    with torch.no_grad():
        for i, lin in enumerate(mlp.net):
            lin.weight.copy_(T(synth.linear_weight(lin.weight.shape[0], lin.weight.shape[1], 500 + i, 2.0), gpu))
            lin.bias.copy_(T(synth.hash_uniform((lin.bias.shape[0],), 600 + i, -0.1, 0.1), gpu))
        mlp.net[0].bias[13] = -INF
        mlp.net[1].bias[200] = -INF
    x = T(np.random.default_rng(8).standard_normal((1000, 143)).astype(np.float32), gpu)
    rm.mlp_wide_overflow()
    got = rm.mlp_forward(x, mlp, check_range=False)
    flagged = rm.mlp_wide_overflow()
    h = x.double()
    for i, lin in enumerate(mlp.net):
        h = torch.nn.functional.linear(h, lin.weight.double(), lin.bias.double())
        if i + 1 < len(mlp.net):
            h = torch.relu(h)
    assert bool(torch.isfinite(h).all())
    assert not flagged
    assert bool(torch.isfinite(got).all())
    assert_nonfinite_like(got, h, 1e-4, "relu(-inf)")


@pytest.mark.parametrize("relu", [True, False])
def test_wide_mlp_inference_nan_row_is_nan_or_reported(gpu, relu):
    """A NaN input row through the split-fp16 wide MLP: that row's outputs are NaN (as torch) and the range flag is up; the other rows are
    bit-identical to a clean run.  Never a finite value in the planted row."""
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf.network import MLP, SkipConnMLP
    mlp = (MLP(143, 2, 256, 3, bias=False) if relu else SkipConnMLP(143, 2, 256, 3, skip_layers=[], bias=False)).to(gpu)
    with torch.no_grad():
        for i, lin in enumerate(mlp.net):
            lin.weight.copy_(T(synth.linear_weight(lin.weight.shape[0], lin.weight.shape[1], 300 + i, 2.0), gpu))
    x = T(np.random.default_rng(3).standard_normal((777, 143)).astype(np.float32), gpu)
    rm.mlp_wide_overflow()
    clean = rm.mlp_forward(x, mlp, check_range=False)
    assert not rm.mlp_wide_overflow()
    xp = x.clone()
    xp[100, 7] = NAN
    got = rm.mlp_forward(xp, mlp, check_range=False)
    assert rm.mlp_wide_overflow()
    assert bool(got[100].isnan().all())
    keep = others(777, [100])
    assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("leaky", [False, True])
def test_wide_mlp_native_fp32_training_forward_nonfinite_rows(gpu, leaky):
    """The native fp32 training forward (sn_mlp_wide_forward_train, WIDE_MLP_FORWARD_NATIVE) with NaN / +inf / -inf in three input rows
    against torch in fp64 (ReLU: NaN kept, -inf -> 0).  Its backward is not pinned at non-finite values."""
    from sanerf_hq_amd import ops, synth
    N, din, n_out = 2000, 143, 2
    ws = [T(synth.linear_weight(256, din, 710, 2.0), gpu), T(synth.linear_weight(256, 256, 711, 2.0), gpu), T(synth.linear_weight(n_out, 256, 712, 2.0), gpu)]
    x = T(np.random.default_rng(4).standard_normal((N, din)).astype(np.float32), gpu)
    xp, _ = plant_rows(x)
    old = ops.WIDE_MLP_FORWARD_NATIVE
    ops.WIDE_MLP_FORWARD_NATIVE = True
    try:
        y = ops._wide_mlp_train.apply(xp.clone().requires_grad_(True), leaky, *[w.clone().requires_grad_(True) for w in ws])
    finally:
        ops.WIDE_MLP_FORWARD_NATIVE = old
    act = (lambda t: torch.nn.functional.leaky_relu(t, 0.01)) if leaky else torch.relu
    x64 = xp.double()
    y64 = torch.nn.functional.linear(act(torch.nn.functional.linear(act(torch.nn.functional.linear(x64, ws[0].double())), ws[1].double())), ws[2].double())
    assert_nonfinite_like(y, y64, 1e-5, "forward")


def test_wide_mlp_split_fp16_training_forward_reports_a_nan_row(gpu):
    """The default (split-fp16) training forward with a NaN input row either propagates it or reports it: with the range check on every
    call it raises the fp16-range error, and never returns a finite value for that row."""
    from sanerf_hq_amd import ops, raymarching as rm, synth
    ws = [T(synth.linear_weight(256, 143, 720, 2.0), gpu).requires_grad_(True), T(synth.linear_weight(256, 256, 721, 2.0), gpu).requires_grad_(True),
          T(synth.linear_weight(2, 256, 722, 2.0), gpu).requires_grad_(True)]
    x = torch.randn(20000, 143, device=gpu)
    x[77, 5] = NAN
    rm.mlp_wide_overflow()
    old = ops.WIDE_MLP_RANGE_CHECK_EVERY
    try:
        ops.WIDE_MLP_RANGE_CHECK_EVERY = 0
        y = ops._wide_mlp_train.apply(x, True, *ws)
        assert bool(y[77].isnan().all())
        assert bool(torch.isfinite(torch.cat([y[:77], y[78:]])).all())
        rm.mlp_wide_overflow()
        ops.WIDE_MLP_RANGE_CHECK_EVERY = 1
        with pytest.raises(RuntimeError, match="fp16 range"):
            ops._wide_mlp_train.apply(x, True, *ws)
    finally:
        ops.WIDE_MLP_RANGE_CHECK_EVERY = old
        rm.mlp_wide_overflow()


# ---------------------------------------------------------------------------------------------------------------------------- renderer

def _render(model, ro, rd, table_dtype=torch.float32):
    from sanerf_hq_amd import raymarching as rm
    plan = rm.RenderPlan(model, model.opt.num_steps, table_dtype)
    out = rm.render_rays(plan, ro, rd, want=("inds",))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("mlp", ["f16x3", "mfma32", "valu"])
@pytest.mark.parametrize("f16", [False, True])
def test_fused_renderer_nan_in_view_mlp_weight(gpu, orc, mlp, f16, monkeypatch):
    """A NaN in one hidden weight of view_mlp: the image is NaN on every ray (as in the oracle), depth and weights_sum are bit-identical to a
    clean render, and the sample indices never change.  On each MLP path and both table precisions."""
    from sanerf_hq_amd import _lib, raymarching as rm
    monkeypatch.setattr(rm.tuning, "mlp_mode", {"f16x3": _lib.MLP_F16X3, "mfma32": _lib.MLP_MFMA32, "valu": _lib.MLP_VALU}[mlp])
    steps = [128, 64, 32]
    params = synthetic_params(steps, seed=3)
    if f16:
        params = {k: (v.astype(np.float16).astype(np.float32) if k.endswith("embeddings") else v) for k, v in params.items()}
    tdt = torch.float16 if f16 else torch.float32
    _, _, ro, rd = camera_rays(orc, 24, 24)
    rot, rdt = T(ro, gpu), T(rd, gpu)
    clean = _render(product_model(params, steps, False, gpu), rot, rdt, tdt)
    pv = dict(params)
    pv["view_mlp.net.1.weight"] = params["view_mlp.net.1.weight"].copy()
    pv["view_mlp.net.1.weight"][4, 9] = np.nan
    got = _render(product_model(pv, steps, False, gpu), rot, rdt, tdt)
    assert np.isnan(got["image"]).all(), "a NaN view-MLP weight must reach every pixel"
    assert np.array_equal(got["depth"], clean["depth"]) and np.array_equal(got["weights_sum"], clean["weights_sum"])
    for k in (1, 2):
        assert np.array_equal(got[f"inds{k}"], clean[f"inds{k}"])
    want = orc.render(oracle_cfg(orc, pv, steps, table_f16=f16), ro, rd)
    assert np.isnan(want["image"]).all()
    np.testing.assert_allclose(got["depth"], want["depth"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("mlp", ["f16x3", "mfma32", "valu"])
def test_fused_renderer_nan_in_grid_mlp_weight_vs_oracle(gpu, orc, mlp, monkeypatch):
    """A NaN in one hidden weight of grid_mlp (the last stage's density MLP): the NaN pattern of image, depth and weights_sum is the oracle's,
    and the sample indices (decided by the clean proposal MLPs) do not change."""
    from sanerf_hq_amd import _lib, raymarching as rm
    monkeypatch.setattr(rm.tuning, "mlp_mode", {"f16x3": _lib.MLP_F16X3, "mfma32": _lib.MLP_MFMA32, "valu": _lib.MLP_VALU}[mlp])
    steps = [128, 64, 32]
    params = synthetic_params(steps, seed=3)
    _, _, ro, rd = camera_rays(orc, 24, 24)
    rot, rdt = T(ro, gpu), T(rd, gpu)
    clean = _render(product_model(params, steps, False, gpu), rot, rdt)
    pg = dict(params)
    pg["grid_mlp.net.1.weight"] = params["grid_mlp.net.1.weight"].copy()
    pg["grid_mlp.net.1.weight"][10, 20] = np.nan
    got = _render(product_model(pg, steps, False, gpu), rot, rdt)
    for k in (1, 2):
        assert np.array_equal(got[f"inds{k}"], clean[f"inds{k}"])
    want = orc.render(oracle_cfg(orc, pg, steps), ro, rd)
    for k in ("image", "depth", "weights_sum"):
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=k)
        fin = ~np.isnan(want[k])
        np.testing.assert_allclose(got[k][fin], want[k][fin], rtol=1e-5, atol=1e-5, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------------- optimiser

@pytest.mark.parametrize("mode", ["plain", "capturable", "lazy"])
def test_adam_nan_gradient_element(gpu, mode):
    """sn_adam_step (host counter, capturable, lazy) with one NaN gradient element against torch.optim.Adam: that element (parameter and both
    moments) goes NaN, every other element is as in torch.  The lazy form skips exactly-zero gradients only, so the NaN element is updated
    (touched) and goes NaN too.  (A pin: the optimiser already behaved so.)"""
    from sanerf_hq_amd.optim import Adam
    n = 4096 * 5 + 3
    rng = np.random.default_rng(12)
    p0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(gpu)
    pa, pb = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    oa = Adam([dict(params=[pa], lr=1e-2, lazy=mode == "lazy")], eps=1e-15, capturable=mode == "capturable")
    ob = torch.optim.Adam([dict(params=[pb], lr=1e-2)], eps=1e-15, foreach=False)
    for step in range(3):
        g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(gpu)
        if step == 1:
            g[1234] = NAN
        pa.grad, pb.grad = g.clone(), g.clone()
        oa.step(); ob.step()
    assert_nonfinite_like(pa, pb, 2e-6, "parameter")
    assert int(pa.isnan().sum()) == 1 and bool(pa[1234].isnan())
    for k in ("exp_avg", "exp_avg_sq"):
        assert_nonfinite_like(oa.state[pa][k], ob.state[pb][k], 1e-6, k)
