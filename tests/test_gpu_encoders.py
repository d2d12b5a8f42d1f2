"""GPU tests of the direction side of the field against the fp64 statement of tests/encoders_ref64.py: the SH and frequency encoders
(encoders.hip: k_sh_forward / k_sh_backward, k_freq_forward / k_freq_backward), the per-ray head k_ray_composite[_backward] and
k_composite[_backward] (raymarch.hip).  The CPU tests of tests/test_encoders_ref64.py anchor that statement (Legendre recurrence, committed
vectors, central differences, a per-ray loop), hold the fp32 text of the kernels and the sequential oracle to the same bounds and show that
a literal of sh_basis.inc changed by a relative 1e-4 (5e-6 is the smallest change caught for every literal), swapped dy_dx planes, a
dropped initial gradient, exchanged sin / cos and a flipped sign all miss them.

  * through the raw C ABI, and once per family through the autograd wrapper;
  * SH: degrees 1..8, B = 1, 255, 256, 257, 4099 (placed points -- axes, planes where whole polynomials vanish, -0.0, the origin, a
    point far off the sphere -- plus random unit and off-sphere vectors), with and without dy_dx (same bits), into NaN-filled buffers with
    room past the end; the backward from zeros and from random content (it accumulates);
  * frequency encoder: every (D, deg) of encoders_cases.FREQ_CASES, inputs in +-1, +-2, +-4 with 0, -0.0 and powers of two;
  * head: every (N, T) of encoders_cases.HEAD_SHAPES, |d| from 1e-3 to 1e3, weights that sum to 1 and weights of zeros, each subset of
    the three output gradients (NULL pointers in the kernel); composite: K = 1 .. 256;
  * rejections and empty batches.

Every tolerance is a derived bound (encoders_ref64.py) and every assertion is `exact and ratio <= 1`, with one exception that cannot be
derived: the accuracy of the device's sinf / cosf.  FREQ_FWD_BAR: the worst |kernel - fp64| over all the frequency cases here measured on an
MI355X is 6.95e-8 = 1.17 x 2^-24 (D = 4, deg = 12; every case with a frequency gives 1.08 .. 1.17 x 2^-24); the bar is twice that rounded
up to a power of two, 2^-22 = 2.4e-7 (the suite's older oracle comparison allows 2e-6), and is the eps_fwd of the backward bound.

Worst |err| / bound per family (a measurement against the fp64 statement, not a threshold).  The first column is the fp32 text of the kernel in
numpy on the CPU, the second the sequential oracle on the CPU (both printed by tests/test_encoders_ref64.py), the third these tests on
an MI355X (they print every ratio, pytest -s):

  family                                        fp32 text  oracle   kernel
  SH values (on / off the sphere)                 0.22      0.26    0.20
  SH partials                                     0.22      0.19    0.18
  SH backward, from zeros                         0.04      0.04    0.07
  SH backward, from random content                0.09      0.09    0.09
  frequency backward (eps_fwd: CPU the worst host
    sin / cos error of the case, kernel the bar)  0.22      0.24    0.15
  head: weights_sum, depth, feature sums          0.04       -      0.12
  head: SH channels                               0.06       -      0.11
  head: g_weights                                 0.03       -      0.05
  head: g_raw (one rounding: at most 1)           1.00       -      1.00
  composite forward / g_weights                    -         -      0.25 / 0.28
"""
import ctypes

import pytest
import torch

import encoders_cases as K
import encoders_ref64 as R
from grid_ref64 import worst_ratio

pytestmark = pytest.mark.gpu

ERR_INVALID = -1                                                                                 # include/sanerf_hip.h: SN_ERR_INVALID
FREQ_FWD_BAR = 2.0 ** -22                                                                            # see the module docstring
NAN = float("nan")


def _l():
    from sanerf_hq_amd import _lib as m
    return m.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    torch.cuda.synchronize()
    assert rc == 0, _l().sn_last_error().decode()


def _nan(n, dev, guard=64):
    """A flat NaN-filled buffer of n elements with `guard` more past the end."""
    return torch.full((n + guard,), NAN, device=dev)


def _untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all()) and not bool(torch.isnan(buf[:n]).any())


def _check(got, ref, bound, what):
    ratio, exact = worst_ratio(got, ref, bound)
    assert exact and ratio <= 1.0, f"{what}: worst |err| / bound {ratio:.3f}, zero-bound elements exact: {exact}"
    return ratio


# ---- spherical harmonics -------------------------------------------------------------------------------------------------------------
SH_B = [1, 255, 256, 257, 4099]


@pytest.fixture(scope="module")
def sh_ref(gpu):
    """The 4099 points, the placed ones shuffled among the random unit and off-sphere vectors so that every batch size takes a prefix with
    all kinds in it, and their degree-8 statement, computed once: a lower degree is the prefix of the same columns."""
    pts = R.sh_points(4099, 31)
    pts = pts[torch.randperm(4099, generator=torch.Generator().manual_seed(32))].to(gpu)
    return pts, R.sh_forward(pts, 8)


def _sh_slice(sh_ref, B, degree):
    pts, fw = sh_ref
    C2 = degree * degree
    return pts[:B].contiguous(), dict(y=fw["y"][:B, :C2], y_mass=fw["y_mass"][:B, :C2], dy_dx=fw["dy_dx"][:B, :, :C2], dy_dx_mass=fw["dy_dx_mass"][:B, :, :C2])


def hip_sh_forward(x, degree, want_dy_dx):
    B, C2 = x.shape[0], degree * degree
    out, dd = _nan(B * C2, x.device), (_nan(B * 3 * C2, x.device) if want_dy_dx else None)
    _ok(_l().sn_sh_encode_forward(_p(x), _p(out), B, 3, degree, _p(dd), _s()))
    assert _untouched(out, B * C2), "outputs: a write past B * degree^2 elements, or an element left unwritten"
    assert dd is None or _untouched(dd, B * 3 * C2), "dy_dx: a write past B * 3 * degree^2 elements, or an element left unwritten"
    return out[:B * C2].view(B, C2), (None if dd is None else dd[:B * 3 * C2].view(B, 3, C2))


@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_forward_and_dy_dx_match_fp64(gpu, sh_ref, degree):
    rv = rd = 0.0
    for B in SH_B:
        x, ref = _sh_slice(sh_ref, B, degree)
        y, dd = hip_sh_forward(x, degree, True)
        y0, _ = hip_sh_forward(x, degree, False)
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), "dy_dx == NULL changes the bits of outputs"
        rv = max(rv, _check(y, ref["y"], R.sh_bound(ref["y_mass"], 0, degree), f"SH values degree {degree} B={B}"))
        rd = max(rd, _check(dd, ref["dy_dx"], R.sh_dy_dx_bound(ref["dy_dx_mass"], degree), f"SH dy_dx degree {degree} B={B}"))
    print(f"SH degree {degree}: values {rv:.3f} partials {rd:.3f}")


@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_backward_accumulates_and_matches_fp64(gpu, sh_ref, degree):
    gen = torch.Generator(device=gpu).manual_seed(degree)
    r0 = r1 = 0.0
    for B in SH_B:
        x, ref = _sh_slice(sh_ref, B, degree)
        _, dd = hip_sh_forward(x, degree, True)
        g = torch.randn(B, degree * degree, generator=gen, device=gpu)
        for start in ("zeros", "random"):
            g0 = torch.zeros(B, 3, device=gpu) if start == "zeros" else torch.randn(B, 3, generator=gen, device=gpu)
            buf = _nan(B * 3, gpu)
            buf[:B * 3] = g0.view(-1)
            _ok(_l().sn_sh_encode_backward(_p(g), _p(x), B, 3, degree, _p(dd.contiguous()), _p(buf), _s()))
            assert _untouched(buf, B * 3)
            want = R.sh_backward(g, ref["dy_dx"], g0)
            ratio = _check(buf[:B * 3].view(B, 3), want["grad_inputs"], R.sh_backward_bound(g, want["mass"], ref["dy_dx_mass"], degree),
                           f"SH backward degree {degree} B={B} from {start}")
            r0, r1 = (max(r0, ratio), r1) if start == "zeros" else (r0, max(r1, ratio))
    print(f"SH backward degree {degree}: from zeros {r0:.3f}, from random content {r1:.3f}")


def test_sh_wrapper_layout_under_autograd(gpu, sh_ref):
    from sanerf_hq_amd.shencoder import sh_encode
    x, ref = _sh_slice(sh_ref, 257, 5)
    xt = x.clone().requires_grad_(True)
    y = sh_encode(xt, 5, True)
    g = torch.randn(257, 25, generator=torch.Generator(device=gpu).manual_seed(9), device=gpu)
    y.backward(g)
    _check(y.detach(), ref["y"], R.sh_bound(ref["y_mass"], 0, 5), "sh_encode values")
    want = R.sh_backward(g, ref["dy_dx"])
    print(f"sh_encode under autograd: {_check(xt.grad, want['grad_inputs'], R.sh_backward_bound(g, want['mass'], ref['dy_dx_mass'], 5), 'sh_encode input gradient'):.3f}")


# ---- frequency encoder ---------------------------------------------------------------------------------------------------------------
def hip_freq_forward(x, deg):
    B, D = x.shape
    C = R.freq_columns(D, deg)
    out = _nan(B * C, x.device)
    _ok(_l().sn_freq_encode_forward(_p(x), B, D, deg, C, _p(out), _s()))
    assert _untouched(out, B * C)
    return out[:B * C].view(B, C)


@pytest.mark.parametrize("D,deg", K.FREQ_CASES)
def test_freq_forward_and_backward_match_fp64(gpu, D, deg):
    """Forward: identity columns bit-equal to the input, sin / cos columns within FREQ_FWD_BAR of the float64 values (the one measured bar,
    see the module docstring).  Backward through the ABI from the kernel's own outputs, inside the derived bound with eps_fwd = that bar."""
    worst, rb = 0.0, 0.0
    for B in (1, 257, 4099):
        for rng in (1.0, 2.0, 4.0):
            x = K.freq_inputs(B, D, rng, 100 * D + deg, gpu)
            if B == 1:                                                                           # one row: make it the full-range one
                x = x * 0 + rng * (1 - 2.0 ** -10)
            C = R.freq_columns(D, deg)
            y = hip_freq_forward(x, deg)
            assert torch.equal(y[:, :D].view(torch.int32), x.view(torch.int32)), "identity columns are not the input's bits"
            y64 = R.freq_values(x, deg)
            worst = max(worst, float((y.double() - y64).abs().max()))
            g = torch.randn(B, C, generator=torch.Generator(device=gpu).manual_seed(B + deg), device=gpu)
            gi = _nan(B * D, gpu)
            _ok(_l().sn_freq_encode_backward(_p(g), _p(y.contiguous()), B, D, deg, C, _p(gi), _s()))
            assert _untouched(gi, B * D)
            ref = R.freq_backward(x, g, deg)
            rb = max(rb, _check(gi[:B * D].view(B, D), ref["grad_inputs"], R.freq_backward_bound(ref["M"], ref["E"], deg, FREQ_FWD_BAR),
                                f"freq backward D={D} deg={deg} B={B} +-{rng}"))
    print(f"freq D={D} deg={deg}: forward worst |err| {worst:.3e} = {worst / R.U:.2f} u, backward {rb:.3f}")
    assert worst <= FREQ_FWD_BAR, f"sin / cos columns: {worst:.3e} > {FREQ_FWD_BAR:.3e}"


@pytest.mark.parametrize("D,deg,shape", [(3, 10, (257,)), (2, 6, (17, 5))])
def test_freq_encoder_module_under_autograd(gpu, D, deg, shape):
    from sanerf_hq_amd.freqencoder import FreqEncoder
    n = 1
    for s in shape:
        n *= s
    x = K.freq_inputs(n, D, 2.0, 5, gpu)
    xt = x.view(*shape, D).clone().requires_grad_(True)
    y = FreqEncoder(input_dim=D, degree=deg)(xt)
    C = R.freq_columns(D, deg)
    assert tuple(y.shape) == (*shape, C)
    g = torch.randn(n, C, generator=torch.Generator(device=gpu).manual_seed(6), device=gpu)
    y.backward(g.view(*shape, C))
    assert float((y.detach().view(n, C).double() - R.freq_values(x, deg)).abs().max()) <= FREQ_FWD_BAR
    ref = R.freq_backward(x, g, deg)
    _check(xt.grad.view(n, D), ref["grad_inputs"], R.freq_backward_bound(ref["M"], ref["E"], deg, FREQ_FWD_BAR), "FreqEncoder input gradient")


# ---- per-ray head --------------------------------------------------------------------------------------------------------------------
def hip_head_forward(w, t, raw, d):
    N, T = w.shape
    ws, depth, f = _nan(N, w.device), _nan(N, w.device), _nan(N * 31, w.device)
    _ok(_l().sn_rm_ray_composite(_p(w), _p(t), _p(raw), _p(d), N, T, _p(ws), _p(depth), _p(f), _s()))
    assert _untouched(ws, N) and _untouched(depth, N) and _untouched(f, N * 31)
    return dict(ws=ws[:N], depth=depth[:N], f=f[:N * 31].view(N, 31))


def hip_head_backward(w, t, raw, d, grads):
    N, T = w.shape
    gw, gr = _nan(N * T, w.device), _nan(N * T * 16, w.device)
    _ok(_l().sn_rm_ray_composite_backward(_p(w), _p(t), _p(raw), _p(d), *[_p(g) for g in grads], N, T, _p(gw), _p(gr), _s()))
    assert _untouched(gw, N * T) and _untouched(gr, N * T * 16)
    return dict(g_weights=gw[:N * T].view(N, T), g_raw=gr[:N * T * 16].view(N, T, 16))


def _assert_head(res, what, worst):
    for k, (ratio, exact) in res.items():
        assert exact and ratio <= 1.0, f"{what}: {k} worst |err| / bound {ratio:.3f}, zero-bound elements exact: {exact}"
        worst[k] = max(worst.get(k, 0.0), ratio)


@pytest.mark.parametrize("N,T", K.HEAD_SHAPES)
def test_head_forward_and_every_gradient_subset_match_fp64(gpu, N, T):
    from sanerf_hq_amd import raymarching as rm
    worst = {}
    for zero in (False, True):
        w, t, raw, d, g_ws, g_depth, g_f = K.head_inputs(N, T, 10 * N + T, zero_weights=zero, device=gpu)
        _assert_head(K.head_checks(hip_head_forward(w, t, raw, d), w, t, raw, d, (None, None, None)), f"head forward N={N} T={T}", worst)
        for keep in K.GRAD_SETS:
            grads = tuple(g if k else None for g, k in zip((g_ws, g_depth, g_f), keep))
            got = hip_head_backward(w, t, raw, d, grads)
            assert not bool(got["g_raw"][..., 0].any()), "g_raw[..., 0] is not exactly 0"
            _assert_head(K.head_checks(got, w, t, raw, d, grads), f"head backward (ABI) N={N} T={T} gradients {keep}", worst)
            if zero:
                continue
            wt, rt = w.clone().requires_grad_(True), raw.clone().requires_grad_(True)
            outs = rm.ray_composite(wt, t, rt, d)
            sum((o * g).sum() for o, g in zip(outs, grads) if g is not None).backward()
            got = dict(g_weights=wt.grad, g_raw=rt.grad)
            assert not bool(rt.grad[..., 0].any())
            _assert_head(K.head_checks(got, w, t, raw, d, grads), f"head backward (autograd) N={N} T={T} gradients {keep}", worst)
    print(f"head N={N} T={T}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- composite -----------------------------------------------------------------------------------------------------------------------
def composite_gw_bound(K_, mass):
    """2 (K + 1) u sum_k |v g|: the wrapper sums the K products v g in fp32 in an order of torch's choosing: K products rounded once each
    and K - 1 additions, each rounding a partial sum of at most the mass -- at most K in units of u * mass, taken as K + 1."""
    return 2.0 * (K_ + 1) * R.U * mass


@pytest.mark.parametrize("K_", [1, 3, 15, 31, 256])
def test_composite_forward_and_both_gradients_match_fp64(gpu, K_):
    from sanerf_hq_amd import raymarching as rm
    rf = rw = 0.0
    for T in (1, 33):
        for N in (1, 257):
            gen = torch.Generator(device=gpu).manual_seed(1000 * K_ + 10 * T + N)
            w = torch.rand(N, T, generator=gen, device=gpu)
            v = torch.randn(N, T, K_, generator=gen, device=gpu)
            g = torch.randn(N, K_, generator=gen, device=gpu)
            ref, gref = R.composite(w, v), R.composite_grads(w, v, g)
            out, gv = _nan(N * K_, gpu), _nan(N * T * K_, gpu)
            _ok(_l().sn_rm_composite(_p(w), _p(v), N, T, K_, _p(out), _s()))
            _ok(_l().sn_rm_composite_backward(_p(w), _p(g), N, T, K_, _p(gv), _s()))
            assert _untouched(out, N * K_) and _untouched(gv, N * T * K_)
            what = f"composite K={K_} T={T} N={N}"
            rf = max(rf, _check(out[:N * K_].view(N, K_), ref["out"], R.sum_bound(T, ref["mass"]), what + " forward"))
            _check(gv[:N * T * K_].view(N, T, K_), gref["g_values"], R.product_bound(gref["g_values"]), what + " g_values")
            wt, vt = w.clone().requires_grad_(True), v.clone().requires_grad_(True)
            o = rm.composite(wt, vt)
            o.backward(g)
            assert torch.equal(o.detach(), out[:N * K_].view(N, K_))
            _check(vt.grad, gref["g_values"], R.product_bound(gref["g_values"]), what + " g_values (autograd)")
            rw = max(rw, _check(wt.grad, gref["g_weights"], composite_gw_bound(K_, gref["g_weights_mass"]), what + " g_weights (autograd)"))
    print(f"composite K={K_}: forward {rf:.3f}, g_weights {rw:.3f}")


# ---- rejections and empties ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch_and_empty_batches_are_fine(gpu):
    l = _l()
    x, a, b, c = torch.rand(8, 3, device=gpu), _nan(8 * 64 * 3, gpu, 0), _nan(8 * 64 * 3, gpu, 0), _nan(8 * 64 * 3, gpu, 0)
    s = _s()
    bad = [
        l.sn_sh_encode_forward(_p(x), _p(a), 8, 2, 4, _p(b), s), l.sn_sh_encode_forward(_p(x), _p(a), 6, 4, 4, _p(b), s),      # D != 3
        l.sn_sh_encode_backward(_p(x), _p(x), 8, 2, 4, _p(x), _p(a), s),
        l.sn_sh_encode_forward(_p(x), _p(a), 8, 3, 0, _p(b), s), l.sn_sh_encode_backward(_p(x), _p(x), 8, 3, 0, _p(x), _p(a), s),  # degree 0
        l.sn_sh_encode_backward(_p(x), _p(x), 8, 3, 9, _p(x), _p(a), s),                                                          # degree 9
        l.sn_sh_encode_forward(None, _p(a), 8, 3, 4, _p(b), s), l.sn_sh_encode_forward(_p(x), None, 8, 3, 4, _p(b), s),
        l.sn_sh_encode_backward(None, _p(x), 8, 3, 4, _p(x), _p(a), s), l.sn_sh_encode_backward(_p(x), _p(x), 8, 3, 4, None, _p(a), s),
        l.sn_sh_encode_backward(_p(x), _p(x), 8, 3, 4, _p(x), None, s),
        l.sn_freq_encode_forward(_p(x), 8, 3, 4, 24, _p(a), s), l.sn_freq_encode_forward(_p(x), 8, 2, 4, 27, _p(a), s),           # C != D + 2 D deg
        l.sn_freq_encode_backward(_p(x), _p(x), 8, 3, 4, 28, _p(a), s), l.sn_freq_encode_backward(_p(x), _p(x), 8, 3, 0, 4, _p(a), s),
        l.sn_freq_encode_forward(None, 8, 3, 4, 27, _p(a), s), l.sn_freq_encode_forward(_p(x), 8, 3, 4, 27, None, s),
        l.sn_freq_encode_backward(None, _p(x), 8, 3, 4, 27, _p(a), s), l.sn_freq_encode_backward(_p(x), None, 8, 3, 4, 27, _p(a), s),
        l.sn_freq_encode_backward(_p(x), _p(x), 8, 3, 4, 27, None, s),
        l.sn_rm_ray_composite(_p(x), _p(x), _p(x), None, 1, 1, _p(a), _p(b), _p(c), s),
        l.sn_rm_ray_composite_backward(_p(x), _p(x), _p(x), _p(x), None, None, None, 1, 1, None, _p(a), s),
        l.sn_rm_ray_composite_backward(_p(x), _p(x), _p(x), _p(x), None, None, None, 1, 1, _p(a), None, s),
        l.sn_rm_composite(_p(x), None, 1, 1, 1, _p(a), s), l.sn_rm_composite(_p(x), _p(x), 1, 1, 1, None, s),
        l.sn_rm_composite_backward(None, _p(x), 1, 1, 1, _p(a), s), l.sn_rm_composite_backward(_p(x), _p(x), 1, 1, 1, None, s),
    ]
    torch.cuda.synchronize()
    assert all(rc == ERR_INVALID for rc in bad), bad
    empty = [
        l.sn_sh_encode_forward(_p(x), _p(a), 0, 3, 4, _p(b), s), l.sn_sh_encode_backward(_p(x), _p(x), 0, 3, 4, _p(x), _p(a), s),
        l.sn_freq_encode_forward(_p(x), 0, 3, 4, 27, _p(a), s), l.sn_freq_encode_backward(_p(x), _p(x), 0, 3, 4, 27, _p(a), s),
        l.sn_rm_ray_composite(_p(x), _p(x), _p(x), _p(x), 0, 4, _p(a), _p(b), _p(c), s),
        l.sn_rm_ray_composite_backward(_p(x), _p(x), _p(x), _p(x), None, None, None, 0, 4, _p(a), _p(b), s),
        l.sn_rm_composite(_p(x), _p(x), 0, 4, 3, _p(a), s), l.sn_rm_composite_backward(_p(x), _p(x), 0, 4, 3, _p(a), s),
    ]
    torch.cuda.synchronize()
    assert all(rc == 0 for rc in empty), empty
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and bool(torch.isnan(c).all()), "a refused or empty call wrote something"
