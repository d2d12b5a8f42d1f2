"""CPU anchors of tests/encoders_ref64.py, the fp64 statement of the SH and frequency encoders, the per-ray head and composite.

  * the SH of the statement against a second, differently shaped one written here (associated-Legendre recurrence with atan2, cos m phi,
    sin m phi) and against the committed vectors of tests/golden/kat_encoders.npz;
  * its autograd dy_dx, and the frequency backward, against a 4th-order central difference of the float64 forward alone;
  * the fp32 TEXT of the kernels (encoders_cases.py: sh_basis.inc parsed into numpy float32, k_sh_backward, k_freq_*, the head) and the
    sequential oracle stay inside the derived bounds -- every ratio is printed (pytest -s) and copied into the table of
    tests/test_gpu_encoders.py;
  * sensitivity: the same statement FAILS its bound when any single literal of sh_basis.inc moves by a relative 1e-4, when two dy_dx planes
    are swapped, the initial gradient is dropped, sin and cos change places at one frequency or the cosine term of the frequency backward
    changes sign;
  * the head and composite statements against a plain per-ray Python loop.
"""
import math
import os

import numpy as np
import pytest
import torch

import encoders_cases as K
import encoders_ref64 as R
from grid_ref64 import worst_ratio
from helpers import GOLD

F32 = np.float32
REL_CHANGE = 1e-4                                                                                # what a changed literal must not survive


@pytest.fixture(scope="module")
def parsed():
    return K.parse_sh_inc()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def sh_by_recurrence(dirs, degree):
    """Real SH of unit vectors [B, 3] float64 from associated Legendre functions by the standard recurrences, the K_l^m normalisation and
    sqrt 2 cos / sin of m phi (the shape of tools/gen_kat_encoders.py::sh_basis, vectorised)."""
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    phi, s = np.arctan2(y, x), np.sqrt(np.maximum(0.0, 1.0 - z * z))
    P = {}
    for m in range(degree):
        pmm = np.ones_like(z)
        for k in range(1, m + 1):
            pmm = pmm * (-(2 * k - 1) * s)                                                       # Condon-Shortley: (-1)^m (2m-1)!! s^m
        P[(m, m)] = pmm
        if m + 1 < degree:
            P[(m + 1, m)] = z * (2 * m + 1) * pmm
        for l in range(m + 2, degree):
            P[(l, m)] = ((2 * l - 1) * z * P[(l - 1, m)] - (l + m - 1) * P[(l - 2, m)]) / (l - m)
    out = np.zeros((dirs.shape[0], degree * degree))
    for l in range(degree):
        for m in range(-l, l + 1):
            am = abs(m)
            Kn = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - am) / math.factorial(l + am))
            ang = 1.0 if m == 0 else math.sqrt(2.0) * (np.cos(m * phi) if m > 0 else np.sin(am * phi))
            out[:, l * l + l + m] = Kn * ang * P[(l, am)]
    return out


@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_statement_matches_the_legendre_recurrence(degree):
    rng = np.random.default_rng(degree)
    d = rng.standard_normal((4000, 3))
    d = np.concatenate([d, R.placed_points().double().numpy()[[0, 1, 2, 3, 4, 5, 6, 7]]])
    d /= np.linalg.norm(d, axis=1, keepdims=True)                                                # unit in float64
    err = float(np.abs(R.sh_values(_t(d), degree).numpy() - sh_by_recurrence(d, degree)).max())
    print(f"SH degree {degree}: polynomial form vs recurrence {err:.2e}")
    assert err <= 1e-12


def test_sh_statement_matches_the_committed_vectors():
    """tests/golden/kat_encoders.npz holds the recurrence on the fp64-renormalised directions; the stored fp32 directions are unit only to
    3e-8, and the polynomial form evaluated ON them differs from the vectors by 1.0e-7 at degree 4 and 4.3e-7 at degree 8 (measured on the
    CPU): the homogeneous degree-l part moves by l times the radius error.  Hence 1e-6 here, against 1e-12 above."""
    kat = np.load(os.path.join(GOLD, "kat_encoders.npz"))
    d = _t(kat["sh.dirs"])
    assert float((d.double().norm(dim=1) - 1).abs().max()) < 1e-7
    for deg in (4, 8):
        err = float((R.sh_values(d, deg) - _t(kat[f"sh.y{deg}"])).abs().max())
        print(f"SH degree {deg}: statement on the stored directions vs vectors {err:.2e}")
        assert err <= 1e-6


def test_term_counts_are_those_of_the_generated_text(parsed):
    """n of every polynomial, value and partials, counted from the coefficient tables = the number of monomials the text sums."""
    for which, macro in enumerate(K.MACROS):
        assert [len(t) for t in parsed[macro]] == R.N_TERMS[which].tolist(), macro


# ---- autograd against a central difference -------------------------------------------------------------------------------------------
def _central(f, x, d, h):
    e = torch.zeros_like(x)
    e[:, d] = h
    return (-f(x + 2 * e) + 8 * f(x + e) - 8 * f(x - e) + f(x - 2 * e)) / (12 * h)


def test_sh_dy_dx_matches_a_central_difference_on_and_off_the_sphere():
    """4th-order central difference of the float64 forward, step h: truncation h^4 / 30 |d^5 Y|.  Along one axis Y is a polynomial of degree
    <= 7 whose coefficients are the other two coordinates' monomials, so |d^5 Y| <= 7!/2! M1 = 2520 M1 with M1 the absolute mass at the
    point with every |coordinate| raised to max(|.|, 1) + 2 h (there |v|^(k-5) <= |v|^k).  Round-off of the difference: 18 function values
    within 2^-52 M1 each over 12 h, doubled."""
    h = 1e-3
    x = R.sh_points(3000, 11).double()
    fw = R.sh_forward(x, 8)
    M1 = R.sh_forward(torch.clamp(x.abs(), min=1.0) + 2 * h, 8, False)["y_mass"]
    tol = h ** 4 / 30 * 2520 * M1 + 2 * 18 * 2.0 ** -52 * M1 / (12 * h)
    worst = 0.0
    for d in range(3):
        err = (_central(lambda v: R.sh_values(v, 8), x, d, h) - fw["dy_dx"][:, d]).abs()
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all())
    print(f"SH dy_dx vs central difference: worst err / tolerance {worst:.3f}, tolerance <= {float(tol.max()):.1e}")


@pytest.mark.parametrize("D,deg", [(3, 6), (1, 1), (2, 4), (3, 0)])
def test_freq_backward_matches_a_central_difference(D, deg):
    """Truncation h^4 / 30 sum_f 2^(5 f) (|g_s| + |g_c|): the fifth derivative of sin(2^f x) is 2^(5 f) cos.  Round-off as above, on the mass of the
    whole row: the differenced scalar is sum(y * g) over all columns."""
    h = 1e-4
    x = K.freq_inputs(300, D, 2.0, 3).double()
    g = torch.randn(300, R.freq_columns(D, deg), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    ref = R.freq_backward(x, g, deg)
    E5 = torch.zeros(300, D, dtype=torch.float64)
    for f in range(deg):
        E5 += 2.0 ** (5 * f) * (g[:, D + 2 * D * f:2 * D + 2 * D * f].abs() + g[:, 2 * D + 2 * D * f:3 * D + 2 * D * f].abs())
    mass = (g[:, :D].abs() * (x.abs() + 1) + ref["E"]).sum(1, keepdim=True)                     # the differenced scalar sums the whole row
    tol = h ** 4 / 30 * E5 + 2 * 18 * 2.0 ** -52 * mass / (12 * h)
    for d in range(D):
        fd = _central(lambda v: (R.freq_values(v, deg) * g).sum(-1, keepdim=True), x, d, h)[:, 0]
        assert bool(((fd - ref["grad_inputs"][:, d]).abs() <= tol[:, d]).all())


# ---- the fp32 text of the SH kernels and the oracle stay inside the bounds ---------------------------------------------------------------
def _sh_ratios(y, dd, fw, degree):
    rv, ev = worst_ratio(_t(y), fw["y"], R.sh_bound(fw["y_mass"], 0, degree))
    rd, ed = worst_ratio(_t(dd).reshape(-1, 3, degree * degree), fw["dy_dx"], R.sh_dy_dx_bound(fw["dy_dx_mass"], degree))
    return rv, rd, ev and ed


def _sphere_and_off(seed, n):
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(2 * n, 3, generator=gen, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True)
    off = v[n:] * (0.25 + 1.75 * torch.rand(n, 1, generator=gen, dtype=torch.float64))
    return {"on the sphere": v[:n].float(), "off the sphere": torch.cat([R.placed_points(), off.float()])}


def test_sh_fp32_text_and_oracle_stay_inside_the_bound(parsed, orc):
    """200 000 unit vectors, 200 000 of radius 0.25 .. 2 and the placed points, degree 8 (every lower degree is a prefix of the same text).
    The oracle evaluates factored forms; their absolute mass is the expanded one (the factors' monomials do not merge) and they stay inside
    the kernel's count, so no count of its own is needed."""
    for name, pts in _sphere_and_off(1, 200000).items():
        fw = R.sh_forward(pts, 8)
        rv, rd, exact = _sh_ratios(*K.sh_text32(parsed, pts.numpy(), 8), fw, 8)
        oy, od = orc.sh_encode_forward(pts.numpy(), 8, True)
        ov, odr, oexact = _sh_ratios(oy, od, fw, 8)
        print(f"SH {name}: fp32 text values {rv:.3f} partials {rd:.3f}; oracle values {ov:.3f} partials {odr:.3f}")
        assert exact and oexact and max(rv, rd, ov, odr) <= 1.0


@pytest.mark.parametrize("degree", [1, 2, 5, 8])
def test_sh_backward_fp32_text_and_oracle_stay_inside_the_bound(parsed, orc, degree):
    pts = R.sh_points(4099, 20 + degree)
    gen = torch.Generator().manual_seed(degree)
    g = torch.randn(4099, degree * degree, generator=gen)
    fw = R.sh_forward(pts, degree)
    _, dd = K.sh_text32(parsed, pts.numpy(), degree)
    for start in ("zeros", "random"):
        g0 = torch.zeros(4099, 3) if start == "zeros" else torch.randn(4099, 3, generator=gen)
        ref = R.sh_backward(g, fw["dy_dx"], g0)
        bound = R.sh_backward_bound(g, ref["mass"], fw["dy_dx_mass"], degree)
        ratio, exact = worst_ratio(_t(K.sh_backward_text32(g.numpy(), dd, g0.numpy())), ref["grad_inputs"], bound)
        gi = g0.numpy().copy()
        orc.lib().orc_sh_encode_backward(orc._ptr(g.numpy()), orc._ptr(pts.numpy()), 4099, 3, degree, orc._ptr(np.ascontiguousarray(dd)), orc._ptr(gi))
        oratio, oexact = worst_ratio(_t(gi), ref["grad_inputs"], bound)
        print(f"SH backward degree {degree} from {start}: fp32 text {ratio:.3f}, oracle {oratio:.3f}")
        assert exact and oexact and max(ratio, oratio) <= 1.0
        # sensitivity: the initial content dropped, and two planes of dy_dx swapped in the last degree block
        if start == "random":
            dropped = K.sh_backward_text32(g.numpy(), dd, np.zeros((4099, 3), F32))
            assert worst_ratio(_t(dropped), ref["grad_inputs"], bound)[0] > 1.0
        if degree > 1:
            swapped = dd.copy()
            lo = (degree - 1) ** 2
            swapped[:, 1, lo:], swapped[:, 2, lo:] = dd[:, 2, lo:], dd[:, 1, lo:]
            r = worst_ratio(_t(swapped), fw["dy_dx"], R.sh_dy_dx_bound(fw["dy_dx_mass"], degree))
            rb = worst_ratio(_t(K.sh_backward_text32(g.numpy(), swapped, g0.numpy())), ref["grad_inputs"], bound)
            assert (not r[1] or r[0] > 1.0) and rb[0] > 1.0


def test_every_literal_of_the_generated_text_is_pinned(parsed):
    """Each of the 590 literals of the four macros, multiplied by 1 + 1e-4 in turn, makes the fp32 text miss the bound of its polynomial on
    encoders_cases.sensitivity_points() (and by 1 - 1e-4).  Measured on the CPU with the same points: the smallest relative change
    that is caught for EVERY literal is 5e-6 (see REL_CHANGE); unchanged, the text stays inside (first assertion)."""
    pts = K.sensitivity_points()
    fw = R.sh_forward(pts, 8)
    p = pts.numpy()
    pw = [K.powers32(p[:, a]) for a in range(3)]
    missed = []
    for which, macro in enumerate(K.MACROS):
        for i, terms in enumerate(parsed[macro]):
            ref = fw["y"][:, i] if which == 0 else fw["dy_dx"][:, which - 1, i]
            mass = fw["y_mass"][:, i] if which == 0 else fw["dy_dx_mass"][:, which - 1, i]
            bound = 2.0 * (R.L_OF[i] + 4 + R.N_TERMS[which][i]) * R.U * mass
            ratio, exact = worst_ratio(_t(K.eval_terms32(terms, pw)), ref, bound)
            assert exact and ratio <= 1.0, (macro, i, ratio)
            for j in range(len(terms)):
                for factor in (1 + REL_CHANGE, 1 - REL_CHANGE):
                    if worst_ratio(_t(K.eval_terms32(terms, pw, scale=(j, factor))), ref, bound)[0] <= 1.0:
                        missed.append((macro, i, j, factor))
    assert not missed, missed[:10]


# ---- frequency encoder ---------------------------------------------------------------------------------------------------------------
FREQ_CPU = [(3, 10, 2.0), (1, 1, 1.0), (2, 6, 4.0), (5, 4, 1.0), (3, 0, 1.0), (4, 12, 2.0)]


@pytest.mark.parametrize("D,deg,rng", FREQ_CPU)
def test_freq_fp32_text_and_oracle_stay_inside_the_bound(orc, D, deg, rng):
    """k_freq_forward / k_freq_backward in numpy float32 and the oracle.  eps_fwd is the worst error of the host's fp32 sin / cos seen
    on this case (the device's own figure is measured in tests/test_gpu_encoders.py); identity columns are bit-equal to the input."""
    B = 4099
    x = K.freq_inputs(B, D, rng, 7 * D + deg)
    g = torch.randn(B, R.freq_columns(D, deg), generator=torch.Generator().manual_seed(deg))
    y64 = R.freq_values(x, deg)
    ref = R.freq_backward(x, g, deg)
    for name, y in (("fp32 text", K.freq_forward_text32(x.numpy(), deg)), ("oracle", orc.freq_encode_forward(x.numpy(), deg))):
        assert y.shape == (B, R.freq_columns(D, deg)) and np.array_equal(y[:, :D].view(np.uint32), x.numpy().view(np.uint32))
        eps = float((_t(y).double() - y64).abs().max())
        assert eps <= 2e-6
        bound = R.freq_backward_bound(ref["M"], ref["E"], deg, eps)
        gi = K.freq_backward_text32(g.numpy(), y, D, deg) if name == "fp32 text" else orc.freq_encode_backward(g.numpy(), y, D, deg)
        ratio, exact = worst_ratio(_t(gi), ref["grad_inputs"], bound)
        print(f"freq D={D} deg={deg} +-{rng}: {name} forward err {eps / R.U:.2f} u, backward {ratio:.3f}")
        assert exact and ratio <= 1.0
        if name == "fp32 text" and deg > 0:
            # sensitivity: sin and cos exchanged at the last frequency; the cosine term's sign flipped in the backward
            f = deg - 1
            sw = y.copy()
            sw[:, D + 2 * D * f:2 * D + 2 * D * f], sw[:, 2 * D + 2 * D * f:3 * D + 2 * D * f] = y[:, 2 * D + 2 * D * f:3 * D + 2 * D * f], y[:, D + 2 * D * f:2 * D + 2 * D * f]
            assert float((_t(sw).double() - y64).abs().max()) > 2e-6
            assert worst_ratio(_t(K.freq_backward_text32(g.numpy(), sw, D, deg)), ref["grad_inputs"], bound)[0] > 1.0
            assert worst_ratio(_t(K.freq_backward_text32(g.numpy(), y, D, deg, cos_sign=-1.0)), ref["grad_inputs"], bound)[0] > 1.0


# ---- per-ray head and composite ------------------------------------------------------------------------------------------------------
def test_head_and_composite_statements_match_a_per_ray_loop():
    """A handful of rays in plain Python floats, the SH from the recurrence above: values and the gradients written out term by term."""
    N, T = 5, 7
    w, t, raw, d, g_ws, g_depth, g_f = [v.double() for v in K.head_inputs(N, T, 3)]
    fw = R.head_forward(w, t, raw, d)
    bw = R.head_backward(w, t, raw, d, g_ws, g_depth, g_f)
    sh = sh_by_recurrence((d / d.norm(dim=1, keepdim=True)).numpy(), 4)
    for n in range(N):
        ws = sum(float(w[n, j]) for j in range(T))
        depth = sum(float(w[n, j]) * float(t[n, j]) for j in range(T))
        assert abs(ws - float(fw["ws"][n])) <= 1e-14 and abs(depth - float(fw["depth"][n])) <= 1e-13
        for c in range(15):
            assert abs(sum(float(w[n, j]) * float(raw[n, j, 1 + c]) for j in range(T)) - float(fw["f"][n, c])) <= 1e-13
        for k in range(16):
            assert abs(sh[n, k] * ws - float(fw["f"][n, 15 + k])) <= 1e-12
        for j in range(T):
            gw = float(g_ws[n]) + float(g_depth[n]) * float(t[n, j]) + sum(float(g_f[n, c]) * float(raw[n, j, 1 + c]) for c in range(15)) \
                + sum(float(g_f[n, 15 + k]) * sh[n, k] for k in range(16))
            assert abs(gw - float(bw["g_weights"][n, j])) <= 1e-12
            assert float(bw["g_raw"][n, j, 0]) == 0.0
            for c in range(15):
                assert abs(float(w[n, j]) * float(g_f[n, c]) - float(bw["g_raw"][n, j, 1 + c])) <= 1e-15
    K_ = 3
    v = torch.randn(N, T, K_, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    g = torch.randn(N, K_, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    out, grads = R.composite(w, v), R.composite_grads(w, v, g)
    for n in range(N):
        for k in range(K_):
            assert abs(sum(float(w[n, j]) * float(v[n, j, k]) for j in range(T)) - float(out["out"][n, k])) <= 1e-14
        for j in range(T):
            assert abs(sum(float(v[n, j, k]) * float(g[n, k]) for k in range(K_)) - float(grads["g_weights"][n, j])) <= 1e-13
            for k in range(K_):
                assert abs(float(w[n, j]) * float(g[n, k]) - float(grads["g_values"][n, j, k])) <= 1e-15


@pytest.mark.parametrize("N,T", [(1, 1), (17, 64), (130, 300)])
def test_head_fp32_text_stays_inside_the_bounds(parsed, N, T):
    for zero in (False, True):
        w, t, raw, d, g_ws, g_depth, g_f = K.head_inputs(N, T, N + T, zero_weights=zero)
        a = [v.numpy() for v in (w, t, raw, d)]
        ws, depth, f = K.head_forward_text32(parsed, *a)
        for keep in K.GRAD_SETS:
            grads = tuple(g if k else None for g, k in zip((g_ws, g_depth, g_f), keep))
            gw, gr = K.head_backward_text32(parsed, *a, *[None if g is None else g.numpy() for g in grads])
            res = K.head_checks(dict(ws=_t(ws), depth=_t(depth), f=_t(f), g_weights=_t(gw), g_raw=_t(gr)), w, t, raw, d, grads)
            assert all(exact and ratio <= 1.0 for ratio, exact in res.values()), res
            assert not gr[..., 0].any()
        print(f"head N={N} T={T} zero weights={zero}: " + ", ".join(f"{k} {v[0]:.3f}" for k, v in res.items()))
    # sensitivity: a backward that forgets the g_depth term misses
    w, t, raw, d, g_ws, g_depth, g_f = K.head_inputs(N, T, N + T)
    a = [v.numpy() for v in (w, t, raw, d)]
    gw, gr = K.head_backward_text32(parsed, *a, g_ws.numpy(), None, g_f.numpy())
    res = K.head_checks(dict(g_weights=_t(gw), g_raw=_t(gr)), w, t, raw, d, (g_ws, g_depth, g_f))
    assert res["g_weights"][0] > 1.0
