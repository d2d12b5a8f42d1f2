"""An fp64 statement of the direction side of the field for the tests, and the fp32 round-off bounds that go with it: the SH and frequency
encoders (csrc/encoders.hip), the per-ray head k_ray_composite[_backward] and k_composite[_backward] (csrc/raymarch.hip).

Written for the tests alone, in the style of grid_ref64.py: vectorised torch that runs on any device; nothing here imports oracle/ or the
package's encoders, and sh_basis.inc is not read.

Real spherical harmonics, from the definition tools/gen_sh.py documents (index l^2 + l + m, Condon-Shortley phase, l < degree <= 8):

    Y_l^m(x, y, z) = N_l^|m| (-1)^m  d^|m|/dz^|m| P_l(z)  A_m(x, y)
    A_m = sqrt 2 Re (x + i y)^m  (m > 0),   sqrt 2 Im (x + i y)^|m|  (m < 0),   1  (m = 0)
    N_l^m = sqrt((2 l + 1) / (4 pi) (l - m)! / (l + m)!)

The Legendre factor is a polynomial in z alone (numpy.polynomial.legendre, computed once), A_m a polynomial in x and y: Y is a polynomial
in INDEPENDENT x, y, z, defined off the sphere, and its three partials are unique polynomials.  dy_dx comes from torch.autograd (forward
mode, one pass per input dimension) on the float64 forward, not from a derivative list.  The expanded polynomial is the product of a
z-polynomial and an (x, y)-polynomial and no two of its monomials merge, so the absolute mass of its monomials factors as well:
sum |monomial| = |N| (sum_k |p_k| |z|^k) (sum_j |a_j| |x|^a |y|^b); the masses of the partials follow in the same way from the coefficient
arrays of the differentiated factor, and the number of monomials n is the product of the two term counts.

Bounds (u = 2^-24, first-order count of the fp32 roundings, factor 2 of margin as in grid_ref64.py; the library is built with
-ffp-contract=off, so the counts are what the text of the kernels performs).  Each count is derived in the docstring of its function:
sh_bound, sh_backward_bound, freq_backward_bound, sum_bound, head_sh_bound, head_gw_bound, product_bound.
"""
import math

import numpy as np
import torch
from numpy.polynomial import legendre as _leg
from numpy.polynomial import polynomial as _poly

U = 2.0 ** -24
MAXDEG = 8
NP = MAXDEG                                                                                      # powers 0 .. 7 of each coordinate


# ---- spherical harmonics: coefficient tables, built once ----------------------------------------------------------------------------
def _tables():
    """PZ [64, 8]: N (-1)^m d^|m|/dz^|m| P_l as ascending coefficients in z;  AXY [64, 8, 8]: A_m as coefficients of x^a y^b."""
    pz = np.zeros((MAXDEG * MAXDEG, NP))
    axy = np.zeros((MAXDEG * MAXDEG, NP, NP))
    for l in range(MAXDEG):
        base = _leg.leg2poly([0.0] * l + [1.0])                                                  # P_l(z), ascending powers
        for m in range(-l, l + 1):
            am, i = abs(m), l * l + l + m
            p = _poly.polyder(base, am) if am else base
            N = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - am) / math.factorial(l + am)) * (-1.0) ** am
            pz[i, :len(p)] = N * p
            if m == 0:
                axy[i, 0, 0] = 1.0
                continue
            for j in range(am + 1):                                                              # (x + i y)^am = sum C(am, j) x^(am-j) i^j y^j
                if m > 0 and j % 2 == 0:
                    axy[i, am - j, j] = math.sqrt(2.0) * math.comb(am, j) * (-1.0) ** (j // 2)
                if m < 0 and j % 2 == 1:
                    axy[i, am - j, j] = math.sqrt(2.0) * math.comb(am, j) * (-1.0) ** ((j - 1) // 2)
    return pz, axy


def _d_first(c):
    """Coefficients of the derivative in the first exponent axis after the function index: c[i, a, ...] -> a c[i, a, ...] at a - 1."""
    out = np.zeros_like(c)
    k = np.arange(1, c.shape[1]).reshape((1, -1) + (1,) * (c.ndim - 2))
    out[:, :-1] = c[:, 1:] * k
    return out


_PZ, _AXY = _tables()
_DPZ = _d_first(_PZ)
_DAX = _d_first(_AXY)
_DAY = np.swapaxes(_d_first(np.swapaxes(_AXY, 1, 2)), 1, 2)
L_OF = np.array([int(math.isqrt(i)) for i in range(MAXDEG * MAXDEG)])                            # l of index i


def _nnz(c):
    return (c.reshape(c.shape[0], -1) != 0).sum(axis=1)


# term counts n of the expanded polynomials: value, d/dx, d/dy, d/dz -- [4, 64]
N_TERMS = np.stack([_nnz(_PZ) * _nnz(_AXY), _nnz(_PZ) * _nnz(_DAX), _nnz(_PZ) * _nnz(_DAY), _nnz(_DPZ) * _nnz(_AXY)])


def _powers(v):
    """[B] -> [B, 8]: v^0 .. v^7 by repeated multiplication (differentiable at 0, keeps (+-0)^0 = 1)."""
    p = [torch.ones_like(v)]
    for _ in range(NP - 1):
        p.append(p[-1] * v)
    return torch.stack(p, dim=1)


def _t(a, like, C2):
    return torch.as_tensor(a[:C2].reshape(C2, -1), dtype=torch.float64, device=like.device)


def _sh_eval(x64, degree, pz, axy, absolute=False):
    """[B, 3] float64 -> [B, degree^2]: (sum_k pz_k z^k) (sum_ab axy_ab x^a y^b), or the same with every monomial in absolute value."""
    C2 = degree * degree
    xp, yp, zp = _powers(x64[:, 0]), _powers(x64[:, 1]), _powers(x64[:, 2])
    xy = (xp[:, :, None] * yp[:, None, :]).reshape(-1, NP * NP)
    pz, axy = _t(pz, x64, C2), _t(axy, x64, C2)
    if absolute:
        return (zp.abs() @ pz.abs().T) * (xy.abs() @ axy.abs().T)
    return (zp @ pz.T) * (xy @ axy.T)


def sh_values(x, degree):
    """x [B, 3] (any float dtype, read exactly) -> Y [B, degree^2] float64; differentiable."""
    assert 1 <= degree <= MAXDEG
    return _sh_eval(x.double(), degree, _PZ, _AXY)


def sh_forward(x, degree, want_dy_dx=True):
    """x [B, 3] -> dict of float64 tensors: y, y_mass [B, C2];  with want_dy_dx also dy_dx, dy_dx_mass [B, 3, C2] (the layout of the ABI)
    -- dy_dx by forward-mode autograd of sh_values, the masses from the coefficient tables.  n: N_TERMS."""
    import torch.autograd.forward_ad as fwad
    x64 = x.detach().double()
    out = dict(y=sh_values(x64, degree), y_mass=_sh_eval(x64, degree, _PZ, _AXY, True))
    if want_dy_dx:
        planes = []
        for d in range(3):
            tangent = torch.zeros_like(x64)
            tangent[:, d] = 1.0
            with fwad.dual_level():
                planes.append(fwad.unpack_dual(sh_values(fwad.make_dual(x64, tangent), degree)).tangent)
        out["dy_dx"] = torch.stack(planes, dim=1)
        out["dy_dx_mass"] = torch.stack([_sh_eval(x64, degree, _PZ, _DAX, True), _sh_eval(x64, degree, _PZ, _DAY, True),
                                         _sh_eval(x64, degree, _DPZ, _AXY, True)], dim=1)
    return out


def sh_count(which, degree, device=None):
    """[C2] float64: l + 4 + n of the value (which = 0) or the partial in x, y, z (1, 2, 3)."""
    C2 = degree * degree
    return torch.as_tensor((L_OF + 4 + N_TERMS[which])[:C2], dtype=torch.float64, device=device)


def sh_bound(mass, which, degree):
    """2 (l + 4 + n) u mass, for the value (which = 0, mass [B, C2]) or one partial (1, 2, 3).  The kernel evaluates a sum of n monomials
    literal * x^a * y^b * z^c, a + b + c <= l, over cached powers, left to right:
      n - 1  additions, each rounding a partial sum that is at most the mass;
      <= l   roundings inside the cached powers: x2 = x x carries 1, x3 = x2 x 2, x4 = x2 x2 3, x5 4, x6 = x3 x3 5, x7 6 -- a power
             v^a carries a - 1, a monomial of total degree <= l at most l;
      <= 3   products literal * x^a * y^b * z^c;
      1      the literal, a rounded fp32 constant;
    l + 3 + n in all, taken as l + 4 + n.  A polynomial without monomials has mass 0 and must be returned as an exact 0."""
    return 2.0 * sh_count(which, degree, mass.device) * U * mass


def sh_dy_dx_bound(dy_dx_mass, degree):
    """[B, 3, C2]: sh_bound of the three planes."""
    return torch.stack([sh_bound(dy_dx_mass[:, d], d + 1, degree) for d in range(3)], dim=1)


def sh_backward(grad, dy_dx, g0=None):
    """grad [B, C2], dy_dx [B, 3, C2] float64 (sh_forward's), g0 [B, 3] or None -> dict: grad_inputs = g0 + sum_c grad dy_dx [B, 3]
    (the kernel ACCUMULATES into what grad_inputs holds), mass [B, 3] = |g0| + sum |grad dy_dx|."""
    g = grad.double()[:, None, :]
    gi, mass = (g * dy_dx).sum(-1), (g * dy_dx).abs().sum(-1)
    if g0 is not None:
        gi, mass = gi + g0.double(), mass + g0.double().abs()
    return dict(grad_inputs=gi, mass=mass)


def sh_backward_bound(grad, mass, dy_dx_mass, degree):
    """2 ((C2 + 1) u mass + sum_c |grad_c| bound(dy_dx_c)):  r = g0, then C2 fused multiply-adds r = fma(g, dy_dx, r), each rounding a
    partial sum that is at most mass = |g0| + sum |g dy_dx| -- the initial content enters the chain exactly and is part of every partial sum,
    which is why it is in the mass (from zeros the mass is sum |g dy_dx| alone); one more for the count's margin.  The kernel reads the fp32
    dy_dx that the forward wrote, so each term carries that value's own error, bound(dy_dx), times |g|."""
    C2 = degree * degree
    carried = (grad.double().abs()[:, None, :] * sh_dy_dx_bound(dy_dx_mass, degree)).sum(-1)
    return 2.0 * ((C2 + 1) * U * mass + carried)


# ---- frequency encoder ---------------------------------------------------------------------------------------------------------------
def freq_columns(D, deg):
    """Column layout of include/sanerf_hip.h / freq.py: [x (D) | sin 2^0 x (D) | cos 2^0 x (D) | sin 2^1 x | ...]: C = D + 2 D deg."""
    return D + 2 * D * deg


def freq_values(x, deg):
    """x [B, D] -> [B, D + 2 D deg] float64; differentiable.  x 2^f is exact in fp32 and in float64."""
    x64 = x.double()
    cols = [x64]
    for f in range(deg):
        v = x64 * float(2 ** f)
        cols += [torch.sin(v), torch.cos(v)]
    return torch.cat(cols, dim=1)


def freq_backward(x, grad, deg):
    """x [B, D], grad [B, C] -> dict: grad_inputs [B, D] by autograd of freq_values in float64;
    M = |g_x| + sum_f 2^f (|g_s cos| + |g_c sin|) and E = sum_f 2^f (|g_s| + |g_c|), both [B, D]."""
    B, D = x.shape
    x64 = x.detach().double().requires_grad_(True)
    g = grad.double()
    (gi,) = torch.autograd.grad(freq_values(x64, deg), x64, g)
    y = freq_values(x64.detach(), deg)
    M, E = g[:, :D].abs(), torch.zeros(B, D, dtype=torch.float64, device=x.device)
    for f in range(deg):
        s, c = slice(D + 2 * D * f, 2 * D + 2 * D * f), slice(2 * D + 2 * D * f, 3 * D + 2 * D * f)
        M = M + 2.0 ** f * ((g[:, s] * y[:, c]).abs() + (g[:, c] * y[:, s]).abs())
        E = E + 2.0 ** f * (g[:, s].abs() + g[:, c].abs())
    return dict(grad_inputs=gi, M=M, E=E)


def freq_backward_bound(M, E, deg, eps_fwd):
    """2 ((deg + 3) u M + eps_fwd E).  The kernel computes r = g_x; r += 2^f (g_s o_c - g_c o_s) per frequency from the fp32 outputs o:
    two products (one rounding each, relative to their own term), the difference (one rounding, at most the two terms' mass), the factor
    2^f (exact), and deg additions that round a partial sum of at most M: deg + 2, taken as deg + 3.  Each output it reads is within
    eps_fwd of the true sine / cosine, and enters with the weight 2^f |g|: eps_fwd E."""
    return 2.0 * ((deg + 3) * U * M + eps_fwd * E)


# ---- per-ray head and composite ----------------------------------------------------------------------------------------------------
def sum_bound(T, mass):
    """2 (T + 1) u sum |w v|: a chain of T fused multiply-adds (or T additions) from zero, each rounding a partial sum of at most the mass."""
    return 2.0 * (T + 1) * U * mass


def product_bound(exact):
    """u |w g|: one correctly rounded fp32 product (no margin needed: that is what IEEE rounding gives; exactly 0 where a factor is 0)."""
    return U * exact.abs()


def composite(w, v):
    """w [N, T], v [N, T, K] -> dict: out = sum_t w v [N, K] float64 (differentiable), mass = sum_t |w v|."""
    p = w.double()[:, :, None] * v.double()
    return dict(out=p.sum(1), mass=p.detach().abs().sum(1))


def composite_grads(w, v, g):
    """Autograd gradients of sum(composite * g) in float64: dict g_weights [N, T] with its mass sum_k |v g|, g_values [N, T, K]."""
    w64, v64 = w.detach().double().requires_grad_(True), v.detach().double().requires_grad_(True)
    gw, gv = torch.autograd.grad(composite(w64, v64)["out"], (w64, v64), g.double())
    return dict(g_weights=gw, g_weights_mass=(v64.detach() * g.double()[:, None, :]).abs().sum(-1), g_values=gv)


def head_direction(d):
    """[N, 3] -> d / |d| in float64."""
    d64 = d.double()
    return d64 / d64.pow(2).sum(-1, keepdim=True).sqrt()


def head_forward(w, t, raw, d):
    """weights [N, T], rays_t [N, T], raw [N, T, 16], rays_d [N, 3] (unnormalised) -> dict, all float64 and differentiable in w and raw:
    ws = sum w [N];  depth = sum w t [N];  f [N, 31]: f[:, 0:15] = sum w raw[..., 1:16], f[:, 15:31] = SH4(d / |d|) ws."""
    w64, raw64 = w.double(), raw.double()
    ws = w64.sum(-1)
    sh = sh_values(head_direction(d.detach()), 4)
    return dict(ws=ws, depth=(w64 * t.double()).sum(-1), f=torch.cat([(w64[:, :, None] * raw64[..., 1:]).sum(1), sh * ws[:, None]], dim=-1), sh=sh)


def head_masses(w, t, raw):
    w64 = w.detach().double()
    return dict(ws=w64.abs().sum(-1), depth=(w64 * t.double()).abs().sum(-1), f=(w64[:, :, None] * raw.detach().double()[..., 1:]).abs().sum(1))


def head_sh_bound(d):
    """[N, 16] bound on the kernel's fp32 SH4 of its own fp32-normalised direction against sh_values(d / |d|, 4):
    the sh_bound at the fp64-normalised direction, widened by 2 * 4 u sum_i |x_i| mass(d_i Y).  The kernel normalises in fp32: three squares
    and two additions (3 u relative on the sum of non-negative terms, halved by the root), the square root, the reciprocal and the product:
    each component is within 4 u |x_i| of the exact one, which moves Y by at most |x_i| |d_i Y| <= |x_i| mass(d_i Y) times that."""
    fw = sh_forward(head_direction(d), 4)
    xn = head_direction(d).abs()
    return sh_bound(fw["y_mass"], 0, 4) + 2.0 * 4 * U * (xn[:, :, None] * fw["dy_dx_mass"]).sum(1)


def head_f_sh_bound(d, sh, ws, ws_mass, T):
    """[N, 16] bound on f[:, 15:31] = Y ws:  |ws| bound(Y) + |Y| bound(ws) + u |Y ws| (the product)."""
    return ws.abs()[:, None] * head_sh_bound(d) + sh.abs() * sum_bound(T, ws_mass)[:, None] + U * (sh * ws[:, None]).abs()


def head_backward(w, t, raw, d, g_ws, g_depth, g_f):
    """Autograd gradients of the head in float64 for the output gradients that are not None -> dict:
    g_weights [N, T], g_raw [N, T, 16], terms [N, T] = sum of the absolute values of the (at most 33) terms of g_weights,
    sh_carried [N] = sum_k |g_f[15 + k]| bound(Y_k) with the head's widened SH bound."""
    w64, raw64 = w.detach().double().requires_grad_(True), raw.detach().double().requires_grad_(True)
    fw = head_forward(w64, t, raw64, d)
    N, T = w.shape
    loss = torch.zeros((), dtype=torch.float64, device=w.device)
    terms = torch.zeros(N, T, dtype=torch.float64, device=w.device)
    carried = torch.zeros(N, dtype=torch.float64, device=w.device)
    if g_ws is not None:
        loss = loss + (fw["ws"] * g_ws.double()).sum()
        terms = terms + g_ws.double().abs()[:, None]
    if g_depth is not None:
        loss = loss + (fw["depth"] * g_depth.double()).sum()
        terms = terms + (g_depth.double()[:, None] * t.double()).abs()
    if g_f is not None:
        gf = g_f.double()
        loss = loss + (fw["f"] * gf).sum()
        terms = terms + (gf[:, None, :15] * raw64.detach()[..., 1:]).abs().sum(-1) + (gf[:, 15:] * fw["sh"].detach()).abs().sum(-1)[:, None]
        carried = (gf[:, 15:].abs() * head_sh_bound(d)).sum(-1)
    if loss.requires_grad:
        gw, gr = torch.autograd.grad(loss, (w64, raw64), allow_unused=True)
    else:
        gw = gr = None
    gw = torch.zeros_like(w64) if gw is None else gw
    gr = torch.zeros_like(raw64) if gr is None else gr
    return dict(g_weights=gw, g_raw=gr, terms=terms, sh_carried=carried)


def head_gw_bound(terms, sh_carried):
    """2 (34 u sum |terms| + sum_k |g_f[15 + k]| bound(Y_k)): the kernel builds g_weights as one chain of 33 terms -- g_wsum, 16 fused
    multiply-adds with the SH values, 15 with the raw channels, 1 with g_depth t -- each rounding a partial sum of at most the terms' mass:
    33, taken as 34; the SH values it multiplies are its own fp32 ones."""
    return 2.0 * (34 * U * terms + sh_carried[:, None])


# ---- placed points -------------------------------------------------------------------------------------------------------------------
def placed_points():
    """[P, 3] float32: the six axis directions, points with exactly representable structure, the origin, a point far off the sphere, -0.0
    components, and points in the planes x = 0, y = 0, z = 0 where whole polynomials vanish."""
    s = math.sqrt(0.5)
    pts = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
           [0.6, 0.8, 0], [0, 0.6, -0.8], [1e-4, 0, 1], [0, 0, 0], [2, -1.5, 0.5],
           [-0.0, 1, 0], [1, -0.0, -0.0], [-0.0, -0.0, 1], [-0.0, -0.0, -0.0],
           [0, s, s], [0, -0.3, 0.7], [0, 1.5, -0.25],                                            # x = 0
           [s, 0, -s], [0.3, 0, 0.9], [-1.25, 0, 0.5],                                            # y = 0
           [s, s, 0], [-0.28, 0.96, 0], [1.75, -0.5, 0]]                                          # z = 0
    return torch.tensor(pts, dtype=torch.float32)


def sh_points(B, seed, device=None):
    """[B, 3] float32: the placed points (as many as fit), then random unit vectors and vectors of radius 0.25 .. 2, half and half."""
    gen = torch.Generator().manual_seed(seed)
    placed = placed_points()[:B]
    n = B - placed.shape[0]
    v = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True)
    r = torch.ones(n, 1, dtype=torch.float64)
    r[n // 2:] = 0.25 + 1.75 * torch.rand(n - n // 2, 1, generator=gen, dtype=torch.float64)
    return torch.cat([placed, (v * r).float()]).to(device)
