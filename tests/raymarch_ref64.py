"""Plain numpy fp64 references of the stand-alone ray operators (raymarch.hip), with the condition scale of every output element.

Each function restates the lines of nerf/renderer.py it names on the fp32 inputs promoted to fp64 (the program's own fp32 constants,
0.01f and 1e-8f, promoted likewise); nothing here calls a kernel, the oracle or torch.  The `scale` of an element is a first-order bound
on what fp32 rounding of the same formula may move, in units of the fp32 unit round-off 2^-24: a kernel element is held to

    |got - ref| <= K * 2^-24 * scale + 2^-149

with one measured constant K per operator (raymarch_cases.py).  A scale of 0 asks for the exact value (up to one subnormal step).
"""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -149
F = np.float64
PAD = F(np.float32(0.01))        # renderer.py:91 in an fp32 program
DEN = F(np.float32(1e-8))        # renderer.py:49


def _quiet():
    return np.errstate(all="ignore")


def _mul0(a, b):
    """a * b with 0 * inf = 0: a factor that is exactly zero has no rounding to propagate."""
    with _quiet():
        return np.where((a == 0) | (b == 0), 0.0, a * b)


# ---------------------------------------------------------------------------------------------------------------------
# renderer.py:308-325 and its derivative w.r.t. sigma
# ---------------------------------------------------------------------------------------------------------------------
def weights(real_bins, sigmas, last_opaque, grad=None):
    """-> dict(w, c, ds, delta, T, scale_w [, gs, scale_gs]).  c is the exclusive running optical depth, ds the per-sample depth (the
    opaque last sample's is +inf).  The gradient follows the operator's statement: dL/dsigma_i = delta_i (g_i e^{-ds_i} T_i -
    sum_{j>i} g_j w_j); the opaque last sample is a constant; a NaN weight (nan_to_num -> 0) passes nothing."""
    rb, sg = np.asarray(real_bins, F), np.asarray(sigmas, F)
    with _quiet():
        delta = rb[:, 1:] - rb[:, :-1]
        ds = delta * sg
        if last_opaque:
            ds = np.concatenate([ds[:, :-1], np.full_like(ds[:, -1:], np.inf)], axis=1)
        c = np.concatenate([np.zeros_like(ds[:, :1]), np.cumsum(ds[:, :-1], axis=1)], axis=1)
        e = np.exp(-ds)
        tr = np.exp(-c)
        raw = (1.0 - e) * tr
        bad = np.isnan(raw)
        w = np.where(bad, 0.0, raw)
        scale_w = np.where(bad, 0.0, 2.0 * tr + _mul0(w, 2.0 + c))
    out = dict(w=w, c=c, ds=ds, delta=delta, T=tr, bad=bad, scale_w=scale_w)
    if grad is not None:
        g = np.asarray(grad, F)
        with _quiet():
            gw = np.where(bad, 0.0, g * w)
            # below 2^-126 an fp32 intermediate rounds by an absolute 2^-150, not by a relative 2^-24: e^-c, e^-ds e^-c, w and their products
            # with g count as 2^-126 (times 1 + |g|) where they are smaller than that and not exactly zero; larger ones enter as they are.
            # The bar's own 2^-149 covers this for the forward weights; here the intermediates are still multiplied by g and delta.
            sub = lambda x: np.where((x != 0) & (np.abs(x) < 2.0 ** -126), 2.0 ** -126, 0.0)      # noqa: E731
            agw = np.where(bad, 0.0, _mul0(np.abs(g) * w + (np.abs(g) + 1.0) * sub(w), 1.0 + c))
            shift = lambda a: np.concatenate([a[:, 1:], np.zeros_like(a[:, :1])], axis=1)      # noqa: E731
            after = shift(np.cumsum(gw[:, ::-1], axis=1)[:, ::-1])                  # sum over j > i, summed from the far end (no cancellation)
            aafter = shift(np.cumsum(agw[:, ::-1], axis=1)[:, ::-1])
            et = _mul0(e, tr)
            dterm = np.where(bad, 0.0, g * et)
            adterm = np.where(bad, 0.0, _mul0(np.abs(g) * et + (np.abs(g) + 1.0) * sub(et), 1.0 + c + ds))
            const = np.zeros_like(bad)
            if last_opaque:
                const[:, -1] = True
            gs = np.where(const, 0.0, _mul0(delta, dterm - after))
            scale_gs = np.where(const, 0.0, _mul0(np.abs(delta), adterm + aafter))
        out.update(gs=gs, scale_gs=scale_gs)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# renderer.py:84-119
# ---------------------------------------------------------------------------------------------------------------------
def linspace_u(T):
    """renderer.py:97 in fp64."""
    return np.linspace(0.5 / T, 1 - 0.5 / T, T, dtype=F)


def sample_pdf(bins, weights_, u, near=16.0 * EPS):
    """u: [T] or [N,T].  -> dict(cdf, inds, out, scale, knot_gap).  knot_gap[n,j] is the distance from u to the nearest cdf knot next to
    its interval (the only place an fp32 searchsorted may differ).  Where u lies within `near` of a knot the scale takes the steeper of
    the two adjoining intervals: either side's line is a valid answer there."""
    b, w = np.asarray(bins, F), np.asarray(weights_, F)
    N, T0 = w.shape
    u = np.broadcast_to(np.asarray(u, F), (N, np.shape(u)[-1]))
    with _quiet():
        wp = w + PAD
        pdf = wp / wp.sum(axis=1, keepdims=True)
        cdf = np.minimum(np.cumsum(pdf, axis=1), 1.0)
        cdf = np.concatenate([np.zeros_like(cdf[:, :1]), cdf], axis=1)
        inds = np.stack([np.searchsorted(cdf[n], u[n], side="right") for n in range(N)])
        below, above = np.clip(inds - 1, 0, T0), np.clip(inds, 0, T0)
        take = lambda a, i: np.take_along_axis(a, i, axis=1)      # noqa: E731
        c0, c1, b0, b1 = take(cdf, below), take(cdf, above), take(b, below), take(b, above)
        t = np.clip(np.nan_to_num((u - c0) / (c1 - c0), nan=0.0, posinf=np.finfo(np.float32).max, neginf=-np.finfo(np.float32).max), 0.0, 1.0)
        out = b0 + t * (b1 - b0)
        slope_all = np.where(np.diff(cdf, axis=1) > 0, np.diff(b, axis=1) / np.diff(cdf, axis=1), 0.0)      # [N,T0]
        iv = np.clip(inds - 1, 0, T0 - 1)                         # interval of the sample
        slope = np.where(c1 > c0, take(slope_all, iv), 0.0)
        lo_gap, hi_gap = np.abs(u - c0), np.abs(c1 - u)
        left = np.where(lo_gap <= near, take(slope_all, np.clip(iv - 1, 0, T0 - 1)), 0.0)
        right = np.where(hi_gap <= near, take(slope_all, np.clip(iv + 1, 0, T0 - 1)), 0.0)
        steep = np.maximum(slope, np.maximum(left, right))
        scale = steep * np.maximum(c1, u) + np.maximum(np.abs(b0), np.abs(b1))
        knot_gap = np.minimum(lo_gap, hi_gap)
    return dict(cdf=cdf, inds=inds, out=out, scale=scale, knot_gap=knot_gap, below_gap=lo_gap, above_gap=hi_gap)


# ---------------------------------------------------------------------------------------------------------------------
# renderer.py:249-252, 277-285, 60-69 and gridencoder/grid.py:156
# ---------------------------------------------------------------------------------------------------------------------
def spacing(x):
    x = np.asarray(x, F)
    with _quiet():
        return np.where(x < 1, x / 2, 1 - 1 / (2 * x))


def spacing_inv(x):
    x = np.asarray(x, F)
    with _quiet():
        return np.where(x < 0.5, 2 * x, 1 / (2 - 2 * x))


def contract(p):
    """renderer.py:60-69 on [..., 3]; -> z."""
    p = np.asarray(p, F)
    mag = np.abs(p).max(axis=-1, keepdims=True)
    idx = np.abs(p).argmax(axis=-1)[..., None]
    with _quiet():
        sc = np.repeat(1 / mag, 3, axis=-1)
        np.put_along_axis(sc, idx, (2 - 1 / mag) / mag, axis=-1)
        return np.where(mag < 1, p, p * sc)


def sample_positions(rays_o, rays_d, nears, fars, bins, contract_=True, grid_bound=0.0):
    """-> dict(real_bins, rays_t, xyzs, scale_rb, scale_t, scale_x).  The scale of real_bins is r + spacing_inv'(x) (|a| + |c|) with
    a = s_near (1 - b), c = s_far b, x = a + c; it goes through o + d t term by term, through the contraction with its Lipschitz constant
    2 in the max norm, and through (z + B) / (2 B)."""
    o, d, b = np.asarray(rays_o, F), np.asarray(rays_d, F), np.asarray(bins, F)
    near, far = np.asarray(nears, F).reshape(-1, 1), np.asarray(fars, F).reshape(-1, 1)
    with _quiet():
        sn, sf = spacing(near), spacing(far)
        a, c = sn * (1 - b), sf * b
        x = a + c
        r = spacing_inv(x)
        dinv = np.where(x < 0.5, 2.0, 2.0 * r * r)
        scale_rb = np.abs(r) + dinv * (np.abs(a) + np.abs(c))
        t = (r[:, 1:] + r[:, :-1]) / 2
        scale_t = (scale_rb[:, 1:] + scale_rb[:, :-1]) / 2 + np.abs(t)
        p = o[:, None, :] + d[:, None, :] * t[:, :, None]
        scale_x = np.abs(d)[:, None, :] * scale_t[:, :, None] + np.abs(d[:, None, :] * t[:, :, None]) + np.abs(p)
        if contract_:
            z = contract(p)
            scale_x = 2.0 * scale_x.max(axis=-1, keepdims=True) + 3.0 * np.abs(z) + 0.0 * scale_x
            p = z
        if grid_bound > 0:
            q = (p + grid_bound) / (2 * grid_bound)
            scale_x = (scale_x + np.abs(p) + grid_bound) / (2 * grid_bound) + np.abs(q)
            p = q
    return dict(real_bins=r, rays_t=t, xyzs=p, scale_rb=scale_rb, scale_t=scale_t, scale_x=scale_x)


# ---------------------------------------------------------------------------------------------------------------------
# renderer.py:333-338, 361, 384
# ---------------------------------------------------------------------------------------------------------------------
def composite(weights_, values, grad_out):
    """values [N,T,K], grad_out [N,K] -> dict(out, gw, gv and their scales): out = sum_t w v, d/dw = sum_k v g, d/dv = w g."""
    w, v, g = np.asarray(weights_, F), np.asarray(values, F), np.asarray(grad_out, F)
    out = (w[:, :, None] * v).sum(axis=1)
    gw = (v * g[:, None, :]).sum(axis=2)
    gv = w[:, :, None] * g[:, None, :]
    return dict(out=out, gw=gw, gv=gv, scale_out=np.abs(w[:, :, None] * v).sum(axis=1), scale_gw=np.abs(v * g[:, None, :]).sum(axis=2),
                scale_gv=np.abs(gv))


# ---------------------------------------------------------------------------------------------------------------------
# renderer.py:30-57, one proposal stage
# ---------------------------------------------------------------------------------------------------------------------
def proposal_loss_stage(bins, weights_, ref_bins, ref_weights):
    """-> dict(per_ray, gw, lo, hi, scale_per_ray, scale_gw): per_ray[n] = sum_j max(rw_j - bound_j, 0)^2 / (rw_j + 1e-8) (the mean is
    per_ray.sum() / (N Tr)) and gw = d per_ray / d w.  term_j moves by |d term / d bound| times the rounding of rw - (cum[hi+1] - cum[lo]);
    g_j = d term_j / d bound_j moves by |d g / d bound| = 2 / (rw + 1e-8) times the same, plus its own rounding."""
    b, w, rb, rw = (np.asarray(a, F) for a in (bins, weights_, ref_bins, ref_weights))
    N, T = w.shape
    Tr = rw.shape[1]
    cum = np.concatenate([np.zeros((N, 1)), np.cumsum(w, axis=1)], axis=1)
    lo = np.stack([np.searchsorted(b[n, :-1], rb[n, :-1], side="right") - 1 for n in range(N)]).clip(0, T - 1)
    hi = np.stack([np.searchsorted(b[n, 1:], rb[n, 1:], side="right") for n in range(N)]).clip(0, T - 1)
    chi, clo = np.take_along_axis(cum, hi + 1, axis=1), np.take_along_axis(cum, lo, axis=1)
    d = np.maximum(rw - (chi - clo), 0.0)
    den = rw + DEN
    term = d * d / den
    g = -2.0 * d / den
    moved = np.abs(rw) + np.abs(chi) + np.abs(clo)
    scale_g = np.where(d > 0, 2.0 * moved / den, 0.0) + np.abs(g)
    # a final-stage interval whose rw - bound sits within fp32 rounding of the clamp may switch on or off: |g| there is at most
    # 2 * (that rounding) / (rw + 1e-8)
    edge = np.abs(rw - (chi - clo)) <= 8 * EPS * moved
    scale_g = np.where(edge, 2.0 * moved / den + np.abs(g), scale_g)
    scale_term = moved * np.where(edge, np.maximum(np.abs(g), 16 * EPS * moved / den), np.abs(g)) + term
    gw, scale_gw = np.zeros((N, T)), np.zeros((N, T))
    i = np.arange(T)
    for n in range(N):                                       # w_i is in bound_j for lo_j <= i <= hi_j: summed term by term (no prefix differences)
        inside = (lo[n][:, None] <= i) & (i <= hi[n][:, None])
        gw[n] = (inside * g[n][:, None]).sum(axis=0)
        scale_gw[n] = (inside * scale_g[n][:, None]).sum(axis=0)
    return dict(per_ray=term.sum(axis=1), gw=gw, lo=lo, hi=hi, scale_per_ray=scale_term.sum(axis=1), scale_gw=scale_gw)
