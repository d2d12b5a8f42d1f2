"""Cases and fp32 statements shared by tests/test_encoders_ref64.py (CPU) and tests/test_gpu_encoders.py (MI355X).

The fp32 statements restate the TEXT of the kernels in numpy float32 -- the generated polynomials of sanerf-hq_amd/csrc/sh_basis.inc parsed
into the same cached powers and left-to-right sums, k_sh_backward, k_freq_forward / k_freq_backward, k_ray_composite[_backward] -- so
that the CPU tests can show that the arithmetic alone stays inside the bounds of encoders_ref64.py before a kernel is held to them.
A fused multiply-add is emulated in float64: the product of two fp32 numbers is exact there, the sum is rounded to float64 and then to fp32.
"""
import os
import re

import numpy as np
import torch

import encoders_ref64 as R
from grid_ref64 import worst_ratio as R_worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH_INC = os.path.join(ROOT, "sanerf-hq_amd", "csrc", "sh_basis.inc")
MACROS = ("SN_SH_VALUES", "SN_SH_DX", "SN_SH_DY", "SN_SH_DZ")
F32 = np.float32

# (D, deg) of the frequency encoder: the product's (3, 10 / 6 / 4), other widths, a single frequency, twelve, and none
FREQ_CASES = [(3, 10), (3, 6), (3, 4), (1, 1), (2, 6), (5, 4), (4, 12), (3, 0)]
HEAD_SHAPES = [(1, 1), (15, 7), (16, 33), (17, 64), (130, 300), (4099, 32)]


# ---- sh_basis.inc as numpy float32 ---------------------------------------------------------------------------------------------------
def parse_sh_inc(path=SH_INC):
    """{macro: 64 lists of (literal as a Python float, (a, b, c))} in the order of the text; `0.0f` is an empty list."""
    out, cur = {}, None
    term = re.compile(r"^(-?[0-9.]+(?:e-?[0-9]+)?)f((?:\*[xyz][2-7]?)*)$")
    for line in open(path):
        m = re.match(r"#define (SN_SH_\w+)\(o\)", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"\s*o\[(\d+)\] = (.*); \\", line)
        if not m or cur is None:
            continue
        assert int(m.group(1)) == len(cur), line
        terms = []
        for tok in m.group(2).replace(" - ", " + -").split(" + "):
            t = term.match(tok)
            assert t, (tok, line)
            e = {"x": 0, "y": 0, "z": 0}
            for fac in t.group(2).split("*")[1:]:
                assert e[fac[0]] == 0, tok
                e[fac[0]] = int(fac[1:] or 1)
            terms.append((float(t.group(1)), (e["x"], e["y"], e["z"])))
        cur.append([] if terms == [(0.0, (0, 0, 0))] else terms)
    assert tuple(out) == MACROS and all(len(v) == 64 for v in out.values())
    return out


def powers32(v):
    """SN_SH_POWERS: v2 = v v, v3 = v2 v, v4 = v2 v2, v5 = v4 v, v6 = v3 v3, v7 = v6 v in fp32; index = exponent (0 unused)."""
    v = v.astype(F32)
    v2 = v * v; v3 = v2 * v; v4 = v2 * v2; v5 = v4 * v; v6 = v3 * v3; v7 = v6 * v
    return [None, v, v2, v3, v4, v5, v6, v7]


def eval_terms32(terms, pw, scale=None):
    """One polynomial of the text: ((literal * x^a) * y^b) * z^c per monomial, summed left to right, all in fp32.
    scale = (j, factor): the j-th literal is multiplied by factor (in float64) before it is rounded to fp32."""
    B = pw[0][1].shape[0]
    acc = None
    for j, (lit, mon) in enumerate(terms):
        if scale is not None and scale[0] == j:
            lit = lit * scale[1]
        t = np.full(B, F32(lit), dtype=F32)
        for axis, e in enumerate(mon):
            if e:
                t = t * pw[axis][e]
        acc = t if acc is None else acc + t
    return np.zeros(B, F32) if acc is None else acc


def sh_text32(parsed, pts, degree, want_dy_dx=True):
    """The text of k_sh_forward on pts [B, 3] float32 -> y [B, C2], dy_dx [B, 3, C2] (float32)."""
    pw = [powers32(pts[:, a]) for a in range(3)]
    C2 = degree * degree
    y = np.stack([eval_terms32(parsed["SN_SH_VALUES"][i], pw) for i in range(C2)], axis=1)
    if not want_dy_dx:
        return y, None
    dd = np.stack([np.stack([eval_terms32(parsed[m][i], pw) for i in range(C2)], axis=1) for m in MACROS[1:]], axis=1)
    return y, dd


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def sh_backward_text32(grad, dy_dx, g0):
    """k_sh_backward: r = grad_inputs; r = fmaf(g[ch], dy_dx[ch], r) over the channels."""
    r = g0.astype(F32).copy()
    for ch in range(grad.shape[1]):
        r = fma32(grad[:, None, ch], dy_dx[:, :, ch], r)
    return r


def freq_forward_text32(x, deg):
    """k_freq_forward with the host's fp32 sin / cos."""
    cols = [x.astype(F32)]
    for f in range(deg):
        v = np.ldexp(x.astype(F32), f).astype(F32)
        cols += [np.sin(v), np.cos(v)]
    return np.concatenate(cols, axis=1).astype(F32)


def freq_backward_text32(grad, outputs, D, deg, cos_sign=1.0):
    """k_freq_backward: r = g_x; r += 2^f * (g_s * o_c - g_c * o_s)."""
    g, o = grad.astype(F32), outputs.astype(F32)
    r = g[:, :D].copy()
    for f in range(deg):
        s, c = slice(D + 2 * D * f, 2 * D + 2 * D * f), slice(2 * D + 2 * D * f, 3 * D + 2 * D * f)
        r = r + F32(2.0 ** f) * (F32(cos_sign) * (g[:, s] * o[:, c]) - g[:, c] * o[:, s])
    return r


def head_forward_text32(parsed, w, t, raw, d):
    """k_ray_composite: ws by additions, depth and the 15 feature channels by fmaf chains, SH4 of the fp32-normalised direction times ws."""
    N, T = w.shape
    ws, depth, f = np.zeros(N, F32), np.zeros(N, F32), np.zeros((N, 15), F32)
    for j in range(T):
        ws = ws + w[:, j]
        depth = fma32(w[:, j], t[:, j], depth)
        f = fma32(w[:, j, None], raw[:, j, 1:], f)
    sh = head_sh_text32(parsed, d)
    return ws, depth, np.concatenate([f, sh * ws[:, None]], axis=1)


def head_sh_text32(parsed, d):
    x, y, z = d[:, 0].astype(F32), d[:, 1].astype(F32), d[:, 2].astype(F32)
    inv = F32(1.0) / np.sqrt(x * x + y * y + z * z)
    return sh_text32(parsed, np.stack([x * inv, y * inv, z * inv], axis=1), 4, False)[0]


def head_backward_text32(parsed, w, t, raw, d, g_ws, g_depth, g_f):
    """k_ray_composite_backward with its three optional gradients (None = NULL)."""
    N, T = w.shape
    sh = head_sh_text32(parsed, d)
    k_ray = g_ws.astype(F32).copy() if g_ws is not None else np.zeros(N, F32)
    if g_f is not None:
        for k in range(16):
            k_ray = fma32(g_f[:, 15 + k], sh[:, k], k_ray)
    gw = np.repeat(k_ray[:, None], T, axis=1)
    go = np.zeros((N, T, 16), F32)
    for c in range(15):
        g = g_f[:, c] if g_f is not None else np.zeros(N, F32)
        gw = fma32(g[:, None], raw[:, :, 1 + c], gw)
        go[:, :, 1 + c] = w * g[:, None]
    if g_depth is not None:
        gw = fma32(g_depth[:, None], t, gw)
    return gw, go


# ---- the head against the statement ----------------------------------------------------------------------------------------------------
def head_checks(got, w, t, raw, d, grads):
    """(worst ratio, exact) per quantity of a head implementation got = dict(ws, depth, f, g_weights, g_raw) against the statement;
    grads = (g_ws, g_depth, g_f) with None for an absent one. """
    N, T = w.shape
    fw, m = R.head_forward(w, t, raw, d), R.head_masses(w, t, raw)
    bw = R.head_backward(w, t, raw, d, *grads)
    out = {}
    if "ws" in got:
        out["ws"] = R_worst_ratio(got["ws"], fw["ws"], R.sum_bound(T, m["ws"]))
        out["depth"] = R_worst_ratio(got["depth"], fw["depth"], R.sum_bound(T, m["depth"]))
        out["f"] = R_worst_ratio(got["f"][:, :15], fw["f"][:, :15], R.sum_bound(T, m["f"]))
        out["f_sh"] = R_worst_ratio(got["f"][:, 15:], fw["f"][:, 15:], R.head_f_sh_bound(d, fw["sh"], fw["ws"], m["ws"], T))
    if "g_weights" in got:
        out["g_weights"] = R_worst_ratio(got["g_weights"], bw["g_weights"], R.head_gw_bound(bw["terms"], bw["sh_carried"]))
        out["g_raw"] = R_worst_ratio(got["g_raw"], bw["g_raw"], R.product_bound(bw["g_raw"]))
    return out


GRAD_SETS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def sensitivity_points():
    """A few thousand points for the literal-by-literal loop: the placed points, random unit and off-sphere vectors, and points where single
    monomials dominate -- a small radius for the low-order terms, a large one for the high-order terms, directions near an axis and near a
    coordinate plane for the mixed terms."""
    gen = torch.Generator().manual_seed(77)
    base = R.sh_points(2048, 5).double()
    v = torch.randn(2560, 3, generator=gen, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True)
    extra = [v[:256] * 0.02, v[256:512] * 0.1, v[512:768] * 2.0, v[768:1024] * 3.0]
    for a in range(3):                                                                           # near the axis a, and near the plane a = 0
        near = v[1024 + 256 * a:1280 + 256 * a].clone()
        near[:, [b for b in range(3) if b != a]] *= 0.05
        extra.append(near / near.norm(dim=1, keepdim=True) * 1.5)
        flat = v[1792 + 256 * a:2048 + 256 * a].clone()
        flat[:, a] *= 0.03
        extra.append(flat / flat.norm(dim=1, keepdim=True) * 1.5)
    return torch.cat([base] + extra).float()


def freq_inputs(B, D, rng_range, seed, device=None):
    """[B, D] float32 in +-rng_range with 0, -0.0 and exact powers of two placed in the first rows."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, D, generator=gen, dtype=torch.float64) * 2 - 1) * rng_range
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -10, -(2.0 ** -24), 2.0, -4.0, 0.25], dtype=torch.float64)
    special = special[special.abs() <= rng_range]
    k = min(B * D, special.numel())
    x.view(-1)[:k] = special[:k]
    return x.float().to(device)


def head_inputs(N, T, seed, zero_weights=False, device=None):
    """weights that sum to 1 per ray (or zeros), mid-points in [0, 5), raw ~ N(0, 1), unnormalised directions with |d| from 1e-3 to 1e3, the
    first rays along the axes; the three output gradients."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.rand(N, T, generator=gen, dtype=torch.float64)
    w = torch.zeros(N, T) if zero_weights else (w / w.sum(-1, keepdim=True)).float()
    t = (torch.rand(N, T, generator=gen) * 5).float()
    raw = torch.randn(N, T, 16, generator=gen)
    d = torch.randn(N, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True) * 10.0 ** (torch.rand(N, 1, generator=gen, dtype=torch.float64) * 6 - 3)
    axes = torch.tensor([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1e-3, 0, 0], [0, 1e3, 0], [0, 0, -2]], dtype=torch.float64)
    k = min(N - 1, axes.shape[0]) if N > 1 else 0                                                # keep at least one random direction
    d[:k] = axes[:k]
    g = (torch.randn(N, generator=gen), torch.randn(N, generator=gen), torch.randn(N, 31, generator=gen))
    return tuple(v.float().to(device) for v in (w, t, raw, d.float()) + g)
