"""One Adam step, for the tests: the fp64 statement, the fp32 restatement of the kernel, the round-off budget between the two, the
element table and hyper-parameter table they are held to, and the planted defects the budget was built to catch.

Written for the tests alone: nothing here imports the package.

  step64   one step of torch's _single_tensor_adam (torch/optim/adam.py) in float64, in torch ops, on any device:
               g = -g if maximize;  g += wd p;  m' = m + (1-b1)(g - m);  v' = b2 v + (1-b2) g^2
               denom = sqrt(v') / sqrt(1 - b2^t) + eps;  p' = p - lr / (1 - b1^t) m' / denom
           with the kernel's fp32 inputs widened and every scalar a Python double.  `lazy` (include/sanerf_hip.h, SN_ADAM_LAZY):
           elements with g == 0 keep p, m and v.  `lr_scale`: the rate is lr * float64(float32(lr_scale)), as k_adam_multi forms it.
  step32   the same step as adam_one of csrc/optim.hip writes it, operation for operation in NumPy float32: what the kernel must give
           to the bit where the host forms the scalars (the library is built with -ffp-contract=off,
           -fhip-fp32-correctly-rounded-divide-sqrt and -fno-gpu-flush-denormals-to-zero, so every operation below is one IEEE
           rounding on the device as well).
  budget   per element, how far a correct fp32 evaluation may be from step64 -- derived below, not tuned.
  cases    the element table: every regime in one array.
  HYPERS   the hyper-parameter rows;  CANCEL_HYPERS two more, at which the decayed gradient of the table's last elements is exactly 0.
  MUTANTS  step32 with one defect planted at a time.

The budget (u = 2^-24, the unit round-off of fp32; first order in u; x^ is the fp32 value of x).  Inputs are exact.  A scalar that
the host rounds to fp32 (wd, 1-b1, b2, 1-b2, lr/bc1, 1/sqrt(bc2), eps) is off by u relative, counted where the scalar is used.

  g_eff   wd = 0: exact (a negation).  Else fl(g + fl(wd^ p)): u wd|p| for wd^, u wd|p| for the product, u |g_eff| for the sum
              t_g = u (|g_eff| + 2 wd |p|)
  m'      fl(m + fl(c1^ fl(g^ - m))): the difference inherits t_g and rounds once (u |g_eff - m|); c1^ and the product are 2 u more on
          (1-b1)|g_eff - m|; the sum rounds to u |m'|.  The bound is in the size of the TERMS: g - m cancels, so nothing relative to |m'|
          can hold.
              t_m = u (3 (1-b1) |g_eff - m| + |m'|) + (1-b1) t_g
  v'      fl(fl(v b2^) + fl(c2^ fl(g^ g^))): the square carries 2 |g_eff| t_g and rounds once, c2^ and its product 2 u more: 3 u on
          (1-b2) g_eff^2; b2^ and its product 2 u on b2 v; the sum u v'.  (All terms are >= 0: this is <= 4 u v'.)
              t_v = u (3 (1-b2) g_eff^2 + 2 b2 v + v') + 2 (1-b2) |g_eff| t_g
  denom   fl(fl(sqrtf(v'^) ibs^) + eps^), s = sqrt(v') / sqrt(bc2): the root rounds once (correctly rounded: u), ibs^ and the product
          2 u more on s; eps^ is u eps; the sum u denom.  The root passes t_v on as t_v / (2 sqrt(v')).
              t_den = u (3 s + eps + denom) + t_v / (2 sqrt(v') sqrt(bc2))          (<= 4 u denom + ...)
  p'      fl(p - fl(ss^ fl(m'^ / denom^))), D = p - p' = lr/bc1 m'/denom: the quotient inherits t_m / denom and |m'/denom| t_den /
          denom and rounds once, ss^ and the product 2 u more: 3 u |D|; the difference u |p'|.
              t_p = u (|p'| + 3 |D|) + lr/bc1 t_m / denom + |D| t_den / denom

Underflow.  A product or quotient whose result is below 2^-126 is rounded to a multiple of the smallest denormal d = 2^-149: an
ABSOLUTE error of up to d/2 that no relative term covers (sums and differences of fp32 numbers are exact down there, and sqrtf of a
denormal is a normal number).  Counted per operation: wd^ p (d/2 into t_g); c1^ (g - m) (d/2 into t_m); g g, c2^ (g g), v b2^
(3 d/2 into t_v, call it a_v); m'/denom and ss^ times it (d/2 each into t_p, the first scaled by lr/bc1).  In denom the absolute
part of t_v does not pass through the first-order root: a_v can exceed v' itself (g = 1e-30: v' = 1e-63, v'^ = 0).  There
|sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= min(|a - b| / sqrt(b), sqrt|a - b|) holds exactly, so a_v enters denom as
min(a_v / sqrt(v'), sqrt(a_v)) / sqrt(bc2): at most sqrt(3 d/2) = 4.6e-23, which is 5e-8 of eps = 1e-15 -- the size of u, and why these
rows need the term.

budget() returns 2 x these sums: the factor is the slack for what a first-order count drops (products of two errors, |x^| for |x| in
a bound).  Elements that the kernel must leave alone -- lazy with g = 0, or g_eff = m = v = 0 -- have a budget of exactly 0.
"""
import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
DENORM = 2.0 ** -149                                                     # the smallest fp32 denormal


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def step64(p, g, m, v, *, lr, betas, eps, weight_decay, maximize, lazy, step, lr_scale=None):
    """p, g, m, v: tensors of the kernel's fp32 values (any device) -> dict of float64 tensors: p, m, v (the new values) and what
    budget() needs: g_eff, denom, skip (bool: elements the step leaves alone under `lazy`)."""
    b1, b2 = float(betas[0]), float(betas[1])
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    ge = -g if maximize else g
    if weight_decay != 0:
        ge = torch.add(ge, p, alpha=float(weight_decay))               # g + wd p
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    rate = float(lr) if lr_scale is None else float(lr) * float(np.float64(np.float32(lr_scale)))
    # spelled with the ops _single_tensor_adam uses, so that two float64 evaluations of one statement do not differ by their own
    # rounding order (which g - m and p - D amplify without limit where they cancel)
    m1 = torch.lerp(m, ge, 1.0 - b1)                                    # m + (1-b1)(g - m)
    v1 = torch.addcmul(v * b2, ge, ge, value=1.0 - b2)                   # b2 v + (1-b2) g g
    denom = v1.sqrt() / math.sqrt(bc2) + float(eps)
    p1 = torch.addcdiv(p, m1, denom, value=-(rate / bc1))                # p - lr/bc1 m'/denom
    skip = (g == 0) if lazy else torch.zeros_like(g, dtype=torch.bool)
    return dict(p=torch.where(skip, p, p1), m=torch.where(skip, m, m1), v=torch.where(skip, v, v1), g_eff=ge, denom=denom, skip=skip)


# ---- the restatement of adam_one --------------------------------------------------------------------------------------------------
def _scalars32(lr, betas, eps, weight_decay, step, lr_scale):
    """The kernel's fp32 scalars as sn_adam_step / sn_adam_step_multi form them: in double, rounded once."""
    f = np.float32
    b1, b2 = float(betas[0]), float(betas[1])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    rate = float(lr) if lr_scale is None else float(lr) * float(np.float64(f(lr_scale)))
    return dict(c1=f(1.0 - b1), b2=f(b2), c2=f(1.0 - b2), ss=f(rate / bc1), ibs=f(1.0 / math.sqrt(bc2)), eps=f(eps), wd=f(weight_decay))


def _step32(p, g, m, v, s, maximize, lazy, eps_inside=False, maximize_late=False, decoupled=False, lazy_decay=False):
    """adam_one on float32 arrays with the scalars s; the keyword flags plant the defects of MUTANTS."""
    f = np.float32
    assert all(a.dtype == np.float32 for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        ge = -g if (maximize and not maximize_late) else g
        if s["wd"] != 0 and not decoupled:
            ge = ge + s["wd"] * p
        if maximize and maximize_late:
            ge = -ge
        skip = (ge == 0) & (np.ones_like(ge, dtype=bool) if lazy else ((m == 0) & (v == 0)))
        m1 = m + s["c1"] * (ge - m)
        gg = ge * ge
        v1 = v * s["b2"] + s["c2"] * gg
        denom = (np.sqrt(v1) + s["eps"]) * s["ibs"] if eps_inside else np.sqrt(v1) * s["ibs"] + s["eps"]
        p1 = p - s["ss"] * (m1 / denom)
        if decoupled and s["wd"] != 0:
            p1 = p1 - f(float(s["ss"]) * float(s["wd"])) * p
    assert m1.dtype == v1.dtype == p1.dtype == denom.dtype == np.float32
    out = dict(p=np.where(skip, p, p1), m=np.where(skip, m, m1), v=np.where(skip, v, v1))
    if lazy_decay:                                                       # skipped rows: the parameter stays, the moments move on
        out["m"], out["v"] = np.where(skip, m1, out["m"]), np.where(skip, v1, out["v"])
    return out


def step32(p, g, m, v, *, lr, betas, eps, weight_decay, maximize, lazy, step, lr_scale=None):
    """NumPy float32 arrays -> dict of float32 arrays p, m, v: the kernel's step, every operation rounded on its own."""
    return _step32(p, g, m, v, _scalars32(lr, betas, eps, weight_decay, step, lr_scale), maximize, lazy)


def _mutant(scalars=None, **flags):
    def run(p, g, m, v, *, lr, betas, eps, weight_decay, maximize, lazy, step, lr_scale=None):
        s = _scalars32(lr, betas, eps, weight_decay, step, lr_scale)
        if scalars is not None:
            s = scalars(s, lr=lr, betas=betas, step=step)
        return _step32(p, g, m, v, s, maximize, lazy, **flags)
    return run


def _one_minus_float_beta2(s, **kw):
    return dict(s, c2=np.float32(1.0) - s["b2"])                         # 1 - beta2 formed from the rounded beta2


def _bc2_without_root(s, betas, step, **kw):
    return dict(s, ibs=np.float32(1.0 / (1.0 - float(betas[1]) ** step)))


def _step_plus_one(s, lr, betas, step, **kw):
    b1, b2 = float(betas[0]), float(betas[1])
    return dict(s, ss=np.float32(float(lr) / (1.0 - b1 ** (step + 1))), ibs=np.float32(1.0 / math.sqrt(1.0 - b2 ** (step + 1))))


MUTANTS = {
    "one_minus_beta2_from_float_beta2": _mutant(_one_minus_float_beta2),
    "eps_before_the_bias_correction": _mutant(eps_inside=True),
    "bias_correction2_without_sqrt": _mutant(_bc2_without_root),
    "maximize_after_weight_decay": _mutant(maximize_late=True),
    "decoupled_weight_decay": _mutant(decoupled=True),
    "step_count_off_by_one": _mutant(_step_plus_one),
    "lazy_rows_decay_their_moments": _mutant(lazy_decay=True),
}


# ---- the budget -------------------------------------------------------------------------------------------------------------------
def budget(p, g, m, v, ref, *, lr, betas, eps, weight_decay, maximize, lazy, step, lr_scale=None):
    """The inputs (fp32 values, any device) and ref = step64(...) of them -> dict of float64 tensors p, m, v: the bound on
    |fp32 result - ref| per element.  The module docstring derives every term."""
    b1, b2 = float(betas[0]), float(betas[1])
    wd, eps = float(weight_decay), float(eps)
    p, m, v = p.double(), m.double(), v.double()
    ge, denom, m1, v1, p1 = ref["g_eff"], ref["denom"], ref["m"], ref["v"], ref["p"]
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    rate = (float(lr) if lr_scale is None else float(lr) * float(np.float64(np.float32(lr_scale)))) / bc1
    half = 0.5 * DENORM
    # (m1, v1, p1 of a skipped element are the old values: its budget is set to zero at the end, whatever comes out here)
    t_g = U * (ge.abs() + 2.0 * wd * p.abs()) + half if wd != 0 else torch.zeros_like(ge)
    t_m = U * (3.0 * (1.0 - b1) * (ge - m).abs() + m1.abs()) + (1.0 - b1) * t_g + half
    a_v = 3.0 * half
    t_v_rel = U * (3.0 * (1.0 - b2) * ge * ge + 2.0 * b2 * v + v1) + 2.0 * (1.0 - b2) * ge.abs() * t_g
    root = v1.sqrt()
    safe = root.clamp_min(1e-300)
    through_root = t_v_rel / (2.0 * safe) + torch.clamp(a_v / safe, max=math.sqrt(a_v))
    s = root / math.sqrt(bc2)
    t_den = U * (3.0 * s + eps + denom) + through_root / math.sqrt(bc2)
    q = m1 / denom
    delta = rate * q
    t_p = U * (p1.abs() + 3.0 * delta.abs()) + rate * (t_m / denom + q.abs() * t_den / denom + half) + half
    still = ref["skip"] | ((ge == 0) & (m == 0) & (v == 0))
    zero = torch.zeros_like(t_p)
    return dict(p=torch.where(still, zero, 2.0 * t_p), m=torch.where(still, zero, 2.0 * t_m), v=torch.where(still, zero, 2.0 * (t_v_rel + a_v)))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements with a positive bound, and whether every element with bound 0 is met exactly."""
    err = (got.double() - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    exact = bool((err[~pos] == 0).all())
    return ratio, exact


# ---- the cases --------------------------------------------------------------------------------------------------------------------
N_MAIN, N_UNDER, N_DENORMAL, N_CANCEL = 65536, 4096, 256, 16
CANCEL_WD = 0.5


def cases(seed=0):
    """dict of float32 arrays p, g, m, v of N_MAIN + N_UNDER + N_DENORMAL + N_CANCEL (69 904) elements, and `cancel`, the slice of the last block.
      main      |g| log-uniform in [1e-16, 1e12] with a random sign; a seventh of them exactly +0 or -0
      under     |g| log-uniform in [1e-30, 1e-17]: g g or (1-b2) g g leaves the normal range (denormal, or 0); moments on that scale
                are denormals or 0 themselves
      denormal  g itself an fp32 denormal, |g| in [1e-44, 1e-38]
      moments   |m| = |g| 10^[-1, 1] with a sign of its own (half of them cancel against g), v = g^2 10^[-2, 2]; where g = 0 they sit
                on a scale of their own (g = 0 with m, v != 0: the coasting rows that `lazy` freezes); a fifth of all elements has
                m = v = 0 (a first step) -- so a thirty-fifth has g = m = v = 0, the rows no step may write
      p         N(0, 1); a quarter uniform in [-1e-4, 1e-4] (the tables' initial range); a tenth exactly 0
      cancel    p = 0.5, m = v = 0 and g = -0.25 (first half), g = +0.25 (second half: the maximize twin): with weight_decay = 0.5
                the effective gradient is exactly 0 -- two whole quads of each kind, the block begins at a multiple of 4
    No NaN, no inf."""
    rng = np.random.RandomState(seed)
    n = N_MAIN + N_UNDER + N_DENORMAL

    def log_uniform(lo, hi, size):
        return 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), size)

    mag = np.concatenate([log_uniform(1e-16, 1e12, N_MAIN), log_uniform(1e-30, 1e-17, N_UNDER), log_uniform(1e-44, 1e-38, N_DENORMAL)])
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    gzero = np.zeros(n, dtype=bool)
    gzero[:N_MAIN] = rng.rand(N_MAIN) < 1.0 / 7.0
    g = np.where(gzero, 0.0, mag) * sign                                 # (-1.0 * 0.0 = -0.0: both zeros occur)
    scale = np.where(gzero, log_uniform(1e-12, 1e6, n), mag)
    m = scale * 10.0 ** rng.uniform(-1.0, 1.0, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    v = scale * scale * 10.0 ** rng.uniform(-2.0, 2.0, n)
    first = rng.rand(n) < 0.2
    m, v = np.where(first, 0.0, m), np.where(first, 0.0, v)
    p = rng.randn(n)
    kind = rng.rand(n)
    p = np.where(kind < 0.25, rng.uniform(-1e-4, 1e-4, n), p)
    p = np.where(kind > 0.9, 0.0, p)
    h = N_CANCEL // 2
    p = np.concatenate([p, np.full(N_CANCEL, 0.5)])
    g = np.concatenate([g, np.full(h, -0.25), np.full(h, 0.25)])
    m, v = np.concatenate([m, np.zeros(N_CANCEL)]), np.concatenate([v, np.zeros(N_CANCEL)])
    out = {k: a.astype(np.float32) for k, a in dict(p=p, g=g, m=m, v=v).items()}
    assert all(np.isfinite(a).all() for a in out.values()) and n % 4 == 0
    out["cancel"] = slice(n, n + N_CANCEL)
    return out


def _rows():
    rows = []
    for betas, eps, step, lr, maximize in itertools.product(((0.9, 0.999), (0.5, 0.99), (0.0, 0.0)), (1e-15, 1e-8), (1, 2, 7, 1000, 100000),
                                                            (1e-2, 3e-5), (False, True)):
        for wd, lazy in ((0.0, False), (1e-3, False), (0.0, True)):
            rows.append(dict(lr=lr, betas=betas, eps=eps, weight_decay=wd, maximize=maximize, lazy=lazy, step=step))
    return rows


HYPERS = _rows()                                                         # 360 rows: the product of the options, `lazy` with weight_decay = 0
CANCEL_HYPERS = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=CANCEL_WD, maximize=mx, lazy=False, step=1) for mx in (False, True)]


def row_id(h):
    return "b{}_{}-eps{:g}-wd{:g}-{}{}-t{}-lr{:g}".format(h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], "max" if h["maximize"] else "min",
                                                          "-lazy" if h["lazy"] else "", h["step"], h["lr"])
