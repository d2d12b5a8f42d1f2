"""CPU: tests/adam_ref64.py held to torch and to itself, without a GPU --
  * step64 IS torch's Adam: against torch.optim.Adam(foreach=False) on float64 tensors, the state (step, exp_avg, exp_avg_sq) loaded
    through load_state_dict, every row of HYPERS, 1e-13 relative per element; the `lazy` rows against torch.optim.SparseAdam;
  * the budget can be met: step32, the fp32 restatement of the kernel, stays inside budget() on every element of cases() x every row;
  * the budget bites: every entry of MUTANTS leaves it somewhere.
The GPU side (tests/test_gpu_adam_ref64.py) holds k_adam and k_adam_multi to the same statement, budget, cases and rows."""
import functools
import math

import numpy as np
import pytest
import torch

import adam_ref64 as ref

RTOL = 1e-13


@functools.lru_cache(maxsize=None)
def table():
    c = ref.cases(0)
    return c, {k: torch.from_numpy(c[k]) for k in "pgmv"}


def loaded(opt, step, m, v, step_value):
    """The optimiser with (step - 1, m, v) as its state, through load_state_dict as a checkpoint would arrive."""
    sd = opt.state_dict()
    sd["state"] = {0: {"step": step_value(step - 1), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}}
    opt.load_state_dict(sd)
    return opt


def assert_close(got, want, what, scale=None):
    """|got - want| <= 1e-13 scale per element; scale is |want| itself unless one is given."""
    err = (got - want).abs()
    scale = want.abs() if scale is None else scale
    bad = err > RTOL * scale
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements, worst relative {float((err / scale.clamp_min(1e-300))[bad].max()):.3e}"


def test_the_case_table_holds_every_regime():
    c, _ = table()
    p, g, m, v = (c[k] for k in "pgmv")
    n = g.size
    assert 69000 <= n <= 71000 and all(a.dtype == np.float32 and a.shape == (n,) and np.isfinite(a).all() for a in (p, g, m, v))
    tiny = float(np.finfo(np.float32).tiny)
    assert np.abs(g[g != 0]).min() < tiny and np.abs(g).max() > 1e11                       # denormal gradients up to 1e12
    assert 0.1 < (g[:ref.N_MAIN] == 0).mean() < 0.18 and (np.signbit(g) & (g == 0)).any() and (~np.signbit(g) & (g == 0)).any()
    assert ((np.abs(g) >= 1e-30) & (np.abs(g) <= 1e-17)).sum() >= ref.N_UNDER
    assert ((v > 0) & (v < tiny)).any(), "denormal second moments"
    assert 0.17 < ((m == 0) & (v == 0)).mean() < 0.23
    assert ((g == 0) & (m != 0) & (v != 0)).sum() > 1000 and ((g == 0) & (m == 0) & (v == 0)).sum() > 100
    assert (v >= 0).all() and (p == 0).sum() > 1000 and ((p != 0) & (np.abs(p) <= 1e-4)).sum() > 10000
    k = c["cancel"]
    assert k.start % 4 == 0 and k.stop == n
    for mx, half in ((False, slice(k.start, k.start + 8)), (True, slice(k.start + 8, k.stop))):
        ge = (-g[half] if mx else g[half]) + np.float32(ref.CANCEL_WD) * p[half]
        assert (ge == 0).all() and (g[half] != 0).all() and (m[half] == 0).all() and (v[half] == 0).all()
    assert len(ref.HYPERS) == 360 and sum(h["lazy"] for h in ref.HYPERS) == 120 and not any(h["lazy"] and h["weight_decay"] for h in ref.HYPERS)
    assert len({ref.row_id(h) for h in ref.HYPERS}) == 360


def test_step64_is_torch_adam_in_float64():
    """Every dense row of HYPERS and both CANCEL_HYPERS rows, all elements: p', m', v' within 1e-13 relative of torch's own float64 step."""
    _, T = table()
    rows = [h for h in ref.HYPERS + ref.CANCEL_HYPERS if not h["lazy"]]
    for h in rows:
        p = torch.nn.Parameter(T["p"].double().clone())
        p.grad = T["g"].double().clone()
        opt = torch.optim.Adam([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], maximize=h["maximize"], foreach=False)
        loaded(opt, h["step"], T["m"], T["v"], lambda s: torch.tensor(float(s))).step()
        assert float(opt.state[p]["step"]) == h["step"]
        r = ref.step64(T["p"], T["g"], T["m"], T["v"], **h)
        assert_close(r["p"], p.detach(), f"p' {ref.row_id(h)}")
        assert_close(r["m"], opt.state[p]["exp_avg"], f"m' {ref.row_id(h)}")
        assert_close(r["v"], opt.state[p]["exp_avg_sq"], f"v' {ref.row_id(h)}")
    assert len(rows) == 242


def test_lazy_is_torch_sparse_adam_in_float64():
    """The `lazy` rows against torch.optim.SparseAdam with g.to_sparse() as the gradient: untouched elements keep p, m and v to the bit, the
    touched ones agree within 1e-13 relative.

    SparseAdam departs from the header's rule in one place, for a reason of its own: it adds eps BEFORE the second bias correction
    (torch/optim/_functional.py sparse_adam: denom = sqrt(v') + eps, step_size = lr sqrt(bc2) / bc1), so its eps acts as eps / sqrt(bc2)
    where the dense recipe -- which the header words `lazy` in terms of, and the kernel shares with the dense path -- has eps.  The two
    are the same function of the state when SparseAdam is given eps sqrt(bc2), which is what this test hands it (for the rows with
    bc2 = 1 -- step 100000, or beta2 = 0 -- that is eps itself).  The moments do not involve eps and are compared as they come.

    What 1e-13 is relative to, here: SparseAdam rounds the same real functions in another order -- m + (g - m)(1-b1) product by product
    where lerp fuses, v + (g^2 - v)(1-b2) where the dense recipe has b2 v + (1-b2) g^2 -- and each rounding is 1.1e-16 of the TERMS.
    Where g - m or p - D cancels (a few elements of the table: m' three decades below g), that is not 1e-13 of the RESULT, for any
    two orders.  So m' is held to 1e-13 max(|m|, |g|, |m'|), v' to 1e-13 max(v, g^2, v'), and p' to 1e-13 (max(|p|, |p'|) + lr/bc1
    max(|m|, |g|) / denom), the last term being what the quotient inherits from m'.  (The dense test above needs none of this: step64
    is spelled in the ops torch's dense recipe uses, and is held to 1e-13 of the result itself.)"""
    _, T = table()
    rows = [h for h in ref.HYPERS if h["lazy"]]
    touched = T["g"] != 0
    for h in rows:
        bc2 = 1.0 - h["betas"][1] ** h["step"]
        p = torch.nn.Parameter(T["p"].double().clone())
        p.grad = T["g"].double().to_sparse()
        opt = torch.optim.SparseAdam([p], lr=h["lr"], betas=h["betas"], eps=h["eps"] * math.sqrt(bc2), maximize=h["maximize"])
        loaded(opt, h["step"], T["m"], T["v"], int).step()
        assert opt.state[p]["step"] == h["step"]
        r = ref.step64(T["p"], T["g"], T["m"], T["v"], **h)
        g64, m64, v64, p64 = T["g"].double(), T["m"].double(), T["v"].double(), T["p"].double()
        terms = torch.maximum(m64.abs(), g64.abs())
        scale = dict(m=torch.maximum(terms, r["m"].abs()), v=torch.maximum(torch.maximum(v64, g64 * g64), r["v"]),
                     p=torch.maximum(p64.abs(), r["p"].abs()) + h["lr"] / (1.0 - h["betas"][0] ** h["step"]) * terms / r["denom"])
        for key, got, before in (("p", p.detach(), p64), ("m", opt.state[p]["exp_avg"], m64), ("v", opt.state[p]["exp_avg_sq"], v64)):
            assert torch.equal(got[~touched], before[~touched]), f"SparseAdam moved an untouched {key}"
            assert torch.equal(r[key][~touched], before[~touched]), f"step64 moved an untouched {key} ({ref.row_id(h)})"
            assert_close(r[key][touched], got[touched], f"{key}' {ref.row_id(h)}", scale[key][touched])
        assert torch.equal(r["skip"], ~touched)
    assert len(rows) == 120


@functools.lru_cache(maxsize=None)
def sweep():
    """One pass over every row: step64 and the budget once per row, then step32 and every mutant against them.
    -> {name: {"p" | "m" | "v": (worst error / budget, its row), "exact": every zero-budget element met exactly}}"""
    c, T = table()
    arrays = [c[k] for k in "pgmv"]
    names = ["step32"] + list(ref.MUTANTS)
    out = {n: {"p": (0.0, None), "m": (0.0, None), "v": (0.0, None), "exact": True} for n in names}
    for h in ref.HYPERS + ref.CANCEL_HYPERS:
        r = ref.step64(T["p"], T["g"], T["m"], T["v"], **h)
        b = ref.budget(T["p"], T["g"], T["m"], T["v"], r, **h)
        for n in names:
            got = (ref.step32 if n == "step32" else ref.MUTANTS[n])(*arrays, **h)
            for k in "pmv":
                ratio, exact = ref.worst_ratio(torch.from_numpy(got[k]), r[k], b[k])
                if not exact:
                    out[n]["exact"] = False
                if ratio > out[n][k][0]:
                    out[n][k] = (ratio, ref.row_id(h))
    return out


def test_step32_stays_inside_the_budget_everywhere():
    """The condition that keeps the bound honest: the fp32 restatement alone, on every element x every row, uses less than the budget --
    and leaves the elements with a budget of 0 (lazy rows, all-zero rows) exactly as they were."""
    w = sweep()["step32"]
    for k in "pmv":
        print(f"step32 {k}': worst error / budget = {w[k][0]:.3f} at {w[k][1]}")
    assert w["exact"]
    assert all(w[k][0] < 1.0 for k in "pmv"), w


@pytest.mark.parametrize("name", list(ref.MUTANTS))
def test_the_budget_rejects_every_planted_defect(name):
    w = sweep()[name]
    factor = max(w[k][0] for k in "pmv")
    for k in "pmv":
        print(f"{name} {k}': worst error / budget = {w[k][0]:.3e} at {w[k][1]}")
    print(f"{name}: elements with a budget of 0 (rows no step may write) all kept = {w['exact']}")
    assert factor > 1.0 or not w["exact"], f"{name} slips through: {w}"


def test_step32_forms_its_scalars_from_doubles():
    """The three scalars that differ when formed in fp32: 1 - beta2 (the comment in sn_adam_step), the step size and 1 / sqrt(bc2)."""
    s = ref._scalars32(1e-2, (0.9, 0.999), 1e-15, 0.0, 7, None)
    assert s["c2"] == np.float32(1.0 - 0.999) != np.float32(1.0) - np.float32(0.999)
    assert s["ss"] == np.float32(1e-2 / (1.0 - 0.9 ** 7)) and s["ibs"] == np.float32(1.0 / (1.0 - 0.999 ** 7) ** 0.5)
    assert all(v.dtype == np.float32 for v in s.values())
    t = ref._scalars32(1e-2, (0.9, 0.999), 1e-15, 0.0, 7, 0.1 ** 0.35)
    assert t["ss"] == np.float32(1e-2 * float(np.float32(0.1 ** 0.35)) / (1.0 - 0.9 ** 7))
