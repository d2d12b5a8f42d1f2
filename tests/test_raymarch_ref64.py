"""The fp64 references of the ray operators (raymarch_ref64.py) and the bars of raymarch_cases.py, without a GPU:

  * the references agree with torch's fp64 evaluation (and autograd) of the reference's lines, and with the reference's own fp32 results
    kept in tests/golden (pdf_*);
  * the constants K of the bars are measured on fp32 restatements that are not the code under test;
  * fp32 restatements with one planted defect each fail the same comparison functions the GPU file uses.
"""
import math

import numpy as np
import pytest
import torch

import raymarch_cases as rc
import raymarch_ref64 as r64
from helpers import golden

F32 = np.float32
INF = F32(np.inf)


def tn(a):
    """a torch tensor of a copy (the cases are read-only)"""
    return torch.from_numpy(np.array(a))


def quiet():
    return np.errstate(all="ignore")


def exp32(x):
    """correctly rounded fp32 exponential"""
    with quiet():
        return np.exp(np.asarray(x, np.float64)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the reference's lines in numpy, each defect behind a switch.  A running sum follows torch.cumsum on the CPU:
# accumulated in fp64, every prefix rounded to fp32.
# ---------------------------------------------------------------------------------------------------------------------
def cumsum32(x):
    with quiet():
        return np.cumsum(x, axis=1, dtype=np.float64).astype(F32)


def weights_f32(rb, sg, opaque, g=None, drop_inf=False, inclusive=False, suffix_from_i=False, suffix_cancels=False):
    with quiet():
        delta = rb[:, 1:] - rb[:, :-1]
        ds = (delta * sg).astype(F32)
        if opaque:
            ds[:, -1] = INF
        add = np.where(ds == INF, F32(0), ds) if drop_inf else ds
        incl = cumsum32(add)
        c = incl if inclusive else np.concatenate([np.zeros_like(incl[:, :1]), incl[:, :-1]], axis=1)
        e, tr = exp32(-ds), exp32(-c)
        raw = (F32(1) - e) * tr
        bad = np.isnan(raw)
        w = np.where(bad, F32(0), raw)
        if g is None:
            return w
        gw = np.where(bad, F32(0), g * w)
        rev = cumsum32(gw[:, ::-1])[:, ::-1]
        after = rev if suffix_from_i else np.concatenate([rev[:, 1:], np.zeros_like(rev[:, :1])], axis=1)
        if suffix_cancels:
            after = (rev - gw).astype(F32)
        et = np.where((e == 0) | (tr == 0), F32(0), e * tr)
        dterm = np.where(bad, F32(0), g * et)
        inner = (dterm - after).astype(F32)
        gs = np.where((delta == 0) | (inner == 0), F32(0), delta * inner).astype(F32)
        if opaque:
            gs[:, -1] = 0
    return w, gs


def sample_pdf_f32(bins, w, u, T, left=False, no_clamp=False, no_pad=False):
    N, T0 = w.shape
    with quiet():
        if u is None:
            u = torch.linspace(0.5 / T, 1 - 0.5 / T, T).numpy()
        u = np.ascontiguousarray(np.broadcast_to(u, (N, T)))
        wp = w if no_pad else w + F32(0.01)
        pdf = (wp / wp.sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
        cdf = cumsum32(pdf)
        if not no_clamp:
            cdf = np.minimum(cdf, F32(1))
        cdf = np.concatenate([np.zeros_like(cdf[:, :1]), cdf], axis=1)
        inds = np.stack([np.searchsorted(cdf[n], u[n], side="left" if left else "right") for n in range(N)])
        below, above = np.clip(inds - 1, 0, T0), np.clip(inds, 0, T0)
        take = lambda a, i: np.take_along_axis(a, i, axis=1)      # noqa: E731
        c0, c1, b0, b1 = take(cdf, below), take(cdf, above), take(bins, below), take(bins, above)
        t = np.clip(np.nan_to_num(((u - c0) / (c1 - c0)).astype(F32)), 0, 1).astype(F32)
        return (b0 + t * (b1 - b0)).astype(F32), inds.astype(np.int32)


def spacing_f32(x):
    with quiet():
        return np.where(x < 1, x / F32(2), F32(1) - F32(1) / (F32(2) * x)).astype(F32)


def spacing_inv_f32(x):
    with quiet():
        return np.where(x < F32(0.5), F32(2) * x, F32(1) / (F32(2) - F32(2) * x)).astype(F32)


def positions_f32(o, d, near, far, bins, contract, bound):
    with quiet():
        sn, sf = spacing_f32(near), spacing_f32(far)
        rb = spacing_inv_f32((sn * (F32(1) - bins) + sf * bins).astype(F32))
        t = ((rb[:, 1:] + rb[:, :-1]) / F32(2)).astype(F32)
        p = (o[:, None, :] + d[:, None, :] * t[:, :, None]).astype(F32)
        if contract:
            mag = np.abs(p).max(axis=-1, keepdims=True)
            idx = np.abs(p).argmax(axis=-1)[..., None]
            sc = np.repeat(F32(1) / mag, 3, axis=-1)
            np.put_along_axis(sc, idx, (F32(2) - F32(1) / mag) / mag, axis=-1)
            p = np.where(mag < 1, p, p * sc).astype(F32)
        if bound > 0:
            p = ((p + F32(bound)) / F32(2 * bound)).astype(F32)
    return rb, t, p


def composite_f32(w, v, g):
    """sequential sums, as a kernel's loop has them"""
    out = np.zeros((w.shape[0], v.shape[2]), F32)
    for t in range(w.shape[1]):
        out = (out + w[:, t, None] * v[:, t, :]).astype(F32)
    gw = np.zeros_like(w)
    for k in range(v.shape[2]):
        gw = (gw + v[:, :, k] * g[:, None, k]).astype(F32)
    return out, gw, (w[:, :, None] * g[:, None, :]).astype(F32)


def proposal_f32(b, w, rb, rw, no_hi_clamp=False):
    """-> per-ray sums and d/dw; an unclamped hi reads one past the end of the running sum (taken as 0 here)"""
    N, T = w.shape
    cum = np.concatenate([np.zeros((N, 1), F32), cumsum32(w), np.zeros((N, 1), F32)], axis=1)
    lo = np.stack([np.searchsorted(b[n, :-1], rb[n, :-1], side="right") - 1 for n in range(N)]).clip(0, T - 1)
    hi = np.stack([np.searchsorted(b[n, 1:], rb[n, 1:], side="right") for n in range(N)])
    if not no_hi_clamp:
        hi = hi.clip(0, T - 1)
    bound = (np.take_along_axis(cum, hi + 1, axis=1) - np.take_along_axis(cum, lo, axis=1)).astype(F32)
    d = np.maximum(rw - bound, F32(0)).astype(F32)
    den = (rw + F32(1e-8)).astype(F32)
    term = (d * d / den).astype(F32)
    gj = (F32(-2) * d / den).astype(F32)
    i = np.arange(T)
    gw = np.stack([(((lo[n][:, None] <= i) & (i <= hi[n][:, None])) * gj[n][:, None]).sum(axis=0, dtype=F32) for n in range(N)])
    return term.sum(axis=1, dtype=F32), gw.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# torch fp64 statements of the reference's lines
# ---------------------------------------------------------------------------------------------------------------------
def torch_weights64(rb, sg, g, opaque):
    s = tn(sg).double().requires_grad_(True)
    rbd = tn(rb).double()
    ds = (rbd[..., 1:] - rbd[..., :-1]) * s
    if opaque:
        ds = torch.cat([ds[..., :-1], torch.full_like(ds[..., -1:], torch.inf)], dim=-1)
    alphas = 1 - torch.exp(-ds)
    trans = torch.cumsum(ds[..., :-1], dim=-1)
    trans = torch.exp(-torch.cat([torch.zeros_like(ds[..., :1]), trans], dim=-1))
    w = (alphas * trans).nan_to_num(0)
    (w * tn(g).double()).sum().backward()
    return w.detach().numpy(), s.grad.numpy()


def torch_pdf64(bins, weights, u):
    bins, weights = tn(bins).double(), tn(weights).double()
    N, T0 = weights.shape
    weights = weights + float(np.float32(0.01))
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1).clamp(max=1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = tn(np.ascontiguousarray(np.broadcast_to(u, (N, np.shape(u)[-1])))).double().contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below, above = torch.clamp(inds - 1, 0, T0), torch.clamp(inds, 0, T0)
    c0, c1 = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    b0, b1 = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
    t = torch.clamp(torch.nan_to_num((u - c0) / (c1 - c0)), 0, 1)
    return (b0 + t * (b1 - b0)).numpy(), inds.numpy()


def torch_proposal64(b, w, rb, rw):
    w2 = tn(w).double().requires_grad_(True)
    bd, rbd, rwd = (tn(a).double() for a in (b, rb, rw))
    cum = torch.cat([torch.zeros_like(w2[..., :1]), torch.cumsum(w2, dim=-1)], dim=-1)
    last = w.shape[1] - 1
    lo = (torch.searchsorted(bd[..., :-1].contiguous(), rbd[..., :-1].contiguous(), right=True) - 1).clamp(0, last)
    hi = torch.searchsorted(bd[..., 1:].contiguous(), rbd[..., 1:].contiguous(), right=True).clamp(0, last)
    bound = torch.take_along_dim(cum[..., 1:], hi, dim=-1) - torch.take_along_dim(cum[..., :-1], lo, dim=-1)
    per_ray = ((rwd - bound).clamp(min=0) ** 2 / (rwd + float(np.float32(1e-8)))).sum(dim=-1)
    per_ray.sum().backward()
    return per_ray.detach().numpy(), w2.grad.numpy()


AGREE = 1e-5        # fp64 against fp64, in units of 2^-24 * scale (fp64's own unit is 2^-29 of that)


# ---------------------------------------------------------------------------------------------------------------------
# the references are pinned
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", rc.WEIGHTS_T)
@pytest.mark.parametrize("opaque", [True, False])
def test_weights_reference_equals_torch_fp64_autograd(T, opaque):
    c, ref = rc.weights_case(T), rc.weights_ref(T, opaque)
    w, gs = torch_weights64(c["rb"], c["sg"], c["g"], opaque)
    assert rc.ratio(w, ref["w"], ref["scale_w"]) < AGREE                       # forward: every ray, the non-finite ones included
    torch_bad = ~np.isfinite(gs).all(axis=1)
    assert set(np.nonzero(torch_bad)[0]) <= set(rc.WEIGHTS_NONFINITE_ROWS), np.nonzero(torch_bad)[0]
    ok = ~torch_bad
    assert ok.sum() >= rc.WEIGHTS_N - len(rc.WEIGHTS_NONFINITE_ROWS)
    assert rc.ratio(gs[ok], ref["gs"][ok], ref["scale_gs"][ok]) < AGREE
    # where torch has none: the documented behaviour, finite everywhere
    assert np.isfinite(ref["gs"]).all() and np.isfinite(ref["w"]).all()
    if rc.weights_has_nan(T, opaque):
        for r in rc.weights_rows("inf_zero_width"):
            assert (ref["gs"][r, c["mid"]:] == 0).all() and (ref["w"][r, c["mid"]:] == 0).all()
    if opaque:
        assert (ref["gs"][:, -1] == 0).all()


@pytest.mark.parametrize("T0,T", rc.PDF_SHAPES)
def test_sample_pdf_reference_equals_torch_fp64(T0, T):
    c = rc.pdf_case(T0, T)
    for form in rc.U_FORMS:
        ref = rc.pdf_ref(T0, T, form)
        u = rc.pdf_u(c, form)
        out, inds = torch_pdf64(c["bins"], c["w"], r64.linspace_u(T) if u is None else u)
        assert np.array_equal(inds, ref["inds"]), form
        assert rc.ratio(out, ref["out"], ref["scale"]) < AGREE, form


@pytest.mark.parametrize("tag,T", [("a", 65), ("b", 33), ("c", 17), ("d", 33)])
def test_sample_pdf_reference_against_the_reference_goldens(tag, T):
    """pdf_* hold the reference's own fp32 torch results: bins within the bar, indices equal except where u lies within the measured cdf
    rounding of a knot -- at most the 2 per case that test_sample_pdf_indices_bit_exact_vs_oracle allows."""
    g = golden("units")
    bins, w, u = g[f"pdf_{tag}_bins"], g[f"pdf_{tag}_w"], g[f"pdf_{tag}_u"]
    ref = r64.sample_pdf(bins, w, u)
    rc.hold(g[f"pdf_{tag}_out"], ref["out"], ref["scale"], rc.K["sample_pdf"], f"golden pdf_{tag}")
    diff = g[f"pdf_{tag}_inds"] != ref["inds"]
    print(f"pdf_{tag}: {int(diff.sum())} golden indices differ from fp64")
    assert diff.sum() <= 2
    assert (ref["knot_gap"][diff] <= rc.K["sample_pdf_knot"] * rc.EPS).all()


@pytest.mark.parametrize("T", rc.POS_T)
def test_positions_reference_equals_torch_fp64(T):
    c = rc.pos_case(T)
    hit = ~c["miss"]
    o, d, near, far, bins = (tn(c[k]).double() for k in ("o", "d", "near", "far", "bins"))
    g = lambda x: torch.where(x < 1, x / 2, 1 - 1 / (2 * x))                # noqa: E731
    ginv = lambda x: torch.where(x < 0.5, 2 * x, 1 / (2 - 2 * x))           # noqa: E731
    rb = ginv(g(near) * (1 - bins) + g(far) * bins)
    t = (rb[..., 1:] + rb[..., :-1]) / 2
    x = o.unsqueeze(1) + d.unsqueeze(1) * t.unsqueeze(2)
    flat = x.view(-1, 3)
    mag, idx = flat.abs().max(1, keepdim=True)
    scale = 1 / mag.repeat(1, 3)
    scale.scatter_(1, idx, (2 - 1 / mag) / mag)
    z = torch.where(mag < 1, flat, flat * scale).view(x.shape)
    for contract in (True, False):
        for bound in rc.POS_BOUNDS:
            ref = rc.pos_ref(T, contract, bound)
            p = z if contract else x
            p = (p + bound) / (2 * bound) if bound > 0 else p
            assert rc.ratio(rb.numpy()[hit], ref["real_bins"][hit], ref["scale_rb"][hit]) < AGREE
            assert rc.ratio(t.numpy()[hit], ref["rays_t"][hit], ref["scale_t"][hit]) < AGREE
            assert rc.ratio(p.numpy()[hit], ref["xyzs"][hit], ref["scale_x"][hit]) < AGREE
    fn, inv, _ = rc.spacing_points()
    assert np.array_equal(r64.spacing(fn), g(tn(fn).double()).numpy())
    assert np.array_equal(r64.spacing_inv(inv), ginv(tn(inv).double()).numpy())


@pytest.mark.parametrize("N,T,Kc", rc.COMPOSITE_SHAPES)
def test_composite_reference_equals_torch_fp64_autograd(N, T, Kc):
    c, ref = rc.composite_case(N, T, Kc), rc.composite_ref(N, T, Kc)
    w = tn(c["w"]).double().requires_grad_(True)
    v = tn(c["v"]).double().requires_grad_(True)
    out = (w.unsqueeze(-1) * v).sum(dim=1)
    (out * tn(c["g"]).double()).sum().backward()
    assert rc.ratio(out.detach().numpy(), ref["out"], ref["scale_out"]) < AGREE
    assert rc.ratio(w.grad.numpy(), ref["gw"], ref["scale_gw"]) < AGREE
    assert rc.ratio(v.grad.numpy(), ref["gv"], ref["scale_gv"]) < AGREE


@pytest.mark.parametrize("T,Tr", rc.PROPOSAL_SHAPES)
def test_proposal_reference_equals_torch_fp64_autograd(T, Tr):
    c, ref = rc.proposal_case(T, Tr), rc.proposal_ref(T, Tr)
    per_ray, gw = torch_proposal64(c["b"], c["w"], c["rb"], c["rw"])
    assert rc.ratio(per_ray, ref["per_ray"], ref["scale_per_ray"]) < AGREE
    # torch's cumsum backward differences prefix sums: its own fp64 noise floor is ~1e-13 of a ray's largest gradient
    assert rc.ratio(gw, ref["gw"], ref["scale_gw"] + 0.2 * np.abs(ref["gw"]).max(axis=1, keepdims=True)) < AGREE
    # the rows do what they are built for
    for r in range(rc.PROPOSAL_N):
        kind = rc.proposal_kind(r)
        if kind == "zero_w":
            assert np.allclose(ref["per_ray"][r], (c["rw"][r].astype(np.float64) ** 2 / (c["rw"][r] + r64.DEN)).sum())
        if kind == "covered":
            assert ref["per_ray"][r] <= 1e-12
        if kind == "below":
            assert (ref["lo"][r] == 0).all()
        if kind == "above":
            assert (ref["hi"][r] == T - 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# the constants are measured
# ---------------------------------------------------------------------------------------------------------------------
def oracle_pdf_runs(orc):
    """(T0, T, form, out, inds) of the oracle over every sample_pdf case"""
    for T0, T in rc.PDF_SHAPES:
        c = rc.pdf_case(T0, T)
        for form in rc.U_FORMS:
            u = rc.pdf_u(c, form)
            if form == "per_ray":                                   # the oracle takes one u row for all rays: ray by ray
                rows = [orc.sample_pdf(c["bins"][r:r + 1], c["w"][r:r + 1], T, u=u[r]) for r in range(rc.PDF_N)]
                out, inds = np.concatenate([a for a, _ in rows]), np.concatenate([b for _, b in rows])
            else:
                out, inds = orc.sample_pdf(c["bins"], c["w"], T, u=u)
            yield T0, T, form, out, inds


def measure(orc):
    m = {k: 0.0 for k in rc.MEASURED}
    up = lambda k, v: m.__setitem__(k, max(m[k], v))           # noqa: E731
    for T in rc.WEIGHTS_T:
        c = rc.weights_case(T)
        for opaque in (True, False):
            ref = rc.weights_ref(T, opaque)
            up("weights", rc.ratio(orc.weights_from_sigma(c["rb"], c["sg"], opaque), ref["w"], ref["scale_w"]))
            up("weights_backward", rc.ratio(weights_f32(c["rb"], c["sg"], opaque, c["g"])[1], ref["gs"], ref["scale_gs"]))
    exceptions = 0
    for T0, T, form, out, inds in oracle_pdf_runs(orc):
        ref = rc.pdf_ref(T0, T, form)
        up("sample_pdf", rc.ratio(out, ref["out"], ref["scale"]))
        diff = inds != ref["inds"]
        exceptions += int(diff.sum())
        if diff.any():
            up("sample_pdf_knot", float(ref["knot_gap"][diff].max()) / rc.EPS)
    for T in rc.POS_T:
        c = rc.pos_case(T)
        hit = ~c["miss"]
        for contract in (True, False):
            for bound in rc.POS_BOUNDS:
                ref = rc.pos_ref(T, contract, bound)
                rb, t, p = positions_f32(c["o"], c["d"], c["near"], c["far"], c["bins"], contract, bound)
                up("real_bins", rc.ratio(rb[hit], ref["real_bins"][hit], ref["scale_rb"][hit]))
                up("rays_t", rc.ratio(t[hit], ref["rays_t"][hit], ref["scale_t"][hit]))
                up("xyzs", rc.ratio(p[hit], ref["xyzs"][hit], ref["scale_x"][hit]))
    for N, T, Kc in rc.COMPOSITE_SHAPES:
        c, ref = rc.composite_case(N, T, Kc), rc.composite_ref(N, T, Kc)
        out, gw, gv = composite_f32(c["w"], c["v"], c["g"])
        up("composite", rc.ratio(out, ref["out"], ref["scale_out"]))
        up("composite_gw", rc.ratio(gw, ref["gw"], ref["scale_gw"]))
        up("composite_gv", rc.ratio(gv, ref["gv"], ref["scale_gv"]))
    for T, Tr in rc.PROPOSAL_SHAPES:
        c, ref = rc.proposal_case(T, Tr), rc.proposal_ref(T, Tr)
        per_ray, gw = proposal_f32(c["b"], c["w"], c["rb"], c["rw"])
        up("proposal", rc.ratio(per_ray, ref["per_ray"], ref["scale_per_ray"]))
        up("proposal_gw", rc.ratio(gw, ref["gw"], ref["scale_gw"]))
        n = F32(rc.PROPOSAL_N * Tr)
        mean, scale_mean, gwm, scale_gwm = rc.proposal_mean_ref(T, Tr)
        up("proposal", rc.ratio(np.asarray([per_ray.sum(dtype=F32) / n]), mean, scale_mean))
        up("proposal_gw", rc.ratio(gw / n, gwm, scale_gwm))
    return m, exceptions


def test_measured_constants(orc):
    """the fp32 restatements stay within K on every case; K is the recorded measurement doubled and rounded up"""
    m, exceptions = measure(orc)
    for k, v in m.items():
        print(f"{k:20s} measured {v:10.4f}   recorded {rc.MEASURED[k][0]:10.4f}   K {rc.K[k]}")
    print(f"sample_pdf index exceptions of the oracle: {exceptions} (recorded {rc.PDF_INDEX_EXCEPTIONS})")
    for k, v in m.items():
        recorded, K = rc.MEASURED[k]
        assert K == max(1, math.ceil(2 * recorded)), k
        assert v <= K, f"{k}: the fp32 restatement is {v} * 2^-24 * scale from fp64, beyond K = {K}"
        assert v <= recorded * 1.001 + 1e-9, f"{k}: measured {v}, recorded {recorded}: the cases drifted; record the new figure"
    assert exceptions == rc.PDF_INDEX_EXCEPTIONS


def test_restatements_pass_the_comparisons(orc):
    """what the GPU file asks of the kernels, asked of the fp32 restatements (so the planted defects below differ in one thing only)"""
    for T in rc.WEIGHTS_T:
        c = rc.weights_case(T)
        for opaque in (True, False):
            rc.check_weights(T, opaque, orc.weights_from_sigma(c["rb"], c["sg"], opaque))
            rc.check_weights_backward(T, opaque, weights_f32(c["rb"], c["sg"], opaque, c["g"])[1])
    total = sum(rc.check_pdf(T0, T, form, out, inds) for T0, T, form, out, inds in oracle_pdf_runs(orc))
    assert total == rc.PDF_INDEX_EXCEPTIONS
    for T in rc.POS_T:
        c = rc.pos_case(T)
        for contract in (True, False):
            for bound in rc.POS_BOUNDS:
                rc.check_positions(T, contract, bound, *positions_f32(c["o"], c["d"], c["near"], c["far"], c["bins"], contract, bound))
    for N, T, Kc in rc.COMPOSITE_SHAPES:
        c = rc.composite_case(N, T, Kc)
        rc.check_composite(N, T, Kc, *composite_f32(c["w"], c["v"], c["g"]))
    for T, Tr in rc.PROPOSAL_SHAPES:
        c = rc.proposal_case(T, Tr)
        per_ray, gw = proposal_f32(c["b"], c["w"], c["rb"], c["rw"])
        rc.check_proposal(T, Tr, per_ray, gw)
        n = F32(rc.PROPOSAL_N * Tr)
        rc.check_proposal_mean(T, Tr, per_ray.sum(dtype=F32) / n, gw / n)


def test_the_two_lds_boundary_cases_have_one_answer():
    """(2047, 33) and (2048, 33) differ by one bin of zero width and zero probability: each meets the other's reference"""
    for form in rc.U_FORMS:
        a, b = rc.pdf_ref(2047, 33, form), rc.pdf_ref(2048, 33, form)
        assert rc.ratio(a["out"], b["out"], b["scale"]) < AGREE and rc.ratio(b["out"], a["out"], a["scale"]) < AGREE


def test_spacing_statements_on_the_cpu():
    """what the GPU file asserts of the spacing ops and of rays that miss the box, on the fp32 restatement first"""
    fn, inv, branch = rc.spacing_points()
    for x, f32, f64, pts in ((fn, spacing_f32, r64.spacing, branch["fn"]), (inv, spacing_inv_f32, r64.spacing_inv, branch["inv"])):
        got, want = f32(x), f64(x).astype(F32)
        assert (np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1).all()
        at = np.isin(x, pts)
        assert at.any() and np.array_equal(got[at], want[at])
    assert spacing_f32(F32(1e9)) == 1.0
    for T in rc.POS_T:
        c = rc.pos_case(T)
        assert np.array_equal(c["miss"], c["near"][:, 0] == F32(1e9)) and np.array_equal(c["miss"], c["far"][:, 0] == F32(1e9))
        rb, _, _ = positions_f32(c["o"], c["d"], c["near"], c["far"], c["bins"], True, 0.0)
        assert not np.isnan(rb[c["miss"]]).any() and (rb[c["miss"]] >= 2.0 ** 23).all()


# ---------------------------------------------------------------------------------------------------------------------
# the bars bite
# ---------------------------------------------------------------------------------------------------------------------
def failures(runs):
    """number of (case, thunk) pairs whose comparison raises"""
    n = 0
    for thunk in runs:
        try:
            thunk()
        except AssertionError:
            n += 1
    return n


def weights_runs(**defect):
    for T in rc.WEIGHTS_T:
        c = rc.weights_case(T)
        for opaque in (True, False):
            def run(T=T, c=c, opaque=opaque):
                w, gs = weights_f32(c["rb"], c["sg"], opaque, c["g"], **defect)
                rc.check_weights(T, opaque, w)
                rc.check_weights_backward(T, opaque, gs)
            yield run


def pdf_runs(**defect):
    for T0, T in rc.PDF_SHAPES:
        c = rc.pdf_case(T0, T)
        for form in rc.U_FORMS:
            def run(T0=T0, T=T, c=c, form=form):
                out, inds = sample_pdf_f32(c["bins"], c["w"], rc.pdf_u(c, form), T, **defect)
                rc.check_pdf(T0, T, form, out, inds)
            yield run


def proposal_runs(**defect):
    for T, Tr in rc.PROPOSAL_SHAPES:
        c = rc.proposal_case(T, Tr)
        def run(T=T, Tr=Tr, c=c):
            rc.check_proposal(T, Tr, *proposal_f32(c["b"], c["w"], c["rb"], c["rw"], **defect))
        yield run


@pytest.mark.parametrize("runs,defect", [
    (weights_runs, dict(drop_inf=True)),             # +inf dropped from the running depth
    (weights_runs, dict(inclusive=True)),            # T_i taken inclusive instead of exclusive
    (weights_runs, dict(suffix_from_i=True)),        # the gradient's suffix sum starting at j >= i
    (weights_runs, dict(suffix_cancels=True)),       # the suffix sum taken as (inclusive suffix) - (own term): cancels where the own term is large
    (pdf_runs, dict(left=True)),                     # searchsorted left instead of right
    (pdf_runs, dict(no_clamp=True)),                 # the cdf clamp at 1 removed
    (pdf_runs, dict(no_pad=True)),                   # the 0.01 pad missing
    (proposal_runs, dict(no_hi_clamp=True)),         # hi not clamped
], ids=["inf_dropped", "inclusive_T", "suffix_from_i", "suffix_cancels", "searchsorted_left", "no_cdf_clamp", "no_pad", "hi_unclamped"])
def test_planted_defects_fail(runs, defect):
    assert failures(runs()) == 0, "the restatement itself must pass"
    n = failures(runs(**defect))
    print(f"{defect}: {n} cases fail")
    assert n >= 1
