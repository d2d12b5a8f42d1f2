"""Seeded case builders and the comparison functions of the ray operators' fp64 tests, shared by the CPU file (test_raymarch_ref64.py:
pins the references, measures the constants, shows that planted defects fail) and the GPU file (test_gpu_raymarch_ref64.py).

Every comparison holds each output element to |got - ref64| <= K * 2^-24 * scale + 2^-149 with the reference's own condition scale
(raymarch_ref64.py).  K is measured on the CPU: the largest |fp32 - fp64| / (2^-24 * scale) of an fp32 restatement that is not the code
under test (the oracle where it has the operator, numpy / torch-CPU float32 elsewhere) over these cases, doubled and rounded up -- the
factor 2 covers fmaf contraction and the device's different but equally valid summation order.  The subnormal step 2^-149 of the bar is
taken off |fp32 - fp64| before the ratio is formed (a subnormal result cannot be closer than that, whatever its scale).
"""
import functools

import numpy as np

import raymarch_ref64 as r64
from raymarch_ref64 import EPS, TINY

F32 = np.float32
FMAX = np.finfo(np.float32).max

# operator                      measured   K          (test_raymarch_ref64.py::test_measured_constants: K = ceil(2 * measured))
MEASURED = {
    "weights":                  (1.406, 3),
    "weights_backward":         (2.6397, 6),
    "sample_pdf":               (2.094, 5),
    "sample_pdf_knot":          (1.0, 2),      # |u - knot| / 2^-24 where an fp32 index differs from the fp64 one
    "real_bins":                (1.6722, 4),
    "rays_t":                   (1.116, 3),
    "xyzs":                     (1.0787, 3),
    "composite":                (8.1988, 17),
    "composite_gw":             (7.1294, 15),
    "composite_gv":             (0.9994, 2),
    "proposal":                 (0.6629, 2),
    "proposal_gw":              (3.702, 8),
}
K = {k: v[1] for k, v in MEASURED.items()}
# elements of all sample_pdf cases (every u form) whose oracle index differs from the fp64 index; the kernels may have no more
PDF_INDEX_EXCEPTIONS = 92


def ratio(got, ref, scale):
    """largest (|got - ref| - 2^-149) / (2^-24 * scale) over the elements; inf where a zero scale is missed (or a NaN appears)"""
    got, ref, scale = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref) - TINY
        r = np.where(err <= 0, 0.0, np.where(scale > 0, err / (EPS * scale), np.inf))
        r = np.where(np.isfinite(got) & np.isfinite(ref) & np.isfinite(scale), r, np.inf)
    return float(r.max()) if r.size else 0.0


def hold(got, ref, scale, k, what):
    """every element within k * 2^-24 * scale + 2^-149"""
    got = np.asarray(got, np.float64)
    assert got.shape == np.shape(ref), f"{what}: shape {got.shape} != {np.shape(ref)}"
    r = ratio(got, ref, scale)
    print(f"{what}: worst (|got - ref64| - 2^-149) / (2^-24 scale) = {r:.3f}  (K = {k})")
    if not r <= k:
        with np.errstate(all="ignore"):
            bad = ~(np.abs(got - ref) <= k * EPS * np.asarray(scale) + TINY)
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside K={k}; first at {i}: got {got[i]!r}, ref64 {np.asarray(ref)[i]!r}, "
                             f"scale {np.asarray(scale)[i]!r}")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


# =====================================================================================================================
# weights_from_sigma
# =====================================================================================================================
WEIGHTS_T = (1, 63, 64, 65, 256, 257, 300)          # 256 / 257: the backward's register and LDS instantiations
WEIGHTS_N = 64
WEIGHTS_TILED = 65537                               # rays of the lane-per-ray launch (T = 65): the same 64 rows, tiled
WEIGHT_KINDS = ("random", "zero", "zero_width", "saturated", "subnormal", "inf_mid", "overflow_mid", "inf_zero_width", "max_last")


def weights_kind(row):
    return WEIGHT_KINDS[row % len(WEIGHT_KINDS)]


def weights_rows(kind):
    return [r for r in range(WEIGHTS_N) if weights_kind(r) == kind]


# rays whose per-sample depth is +inf or NaN before the last sample, in fp64 too: torch's own fp64 derivative is not finite on (some of) them
WEIGHTS_NONFINITE_ROWS = tuple(weights_rows("inf_mid") + weights_rows("inf_zero_width"))


@functools.lru_cache(maxsize=None)
def weights_case(T):
    """-> dict(rb [64,T+1], sg [64,T], g [64,T], mid): row r is of kind weights_kind(r); `mid` is the sample the non-finite kinds touch."""
    rng = np.random.default_rng(1000 + T)
    N = WEIGHTS_N
    rb = np.sort(rng.uniform(0.2, 30.0, (N, T + 1)), axis=1).astype(F32)
    sg = np.exp(rng.uniform(-6.0, 3.0, (N, T))).astype(F32)
    g = rng.standard_normal((N, T)).astype(F32)
    mid = T // 2
    q = max(T // 4, 1)
    for r in range(N):
        kind = weights_kind(r)
        if kind == "zero":
            sg[r] = 0.0
        elif kind == "zero_width":                          # runs of repeated edges
            for s in range(0, T, 7):
                rb[r, s + 1:min(s + 4, T + 1)] = rb[r, s]
        elif kind == "saturated":                           # optical depth beyond 104 inside the first quarter
            sg[r, :q] = F32(480.0) / (rb[r, q] - rb[r, 0])
        elif kind == "subnormal":                           # the depth climbs evenly to 110: it crosses 87..104, where e^-c is subnormal
            sg[r] = (F32(110.0 / T) / np.maximum(rb[r, 1:] - rb[r, :-1], F32(1e-6))).astype(F32)
        elif kind == "inf_mid":
            sg[r, mid] = np.inf
        elif kind == "overflow_mid":                        # finite operands, product beyond fp32's range
            rb[r, mid + 1:] += F32(4.0)
            sg[r, mid] = F32(3.0e38)
        elif kind == "inf_zero_width":                      # 0 * inf = NaN
            rb[r, mid + 1] = rb[r, mid]
            sg[r, mid] = np.inf
        elif kind == "max_last":
            sg[r, T - 1] = FMAX
    assert (np.diff(rb, axis=1) >= 0).all()
    delta = rb[:, 1:] - rb[:, :-1]
    for r in weights_rows("inf_mid"):
        assert delta[r, mid] > 0
    with np.errstate(all="ignore"):
        for r in weights_rows("overflow_mid"):
            assert np.isinf(delta[r, mid] * sg[r, mid]) and np.isfinite(sg[r, mid])
    for a in (rb, sg, g):
        a.setflags(write=False)
    return dict(rb=rb, sg=sg, g=g, mid=mid, T=T)


@functools.lru_cache(maxsize=None)
def weights_ref(T, last_opaque):
    c = weights_case(T)
    return r64.weights(c["rb"], c["sg"], last_opaque, c["g"])


def weights_has_nan(T, last_opaque):
    """the inf_zero_width rows have ds = NaN at `mid`, unless that is the opaque last sample (whose ds is set to +inf)"""
    return not (last_opaque and T // 2 == T - 1)


def tiled(a, n=WEIGHTS_TILED):
    return np.ascontiguousarray(np.tile(a, (-(-n // a.shape[0]),) + (1,) * (a.ndim - 1))[:n])


def check_weights(T, last_opaque, w, what="weights"):
    """forward: the per-element bar; exact zeros after a mid-ray +inf / NaN; every ray's sum <= 1 + K 2^-24 T"""
    c, ref = weights_case(T), weights_ref(T, last_opaque)
    w = np.asarray(w)
    rows = np.arange(w.shape[0]) % WEIGHTS_N
    assert np.isfinite(w).all(), f"{what}: non-finite weight"
    hold(w, ref["w"][rows], ref["scale_w"][rows], K["weights"], f"{what} T={T} opaque={last_opaque}")
    for kind in ("inf_mid", "overflow_mid", "inf_zero_width"):
        sel = np.isin(rows, weights_rows(kind))
        first = c["mid"] if kind == "inf_zero_width" and weights_has_nan(T, last_opaque) else c["mid"] + 1
        after = w[sel][:, first:]
        assert (after == 0).all(), f"{what} T={T} opaque={last_opaque}: {int((after != 0).sum())} weights after the mid-ray {kind} sample are not 0 (max {after.max() if after.size else 0})"
    sums = w.astype(np.float64).sum(axis=1)
    assert (sums <= 1.0 + K["weights"] * EPS * T).all(), f"{what} T={T} opaque={last_opaque}: a ray's weights sum to {sums.max()} (ray {int(sums.argmax())}, kind {weights_kind(int(sums.argmax()) % WEIGHTS_N)})"


def check_weights_backward(T, last_opaque, gs, what="weights backward"):
    """the per-element bar against the analytic fp64 gradient (which on the rays torch cannot differentiate states the documented behaviour:
    nothing through a NaN weight, nothing through the opaque sample), finite everywhere"""
    c, ref = weights_case(T), weights_ref(T, last_opaque)
    gs = np.asarray(gs)
    rows = np.arange(gs.shape[0]) % WEIGHTS_N
    assert np.isfinite(gs).all(), f"{what}: non-finite gradient"
    hold(gs, ref["gs"][rows], ref["scale_gs"][rows], K["weights_backward"], f"{what} T={T} opaque={last_opaque}")
    if last_opaque:
        assert (gs[:, -1] == 0).all(), f"{what}: the opaque last sample is a constant"
    if weights_has_nan(T, last_opaque):
        sel = np.isin(rows, weights_rows("inf_zero_width"))
        assert (gs[sel][:, c["mid"]:] == 0).all(), f"{what}: gradient through NaN weights"


# =====================================================================================================================
# sample_pdf
# =====================================================================================================================
PDF_SHAPES = ((1, 1), (1, 5), (4, 9), (63, 64), (64, 65), (128, 65), (37, 90), (2047, 33), (2048, 33))
PDF_N = 37
PDF_TILED_SHAPE = (64, 65)
PDF_KINDS = ("random", "zero", "one_hot_first", "one_hot_last", "huge", "zero_width", "equal")
U_FORMS = ("none", "shared", "per_ray")


def pdf_kind(row, T0):
    k = PDF_KINDS[row % len(PDF_KINDS)]
    return "random" if k == "equal" and T0 & (T0 - 1) else k            # exact knots need a power of two


def _knot_row(rng, T0, T):
    """a sorted u row that holds 0, 1, exact knots k / T0 and their fp32 neighbours (as many as fit), the rest uniform draws"""
    ks = sorted({1 % (T0 + 1), T0 // 2, T0 - 1} - {0, T0}) if T0 > 1 else []
    must = [0.0, 1.0] + [k / T0 for k in ks]
    near = [v for k in ks for v in (np.nextafter(F32(k / T0), F32(0)), np.nextafter(F32(k / T0), F32(2)))]
    near += [np.nextafter(F32(0), F32(1)), np.nextafter(F32(1), F32(0))]
    vals = (must + near)[:T] if T >= 2 else [0.5]
    vals = list(vals) + list(rng.uniform(0, 1, max(T - len(vals), 0)))
    return np.sort(np.asarray(vals, F32))


@functools.lru_cache(maxsize=None)
def pdf_case(T0, T):
    """-> dict(bins [37,T0+1], w [37,T0], u_shared [T], u_per_ray [37,T], knots [T]: True where u_shared is an exact knot k / T0)."""
    if T0 == 2048:
        # the (2047, T) case with one more bin of zero width and zero probability (w = -0.01f: w + 0.01f = 0 exactly), so the two cases have
        # the same answer: a mistake at the LDS boundary shows as a mismatch between them
        c = pdf_case(2047, T)
        bins = np.concatenate([c["bins"], c["bins"][:, -1:]], axis=1)
        w = np.concatenate([c["w"], np.full((PDF_N, 1), -F32(0.01), F32)], axis=1)
        out = dict(c, bins=bins, w=w, T0=T0)
        for a in (bins, w):
            a.setflags(write=False)
        return out
    rng = np.random.default_rng(2000 + 31 * T0 + T)
    N = PDF_N
    bins = np.sort(rng.uniform(0, 1, (N, T0 + 1)), axis=1).astype(F32)
    w = (rng.uniform(0, 1, (N, T0)) ** 6).astype(F32)
    for r in range(N):
        kind = pdf_kind(r, T0)
        if kind == "zero":
            w[r] = 0
        elif kind == "one_hot_first":
            w[r] = 0; w[r, 0] = 1
        elif kind == "one_hot_last":
            w[r] = 0; w[r, -1] = 1
        elif kind == "huge":
            w[r] = 0; w[r, T0 // 3] = 1e30
        elif kind == "zero_width":
            for s in range(0, T0, 5):
                bins[r, s + 1:min(s + 3, T0 + 1)] = bins[r, s]
        elif kind == "equal":
            w[r] = 0.25
    u_shared = _knot_row(rng, T0, T)
    jit = (np.linspace(0.5 / T, 1 - 0.5 / T, T)[None] + (rng.uniform(0, 1, (N, T)) - 0.5) / T).astype(F32)      # renderer.py:97-102
    u_per_ray = np.where((np.arange(N) % 2 == 0)[:, None], jit, np.sort(rng.uniform(0, 1, (N, T)), axis=1).astype(F32)).astype(F32)
    steps_back = []
    for r in range(N):
        if pdf_kind(r, T0) == "equal":
            u_per_ray[r] = u_shared
        elif pdf_kind(r, T0) == "zero" and not T0 & (T0 - 1) and T >= 4:
            # a row that steps back by one ulp across a knot (all-zero weights: the cdf is k / T0 exactly), as a perturbed row can when two
            # neighbouring draws are 1 apart: torch.searchsorted looks every element up on its own
            knot = F32(max(T0 // 2, 1) / T0)
            row = np.sort(np.concatenate([rng.uniform(0, 1, T - 2).astype(F32), [knot, knot]]))
            row[int(np.argmax(row == knot)) + 1] = np.nextafter(knot, F32(0))
            u_per_ray[r] = row
            steps_back.append(r)
    # (check_pdf's index rule alone accepts a merge pass that does not step back with u: the knot is one ulp from u, inside K.  What tells it
    # apart is the bit-equality of the wave and lane routes on these rows and the count of index exceptions: both have to stay.)
    back = np.diff(u_per_ray, axis=1) < 0
    assert not back[[r for r in range(N) if r not in steps_back]].any() and (back.sum(axis=1) <= 1).all() and (np.diff(u_shared) >= 0).all()
    assert u_per_ray.min() >= 0
    knots = (u_shared.astype(np.float64) * T0 == np.round(u_shared.astype(np.float64) * T0)) if not T0 & (T0 - 1) else np.zeros(T, bool)
    for a in (bins, w, u_shared, u_per_ray):
        a.setflags(write=False)
    return dict(bins=bins, w=w, u_shared=u_shared, u_per_ray=u_per_ray, knots=knots, T0=T0, T=T)


def pdf_u(case, form):
    return {"none": None, "shared": case["u_shared"], "per_ray": case["u_per_ray"]}[form]


@functools.lru_cache(maxsize=None)
def pdf_ref(T0, T, form):
    c = pdf_case(T0, T)
    u = pdf_u(c, form)
    return r64.sample_pdf(c["bins"], c["w"], r64.linspace_u(T) if u is None else u)


def check_pdf(T0, T, form, out, inds, what="sample_pdf", ref=None):
    """bins to the bar; an index differs from the fp64 one only within K 2^-24 of the knot between them; exact-knot rows exact.
    -> number of differing indices"""
    c = pdf_case(T0, T)
    ref = pdf_ref(T0, T, form) if ref is None else ref
    out = np.asarray(out)
    rows = np.arange(out.shape[0]) % PDF_N
    tag = f"{what} T0={T0} T={T} u={form}"
    hold(out, ref["out"][rows], ref["scale"][rows], K["sample_pdf"], tag)
    if inds is None:
        return 0
    inds = np.asarray(inds)
    if form != "none":          # the cdf is clamped at 1 (renderer.py:94): at u >= 1 every knot is passed, in any precision
        top = np.broadcast_to(pdf_u(c, form), ref["out"].shape)[rows] >= 1
        assert (inds[top] == T0 + 1).all() and np.array_equal(out[top], np.broadcast_to(c["bins"][rows][:, -1:], out.shape)[top]), \
            f"{tag}: u >= 1 must give ind = T0 + 1 and the last edge"
    want = ref["inds"][rows]
    diff = inds != want
    if diff.any():
        cdf = ref["cdf"][rows]
        u = pdf_u(c, form)
        u = np.broadcast_to(np.asarray(r64.linspace_u(T) if u is None else u, np.float64), ref["out"].shape)[rows]
        far = np.where(inds > want, np.take_along_axis(cdf, np.clip(inds - 1, 0, T0), axis=1) - u, u - np.take_along_axis(cdf, np.clip(inds, 0, T0), axis=1))
        worst = float(far[diff].max()) / EPS
        print(f"{tag}: {int(diff.sum())} indices differ from fp64, farthest knot {worst:.3f} * 2^-24 from u")
        assert worst <= K["sample_pdf_knot"], f"{tag}: an index differs from the fp64 index with u {worst:.2f} * 2^-24 from the knot (K = {K['sample_pdf_knot']})"
    if form != "none" and c["knots"].any():
        for r in np.nonzero([pdf_kind(int(q), T0) == "equal" for q in rows])[0]:
            uk = c["u_shared"][c["knots"]].astype(np.float64)
            k = np.round(uk * T0).astype(np.int64)
            assert np.array_equal(inds[r][c["knots"]], k + 1), f"{tag}: ray {r}: u = k/T0 must give ind = k + 1, got {inds[r][c['knots']]} for k = {k}"
            assert np.array_equal(out[r][c["knots"]], c["bins"][r % PDF_N][k]), f"{tag}: ray {r}: u = k/T0 must give bins[k] exactly"
    return int(diff.sum())


# =====================================================================================================================
# spacing functions and sample_positions
# =====================================================================================================================
def _ulps(x, n):
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf) if n > 0 else F32(-np.inf))
    return x


@functools.lru_cache(maxsize=None)
def spacing_points():
    """-> (x for spacing_fn, x for spacing_inv, their branch points)"""
    rng = np.random.default_rng(3000)
    sub = [1e-45, 3e-45, 1e-40, 5.8e-39, 1.1754942e-38, 1.1754944e-38]
    fn = np.concatenate([[0.0], sub, [_ulps(1, -1), 1.0, _ulps(1, 1), _ulps(0.5, -1), 0.5, _ulps(0.5, 1), 1e9, 0.05, 2.0, 128.0],
                         np.exp(rng.uniform(-20, 20, 400))]).astype(F32)
    inv = np.concatenate([[0.0], sub, [_ulps(0.5, -1), 0.5, _ulps(0.5, 1), _ulps(1, -1), _ulps(1, -2), 1 - 2.0 ** -20, 0.25, 0.75],
                          rng.uniform(0, 1, 400) ** 0.25, 1 - np.exp(rng.uniform(-16, -1, 200))]).astype(F32)
    inv = inv[inv <= _ulps(1, -1)]
    return fn, inv, {"fn": (F32(1.0), F32(0.5)), "inv": (F32(0.5), F32(1.0))}


def near_far_f32(rays_o, rays_d, aabb, min_near):
    """renderer.py:122-139 in numpy float32"""
    o, d, ab = np.asarray(rays_o, F32), np.asarray(rays_d, F32), np.asarray(aabb, F32)
    with np.errstate(all="ignore"):
        den = d + F32(1e-15)
        tmin, tmax = (ab[:3] - o) / den, (ab[3:] - o) / den
        near = np.where(tmin < tmax, tmin, tmax).max(axis=1, keepdims=True)
        far = np.where(tmin > tmax, tmin, tmax).min(axis=1, keepdims=True)
    miss = far < near
    near[miss] = 1e9
    far[miss] = 1e9
    return np.maximum(near, F32(min_near)).astype(F32), far.astype(F32)


POS_N = 128
POS_T = (1, 48)
POS_BOUNDS = (0.0, 2.0, 1.5)
POS_MIN_NEAR = 0.05
POS_AABBS = ((-128.0,) * 3 + (128.0,) * 3, (-1.0,) * 3 + (1.0,) * 3)


@functools.lru_cache(maxsize=None)
def pos_case(T):
    """-> dict(o, d [128,3], aabb_of_ray [128] (index into POS_AABBS), near, far [128,1], bins [128,T+1], miss [128])"""
    rng = np.random.default_rng(4000 + T)
    N = POS_N
    o = rng.uniform(-0.9, 0.9, (N, 3))
    o[::4] = rng.uniform(-300, 300, (N // 4, 3))                       # outside both boxes (some outside the large one)
    o[1::8] = rng.uniform(1.5, 3.0, (N // 8, 3)) * rng.choice([-1, 1], (N // 8, 3))
    d = rng.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[2::16, 0] = 0.0                                                  # a zero direction component
    d[5::16, 2] = 0.0
    o, d = o.astype(F32), d.astype(F32)
    which = (np.arange(N) >= N // 2).astype(np.int64)
    near, far = np.empty((N, 1), F32), np.empty((N, 1), F32)
    for k, ab in enumerate(POS_AABBS):
        n_, f_ = near_far_f32(o[which == k], d[which == k], ab, POS_MIN_NEAR)
        near[which == k], far[which == k] = n_, f_
    bins = np.sort(rng.uniform(0, 1, (N, T + 1)), axis=1).astype(F32)
    bins[:, 0] = 0.0
    bins[:, -1] = 1.0
    if T >= 8:
        bins[::3, 3:6] = bins[::3, 3:4]                                # repeated edges
        bins[1::5, 1] = 0.0
        bins[1::5, -2] = 1.0
    # the rays left out of the fp64 comparison are found from the reference, not from near: those where fp32 rounding may move an edge by more
    # than the edge itself (2^-24 * scale >= |real_bins|; spacing(1e9) rounds to 1 in fp32).  The tests assert that they are the rays with near == 1e9.
    ref = r64.sample_positions(o, d, near, far, bins, False, 0.0)
    miss = (EPS * ref["scale_rb"] >= np.abs(ref["real_bins"])).any(axis=1)
    assert miss.any() and (~miss).sum() > N // 3
    for a in (o, d, near, far, bins):
        a.setflags(write=False)
    return dict(o=o, d=d, which=which, near=near, far=far, bins=bins, miss=miss, T=T)


@functools.lru_cache(maxsize=None)
def pos_ref(T, contract, bound):
    c = pos_case(T)
    return r64.sample_positions(c["o"], c["d"], c["near"], c["far"], c["bins"], contract, bound)


def check_positions(T, contract, bound, real_bins, rays_t, xyzs, what="sample_positions"):
    c, ref = pos_case(T), pos_ref(T, contract, bound)
    hit = ~c["miss"]
    tag = f"{what} T={T} contract={contract} bound={bound}"
    hold(np.asarray(real_bins)[hit], ref["real_bins"][hit], ref["scale_rb"][hit], K["real_bins"], tag + " real_bins")
    hold(np.asarray(rays_t)[hit], ref["rays_t"][hit], ref["scale_t"][hit], K["rays_t"], tag + " rays_t")
    hold(np.asarray(xyzs)[hit], ref["xyzs"][hit], ref["scale_x"][hit], K["xyzs"], tag + " xyzs")
    # rays that miss the box: spacing(1e9) rounds to 1 in fp32, so x is 1 - 2^-24 or 1 and 1 / (2 - 2x) is 2^23 or +inf
    rb = np.asarray(real_bins)[c["miss"]]
    assert not np.isnan(rb).any() and (rb >= 2.0 ** 23).all(), f"{tag}: real_bins of rays that miss the box: min {rb.min()}, NaNs {int(np.isnan(rb).sum())}"


# =====================================================================================================================
# composite
# =====================================================================================================================
COMPOSITE_SHAPES = ((257, 1, 1), (257, 33, 7), (65, 300, 31), (257, 33, 0))         # K = 0: the 2-D `values` form


@functools.lru_cache(maxsize=None)
def composite_case(N, T, Kc):
    rng = np.random.default_rng(5000 + N + 7 * T + 13 * Kc)
    k = max(Kc, 1)
    w = (rng.uniform(0, 1, (N, T)) ** 3).astype(F32)
    w[rng.uniform(0, 1, (N, T)) < 0.2] = 0.0
    v = (10.0 ** rng.uniform(-4, 4, (N, T, k))).astype(F32)
    v *= np.where((np.arange(T) % 2 == 0)[None, :, None], 1, -1).astype(F32)    # alternating signs: the plain sum cancels
    g = rng.standard_normal((N, k)).astype(F32)
    for a in (w, v, g):
        a.setflags(write=False)
    return dict(w=w, v=v, g=g, two_d=Kc == 0)


@functools.lru_cache(maxsize=None)
def composite_ref(N, T, Kc):
    c = composite_case(N, T, Kc)
    return r64.composite(c["w"], c["v"], c["g"])


def check_composite(N, T, Kc, out, gw, gv, what="composite"):
    ref = composite_ref(N, T, Kc)
    tag = f"{what} N={N} T={T} K={Kc}"
    shape = ref["out"].shape
    hold(np.asarray(out).reshape(shape), ref["out"], ref["scale_out"], K["composite"], tag + " out")
    hold(np.asarray(gw), ref["gw"], ref["scale_gw"], K["composite_gw"], tag + " d/dw")
    hold(np.asarray(gv).reshape(ref["gv"].shape), ref["gv"], ref["scale_gv"], K["composite_gv"], tag + " d/dvalues")


# =====================================================================================================================
# proposal loss
# =====================================================================================================================
PROPOSAL_SHAPES = ((1, 1), (5, 1), (33, 17), (512, 512), (513, 64), (64, 513))       # (T, Tr); beyond 512 either way: the workspace route
PROPOSAL_N = 67
PROPOSAL_KINDS = ("straddle", "below", "above", "shared", "zero_width", "zero_rw", "covered", "zero_w")


def proposal_kind(row):
    return PROPOSAL_KINDS[row % len(PROPOSAL_KINDS)]


@functools.lru_cache(maxsize=None)
def proposal_case(T, Tr):
    """-> dict(b [67,T+1], w [67,T] of the proposal stage, rb [67,Tr+1], rw [67,Tr] of the final stage)"""
    rng = np.random.default_rng(6000 + 17 * T + Tr)
    N = PROPOSAL_N
    b = np.sort(rng.uniform(0.2, 0.8, (N, T + 1)), axis=1).astype(F32)
    rb = np.sort(rng.uniform(0.0, 1.0, (N, Tr + 1)), axis=1).astype(F32)
    w = (rng.uniform(0, 1, (N, T)) ** 3).astype(F32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(F32)
    rw = (rng.uniform(0, 1, (N, Tr)) ** 3).astype(F32)
    rw = (rw / rw.sum(axis=1, keepdims=True)).astype(F32)
    for r in range(N):
        kind = proposal_kind(r)
        if kind == "below":
            rb[r] = np.sort(rng.uniform(0.0, 0.15, Tr + 1)).astype(F32)
        elif kind == "above":
            rb[r] = np.sort(rng.uniform(0.85, 1.0, Tr + 1)).astype(F32)
        elif kind == "shared":                               # every other final-stage edge is a proposal edge: ties under right=True
            rb[r, ::2] = b[r, rng.integers(0, T + 1, rb[r, ::2].shape[0])]
            rb[r] = np.sort(rb[r])
        elif kind == "zero_width":
            for s in range(0, T, 4):
                b[r, s + 1:min(s + 3, T + 1)] = b[r, s]
        elif kind == "zero_rw":
            rw[r, ::2] = 0.0
        elif kind == "covered":                              # the final stage's edges are proposal edges and its weights the proposal's sums
            idx = np.sort(np.concatenate([[0, T], rng.integers(0, T + 1, Tr - 1)]))
            rb[r] = b[r, idx]
            cum = np.concatenate([[0.0], np.cumsum(w[r].astype(np.float64))])
            rw[r] = (cum[idx[1:]] - cum[idx[:-1]]).astype(F32)
        elif kind == "zero_w":
            w[r] = 0.0
    for a in (b, w, rb, rw):
        a.setflags(write=False)
    return dict(b=b, w=w, rb=rb, rw=rw, T=T, Tr=Tr)


@functools.lru_cache(maxsize=None)
def proposal_ref(T, Tr):
    c = proposal_case(T, Tr)
    return r64.proposal_loss_stage(c["b"], c["w"], c["rb"], c["rw"])


def check_proposal(T, Tr, per_ray, gw, what="proposal loss"):
    """per_ray [67] = sum_j term_j and gw [67,T] = d per_ray / d w"""
    ref = proposal_ref(T, Tr)
    tag = f"{what} T={T} Tr={Tr}"
    if per_ray is not None:
        hold(np.asarray(per_ray), ref["per_ray"], ref["scale_per_ray"], K["proposal"], tag + " per ray")
    if gw is not None:
        hold(np.asarray(gw), ref["gw"], ref["scale_gw"], K["proposal_gw"], tag + " d/dw")


def proposal_mean_ref(T, Tr):
    """the public form: loss = per_ray.sum() / (N Tr) and its gradient, each with one more sum / division to round
    -> (mean [1], its scale, d mean / d w, its scale)"""
    ref = proposal_ref(T, Tr)
    n = float(PROPOSAL_N * Tr)
    mean = ref["per_ray"].sum() / n
    return np.asarray([mean]), np.asarray([ref["scale_per_ray"].sum() / n + mean]), ref["gw"] / n, (ref["scale_gw"] + np.abs(ref["gw"])) / n


def check_proposal_mean(T, Tr, loss, gw_mean, what="proposal loss (mean)"):
    mean, scale_mean, gw, scale_gw = proposal_mean_ref(T, Tr)
    tag = f"{what} T={T} Tr={Tr}"
    hold(np.asarray(loss, np.float64).reshape(1), mean, scale_mean, K["proposal"], tag + " value")
    hold(np.asarray(gw_mean), gw, scale_gw, K["proposal_gw"], tag + " d/dw")
