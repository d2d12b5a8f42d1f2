"""The stand-alone ray operators of raymarch.hip against plain fp64 references (raymarch_ref64.py) at their edges and on every route:
weights_from_sigma forward (one wave per ray / one lane per ray) and backward (registers / LDS), sample_pdf (both routes, the LDS
boundary, exact knots), the spacing functions, sample_positions, composite and the proposal loss (LDS / workspace).

Every output element is held to |got - ref64| <= K * 2^-24 * scale + 2^-149; cases, scales' constants K and the comparison functions are
those of raymarch_cases.py, which test_raymarch_ref64.py pins and measures without a GPU.  Every operator is called twice: equal bits.
"""
import numpy as np
import pytest
import torch

import raymarch_cases as rc
import raymarch_ref64 as r64

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice(fn):
    """fn() -> tensor or tuple of tensors, called twice: the same bits"""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert same_bits(x, y), "two calls differ"
    return a


# ---------------------------------------------------------------------------------------------------------------------
# weights_from_sigma
# ---------------------------------------------------------------------------------------------------------------------
def run_weights(gpu, rb, sg, g, opaque):
    from sanerf_hq_amd import raymarching as rm

    def once():
        s = T(sg, gpu).requires_grad_(True)
        w = rm.weights_from_sigma(T(rb, gpu), s, opaque)
        w.backward(T(g, gpu))
        return w.detach(), s.grad
    w, gs = twice(once)
    assert same_bits(w, rm.weights_from_sigma(T(rb, gpu), T(sg, gpu), opaque)), "the no-grad call differs"
    return w, gs


@pytest.mark.parametrize("opaque", [True, False])
@pytest.mark.parametrize("T_", rc.WEIGHTS_T)
def test_weights_one_wave_per_ray_forward_and_backward(gpu, T_, opaque):
    """64 rays: the forward's wave-per-ray kernel; the backward's register (T <= 256) or LDS (257, 300) instantiation."""
    c = rc.weights_case(T_)
    w, gs = run_weights(gpu, c["rb"], c["sg"], c["g"], opaque)
    rc.check_weights(T_, opaque, npy(w))
    rc.check_weights_backward(T_, opaque, npy(gs))


@pytest.mark.parametrize("opaque", [True, False])
def test_weights_one_lane_per_ray_equals_one_wave_per_ray(gpu, opaque):
    """the same 64 rows tiled to 65 537 rays (T = 65) take the lane-per-ray forward: bit-equal row for row, the non-finite rows included"""
    T_ = 65
    c = rc.weights_case(T_)
    small_w, small_gs = run_weights(gpu, c["rb"], c["sg"], c["g"], opaque)
    w, gs = run_weights(gpu, rc.tiled(c["rb"]), rc.tiled(c["sg"]), rc.tiled(c["g"]), opaque)
    assert w.shape[0] == rc.WEIGHTS_TILED > 65536
    rc.check_weights(T_, opaque, npy(w), "weights (lane per ray)")
    rc.check_weights_backward(T_, opaque, npy(gs), "weights backward (65 537 rays)")
    rows = torch.arange(w.shape[0], device=gpu) % rc.WEIGHTS_N
    differ = (w.view(torch.int32) != small_w[rows].view(torch.int32)).any(dim=1)
    kinds = sorted({rc.weights_kind(int(r) % rc.WEIGHTS_N) for r in torch.nonzero(differ)[:64, 0]})
    assert not bool(differ.any()), f"{int(differ.sum())} rays differ between the two forward routes, kinds {kinds}"
    assert same_bits(gs, small_gs[rows])


def test_weights_backward_registers_and_lds_give_the_same_bits(gpu):
    """T = 257 takes the LDS instantiation.  A 257-sample ray that is a 256-sample ray plus one empty sample (sigma = 0, upstream 0) has
    the same first 256 gradients: the same operations on the same values."""
    c = rc.weights_case(256)
    _, short = run_weights(gpu, c["rb"], c["sg"], c["g"], False)
    rb = np.concatenate([c["rb"], c["rb"][:, -1:] + np.float32(1)], axis=1)
    zero = np.zeros((rc.WEIGHTS_N, 1), np.float32)
    _, long = run_weights(gpu, rb, np.concatenate([c["sg"], zero], axis=1), np.concatenate([c["g"], zero], axis=1), False)
    assert same_bits(long[:, :256].contiguous(), short)
    assert float(long[:, 256].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# sample_pdf
# ---------------------------------------------------------------------------------------------------------------------
def run_pdf(gpu, bins, w, T_, u):
    from sanerf_hq_amd import raymarching as rm
    ut = None if u is None else T(u, gpu)
    return twice(lambda: rm.sample_pdf(T(bins, gpu), T(w, gpu), T_, return_inds=True, u=ut))


@pytest.fixture(scope="module")
def pdf_runs(gpu):
    """{(T0, T, form): (out, inds)} of every case, N = 37 rays: one wave per ray up to T0 = 2047, one lane per ray at T0 = 2048"""
    runs = {}
    for T0, T_ in rc.PDF_SHAPES:
        c = rc.pdf_case(T0, T_)
        for form in rc.U_FORMS:
            out, inds = run_pdf(gpu, c["bins"], c["w"], T_, rc.pdf_u(c, form))
            runs[T0, T_, form] = (npy(out), npy(inds))
    return runs


@pytest.mark.parametrize("form", rc.U_FORMS)
@pytest.mark.parametrize("T0,T_", rc.PDF_SHAPES)
def test_sample_pdf_bins_and_indices(pdf_runs, T0, T_, form):
    rc.check_pdf(T0, T_, form, *pdf_runs[T0, T_, form])


def test_sample_pdf_index_exceptions_are_no_more_than_the_oracles(pdf_runs):
    total = sum(rc.check_pdf(T0, T_, form, out, inds) for (T0, T_, form), (out, inds) in pdf_runs.items())
    print(f"{total} indices differ from fp64 over all cases (the oracle: {rc.PDF_INDEX_EXCEPTIONS})")
    assert total <= rc.PDF_INDEX_EXCEPTIONS


@pytest.mark.parametrize("form", rc.U_FORMS)
def test_sample_pdf_lds_boundary_cases_meet_each_others_reference(pdf_runs, form):
    """T0 = 2047 is the largest one-wave-per-ray launch (64 KiB of LDS), T0 = 2048 runs one lane per ray; the second case is the first
    with one more bin of zero width and zero probability, so each answer meets the other's reference"""
    a, b = pdf_runs[2047, 33, form], pdf_runs[2048, 33, form]
    rc.check_pdf(2047, 33, form, a[0], None, "sample_pdf (2047 against the 2048 reference)", ref=rc.pdf_ref(2048, 33, form))
    rc.check_pdf(2048, 33, form, b[0], None, "sample_pdf (2048 against the 2047 reference)", ref=rc.pdf_ref(2047, 33, form))


@pytest.mark.parametrize("form", rc.U_FORMS)
def test_sample_pdf_one_lane_per_ray_equals_one_wave_per_ray(gpu, pdf_runs, form):
    T0, T_ = rc.PDF_TILED_SHAPE
    c = rc.pdf_case(T0, T_)
    u = rc.pdf_u(c, form)
    n = rc.WEIGHTS_TILED
    out, inds = run_pdf(gpu, rc.tiled(c["bins"], n), rc.tiled(c["w"], n), T_, rc.tiled(u, n) if form == "per_ray" else u)
    rows = np.arange(n) % rc.PDF_N
    small_out, small_inds = pdf_runs[T0, T_, form]
    out, inds = npy(out), npy(inds)
    assert np.array_equal(rc.bits(out), rc.bits(small_out)[rows]) and np.array_equal(inds, small_inds[rows])
    rc.check_pdf(T0, T_, form, out, inds, "sample_pdf (lane per ray)")


# ---------------------------------------------------------------------------------------------------------------------
# spacing functions, sample_positions
# ---------------------------------------------------------------------------------------------------------------------
def test_spacing_ops_within_one_ulp_and_exact_at_the_branch_points(gpu):
    from sanerf_hq_amd import _lib
    fn, inv, branch = rc.spacing_points()
    for op, x, f64, pts in ((2, fn, r64.spacing, branch["fn"]), (3, inv, r64.spacing_inv, branch["inv"])):
        xt = T(x, gpu)

        def once():
            yt = torch.empty_like(xt)
            _lib.check(_lib.lib().sn_debug_eval(op, xt.data_ptr(), None, x.size, yt.data_ptr(), _lib.stream()), "debug_eval")
            return yt
        got = npy(twice(once))
        want = f64(x).astype(np.float32)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert np.isfinite(got).all() and ulps.max() <= 1, f"op {op}: {int(ulps.max())} ulps at x = {x[int(ulps.argmax())]!r}"
        at = np.isin(x, pts)
        assert np.array_equal(got[at], want[at]), f"op {op}: not exact at the branch points"


@pytest.mark.parametrize("bound", rc.POS_BOUNDS)
@pytest.mark.parametrize("contract", [True, False])
@pytest.mark.parametrize("T_", rc.POS_T)
def test_sample_positions(gpu, T_, contract, bound):
    from sanerf_hq_amd import raymarching as rm
    c = rc.pos_case(T_)
    near_dev = np.empty_like(c["near"])
    for k, ab in enumerate(rc.POS_AABBS):                  # the case's nears / fars are what near_far_from_aabb gives
        sel = c["which"] == k
        near, far = rm.near_far_from_aabb(T(c["o"][sel], gpu), T(c["d"][sel], gpu), torch.tensor(ab), rc.POS_MIN_NEAR)
        assert np.array_equal(npy(near), c["near"][sel]) and np.array_equal(npy(far), c["far"][sel])
        near_dev[sel] = npy(near)
    rb, t, x = twice(lambda: rm.sample_positions(T(c["o"], gpu), T(c["d"], gpu), T(c["near"], gpu), T(c["far"], gpu), T(c["bins"], gpu),
                                                 contract=contract, grid_bound=bound))
    # c["miss"]: the rays whose fp64 condition scale puts them beyond fp32 (raymarch_cases.pos_case) -- exactly those the kernel reports as missing
    assert np.array_equal(c["miss"], near_dev[:, 0] == np.float32(1e9)), "the rays left out are those that miss the box"
    rc.check_positions(T_, contract, bound, npy(rb), npy(t), npy(x))


# ---------------------------------------------------------------------------------------------------------------------
# composite
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T_,Kc", rc.COMPOSITE_SHAPES)
def test_composite_value_and_both_gradients(gpu, N, T_, Kc):
    from sanerf_hq_amd import raymarching as rm
    c = rc.composite_case(N, T_, Kc)
    v_np, g_np = (c["v"][:, :, 0], c["g"][:, 0]) if c["two_d"] else (c["v"], c["g"])

    def once():
        w, v = T(c["w"], gpu).requires_grad_(True), T(v_np, gpu).requires_grad_(True)
        out = rm.composite(w, v)
        out.backward(T(g_np, gpu))
        return out.detach(), w.grad, v.grad
    out, gw, gv = twice(once)
    assert out.shape == ((N,) if c["two_d"] else (N, Kc))
    rc.check_composite(N, T_, Kc, npy(out), npy(gw), npy(gv))


# ---------------------------------------------------------------------------------------------------------------------
# proposal loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_,Tr", rc.PROPOSAL_SHAPES)
def test_proposal_loss_value_and_gradient(gpu, T_, Tr):
    """per ray through the kernel's own entry point, then the two public forms (one stage; all stages in one node): LDS route up to 512
    samples on either side, the workspace route beyond"""
    from sanerf_hq_amd import _lib, raymarching as rm
    from sanerf_hq_amd.raymarching import march
    c = rc.proposal_case(T_, Tr)
    b, rb, rw = T(c["b"], gpu), T(c["rb"], gpu), T(c["rw"], gpu)

    def kernel():
        w = T(c["w"], gpu)
        per_ray, gw = torch.empty(rc.PROPOSAL_N, device=gpu), torch.empty_like(w)
        march._proposal_loss_launch(b, w, rb, rw, 1.0, None, _lib.dev(per_ray, "loss_per_ray"), None, "proposal_loss")
        march._proposal_loss_launch(b, w, rb, rw, 1.0, None, None, _lib.dev(gw, "grad_weights"), "proposal_loss_backward")
        return per_ray, gw
    per_ray, gw = twice(kernel)
    rc.check_proposal(T_, Tr, npy(per_ray), npy(gw))

    def stage():
        w = T(c["w"], gpu).requires_grad_(True)
        loss = rm.proposal_loss_stage(b, w, rb, rw)
        loss.backward()
        return loss.detach().reshape(1), w.grad

    def all_stages():
        w = T(c["w"], gpu).requires_grad_(True)
        loss = rm.proposal_loss_all([b, rb], [w, rw])
        loss.backward()
        return loss.detach().reshape(1), w.grad
    l1, g1 = twice(stage)
    l2, g2 = twice(all_stages)
    rc.check_proposal_mean(T_, Tr, npy(l1), npy(g1), "proposal_loss_stage")
    rc.check_proposal_mean(T_, Tr, npy(l2), npy(g2), "proposal_loss_all")
    _, scale_mean, _, scale_gw = rc.proposal_mean_ref(T_, Tr)
    rc.hold(npy(l1), npy(l2).astype(np.float64), scale_mean, rc.K["proposal"], "proposal_loss_stage against proposal_loss_all, value")
    rc.hold(npy(g1), npy(g2).astype(np.float64), scale_gw, rc.K["proposal_gw"], "proposal_loss_stage against proposal_loss_all, d/dw")
