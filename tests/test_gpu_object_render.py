"""GPU: render a segmented object alone -- the per-sample label kernel (sn_rm_mask_point_labels), the gated re-integration
(sn_rm_object_composite) and NeRFRenderer.render_object -- against the fp64 statement in tests/object_ref64.py."""
import pytest
import torch

import object_cases as oc
import object_ref64 as oref
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu


def _to(gpu, *ts):
    return [t.to(gpu) if torch.is_tensor(t) else t for t in ts]


# ---- labels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,K,L", oc.LABEL_CASES)
def test_point_labels_against_their_own_logits_and_fp64(gpu, N, T, K, L):
    from sanerf_hq_amd import raymarching as rm
    enc, mlp, xyz, extra, live = oc.label_case(N, T, K, L)
    ref = oc.label_ref(N, T, K, L)
    enc_g, mlp_g = enc.to(gpu), mlp.to(gpu)
    xyz_g, extra_g, live_g = _to(gpu, xyz, extra, live)
    assert rm.mask_point_labels_fusable(enc_g, mlp_g, T, oc.E)
    labels, logits = rm.mask_point_labels(live_g, xyz_g, extra_g, enc_g, mlp_g, 1.0, want_logits=True)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (N, T) and tuple(logits.shape) == (N, T, K)
    labels_c, logits_c = labels.cpu(), logits.cpu()
    skipped = oref.skipped_tiles(live)
    assert skipped.any() and ((live == 0) & ~skipped).any(), "the case must have skipped tiles AND evaluated samples with y == 0"
    # (a) the lowest-index argmax of the kernel's own logits, exactly; 255 exactly on the skipped tiles, and only where y == 0
    assert torch.equal(labels_c[~skipped].long(), oref.labels_from_logits(logits_c)[~skipped])
    assert torch.equal(labels_c == oref.LABEL_SKIPPED, skipped) and (live[labels_c == oref.LABEL_SKIPPED] == 0).all()
    assert (logits_c[skipped] == 0).all() and torch.isfinite(logits_c).all()
    # (b) the kernel's logits against the fp64 perceptron on the fp64 grid encoding
    err = float((logits_c.double() - ref["logits"])[~skipped].abs().max())
    print(f"labels {N}x{T} K={K} L={L}: max |logit - ref64| = {err:.3e} (tau = {ref['tau']:.3e})")
    assert err <= ref["tau"]
    # (c) where the fp64 margin exceeds 2 tau the labels are the fp64 labels; the margin leaves out at most 2 % of the evaluated samples
    sure = ~skipped & (ref["margin"] > 2 * ref["tau"])
    share = 1.0 - float(sure.sum()) / float((~skipped).sum())
    print(f"  left out by the margin: {share:.4%}")
    assert share <= oc.MARGIN_SHARE_MAX
    assert torch.equal(labels_c[sure].long(), ref["labels"][sure])
    # (d) two calls give equal bits; production form (no logits) gives the same labels
    labels2, logits2 = rm.mask_point_labels(live_g, xyz_g, extra_g, enc_g, mlp_g, 1.0, want_logits=True)
    assert torch.equal(labels, labels2) and torch.equal(logits, logits2)
    assert torch.equal(labels, rm.mask_point_labels(live_g, xyz_g, extra_g, enc_g, mlp_g, 1.0))


@pytest.mark.parametrize("N,T,K,L", oc.LABEL_CASES)
def test_mask_head_keeps_its_route_and_its_bits(gpu, experiments_build, N, T, K, L):
    """(e) sn_rm_mask_head still launches the compositing instantiation of k_mask16: the existing same-box A/B against k_mlp_wide_j<3>
    (sn_debug_set("mask_head16", 0), experiments builds) with its existing 2e-6 bound, and equal bits from call to call."""
    from sanerf_hq_amd import _lib, raymarching as rm
    enc, mlp, xyz, extra, live = oc.label_case(N, T, K, L)
    enc_g, mlp_g = enc.to(gpu), mlp.to(gpu)
    xyz_g, extra_g, w = _to(gpu, xyz, extra, live)
    b = rm.mask_head(w, xyz_g, extra_g, enc_g, mlp_g, 1.0).clone()
    try:
        _lib.check(_lib.lib().sn_debug_set(b"mask_head16", 0), "debug_set")
        a = rm.mask_head(w, xyz_g, extra_g, enc_g, mlp_g, 1.0).clone()
    finally:
        _lib.check(_lib.lib().sn_debug_set(b"mask_head16", 8), "debug_set")
    assert torch.isfinite(b).all() and float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max()))
    assert torch.equal(b, rm.mask_head(w, xyz_g, extra_g, enc_g, mlp_g, 1.0))


def test_mask_head_composites_the_label_kernels_logits(gpu):
    """The two instantiations of k_mask16 share everything in front of the epilogue: sum_t w logits of the label instantiation's logits is
    the compositing instantiation's output up to the rounding of the T-term sum (fp64 sum of the fp32 logits, (T + 2) u of the mass)."""
    from sanerf_hq_amd import raymarching as rm
    N, T, K, L = oc.LABEL_CASES[1]
    enc, mlp, xyz, extra, _ = oc.label_case(N, T, K, L)
    enc_g, mlp_g = enc.to(gpu), mlp.to(gpu)
    xyz_g, extra_g = _to(gpu, xyz, extra)
    w = torch.rand(N, T, generator=torch.Generator().manual_seed(5)).to(gpu) + 0.1
    _, logits = rm.mask_point_labels(w, xyz_g, extra_g, enc_g, mlp_g, 1.0, want_logits=True)
    out = rm.mask_head(w, xyz_g, extra_g, enc_g, mlp_g, 1.0)
    terms = w.double()[:, :, None] * logits.double()
    assert ((out.double() - terms.sum(1)).abs() <= (T + 2) * oref.U * terms.abs().sum(1)).all()


# ---- composite ---------------------------------------------------------------------------------------------------------------------
def _within(got, ref, bound, what):
    bad = (got.double().cpu() - ref).abs() > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} values beyond the bound, worst excess {float(((got.double().cpu() - ref).abs() - bound).max()):.3e}"


@pytest.mark.parametrize("T", [4, 32, 128])
@pytest.mark.parametrize("N", [1, 33, 1000])
def test_object_composite_against_fp64(gpu, N, T):
    from sanerf_hq_amd import raymarching as rm
    sig, rb, geo, rd, labels = [t[:N] for t in oc.composite_case(T)]
    sig_g, rb_g, geo_g, rd_g, lab_g = _to(gpu, sig, rb, geo, rd, labels)
    allk = (1 << oc.COMPOSITE_K) - 1
    for keep in (0, allk, 0b01000):
        for invert in (False, True):
            for last in (False, True):
                ws, depth, f, w = rm.object_composite(lab_g, sig_g, rb_g, geo_g, rd_g, keep, invert, last, want_weights=True)
                ref = oref.object_ref64(sig, rb, geo, rd, keep, invert, last, labels=labels)
                what = f"N={N} T={T} keep={keep:#b} invert={invert} last={last}"
                assert torch.isfinite(w).all() and torch.isfinite(f).all(), what
                _within(w, ref["weights"], ref["weights_bound"], what + " weights")
                _within(ws, ref["weights_sum"], ref["weights_sum_bound"], what + " weights_sum")
                _within(depth, ref["depth"], ref["depth_bound"], what + " depth")
                _within(f, ref["f_image"], ref["f_image_bound"], what + " f_image")
                ws2, depth2, f2 = rm.object_composite(lab_g, sig_g, rb_g, geo_g, rd_g, keep, invert, last)
                assert torch.equal(ws, ws2) and torch.equal(depth, depth2) and torch.equal(f, f2)
                if keep == 0 and not invert:
                    assert (ws == 0).all() and (depth == 0).all() and (f == 0).all() and (w == 0).all()
    if N >= 2:      # the gated-away occluder of ray 1 (sigma = 1e30, label 3): the samples behind it carry weight although the plain weights are 0
        w = rm.object_composite(lab_g, sig_g, rb_g, geo_g, rd_g, allk & ~0b01000, False, False, want_weights=True)[3]
        plain = oref.plain_weights64(sig, rb, False)
        assert (plain[1, 2:] == 0).all() and float(w[1, 2:].sum()) > 0 and float(w[1, 1]) == 0


@pytest.mark.parametrize("T", [4, 32, 128])
def test_object_composite_does_not_depend_on_the_number_of_rays(gpu, T):
    """N = 1, 33 and 1000 give equal bits for the rays they share: the order of every sum is a function of T alone."""
    from sanerf_hq_amd import raymarching as rm
    case = oc.composite_case(T)
    outs = {}
    for N in (1, 33, 1000):
        sig_g, rb_g, geo_g, rd_g, lab_g = _to(gpu, *[t[:N] for t in case])
        outs[N] = rm.object_composite(lab_g, sig_g, rb_g, geo_g, rd_g, 0b10110, False, True, want_weights=True)
    for N in (1, 33):
        for a, b in zip(outs[N], outs[1000]):
            assert torch.equal(a, b[:N])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]
H, W = 20, 24


def _model(gpu, n_inst=2):
    """The reference-shaped field with the mask head only (no SAM head: render() and render_object() then share one render plan)."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)                      # (n_inst != 2: the last mask layer has no synthetic parameters and keeps this seeded init)
    model = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=n_inst))
    own = model.state_dict()
    sd = {k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}
    assert any(k.startswith("m_grid") for k in sd) and any(k.startswith("mask_mlp") for k in sd)
    model.load_state_dict(sd, strict=False)
    return model.to(gpu).eval()


def _rays(gpu):
    from sanerf_hq_amd import raymarching as rm, synth
    return rm.generate_rays(synth.orbit_pose(1.0, 20.0, 30.0), synth.pinhole_intrinsics(H, W), H, W, device=gpu)


def _by_hand(model, ro, rd, keep, invert, bg):
    """render_object's own operators, called one by one."""
    from sanerf_hq_amd import raymarching as rm
    last_opaque = model.opt.background == "last_sample"
    out = rm.render_rays(model._get_plan(), ro, rd, bg_color=bg, want=["xyzs_last", "geo_feat_last", "sigmas_last", "bins_last"])
    k = len(STEPS) - 1
    nears, fars = rm.near_far_from_aabb(ro, rd, model.aabb_infer, model.min_near)
    real_bins = rm.sample_positions(ro, rd, nears, fars, out[f"bins{k}"], contract=model.opt.contract)[0]
    sig, geo = out[f"sigmas{k}"], out["geo_feat_last"]
    live = (real_bins[:, 1:] - real_bins[:, :-1]) * sig
    if last_opaque:
        live[:, -1] = 1.0
    labels, logits = rm.mask_point_labels(live, out["xyzs_last"], geo, model.m_grid, model.mask_mlp[0], model.bound, want_logits=True)
    ws, depth, f = rm.object_composite(labels, sig, real_bins, geo, rd, keep, invert, last_opaque)
    image = model.view_mlp.forward_sigmoid_bg(f, ws, bg)
    return dict(image=out["image"], depth=out["depth"], weights_sum=out["weights_sum"], object_image=image, object_depth=depth,
                object_weights_sum=ws), dict(labels=labels, logits=logits, sig=sig, real_bins=real_bins, geo=geo, live=live)


@pytest.mark.parametrize("background", ["last_sample", "white"])
def test_render_object_end_to_end(gpu, background):
    from sanerf_hq_amd import raymarching as rm
    model = _model(gpu)
    model.opt.background = background
    model.invalidate_render_plan()
    ro, rd = _rays(gpu)
    N, bg = ro.shape[0], 0.25
    with torch.no_grad():
        res = model.render_object(ro, rd, [1], bg_color=bg, H=H, W=W)
        res = {k: v.clone() for k, v in res.items()}
        assert set(res) == {"image", "depth", "weights_sum", "object_image", "object_depth", "object_weights_sum", "mesh_image"}
        assert torch.equal(res["mesh_image"], res["object_image"]) and tuple(res["object_image"].shape) == (N, 3)
        # the chain of its own operators, bit for bit; the full scene is the ordinary render's
        hand, mid = _by_hand(model, ro, rd, 0b10, False, bg)
        for k, v in hand.items():
            assert torch.equal(res[k], v), k
        plain = model.render(ro, rd, staged=False, perturb=False, bg_color=bg, H=H, W=W)
        for k in ("image", "depth", "weights_sum"):
            assert torch.equal(res[k], plain[k]), k
        assert 0 < int((mid["labels"] == 1).sum()) and 0 < int((mid["labels"] == 0).sum()), "the scene must have samples of both instances"
        # 255 only where y == 0
        assert (mid["live"][mid["labels"] == oref.LABEL_SKIPPED] == 0).all()
        # staged with max_ray_batch = 100 (chunks that are no multiple of the kernel's 32-ray groups): same bits
        model.opt.max_ray_batch = 100
        staged = model.render_object(ro, rd, [1], staged=True, bg_color=bg, H=H, W=W)
        model.opt.max_ray_batch = 16384
        for k, v in res.items():
            assert torch.equal(staged[k], v), k
        # against the fp64 statement on the kernel's own labels
        last_opaque = background == "last_sample"
        view = [l.weight.detach().cpu() for l in model.view_mlp.net]
        cpu = {k: v.cpu() for k, v in mid.items()}
        for keep, invert in ((0b10, False), (0b10, True), (0b01, False)):
            got = model.render_object(ro, rd, [i for i in range(2) if (keep >> i) & 1], invert=invert, bg_color=bg)
            ref = oref.object_ref64(cpu["sig"], cpu["real_bins"], cpu["geo"], rd.cpu(), keep, invert, last_opaque, labels=cpu["labels"].long(),
                                    view_weights=view, bg=bg)
            _within(got["object_weights_sum"], ref["weights_sum"], ref["weights_sum_bound"], "object_weights_sum")
            _within(got["object_depth"], ref["depth"], ref["depth_bound"], "object_depth")
            _within(got["object_image"], ref["object_image"], _image_bound(view, ref), "object_image")
        # S = all ids: the ordinary render (each side within the composite bound of the fp64 value: twice the bound between them)
        both = model.render_object(ro, rd, [0, 1], bg_color=bg)
        ref = oref.object_ref64(cpu["sig"], cpu["real_bins"], cpu["geo"], rd.cpu(), 0b11, False, last_opaque, labels=cpu["labels"].long(),
                                view_weights=view, bg=bg)
        assert ((both["object_weights_sum"] - both["weights_sum"]).abs().double().cpu() <= 2 * ref["weights_sum_bound"]).all()
        assert ((both["object_depth"] - both["depth"]).abs().double().cpu() <= 2 * ref["depth_bound"]).all()
        assert ((both["object_image"] - both["image"]).abs().double().cpu() <= 2 * _image_bound(view, ref)).all()
        # S = {}: no weight anywhere, and every pixel is the empty ray's colour, exactly (object_ref64's note: sigmoid(view_mlp(0)) + bg)
        none = model.render_object(ro, rd, [], bg_color=bg)
        assert (none["object_weights_sum"] == 0).all() and (none["object_depth"] == 0).all()
        zero = torch.zeros(N, 31, device=gpu)
        assert torch.equal(none["object_image"], model.view_mlp.forward_sigmoid_bg(zero, torch.zeros(N, device=gpu), bg))
        assert torch.equal(none["object_image"], torch.full((N, 3), 0.5 + bg, device=gpu))
        # a per-ray tensor background is blended afterwards
        bgt = torch.rand(N, 3, generator=torch.Generator().manual_seed(2)).to(gpu)
        t = model.render_object(ro, rd, [1], bg_color=bgt)
        z = model.render_object(ro, rd, [1], bg_color=0.0)
        assert torch.equal(t["object_image"], z["object_image"] + (1 - z["object_weights_sum"]).unsqueeze(-1) * bgt)
    with pytest.raises(RuntimeError, match="inference render"):
        model.render_object(ro, rd, [1])
    with pytest.raises(ValueError, match="outside"):
        with torch.no_grad():
            model.render_object(ro, rd, [40])
    model.opt.render_mesh = True
    assert model.run(ro, rd) == {}


def _image_bound(view, ref):
    """Bound on sigmoid(view_mlp(f)) + (1 - ws) bg for an f within f_image_bound of the fp64 one: the perceptron is 1-Lipschitz per ReLU
    and |W| e bounds a layer's change elementwise; sigmoid has slope <= 1/4; the head's own fp32 arithmetic is taken at the project's bound
    for its perceptron kernels, 1e-4 max(1, |pre-activation|) in front of the sigmoid; the background term moves with weights_sum (|bg| <= 1)."""
    e = ref["f_image_bound"]
    h = ref["f_image"]
    for i, Wm in enumerate(view):
        e = e @ Wm.double().abs().t()
        h = h @ Wm.double().t()
        if i + 1 < len(view):
            h = torch.relu(h)
    return 0.25 * (e + 1e-4 * h.abs().clamp(min=1.0)) + ref["weights_sum_bound"][:, None] + 4 * oref.U


def test_render_object_fallback_for_a_head_the_label_kernel_does_not_take(gpu):
    """K = 20 outputs: the labels come from m_grid.forward_cat -> the matrix-core perceptron -> argmax; everything behind them is the same
    composite.  The route agrees with the definition on its own logits."""
    from sanerf_hq_amd import raymarching as rm
    model = _model(gpu, n_inst=20)
    ro, rd = _rays(gpu)
    assert not rm.mask_point_labels_fusable(model.m_grid, model.mask_mlp[0], STEPS[-1], 15)
    with torch.no_grad():
        keep_ids = [0, 3, 7, 11, 19]
        res = model.render_object(ro, rd, keep_ids, bg_color=1.0)
        out = rm.render_rays(model._get_plan(), ro, rd, bg_color=1.0, want=["xyzs_last", "geo_feat_last", "sigmas_last", "bins_last"])
        k = len(STEPS) - 1
        nears, fars = rm.near_far_from_aabb(ro, rd, model.aabb_infer, model.min_near)
        real_bins = rm.sample_positions(ro, rd, nears, fars, out[f"bins{k}"], contract=model.opt.contract)[0]
        sig, geo = out[f"sigmas{k}"], out["geo_feat_last"]
        labels, logits = model._point_labels(torch.ones_like(sig), out["xyzs_last"], geo, want_logits=True)
        assert tuple(logits.shape) == (ro.shape[0], STEPS[-1], 20) and labels.dtype == torch.uint8
        lab64 = oref.labels_from_logits(logits.cpu())
        assert torch.equal(labels.cpu().long(), lab64) and len(lab64.unique()) >= 3
        ref = oref.object_ref64(sig.cpu(), real_bins.cpu(), geo.cpu(), rd.cpu(), rm.keep_mask_of(keep_ids), False, True, labels=lab64,
                                view_weights=[l.weight.detach().cpu() for l in model.view_mlp.net], bg=1.0)
        _within(res["object_weights_sum"], ref["weights_sum"], ref["weights_sum_bound"], "object_weights_sum")
        _within(res["object_depth"], ref["depth"], ref["depth_bound"], "object_depth")
        _within(res["object_image"], ref["object_image"], _image_bound([l.weight.detach().cpu() for l in model.view_mlp.net], ref), "object_image")
        # the same model with the label kernel switched off takes the same route: nothing changes
        model.fused_point_labels = False
        again = model.render_object(ro, rd, keep_ids, bg_color=1.0)
        for kk, v in res.items():
            assert torch.equal(again[kk], v), kk


def test_fused_and_operator_chain_labels_agree(gpu):
    """The reference-shaped head through both label routes: logits within twice the project's bound for these kernels of each other
    (each is within tau of the exact ones), and equal labels wherever the top-two margin exceeds 4 tau."""
    from sanerf_hq_amd import raymarching as rm
    model = _model(gpu)
    ro, rd = _rays(gpu)
    with torch.no_grad():
        _, mid = _by_hand(model, ro, rd, 0b10, False, 1.0)
        out = rm.render_rays(model._get_plan(), ro, rd, bg_color=1.0, want=["xyzs_last", "geo_feat_last"])
        model.fused_point_labels = False
        lab_chain, logit_chain = model._point_labels(mid["live"], out["xyzs_last"], out["geo_feat_last"], want_logits=True)
    evaluated = mid["labels"] != oref.LABEL_SKIPPED
    tau = oc.TAU_REL * max(1.0, float(logit_chain.abs().max()))
    assert float((mid["logits"] - logit_chain)[evaluated].abs().max()) <= 2 * tau
    sure = evaluated & (oref.top_two_margin(logit_chain.cpu()).to(evaluated.device) > 4 * tau)
    assert torch.equal(mid["labels"][sure], lab_chain[sure])


def test_render_object_replays_as_a_graph(gpu):
    from sanerf_hq_amd.graph import GraphedStep
    model = _model(gpu)
    ro, rd = _rays(gpu)
    with torch.no_grad():
        eager = {k: v.clone() for k, v in model.render_object(ro, rd, [1], bg_color=0.5).items()}
        step = GraphedStep(lambda: model.render_object(ro, rd, [1], bg_color=0.5), warmup=2)
        for v in step.result.values():
            v.zero_()
        out = step()
        torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(out[k], v), k
