"""CPU: the fp64 statement of the object render (tests/object_ref64.py) against the properties its definition implies."""
import math

import torch

import object_ref64 as oref

K = 4
ALL = (1 << K) - 1


def _case(N=9, T=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    sig = torch.rand(N, T, generator=g) * 6.0
    rb = torch.cumsum(torch.rand(N, T + 1, generator=g) * 0.2 + 0.01, dim=-1)
    geo = torch.randn(N, T, 15, generator=g)
    rd = torch.randn(N, 3, generator=g)
    labels = torch.randint(0, K, (N, T), generator=g)
    return sig, rb, geo, rd, labels


def _view(seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(32, 31, generator=g) * 0.3, torch.randn(32, 32, generator=g) * 0.3, torch.randn(3, 32, generator=g) * 0.3]


def test_all_ids_reproduce_the_plain_weights():
    sig, rb, geo, rd, labels = _case()
    for last in (False, True):
        r = oref.object_ref64(sig, rb, geo, rd, ALL, False, last, labels=labels)
        w = oref.plain_weights64(sig, rb, last)
        assert torch.equal(r["weights"], w)
        assert torch.equal(r["weights_sum"], w.sum(-1))
        assert torch.equal(r["f_image"][:, :15], (w[:, :, None] * geo.double()).sum(1))


def test_empty_set_gives_zeros_and_the_empty_ray_colour():
    """Nothing kept: every output is 0 and object_image = sigmoid(view_mlp(0)) + bg = 0.5 + bg for the bias-free head (object_ref64's note:
    the ordinary render gives an empty ray the same colour)."""
    sig, rb, geo, rd, labels = _case()
    bg = torch.rand(sig.shape[0], 3)
    for last in (False, True):
        r = oref.object_ref64(sig, rb, geo, rd, 0, False, last, labels=labels, view_weights=_view(), bg=bg)
        assert (r["weights"] == 0).all() and (r["weights_sum"] == 0).all() and (r["depth"] == 0).all() and (r["f_image"] == 0).all()
        assert torch.equal(r["object_image"], 0.5 + bg.double())


def test_invert_equals_the_complement():
    sig, rb, geo, rd, labels = _case()
    labels[0, 3] = oref.LABEL_SKIPPED                  # in no set: kept by every inverted gate, also by the complement's
    for S in (0b0001, 0b0110, 0b1011):
        a = oref.object_ref64(sig, rb, geo, rd, S, True, True, labels=labels)
        b = oref.object_ref64(sig, rb, geo, rd, ~S & 0xFFFFFFFF, False, True, labels=labels)
        keep = labels != oref.LABEL_SKIPPED
        assert torch.equal(a["gate"][keep], b["gate"][keep])
        assert bool(a["gate"][0, 3]) and not bool(b["gate"][0, 3])      # 255 is in no S: only the inverted gate lets it through
        labels2 = labels.clone()
        labels2[0, 3] = 0
        a2 = oref.object_ref64(sig, rb, geo, rd, S, True, True, labels=labels2)
        b2 = oref.object_ref64(sig, rb, geo, rd, ~S & ALL, False, True, labels=labels2)
        for k in ("weights", "weights_sum", "depth", "f_image"):
            assert torch.equal(a2[k], b2[k]), k


def test_gated_infinite_density_gives_no_nan():
    sig, rb, geo, rd, labels = _case()
    sig[:, 5] = math.inf
    labels[:, 5] = 2
    r = oref.object_ref64(sig, rb, geo, rd, 0b0001 | 0b1000, False, False, labels=labels)
    assert (r["y"][:, 5] == 0).all() and torch.isfinite(r["weights"]).all() and (r["weights"][:, 6:].abs().sum() > 0)
    kept = oref.object_ref64(sig, rb, geo, rd, 0b0100, False, False, labels=labels)       # kept: opaque there, nothing behind it
    assert (kept["weights"][:, 6:] == 0).all() and torch.isfinite(kept["weights"]).all()


def test_last_sample_is_opaque_only_when_kept():
    sig, rb, geo, rd, labels = _case()
    labels[:, -1] = torch.arange(sig.shape[0]) % 2
    r = oref.object_ref64(sig, rb, geo, rd, 0b0001, False, True, labels=labels)
    kept = labels[:, -1] == 0
    assert torch.allclose(r["weights_sum"][kept], torch.ones(int(kept.sum()), dtype=torch.float64), rtol=0, atol=1e-15)
    assert (r["weights"][~kept, -1] == 0).all() and (r["weights_sum"][~kept] < 1).all()


def test_weight_behind_a_gated_away_occluder():
    """The ordinary transmittance behind the occluder underflows to exactly 0; with the occluder gated away the samples behind it carry weight."""
    sig, rb, geo, rd, labels = _case()
    sig[:, 2] = 1e30
    labels[:, 2] = 1
    labels[:, 3:] = 0
    plain = oref.plain_weights64(sig, rb, False)
    assert (plain[:, 3:] == 0).all()
    r = oref.object_ref64(sig, rb, geo, rd, 0b0001, False, False, labels=labels)
    assert (r["weights"][:, 3:] > 0).all() and (r["weights"][:, 2] == 0).all()


def test_labels_take_the_lowest_index_and_skip_nan():
    lg = torch.tensor([[1.0, 3.0, 3.0], [float("nan"), -1.0, -2.0], [float("nan")] * 3, [-math.inf] * 3, [2.0, 2.0, 2.0]])
    assert oref.labels_from_logits(lg).tolist() == [1, 1, 0, 0, 0]
    assert oref.top_two_margin(torch.tensor([[1.0, 4.0, 2.5]])).tolist() == [1.5]


def test_skipped_tiles_follow_the_kernel_tiling():
    live = torch.zeros(40, 8)
    live[3, 5] = 1.0                    # rays 0..31, depth group 1
    live[39, 0] = float("nan")          # NaN counts as live: rays 32..39, depth group 0
    sk = oref.skipped_tiles(live)
    assert not sk[:32, 4:8].any() and sk[:32, 0:4].all() and not sk[32:, 0:4].any() and sk[32:, 4:8].all()


def test_margin_condition_of_the_committed_label_seeds():
    """The condition of the GPU label test (c), checked here on the CPU with the fp64 statement: the 2 tau margin leaves out at most 2 % of
    the evaluated samples of every label case, and every case has skipped tiles as well as evaluated samples with y == 0."""
    import helpers  # noqa: F401  (puts the package on the path)
    import object_cases as oc
    for case in oc.LABEL_CASES:
        assert oc.margin_share(*case) <= oc.MARGIN_SHARE_MAX, case
        live = oc.label_case(*case)[4]
        skipped = oref.skipped_tiles(live)
        assert skipped.any() and ((live == 0) & ~skipped).any() and (live[skipped] == 0).all()
