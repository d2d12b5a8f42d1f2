"""CPU: the fp64 statement of the vertex probes (tests/mesh_attr_ref64.py) on hand-worked values, and the near-tie share of the random
cases the GPU test uses."""
import math

import pytest
import torch

import mesh_attr_ref64 as ma


def _geo(K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, K, 15, generator=g).double()


D = torch.tensor([[0.0, 0.6, -0.8]])


@pytest.mark.parametrize("K", ma.SAMPLES)
def test_one_opaque_sample(K):
    """h sigma = inf at i0 and nothing in front: w = e_{i0}, so g = geo_{i0}, W = 1 and the label is label_{i0}."""
    i0 = K // 2 + 1
    sg = torch.zeros(1, K)
    sg[0, i0] = math.inf
    sg[0, i0 + 1:] = 3.0                                       # behind the opaque sample: transmittance 0
    geo = _geo(K)
    labels = torch.full((1, K), 2, dtype=torch.uint8)
    labels[0, i0] = 7
    r = ma.vertex_probe_ref64(sg, geo, D, 0.25, labels=labels, keep_mask=0xFFFFFFFF)
    want = torch.zeros(K, dtype=torch.float64)
    want[i0] = 1.0
    assert torch.equal(r["weights"][0], want)
    assert float(r["coverage"]) == 1.0 and bool(r["normal"])
    assert torch.equal(r["g"][0], geo[0, i0]) and torch.equal(r["f"][0, :15], geo[0, i0])
    assert int(r["vertex_label"]) == 7 and bool(r["label_certain"])


@pytest.mark.parametrize("K", ma.SAMPLES)
def test_constant_sigma_gives_geometric_weights(K):
    h, s = 0.125, 2.0                                          # y = 0.25 exactly
    a = 1.0 - math.exp(-h * s)
    r = ma.vertex_probe_ref64(torch.full((1, K), s), _geo(K, 1), D, h)
    want = torch.tensor([a * (1.0 - a) ** i for i in range(K)], dtype=torch.float64)
    assert torch.allclose(r["weights"][0], want, rtol=1e-14, atol=0)
    assert abs(float(r["coverage"]) - (1.0 - (1.0 - a) ** K)) < 1e-15
    g = (want[:, None] * _geo(K, 1)[0]).sum(0) / want.sum()
    assert torch.allclose(r["g"][0], g, rtol=1e-13, atol=1e-15)
    # SH4 of the unit direction: the constant and the three linear terms
    sh = r["f"][0, 15:]
    assert abs(float(sh[0]) - 0.28209479177387814) < 1e-15
    c1 = 0.4886025119029199
    assert torch.allclose(sh[1:4], torch.tensor([-c1 * 0.6, c1 * -0.8, -c1 * 0.0], dtype=torch.float64), atol=1e-15)
    assert r["weights_bound"].min() > 0 and float(r["coverage_bound"]) < 1e-5 and float(r["g_bound"].max()) < 1e-4


@pytest.mark.parametrize("invert", [False, True])
def test_everything_gated_out(invert):
    K = 8
    sg = torch.full((1, K), 50.0)
    sg[0, 2] = math.inf                                        # a select, not a product: no NaN from 0 * inf
    geo = _geo(K, 2)
    labels = torch.full((1, K), 1, dtype=torch.uint8)
    r = ma.vertex_probe_ref64(sg, geo, D, 0.5, labels=labels, keep_mask=0b101 if not invert else 0b010, invert=invert)
    assert float(r["coverage"]) == 0.0 and not bool(r["normal"]) and float(r["weights"].abs().sum()) == 0.0
    assert torch.allclose(r["g"][0], geo[0].sum(0) / K, rtol=1e-15, atol=0)
    assert int(r["vertex_label"]) == ma.LABEL_NONE and bool(r["label_certain"]) and bool(r["branch_certain"])
    assert float(r["coverage_bound"]) == 0.0                   # exp(-0) = 1 exactly: the device's W is exactly 0 too
    # the same samples kept: something is hit
    r = ma.vertex_probe_ref64(sg, geo, D, 0.5, labels=labels, keep_mask=0b010)
    assert float(r["coverage"]) == 1.0 and int(r["vertex_label"]) == 1


def test_labels_past_31_are_in_no_set_and_do_not_vote():
    K = 4
    labels = torch.tensor([[255, 40, 32, 255]], dtype=torch.uint8)
    sg = torch.full((1, K), 1.0)
    r = ma.vertex_probe_ref64(sg, _geo(K), D, 1.0, labels=labels, keep_mask=0xFFFFFFFF)
    assert float(r["coverage"]) == 0.0 and int(r["vertex_label"]) == ma.LABEL_NONE
    r = ma.vertex_probe_ref64(sg, _geo(K), D, 1.0, labels=labels, keep_mask=0, invert=True)
    assert float(r["coverage"]) > 0.9 and int(r["vertex_label"]) == ma.LABEL_NONE and float(r["votes"].sum()) == 0.0


def test_a_tie_of_votes_goes_to_the_lower_index():
    """y = (ln 2, inf, ...): w = (1/2, 1/2, 0, ...) -- exp(-ln 2) is exactly 1/2 in float64 -- so two labels tie at 1/2."""
    K = 4
    sg = torch.tensor([[math.log(2.0), math.inf, 1.0, 1.0]], dtype=torch.float64)
    for first, second in ((9, 4), (4, 9)):
        labels = torch.tensor([[first, second, 1, 1]], dtype=torch.uint8)
        r = ma.vertex_probe_ref64(sg, _geo(K), D, 1.0, labels=labels)
        assert r["weights"][0].tolist() == [0.5, 0.5, 0.0, 0.0]
        assert float(r["votes"][0, 4]) == float(r["votes"][0, 9]) == 0.5
        assert int(r["vertex_label"]) == 4
        assert not bool(r["label_certain"])                    # a tie is exactly what the bounds cannot decide


def test_degenerate_normals_give_the_default_direction():
    n = torch.tensor([[0.0, 0.0, 0.0], [math.nan, 1.0, 0.0], [1.0, -math.inf, 0.0], [0.0, 3.0, -4.0], [1e-30, 0.0, 0.0], [3e38, 3e38, 0.0]])
    d = ma.probe_direction64(n)
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)
    for i in range(3):
        assert torch.equal(d[i], down), i
    assert torch.allclose(d[3], torch.tensor([0.0, -0.6, 0.8], dtype=torch.float64), atol=1e-16)
    assert torch.equal(d[4], torch.tensor([-1.0, 0.0, 0.0], dtype=torch.float64))
    assert torch.allclose(d[5], torch.tensor([-math.sqrt(0.5), -math.sqrt(0.5), 0.0], dtype=torch.float64), atol=1e-16)


def test_probe_positions_start_outside_and_end_inside():
    for K in ma.SAMPLES:
        c = ma.probe_offsets(K)
        assert float(c[0]) == 0.5 - K / 2 and float(c[-1]) == K / 2 - 0.5 and torch.equal(c, -c.flip(0))
    v = torch.tensor([[1.0, 2.0, 3.0]])
    d = torch.tensor([[0.0, 0.0, -1.0]])
    p = ma.probe_points32(v, d, 4, 0.5)
    assert torch.equal(p[0, :, 2], torch.tensor([3.75, 3.25, 2.75, 2.25])) and torch.equal(p[0, :, :2], v[:, :2].expand(4, 2))


@pytest.mark.parametrize("mode", ["keep", "invert"])
@pytest.mark.parametrize("K", ma.SAMPLES)
def test_the_random_cases_keep_near_ties_rare(K, mode):
    """The GPU test leaves out the vertices whose label the bounds cannot decide and fails above 1 %: the chosen seed stays below it."""
    case = ma.random_case(1000, K, mode)
    r = ma.vertex_probe_ref64(**case)
    left_out = 1.0 - float(r["label_certain"].double().mean())
    print(f"K={K} {mode}: {left_out:.2%} of the vertex labels are within the bounds of a tie; "
          f"{int((~r['branch_certain']).sum())} vertices near the coverage threshold; labels {sorted(set(r['vertex_label'].tolist()))}")
    assert left_out <= 0.01
    assert bool(r["branch_certain"].all())
    assert int((~r["normal"]).sum()) > 0 and int(r["normal"].sum()) > 500      # both branches of step 6 are well populated
    assert set(r["vertex_label"].tolist()) == ({0, 2, ma.LABEL_NONE} if mode == "keep" else {0, 2, ma.LABEL_NONE})
