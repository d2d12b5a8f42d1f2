"""CPU: the numpy restatement of mesh smoothing (tests/mesh_smooth_ref.py) against values worked by hand and against the properties the
definition promises -- what the GPU tests then compare the device with, bit for bit."""
import numpy as np
import pytest

import mesh_ref as mr
import mesh_smooth_ref as sm

# The tetrahedron (100,100,100), (112,100,100), (100,112,100), (100,100,112), oriented outward; origin 0, quantum 1.
TETRA_V = np.array([[100, 100, 100], [112, 100, 100], [100, 112, 100], [100, 100, 112]], dtype=np.float32)
TETRA_T = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)
ZERO = (0.0, 0.0, 0.0)


def _state(v, t, origin=ZERO, quantum=1.0):
    Q0, placed = sm.quantise(v, origin, quantum)
    pairs = sm.corner_pairs(t, len(v))
    return Q0, placed, sm.open_vertices(pairs, len(v)), pairs


def test_tetrahedron_by_hand():
    Q0, placed, is_open, pairs = _state(TETRA_V, TETRA_T)
    assert np.array_equal(Q0, TETRA_V.astype(np.int64)) and placed.all() and not is_open.any()
    assert len(pairs[0]) == 12
    # vertex 0: every neighbour twice, mean (104,104,104), d = 4, 0.5 d = 2.  vertex 1: mean (100,104,104), d = (-12, 4, 4).
    Q = sm.half_step(Q0, placed, is_open, pairs, 0.5)
    assert Q.tolist() == [[102, 102, 102], [106, 102, 102], [102, 106, 102], [102, 102, 106]]
    # normals of the input: at vertex 0 the three faces (0,0,-144) + (0,-144,0) + (-144,0,0); at vertex 1 (0,0,-144) + (0,-144,0) + (144,144,144)
    n, S = sm.geometric_normals(Q0, placed, pairs)
    assert S.tolist() == [[-144, -144, -144], [144, 0, 0], [0, 144, 0], [0, 0, 144]]
    third = np.float32(-1.0 / np.sqrt(3.0))
    assert n.tolist() == [[third] * 3, [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    out = sm.smooth(TETRA_V, TETRA_T, ZERO, 1.0, iterations=1, lam=0.5, mu=0.0)
    assert out["vertices"].tolist() == Q.tolist() and out["flags"].tolist() == [sm.PLACED | sm.MOVED] * 4
    assert np.array_equal(out["normals"], n)                 # a similar tetrahedron


@pytest.mark.parametrize("sign", [1, -1])
def test_ties_go_to_even(sign):
    """f d at exactly +-0.5 and +-1.5: vertex 0 at (100,100,100), the mean of its neighbours at (100,100,100) + sign (1, 3, -1)."""
    v, t = sm.tie_tetrahedron(sign)
    assert np.array_equal(t, TETRA_T)
    Q0, placed, is_open, pairs = _state(v, t)
    assert (Q0[1:].sum(axis=0) - 300).tolist() == [3 * sign, 9 * sign, -3 * sign]
    Q = sm.half_step(Q0, placed, is_open, pairs, 0.5)
    assert Q[0].tolist() == [100, 100 + 2 * sign, 100]      # 0.5 -> 0, 1.5 -> 2, -0.5 -> -0
    Q = sm.half_step(Q0, placed, is_open, pairs, -0.5)
    assert Q[0].tolist() == [100, 100 - 2 * sign, 100]


def test_clamp():
    """A factor of -1 pushes vertex 0 away from its neighbours, past both ends of the range."""
    for corner, far in ((2, 50), (sm.RANGE - 3, sm.RANGE - 51)):
        v = np.array([[corner] * 3, [far, corner, corner], [corner, far, corner], [corner, corner, far]], dtype=np.float32)
        Q0, placed, is_open, pairs = _state(v, TETRA_T)
        assert placed.all()
        Q = sm.half_step(Q0, placed, is_open, pairs, -1.0)
        assert Q[0].tolist() == [0 if corner == 2 else sm.RANGE - 1] * 3
        assert ((Q >= 0) & (Q < sm.RANGE)).all()


@pytest.mark.parametrize("upper", [False, True])
def test_clamp_in_a_whole_iteration(upper):
    """Accepted factors that overshoot: lambda = 0.2, mu = -1 on a pinned fan (what the device tests run)."""
    v, t = sm.clamp_fan(upper)
    out = sm.smooth(v, t, ZERO, 1.0, 1, 0.2, -1.0)
    assert out["open"].tolist() == [False] + [True] * 6 and out["flags"].tolist() == [sm.PLACED | sm.MOVED] + [sm.PLACED | sm.OPEN] * 6
    assert out["Q"][0].tolist() == [sm.RANGE - 1 if upper else 0] * 3
    Q0, placed, is_open, pairs = _state(v, t)
    d = Q0[1:].mean(axis=0) - Q0[0]
    assert (np.abs(0.2 * d - 0.8 * d) > 3.5).all()          # the unclamped move passes the 3 quanta to the end on every axis


def test_quantisation_edges():
    v = np.array([[0, 0, 0], [-0.5, 0, 0], [-0.75, 0, 0], [4194303.25, 1, 1], [4194303.5, 1, 1], [np.nan, 1, 1], [np.inf, 1, 1], [2.5, 3.5, 1]],
                 dtype=np.float32)
    Q, placed = sm.quantise(v, ZERO, 1.0)
    assert placed.tolist() == [True, True, False, True, False, False, False, True]       # rint(-0.5) = -0 is placed; rint(4194303.5) = 2^22 is not
    assert Q[3].tolist() == [4194303, 1, 1] and Q[7].tolist() == [2, 4, 1] and Q[2].tolist() == [0, 0, 0]
    assert sm.check_factors(0.5, -0.53) and sm.check_factors(1.0, 0.0) and sm.check_factors(0.5, -1.0)
    for lam, mu in ((0.0, 0.0), (1.5, 0.0), (0.5, -0.5), (0.5, -0.4), (0.5, 0.3), (0.5, -1.5), (np.nan, 0.0), (0.5, np.nan), (1.0, -1.0)):
        assert not sm.check_factors(lam, mu), (lam, mu)
    origin, quantum = sm.quantisation([0, 0, 0], [23, 23, 11])
    Q, placed = sm.quantise(np.array([[0, 0, 0], [23, 23, 11]], dtype=np.float32), origin, quantum)
    assert placed.all() and abs(Q[0] - 524288).max() <= 1 and abs(Q[1, 0] - 5 * 524288) <= 1       # 2^19 .. 2^19 + 2^21


def test_mix_is_splitmix64():
    # (splitmix64 seeded with 0 returns 0xE220A8397B1DCDAF first: the finaliser of 0 + gamma.  mix(i) finalises i + 1 + gamma.)
    gamma = 0x9E3779B97F4A7C15
    def by_hand(i):
        x = (i + 1 + gamma) & (2 ** 64 - 1)
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return x ^ (x >> 31)
    idx = np.array([0, 1, 2, 1000, 2 ** 31 - 2])
    assert [int(x) for x in sm.mix(idx)] == [by_hand(int(i)) for i in idx]
    assert by_hand(-1) == 0xE220A8397B1DCDAF


def test_closed_and_clipped_sphere():
    origin, quantum = sm.lattice_quantisation()
    m = sm.volume_mesh("sphere")
    assert (len(m["vertices"]), len(m["triangles"])) == (3246, 6488)
    out = sm.smooth(m["vertices"], m["triangles"], origin, quantum, 0)
    assert not out["open"].any() and out["placed"].all() and not (out["flags"] & sm.MOVED).any()
    assert np.array_equal(out["vertices"].view(np.uint32), m["vertices"].view(np.uint32))      # zero iterations: the input bits
    c = sm.volume_mesh("clipped_sphere")
    oc = sm.smooth(c["vertices"], c["triangles"], origin, quantum, 3)
    edge = sm.boundary_vertices(c["triangles"], len(c["vertices"]))
    assert out["open"].sum() == 0 and oc["open"].sum() == 92 and np.array_equal(np.nonzero(oc["open"])[0], edge)
    # pinned vertices keep their bits; the others moved somewhere
    assert np.array_equal(oc["vertices"][edge].view(np.uint32), c["vertices"][edge].view(np.uint32))
    assert not (oc["flags"][edge] & sm.MOVED).any() and (oc["flags"] & sm.MOVED != 0).sum() > len(c["vertices"]) // 2
    unpinned = sm.smooth(c["vertices"], c["triangles"], origin, quantum, 3, pin_open=False)
    assert (unpinned["flags"][edge] & sm.MOVED).any()
    # normals: outward and of unit length to one fp32 rounding -- of the meshes as they come, and of the closed sphere smoothed.  (Not of
    # the clipped sphere smoothed with its rim pinned: after 3 iterations one rim vertex has a neighbour pulled past it, a folded triangle.)
    c0 = sm.smooth(c["vertices"], c["triangles"], origin, quantum, 0)
    m10 = sm.smooth(m["vertices"], m["triangles"], origin, quantum, 10)
    for res, centre in ((out, (11.3, 12.1, 10.7)), (m10, (11.3, 12.1, 10.7)), (c0, (11.3, 12.1, 3.2))):
        n = res["normals"].astype(np.float64)
        assert ((n * (res["vertices"].astype(np.float64) - np.asarray(centre))).sum(axis=1) > 0).all()
        err = np.abs(np.linalg.norm(n, axis=1) - 1.0).max()
        print(f"| |n| - 1 | <= {err / 2.0 ** -24:.2f} x 2^-24")
        assert err <= 2.0 ** -23


def test_noisy_sphere_smooths_without_shrinking():
    origin, quantum = sm.lattice_quantisation()
    m = sm.volume_mesh("noisy_sphere")
    v, t = m["vertices"], m["triangles"]
    taubin = sm.smooth(v, t, origin, quantum, 10)
    laplace = sm.smooth(v, t, origin, quantum, 10, 0.5, 0.0)
    a0, a1 = sm.mean_dihedral_degrees(v, t), sm.mean_dihedral_degrees(taubin["vertices"], t)
    vol0 = mr.signed_volume(v, t)
    dt, dl = mr.signed_volume(taubin["vertices"], t) / vol0 - 1.0, mr.signed_volume(laplace["vertices"], t) / vol0 - 1.0
    print(f"mean dihedral angle {a0:.1f} -> {a1:.1f} degrees; volume change: Taubin {dt:+.2%}, Laplacian {dl:+.2%}")
    assert a1 < a0 and abs(dt) < abs(dl)


def test_steps_compose():
    origin, quantum = sm.lattice_quantisation()
    m = sm.volume_mesh("two_blobs")
    Q0, placed, is_open, pairs = _state(m["vertices"], m["triangles"], origin, quantum)
    for mu in (-0.53, 0.0):
        five = sm.steps(Q0, placed, is_open, pairs, 5, 0.5, mu)
        assert np.array_equal(sm.steps(sm.steps(Q0, placed, is_open, pairs, 3, 0.5, mu), placed, is_open, pairs, 2, 0.5, mu), five)
        assert not np.array_equal(five, Q0)


def test_long_row_and_malformed_fixtures():
    v, t = sm.double_cone()
    pairs = sm.corner_pairs(t, len(v))
    assert np.bincount(pairs[0])[:2].tolist() == [5000, 5000] and not sm.open_vertices(pairs, len(v)).any()
    out = sm.smooth(v, t, *sm.bounding_quantisation(v), 3)
    assert out["normals"][0, 2] > 0.99 and out["normals"][1, 2] < -0.99 and (out["flags"] & sm.MOVED).all()
    v, t, (origin, quantum) = sm.malformed()
    out = sm.smooth(v, t, origin, quantum, 3)
    lost = ~out["placed"]
    assert lost.sum() == 3 and np.array_equal(out["vertices"][lost].view(np.uint32), v[lost].view(np.uint32))
    assert np.isfinite(out["vertices"][~lost]).all() and np.isfinite(out["normals"]).all() and not out["normals"][lost].any()
    tv, tt = sm.terrain()
    ot = sm.smooth(tv, tt, *sm.bounding_quantisation(tv), 3)
    assert 50 < ot["open"].sum() < len(tv) // 2


def test_the_package_quantises_as_the_restatement_does():
    """raymarching.smooth_quantisation (host arithmetic) against quantisation() here; the boxes it refuses."""
    from sanerf_hq_amd import raymarching as rm
    rng = np.random.default_rng(11)
    for _ in range(50):
        lo = rng.uniform(-3.0, 3.0, size=3)
        hi = lo + rng.uniform(0.01, 5.0, size=3)
        origin, quantum = rm.smooth_quantisation(lo.tolist(), hi.tolist())
        assert (origin, quantum) == sm.quantisation(lo, hi)
    assert rm.smooth_quantisation([0, 0, 0], [23, 23, 23]) == sm.lattice_quantisation()
    assert sm.lattice_quantisation() == ([-5.75, -5.75, -5.75], 23.0 / 2.0 ** 21)
    for lo, hi in (([1, 1, 1], [1, 1, 1]), ([0, 0, 0], [1e-50, 0, 0]), ([0, 0, 0], [float("inf"), 1, 1]), ([0, 0, 0], [float("nan"), 1, 1])):
        assert rm.smooth_quantisation(lo, hi) is None
