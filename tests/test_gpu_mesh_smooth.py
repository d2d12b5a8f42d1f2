"""GPU: mesh smoothing -- sn_rm_mesh_smooth_build / _steps / _emit against the numpy restatement in tests/mesh_smooth_ref.py: vertices and
normals bit for bit, flags exactly; sizes at the segment edges; a row of 5000 pairs; independence of the vertex order, of the run and of
what the scratch buffer held; the empty cases; NeRFRenderer.extract_mesh(smooth=)."""
import numpy as np
import pytest
import torch

import mesh_ref as mr
import mesh_simplify_ref as ms
import mesh_smooth_ref as sm
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _to_device(v, t, gpu, normals=False):
    return {"vertices": torch.from_numpy(np.ascontiguousarray(v)).to(gpu), "normals": torch.zeros(len(v), 3, device=gpu) if normals else None,
            "triangles": torch.from_numpy(np.ascontiguousarray(t)).to(gpu)}


def _fixture(name):
    """-> (vertices, triangles, (origin, quantum)) of the named mesh: the 24^3 volumes quantised over their lattice's box, the others over
    their own bounding box."""
    if name in sm.VOLUMES:
        m = sm.volume_mesh(name)
        return m["vertices"], m["triangles"], sm.lattice_quantisation()
    v, t = {"terrain": sm.terrain, "cone": sm.double_cone}[name]()
    return v, t, sm.bounding_quantisation(v)


def _assert_equal(out, want, what=""):
    """Vertices and normals bit for bit, flags exactly."""
    assert out["vertices"].dtype == torch.float32 and tuple(out["vertices"].shape) == want["vertices"].shape, what
    assert np.array_equal(_np(out["vertices"]).view(np.uint32), want["vertices"].view(np.uint32)), what
    if out["normals"] is not None:
        assert np.array_equal(_np(out["normals"]).view(np.uint32), want["normals"].view(np.uint32)), what
    if "vertex_flags" in out:
        assert out["vertex_flags"].dtype == torch.uint8 and np.array_equal(_np(out["vertex_flags"]), want["flags"]), what


def _run(mesh, quant, case, what=""):
    from sanerf_hq_amd import raymarching as rm
    N, lam, mu, pin = case
    origin, quantum = quant
    want = sm.smooth(_np(mesh["vertices"]), _np(mesh["triangles"]), origin, quantum, N, lam, mu, pin)
    out = rm.mesh_smooth(mesh, N, lam, mu, pin, origin=origin, quantum=quantum, normals=True, return_flags=True)
    print(f"{what} {case}: V={mesh['vertices'].shape[0]} T={mesh['triangles'].shape[0]} open={int(want['open'].sum())} "
          f"moved={int((want['flags'] & sm.MOVED != 0).sum())}")
    _assert_equal(out, want, what)
    assert out["triangles"] is mesh["triangles"]
    return out, want


@pytest.mark.parametrize("case", sm.CASES)
@pytest.mark.parametrize("name", ["sphere", "two_blobs", "clipped_sphere", "noisy_sphere", "terrain", "cone"])
def test_equal_to_the_restatement(gpu, name, case):
    v, t, quant = _fixture(name)
    out, want = _run(_to_device(v, t, gpu), quant, case, name)
    assert (want["flags"] & sm.MOVED).any() and want["placed"].all()
    assert bool(want["open"].any()) == (name in ("clipped_sphere", "terrain"))
    if name == "cone":                                       # the apexes' rows: 5000 pairs each, summed by a whole wave
        assert (want["flags"][:2] & sm.MOVED).all() and _np(out["normals"])[0, 2] > 0.99


def test_ties_and_clamps(gpu):
    """f d at exactly +-0.5 and +-1.5 (ties to even), and moves that leave the integer range at either end."""
    for sign in (1, -1):
        v, t = sm.tie_tetrahedron(sign)
        for case in ((1, 0.5, 0.0, True), (1, 0.5, -1.0, True)):
            _run(_to_device(v, t, gpu), ((0.0, 0.0, 0.0), 1.0), case, f"ties {sign}")
    for upper in (False, True):
        v, t = sm.clamp_fan(upper)
        out, want = _run(_to_device(v, t, gpu), ((0.0, 0.0, 0.0), 1.0), (1, 0.2, -1.0, True), f"clamp {upper}")
        assert want["Q"][0].tolist() == [sm.RANGE - 1 if upper else 0] * 3
        assert _np(out["vertices"])[0].tolist() == [float(sm.RANGE - 1) if upper else 0.0] * 3


@pytest.mark.parametrize("T", [1, 1024, 1025, 3 * 1024 + 1])
def test_triangle_prefixes(gpu, T):
    m = sm.volume_mesh("sphere")
    _, want = _run(_to_device(m["vertices"], m["triangles"][:T], gpu), sm.lattice_quantisation(), (3, 0.5, -0.53, True), f"first {T} triangles")
    assert want["open"].any() and (want["S"] == 0).all(axis=1).any()          # a patch with a rim; vertices that no triangle of the prefix uses


def test_large_sphere_crosses_many_segments(gpu):
    """96^3: tens of thousands of triangles, dozens of scan segments of 1024 vertices."""
    from sanerf_hq_amd import raymarching as rm
    mesh = rm.isosurface(torch.from_numpy(mr.sphere_volume(96, (47.3, 48.1, 46.7), 37.6)).to(gpu), 0.0, normals=False)
    assert mesh["triangles"].shape[0] > 50 * 1024 and mesh["vertices"].shape[0] > 24 * 1024
    quant = sm.lattice_quantisation((96, 96, 96))
    _, want = _run(mesh, quant, (3, 0.5, -0.53, True), "sphere 96^3")
    assert not want["open"].any()
    # the default quantisation (the mesh's own bounding box, read back) against its restatement
    own = sm.bounding_quantisation(_np(mesh["vertices"]))
    out = rm.mesh_smooth(mesh, 3, normals=True, return_flags=True)
    _assert_equal(out, sm.smooth(_np(mesh["vertices"]), _np(mesh["triangles"]), *own, 3), "default quantisation")


def test_malformed_mesh(gpu):
    """Indices out of range, rows that repeat an index, NaN and infinite vertices, a vertex beyond the integer range: results, no fault."""
    v, t, quant = sm.malformed()
    for case in ((3, 0.5, -0.53, True), (2, 0.5, 0.0, False)):
        out, want = _run(_to_device(v, t, gpu), quant, case, "malformed")
        lost = ~want["placed"]
        assert lost.sum() == 3
        got = _np(out["vertices"])
        assert np.array_equal(got[lost].view(np.uint32), v[lost].view(np.uint32))          # unplaced rows keep their bits
        assert np.isfinite(got[~lost]).all() and torch.isfinite(out["normals"]).all()
        assert not (_np(out["vertex_flags"])[lost] & (sm.PLACED | sm.MOVED)).any()


def test_vertex_order_does_not_matter(gpu):
    """Permuted vertices, relabelled triangles: permuted, equal bits -- what the integer sums are for."""
    from sanerf_hq_amd import raymarching as rm
    m = sm.volume_mesh("clipped_sphere")
    mesh = _to_device(m["vertices"], m["triangles"], gpu)
    origin, quantum = sm.lattice_quantisation()
    base = rm.mesh_smooth(mesh, 3, origin=origin, quantum=quantum, normals=True, return_flags=True)
    V = mesh["vertices"].shape[0]
    for seed in (1, 2):
        perm = torch.from_numpy(np.random.default_rng(seed).permutation(V)).to(gpu)        # new row j holds old vertex perm[j]
        inverse = torch.empty_like(perm)
        inverse[perm] = torch.arange(V, device=gpu)
        other = {"vertices": mesh["vertices"][perm].contiguous(), "normals": None,
                 "triangles": inverse[mesh["triangles"].long()].to(torch.int32).flip(0).contiguous()}      # and the triangles in another order
        out = rm.mesh_smooth(other, 3, origin=origin, quantum=quantum, normals=True, return_flags=True)
        for key in ("vertices", "normals"):
            assert torch.equal(out[key].view(torch.int32), base[key][perm].view(torch.int32)), key
        assert torch.equal(out["vertex_flags"], base["vertex_flags"][perm])


def test_two_calls_and_a_poisoned_scratch_give_equal_bits(gpu):
    from sanerf_hq_amd import _buffers, raymarching as rm
    m = sm.volume_mesh("two_blobs")
    mesh = _to_device(m["vertices"], m["triangles"], gpu)
    origin, quantum = sm.lattice_quantisation()
    call = lambda: rm.mesh_smooth(mesh, 3, origin=origin, quantum=quantum, normals=True, return_flags=True)
    first, again = call(), call()
    _buffers.scratch("mesh_smooth", torch.device(gpu), 8 << 20).fill_(0xA5)                # nothing of an earlier call, or of the fill, may show
    poisoned = call()
    for other in (again, poisoned):
        for key in ("vertices", "normals", "vertex_flags"):
            assert torch.equal(first[key].view(torch.uint8), other[key].view(torch.uint8)), key


def test_phases_compose(gpu):
    """build, steps(3), steps(2), emit equals mesh_smooth(5) -- for Taubin iterations and for Laplacian ones, whose half-steps end in the
    other buffer; an emit between the steps changes nothing."""
    from sanerf_hq_amd import raymarching as rm
    m = sm.volume_mesh("noisy_sphere")
    mesh = _to_device(m["vertices"], m["triangles"], gpu)
    V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    origin, quantum = sm.lattice_quantisation()
    for mu in (-0.53, 0.0):
        whole = rm.mesh_smooth(mesh, 5, 0.5, mu, origin=origin, quantum=quantum, normals=True)
        ws = rm.mesh_smooth_build(mesh["vertices"], mesh["triangles"], origin, quantum)
        rm.mesh_smooth_steps(V, T, ws, 3, 0.5, mu)
        mid_v = torch.empty(V, 3, device=gpu)
        rm.mesh_smooth_emit(mesh["vertices"], T, origin, quantum, ws, mid_v)
        rm.mesh_smooth_steps(V, T, ws, 2, 0.5, mu)
        out_v, out_n = torch.empty(V, 3, device=gpu), torch.empty(V, 3, device=gpu)
        rm.mesh_smooth_emit(mesh["vertices"], T, origin, quantum, ws, out_v, out_n)
        assert torch.equal(out_v.view(torch.int32), whole["vertices"].view(torch.int32)) and torch.equal(out_n.view(torch.int32), whole["normals"].view(torch.int32))
        three = rm.mesh_smooth(mesh, 3, 0.5, mu, origin=origin, quantum=quantum)
        assert torch.equal(mid_v.view(torch.int32), three["vertices"].view(torch.int32)) and not torch.equal(mid_v, out_v)


def test_empty_cases_and_normals_only(gpu):
    from sanerf_hq_amd import raymarching as rm
    m = sm.volume_mesh("sphere")
    mesh = _to_device(m["vertices"], m["triangles"], gpu, normals=True)
    origin, quantum = sm.lattice_quantisation()
    want = sm.smooth(m["vertices"], m["triangles"], origin, quantum, 0)
    # iterations = 0: the input's bits, the geometric normals (the input's own normals are not read)
    out = rm.mesh_smooth(mesh, 0, origin=origin, quantum=quantum, return_flags=True)
    assert torch.equal(out["vertices"].view(torch.int32), mesh["vertices"].view(torch.int32)) and out["vertices"] is not mesh["vertices"]
    _assert_equal(out, want, "zero iterations")
    assert not (_np(out["vertex_flags"]) & sm.MOVED).any()
    n = rm.mesh_vertex_normals(mesh, origin=origin, quantum=quantum)
    assert np.array_equal(_np(n).view(np.uint32), want["normals"].view(np.uint32))
    assert (torch.linalg.vector_norm(n.double(), dim=1) - 1.0).abs().max() <= 2.0 ** -23
    # normals: default iff the input has them; None / False / True
    assert rm.mesh_smooth(dict(mesh, normals=None), 1, origin=origin, quantum=quantum)["normals"] is None
    assert rm.mesh_smooth(mesh, 1, origin=origin, quantum=quantum, normals=False)["normals"] is None
    assert rm.mesh_smooth(dict(mesh, normals=None), 1, origin=origin, quantum=quantum, normals=True)["normals"].shape == (len(m["vertices"]), 3)
    with_n, without = rm.mesh_smooth(mesh, 2, origin=origin, quantum=quantum), rm.mesh_smooth(mesh, 2, origin=origin, quantum=quantum, normals=False)
    assert torch.equal(with_n["vertices"], without["vertices"]) and "vertex_flags" not in with_n
    extra = rm.mesh_smooth(dict(mesh, colors=mesh["vertices"]), 1, origin=origin, quantum=quantum)
    assert sorted(extra) == ["colors", "normals", "triangles", "vertices"]                 # the keys of the input
    # T = 0: nothing moves, normals zero; V = 0; no finite vertex; a box without extent
    none = torch.zeros(0, 3, device=gpu, dtype=torch.int32)
    out = rm.mesh_smooth(dict(mesh, triangles=none), 3, origin=origin, quantum=quantum, return_flags=True)
    assert torch.equal(out["vertices"].view(torch.int32), mesh["vertices"].view(torch.int32)) and not out["normals"].any()
    assert (out["vertex_flags"] == sm.PLACED).all()
    for V in (0, 5):
        pts = torch.rand(V, 3, device=gpu)
        out = rm.mesh_smooth({"vertices": pts, "normals": None, "triangles": none}, 3, normals=True, return_flags=True)
        assert torch.equal(out["vertices"], pts) and tuple(out["normals"].shape) == (V, 3) and not out["normals"].any() and out["vertex_flags"].shape == (V,)
    tri = torch.tensor([[0, 1, 2]], device=gpu, dtype=torch.int32)
    nan = {"vertices": torch.full((3, 3), float("nan"), device=gpu), "normals": None, "triangles": tri}
    out = rm.mesh_smooth(nan, 3, normals=True)
    assert torch.isnan(out["vertices"]).all() and not out["normals"].any()
    point = {"vertices": torch.full((3, 3), 0.25, device=gpu), "normals": None, "triangles": tri}
    out = rm.mesh_smooth(point, 3, normals=True)
    assert torch.equal(out["vertices"], point["vertices"]) and not out["normals"].any()


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_mesh_simplify.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


def test_extract_mesh_smooth(gpu, model):
    from sanerf_hq_amd import raymarching as rm
    res = 24
    with torch.no_grad():
        thr = float(model.density_volume(res).median())
        plain = model.extract_mesh(res, threshold=thr)
        off = model.extract_mesh(res, threshold=thr, smooth=0)                   # today's path, bit for bit
        for k in ("vertices", "normals", "triangles"):
            assert torch.equal(plain[k].view(torch.int32), off[k].view(torch.int32)), k
        _, origin, step = model._lattice(res, None)
        quant = sm.lattice_quantisation((res,) * 3, origin, step)
        assert quant == rm.smooth_quantisation(origin, [origin[a] + (res - 1) * step[a] for a in range(3)])
        for kwargs in (dict(simplify=2), dict(keep_largest=1)):
            got = model.extract_mesh(res, threshold=thr, smooth=3, **kwargs)
            before = model.extract_mesh(res, threshold=thr, **kwargs)             # the chain by hand: clean-up and simplification as they are
            by_hand = rm.mesh_smooth(before, 3, origin=quant[0], quantum=quant[1])
            want = sm.smooth(_np(before["vertices"]), _np(before["triangles"]), *quant, 3)
            print(f"extract_mesh smooth=3 {kwargs}: V={before['vertices'].shape[0]} open={int(want['open'].sum())} "
                  f"moved={int((want['flags'] & sm.MOVED != 0).sum())}")
            assert (want["flags"] & sm.MOVED).any() and want["placed"].all()      # (a random field at its median: most of the surface is rim or pinched, and pinned)
            assert torch.equal(got["triangles"], before["triangles"])
            for k in ("vertices", "normals"):
                assert torch.equal(got[k].view(torch.int32), by_hand[k].view(torch.int32)), k
            _assert_equal(got, want, kwargs)
        assert model.extract_mesh(res, threshold=thr, smooth=2, normals=False)["normals"] is None
        # vertex colours: computed on the smoothed mesh, along its own normals
        col = model.extract_mesh(res, threshold=thr, simplify=2, smooth=3, vertex_colors=True)
        smoothed = model.extract_mesh(res, threshold=thr, simplify=2, smooth=3)
        assert torch.equal(col["vertices"], smoothed["vertices"]) and torch.equal(col["normals"], smoothed["normals"])
        attr = model.vertex_attributes(smoothed, 0.5 * min(abs(s) for s in step), samples=8)
        assert torch.equal(col["colors"], attr["colors"]) and torch.equal(col["coverage"], attr["coverage"])
        with pytest.raises(ValueError, match="smooth"):
            model.extract_mesh(res, threshold=thr, smooth=1.5)
