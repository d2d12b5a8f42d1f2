"""GPU: geometry export -- sn_rm_lattice_points, the marching-tetrahedra entries (sn_rm_isosurface_count / _emit) against the numpy
restatement in tests/mesh_ref.py, bit for bit, and NeRFRenderer.density_volume / extract_mesh on the small head model."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as mr
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

ISO_SPECIAL = 0.25
ORIGIN, STEP = (-1.0, 0.5, 2.0), (0.25, 0.37, 0.11)


@functools.lru_cache(maxsize=None)
def _volume(name):
    return {
        "noise765": lambda: mr.noise_volume((7, 6, 5), 3),                                   # unequal dimensions: swapped strides
        "noise_multi": lambda: mr.noise_volume((33, 18, 70), 5),                             # several workgroups, a ragged last segment
        "two": lambda: mr.noise_volume((2, 2, 2), 8),
        "sphere17": lambda: mr.sphere_volume(17, (8.13, 7.92, 8.30), 5.92),
        "torus17": lambda: mr.torus_volume(17, 8.1, 4.7, 2.1),
        "sphere_on_vertices": lambda: mr.sphere_volume(9, (4.0, 4.0, 4.0), 3.0),             # values equal to iso, degenerate triangles
        "sphere_leaves_box": lambda: mr.sphere_volume(9, (4.0, 4.0, 4.0), 6.0),              # an open mesh
        "special": lambda: mr.special_volume((9, 11, 70), 11, ISO_SPECIAL),                  # NaN, +-inf, values equal to iso
    }[name]()


@functools.lru_cache(maxsize=None)
def _ref(name, iso):
    return mr.isosurface(_volume(name), iso, ORIGIN, STEP)


CASES = [("noise765", 0.0), ("noise_multi", 0.0), ("two", 0.0), ("sphere17", 0.0), ("torus17", 0.0), ("sphere_on_vertices", 0.0),
         ("sphere_leaves_box", 0.0), ("special", ISO_SPECIAL)]


@pytest.mark.parametrize("name,iso", CASES)
def test_isosurface_equals_the_restatement(gpu, name, iso):
    from sanerf_hq_amd import raymarching as rm
    f = _volume(name)
    ref = _ref(name, iso)
    vol = torch.from_numpy(f).to(gpu)
    got = rm.isosurface(vol, iso, ORIGIN, STEP)
    v, t, n = got["vertices"].cpu().numpy(), got["triangles"].cpu().numpy(), got["normals"].cpu().numpy()
    print(f"{name}: V={len(v)} T={len(t)} (restatement {len(ref['vertices'])} / {len(ref['triangles'])})")
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == ref["vertices"].shape and t.shape == ref["triangles"].shape
    assert len(v) > 0 and len(t) > 0
    assert np.array_equal(t, ref["triangles"])
    assert np.array_equal(v.view(np.uint32), ref["vertices"].view(np.uint32))
    assert np.isfinite(v).all() and np.isfinite(n).all()
    # two runs give equal bits; without normals nothing else changes
    again = rm.isosurface(vol, iso, ORIGIN, STEP)
    for k in ("vertices", "triangles", "normals"):
        assert torch.equal(got[k], again[k]), k
    bare = rm.isosurface(vol, iso, ORIGIN, STEP, normals=False)
    assert bare["normals"] is None and torch.equal(bare["vertices"], got["vertices"]) and torch.equal(bare["triangles"], got["triangles"])


@pytest.mark.parametrize("name", ["noise765", "noise_multi", "sphere17", "torus17", "sphere_leaves_box"])
def test_normals_within_the_derived_bound(gpu, name):
    from sanerf_hq_amd import raymarching as rm
    f = _volume(name)
    ref = _ref(name, 0.0)
    r64 = mr.normals_ref64(f, 0.0, STEP, ref)
    n = rm.isosurface(torch.from_numpy(f).to(gpu), 0.0, ORIGIN, STEP)["normals"].cpu().numpy().astype(np.float64)
    err = np.abs(n - r64["normals"])
    bounded = r64["tol"].max(axis=1) < 2.0
    print(f"{name}: max |n - n64| = {err[bounded].max():.3e}, largest bound {r64['tol'][bounded].max():.3e}, unbounded {int((~bounded).sum())}")
    assert bounded.mean() > 0.99
    assert (err <= r64["tol"]).all()
    length = np.linalg.norm(n, axis=1)
    assert (np.abs(length[r64["length"] > 0] - 1.0) < 1e-6).all()
    # the fp32 restatement of the normals is within its bound as well (the GPU differs from it by the division's and the root's rounding at most)
    assert (np.abs(ref["normals"].astype(np.float64) - r64["normals"]) <= r64["tol"]).all()


def test_empty_surfaces(gpu):
    from sanerf_hq_amd import raymarching as rm
    vol = torch.from_numpy(mr.noise_volume((9, 8, 7), 1)).to(gpu)
    for iso in (1e6, -1e6):                      # all below, all above
        got = rm.isosurface(vol, iso)
        assert tuple(got["vertices"].shape) == (0, 3) and tuple(got["triangles"].shape) == (0, 3) and tuple(got["normals"].shape) == (0, 3)
        counts, _ = rm.isosurface_counts(vol, iso)
        assert counts.tolist() == [0, 0]


@pytest.mark.parametrize("name,iso", [("noise_multi", 0.0), ("sphere17", 0.0)])
def test_capacities_truncate_and_guards_stay(gpu, name, iso):
    """cap_v and cap_t below the counts: the stored prefix is the full result's; the rows behind the capacities keep their fill."""
    from sanerf_hq_amd import raymarching as rm
    vol = torch.from_numpy(_volume(name)).to(gpu)
    full = rm.isosurface(vol, iso, ORIGIN, STEP)
    nv, nt = full["vertices"].shape[0], full["triangles"].shape[0]
    for cap_v, cap_t in ((nv // 2 + 1, nt // 3 + 1), (1, nt), (nv, 1), (0, 7), (5, 0)):
        counts, ws = rm.isosurface_counts(vol, iso)
        assert counts.tolist() == [nv, nt]
        guard = 64
        v = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        n = torch.full((cap_v + guard, 3), -7.0, device=gpu)
        t = torch.full((cap_t + guard, 3), -7, device=gpu, dtype=torch.int32)
        rm.isosurface_emit(vol, iso, ORIGIN, STEP, ws, v, n, t, cap_v=cap_v, cap_t=cap_t)
        assert torch.equal(v[:cap_v], full["vertices"][:cap_v]) and torch.equal(n[:cap_v], full["normals"][:cap_v])
        assert torch.equal(t[:cap_t], full["triangles"][:cap_t])
        assert (v[cap_v:] == -7.0).all() and (n[cap_v:] == -7.0).all() and (t[cap_t:] == -7).all()


def _torch_lattice(origin, step, shape, device):
    ax = [origin[a] + torch.arange(shape[a], device=device, dtype=torch.float32) * torch.tensor(step[a], device=device, dtype=torch.float32)
          for a in range(3)]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def test_lattice_points_equal_meshgrid_and_contract(gpu):
    from sanerf_hq_amd import raymarching as rm
    shape, origin, step = (7, 6, 5), (-3.0, -0.7, 0.1), (1.0, 0.3, 0.77)       # reaches beyond [-1,1]^3: both branches of the contraction
    want = _torch_lattice(origin, step, shape, gpu)
    assert torch.equal(rm.lattice_points(origin, step, shape, device=gpu), want)
    assert (want.abs().amax(1) > 1).any() and (want.abs().amax(1) < 1).any()
    wantc = rm.contract(want)
    assert torch.equal(rm.lattice_points(origin, step, shape, contract=True, device=gpu), wantc)
    for first, count in ((0, 1), (3, 9), (28, 35), (209, 1), (17, 193), (100, 0)):          # windows that straddle z rows and x slabs
        for c, w in ((False, want), (True, wantc)):
            assert torch.equal(rm.lattice_points(origin, step, shape, first, count, contract=c, device=gpu), w[first:first + count])
    with pytest.raises(ValueError):
        rm.lattice_points(origin, step, shape, 200, 11, device=gpu)


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]
RES = (24, 20, 22)


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_object_render.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


@pytest.fixture(scope="module")
def chain(model, gpu):
    """The operator chain on the whole lattice at once: positions by torch, density(), and both label routes."""
    from sanerf_hq_amd import raymarching as rm
    aabb = [-1.5, -1.0, -1.0, 1.0, 1.25, 1.0]                # partly outside [-1,1]^3: some positions are contracted
    res, origin, step = model._lattice(RES, aabb)
    with torch.no_grad():
        xyz = rm.contract(_torch_lattice(origin, step, res, gpu))
        out = model.density(xyz)
        sigma, geo = out["sigma"].reshape(-1), out["geo_feat"]
        n = xyz.shape[0]
        assert n % 4 == 0
        args = (sigma.reshape(-1, 4), xyz.reshape(-1, 4, 3), geo.reshape(-1, 4, 15).contiguous())
        fused = model._point_labels(*args).reshape(-1)
        model.fused_point_labels = False
        try:
            unfused = model._point_labels(*args).reshape(-1)
        finally:
            model.fused_point_labels = True
    return dict(aabb=aabb, sigma=sigma, fused=fused, unfused=unfused)


def test_density_volume_equals_the_operator_chain(gpu, model, chain):
    total = RES[0] * RES[1] * RES[2]
    with torch.no_grad():
        for chunk in (1 << 20, total // 4, 1000, 4099):          # one chunk; a divisor; divisors of neither the lattice nor 4
            vol = model.density_volume(RES, chain["aabb"], chunk=chunk)
            assert tuple(vol.shape) == RES and vol.dtype == torch.float32
            assert torch.equal(vol.reshape(-1), chain["sigma"]), chunk
    assert float(chain["sigma"].max()) > float(chain["sigma"].min()) >= 0


def test_density_volume_gates_by_label(gpu, model, chain):
    """With instance_ids: sigma * (label in set), bit for bit, the labels from the route the model is set to; invert is the complement."""
    sigma = chain["sigma"]
    zero = torch.zeros_like(sigma)
    assert 0 < int((chain["unfused"] == 1).sum()) < sigma.numel(), "the lattice must see both instances"
    differ = int((chain["fused"] != chain["unfused"]).sum() - (chain["fused"] == 255).sum())
    print(f"labels: fused and unfused routes differ on {differ} of {sigma.numel()} evaluated lattice vertices")
    with torch.no_grad():
        for route, labels in (("unfused", chain["unfused"]), ("fused", chain["fused"])):
            model.fused_point_labels = route == "fused"
            try:
                for ids in ([1], [0], [0, 1], []):
                    in_set = torch.zeros_like(labels, dtype=torch.bool)
                    for i in ids:
                        in_set |= labels == i
                    for chunk in (1 << 20, 4099):
                        keep = model.density_volume(RES, chain["aabb"], instance_ids=ids, chunk=chunk).reshape(-1)
                        drop = model.density_volume(RES, chain["aabb"], instance_ids=ids, invert=True, chunk=chunk).reshape(-1)
                        assert torch.equal(keep, torch.where(in_set, sigma, zero)), (route, ids, chunk)
                        assert torch.equal(drop, torch.where(in_set, zero, sigma)), (route, ids, chunk)
                        assert torch.equal(keep + drop, sigma)
            finally:
                model.fused_point_labels = True
    with pytest.raises(ValueError, match="outside"):
        with torch.no_grad():
            model.density_volume(RES, instance_ids=[40])


def test_extract_mesh(gpu, model):
    from sanerf_hq_amd import raymarching as rm
    with torch.no_grad():
        vol = model.density_volume(24)
        thr = float(vol.median())
        mesh = model.extract_mesh(24, threshold=thr)
        V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
        print(f"extract_mesh 24^3 at the median density {thr:.3g}: V={V} T={T}")
        assert V > 0 and T > 0 and int(mesh["triangles"].min()) >= 0 and int(mesh["triangles"].max()) < V
        res, origin, step = model._lattice(24, None)
        want = rm.isosurface(vol, thr, origin, step)
        for k in ("vertices", "normals", "triangles"):
            assert torch.equal(mesh[k], want[k]), k
        assert float(mesh["vertices"].abs().max()) <= 1.0 + 1e-6 and torch.isfinite(mesh["normals"]).all()
        # threshold=None reads density_thresh; one object alone
        model.density_thresh = thr
        same = model.extract_mesh(24, normals=False)
        assert same["normals"] is None and torch.equal(same["triangles"], mesh["triangles"])
        obj = model.extract_mesh(24, instance_ids=[1])
        gated = model.density_volume(24, instance_ids=[1])
        want = rm.isosurface(gated, thr, origin, step)
        assert torch.equal(obj["triangles"], want["triangles"]) and torch.equal(obj["vertices"], want["vertices"])
        model.density_thresh = model.opt.density_thresh
