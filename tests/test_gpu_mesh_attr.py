"""GPU: vertex colours and instance labels of an exported mesh -- sn_rm_vertex_probe_points against its fp32 restatement (bit for bit) and
fp64 (directions), sn_rm_vertex_probe_composite against tests/mesh_attr_ref64.py within the bounds derived there, and
NeRFRenderer.vertex_attributes / extract_mesh(vertex_colors, vertex_labels) against the operator chain on the small head model."""
import functools
import math

import pytest
import torch

import mesh_attr_ref64 as ma
from helpers import make_opt, synthetic_params

pytestmark = pytest.mark.gpu

H_PROBE = 0.37


@functools.lru_cache(maxsize=None)
def _mesh_points(V):
    """Vertices that reach beyond [-1,1]^3 (both branches of the contraction) and normals of every scale; with V >= 17 the degenerate ones."""
    g = torch.Generator().manual_seed(11 + V)
    v = torch.empty(V, 3).uniform_(-2.5, 2.5, generator=g)
    n = torch.randn(V, 3, generator=g) * torch.exp(torch.empty(V, 1).uniform_(-60.0, 60.0, generator=g))     # |n| from 1e-26 to 1e26
    bad = {}
    if V >= 17:
        n[2] = torch.tensor([0.0, 0.0, 0.0])
        n[4] = torch.tensor([-0.0, 0.0, -0.0])
        n[6] = torch.tensor([math.nan, 1.0, 0.0])
        n[8] = torch.tensor([1.0, math.inf, 0.0])
        n[10] = torch.tensor([-math.inf, -math.inf, math.inf])
        n[12] = torch.tensor([1e-42, 0.0, 0.0])                # a subnormal normal is still a direction
        n[14] = torch.tensor([3e38, -3e38, 3e38])              # squares that would overflow
        bad = {2, 4, 6, 8, 10}
    return v, n, bad


@pytest.mark.parametrize("K", [4, 32])
@pytest.mark.parametrize("V", [1, 17, 1000])
def test_probe_points(gpu, V, K):
    from sanerf_hq_amd import raymarching as rm
    v, n, bad = _mesh_points(V)
    vg, ng = v.to(gpu), n.to(gpu)
    xyz, dirs = rm.vertex_probe_points(vg, ng, K, H_PROBE)
    assert tuple(xyz.shape) == (V, K, 3) and tuple(dirs.shape) == (V, 3) and xyz.dtype == dirs.dtype == torch.float32
    # directions: within the derived bound of fp64; the default for a zero, NaN or inf normal
    d64 = ma.probe_direction64(n)
    err = (dirs.cpu().double() - d64).abs()
    print(f"V={V} K={K}: max |d - d64| = {float(err.max()):.3e} (bound {float(ma.direction_bound(d64).max()):.3e})")
    assert bool((err <= ma.direction_bound(d64)).all())
    assert bool(((dirs.cpu().double().pow(2).sum(-1) - 1).abs() < 1e-6).all())
    down = torch.tensor([0.0, 0.0, -1.0])
    for i in bad:
        assert torch.equal(dirs[i].cpu(), down), i
    if V >= 17:
        assert torch.equal(dirs[12].cpu(), torch.tensor([-1.0, 0.0, 0.0]))
        assert bool((dirs[14].cpu().abs() - 1 / math.sqrt(3)).abs().max() < 1e-6)
    # positions: bit-equal to the fp32 restatement from the kernel's own directions
    want = ma.probe_points32(v, dirs.cpu(), K, H_PROBE)
    assert torch.equal(xyz.cpu(), want)
    if V > 1:
        assert bool((want.abs().amax(-1) > 1).any()) and bool((want.abs().amax(-1) < 1).any())
    # contracted: bit-equal to the contraction operator on the uncontracted output
    xyz_c, dirs_c = rm.vertex_probe_points(vg, ng, K, H_PROBE, contract=True)
    assert torch.equal(xyz_c, rm.contract(xyz.reshape(-1, 3)).reshape(V, K, 3)) and torch.equal(dirs_c, dirs)
    # windows that align with nothing
    for first, count in ((0, 1), (V - 1, 1), (1, V - 1), (3, 11), (5, 0), (13, 977), (301, 333)):
        if first + count > V or first < 0:
            continue
        for c, full in ((False, xyz), (True, xyz_c)):
            wx, wd = rm.vertex_probe_points(vg, ng, K, H_PROBE, first, count, contract=c)
            assert torch.equal(wx, full[first:first + count]) and torch.equal(wd, dirs[first:first + count]), (first, count, c)


# ---- the composite against the fp64 statement ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(V, K, mode):
    case = ma.random_case(V, K, mode)
    return case, ma.vertex_probe_ref64(**case)


def _run(rm, case, gpu, want_labels, rows=slice(None)):
    lab = case.get("labels")
    return rm.vertex_probe_composite(case["sigmas"][rows].to(gpu), case["geo"][rows].to(gpu), case["dirs"][rows].to(gpu), case["h"],
                                     labels=None if lab is None else lab[rows].to(gpu), keep_mask=case.get("keep_mask", 0xFFFFFFFF),
                                     invert=case.get("invert", False), want_labels=want_labels)


@pytest.mark.parametrize("mode", ["plain", "keep", "invert"])
@pytest.mark.parametrize("K", ma.SAMPLES)
@pytest.mark.parametrize("V", [1, 17, 1000])
def test_composite_against_the_fp64_statement(gpu, V, K, mode):
    from sanerf_hq_amd import raymarching as rm
    case, ref = _case(V, K, mode)
    voting = mode != "plain"
    f, cov, vlabel = _run(rm, case, gpu, voting)
    assert tuple(f.shape) == (V, 31) and tuple(cov.shape) == (V,) and (vlabel is None) == (not voting)
    f64, cov64 = f.cpu().double(), cov.cpu().double()
    assert bool(torch.isfinite(f64).all()) and bool(torch.isfinite(cov64).all())
    # a vertex whose W lies within its bound of 2^-126 could take either branch: left out, and none is expected
    sure = ref["branch_certain"]
    assert bool(sure.all()), f"{int((~sure).sum())} vertices within their bound of the coverage threshold"
    err_c = (cov64 - ref["coverage"]).abs()
    err_f = (f64 - ref["f"]).abs()
    fb = ~ref["normal"]
    print(f"V={V} K={K} {mode}: max |W - W64| = {float(err_c.max()):.3e} (largest bound {float(ref['coverage_bound'].max()):.3e}); "
          f"max |f - f64| / bound = {float((err_f / ref['f_bound']).max()):.3f}; fallback rows {int(fb.sum())}"
          + (f", max |g - mean64| there = {float(err_f[fb][:, :15].max()):.3e}" if bool(fb.any()) else ""))
    assert bool((err_c <= ref["coverage_bound"]).all())
    assert bool((err_f <= ref["f_bound"]).all())
    assert bool((cov64[fb] == 0).all())                                          # nothing kept: exactly 0 on the device as well
    if V >= 17:
        assert bool(fb.any()) and bool(ref["normal"].any())                      # both branches of step 6
    if voting:
        got = vlabel.cpu().long()
        certain = ref["label_certain"]
        left_out = 1.0 - float(certain.double().mean())
        print(f"V={V} K={K} {mode}: {left_out:.2%} of the vertex labels are within the bounds of a tie and left out")
        assert left_out <= 0.01
        assert torch.equal(got[certain], ref["vertex_label"][certain])
        assert set(got.tolist()) <= {0, 1, 2, ma.LABEL_NONE}
    # equal bits across two calls; a vertex's result does not depend on V or the launch grid
    f2, cov2, vlabel2 = _run(rm, case, gpu, voting)
    assert torch.equal(f, f2) and torch.equal(cov, cov2) and (not voting or torch.equal(vlabel, vlabel2))
    if V == 1000:
        for rows in (slice(0, 500), slice(500, 1000), slice(333, 334), slice(7, 990)):
            fp, cp, lp = _run(rm, case, gpu, voting, rows)
            assert torch.equal(fp, f[rows]) and torch.equal(cp, cov[rows]) and (not voting or torch.equal(lp, vlabel[rows])), rows


def test_composite_takes_a_view_at_an_odd_offset_and_an_empty_mesh(gpu):
    from sanerf_hq_amd import raymarching as rm
    case, _ = _case(17, 4, "plain")
    f, cov, _ = _run(rm, case, gpu, False)
    flat = torch.zeros(17 * 4 * 15 + 1, device=gpu)
    flat[1:] = case["geo"].to(gpu).reshape(-1)
    shifted = flat[1:].view(17, 4, 15)                                           # 4 bytes past a 16-byte boundary
    assert shifted.data_ptr() % 16 == 4
    f2, cov2, _ = rm.vertex_probe_composite(case["sigmas"].to(gpu), shifted, case["dirs"].to(gpu), case["h"])
    assert torch.equal(f, f2) and torch.equal(cov, cov2)
    f0, c0, l0 = rm.vertex_probe_composite(torch.zeros(0, 8, device=gpu), torch.zeros(0, 8, 15, device=gpu), torch.zeros(0, 3, device=gpu), 0.1,
                                           labels=torch.zeros(0, 8, device=gpu, dtype=torch.uint8), want_labels=True)
    assert tuple(f0.shape) == (0, 31) and tuple(c0.shape) == (0,) and tuple(l0.shape) == (0,)
    x0, d0 = rm.vertex_probe_points(torch.zeros(0, 3, device=gpu), torch.zeros(0, 3, device=gpu), 8, 0.1)
    assert tuple(x0.shape) == (0, 8, 3) and tuple(d0.shape) == (0, 3)


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
STEPS = [16, 8, 4]
RES = 24


@pytest.fixture(scope="module")
def model(gpu):
    """The reference-shaped field with the mask head only, as tests/test_gpu_mesh.py builds it."""
    from sanerf_hq_amd.nerf import NeRFNetwork
    params = synthetic_params(STEPS, heads=True)
    torch.manual_seed(20)
    m = NeRFNetwork(make_opt(num_steps=list(STEPS), with_sam=False, with_mask=True, n_inst=2))
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}, strict=False)
    return m.to(gpu).eval()


@pytest.fixture(scope="module")
def scene(model):
    """The 24^3 mesh at the median density, and the probe step extract_mesh would use."""
    with torch.no_grad():
        thr = float(model.density_volume(RES).median())
        mesh = model.extract_mesh(RES, threshold=thr)
    _, _, step = model._lattice(RES, None)
    return dict(mesh=mesh, thr=thr, h=0.5 * min(step))


@pytest.mark.parametrize("K", [8, 32])
def test_vertex_attributes_equal_the_operator_chain(gpu, model, scene, K):
    from sanerf_hq_amd import raymarching as rm
    mesh, h = scene["mesh"], scene["h"]
    V = mesh["vertices"].shape[0]
    assert V > 1000, "the mesh must span several chunks"
    with torch.no_grad():
        xyz, dirs = rm.vertex_probe_points(mesh["vertices"], mesh["normals"], K, h, contract=bool(model.opt.contract))
        out = model.density(xyz.reshape(-1, 3))
        sigma, geo = out["sigma"].reshape(V, K).float(), out["geo_feat"].reshape(V, K, -1).contiguous()
        labels = model._point_labels(sigma, xyz, geo)
        for ids, invert in ((None, False), ([1], False), ([1], True)):
            keep = 0xFFFFFFFF if ids is None else rm.keep_mask_of(ids)
            f, cov, vl = rm.vertex_probe_composite(sigma, geo, dirs, h, labels, keep, invert, want_labels=True)
            colors = model.view_mlp.forward_sigmoid_bg(f, torch.ones_like(cov), 0.0)
            for chunk in (1 << 17, 1000, 4099):
                got = model.vertex_attributes(mesh, h, samples=K, instance_ids=ids, invert=invert, labels=True, chunk=chunk)
                assert torch.equal(got["colors"], colors), (ids, invert, chunk)
                assert torch.equal(got["coverage"], cov) and torch.equal(got["labels"], vl), (ids, invert, chunk)
                assert got["colors"].dtype == torch.float32 and got["labels"].dtype == torch.uint8
            print(f"K={K} ids={ids} invert={invert}: V={V}, mean coverage {float(cov.mean()):.3f}, "
                  f"labels {torch.bincount(vl.long(), minlength=256)[[0, 1, 255]].tolist()} (0 / 1 / none)")
        # without labels and without a gate nothing of the mask field is asked: colours and coverage are the ungated ones, labels None
        f, cov, _ = rm.vertex_probe_composite(sigma, geo, dirs, h)
        plain = model.vertex_attributes(mesh, h, samples=K, chunk=4099)
        assert plain["labels"] is None and torch.equal(plain["coverage"], cov)
        assert torch.equal(plain["colors"], model.view_mlp.forward_sigmoid_bg(f, torch.ones_like(cov), 0.0))


def test_extract_mesh_with_attributes(gpu, model, scene):
    thr = scene["thr"]
    with torch.no_grad():
        bare = model.extract_mesh(RES, threshold=thr, simplify=2, min_component_triangles=8)
        assert set(bare) == {"vertices", "normals", "triangles"}                 # both flags off: today's keys
        for ids in (None, [1]):
            mesh = model.extract_mesh(RES, threshold=thr, instance_ids=ids, simplify=2, min_component_triangles=8, vertex_colors=True,
                                      vertex_labels=True)
            assert set(mesh) == {"vertices", "normals", "triangles", "colors", "coverage", "labels"}
            V = mesh["vertices"].shape[0]
            if ids is None:
                for k in ("vertices", "normals", "triangles"):
                    assert torch.equal(mesh[k], bare[k]), k
            assert V > 0 and tuple(mesh["colors"].shape) == (V, 3) and tuple(mesh["coverage"].shape) == (V,) and tuple(mesh["labels"].shape) == (V,)
            assert bool(torch.isfinite(mesh["colors"]).all()) and float(mesh["colors"].min()) >= 0.0 and float(mesh["colors"].max()) <= 1.0
            lab = mesh["labels"].long()
            counts = torch.bincount(lab, minlength=256)
            print(f"extract_mesh ids={ids}: V={V}, labels 0 / 1 / none = {counts[[0, 1, 255]].tolist()}, mean coverage {float(mesh['coverage'].mean()):.3f}")
            assert int(counts.sum()) == int(counts[[0, 1, 255]].sum())
            assert bool((mesh["coverage"][lab == 255] == 0).all())
            if ids is not None:
                assert bool((lab[lab != 255] == 1).all())
            # the attributes are those of the final mesh
            _, _, step = model._lattice(RES, None)
            want = model.vertex_attributes(mesh, 0.5 * min(step), samples=8, instance_ids=ids, labels=True)
            assert torch.equal(mesh["colors"], want["colors"]) and torch.equal(mesh["coverage"], want["coverage"]) and torch.equal(mesh["labels"], want["labels"])
        only_c = model.extract_mesh(RES, threshold=thr, vertex_colors=True, probe_samples=4, probe_step=1.0)
        assert set(only_c) == {"vertices", "normals", "triangles", "colors", "coverage"}
        only_l = model.extract_mesh(RES, threshold=thr, vertex_labels=True)
        assert set(only_l) == {"vertices", "normals", "triangles", "labels"}
