"""GPU: the second tile of the one workgroup scan of csrc/mesh_common.h, once per element type.  The scan takes the segment totals 1024 at
a time and carries a 64-bit sum from tile to tile; a segment is 1024 elements, so the carry is used only by lists of more than 1,048,576
elements.  Each test is just past that size and sparse on purpose, so that numpy states what is expected in well under a second:
    uint32_t        mesh_clean  -- the kept vertices and triangles, remapped
    uint64_t        mesh_smooth -- the rows of pairs of the vertices beyond index 1,048,576
    the uint2 pair  isosurface  -- the mesh vertices and triangles owned by lattice vertices beyond 1,048,576
Everything is compared exactly; nothing is masked."""
import numpy as np
import pytest
import torch

import mesh_ref as mr
import mesh_smooth_ref as sm

pytestmark = pytest.mark.gpu

TILE = 1024 * 1024                     # elements in the first tile of the scan
V = 1025 * 1024 + 7
T = 1025 * 1024 + 5


def _np(t):
    return t.cpu().numpy()


def _sparse_rows():
    """The triangle rows that are valid: every 997th, the two at the tile's edge and the last."""
    rows = np.unique(np.concatenate([np.arange(0, T, 997), [TILE - 1, TILE, T - 1]]))
    assert (rows < TILE).sum() > 1000 and (rows >= TILE).sum() >= 3
    return rows


def test_uint32_scan_second_tile_mesh_clean(gpu):
    from sanerf_hq_amd import raymarching as rm
    rng = np.random.default_rng(1025)
    vert = rng.standard_normal((V, 3)).astype(np.float32)
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    rows = _sparse_rows()
    # pairwise disjoint triples over the whole index range, the vertices at the tile's edge and both ends among them
    forced = np.array([0, TILE - 1, TILE, TILE + 1, V - 2, V - 1])
    rest = np.setdiff1d(rng.permutation(V)[:3 * len(rows)], forced)[:3 * len(rows) - len(forced)]
    corners = rng.permutation(np.concatenate([forced, rest]))
    assert len(np.unique(corners)) == 3 * len(rows) and (corners >= TILE).sum() >= 4
    tri = np.full((T, 3), -1, dtype=np.int32)
    tri[rows] = corners.reshape(-1, 3)
    # expected, by numpy alone: every valid row is a component of its own with one triangle, so min_triangles = 1 keeps them all
    source = np.unique(corners)
    want_tri = np.searchsorted(source, tri[rows]).astype(np.int32)
    mesh = {"vertices": torch.from_numpy(vert).to(gpu), "normals": torch.from_numpy(nrm).to(gpu), "triangles": torch.from_numpy(tri).to(gpu)}
    out = rm.mesh_clean(mesh, min_triangles=1, return_source=True)
    print(f"mesh_clean V={V} T={T}: V'={out['vertices'].shape[0]} T'={out['triangles'].shape[0]}, beyond the first tile: "
          f"{int((source >= TILE).sum())} vertices, {int((rows >= TILE).sum())} triangles")
    assert out["source_vertex"].dtype == torch.int32 and np.array_equal(_np(out["source_vertex"]), source)
    assert out["triangles"].dtype == torch.int32 and np.array_equal(_np(out["triangles"]), want_tri)
    assert np.array_equal(_np(out["vertices"]).view(np.uint32), vert[source].view(np.uint32))
    assert np.array_equal(_np(out["normals"]).view(np.uint32), nrm[source].view(np.uint32))


def test_uint64_scan_second_tile_mesh_smooth(gpu):
    from sanerf_hq_amd import raymarching as rm
    rng = np.random.default_rng(1026)
    vert = rng.uniform(0.0, 100.0, size=(V, 3)).astype(np.float32)
    origin, quantum = (-10.0, -10.0, -10.0), 2.0 ** -12        # Q below 110 * 4096 < 2^22: every vertex is placed
    # closed fans of six triangles: a centre and its rim of six, at these first indices -- in the first tile, across its edge, beyond it
    starts = [5, 70001, TILE - 12, TILE - 3, TILE + 4, TILE + 500, V - 7]
    fans = []
    for s in starts:
        ids = s + rng.permutation(7)
        fans += [[ids[0], ids[1 + i], ids[1 + (i + 1) % 6]] for i in range(6)]
    fans = np.array(fans, dtype=np.int32)
    assert fans.max() == V - 1 and len(np.unique(fans)) == 7 * len(starts)
    rows = _sparse_rows()[-len(fans):]                         # (the smoothing does not depend on where a row stands)
    tri = np.full((T, 3), -1, dtype=np.int32)
    tri[rows] = fans
    case = (3, 0.5, -0.53, False)                              # pin_open = False: the rims move too
    want = sm.smooth(vert, tri, origin, quantum, *case)        # the whole mesh: well under a second
    used = np.unique(fans)
    moved = (want["flags"] & sm.MOVED) != 0
    assert want["placed"].all() and moved[used].all() and not np.delete(moved, used).any()
    assert (want["open"][used]).sum() == 6 * len(starts)
    mesh = {"vertices": torch.from_numpy(vert).to(gpu), "normals": None, "triangles": torch.from_numpy(tri).to(gpu)}
    out = rm.mesh_smooth(mesh, *case, origin=origin, quantum=quantum, normals=True, return_flags=True)
    print(f"mesh_smooth V={V} T={T}: {len(used)} vertices in fans, {int((used >= TILE).sum())} of them beyond the first tile")
    assert np.array_equal(_np(out["vertex_flags"]), want["flags"])
    assert np.array_equal(_np(out["vertices"]).view(np.uint32), want["vertices"].view(np.uint32))
    assert np.array_equal(_np(out["normals"]).view(np.uint32), want["normals"].view(np.uint32))


def test_pair_scan_second_tile_isosurface(gpu):
    from sanerf_hq_amd import raymarching as rm
    shape = (3700, 17, 17)                                     # 1,069,300 lattice vertices: 1045 segments
    ball = mr.sphere_volume(17, (8.0, 8.0, 8.0), 5.5)
    for face in (ball[0], ball[-1], ball[:, 0], ball[:, -1], ball[:, :, 0], ball[:, :, -1]):
        assert (face <= 0).all()                               # outside, as the filler: no surface between the copies
    vol = np.full(shape, -1.0, dtype=np.float32)
    for x0 in (0, 3620, 3683):                                 # lattice index 1,048,576 lies at x = 3628.3, inside the second copy
        vol[x0:x0 + 17] = ball
    want = mr.isosurface(vol, 0.0)                             # the whole volume: about half a second
    one = mr.isosurface(ball, 0.0)
    nv, nt = len(want["vertices"]), len(want["triangles"])
    assert (nv, nt) == (3 * len(one["vertices"]), 3 * len(one["triangles"])) and nv > 0
    beyond = int((want["owner"] >= TILE).sum())
    assert nv // 3 < beyond < 2 * nv // 3                      # the edge of the tile cuts the second copy
    dvol = torch.from_numpy(vol).to(gpu)
    counts, _ = rm.isosurface_counts(dvol, 0.0)
    assert counts.tolist() == [nv, nt]
    out = rm.isosurface(dvol, 0.0)
    print(f"isosurface {shape}: V={nv} T={nt}, {beyond} vertices owned beyond the first tile")
    assert np.array_equal(_np(out["triangles"]), want["triangles"])
    assert np.array_equal(_np(out["vertices"]).view(np.uint32), want["vertices"].view(np.uint32))
    # the normals land in the same rows: within the bound that tests/test_gpu_mesh.py holds them to (they are not bit-equal to numpy's)
    r64 = mr.normals_ref64(vol, 0.0, (1.0, 1.0, 1.0), want)
    assert (r64["tol"] < 1e-4).all()
    assert (np.abs(_np(out["normals"]).astype(np.float64) - r64["normals"]) <= r64["tol"]).all()
