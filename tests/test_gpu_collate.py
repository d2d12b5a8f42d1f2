"""GPU: the device-side batch draw (collate.hip: sn_rm_weighted_draw, sn_rm_collate_gather, nerf.DeviceCollate) against the numpy
restatement of tests/collate_ref.py.  The specification is exact, so everything is compared for equality: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import collate_ref as R

pytestmark = pytest.mark.gpu

ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))
H, W, S = 48, 64, 16


def same(t, a):
    """Equal shapes, dtypes and values; NaN equals NaN (an undrawn ray)."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    t = t.detach().cpu()
    if t.shape != a.shape or t.dtype != a.dtype:
        return False
    if t.is_floating_point():
        return torch.equal(torch.isnan(t), torch.isnan(a)) and torch.equal(torch.nan_to_num(t, nan=0.0), torch.nan_to_num(a, nan=0.0))
    return torch.equal(t, a)


# ---- draw -------------------------------------------------------------------------------------------------------------------------------
def run_draw(gpu, w, e, n, **kw):
    from sanerf_hq_amd import raymarching as rm
    out, status = rm.weighted_draw(torch.from_numpy(w).to(gpu), torch.from_numpy(e).to(gpu), n, **kw)
    return out.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("C,n", [(25, 1), (25, 25), (25, 24), (256, 128), (576, 100), (16384, 4096)])
def test_weighted_draw_equals_the_restatement(gpu, C, n, rows):
    rng = np.random.default_rng(C * 7 + n + rows)
    # random rows: the plain case
    w = (rng.random((rows, C), dtype=np.float32) + np.float32(1e-3)).astype(np.float32)
    e = rng.standard_exponential((rows, C)).astype(np.float32)
    got, status = run_draw(gpu, w, e, n)
    want, wstatus = R.weighted_draw(w, e, n)
    assert np.array_equal(got, want) and status == wstatus == 0
    # equal weights and equal exponentials: every key ties, the first n cells
    ones = np.ones((rows, C), dtype=np.float32)
    got, status = run_draw(gpu, ones, ones, n)
    assert np.array_equal(got, np.tile(np.arange(n), (rows, 1))) and status == 0
    # ties only at the threshold: fewer than n keys below it, more than n up to it
    below = min(max(n // 2, 0), C - 1) if n > 1 else 0
    e = np.full((rows, C), 2.0, dtype=np.float32)
    for r in range(rows):
        e[r, rng.permutation(C)[:below]] = 0.5
        if C - below > n:                                            # some keys above the threshold as well
            e[r, rng.permutation(C)[:(C - n) // 3]] = 8.0
    got, status = run_draw(gpu, ones, e, n)
    want, wstatus = R.weighted_draw(ones, e, n)
    assert np.array_equal(got, want) and status == wstatus
    ties = (e == 2.0)
    for r in range(rows):
        taken = np.isin(np.arange(C), got[r]) & ties[r]
        if taken.any() and (ties[r] & ~taken).any() and (e[r] < 2.0).sum() < n <= (e[r] <= 2.0).sum():
            assert np.flatnonzero(taken).max() < np.flatnonzero(ties[r] & ~taken).min(), "ties go to the smaller cell"
    # zeros, a negative and a NaN weight, exponentials of 0 and inf
    w = (rng.random((rows, C), dtype=np.float32) + np.float32(1e-3)).astype(np.float32)
    e = rng.standard_exponential((rows, C)).astype(np.float32)
    w[:, 1], w[:, 3], w[:, 4], w[:, 7] = 0.0, -1.0, np.nan, 0.0
    e[:, 2], e[:, 5], e[:, 7] = 0.0, np.inf, 0.0                     # key 0: drawn first; key inf: never; 0 / 0: never
    got, status = run_draw(gpu, w, e, n)
    want, wstatus = R.weighted_draw(w, e, n)
    assert np.array_equal(got, want) and status == wstatus
    assert not np.isin(got, [1, 3, 4, 5, 7]).any() and (got == 2).any(axis=1).all()
    # one row with n - 2 selectable cells: -1 in its tail, the status word set, the other rows as if nothing had happened
    w = (rng.random((rows, C), dtype=np.float32) + np.float32(1e-3)).astype(np.float32)
    e = rng.standard_exponential((rows, C)).astype(np.float32)
    short, keep = rows // 2, max(n - 2, 0)
    w[short, rng.permutation(C)[keep:]] = 0.0
    got, status = run_draw(gpu, w, e, n)
    want, wstatus = R.weighted_draw(w, e, n)
    assert np.array_equal(got, want) and status == wstatus == 1
    assert (got[short, keep:] == -1).all() and (got[short, :keep] >= 0).all() and len(got[short, keep:]) == min(n, 2)
    for r in range(rows):
        if r != short:
            assert np.array_equal(got[r], R.weighted_draw(w[r:r + 1], e[r:r + 1], n)[0][0]) and (got[r] >= 0).all()


def test_weighted_draw_row_tables_static_outputs_and_sticky_status(gpu):
    from sanerf_hq_amd import raymarching as rm
    rng = np.random.default_rng(21)
    M, C, rows = 5, 256, 4
    w = (rng.random((M, C), dtype=np.float32) ** 4).astype(np.float32)
    e = rng.standard_exponential((rows, C)).astype(np.float32)
    row_u = np.array([0.0, ONE_BELOW, 0.41, 0.79], dtype=np.float32)
    for n in (1, 17):
        got, status = run_draw(gpu, w, e, n, row_u=torch.from_numpy(row_u).to(gpu))
        want, wstatus = R.weighted_draw(w, e, n, row_u=row_u)
        assert np.array_equal(got, want) and status == wstatus == 0
        idx = np.array([4, 0, 9, -3], dtype=np.int64)                # clamped to 0 .. M-1
        got, status = run_draw(gpu, w, e, n, row_index=torch.from_numpy(idx).to(gpu))
        want, wstatus = R.weighted_draw(w, e, n, row_index=idx)
        assert np.array_equal(got, want) and status == wstatus == 0
    out = torch.full((rows, 17), -5, device=gpu, dtype=torch.int64)
    status = torch.ones(1, device=gpu, dtype=torch.int32)
    o2, s2 = rm.weighted_draw(torch.from_numpy(w[:rows]).to(gpu), torch.from_numpy(e).to(gpu), 17, out=out, status=status)
    assert o2 is out and s2 is status and int(status.item()) == 1, "the status word is only ever set"
    assert np.array_equal(out.cpu().numpy(), R.weighted_draw(w[:rows], e, 17)[0])
    again, _ = rm.weighted_draw(torch.from_numpy(w[:rows]).to(gpu), torch.from_numpy(e).to(gpu), 17)
    assert torch.equal(again, out), "two runs give the same bits"


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
_DATA = {}


def dataset(M, n_intr, ch, mask_dtype, Cm=2):
    """The dataset arrays (numpy), built once per shape and never changed."""
    key = (M, n_intr, ch, np.dtype(mask_dtype).name, Cm)
    if key not in _DATA:
        rng = np.random.default_rng(100 + M * 13 + n_intr + ch)
        poses = rng.standard_normal((M, 4, 4)).astype(np.float32)
        poses[:, 3] = (0, 0, 0, 1)
        intr = np.stack([np.array([60 + 3 * k, 58 + 2 * k, W / 2 + 0.25 * k, H / 2 - 0.5 * k], dtype=np.float32) for k in range(n_intr)])
        masks = rng.integers(0, 200, (M, H, W, Cm))
        masks = rng.random((M, H, W, Cm), dtype=np.float32) if np.dtype(mask_dtype) == np.float32 else masks.astype(mask_dtype)
        _DATA[key] = {"poses": poses, "intrinsics": intr, "images": rng.integers(0, 256, (M, H, W, ch), dtype=np.uint8), "masks": masks,
                      "error_map": rng.random((M, S * S), dtype=np.float32), "cam_near_far": rng.random((M, 2), dtype=np.float32)}
    return _DATA[key]


def on(gpu, data):
    return {k: torch.from_numpy(v).to(gpu) for k, v in data.items()}


def uniforms(rng, N, cols):
    u = rng.random((N, cols), dtype=np.float32)
    u[0] = 0.0
    u[-1] = ONE_BELOW
    if N == 1:
        u[0, 1] = ONE_BELOW if cols > 1 else 0.0
        u[0, 0] = 0.0
    return u


def check_against_torch(gpu, t, res, want, N):
    """rays: rays_from_pixels on the same (camera, pixel), bit for bit; gathered values: torch's fancy indexing of the dataset tensors."""
    from sanerf_hq_amd import raymarching as rm
    cam, row, col = (torch.from_numpy(want[k]).to(gpu) for k in ("cam", "row", "col"))
    ok = torch.from_numpy(want["valid"]).to(gpu)
    intr = t["intrinsics"][cam] if t["intrinsics"].shape[0] > 1 else t["intrinsics"]
    ro, rd = rm.rays_from_pixels(t["poses"][cam], intr, row * W + col, W)
    assert torch.equal(res["rays_o"][ok], ro[ok]) and torch.equal(res["rays_d"][ok], rd[ok])
    assert torch.isnan(res["rays_o"][~ok]).all() and torch.isnan(res["rays_d"][~ok]).all()
    if "images" in res:
        # an IEEE division, as specified: tensor / tensor.  (tensor / 255 with a host scalar multiplies by fl(1 / 255) on the device, which is
        # not the same number for every byte; the two differ by at most one unit in the last place.)
        picked = t["images"][cam[:N], row[:N], col[:N]].float()
        assert torch.equal(res["images"][ok[:N]], (picked / torch.full((), 255.0, device=gpu))[ok[:N]])
        assert ((res["images"] - picked / 255)[ok[:N]].abs() <= 2.0 ** -24).all()
    if "masks" in res:
        assert torch.equal(res["masks"][ok], t["masks"][cam, row, col][ok]) and res["masks"].dtype == t["masks"].dtype
    if "cam_near_far" in res:
        assert torch.equal(res["cam_near_far"], t["cam_near_far"][cam])
    if "error_maps" in res:
        sj, si = S / H, S / W                                        # collate_rays's own expression
        assert torch.equal(res["error_maps"][ok], t["error_map"][cam, (row * sj).long() * S + (col * si).long()][ok])
    assert torch.equal(res["poses"], t["poses"][cam].reshape(-1, 16)) and torch.equal(res["intrinsics"], t["intrinsics"][cam if t["intrinsics"].shape[0] > 1 else cam * 0])


def check_against_restatement(res, want):
    for k in ("rays_o", "rays_d", "index", "i", "j", "inds_coarse", "images", "masks", "error_maps", "cam_near_far", "poses"):
        if k in res:
            assert same(res[k], want[k]), k


CASES = [(1, 1, 1, 3, np.int64), (1, 255, 1, 4, np.float32), (1, 257, 1, 3, np.uint8), (5, 1, 5, 4, np.uint8), (5, 255, 1, 3, np.float32),
         (5, 257, 5, 4, np.int64), (5, 257, 1, 3, np.int64), (5, 255, 5, 4, np.float32)]


@pytest.mark.parametrize("M,N,n_intr,ch,mask_dtype", CASES)
def test_uniform_batch_with_patches(gpu, M, N, n_intr, ch, mask_dtype):
    from sanerf_hq_amd import raymarching as rm
    data = dataset(M, n_intr, ch, mask_dtype)
    t = on(gpu, data)
    rng = np.random.default_rng(N * 31 + M)
    u, L, p = uniforms(rng, N, 3), 3, 4
    ul = np.array([0.0, ONE_BELOW, 0.55], dtype=np.float32)
    centres = np.array([S * S - 1, 0, int(rng.integers(0, S * S))], dtype=np.int64)
    res = rm.collate_gather(t["poses"], t["intrinsics"], H, W, u=torch.from_numpy(u).to(gpu), images=t["images"], masks=t["masks"],
                            error_map=t["error_map"], cam_near_far=t["cam_near_far"], error_map_size=S, ul=torch.from_numpy(ul).to(gpu),
                            centres=torch.from_numpy(centres).to(gpu), patch_size=p)
    want = R.gather(data, H, W, N, u=u, S=S, L=L, p=p, ul=ul, centres=centres)
    assert res["rays_o"].shape == (N + L * p * p, 3) and res["images"].shape == (N, ch) and res["masks"].shape == (N + L * p * p, 2)
    assert want["cam"][0] == 0 and want["row"][0] == (0 if N > 1 else H - 1) and want["cam"][N - 1] == (M - 1 if N > 1 else 0)
    assert want["row"][N - 1] == H - 1 and (N == 1 or want["col"][N - 1] == W - 1), "the largest uniform picks the last camera, row and column"
    check_against_restatement(res, want)
    check_against_torch(gpu, t, res, want, N)
    # no patches: the same main part
    main = rm.collate_gather(t["poses"], t["intrinsics"], H, W, u=torch.from_numpy(u).to(gpu), images=t["images"], masks=t["masks"],
                             error_map=t["error_map"], cam_near_far=t["cam_near_far"], error_map_size=S)
    for k, v in main.items():
        assert v.shape[0] == N and torch.equal(v, res[k][:N]), k


@pytest.mark.parametrize("M,N,n_intr", [(1, 1, 1), (5, 255, 5), (5, 257, 1)])
def test_error_map_batch_with_an_undrawn_cell(gpu, M, N, n_intr):
    from sanerf_hq_amd import raymarching as rm
    data = dataset(M, n_intr, 3, np.int64)
    t = on(gpu, data)
    rng = np.random.default_rng(N + 5 * M)
    index = M - 1
    if N <= S * S:                                                   # the cells through the draw itself: a map with too few positive cells leaves -1 behind
        emap = data["error_map"].copy()
        emap[index, rng.permutation(S * S)[max(N - 1, 0):]] = 0.0
        e = rng.standard_exponential((1, S * S)).astype(np.float32)
        cells, status = rm.weighted_draw(torch.from_numpy(emap).to(gpu), torch.from_numpy(e).to(gpu), N, row_index=torch.tensor([index], device=gpu))
        want_cells, _ = R.weighted_draw(emap, e, N, row_index=[index])
        assert np.array_equal(cells.cpu().numpy(), want_cells) and int(status.item()) == 1 and want_cells[0, -1] == -1
    else:                                                            # more rays than cells: no draw without replacement gives these, the gather takes them
        want_cells = rng.integers(0, S * S, (1, N))
        want_cells[0, -1] = -1
        cells = torch.from_numpy(want_cells).to(gpu)
    u = uniforms(rng, N, 2)
    for idx in (index, torch.tensor([index], device=gpu)):          # the image index on the host, or on the device
        res = rm.collate_gather(t["poses"], t["intrinsics"], H, W, u=torch.from_numpy(u).to(gpu), cells=cells, index=idx, images=t["images"],
                                masks=t["masks"], error_map=t["error_map"], cam_near_far=t["cam_near_far"], error_map_size=S)
        want = R.gather(data, H, W, N, mode="error_map", u=u, cells=want_cells[0], index=index, S=S)
        check_against_restatement(res, want)
        check_against_torch(gpu, t, res, want, N)
        assert int(res["i"][-1]) == -1 and int(res["j"][-1]) == -1 and int(res["inds_coarse"][-1]) == -1 and int(res["index"][-1]) == index
        assert torch.isnan(res["images"][-1]).all() and torch.isnan(res["error_maps"][-1]) and (res["masks"][-1] == 0).all()
        assert torch.equal(res["inds_coarse"][:-1], cells[0, :-1])


def test_strided_outputs_leave_the_padding_alone_and_optional_outputs_may_be_absent(gpu):
    from sanerf_hq_amd import raymarching as rm
    M, N, L, p = 5, 257, 3, 4
    data = dataset(M, 5, 4, np.float32)
    t = on(gpu, data)
    rng = np.random.default_rng(77)
    u, ul = uniforms(rng, N, 3), rng.random(L, dtype=np.float32)
    centres = rng.integers(0, S * S, L)
    total = N + L * p * p
    want = R.gather(data, H, W, N, u=u, S=S, L=L, p=p, ul=ul, centres=centres)
    fbuf = torch.full((total, 40), -3.0, device=gpu)                  # rays_o 1:4, rays_d 5:8, error_maps 9, cam_near_far 11:13, masks 14:16, poses 17:33, intrinsics 34:38
    ibuf = torch.full((total, 7), -9, device=gpu, dtype=torch.int64)  # index 0, i 2, j 3, inds_coarse 5
    img = torch.full((N, 6), -3.0, device=gpu)
    out = {"rays_o": fbuf[:, 1:4], "rays_d": fbuf[:, 5:8], "error_maps": fbuf[:, 9], "cam_near_far": fbuf[:, 11:13], "masks": fbuf[:, 14:16],
           "poses": fbuf[:, 17:33], "intrinsics": fbuf[:, 34:38], "index": ibuf[:, 0], "i": ibuf[:, 2], "j": ibuf[:, 3], "inds_coarse": ibuf[:, 5],
           "images": img[:, 1:5]}
    args = dict(u=torch.from_numpy(u).to(gpu), images=t["images"], masks=t["masks"], error_map=t["error_map"], cam_near_far=t["cam_near_far"],
                error_map_size=S, ul=torch.from_numpy(ul).to(gpu), centres=torch.from_numpy(centres).to(gpu), patch_size=p)
    res = rm.collate_gather(t["poses"], t["intrinsics"], H, W, out=out, **args)
    assert res is out
    check_against_restatement(res, want)
    used = torch.zeros(40, dtype=torch.bool)
    for a, b in ((1, 4), (5, 8), (9, 10), (11, 13), (14, 16), (17, 33), (34, 38)):
        used[a:b] = True
    assert (fbuf[:, ~used.to(gpu)] == -3.0).all() and (ibuf[:, [1, 4, 6]] == -9).all() and (img[:, [0, 5]] == -3.0).all(), "the padding is untouched"
    # optional outputs left out: the others are the same
    few = rm.collate_gather(t["poses"], t["intrinsics"], H, W, want=("rays_d", "j", "masks"), **args)
    assert set(few) == {"rays_d", "j", "masks"}
    assert torch.equal(few["rays_d"], res["rays_d"]) and torch.equal(few["j"], res["j"]) and torch.equal(few["masks"], res["masks"])
    bare = rm.collate_gather(t["poses"], t["intrinsics"], H, W, u=torch.from_numpy(u).to(gpu))      # no supervision tensors at all
    assert set(bare) == {"rays_o", "rays_d", "index", "i", "j", "inds_coarse", "poses", "intrinsics"} and torch.equal(bare["rays_o"], res["rays_o"][:N])
    assert same(bare["inds_coarse"], R.coarse_index(want["row"][:N], want["col"][:N], H, W, H)), "without an error map the coarse cells are collate_rays's H-sized ones"
    with pytest.raises(RuntimeError, match="need the dataset tensor"):
        rm.collate_gather(t["poses"], t["intrinsics"], H, W, u=torch.from_numpy(u).to(gpu), want=("images",))
    with pytest.raises(RuntimeError, match="unit column stride"):
        rm.collate_gather(t["poses"], t["intrinsics"], H, W, u=torch.from_numpy(u).to(gpu), out={"rays_o": fbuf[:N, 1:7:2]})


# ---- DeviceCollate ----------------------------------------------------------------------------------------------------------------------
def restated_batch(dc, data, randoms, index=0):
    """The restatement evaluated on a DeviceCollate's random tensors (host copies)."""
    r = {k: v.cpu().numpy() for k, v in randoms.items()}
    emap = data["error_map"]
    cells = centres = None
    if dc.cells_mode:
        cells = R.weighted_draw(emap, r["expo"], dc.N, row_index=[index])[0][0]
    if dc.L > 0:
        centres = R.weighted_draw(emap, r["expo_local"], 1, row_u=r["ul"])[0][:, 0]
    return R.gather(data, dc.H, dc.W, dc.N, mode="error_map" if dc.cells_mode else "uniform", u=r["u"], cells=cells, index=index, S=dc.S,
                    L=dc.L, p=dc.p, ul=r.get("ul"), centres=centres)


def check_batch(res, want, N):
    for k in ("rays_o", "rays_d", "masks", "error_maps", "cam_near_far"):
        assert same(res[k], want[k]), k
    for k in ("index", "i", "j", "inds_coarse", "images"):
        assert same(res[k], want[k][:N]), k
    assert same(res["poses"], want["poses"].reshape(-1, 4, 4))


@pytest.mark.parametrize("cells_mode", [False, True])
def test_device_collate_is_a_function_of_its_randoms(gpu, cells_mode):
    from sanerf_hq_amd.nerf import DeviceCollate, collate_rays
    M, N = 5, (255 if cells_mode else 257)                           # at most S * S cells can be drawn without replacement
    data = dataset(M, 5, 3, np.int64)
    t = on(gpu, data)
    dc = DeviceCollate(t["poses"], t["intrinsics"], H, W, N, images=t["images"], masks=t["masks"], error_map=t["error_map"], cam_near_far=t["cam_near_far"],
                       random_image_batch=not cells_mode, use_error_map=cells_mode, error_map_size=S, num_local_sample=4, local_patch_size=8, index=3)
    g = torch.Generator(device=gpu).manual_seed(5)
    r = {k: (torch.empty_like(v).exponential_(generator=g) if k.startswith("expo") else torch.rand(v.shape, device=gpu, generator=g)) for k, v in dc.randoms.items()}
    first = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in dc.draw(randoms=r).items()}
    dc.draw()                                                        # something else in between
    second = dc.draw(randoms=r)
    for k, v in first.items():
        assert (torch.equal(v, second[k]) or same(v, second[k].cpu().numpy())) if torch.is_tensor(v) else v == second[k], k
    check_batch(second, restated_batch(dc, data, r, index=3), N)
    assert int(dc.status.item()) == 0
    # the keys and shapes of collate_rays
    ref = collate_rays(t["poses"], t["intrinsics"], H, W, N, index=3, images=t["images"], masks=t["masks"], error_map=t["error_map"], cam_near_far=t["cam_near_far"],
                       random_image_batch=not cells_mode, use_error_map=cells_mode, error_map_size=S, num_local_sample=4, local_patch_size=8)
    assert set(ref) == set(second)
    for k, v in ref.items():
        if torch.is_tensor(v) and k not in ("index", "inds_coarse", "intrinsics", "poses") + (("cam_near_far",) if cells_mode else ()):      # [1, ..] there
            assert v.shape == second[k].shape and v.dtype == second[k].dtype, k
    assert second["index"].shape == (N,) and second["inds_coarse"].shape == (N,) and second["poses"].shape == (N + 4 * 64, 4, 4)


def test_device_collate_replays_in_a_graph(gpu):
    """draw() captured on one stream -- a linear graph of the random fills and the two launches -- and replayed: every replay is the
    restatement of the randoms it drew, and successive replays draw different batches."""
    from sanerf_hq_amd.nerf import DeviceCollate
    M, N = 5, 255
    data = dataset(M, 1, 4, np.uint8)
    t = on(gpu, data)
    dc = DeviceCollate(t["poses"], t["intrinsics"], H, W, N, images=t["images"], masks=t["masks"], error_map=t["error_map"], cam_near_far=t["cam_near_far"],
                       error_map_size=S, num_local_sample=3, local_patch_size=4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dc.draw()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = dc.draw()
    seen = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        check_batch(res, restated_batch(dc, data, dc.randoms), N)
        seen.append((res["rays_d"].clone(), dc.randoms["u"].clone()))
    assert int(dc.status.item()) == 0
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(seen[a][1], seen[b][1]) and not torch.equal(seen[a][0], seen[b][0]), "successive replays differ"
