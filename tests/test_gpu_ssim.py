"""GPU: the device-side SSIM meter (rm.image_ssim_accumulate, DeviceMeters(ssim=True), nerf.metrics.SSIMMeter) against the fp64 statement
of tests/ssim_ref64.py.  Bound: |value - fp64| <= 1e-4, the project's bar against the reference; for scale, the fp32
torch-operator statement is 2e-7 .. 1.6e-5 from fp64 on these shapes.  Every case prints the error it shows."""
import functools

import numpy as np
import pytest
import torch

import ssim_ref64 as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-4
TILE_W, TILE_H, MAX_WORKGROUPS = 32, 16, 512         # csrc/ssim.hip: SS_TW, SS_TH, SS_MAX_PARTIALS
# the smallest near-square image whose tile count (19 x 27 = 513) exceeds the launch's workgroup count, ragged in both directions
LOOP_H, LOOP_W = 10 + 26 * TILE_H + 1, 10 + 18 * TILE_W + 1
assert -(-(LOOP_H - 10) // TILE_H) * -(-(LOOP_W - 10) // TILE_W) == MAX_WORKGROUPS + 1

CASES = {
    # name: (H, W, kind)
    "one_pixel": (11, 11, "smooth"),
    "one_tile_row": (12, 75, "smooth"),
    "tiles_37x45": (37, 45, "smooth"),
    "tiles_37x45_noise": (37, 45, "noise"),
    "tiles_70x133": (70, 133, "smooth"),
    "tiles_70x133_noise": (70, 133, "noise"),
    "stride5_70x133": (70, 133, "smooth"),
    "tile_loop": (LOOP_H, LOOP_W, "smooth"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pred, truth) float32 [H,W,3] on the CPU and the fp64 values {None: derived range, 1.0: explicit}; computed once per session."""
    H, W, kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 7)
    if kind == "noise":
        pred, truth = rng.random((H, W, 3)), rng.random((H, W, 3))
    else:
        yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
        truth = np.clip(np.stack([0.5 + 0.4 * np.sin(9 * xx + 5 * yy), 0.5 + 0.4 * np.cos(7 * yy - 3 * xx), 0.1 + 0.8 * xx * yy], -1), 0, 1)
        pred = np.clip(truth + 0.08 * rng.standard_normal(truth.shape), 0, 1)
    pred, truth = torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(truth.astype(np.float32))
    want = {dr: ref.ssim_valid(pred, truth, dr) for dr in (None, 1.0)}
    return pred, truth, want


def on_device(name, dev):
    pred, truth, want = case(name)
    H, W = pred.shape[:2]
    p, t = pred.to(dev), truth.to(dev)
    if name.startswith("stride5"):                       # the prediction as the image columns of a packed [N,5] render buffer
        packed = torch.full((H * W, 5), float("nan"), device=dev)
        packed[:, :3] = p.reshape(-1, 3)
        p = packed[:, :3]
        assert p.stride(0) == 5
        t = t.reshape(-1, 3)
    return p, t, H, W, want


def one_value(p, t, dev, H=None, W=None, data_range=None):
    from sanerf_hq_amd import raymarching as rm
    rec, ws = rm.ssim_record(dev), rm.ssim_workspace(dev)
    rm.image_ssim_accumulate(p, t, rec, ws, H=H, W=W, data_range=data_range)
    r = rm.read_ssim_record(rec)
    assert r["images"] == 1 and not ws.any(), "one image counted, the workspace is zero at rest"
    assert r["ssim_sum"] == r["last"] or (np.isnan(r["ssim_sum"]) and np.isnan(r["last"]))
    return r["last"], rec


@pytest.mark.parametrize("data_range", [None, 1.0], ids=["derived", "explicit"])
@pytest.mark.parametrize("name", list(CASES))
def test_value_equals_the_fp64_statement(gpu, name, data_range):
    p, t, H, W, want = on_device(name, gpu)
    got, _ = one_value(p, t, gpu, H, W, data_range)
    f32 = ref.ssim_f32_torch(*case(name)[:2], data_range)
    err = abs(got - want[data_range])
    print(f"ssim {name} {H}x{W} data_range={'derived' if data_range is None else data_range}: kernel {got:.9f} fp64 {want[data_range]:.9f} "
          f"|err| {err:.3e} (bound {BOUND:.0e}; fp32 torch statement {abs(f32 - want[data_range]):.3e})")
    assert err <= BOUND


def test_near_constant_images_need_centred_moments(gpu):
    """truth = 0.999, pred equal but for a 10 x 10 square of 0.998, derived data_range 1e-3 (c2 = 9e-10): raw fp32 moments give -1.84."""
    truth = torch.full((64, 64, 3), 0.999, dtype=torch.float32)
    pred = truth.clone()
    pred[10:20, 10:20] = 0.998
    want = ref.ssim_valid(pred, truth)
    assert abs(want - 0.88949) < 1e-4
    got, _ = one_value(pred.to(gpu), truth.to(gpu), gpu)
    print(f"ssim near_constant 64x64 data_range=derived: kernel {got:.9f} fp64 {want:.9f} |err| {abs(got - want):.3e} (bound {BOUND:.0e}; "
          f"fp32 torch statement {abs(ref.ssim_f32_torch(pred, truth) - want):.3e})")
    assert abs(got - want) <= BOUND


def test_nan_and_degenerate_inputs(gpu):
    p, t, H, W, _ = on_device("tiles_37x45", gpu)
    p = p.clone()
    p[20, 30, 1] = float("nan")
    for dr in (None, 1.0):
        last, rec = one_value(p, t, gpu, data_range=dr)
        assert np.isnan(last), dr
    c = torch.full((37, 45, 3), 0.5, device=gpu)
    last, _ = one_value(c, c.clone(), gpu)
    assert np.isnan(last), "both images constant, derived range 0: 0 / 0"
    last, _ = one_value(c, c.clone(), gpu, data_range=1.0)
    assert last == 1.0


def test_three_pairs_accumulate_in_order(gpu):
    from sanerf_hq_amd import raymarching as rm
    rec, ws = rm.ssim_record(gpu), rm.ssim_workspace(gpu)
    lasts, total = [], 0.0
    for name, dr in (("tiles_70x133", None), ("stride5_70x133", 1.0), ("tiles_37x45_noise", None)):
        p, t, H, W, want = on_device(name, gpu)
        rm.image_ssim_accumulate(p, t, rec, ws, H=H, W=W, data_range=dr)
        r = rm.read_ssim_record(rec)
        assert abs(r["last"] - want[dr]) <= BOUND
        lasts.append(r["last"])
        total += r["last"]                                # Python floats: the double sum, in order
        assert r["images"] == len(lasts) and r["ssim_sum"] == total
    assert len(set(lasts)) == 3 and not ws.any()


@pytest.mark.parametrize("name", ["tiles_70x133_noise", "tile_loop"])
def test_two_runs_give_equal_bits(gpu, name):
    p, t, H, W, _ = on_device(name, gpu)
    for dr in (None, 1.0):
        (_, a), (_, b) = one_value(p, t, gpu, H, W, dr), one_value(p, t, gpu, H, W, dr)
        assert torch.equal(a, b)


def test_device_meters_update_rgb_in_a_captured_graph(gpu):
    """DeviceMeters(ssim=True).update_rgb captured on one stream and replayed: the records equal the eager ones bit for bit; PSNR and MSE
    are what the default meters give."""
    from sanerf_hq_amd.nerf.mask_output import DeviceMeters
    p, t, H, W, want = on_device("tiles_70x133", gpu)
    eager, plain = DeviceMeters(gpu, ssim=True), DeviceMeters(gpu)
    eager.update_rgb(p, t)
    plain.update_rgb(p, t)
    me, mp = eager.measure(), plain.measure()
    assert list(mp) == ["mIoU", "loss", "PSNR", "MSE"] and list(me) == ["mIoU", "loss", "PSNR", "MSE", "SSIM"]
    assert all(me[k] == mp[k] for k in mp) and torch.equal(eager.record, plain.record), "ssim=True leaves the other meters alone"
    assert abs(me["SSIM"] - want[None]) <= BOUND

    meters = DeviceMeters(gpu, ssim=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meters.update_rgb(p, t)                          # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    meters.clear()
    assert meters.measure()["SSIM"] == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        meters.update_rgb(p, t)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(meters.ssim_record, eager.ssim_record) and torch.equal(meters.record, eager.record)
    assert not meters.ssim_workspace.any()
    # rows with explicit H, W: the same bits
    rows = DeviceMeters(gpu, ssim=True)
    rows.update_rgb(p.reshape(-1, 3), t.reshape(-1, 3), H=H, W=W)
    assert torch.equal(rows.ssim_record, eager.ssim_record)


def test_ssim_meter_has_the_reference_surface(gpu):
    from sanerf_hq_amd.nerf.metrics import SSIMMeter
    meter = SSIMMeter(device=gpu)
    assert meter.measure() == 0
    wants = []
    for name, batch in (("tiles_37x45", False), ("tiles_70x133_noise", True)):
        pred, truth, want = case(name)
        meter.update(pred[None].to(gpu) if batch else pred.to(gpu), truth[None] if batch else truth)     # a host truth is moved, as the reference does
        wants.append(want[None])
    got = meter.measure()
    print(f"ssim meter: measure {got:.9f} fp64 mean {np.mean(wants):.9f} |err| {abs(got - np.mean(wants)):.3e}")
    assert abs(got - np.mean(wants)) <= BOUND
    assert meter.report() == f"SSIM = {got:.6f}"

    class Writer:
        def add_scalar(self, tag, value, step):
            self.seen = (tag, value, step)
    w = Writer()
    meter.write(w, 3, prefix="val")
    assert w.seen == ("val/SSIM", got, 3)
    with pytest.raises(RuntimeError, match="batch of 2"):
        meter.update(torch.rand(2, 16, 16, 3, device=gpu), torch.rand(2, 16, 16, 3, device=gpu))
    with pytest.raises(RuntimeError, match="smaller than the 11 x 11 window"):
        meter.update(torch.rand(10, 16, 3, device=gpu), torch.rand(10, 16, 3, device=gpu))
    assert meter.measure() == got, "a refused update adds nothing"
    meter.clear()
    assert meter.measure() == 0
    explicit = SSIMMeter(device=gpu, data_range=1.0)
    pred, truth, want = case("tiles_37x45")
    explicit.update(pred.to(gpu), truth.to(gpu))
    assert abs(explicit.measure() - want[1.0]) <= BOUND
