"""GPU: the mask field's output stage (rm.mask_output) and the device-side evaluation meters (rm.mask_eval_accumulate,
rm.image_sqerr_accumulate, nerf.mask_output.DeviceMeters) against tests/golden/mask_output.npz -- the reference's own test_step / eval_step
lines, overlays and meters run on the CPU (tools/gen_golden_mask_output.py).  Tolerances: ids, 8-bit images and class counts equal; float
outputs rtol 1e-5 (that of test_gpu_mask_losses.py); mIoU rtol 1e-12 (integer counts, one double division per class)."""

import numpy as np
import pytest
import torch

from helpers import golden, make_opt, synthetic_params
from test_mask_output_host import CASES, VARIANTS, eval_f64

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def image_of(g, case, dev):
    """The case's image on the device; the strided cases as the image columns of a packed [N,5] render buffer."""
    img = T(g[case + ".image"], dev)
    if case in list(g["strided_cases"]):
        packed = torch.full((img.shape[0], 5), float("nan"), device=dev)
        packed[:, :3] = img
        img = packed[:, :3]
        assert img.stride(0) == 5
    return img


def close(got, want, what, rtol=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    rel = np.where(got == want, 0.0, rel)
    print(f"{what}: max rel diff {rel.max():.3e} (bar {rtol:.0e})")
    assert (rel <= rtol).all(), (what, float(rel.max()))


@pytest.mark.parametrize("case", CASES)
def test_mask_output_equals_the_reference_fixture(gpu, case):
    from sanerf_hq_amd import raymarching as rm
    g = golden("mask_output")
    cm, bg, alpha = T(g["color_map"], gpu), T(g["bg"], gpu), float(g["alpha"])
    logits, img = T(g[case + ".logits"], gpu), image_of(g, case, gpu)
    one = int(g[case + ".render_one"])
    for mode, r in VARIANTS:
        o = rm.mask_output(logits, color_map=cm, image=img, mode=mode, render_id=-1 if r == "all" else one, alpha=alpha, bg_color=bg)
        tag = f"{case}.{mode}.{r}"
        assert np.array_equal(o["instance_id"].cpu().numpy(), g[case + ".ids"]), tag
        assert o["instance_id"].dtype == torch.int64 and o["rgb8"].dtype == torch.uint8
        close(o["probs"].cpu().numpy(), g[case + ".probs"], tag + " probs")
        close(o["confidence"].cpu().numpy(), g[case + ".conf"], tag + " confidence")
        close(o["rgb"].cpu().numpy(), g[tag + ".rgb"], tag + " rgb")
        got8, want8 = o["rgb8"].cpu().numpy(), g[tag + ".rgb8"]
        print(f"{tag} rgb8: {(got8 != want8).sum()} of {want8.size} bytes differ")
        assert np.array_equal(got8, want8), tag
    o = rm.mask_output(logits, image=img, mode="none", want=("rgb", "rgb8"))
    assert np.array_equal(o["rgb"].cpu().numpy(), g[case + ".image"]) and np.array_equal(o["rgb8"].cpu().numpy(), g[case + ".none.rgb8"])


@pytest.mark.parametrize("case", CASES + ("k3_unlabelled",))
def test_eval_accumulate_equals_the_reference_fixture(gpu, case):
    from sanerf_hq_amd import raymarching as rm
    g = golden("mask_output")
    src = "k3" if case == "k3_unlabelled" else case
    C = int(g[src + ".shape"][3])
    rec, ws = rm.eval_record(gpu), rm.eval_workspace(gpu)
    rm.mask_eval_accumulate(T(g[src + ".logits"], gpu), T(g[case + ".labels"], gpu), rec, ws, float(g["epsilon"]), num_classes=C)
    r = rm.read_eval_record(rec)
    counts = g[case + ".eval_counts"]
    assert r["images"] == 1 and r["rgb_images"] == 0
    assert np.array_equal(r["inter"], counts[0]) and np.array_equal(r["pred"], counts[1]) and np.array_equal(r["truth"], counts[2])
    close(r["miou_sum"], float(g[case + ".eval_miou"]), case + " mIoU", rtol=1e-12)
    close(r["nll_mean_sum"], float(g[case + ".eval_loss"]), case + " NLL mean")
    assert not ws.any(), "the workspace is zero at rest"


def test_sqerr_accumulate_equals_the_reference_meters(gpu):
    from sanerf_hq_amd import raymarching as rm
    g = golden("mask_output")
    for i in range(3):
        rec, ws = rm.eval_record(gpu), rm.eval_workspace(gpu)
        pred = T(g[f"meters3.{i}.pred"], gpu)
        if i == 1:                                       # the prediction as the image columns of a packed render buffer
            packed = torch.zeros(pred.shape[0], 5, device=gpu)
            packed[:, :3] = pred
            pred = packed[:, :3]
        rm.image_sqerr_accumulate(pred, T(g[f"meters3.{i}.truth"], gpu), rec, ws)
        r = rm.read_eval_record(rec)
        assert r["rgb_images"] == 1 and r["images"] == 0 and not ws.any()
        close(r["mse_sum"], float(g[f"meters3.{i}.mse"]), f"image {i} MSE")
        close(r["psnr_sum"], float(g[f"meters3.{i}.psnr"]), f"image {i} PSNR")


def test_device_meters_over_three_images_equal_the_reference_meters(gpu):
    from sanerf_hq_amd.nerf.mask_output import DeviceMeters
    g = golden("mask_output")
    meters = DeviceMeters(gpu, eps=float(g["epsilon"]))
    assert meters.measure() == {"mIoU": 0, "loss": 0, "PSNR": 0, "MSE": 0}
    for rnd in range(2):                                 # clear() starts a new epoch
        for i in range(3):
            meters.update_mask(T(g[f"meters3.{i}.logits"], gpu), T(g[f"meters3.{i}.labels"], gpu))
            meters.update_rgb(T(g[f"meters3.{i}.pred"], gpu), T(g[f"meters3.{i}.truth"], gpu))
        m = meters.measure()
        want = g["meters3.measure"]
        close(m["mIoU"], want[0], "mIoU", rtol=1e-12)
        close(m["loss"], want[1], "loss")
        close(m["PSNR"], want[2], "PSNR")
        close(m["MSE"], want[3], "MSE")
        meters.clear()
        assert meters.read()["images"] == 0


@pytest.mark.parametrize("N,K,C", [(1, 1, 1), (255, 2, 5), (70000, 4, 4), (512 * 256 * 2 + 77, 5, 7), (40000, 16, 32), (33333, 31, 32)])
def test_other_sizes_equal_the_float64_restatement_and_two_runs_give_equal_bits(gpu, N, K, C):
    """Sizes the fixture does not hold (one pixel; more tiles than workgroups of the accumulating launch; every K template step; C > K
    with labels in K..C-1 and above C-1), against the float64 restatement of test_mask_output_host.py; pixels whose two largest
    probabilities are closer than 1e-3 get a clear winner first.  Two runs: equal bits in every output and in the record."""
    from sanerf_hq_amd import raymarching as rm
    rng = np.random.default_rng(N + K)
    logits = (rng.standard_normal((N, K)) * 2.0).astype(np.float32)
    if K > 1:
        top = np.sort(logits, -1)
        logits[np.arange(N), logits.argmax(-1)] += np.where(top[:, -1] - top[:, -2] < 0.05, 1.0, 0.0).astype(np.float32)
    labels = rng.integers(-1, C + 2, N).astype(np.int64)
    cm = rng.uniform(0.05, 1.0, (C, 3)).astype(np.float32)
    img = rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32)
    if K > 1:
        e = np.exp(logits.astype(np.float64) - logits.max(-1, keepdims=True))
        p = np.sort(e / e.sum(-1, keepdims=True), -1)
        assert (p[:, -1] - p[:, -2]).min() >= 1e-3
    loss, miou, counts = eval_f64(logits, labels, C, 1e-6)
    runs = []
    for _ in range(2):
        rec, ws = rm.eval_record(gpu), rm.eval_workspace(gpu)
        lg, lb, im = T(logits, gpu), T(labels, gpu), T(img, gpu)
        o = rm.mask_output(lg, color_map=T(cm, gpu), image=im, mode="composition", render_id=-1)
        rm.mask_eval_accumulate(lg, lb, rec, ws, 1e-6, num_classes=C)
        rm.image_sqerr_accumulate(o["rgb"], im, rec, ws)
        runs.append({**{k: v.cpu().numpy() for k, v in o.items()}, "record": rec.cpu().numpy()})
        assert not ws.any()
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    r = rm.read_eval_record(T(runs[0]["record"], gpu))
    assert np.array_equal(np.stack([r["inter"], r["pred"], r["truth"]]).astype(np.int64), counts)
    close(r["miou_sum"], miou, "mIoU", rtol=1e-12)
    close(r["nll_mean_sum"], loss, "NLL mean")
    e = np.exp(logits.astype(np.float64) - logits.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True) if K > 1 else 1 / (1 + np.exp(-logits.astype(np.float64)))
    assert np.array_equal(runs[0]["instance_id"], p.argmax(-1))
    close(runs[0]["probs"], p, "probs")
    want = img.astype(np.float64) * np.float32(0.7) + cm.astype(np.float64)[p.argmax(-1)] * np.float32(1 - np.float32(0.7))
    close(runs[0]["rgb"], want, "rgb")
    d = runs[0]["rgb"].astype(np.float32) - img
    close(r["mse_sum"], float((d.astype(np.float64) ** 2).mean()), "MSE", rtol=1e-12)


def test_null_outputs_are_honoured_and_untouched_buffers_keep_their_bits(gpu):
    from sanerf_hq_amd import raymarching as rm
    g = golden("mask_output")
    logits, img, cm = T(g["k8.logits"], gpu), T(g["k8.image"], gpu), T(g["color_map"], gpu)
    N, K = logits.shape
    full = rm.mask_output(logits, color_map=cm, image=img, mode="composition")
    names = ("probs", "instance_id", "confidence", "rgb", "rgb8")
    for keep in names:
        big8 = torch.full((N + 8, 3), 0xAB, device=gpu, dtype=torch.uint8)
        out = {"probs": torch.full((N, K), -7.0, device=gpu), "instance_id": torch.full((N,), -7, device=gpu, dtype=torch.int64),
               "confidence": torch.full((N,), -7.0, device=gpu), "rgb": torch.full((N, 3), -7.0, device=gpu), "rgb8": big8[:N]}
        before = {k: v.clone() for k, v in out.items()}
        res = rm.mask_output(logits, color_map=cm, image=img, mode="composition", want=(keep,), out=out)
        assert res is out
        for k in names:
            assert torch.equal(out[k], full[k] if k == keep else before[k]), (keep, k)
        assert (big8[N:] == 0xAB).all(), "the dword stores of the 8-bit image stop at its last byte"
    # ids alone need neither image nor colour table
    ids = rm.mask_output(logits, want=("instance_id",))
    assert set(ids) == {"instance_id"} and torch.equal(ids["instance_id"], full["instance_id"])


def test_mask_mode_background_forms_and_preallocated_outputs(gpu):
    """'mask' mode: a background given as three numbers, as a number and as a device tensor give the same bits (numbers reach the device
    through fills, which a graph can capture); a preallocated output of the wrong shape or dtype raises and is not replaced."""
    from sanerf_hq_amd import raymarching as rm
    g = golden("mask_output")
    logits, img = T(g["k3.logits"], gpu), T(g["k3.image"], gpu)
    bg = [float(v) for v in g["bg"]]
    a = rm.mask_output(logits, image=img, mode="mask", render_id=2, bg_color=tuple(bg), want=("rgb",))["rgb"]
    b = rm.mask_output(logits, image=img, mode="mask", render_id=2, bg_color=T(g["bg"], gpu), want=("rgb",))["rgb"]
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), g["k3.mask.one.rgb"])
    c = rm.mask_output(logits, image=img, mode="mask", render_id=2, bg_color=0.25, want=("rgb",))["rgb"]
    d = rm.mask_output(logits, image=img, mode="mask", render_id=2, bg_color=[0.25] * 3, want=("rgb",))["rgb"]
    assert torch.equal(c, d)
    N = logits.shape[0]
    for bad in (torch.zeros(N, 4, device=gpu), torch.zeros(N, 3, device=gpu, dtype=torch.float64), torch.zeros(N, 6, device=gpu)[:, ::2]):
        out = {"rgb": bad}
        with pytest.raises(RuntimeError, match="out\\['rgb'\\]"):
            rm.mask_output(logits, image=img, mode="none", want=("rgb",), out=out)
        assert out["rgb"] is bad


@pytest.mark.parametrize("K", [1, 2, 3, 8, 32])
def test_non_finite_logits_follow_torch(gpu, K):
    """DESIGN.md section 4.1 extended to the output stage: NaN and +-inf logits give the ids and probabilities of torch's own softmax
    (sigmoid for K = 1), max and argmax on the same device -- a row with a NaN or +inf, or all -inf, is NaN throughout and its id is 0."""
    from sanerf_hq_amd import raymarching as rm
    torch.manual_seed(K)
    N = 600
    logits = torch.randn(N, K, device=gpu) * 2.0
    logits[torch.arange(N, device=gpu), torch.randint(0, K, (N,), device=gpu)] += 1.5
    specials = [float("nan"), float("inf"), float("-inf")]
    for i in range(0, 300):
        logits[i, (i * 7) % K] = specials[i % 3]
    logits[300:310] = float("-inf")
    logits[310:320] = float("inf")
    logits[320, 0], logits[320, K - 1] = float("inf"), float("-inf")
    o = rm.mask_output(logits, want=("probs", "instance_id", "confidence"))
    p = torch.softmax(logits, -1) if K > 1 else torch.sigmoid(logits)
    conf, ids = torch.max(p, -1)
    assert torch.equal(o["instance_id"], ids)
    assert torch.equal(torch.isnan(o["probs"]), torch.isnan(p)) and torch.equal(torch.isnan(o["confidence"]), torch.isnan(conf))
    fin = ~torch.isnan(p)
    close(o["probs"][fin].cpu().numpy(), p[fin].cpu().numpy(), "finite probabilities")
    # the 8-bit image: NaN -> 0, saturation at both ends
    img = torch.tensor([[float("nan"), -0.5, 2.0], [0.0, 1.0, 0.5]], device=gpu)
    o8 = rm.mask_output(logits[:2], image=img, mode="none", want=("rgb8",))
    assert o8["rgb8"].cpu().tolist() == [[0, 0, 255], [0, 255, 127]]


def test_render_to_image_and_meters_in_one_captured_graph(gpu):
    """A small mask-mode model.render (packed route) -> mask_test_outputs + mask_eval_step, captured with torch.cuda.graph as a single
    chain on one stream and replayed twice on fresh rays: every replay equals the eager run bit for bit, the meters' record included."""
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf import NeRFNetwork
    from sanerf_hq_amd.nerf.mask_output import DeviceMeters, mask_eval_step, mask_test_outputs
    steps = [48, 24, 16]
    params = synthetic_params(steps, heads=True, seed=5)
    opt = make_opt(num_steps=steps, with_mask=True, n_inst=2, render_mask_type="composition", render_mask_instance_id=-1)
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    model = model.to(gpu).eval()
    H = W = 40
    poses = [synth.orbit_pose(1.0, 20.0, a) for a in (30.0, 75.0, 140.0)]
    rays = [rm.generate_rays(p, synth.pinhole_intrinsics(H, W), H, W, device=gpu) for p in poses]
    cm = torch.from_numpy(golden("mask_output")["color_map"]).to(gpu)
    labels = torch.from_numpy((synth.hash_u01(H * W, 3) * 3).astype(np.int64) - 1).to(gpu)        # -1, 0, 1
    ro, rd = rays[0][0].clone(), rays[0][1].clone()
    packed = torch.zeros(H * W, 5, device=gpu)
    meters = DeviceMeters(gpu)

    def chain(meters):
        with torch.no_grad():
            o = model.render(ro, rd, staged=False, perturb=False, return_mask=1, H=H, W=W, tile_w=W, packed=packed)
            assert o["image"].data_ptr() == packed.data_ptr() and o["image"].stride(0) == 5, "the packed route hands out a view of the buffer"
            t = mask_test_outputs(o, opt, cm, bg_color=1.0, rgb8=True)
            mask_eval_step(o, {"masks": labels}, opt, meters)
            return o["instance_mask_logits"], t

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(meters)                                    # warm-up: plans, workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    meters.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg, t = chain(meters)
    replays = []
    for a, b in rays[1:]:
        ro.copy_(a); rd.copy_(b)
        graph.replay()
        replays.append({"logits": lg.clone(), **{k: v.clone() for k, v in t.items()}})
    torch.cuda.synchronize()
    record = meters.record.clone()
    eager = DeviceMeters(gpu)
    for (a, b), rep in zip(rays[1:], replays):
        ro.copy_(a); rd.copy_(b)
        lg2, t2 = chain(eager)
        assert torch.isfinite(lg2).all() and float(lg2.std()) > 0
        assert torch.equal(rep["logits"], lg2)
        for k in t2:
            assert torch.equal(rep[k], t2[k]), k
    assert not torch.equal(replays[0]["logits"], replays[1]["logits"]), "the two replays saw different rays"
    assert torch.equal(record, eager.record)
    m = eager.measure()
    assert eager.read()["images"] == 2 and 0.0 <= m["mIoU"] <= 1.0 and np.isfinite(m["loss"]) and m["loss"] > 0
