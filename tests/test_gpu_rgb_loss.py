"""GPU: the loss tail of the RGB training step (sn_rm_rgb_loss / raymarching.rgb_loss / nerf.rgb_step) against its fp64 statement within
the derived round-off bounds (tests/rgb_loss_ref64.py), against what the reference's own train_step / eval_step computed
(tests/golden/rgb_step.npz), and: determinism, non-finite values against torch's chain on the same device tensors, capture and replay,
and the route -- with `--background random` the whole step stays on the fused training route and matches the tensor-background chain."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rgb_loss_ref64 as ref
from helpers import ROOT, make_opt, synthetic_params

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rgb_step.npz"))
TRAIN = [str(c) for c in GOLD["train_cases"]]
EVAL = [str(c) for c in GOLD["eval_cases"]]
CAP_RAYS = 512 * 256                                  # SN_RGB_LOSS_MAX_WORKGROUPS workgroups of 256 lanes: beyond it a lane loops
SIZES = [1, 63, 256, 257, 1000, CAP_RAYS + 1]
MODES = [(ch, bgm, has_bg, lam, ex) for ch in (3, 4) for bgm in ("value", "colour", "per_ray") for has_bg in (True, False)
         for lam in (0.0, 1e-2) for ex in ((), ((0.03, 1.0), (0.004, 0.002)))]
SENTINEL = -77.0
REAL_RAND = torch.rand


def case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + ".")}


def synthetic(N, channels, seed):
    rng = np.random.default_rng(seed)
    image = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    w = rng.uniform(0, 1, N).astype(np.float32)
    k = max(N // 8, 1)
    w[rng.integers(0, N, k)] = rng.choice(np.array([0.0, 1.0, 3e-6, 1.0 - 3e-6, 1.0 + 1e-6], np.float32), k)
    truth = rng.uniform(0, 1, (N, channels)).astype(np.float32)
    return image, w, truth, rng.uniform(0, 1, (N, 3)).astype(np.float32)


class Tail:
    """sn_rm_rgb_loss through ctypes with a workspace of its own (zeroed once), every output in a buffer filled with a sentinel first."""

    def __init__(self, dev):
        from sanerf_hq_amd import _lib
        self.lib, self._lib, self.dev = _lib.lib(), _lib, dev
        assert _lib.RGB_LOSS_MAX_WORKGROUPS * 256 == CAP_RAYS
        self.ws = torch.zeros(_lib.RGB_LOSS_WORKSPACE_BYTES // 8, device=dev, dtype=torch.int64)

    def __call__(self, image, w, truth, bg=1.0, has_bg=True, lam=0.0, extras=(), want=("pred", "gt", "grad_image", "grad_weights_sum")):
        N = image.shape[0]
        assert image.stride(1) == 1 and truth.stride(1) == 1 and w.is_contiguous()
        full = lambda *s: torch.full(s, SENTINEL, device=self.dev, dtype=torch.float32)   # noqa: E731
        out = {"record": full(4)}
        for k, shape in (("pred", (N, 3)), ("gt", (N, 3)), ("grad_image", (N, 3)), ("grad_weights_sum", (N,))):
            out[k] = full(*shape) if k in want else None
        bg_value, bg_t, bg_rows = 0.0, None, 0
        if torch.is_tensor(bg):
            bg_t, bg_rows = bg.contiguous(), (1 if bg.dim() == 1 else N)
        else:
            bg_value = float(bg)
        ex = [(torch.tensor([v], device=self.dev, dtype=torch.float32), c) for v, c in extras] + [(None, 0.0)] * (2 - len(extras))
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = self.lib.sn_rm_rgb_loss(image.data_ptr(), image.stride(0), w.data_ptr(), truth.data_ptr(), truth.stride(0), truth.shape[1], N, bg_value,
                                     p(bg_t), bg_rows, 1 if has_bg else 0, float(lam), p(ex[0][0]), float(ex[0][1]), p(ex[1][0]), float(ex[1][1]),
                                     p(out["pred"]), p(out["gt"]), p(out["record"]), p(out["grad_image"]), p(out["grad_weights_sum"]),
                                     self.ws.data_ptr(), self._lib.stream())
        assert rc == 0, self.lib.sn_last_error().decode()
        torch.cuda.synchronize()
        assert not bool(self.ws.any()), "the workspace is not all zero after the call"
        return out


@pytest.fixture(scope="module")
def tail(gpu):
    return Tail(gpu)


def ratios(r, out):
    rec = out["record"].cpu().numpy().astype(np.float64)
    q = {"total": ref.worst(rec[0], r["total"], r["total_bound"]), "mse": ref.worst(rec[1], r["mse"], r["mse_bound"]),
         "entropy": ref.worst(rec[2], r["entropy"], r["entropy_bound"])}
    assert rec[3] == 0
    for k, name in (("pred", "pred"), ("gt", "gt"), ("grad_image", "grad_image"), ("grad_weights_sum", "grad_weights_sum")):
        if out[k] is not None:
            q[k] = ref.worst(out[k].cpu().numpy(), r[name], r[name + "_bound"])
    return q


@pytest.mark.parametrize("N", SIZES)
def test_kernel_against_the_statement_within_the_derived_bounds(gpu, tail, N):
    """Every bg_rows mode x image_has_bg x 3 and 4 truth channels x lambda_entropy 0 and > 0 x extras absent and present."""
    T = lambda a: torch.from_numpy(a).to(gpu)   # noqa: E731
    top = {}
    inputs = {ch: synthetic(N, ch, 7 * N + ch) for ch in (3, 4)}
    dev_inputs = {ch: tuple(T(a) for a in v) for ch, v in inputs.items()}
    for ch, bgm, has_bg, lam, ex in MODES:
        image, w, truth, bgN = inputs[ch]
        d_image, d_w, d_truth, d_bgN = dev_inputs[ch]
        bg, d_bg = {"value": (0.75, 0.75), "colour": (bgN[0], d_bgN[0].contiguous()), "per_ray": (bgN, d_bgN)}[bgm]
        out = tail(d_image, d_w, d_truth, d_bg, has_bg, lam, ex)
        r = ref.rgb_loss(image, w, truth, bg=bg, image_has_bg=has_bg, lambda_entropy=lam, extras=ex)
        q = ratios(r, out)
        if has_bg:         # where the statement's gradient is exactly 0 (no background term, clamped or absent entropy term) so is the kernel's
            zero = (r["grad_weights_sum"] == 0)
            assert zero.sum() >= (N if lam == 0 else 0) and not bool(out["grad_weights_sum"][T(zero)].any())
        for k, v in q.items():
            top[k] = max(top.get(k, 0.0), v)
        assert max(q.values()) <= 1.0, (ch, bgm, has_bg, lam, len(ex), q)
    print(f"rgb_loss N={N}: worst |err|/bound over {len(MODES)} modes: " + ", ".join(f"{k} {v:.3f}" for k, v in top.items()))


def test_strided_image_and_truth_are_read_in_place(gpu, tail):
    from sanerf_hq_amd import raymarching as rm
    N = 257
    image, w, truth, bgN = synthetic(N, 4, 3)
    T = lambda a: torch.from_numpy(a).to(gpu)   # noqa: E731
    buf = torch.full((N, 4), 9.0, device=gpu)
    buf[:, :3] = T(image)
    tbuf = torch.full((N, 6), 9.0, device=gpu)
    tbuf[:, 1:5] = T(truth)
    want = tail(T(image), T(w), T(truth), T(bgN), False, 1e-2, ())
    got = tail(buf[:, :3], T(w), tbuf[:, 1:5], T(bgN), False, 1e-2, ())
    for k in want:
        assert torch.equal(want[k], got[k]), k
    # the operator hands the views through (no copy: the kernel gets their strides) and gives the same bits
    loss, pred, gt = rm.rgb_loss(buf[:, :3], T(w), tbuf[:, 1:5], bg=T(bgN), image_has_bg=False, lambda_entropy=1e-2)
    assert torch.equal(loss, want["record"][0]) and torch.equal(pred, want["pred"]) and torch.equal(gt, want["gt"])
    assert not pred.requires_grad and not gt.requires_grad
    loss3, pred3, _ = rm.rgb_loss(buf[:, :3], T(w), tbuf[:, 1:4], bg=T(bgN)[0].contiguous(), image_has_bg=True)
    want3 = tail(T(image), T(w), T(truth[:, :3].copy()), T(bgN)[0].contiguous(), True, 0.0, ())
    assert torch.equal(loss3, want3["record"][0]) and torch.equal(pred3, want3["pred"])


def test_null_optional_outputs_leave_the_others_unchanged(gpu, tail):
    N = 1000
    image, w, truth, bgN = synthetic(N, 4, 4)
    a = tuple(torch.from_numpy(x).to(gpu) for x in (image, w, truth, bgN))
    names = ("pred", "gt", "grad_image", "grad_weights_sum")
    full = tail(*a, False, 1e-2, ((0.03, 1.0),))
    for drop in names + (names,):
        drop = (drop,) if isinstance(drop, str) else drop
        got = tail(*a, False, 1e-2, ((0.03, 1.0),), want=tuple(n for n in names if n not in drop))
        assert torch.equal(got["record"], full["record"])
        for n in names:
            assert got[n] is None if n in drop else torch.equal(got[n], full[n]), (drop, n)


@pytest.mark.parametrize("N", [257, CAP_RAYS + 1])
def test_two_calls_give_equal_bits_and_leave_the_workspace_zero(gpu, tail, N):
    image, w, truth, bgN = synthetic(N, 4, 5)
    a = tuple(torch.from_numpy(x).to(gpu) for x in (image, w, truth, bgN))
    one = tail(*a, False, 1e-2, ((0.03, 1.0), (0.004, 0.002)))
    two = tail(*a, False, 1e-2, ((0.03, 1.0), (0.004, 0.002)))
    for k in one:
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k
        assert not bool((one[k] == SENTINEL).any()), f"{k} was not written everywhere"


def torch_chain(image, w, truth, bg, has_bg, lam):
    """trainer.py:364-392 (and renderer.py:353 for the background term) in torch operators, with its autograd."""
    image = image.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    gt = truth[:, :3] * truth[:, 3:] + bg * (1 - truth[:, 3:]) if truth.shape[1] == 4 else truth
    pred = image if has_bg else image + (1 - w).unsqueeze(-1) * bg
    loss = torch.nn.MSELoss(reduction="none")(pred, gt).mean()
    if lam > 0:
        c = w.clamp(1e-5, 1 - 1e-5)
        loss = loss + lam * (-c * torch.log2(c) - (1 - c) * torch.log2(1 - c)).mean()
    gi, gw = torch.autograd.grad(loss, [image, w], allow_unused=True)
    return {"total": loss.detach(), "pred": pred.detach(), "gt": gt, "grad_image": gi, "grad_weights_sum": torch.zeros_like(w) if gw is None else gw}


@pytest.mark.parametrize("has_bg", [False, True])
def test_non_finite_values_reach_the_outputs_torch_gives_them(gpu, tail, has_bg):
    N, lam = 257, 1e-2
    image, w, truth, bgN = synthetic(N, 4, 6)
    w[5] = 0.4                                             # an inside-the-clamp ray for the plants in weights_sum
    base = {k: torch.from_numpy(v).to(gpu) for k, v in (("image", image), ("w", w), ("truth", truth), ("bg", bgN))}
    checked = 0
    for where, index in (("image", (5, 1)), ("w", (5,)), ("truth", (5, 3)), ("bg", (5, 2))):
        for value in (float("nan"), float("inf"), float("-inf")):
            a = {k: v.clone() for k, v in base.items()}
            a[where][index] = value
            got = tail(a["image"], a["w"], a["truth"], a["bg"], has_bg, lam, ())
            want = torch_chain(a["image"], a["w"], a["truth"], a["bg"], has_bg, lam)
            got = dict(got, total=got["record"][0])
            for k in ("total", "pred", "gt", "grad_image", "grad_weights_sum"):
                g, t = got[k], want[k]
                assert torch.equal(torch.isnan(g), torch.isnan(t)), (where, value, k, "NaN where torch has none, or the reverse")
                assert torch.equal(torch.isposinf(g), torch.isposinf(t)) and torch.equal(torch.isneginf(g), torch.isneginf(t)), (where, value, k)
                checked += int((~torch.isfinite(t)).sum())
    assert checked > 24, "the plants reached the outputs"


def _bounds_for(c, torch_chain_bounds=True):
    ex = []
    if bool(c["update_proposal"]) and float(c["lambda_proposal"]) > 0:
        ex.append((float(c["proposal_loss"]), float(c["lambda_proposal"])))
    if float(c["lambda_distort"]) > 0:
        ex.append((float(c["distort_loss"]), float(c["lambda_distort"])))
    return ref.rgb_loss(c["image0"], c["weights_sum"], c["images"], bg=c["bg"], image_has_bg=False, lambda_entropy=float(c["lambda_entropy"]),
                        extras=ex, torch_chain=torch_chain_bounds)


@pytest.mark.parametrize("name", TRAIN)
def test_reference_train_step_through_rgb_train_loss(gpu, name):
    """Loss, gradients (loss.backward(), and once with a grad_out other than 1), pred_rgb and gt_rgb against the reference's values, within
    the bounds re-derived for torch's chain (both sides are within them of the statement; the kernel's own bounds are tighter)."""
    from sanerf_hq_amd.nerf import rgb_train_loss
    c = case(name)
    r = _bounds_for(c)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu)   # noqa: E731
    opt = SimpleNamespace(lambda_proposal=float(c["lambda_proposal"]), lambda_distort=float(c["lambda_distort"]), lambda_entropy=float(c["lambda_entropy"]))
    random_bg = np.ndim(c["bg"]) == 2
    for grad_out in ((None, 0.5) if name == TRAIN[1] else (None,)):
        image0, w = T(c["image0"]).requires_grad_(True), T(c["weights_sum"]).requires_grad_(True)
        prop, dist = T(c["proposal_loss"]).requires_grad_(True), T(c["distort_loss"]).requires_grad_(True)
        if random_bg:       # rendered over 0, the tail adds the background term
            outputs, bg, has_bg = {"image": image0, "weights_sum": w}, T(c["bg"]), False
        else:               # rendered over 1, as NeRFRenderer does it
            outputs, bg, has_bg = {"image": image0 + (1 - w).unsqueeze(-1) * 1, "weights_sum": w}, 1, True
        if bool(c["update_proposal"]):
            outputs["proposal_loss"] = prop
        outputs["distort_loss"] = dist
        pred, gt, loss = rgb_train_loss(outputs, {"images": T(c["images"])}, opt, bg, image_has_bg=has_bg)
        assert not pred.requires_grad and not gt.requires_grad and loss.dim() == 0
        loss.backward() if grad_out is None else loss.backward(gradient=torch.tensor(grad_out, device=gpu))
        s = 1.0 if grad_out is None else 1.0 / grad_out                  # (a power of two: the scaling is exact)
        q = {"loss": ref.worst(float(loss.detach()), c["loss"], r["total_bound"]), "pred": ref.worst(pred.cpu().numpy(), c["pred_rgb"], r["pred_bound"]),
             "gt": ref.worst(gt.cpu().numpy(), c["gt_rgb"], r["gt_bound"]),
             "grad_image0": ref.worst(image0.grad.cpu().numpy() * s, c["grad_image0"], r["grad_image_bound"]),
             "grad_weights_sum": ref.worst(w.grad.cpu().numpy() * s, c["grad_weights_sum"], r["grad_weights_sum_bound"])}
        print(f"rgb_train_loss vs reference {name} grad_out={grad_out}: |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in q.items()))
        assert max(q.values()) <= 1.0, q
        gp = 0.0 if prop.grad is None else float(prop.grad) * s
        gd = 0.0 if dist.grad is None else float(dist.grad) * s
        assert gp == float(c["grad_proposal_loss"]) and gd == float(c["grad_distort_loss"]), "the extras' gradients are their coefficients"


@pytest.mark.parametrize("name", EVAL)
def test_reference_eval_step_through_rgb_eval_loss(gpu, name):
    from sanerf_hq_amd.nerf import rgb_eval_loss
    c = case(name)
    H, W = int(c["H"]), int(c["W"])
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu)   # noqa: E731
    image = T(c["image0"]) + (1 - T(c["weights_sum"])).unsqueeze(-1) * 1      # the render over bg = 1
    # the same quantity stated from image0, so that the bounds count the render's background term as the CPU test does
    r = ref.rgb_loss(c["image0"], c["weights_sum"], c["images"], bg=1.0, image_has_bg=False, torch_chain=True)
    pred, gt, loss = rgb_eval_loss({"image": image.requires_grad_(True), "weights_sum": T(c["weights_sum"])}, {"images": T(c["images"]).reshape(H, W, -1), "H": H, "W": W})
    assert pred.shape == (H, W, 3) and gt.shape == (H, W, 3) and not loss.requires_grad
    q = {"loss": ref.worst(float(loss.detach()), c["loss"], r["total_bound"]), "pred": ref.worst(pred.reshape(-1, 3).cpu().numpy(), c["pred_rgb"].reshape(-1, 3), r["pred_bound"]),
         "gt": ref.worst(gt.reshape(-1, 3).cpu().numpy(), c["gt_rgb"].reshape(-1, 3), r["gt_bound"])}
    print(f"rgb_eval_loss vs reference {name}: |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q


def test_captured_once_and_replayed_on_new_contents(gpu):
    """rgb_loss with its backward as one graph on a single stream; after the image and background buffers are refilled a replay equals
    an eager call on the new contents, bit for bit."""
    from sanerf_hq_amd import raymarching as rm
    from sanerf_hq_amd.graph import GraphedStep
    N = 1000
    image, w, truth, bgN = synthetic(N, 4, 8)
    T = lambda a: torch.from_numpy(a).to(gpu)   # noqa: E731
    s_image, s_w, s_truth, s_bg = T(image).requires_grad_(True), T(w).requires_grad_(True), T(truth), T(bgN)
    extra = torch.tensor(0.03, device=gpu, requires_grad=True)

    def run(im, ws, bg, ex):
        im.grad = ws.grad = ex.grad = None
        loss, pred, gt = rm.rgb_loss(im, ws, s_truth, bg=bg, image_has_bg=False, lambda_entropy=1e-2, extras=[(ex, 0.5)])
        loss.backward()
        return loss, pred, gt, im.grad, ws.grad, ex.grad

    g = GraphedStep(lambda: run(s_image, s_w, s_bg, extra), warmup=1)
    for seed in (9, 10):
        image2, w2, _, bg2 = synthetic(N, 4, seed)
        with torch.no_grad():
            s_image.copy_(T(image2))
            s_w.copy_(T(w2))
            s_bg.copy_(T(bg2))
        got = [t.clone() for t in g()]
        want = run(T(image2).requires_grad_(True), T(w2).requires_grad_(True), T(bg2), torch.tensor(0.03, device=gpu, requires_grad=True))
        for a, b, k in zip(got, want, ("loss", "pred", "gt", "grad_image", "grad_weights_sum", "grad_extra")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (seed, k)
        assert float(got[5]) == 0.5


class PooledRand:
    """torch.rand served from ONE seeded stream in call order: the fused training route draws all its jitter in one call and the operator
    chain stage by stage, so only a shared stream gives both the same numbers (the same seed, the draws in the same order)."""

    def __init__(self, dev, seed, n):
        self.pool = REAL_RAND(n, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
        self.at = 0

    def __call__(self, *size, device=None, dtype=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        n = math.prod(size)
        assert self.at + n <= self.pool.numel()
        out = self.pool[self.at:self.at + n].clone().reshape(size)
        self.at += n
        return out


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_random_background_step_stays_on_the_fused_route_and_matches_the_tensor_background_chain(gpu, monkeypatch):
    """opt.background = 'random': rgb_train_step runs NeRFRenderer._run_autograd_unit (a spy counts it), and its loss and parameter
    gradients agree with model.render(bg_color=<the same [N,3] tensor>) -- which the fused route refuses -- plus the torch tail.
    Tolerances: those of tests/test_gpu_training.py::test_fused_training_route_equals_the_operator_chain (image 1e-5, loss 1e-6, gradients
    4e-4 relative), which compares the same two routes."""
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf import NeRFNetwork, NeRFRenderer, rgb_train_step
    opt = make_opt(background="random", lambda_proposal=1.0, lambda_distort=0.01, lambda_entropy=1e-3)
    N, H, W = 1024, 64, 64
    roF, rdF = rm.generate_rays(synth.orbit_pose(1.1, 25.0, 60.0), synth.pinhole_intrinsics(H, W), H, W, device=gpu)
    pix = torch.from_numpy((synth.hash_u01(N, 5) * (H * W)).astype(np.int64)).to(gpu)
    data = {"rays_o": roF[pix].contiguous(), "rays_d": rdF[pix].contiguous(), "index": [0],
            "images": torch.from_numpy(synth.hash_uniform((N, 4), 42, 0.0, 1.0)).to(gpu)}
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params([128, 64, 32], seed=1).items()}, strict=False)
    model = model.to(gpu).train()
    calls = []
    real_unit = NeRFRenderer._run_autograd_unit

    def spy(self, *a, **k):
        calls.append(a[2])                                 # bg_color
        return real_unit(self, *a, **k)

    monkeypatch.setattr(NeRFRenderer, "_run_autograd_unit", spy)
    n_rand = N * 3 + N * sum(t + 1 for t in opt.num_steps)

    monkeypatch.setattr(torch, "rand", PooledRand(gpu, 77, n_rand))
    pred, gt, loss = rgb_train_step(model, data, opt, global_step=10)
    loss.backward()
    assert len(calls) == 1 and calls[0] == 0 and not torch.is_tensor(calls[0]), "the step rendered over bg = 0 on the fused route"
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    model.zero_grad(set_to_none=True)
    monkeypatch.setattr(torch, "rand", PooledRand(gpu, 77, n_rand))
    bg = torch.rand(N, 3, device=gpu)                      # trainer.py:358, the first draw of the step
    o = model.render(data["rays_o"], data["rays_d"], staged=False, index=[0], bg_color=bg, perturb=True, update_proposal=True, return_feats=0)
    assert len(calls) == 1, "a tensor background does not take the fused route: this is the operator chain"
    im = data["images"]
    gt_t = im[:, :3] * im[:, 3:] + bg * (1 - im[:, 3:])
    loss_t = torch.nn.MSELoss(reduction="none")(o["image"], gt_t).mean() + opt.lambda_proposal * o["proposal_loss"] + opt.lambda_distort * o["distort_loss"]
    c = o["weights_sum"].clamp(1e-5, 1 - 1e-5)
    loss_t = loss_t + opt.lambda_entropy * (-c * torch.log2(c) - (1 - c) * torch.log2(1 - c)).mean()
    loss_t.backward()
    want = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}

    e_img, e_loss = float((pred - o["image"]).abs().max()), abs(float(loss) - float(loss_t))
    worst_grad = max((_rel(got[n], want[n]), n) for n in want)
    print(f"random background step: max|pred - chain| {e_img:.3e}, |loss - chain| {e_loss:.3e} (loss {float(loss_t):.6f}), worst gradient {worst_grad[1]} rel {worst_grad[0]:.3e}")
    assert torch.equal(gt, gt_t) or float((gt - gt_t).abs().max()) <= 4 * ref.U
    assert e_img < 1e-5
    assert e_loss < 1e-6 * max(1.0, abs(float(loss_t)))
    assert set(got) == set(want) and len(want) >= 7
    for n in want:
        assert _rel(got[n], want[n]) < 4e-4, (n, _rel(got[n], want[n]))


def test_white_background_step_equals_the_render_plus_torch_tail(gpu, monkeypatch):
    """opt.background = 'white': the step renders over 1 as before (fused route, the same seed: the same bits) and the HIP tail replaces
    F.mse_loss + the adds.  Both tails are within their bounds of the statement, so they differ by at most the sum of the two bounds."""
    from sanerf_hq_amd import raymarching as rm, synth
    from sanerf_hq_amd.nerf import NeRFNetwork, NeRFRenderer, rgb_train_step
    opt = make_opt(background="white", lambda_proposal=1.0, lambda_distort=0.0)
    N, H, W = 1024, 64, 64
    roF, rdF = rm.generate_rays(synth.orbit_pose(1.1, 25.0, 60.0), synth.pinhole_intrinsics(H, W), H, W, device=gpu)
    data = {"rays_o": roF[:N].contiguous(), "rays_d": rdF[:N].contiguous(), "images": torch.from_numpy(synth.hash_uniform((N, 3), 42, 0.0, 1.0)).to(gpu)}
    model = NeRFNetwork(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_params([128, 64, 32], seed=1).items()}, strict=False)
    model = model.to(gpu).train()
    calls = []
    real_unit = NeRFRenderer._run_autograd_unit
    monkeypatch.setattr(NeRFRenderer, "_run_autograd_unit", lambda self, *a, **k: (calls.append(a[2]), real_unit(self, *a, **k))[1])

    torch.manual_seed(31)
    pred, gt, loss = rgb_train_step(model, data, opt, global_step=10)
    loss.backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    torch.manual_seed(31)
    o = model.render(data["rays_o"], data["rays_d"], staged=False, bg_color=1, perturb=True, update_proposal=True)
    loss_t = torch.nn.functional.mse_loss(o["image"], data["images"]) + o["proposal_loss"]
    loss_t.backward()
    assert calls == [1, 1]
    assert torch.equal(pred, o["image"]) and torch.equal(gt, data["images"])
    ex = [(float(o["proposal_loss"]), 1.0)]
    args = (o["image"].detach().cpu().numpy(), o["weights_sum"].detach().cpu().numpy(), data["images"].cpu().numpy())
    bound = ref.rgb_loss(*args, bg=1.0, image_has_bg=True, extras=ex)["total_bound"] + ref.rgb_loss(*args, bg=1.0, image_has_bg=True, extras=ex, torch_chain=True)["total_bound"]
    print(f"white background step: |loss - chain| {abs(float(loss) - float(loss_t)):.3e} (bound {bound:.3e})")
    assert abs(float(loss) - float(loss_t)) <= bound
    for n, p in model.named_parameters():
        if p.grad is not None:      # the two tails' gradients differ by round-off alone; the bar is the routes' own (tests/test_gpu_training.py)
            assert _rel(got[n], p.grad) < 4e-4, (n, _rel(got[n], p.grad))
