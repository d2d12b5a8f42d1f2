"""CPU: the fp64 statement of the RGB step's loss tail (tests/rgb_loss_ref64.py) against what the reference's own train_step / eval_step
computed (tests/golden/rgb_step.npz, made by tools/gen_golden_rgb_step.py), and a numpy-float32 transliteration of the kernel's chain
against the statement's bounds.

The fixture is torch's fp32 chain on the CPU.  Its count of roundings differs from the kernel's in the two fp32 sums (n + 12 roundings
for the loss instead of 13) and in the entropy gradient (17 per ray instead of 8), so it is compared within the bounds re-derived for
that chain (rgb_loss_ref64.rgb_loss(torch_chain=True); the derivation is in that module's docstring).  With a scalar background the
reference renders over it; the statement is given image0 and bg = 1 with image_has_bg=False, which is the same quantity with the same
count ((1 - w) * 1 is exact)."""
import os

import numpy as np
import pytest

import rgb_loss_ref64 as ref
from helpers import ROOT

# The transliterated chain must stay below this fraction of every bound: a bound is twice a first-order worst case, which a two-rounding
# quantity such as pred can attain (both roundings at half an ulp), so the fraction is one half plus the second-order terms (of order u).
FRACTION = 0.5 + 1e-6
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rgb_step.npz"))
TRAIN = [str(c) for c in GOLD["train_cases"]]
EVAL = [str(c) for c in GOLD["eval_cases"]]


def case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + ".")}


def extras_of(c):
    """The extras the reference's conditions let into the loss (trainer.py:382-387)."""
    ex = []
    if bool(c["update_proposal"]) and float(c["lambda_proposal"]) > 0:
        ex.append((float(c["proposal_loss"]), float(c["lambda_proposal"])))
    if float(c["lambda_distort"]) > 0:
        ex.append((float(c["distort_loss"]), float(c["lambda_distort"])))
    return ex


worst = ref.worst


def ratios(r, got):
    return {"pred": worst(got["pred"], r["pred"], r["pred_bound"]), "gt": worst(got["gt"], r["gt"], r["gt_bound"]),
            "mse": worst(got["mse"], r["mse"], r["mse_bound"]), "entropy": worst(got["entropy"], r["entropy"], r["entropy_bound"]),
            "total": worst(got["total"], r["total"], r["total_bound"]),
            "grad_image": worst(got["grad_image"], r["grad_image"], r["grad_image_bound"]),
            "grad_weights_sum": worst(got["grad_weights_sum"], r["grad_weights_sum"], r["grad_weights_sum_bound"])}


def test_the_fixture_covers_the_cases_and_keeps_away_from_the_clamp_bounds():
    assert len(TRAIN) == 8 and len(EVAL) == 2
    seen = set()
    for name in TRAIN:
        c = case(name)
        seen.add((c["images"].shape[1], np.ndim(c["bg"]) == 2, float(c["lambda_entropy"]) > 0))
        w = c["weights_sum"]
        assert float(c["margin"]) > 1e-7
        assert np.abs(w.astype(np.float64) - float(ref.LO)).min() > 1e-7 and np.abs(w.astype(np.float64) - float(ref.HI)).min() > 1e-7
        assert (w == 0).any() and (w == 1).any() and (w > 1).any() and ((w > 0) & (w < ref.LO)).any() and ((w > ref.HI) & (w < 1)).any()
        assert ((w >= ref.LO) & (w <= ref.HI)).sum() > w.size // 2
    assert len(seen) == 8, "RGBA / RGB x random / white x entropy off / on"
    assert float(GOLD["clamp_lo"]) == float(ref.LO) and float(GOLD["clamp_hi"]) == float(ref.HI)


@pytest.mark.parametrize("name", TRAIN)
def test_statement_reproduces_the_reference_train_step(name):
    c = case(name)
    r = ref.rgb_loss(c["image0"], c["weights_sum"], c["images"], bg=c["bg"], image_has_bg=False, lambda_entropy=float(c["lambda_entropy"]),
                     extras=extras_of(c), torch_chain=True)
    q = {"loss": worst(c["loss"], r["total"], r["total_bound"]), "pred": worst(c["pred_rgb"], r["pred"], r["pred_bound"]),
         "gt": worst(c["gt_rgb"], r["gt"], r["gt_bound"]), "grad_image0": worst(c["grad_image0"], r["grad_image"], r["grad_image_bound"]),
         "grad_weights_sum": worst(c["grad_weights_sum"], r["grad_weights_sum"], r["grad_weights_sum_bound"])}
    print(f"rgb_loss_ref64 vs reference {name}: |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q
    # the gradients of the extras are their coefficients, where the reference's conditions let them in
    ex = extras_of(c)
    want_p = float(c["lambda_proposal"]) if bool(c["update_proposal"]) and float(c["lambda_proposal"]) > 0 else 0.0
    assert float(c["grad_proposal_loss"]) == np.float32(want_p) and float(c["grad_distort_loss"]) == np.float32(max(float(c["lambda_distort"]), 0.0))
    assert len(ex) == (want_p > 0) + (float(c["lambda_distort"]) > 0)


@pytest.mark.parametrize("name", EVAL)
def test_statement_reproduces_the_reference_eval_step(name):
    c = case(name)
    image = (c["image0"] + (np.float32(1) - c["weights_sum"])[:, None] * np.float32(1)).astype(np.float32)      # the render over bg = 1
    r = ref.rgb_loss(image, c["weights_sum"], c["images"], bg=1.0, image_has_bg=True, torch_chain=True)
    H, W = int(c["H"]), int(c["W"])
    assert c["pred_rgb"].shape == (H, W, 3) and c["gt_rgb"].shape == (H, W, 3)
    q = {"loss": worst(c["loss"], r["total"], r["total_bound"]), "pred": worst(c["pred_rgb"].reshape(-1, 3), r["pred"], r["pred_bound"]),
         "gt": worst(c["gt_rgb"].reshape(-1, 3), r["gt"], r["gt_bound"])}
    print(f"rgb_loss_ref64 vs reference {name}: |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q


def synthetic(N, channels, seed):
    rng = np.random.default_rng(seed)
    image = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    w = rng.uniform(0, 1, N).astype(np.float32)
    w[rng.integers(0, N, max(N // 8, 1))] = rng.choice(np.array([0.0, 1.0, 3e-6, 1.0 - 3e-6, 1.0 + 1e-6], np.float32), max(N // 8, 1))
    truth = rng.uniform(0, 1, (N, channels)).astype(np.float32)
    return image, w, truth, rng.uniform(0, 1, (N, 3)).astype(np.float32)


MODES = [(ch, bgm, has_bg, lam, ex) for ch in (3, 4) for bgm in ("value", "colour", "per_ray") for has_bg in (True, False)
         for lam in (0.0, 1e-2) for ex in ((), ((0.03, 1.0), (0.004, 0.002)))]


def test_float32_transliteration_of_the_kernel_stays_below_half_of_every_bound():
    top = {}
    for name in TRAIN:
        c = case(name)
        kw = dict(bg=c["bg"], image_has_bg=False, lambda_entropy=float(c["lambda_entropy"]), extras=extras_of(c))
        q = ratios(ref.rgb_loss(c["image0"], c["weights_sum"], c["images"], **kw), ref.kernel_chain_f32(c["image0"], c["weights_sum"], c["images"], **kw))
        print(f"kernel chain in float32, fixture {name}: |err|/bound " + ", ".join(f"{k} {v:.3f}" for k, v in q.items()))
        for k, v in q.items():
            top[k] = max(top.get(k, 0.0), v)
    for i, (ch, bgm, has_bg, lam, ex) in enumerate(MODES):
        for N in (1, 63, 257, 1000):
            image, w, truth, bgN = synthetic(N, ch, 100 * i + N)
            bg = {"value": 0.75, "colour": bgN[0], "per_ray": bgN}[bgm]
            kw = dict(bg=bg, image_has_bg=has_bg, lambda_entropy=lam, extras=ex)
            q = ratios(ref.rgb_loss(image, w, truth, **kw), ref.kernel_chain_f32(image, w, truth, **kw))
            if N == 1000:
                print(f"kernel chain in float32, N={N} ch={ch} bg={bgm} has_bg={has_bg} lam={lam} extras={len(ex)}: |err|/bound "
                      + ", ".join(f"{k} {v:.3f}" for k, v in q.items()))
            for k, v in q.items():
                top[k] = max(top.get(k, 0.0), v)
    print("kernel chain in float32, worst |err|/bound over all cases: " + ", ".join(f"{k} {v:.3f}" for k, v in top.items()))
    assert max(top.values()) <= FRACTION, top


def test_answers_known_without_an_oracle():
    N = 37
    image, w, truth, bgN = synthetic(N, 4, 5)
    # an opaque truth equal to the image: nothing to learn, whatever the background
    t = np.concatenate([image, np.ones((N, 1), np.float32)], 1)
    r = ref.rgb_loss(image, w, t, bg=bgN, image_has_bg=True)
    assert r["mse"] == 0 and r["total"] == 0 and not r["grad_image"].any() and not r["grad_weights_sum"].any()
    # a transparent truth is the background
    t0 = np.concatenate([image, np.zeros((N, 1), np.float32)], 1)
    assert np.array_equal(ref.rgb_loss(image, w, t0, bg=bgN)["gt"], bgN.astype(np.float64))
    # the background term is linear: rendering over bg and adding it in the tail are the same quantity
    over = (image.astype(np.float64) + (1 - w.astype(np.float64))[:, None] * bgN)
    a = ref.rgb_loss(image, w, truth, bg=bgN, image_has_bg=False, lambda_entropy=1e-2)
    assert np.array_equal(a["pred"], over)
    # the entropy of 1/2 is one bit, its gradient 0; clamped rays get no entropy gradient
    h = ref.rgb_loss(image, np.full(N, 0.5, np.float32), truth[:, :3], lambda_entropy=1.0)
    assert h["entropy"] == 1.0 and not h["grad_weights_sum"].any()
    z = ref.rgb_loss(image, np.array([0, 1, 2e-6, 1 + 1e-6] * 9 + [0], np.float32), truth[:, :3], lambda_entropy=1.0)
    assert not z["inside"].any() and not z["grad_weights_sum"].any() and not z["grad_weights_sum_bound"].any()
    # the total's derivative with respect to weights_sum, by central differences in fp64 on rays well inside the clamp range
    w_in = np.clip(w, 0.1, 0.9).astype(np.float32)
    base = ref.rgb_loss(image, w_in, truth, bg=bgN, image_has_bg=False, lambda_entropy=0.3)
    for i in (0, 5, 36):
        hstep = np.float32(2.0 ** -10)
        up, dn = w_in.copy(), w_in.copy()
        up[i] += hstep
        dn[i] -= hstep
        fd = (ref.rgb_loss(image, up, truth, bg=bgN, image_has_bg=False, lambda_entropy=0.3)["total"]
              - ref.rgb_loss(image, dn, truth, bg=bgN, image_has_bg=False, lambda_entropy=0.3)["total"]) / (float(up[i]) - float(dn[i]))
        # (the step's own error: h^2 / 6 times the entropy's third derivative, below 150 / ln 2 at w >= 0.1 -- 4e-5 of lambda / N)
        assert abs(fd - base["grad_weights_sum"][i]) <= 1e-4 * 0.3 / N, (i, fd, base["grad_weights_sum"][i])
