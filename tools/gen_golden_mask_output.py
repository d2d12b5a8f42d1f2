#!/usr/bin/env python3
"""Generate tests/golden/mask_output.npz by running the REFERENCE's own code on the CPU:

  * test_step's mask branch (nerf/trainer.py:730-777) and the (x * 255).astype(np.uint8) that follows it (:780-781): these lines sit inside
    a larger method, so they are read from the reference's source file at run time and executed as they are, on tensors made here; they
    call the reference's own overlay_mask_heatmap / overlay_mask_composition (nerf/utils.py);
  * eval_step's mask branch (trainer.py:600-627), executed the same way;
  * the reference's MeanIoUMeter / PSNRMeter / MSEMeter (nerf/metrics.py), imported and called.  The mIoU meter is given (argmax id, label):
    the reference hands it float probabilities, which its astype(int64) turns into zeros.
  * the trainer's 100 x 3 colour table (trainer.py:129-133), through the same matplotlib call (or matplotlib.colormaps[...].resampled(100)
    where plt.cm.get_cmap is gone).

    python tools/gen_golden_mask_output.py --reference <checkout of the reference>

Third-party modules the reference imports at module level and that are not installed are replaced by empty stubs (none is used on these
paths).  The fixture holds arrays only.

The outputs have two discontinuities: the argmax, and the truncation to 8 bits.  The generator draws three times the pixels it needs and
keeps the first ones that stay away from both, then runs the reference on the kept ones, asserts the margins and records them:
  margin_top2  >= 1e-3   between the two largest probabilities of a pixel (the project's existing margin);
  margin_rgb8  >= 1e-2   between every 255 * x that feeds an 8-bit value and the nearest integer -- about four times the 2.6e-3 which the
                         float tolerance of the GPU test (rtol 1e-5) allows after the scaling by 255.  One kind of value is exempt: an x
                         that is exactly 0.0 because a colour-table channel is exactly 0 (17 of the reference table's first 32 rows have
                         one, rows 0 and 1 among them, so no K = 2 heatmap avoids them): 0 * anything is 0 in every evaluation order, there
                         is nothing for a tolerance to move.  Their number is recorded as rgb8_exact_zeros.
"""
import argparse
import importlib
import os
import sys
import textwrap
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

EPS, ALPHA = 1e-6, 0.7
BG = (0.203, 0.551, 0.897)
MODES = ("heatmap", "composition", "mask")
#        name   K   C   H   W   strided image   absent class
CASES = (("k1", 1, 1, 33, 31, False, None),
         ("k2", 2, 2, 33, 31, False, None),
         ("k3", 3, 3, 33, 31, True, None),
         ("k8", 8, 8, 33, 31, False, 5),             # class 5 is in neither the predictions nor the labels
         ("k32", 32, 32, 23, 25, False, None))


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference(ref):
    sys.path.insert(0, ref)
    for _ in range(32):
        try:
            return importlib.import_module("nerf.trainer"), importlib.import_module("nerf.utils"), importlib.import_module("nerf.metrics")
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Stub(e.name)
            for k in [k for k in sys.modules if k.startswith("nerf")]:
                del sys.modules[k]
    raise RuntimeError("could not import the reference's nerf package")


def source_lines(ref, first, last, must_contain):
    src = open(os.path.join(ref, "nerf", "trainer.py")).read().splitlines()
    text = textwrap.dedent("\n".join(src[first - 1:last]))
    assert must_contain in text, f"trainer.py:{first}-{last} is not the expected block"
    return text


def color_table(ref):
    """trainer.py:129-133, the comprehension executed as the reference states it."""
    import matplotlib
    import matplotlib.pyplot as plt
    if not hasattr(plt.cm, "get_cmap"):
        plt.cm.get_cmap = lambda name, n: matplotlib.colormaps[name].resampled(n)
    me = types.SimpleNamespace(device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exec(source_lines(ref, 129, 133, "gist_ncar"), dict(np=np, plt=plt, torch=torch, self=me))
    assert me.color_map.shape == (100, 3) and me.color_map.dtype == torch.float32
    return me.color_map


def test_step_variant(ref, utils, color_map, logits, image, H, W, K, mode, render_id):
    """trainer.py:730-777 + 780-781 for one (mode, render id): pred_rgb, rgb8, the probabilities, max and argmax."""
    opt = types.SimpleNamespace(with_mask=True, n_inst=K, render_mask_type=mode, render_mask_instance_id=render_id)
    ns = dict(torch=torch, np=np, self=types.SimpleNamespace(opt=opt, color_map=color_map), H=H, W=W,
              outputs={"instance_mask_logits": torch.from_numpy(logits)}, pred_rgb=torch.from_numpy(image).reshape(H, W, 3).clone(),
              bg_color=torch.tensor(BG, dtype=torch.float32), overlay_mask_heatmap=utils.overlay_mask_heatmap,
              overlay_mask_composition=utils.overlay_mask_composition)
    exec(source_lines(ref, 730, 777, "overlay_mask_heatmap"), ns)
    exec(source_lines(ref, 780, 781, "astype(np.uint8)"), ns)
    probs = ns["inst_mask"] if K > 1 else torch.sigmoid(torch.from_numpy(logits).reshape(H, W, K))
    conf, ids = torch.max(probs, -1)
    return dict(rgb=ns["pred_rgb"].numpy().reshape(-1, 3).copy(), rgb8=ns["save_pred_rgb"].reshape(-1, 3).copy(),
                probs=probs.numpy().reshape(-1, K).copy(), conf=conf.numpy().reshape(-1).copy(), ids=ids.numpy().reshape(-1).astype(np.int64))


def variants(K):
    return [(m, r) for m in MODES for r in (-1, K - 1)]


def run_test_step(ref, utils, color_map, logits, image, H, W, K):
    out = {}
    for mode, rid in variants(K):
        v = test_step_variant(ref, utils, color_map, logits, image, H, W, K, mode, rid)
        tag = f"{mode}.{'all' if rid < 0 else 'one'}"
        out[tag + ".rgb"], out[tag + ".rgb8"] = v["rgb"], v["rgb8"]
        for k in ("probs", "conf", "ids"):
            assert k not in out or np.array_equal(out[k], v[k])
            out[k] = v[k]
    out["none.rgb8"] = (image * 255).astype(np.uint8)                 # trainer.py:726-727 on the plain render
    return out


def int_distance(x):
    v = 255.0 * x.astype(np.float64)
    d = np.abs(v - np.rint(v))
    return np.where(x == 0.0, np.inf, d)                              # the exempt kind: exact zeros (module docstring)


def pixel_margins(out, image, K):
    top2 = np.full(len(image), np.inf)
    if K > 1:
        ps = np.sort(out["probs"], axis=-1)
        top2 = (ps[:, -1] - ps[:, -2]).astype(np.float64)
    d8 = int_distance(image).min(-1)
    for mode, rid in variants(K):
        d8 = np.minimum(d8, int_distance(out[f"{mode}.{'all' if rid < 0 else 'one'}.rgb"]).min(-1))
    return top2, d8


def eval_image(ref, metrics, logits, labels, H, W, K):
    """trainer.py:600-627 for one view + MeanIoUMeter.update on (argmax id, label)."""
    opt = types.SimpleNamespace(n_inst=K, epsilon=EPS, label_regularization_weight=0)
    ns = dict(torch=torch, self=types.SimpleNamespace(opt=opt, device="cpu"), H=H, W=W,
              data={"masks": torch.from_numpy(labels).reshape(1, H, W), "use_default_intrinsics": False},
              outputs={"instance_mask_logits": torch.from_numpy(logits)})
    exec(source_lines(ref, 600, 627, "torch.gather"), ns)
    ids = ns["pred_mask"].argmax(-1).reshape(-1)
    meter = metrics.MeanIoUMeter()
    miou = meter.update(ids, torch.from_numpy(labels))
    C = max(int(ids.max()), int(labels.max())) + 1
    idn = ids.numpy()
    counts = np.zeros((3, 32), dtype=np.int64)
    for i in range(32):
        counts[0, i] = np.logical_and(idn == i, labels == i).sum()
        counts[1, i] = (idn == i).sum()
        counts[2, i] = (labels == i).sum()
    assert counts[:, C:].sum() == 0
    return float(ns["loss"].item()), float(miou), counts


def make_inputs(rng, n, K, absent):
    logits = (rng.standard_normal((n, K)) * 2.0).astype(np.float32)
    if absent is not None:
        logits[:, absent] -= 6.0
    image = rng.uniform(0.02, 0.98, (n, 3)).astype(np.float32)
    return logits, image


def make_labels(rng, ids, C, absent):
    classes = np.array([c for c in range(C) if c != absent])
    lab = np.where(rng.uniform(size=len(ids)) < 0.6, ids, rng.choice(classes, len(ids)))
    lab = np.where(rng.uniform(size=len(ids)) < 0.1, -1, lab).astype(np.int64)
    return lab


def rgb_pair(rng, n, metrics):
    truth = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    pred = np.clip(truth + rng.normal(0.0, 0.05, (n, 3)), 0.0, 1.0).astype(np.float32)
    m, p = metrics.MSEMeter(), metrics.PSNRMeter()
    m.update(torch.from_numpy(pred), torch.from_numpy(truth))
    psnr = p.update(torch.from_numpy(pred), torch.from_numpy(truth))
    return pred, truth, float(m.measure()), float(psnr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(GOLD, "mask_output.npz"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    ref = args.reference
    trainer, utils, metrics = import_reference(ref)
    cm = color_table(ref)
    arrays = dict(color_map=cm.numpy().copy(), epsilon=np.float32(EPS), alpha=np.float32(ALPHA), bg=np.array(BG, dtype=np.float32),
                  cases=np.array([c[0] for c in CASES]), strided_cases=np.array([c[0] for c in CASES if c[5]]))
    kept = {}
    for n, (name, K, C, H, W, _, absent) in enumerate(CASES):
        rng = np.random.default_rng(100 + n)
        N = H * W
        logits, image = make_inputs(rng, 3 * N, K, absent)
        surplus = run_test_step(ref, utils, cm, logits, image, 3 * H, W, K)
        top2, d8 = pixel_margins(surplus, image, K)
        ok = np.flatnonzero((top2 >= 1e-3) & (d8 >= 1e-2) & (surplus["ids"] != (-1 if absent is None else absent)))
        assert len(ok) >= N, (name, len(ok), N)
        logits, image = np.ascontiguousarray(logits[ok[:N]]), np.ascontiguousarray(image[ok[:N]])
        out = run_test_step(ref, utils, cm, logits, image, H, W, K)
        top2, d8 = pixel_margins(out, image, K)
        m_top2, m_rgb8 = float(top2.min()), float(d8.min())
        assert m_top2 >= 1e-3 and m_rgb8 >= 1e-2, (name, m_top2, m_rgb8)
        zeros = sum(int((out[f"{m}.{'all' if r < 0 else 'one'}.rgb"] == 0.0).sum()) for m, r in variants(K))
        labels = make_labels(rng, out["ids"], C, absent)
        if C > K:
            assert labels.max() == C - 1
        loss, miou, counts = eval_image(ref, metrics, logits, labels, H, W, K)
        if absent is not None:
            assert counts[1, absent] == 0 and counts[2, absent] == 0
        out.update(logits=logits, image=image, labels=labels, shape=np.array([H, W, K, C], dtype=np.int64), render_one=np.int64(K - 1),
                   margin_top2=np.float64(m_top2), margin_rgb8=np.float64(m_rgb8), rgb8_exact_zeros=np.int64(zeros),
                   eval_loss=np.float64(loss), eval_miou=np.float64(miou), eval_counts=counts)
        kept[name] = (logits, labels, H, W, K)
        print(f"{name}: K={K} C={C} N={N}, margins top2 {m_top2:.2e} rgb8 {m_rgb8:.2e} ({zeros} exact zeros), loss {loss:.6f}, mIoU {miou:.6f}")
        arrays.update({f"{name}.{k}": v for k, v in out.items()})

    # one image with no labelled pixel (the logits of k3)
    logits, _, H, W, K = kept["k3"]
    none = np.full(H * W, -1, dtype=np.int64)
    loss, miou, counts = eval_image(ref, metrics, logits, none, H, W, K)
    assert loss == 0.0
    arrays.update({"k3_unlabelled.labels": none, "k3_unlabelled.eval_loss": np.float64(loss), "k3_unlabelled.eval_miou": np.float64(miou),
                   "k3_unlabelled.eval_counts": counts})

    # three images through the reference's meters: mIoU, mean loss (trainer.py:1603-1604, 1698), PSNR, MSE
    rng = np.random.default_rng(999)
    logits_b = (rng.standard_normal((H * W, K)) * 2.0).astype(np.float32)
    pb = torch.softmax(torch.from_numpy(logits_b), -1).numpy()
    sb = np.sort(pb, -1)
    logits_b[(sb[:, -1] - sb[:, -2]) < 1e-3, 0] += 1.0
    labels_b = make_labels(rng, pb.argmax(-1), K, None)
    views = [(logits, kept["k3"][1]), (logits, none), (logits_b, labels_b)]
    miou_meter, psnr_meter, mse_meter, total = metrics.MeanIoUMeter(), metrics.PSNRMeter(), metrics.MSEMeter(), 0.0
    for i, (lg, lb) in enumerate(views):
        loss, _, _ = eval_image(ref, metrics, lg, lb, H, W, K)
        total += loss
        miou_meter.update(torch.softmax(torch.from_numpy(lg), -1).argmax(-1), torch.from_numpy(lb))
        pred, truth, mse, psnr = rgb_pair(rng, H * W, metrics)
        psnr_meter.update(torch.from_numpy(pred), torch.from_numpy(truth))
        mse_meter.update(torch.from_numpy(pred), torch.from_numpy(truth))
        arrays.update({f"meters3.{i}.logits": lg, f"meters3.{i}.labels": lb, f"meters3.{i}.pred": pred, f"meters3.{i}.truth": truth,
                       f"meters3.{i}.mse": np.float64(mse), f"meters3.{i}.psnr": np.float64(psnr)})
    arrays["meters3.measure"] = np.array([miou_meter.measure(), total / len(views), psnr_meter.measure(), mse_meter.measure()], dtype=np.float64)
    print("meters3: mIoU %.6f loss %.6f PSNR %.4f MSE %.6f" % tuple(arrays["meters3.measure"]))
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
