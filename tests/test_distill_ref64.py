"""CPU: the fp64 statement of the feature-distillation loss (tests/distill_ref64.py) against torch's fp64 F.interpolate(mode="bilinear")
plus autograd, and against answers known without any oracle.

Against torch the bound is the fp32 taps' own error: src = (o + 0.5) s - 0.5 carries three fp32 roundings of a value below n_in, so a
weight is off by at most B = 3 n_in u (u = 2^-24, n_in = max(h, w)) and the prediction by B * range, range = max f - min f.  For the
gradient: the product wy wx is off by at most 2 B, and d by B * range, so
    |grad - autograd| <= (2 / n) (2 B sum_{o reaching the pixel} |d| + sum_o w B range)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_ref64 as ref

U = ref.U
SHAPES = [(64, 64, 64, 64, 8), (24, 24, 32, 32, 5), (64, 64, 32, 32, 3), (64, 64, 16, 16, 3), (8, 8, 64, 64, 4), (37, 21, 64, 64, 3),
          (64, 64, 48, 80, 3), (1, 1, 4, 4, 2), (11, 13, 5, 7, 3)]


def data(h, w, Ho, Wo, C, seed=0):
    g = torch.Generator().manual_seed(1000 * h + 10 * Wo + C + seed)
    return torch.randn(h * w, C, generator=g), torch.randn(C, Ho, Wo, generator=g)


def torch64(feat, h, w, target):
    f = feat.double().clone().requires_grad_(True)
    C, Ho, Wo = target.shape
    pred = F.interpolate(f.reshape(1, h, w, C).permute(0, 3, 1, 2).contiguous(), (Ho, Wo), mode="bilinear")
    loss = torch.nn.MSELoss(reduction="none")(pred, target.double()[None]).mean()
    loss.backward()
    return pred.detach()[0], float(loss.detach()), f.grad


@pytest.mark.parametrize("h,w,Ho,Wo,C", SHAPES)
def test_statement_vs_torch_fp64_interpolate_and_autograd(h, w, Ho, Wo, C):
    feat, target = data(h, w, Ho, Wo, C)
    r = ref.distill(feat, h, w, target)
    pred, loss, grad = torch64(feat, h, w, target)
    rng = float(feat.max() - feat.min())
    B = 3 * max(h, w) * U
    e_pred = float((r["pred"] - pred).abs().max())
    n = r["n"]
    d = r["d"]
    Iy, Ix = (ref.weight_matrix(h, Ho) != 0).double(), (ref.weight_matrix(w, Wo) != 0).double()
    reach_d = ref.adjoint(d.abs(), h, w, Iy, Ix)
    grad_bound = (2.0 / n) * (2 * B * reach_d + ref.adjoint(torch.full_like(d, B * rng), h, w)) + 1e-18
    e_grad = float(((r["grad"] - grad).abs() / grad_bound).max())
    loss_bound = float((2 * d.abs() * B * rng).mean() + (B * rng) ** 2) + 1e-15
    print(f"distill_ref64 {h}x{w}->{Ho}x{Wo} C={C}: |pred - torch fp64| {e_pred:.3e} (bound {B * rng:.3e}), |loss| {abs(r['loss'] - loss):.3e} "
          f"(bound {loss_bound:.3e}), grad err/bound {e_grad:.3e}")
    assert e_pred <= B * rng
    assert abs(r["loss"] - loss) <= loss_bound
    assert e_grad <= 1.0
    pow2 = lambda a, b: max(a, b) % min(a, b) == 0 and (max(a, b) // min(a, b)) & (max(a, b) // min(a, b) - 1) == 0
    if pow2(h, Ho) and pow2(w, Wo):            # a power-of-two ratio: every fp32 tap is exact, the two statements differ by fp64 round-off alone
        assert e_pred <= 1e-14 * max(rng, 1.0)


def test_constant_map_stays_constant():
    h, w, Ho, Wo, C = 7, 9, 13, 5, 3
    feat = torch.full((h * w, C), 1.75)
    pred = ref.resize(feat, h, w, Ho, Wo)
    assert float((pred - 1.75).abs().max()) <= 4 * U * 1.75                # l0 = fl(1 - l1): l0 + l1 = 1 to within u per axis
    r = ref.distill(feat, h, w, torch.full((C, Ho, Wo), 1.75))
    assert r["loss"] <= (4 * U * 1.75) ** 2


def test_identity_resize_is_exact():
    h, w, C = 6, 5, 4
    feat, target = data(h, w, h, w, C)
    r = ref.distill(feat, h, w, target, scale=3.0)
    f = feat.double().reshape(h, w, C).permute(2, 0, 1)
    assert torch.equal(r["pred"], f)
    d = f - target.double()
    assert r["loss"] == float((d * d).sum() / d.numel())
    assert torch.allclose(r["grad"], (3.0 * 2.0 / d.numel()) * d.permute(1, 2, 0).reshape(h * w, C), rtol=1e-15, atol=0)
    i0, i1, l0, l1 = ref.taps(h, h)
    assert np.array_equal(i0, np.arange(h)) and np.all(l1 == 0) and np.all(l0 == 1)


def test_two_times_upsampling_reproduces_a_ramp_in_the_interior():
    h, w = 6, 8
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    feat = torch.stack([3 * xx + 5 * yy, xx - 2 * yy], -1).reshape(h * w, 2)
    pred = ref.resize(feat, h, w, 2 * h, 2 * w)
    oy, ox = torch.meshgrid(torch.arange(2 * h, dtype=torch.float64), torch.arange(2 * w, dtype=torch.float64), indexing="ij")
    sy, sx = oy / 2 - 0.25, ox / 2 - 0.25                                  # the source position of an output: exact in fp32 at 2x
    want = torch.stack([3 * sx + 5 * sy, sx - 2 * sy])
    assert torch.equal(pred[:, 1:-1, 1:-1], want[:, 1:-1, 1:-1])          # (the border rows clamp: src = max(.., 0), i1 = i0 at the end)
    assert torch.equal(pred[:, 0, 1:-1], torch.stack([3 * sx[0, 1:-1], sx[0, 1:-1]]))


@pytest.mark.parametrize("h,w,Ho,Wo,C", [(24, 24, 32, 32, 3), (64, 64, 16, 16, 2), (8, 8, 64, 64, 2), (11, 13, 5, 7, 3)])
def test_adjoint_identity(h, w, Ho, Wo, C):
    """<grad, V> = (2 / n) <d, resize(V)> for any V: the gradient is the transpose of the forward's own weights."""
    feat, target = data(h, w, Ho, Wo, C)
    r = ref.distill(feat, h, w, target)
    V = torch.randn(h * w, C, generator=torch.Generator().manual_seed(5)).double()
    lhs = float((r["grad"] * V).sum())
    rhs = float((2.0 / r["n"]) * (r["d"] * ref.resize(V, h, w, Ho, Wo)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-30)
    if Ho * 4 == h:                                                      # 64 -> 16: three source rows in four get nothing
        untouched = (ref.weight_matrix(h, Ho) != 0).sum(0) == 0
        assert int(untouched.sum()) >= h // 2
        assert not r["grad"].reshape(h, w, C)[untouched].any()
