"""An fp64 statement of the SAM-feature distillation loss (sn_rm_feature_distill_loss, include/sanerf_hip.h) for the tests alone, and the
fp32 round-off bounds that go with it.  Plain numpy / torch on the CPU; nothing here imports the package.

The taps of output index o on an axis of n_in samples resized to n_out are kept in fp32, because every implementation has them in fp32
and they decide which samples an output touches:

    s = float(n_in) / float(n_out);  src = max((o + 0.5f) * s - 0.5f, 0);  i0 = min(int(src), n_in - 1);  i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0;  l0 = 1 - l1

Everything after that is float64:

    pred[c,oy,ox] = l0y (l0x f[y0,x0,c] + l1x f[y0,x1,c]) + l1y (l0x f[y1,x0,c] + l1x f[y1,x1,c])
    d = pred - target;  loss = sum d^2 / n, n = C Ho Wo;  grad[y w + x, c] = scale (2 / n) sum_o w(o -> pixel) d[c, o]

written as the two weight matrices Wy [Ho,h], Wx [Wo,w] (row o carries l0 at i0 and l1 at i1, added where both land on the last sample).

Bounds (u = 2^-24, first-order count of the kernel's fp32 roundings, factor 2 of margin as in tests/grid_ref64.py), all from the fp64 side:
  pred    2 * 4 u sum|w f|                 a term meets four roundings: lx * f, the add, ly * (..), the add
  d       pred's bound + 2 u |d|           the one subtraction
  loss    mean(2 |d| e_d + e_d^2) + 2 u loss      e_d = d's bound; the double sum is exact at this scale, the result is stored as a float
  grad    2 (|coef| (sum |w| e_d' + K u sum |w d|) + 5 u |grad|)
          e_d' = e_d / 2 (its margin is not doubled twice); K = ny + nx + 4: the wx * d products, the <= nx adds of a row, wy * row, the
          <= ny adds, and the l0 + l1 add on the last sample of either axis (nx, ny: the longest range of outputs that reaches one source
          sample); 5 u: scale * scale_dev, float(n), 2 / n, their product, and the product with the sum
"""
import numpy as np
import torch

U = 2.0 ** -24


def taps(n_in: int, n_out: int):
    """(i0, i1 int64 [n_out]; l0, l1 float32 [n_out]) by the contract's fp32 chain."""
    o = np.arange(n_out, dtype=np.float32)
    assert n_out < 2 ** 24
    s = np.float32(n_in) / np.float32(n_out)
    src = np.maximum((o + np.float32(0.5)) * s - np.float32(0.5), np.float32(0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def weight_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out, n_in] float64: what output o takes from sample i."""
    i0, i1, l0, l1 = taps(n_in, n_out)
    W = np.zeros((n_out, n_in), dtype=np.float64)
    rows = np.arange(n_out)
    np.add.at(W, (rows, i0), l0.astype(np.float64))
    np.add.at(W, (rows, i1), l1.astype(np.float64))
    return torch.from_numpy(W)


def reach(n_in: int, n_out: int) -> int:
    """The longest range of outputs whose taps reach one source sample: #{o : i - 1 <= i0(o) <= i}, maximised over i."""
    i0 = taps(n_in, n_out)[0]
    return max(int(((i0 >= i - 1) & (i0 <= i)).sum()) for i in range(n_in))


def _f(feat, h, w):
    f = torch.as_tensor(feat).detach().cpu().to(torch.float64)
    return f.reshape(h, w, -1)


def resize(feat, h: int, w: int, Ho: int, Wo: int, Wy=None, Wx=None) -> torch.Tensor:
    """feat [h*w, C] (or [h,w,C]) -> [C, Ho, Wo] float64."""
    f = _f(feat, h, w)
    C = f.shape[-1]
    Wy = weight_matrix(h, Ho) if Wy is None else Wy
    Wx = weight_matrix(w, Wo) if Wx is None else Wx
    t = (Wy @ f.reshape(h, w * C)).reshape(Ho, w, C)                       # [Ho, w, C]
    t = torch.matmul(Wx, t)                                               # [Ho, Wo, C]
    return t.permute(2, 0, 1).contiguous()


def adjoint(g, h: int, w: int, Wy=None, Wx=None) -> torch.Tensor:
    """g [C, Ho, Wo] -> [h*w, C] float64: sum_o w(o -> pixel) g[c, o]."""
    g = torch.as_tensor(g).to(torch.float64)
    C, Ho, Wo = g.shape
    Wy = weight_matrix(h, Ho) if Wy is None else Wy
    Wx = weight_matrix(w, Wo) if Wx is None else Wx
    t = g.permute(1, 2, 0)                                                # [Ho, Wo, C]
    t = torch.matmul(Wx.t(), t)                                           # [Ho, w, C]
    t = (Wy.t() @ t.reshape(Ho, w * C)).reshape(h * w, C)
    return t.contiguous()


def distill(feat, h: int, w: int, target, scale: float = 1.0) -> dict:
    """The statement and its bounds.  target [C,Ho,Wo] (or [1,C,Ho,Wo]).  Returns float64 tensors: pred, d [C,Ho,Wo], loss (float),
    grad [h*w, C], and the bounds pred_bound, loss_bound, grad_bound of the docstring."""
    tgt = torch.as_tensor(target).detach().cpu().to(torch.float64)
    if tgt.dim() == 4:
        tgt = tgt[0]
    C, Ho, Wo = tgt.shape
    f = _f(feat, h, w)
    assert f.shape[-1] == C
    Wy, Wx = weight_matrix(h, Ho), weight_matrix(w, Wo)
    n = C * Ho * Wo
    pred = resize(f, h, w, Ho, Wo, Wy, Wx)
    d = pred - tgt
    loss = float((d * d).sum() / n)
    coef = float(scale) * 2.0 / n
    grad = coef * adjoint(d, h, w, Wy, Wx)
    mass_pred = resize(f.abs(), h, w, Ho, Wo, Wy, Wx)
    e_pred = 4 * U * mass_pred                                            # first order, no margin yet
    e_d = e_pred + U * d.abs()
    pred_bound = 2 * e_pred
    loss_bound = float((2 * d.abs() * (2 * e_d) + (2 * e_d) ** 2).mean()) + 2 * U * loss
    K = reach(h, Ho) + reach(w, Wo) + 4
    grad_bound = 2 * (abs(coef) * (adjoint(e_d, h, w, Wy, Wx) + K * U * adjoint(d.abs(), h, w, Wy, Wx)) + 5 * U * grad.abs())
    return {"pred": pred, "d": d, "loss": loss, "grad": grad, "pred_bound": pred_bound, "loss_bound": loss_bound, "grad_bound": grad_bound,
            "mass_pred": mass_pred, "n": n, "K": K}
