"""An fp64 statement of the fp32 matrix-core operators for the tests, and the fp32 round-off bounds that go with it: the small bias-free
ReLU perceptrons (csrc/mlp_small.hip: sn_mlp_small_forward_train / sn_mlp_small_backward, with trunc_exp and sigmoid + background folded in),
the weight gradient of a linear layer (sn_linear_wgrad) and the general product (sn_gemm_f32).

Written for the tests alone: plain torch in float64 that runs on any device and imports nothing from the package or from oracle/.

u = 2^-24.  Every bound is a first-order count of the fp32 roundings times the factor 2 of margin that grid_ref64.py uses, per ELEMENT:

  chain, forward    h_0 = x, a_l = W_l h_{l-1}, h_l = relu(a_l), raw = a_L.
                    E_l = |W_l| E_{l-1} + 2 (K_l + 1) u |W_l| (|h_{l-1}| + E_{l-1}),  E_0 = 0
                    K_l + 1: the roundings of a K_l-term fp32 sum in any order (every partial sum is bounded by the absolute mass).  The first
                    term carries the error the inputs already have.  ReLU is 1-Lipschitz: E_l holds for h_l as it does for a_l, no exclusions.
  chain, backward   with the hidden outputs GIVEN (the C ABI's contract: sn_mlp_small_backward takes `hidden` and gates on hidden > 0):
                    g_{l-1} = [hidden_{l-1} > 0] (W_l^T g_l), the same recurrence through |W_l|^T with K = the layer's output width; a gated-out
                    element is exactly 0 and its bound is 0.  Nothing a forward kernel produced enters, and no ReLU flip is ambiguous.
  trunc_exp         forward exp(raw[:, 0]); backward g exp(clamp(raw, -15, 15)) added to channel 0 of the raw output's gradient
                    (activation.py:5-17).  The device exp is taken at EXP_REL = 2.5e-7 relative, the bar the suite already asserts of it
                    (test_device_exp_matches_the_oracle_bit_for_bit).
                      forward   exp(raw) (expm1(E_raw) + EXP_REL exp(E_raw))          the kernel exponentiates ITS raw output, off by <= E_raw
                      backward  EXP_REL |g| e + 2 * 1 u (|g| e + |g_raw|)              one fma folds the term into the raw output's gradient
  sigmoid + bg      forward sigmoid(raw) + (1 - ws) bg; backward g s (1 - s) into the raw output's gradient and -bg sum_c g to ws
                    (renderer.py:349-353).  s = 1 / (1 + exp(-x)): the exp, ONE addition, ONE division -- an absolute error of
                      ds = s (EXP_REL (1 - s) + 2 * 2 u)                               (d/de of 1 / (1 + e) times e is s (1 - s))
                      forward   E_raw / 4 + ds + 2 u (2 |t| + |s + t|)                 t = (1 - ws) bg: TWO roundings; the final sum: ONE; sigmoid' <= 1/4
                      backward  d = s (1 - s):  dd = ds + 2 * 2 u d                    |1 - 2 s| <= 1 on ds; 1 - s: ONE rounding, the product: ONE
                                |g| dd + 2 * 1 u (|g| d + |g_raw|)                     one fma, as above
                      to ws     2 (C + 1) u |bg| sum_c |g|                             C additions and the product with bg
  wgrad             dw = dy^T x,  2 (M + 1) u sum_m |dy| |x|
  gemm              act(A B + bias),  2 (K + 2) u (sum |a| |b| + |bias|); leaky ReLU multiplies by the fp32 literal 0.01f: one more rounding.
"""
import torch

from grid_ref64 import worst_ratio  # noqa: F401  (the one ratio helper of the suite; re-exported for the tests of this family)

U = 2.0 ** -24
EXP_REL = 2.5e-7
ACT_NONE, ACT_TRUNC_EXP0, ACT_SIGMOID_BG = 0, 1, 2
LEAKY = float(torch.tensor(0.01, dtype=torch.float32))


def _layer(h, E, W, K):
    """One matrix of a chain applied to rows: (h W^T, its bound).  W [out, in] float64, K = terms per sum."""
    Wa = W.abs()
    return h @ W.t(), E @ Wa.t() + 2.0 * (K + 1) * U * ((h.abs() + E) @ Wa.t())


def chain_forward(x, weights):
    """x [M, d0], weights: list of nn.Linear.weight [d_l, d_{l-1}] -> dict of float64: hidden / hidden_bound (lists, one per hidden layer, post-ReLU),
    raw / raw_bound [M, dL]."""
    h = x.double()
    E = torch.zeros_like(h)
    hs, Es = [], []
    for l, W in enumerate(weights):
        a, E = _layer(h, E, W.double(), W.shape[1])
        if l + 1 < len(weights):
            h = torch.relu(a)
            hs.append(h)
            Es.append(E)
    return dict(hidden=hs, hidden_bound=Es, raw=a, raw_bound=E)


def chain_backward(g_last, weights, hidden, g_last_bound=None):
    """g_last [M, dL] = gradient of the last pre-activation, hidden: the hidden outputs AS GIVEN to the kernel (the gate is hidden > 0) ->
    dict of float64: grad_hidden / grad_hidden_bound (lists indexed by forward layer: gradient of that layer's pre-activation), grad_in / grad_in_bound."""
    g = g_last.double()
    E = torch.zeros_like(g) if g_last_bound is None else g_last_bound.double()
    L = len(weights)
    gh, gE = [None] * (L - 1), [None] * (L - 1)
    for l in range(L - 1, 0, -1):
        W = weights[l].double()
        t, Et = _layer(g, E, W.t(), W.shape[0])
        gate = (hidden[l - 1] > 0).double()
        g, E = t * gate, Et * gate
        gh[l - 1], gE[l - 1] = g, E
    W = weights[0].double()
    gi, Ei = _layer(g, E, W.t(), W.shape[0])
    return dict(grad_hidden=gh, grad_hidden_bound=gE, grad_in=gi, grad_in_bound=Ei)


def sigmoid_abs_error(s):
    return s * (EXP_REL * (1.0 - s) + 2.0 * 2 * U)


def act_forward(act, raw, raw_bound, aux_in=None, bg=0.0):
    """(activated output, bound) of what the kernel computes from its own raw output, which is within raw_bound of raw."""
    raw = raw.double()
    if act == ACT_TRUNC_EXP0:
        y, E = torch.exp(raw[:, 0]), raw_bound[:, 0]
        return y, y * (torch.expm1(E) + EXP_REL * torch.exp(E))
    assert act == ACT_SIGMOID_BG
    s = torch.sigmoid(raw)
    t = ((1.0 - aux_in.double()) * float(bg))[:, None]
    return s + t, raw_bound / 4.0 + sigmoid_abs_error(s) + 2.0 * U * (2.0 * t.abs() + (s + t).abs())


def act_backward(act, raw, g_raw, g_aux, bg=0.0):
    """Gradient of the last pre-activation from the gradient of the raw output (g_raw, may be None) and of the activated output (g_aux, may be
    None), raw = the forward's raw output as given -> dict: grad_last, grad_last_bound [M, dL]; with the sigmoid also grad_aux_in and its bound [M]."""
    raw = raw.double()
    g0 = torch.zeros_like(raw) if g_raw is None else g_raw.double()
    if g_aux is None:
        return dict(grad_last=g0, grad_last_bound=torch.zeros_like(g0))
    ga = g_aux.double()
    out, bound = g0.clone(), torch.zeros_like(g0)
    if act == ACT_TRUNC_EXP0:
        ga = ga.reshape(-1)
        e = torch.exp(torch.clamp(raw[:, 0], -15.0, 15.0))
        out[:, 0] += ga * e
        bound[:, 0] = EXP_REL * ga.abs() * e + 2.0 * U * (ga.abs() * e + g0[:, 0].abs())
        return dict(grad_last=out, grad_last_bound=bound)
    assert act == ACT_SIGMOID_BG
    s = torch.sigmoid(raw)
    d = s * (1.0 - s)
    dd = sigmoid_abs_error(s) + 2.0 * 2 * U * d
    out = g0 + ga * d
    bound = ga.abs() * dd + 2.0 * U * (ga.abs() * d + g0.abs())
    C = raw.shape[1]
    return dict(grad_last=out, grad_last_bound=bound, grad_aux_in=-float(bg) * ga.sum(1),
                grad_aux_in_bound=2.0 * (C + 1) * U * abs(float(bg)) * ga.abs().sum(1))


def wgrad(x, dy):
    """dw [N, K] = dy [M, N]^T x [M, K] and its bound."""
    xd, yd = x.double(), dy.double()
    return yd.t() @ xd, 2.0 * (x.shape[0] + 1) * U * (yd.abs().t() @ xd.abs())


def gemm(a, b, bias=None, act=0):
    """act(a [M, K] @ b [K, N] + bias [N]) and its bound; act: 0 none, 1 ReLU, 2 leaky ReLU with the fp32 slope 0.01f (both 1-Lipschitz)."""
    ad, bd = a.double(), b.double()
    K = a.shape[1]
    v = ad @ bd
    mass = ad.abs() @ bd.abs()
    if bias is not None:
        v = v + bias.double()
        mass = mass + bias.double().abs()
    if act == 1:
        v = torch.relu(v)
    elif act == 2:
        v = torch.maximum(v, LEAKY * v)
    return v, 2.0 * (K + 2 + (1 if act == 2 else 0)) * U * mass
