"""An fp64 statement of the 256-wide split-fp16 perceptron kernels of csrc/mlp.hip (k_pack_mlp_wide, k_mlp_wide_j<0|1|2> and its SAVE = 1
training instantiation, the backward kernels k_mlp_wide<4> and k_mlp_wide<5>) and the per-element bounds that go with it.

Written for the tests alone: plain torch that runs on any device and imports nothing from the package or from oracle/.

The scheme.  Every fp32 operand v is held as two fp16 halves, hi = fp16(v) and lo = fp16(v - hi), both round-to-nearest (v - hi is exact
in fp32), and a product w * h is taken as THREE fp16 x fp16 products with fp32 accumulation: Wh*hh + Wl*hh + Wh*hl.  The Wl*hl term is
absent by design.  split() states the halves (fp16 subnormals kept -- the default of hipcc's kernel mode -- or flushed to zero), layer() the
three-product sum in float64.  On data for which every kept product and every partial sum is exact in fp32 the statement IS the answer
(wide_cases.py); on float data the bounds below hold per ELEMENT.

Bounds (u = 2^-24; a first-order count of the roundings times the factor 2 of margin of the sibling modules).  They bound the distance of
the kernel from the statement; the representation terms also cover the distance of either from the product of the unsplit values.
  rho(v) = |v - hi - lo|   the representation error of an operand.  For the inputs and the weights it is evaluated EXACTLY from split().  A
           hidden value, which the kernel holds with error E, has 11 + 11 significand bits and a sign in its two halves:
           rho(h) <= 4 u (|h| + E) + 2^-25   (2^-23 relative, i.e. 2 u, for the kernel's value AND for the statement's; the absolute floor is
           half of fp16's subnormal spacing 2^-24, below which a lo half has no bits left).
  layer    K terms, each three products, accumulated in fp32 from the bias in any order: the products are exact in fp32 (11 x 11 bits), their
           3 K additions round, the matrix unit may add a k-step's sixteen products in a tree of its own and the bias is one more term: counted
           as 3 K + 2 roundings of partial sums, each bounded by the absolute mass; one more (3 K + 3) where the fp32 product 0.01f * t of a
           leaky unit follows.  With the margin:
             E' = |W| E + |W| rho(h) + rho(W) (|h| + E) + |Wl| |hl| + 2 (3 K + 2) u (|W| (|h| + E) + |bias|),   |hl| <= 2^-11 (|h| + E)
           (for the inputs |hl| is taken from split()).  |Wl| |hl| is the term the scheme drops.  The activation max(t, 0.01f t) or
           max(t, 0) is 1-Lipschitz: E' holds for the hidden output as it does for the pre-activation, no exclusions.
  backward the same recurrence through |W|^T with K = the layer's output width and the gates GIVEN (slope 1, 0.01f or 0; a unit with
           slope 0 is exactly 0 and its bound is 0).  Every row of grad_out is scaled by the power of two that brings its largest entry
           into [1, 2) and the results are scaled back: exact, so the scale drops out of values and bounds while the row's exponent is
           inside the kernel's window -100 < e < 100 (outside it the row runs unscaled, which the statement follows).
  LayerNorm over n outputs y held with error E (mean, biased variance, 1 / sqrtf and the division correctly rounded in this build):
             dm  = mean(E) + 2 (n + 1) u mean(|y| + E)                       n - 1 additions, one cross-lane addition, one division
             Ed  = E + dm + 2 u (|d| + E + dm)                               d = y - mean: one rounding
             dv  = mean(2 |d| Ed + Ed^2) + 2 (n + 2) u mean((|d| + Ed)^2)    n products, n additions, one division
             da  = dv + 2 u (var + eps)                                      the addition of eps
             dr  = da / 2 (a - da)^-3/2 + 2 * 2 u (a - da)^-1/2              a = var + eps; the square root and the division
             out = d r w + b:  |w| (Ed (r + dr) + |d| dr) + 2 * 3 u (|d r w| + |b|)
"""
import torch

U = 2.0 ** -24
LEAKY = float(torch.tensor(0.01, dtype=torch.float32))
F16_MIN_NORMAL = 2.0 ** -14
WIDE = 256


def _flush(h16):
    return torch.where(h16.float().abs() < F16_MIN_NORMAL, torch.zeros_like(h16), h16)


def split(v, keep_subnormals=True):
    """(hi, lo) of the fp32 value of v, as float64: hi = fp16(v), lo = fp16(v - hi), round-to-nearest; keep_subnormals=False flushes fp16
    subnormals of either half to zero."""
    v32 = v.to(torch.float32)
    hi = v32.to(torch.float16)
    if not keep_subnormals:
        hi = _flush(hi)
    lo = (v32 - hi.float()).to(torch.float16)
    if not keep_subnormals:
        lo = _flush(lo)
    return hi.double(), lo.double()


def layer(h, W, bias=None, keep_subnormals=True):
    """sum_k (Wh*hh + Wl*hh + Wh*hl) + bias in float64: h [M, K], W [N, K] (nn.Linear.weight), bias [N] or None -> [M, N]."""
    hh, hl = split(h, keep_subnormals)
    Wh, Wl = split(W, keep_subnormals)
    y = hh @ Wh.t() + hh @ Wl.t() + hl @ Wh.t()
    return y if bias is None else y + bias.double()


def _block(v, E, rho, lo_abs, W, keep):
    """One operand block [M, K] (values v with error E, representation error rho, |lo| <= lo_abs) against the weight columns W [N, K]:
    (three-product sum, error carried in, absolute mass)."""
    Wd = W.double()
    Wh, Wl = split(W, keep)
    Wa = Wd.abs()
    carried = E @ Wa.t() + rho @ Wa.t() + (v.abs() + E) @ (Wd - Wh - Wl).abs().t() + lo_abs @ Wl.abs().t()
    return layer(v, W, None, keep), carried, (v.abs() + E) @ Wa.t()


def _external(x, keep):
    """An external operand (inputs, grad_out): exact in fp32, its halves stated by split()."""
    xd = x.to(torch.float32).double()
    hi, lo = split(x, keep)
    return xd, torch.zeros_like(xd), (xd - hi - lo).abs(), lo.abs()


def _internal(h, E):
    return h, E, 4.0 * U * (h.abs() + E) + 2.0 ** -25, 2.0 ** -11 * (h.abs() + E)


def chain_forward(x, weights, biases=None, skip_layers=(), leaky=False, keep_subnormals=True):
    """SkipConnMLP / MLP of nerf/network.py:9-66.  x [M, din]; weights: nn.Linear.weight per layer, a skip layer's is [out, 256 + din] and
    consumes cat([h, x]); biases: None or a list with None entries; LeakyReLU with the fp32 literal 0.01f, else ReLU, spelled max(t, slope t);
    no activation after the last layer -> dict of float64: hidden / hidden_bound (lists, post-activation), raw / raw_bound, and mass (per layer,
    the absolute mass sum |w| |h| + |bias| that bounds every partial sum)."""
    keep = keep_subnormals
    L = len(weights)
    ext = _external(x, keep)
    h = E = None
    hs, Es, masses = [], [], []
    for l, W in enumerate(weights):
        blocks = [(ext, W)] if l == 0 else [(_internal(h, E), W[:, :WIDE])]
        if l > 0 and l in skip_layers:
            blocks.append((ext, W[:, WIDE:]))
        K = sum(Wb.shape[1] for _, Wb in blocks)
        assert K == W.shape[1], f"layer {l}: weight has {W.shape[1]} columns, its input {K}"
        y = carried = mass = 0.0
        for op, Wb in blocks:
            yb, cb, mb = _block(*op, Wb, keep)
            y, carried, mass = y + yb, carried + cb, mass + mb
        b = biases[l] if biases is not None else None
        if b is not None:
            y, mass = y + b.double(), mass + b.double().abs()
        last = l + 1 == L
        E = carried + 2.0 * (3 * K + (3 if leaky and not last else 2)) * U * mass
        masses.append(mass)
        if last:
            return dict(hidden=hs, hidden_bound=Es, raw=y, raw_bound=E, mass=masses)
        h = torch.maximum(y, (LEAKY if leaky else 0.0) * y) + 0.0
        hs.append(h)
        Es.append(E)


def row_scale(g):
    """The exact power of two per row that the backward kernels multiply grad_out by (1 where they leave the row alone)."""
    g = g.to(torch.float32).double()
    mx = g.abs().amax(1)
    _, ex = torch.frexp(mx)                          # mx = m 2^ex, m in [0.5, 1): the IEEE exponent is ex - 1
    e = (ex - 1).double()
    scaled = (mx > 0) & torch.isfinite(mx) & (e > -100) & (e < 100)
    return torch.where(scaled, torch.exp2(-e), torch.ones_like(e))[:, None]


def chain_backward(g_last, weights, gate, leaky=False, keep_subnormals=True):
    """g_last [M, dL] = gradient of the last pre-activation; gate: per hidden layer a bool [M, 256], GIVEN (hidden > 0 for
    sn_mlp_wide_backward, the bit for sn_mlp_wide_backward_bits); slope 0.01f or 0 where the gate is closed -> dict of float64:
    grad_hidden / grad_hidden_bound (lists indexed by forward layer: gradient of that layer's pre-activation), grad_in / grad_in_bound; scale
    [M, 1], and in the SCALED domain mass (per forward layer) and scaled_in (grad_in before it is scaled back)."""
    keep = keep_subnormals
    L = len(weights)
    s = row_scale(g_last)
    op = _external(g_last.to(torch.float32).double() * s, keep)
    gh, gE, masses = [None] * (L - 1), [None] * (L - 1), [None] * L
    for l in range(L - 1, -1, -1):
        Wt = weights[l].t()                              # [in, out]: the layer's transposed matrix
        y, carried, mass = _block(*op, Wt, keep)
        K = Wt.shape[1]
        masses[l] = mass
        if l == 0:
            E = carried + 2.0 * (3 * K + 2) * U * mass
            return dict(grad_hidden=gh, grad_hidden_bound=gE, grad_in=y / s + 0.0, grad_in_bound=E / s, scale=s, mass=masses, scaled_in=y)
        open_ = gate[l - 1].to(y.device)
        slope = torch.where(open_, 1.0, LEAKY if leaky else 0.0).double()
        E = (carried + 2.0 * (3 * K + (3 if leaky else 2)) * U * mass) * slope
        y = y * slope + 0.0
        gh[l - 1], gE[l - 1] = y / s + 0.0, E / s
        op = _internal(y, E)


def layer_norm(y, w, b, eps, E=None):
    """torch.nn.LayerNorm over the last dimension in float64 -> (out, bound); E: the error y already has."""
    y = y.double()
    E = torch.zeros_like(y) if E is None else E.double()
    w, b = w.double(), b.double()
    n = y.shape[1]
    mean = y.mean(1, keepdim=True)
    d = y - mean
    var = (d * d).mean(1, keepdim=True)
    a = var + eps
    r = a.rsqrt()
    out = d * r * w + b
    dm = E.mean(1, keepdim=True) + 2.0 * (n + 1) * U * (y.abs() + E).mean(1, keepdim=True)
    Ed = E + dm + 2.0 * U * (d.abs() + E + dm)
    dv = (2.0 * d.abs() * Ed + Ed * Ed).mean(1, keepdim=True) + 2.0 * (n + 2) * U * ((d.abs() + Ed) ** 2).mean(1, keepdim=True)
    da = dv + 2.0 * U * a
    a_lo = torch.clamp(a - da, min=1e-300)
    dr = 0.5 * da * a_lo ** -1.5 + 2.0 * 2 * U * a_lo ** -0.5
    bound = w.abs() * (Ed * (r + dr) + d.abs() * dr) + 2.0 * 3 * U * ((d * r * w).abs() + b.abs())
    return out, bound


# ---- sign bits (WideArgs::bits of csrc/mlp.hip): per row two half-waves of four 32-bit words; bit 16 t + r of half-wave `half`
#      <-> neuron 32 t + (r & 3) + 8 (r >> 2) + 4 half ----
def _neuron_of_bit():
    idx = torch.empty(8, 32, dtype=torch.long)
    for half in range(2):
        for t in range(8):
            for r in range(16):
                B = 16 * t + r
                idx[4 * half + (B >> 5), B & 31] = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half
    return idx


def pack_sign_bits(positive):
    """bool [M, 256] -> int32 [M, 8]."""
    idx = _neuron_of_bit().to(positive.device)
    bits = positive[:, idx].to(torch.int64)                                  # [M, 8, 32]
    words = (bits << torch.arange(32, device=positive.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def unpack_sign_bits(words):
    """int32 [M, 8] -> bool [M, 256]."""
    idx = _neuron_of_bit().to(words.device)
    bits = (words.to(torch.int64)[:, :, None] >> torch.arange(32, device=words.device)) & 1
    out = torch.zeros(words.shape[0], WIDE, dtype=torch.bool, device=words.device)
    out[:, idx.reshape(-1)] = bits.reshape(words.shape[0], -1).bool()
    return out
