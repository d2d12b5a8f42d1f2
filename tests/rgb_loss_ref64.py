"""An fp64 statement of the RGB step's loss tail (sn_rm_rgb_loss, include/sanerf_hip.h) for the tests alone, and the fp32 round-off
bounds that go with it.  Plain numpy on the CPU; nothing here imports the package.

The inputs are fp32 numbers, and so are the scalar arguments of the entry point (bg_value, lambda_entropy, the coefficients): they are
rounded to fp32 first and exact from then on.  The clamp decisions and the clamp bounds are kept in fp32, because every implementation
has them in fp32 and they decide which branch a ray takes:

    lo = (float)1e-5, hi = (float)(1 - 1e-5);  c = min(max(weights_sum, lo), hi);  inside = lo <= weights_sum <= hi   (a NaN: outside)

Everything after that is float64 (b: the ray's background, a: the truth's alpha):

    gt = t a + b (1 - a)   (RGBA; t otherwise)         pred = image [+ (1 - w) b  unless image_has_bg]         d = pred - gt
    mse = sum d^2 / (3 N)          e = -c log2 c - (1 - c) log2(1 - c),  entropy = sum e / N   (0 when lambda_entropy == 0)
    total = mse + lambda_entropy entropy + coef0 x0 + coef1 x1
    g = grad_image = 2 d / (3 N)
    grad_weights_sum = A + B,   A = -sum_c g_c b_c  (0 with image_has_bg),   B = lambda_entropy / N (log2(1 - c) - log2 c)  (inside; else 0)

Bounds: u = 2^-24, a first-order count of the kernel's fp32 roundings, factor 2 of margin as in tests/grid_ref64.py and
tests/distill_ref64.py, all from the fp64 side.  e_x is the first-order error of x before the margin.
  gt      e_gt = u (|t a| + 2 |b (1 - a)| + |gt|)      t * a;  1 - a and b * (1 - a), both scaled by |b (1 - a)|;  the add.  RGB truth: 0
  pred    e_pred = u (2 |(1 - w) b| + |pred|)          1 - w and (1 - w) * b;  the add.  image_has_bg: 0
  d       e_d = e_pred + e_gt + u |d|                  the one subtraction
  mse     mean(2 |d| e_d + e_d^2) + u mse              the squares and their sum are double (exact at this scale); one rounding to float
  g       (2 / (3 N)) e_d + 3 u |g|                    float(3 N), 1 / it, the product (2 d is exact)
  e       u (3 |c l0| + 4 |(1 - c) l1| + (1 - c) / ln 2 + |e|),  l0 = log2 c, l1 = log2(1 - c)
              log2f is within 1 ulp = 2 u relative -- the HIP math API reference ("Single precision mathematical functions": log2f,
              maximum ULP difference 1) --, so l0 is off by 2 u |l0|; 1 - c is rounded (u (1 - c)), which moves l1 by u / ln 2 and the
              product by u |(1 - c) l1|; l1's own 2 u |l1|; the two products u each; the subtraction u |e|
  entropy mean(e_e) + u |entropy|                      the sum is double; one rounding to float
  total   e_mse + |lam| e_entropy + u (|lam ent| + |coef0 x0| + |coef1 x1|) + 3 u (mse + |lam ent| + |coef0 x0| + |coef1 x1|)
              three products, three adds, each add's result bounded by the sum of the magnitudes: this form holds for any order of the
              adds (the kernel's, and the reference's mse + proposal + distort + entropy)
  A       sum_c |b_c| e_g_c + 3 u sum_c |g_c b_c|       three products, two adds (partial sums bounded by the sum of magnitudes), any order
  B       |k| u (2 |l0| + 2 |l1| + 1 / ln 2 + |l1 - l0|) + 3 u |B|,  k = lam / N
              l0 and l1 as above, their subtraction; float(N), lam / it, the product with k
  grad_weights_sum   e_A + e_B + u |A + B|              the final add
Where the statement's gradient is exactly 0 (a clamped or absent entropy term with image_has_bg) the bound is 0: the kernel's is 0 too.

torch's fp32 chain (what the reference ran to make tests/golden/rgb_step.npz) counts differently in three places; `torch_chain=True`
returns the bounds re-derived for it:
  mse, entropy   torch sums n fp32 terms in fp32, in an order it does not state; any order of n non-negative terms (the squares; the e are
              non-negative too) is within (n - 1) u of their sum, and each square is rounded once more: + n u mse (n = 3 N),
              + N u entropy.  13 roundings become n + 12.
  B           autograd differentiates -w log2 w - (1 - w) log2(1 - w) term by term: -log2 w - 1 / ln 2 and log2(1 - w) + 1 / ln 2, whose
              1 / ln 2 cancel only up to their own roundings.  Each 1 / ln 2 term carries three (w * ln 2, the division, the product
              with w), the four contributions to w are accumulated by three adds of partial sums below |l0| + |l1| + 2 / ln 2:
              e_B = |k| u (5 (|l0| + |l1|) + 13 / ln 2) + 3 u |B|.  The count per ray goes from 8 to 17.
Everything else (gt, pred, d, g, A, total) has the same count in both chains.
"""
import numpy as np

U = 2.0 ** -24
LO, HI = np.float32(1e-5), np.float32(1.0 - 1e-5)
LN2 = float(np.log(2.0))


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def rgb_loss(image, weights_sum, truth, bg=1.0, image_has_bg=True, lambda_entropy=0.0, extras=(), torch_chain=False) -> dict:
    """The statement and its bounds.  image [N,3], weights_sum [N], truth [N,3] or [N,4], bg: a number, [3] or [N,3]; extras: up to two
    (value, coefficient) pairs.  Returns float64 arrays / floats: pred, gt [N,3], mse, entropy, total, grad_image [N,3],
    grad_weights_sum [N], inside [N] (bool), and pred_bound, gt_bound, mse_bound, entropy_bound, total_bound, grad_image_bound,
    grad_weights_sum_bound."""
    im32, w32, tr32 = _f32(image).reshape(-1, 3), _f32(weights_sum).reshape(-1), _f32(truth)
    tr32 = tr32.reshape(-1, tr32.shape[-1])
    N = im32.shape[0]
    assert w32.shape[0] == N and tr32.shape[0] == N and tr32.shape[1] in (3, 4)
    b = np.broadcast_to(_f32(bg).astype(np.float64).reshape(-1, 3) if np.ndim(bg) else np.float64(np.float32(bg)), (N, 3))
    lam = float(np.float32(lambda_entropy))
    ex = [(float(np.float32(v)), float(np.float32(c))) for v, c in extras]
    im, w, tr = im32.astype(np.float64), w32.astype(np.float64), tr32.astype(np.float64)

    # the fp32 decisions
    c32 = np.where(w32 < LO, LO, w32)
    c32 = np.where(c32 > HI, HI, c32).astype(np.float32)
    inside = (w32 >= LO) & (w32 <= HI)
    c = c32.astype(np.float64)

    if tr.shape[1] == 4:
        a = tr[:, 3:4]
        ta, bb = tr[:, :3] * a, b * (1.0 - a)
        gt = ta + bb
        e_gt = U * (np.abs(ta) + 2 * np.abs(bb) + np.abs(gt))
    else:
        gt = tr[:, :3].copy()
        e_gt = np.zeros_like(gt)
    if image_has_bg:
        pred = im.copy()
        e_pred = np.zeros_like(pred)
    else:
        wb = (1.0 - w)[:, None] * b
        pred = im + wb
        e_pred = U * (2 * np.abs(wb) + np.abs(pred))
    d = pred - gt
    e_d = e_pred + e_gt + U * np.abs(d)
    n = 3 * N
    mse = float((d * d).sum() / n)
    e_mse = float((2 * np.abs(d) * e_d + e_d ** 2).mean()) + U * mse
    g = 2.0 * d / n
    e_g = (2.0 / n) * e_d + 3 * U * np.abs(g)

    with np.errstate(divide="ignore", invalid="ignore"):
        l0, l1 = np.log2(c), np.log2(1.0 - c)
    if lam != 0.0:
        e = -c * l0 - (1.0 - c) * l1
        e_e = U * (3 * np.abs(c * l0) + 4 * np.abs((1.0 - c) * l1) + (1.0 - c) / LN2 + np.abs(e))
        entropy = float(e.sum() / N)
        e_entropy = float(e_e.mean()) + U * abs(entropy)
    else:
        entropy, e_entropy = 0.0, 0.0
    terms = [lam * entropy] + [v * cf for v, cf in ex]
    total = mse + sum(terms)
    mags = sum(abs(t) for t in terms)
    e_total = e_mse + abs(lam) * e_entropy + U * mags + 3 * U * (mse + mags)

    if image_has_bg:
        A, e_A = np.zeros(N), np.zeros(N)
    else:
        gb = g * b
        A = -gb.sum(-1)
        e_A = (np.abs(b) * e_g).sum(-1) + 3 * U * np.abs(gb).sum(-1)
    k = lam / N
    if lam != 0.0:
        B = np.where(inside, k * (l1 - l0), 0.0)
        if torch_chain:
            e_B = np.where(inside, abs(k) * U * (5 * (np.abs(l0) + np.abs(l1)) + 13 / LN2) + 3 * U * np.abs(B), 0.0)
        else:
            e_B = np.where(inside, abs(k) * U * (2 * np.abs(l0) + 2 * np.abs(l1) + 1 / LN2 + np.abs(l1 - l0)) + 3 * U * np.abs(B), 0.0)
    else:
        B, e_B = np.zeros(N), np.zeros(N)
    gw = A + B
    e_gw = e_A + e_B + U * np.abs(gw)
    if torch_chain:
        e_mse += n * U * mse
        e_total += n * U * mse
        if lam != 0.0:
            e_entropy += N * U * abs(entropy)
            e_total += abs(lam) * N * U * abs(entropy)
    return {"pred": pred, "gt": gt, "d": d, "mse": mse, "entropy": entropy, "total": total, "grad_image": g, "grad_weights_sum": gw,
            "inside": inside, "N": N,
            "pred_bound": 2 * e_pred, "gt_bound": 2 * e_gt, "mse_bound": 2 * e_mse, "entropy_bound": 2 * e_entropy, "total_bound": 2 * e_total,
            "grad_image_bound": 2 * e_g, "grad_weights_sum_bound": 2 * e_gw}


def worst(got, want, bound) -> float:
    """max |got - want| / bound; where the bound is 0 the values must be equal."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - want)
    assert np.all(err[bound == 0] == 0), "a value whose bound is 0 differs"
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


def kernel_chain_f32(image, weights_sum, truth, bg=1.0, image_has_bg=True, lambda_entropy=0.0, extras=()) -> dict:
    """A numpy-float32 transliteration of k_rgb_loss's chain, operation by operation (np.log2 on float32 in place of log2f; the two sums in
    float64 as the kernel has them): what the bounds above are meant to cover."""
    f = np.float32
    im, w, tr = _f32(image).reshape(-1, 3), _f32(weights_sum).reshape(-1), _f32(truth)
    tr = tr.reshape(-1, tr.shape[-1])
    N = im.shape[0]
    b = np.broadcast_to(_f32(bg).reshape(-1, 3) if np.ndim(bg) else f(bg), (N, 3)).astype(np.float32)
    lam = f(lambda_entropy)
    if tr.shape[1] == 4:
        a = tr[:, 3:4]
        gt = tr[:, :3] * a + b * (f(1) - a)
    else:
        gt = tr[:, :3]
    pred = im if image_has_bg else im + (f(1) - w)[:, None] * b
    d = pred - gt
    assert gt.dtype == np.float32 and pred.dtype == np.float32 and d.dtype == np.float32
    inv = f(1) / f(3 * N)
    g = (f(2) * d) * inv
    mse = f((d.astype(np.float64) ** 2).sum() / (3.0 * N))
    gw = np.zeros(N, np.float32) if image_has_bg else -((g[:, 0] * b[:, 0] + g[:, 1] * b[:, 1]) + g[:, 2] * b[:, 2])
    entropy = f(0)
    if lam != 0:
        c = np.where(w < LO, LO, w)
        c = np.where(c > HI, HI, c).astype(np.float32)
        omc = f(1) - c
        with np.errstate(divide="ignore", invalid="ignore"):
            l0, l1 = np.log2(c), np.log2(omc)
        e = (-c) * l0 - omc * l1
        assert e.dtype == np.float32
        entropy = f(e.astype(np.float64).sum() / N)
        k = lam / f(N)
        gw = np.where((w >= LO) & (w <= HI), gw + k * (l1 - l0), gw).astype(np.float32)
    total = mse + lam * entropy
    for v, cf in extras:
        total = total + f(cf) * f(v)
    assert g.dtype == np.float32 and gw.dtype == np.float32 and np.asarray(total).dtype == np.float32
    return {"pred": pred, "gt": gt, "mse": mse, "entropy": entropy, "total": total, "grad_image": g, "grad_weights_sum": gw}
