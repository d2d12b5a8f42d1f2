"""An fp64 statement of the SSIM the reference's SSIMMeter computes (nerf/metrics.py:124-131: torchmetrics'
structural_similarity_index_measure at its defaults), for the tests alone: plain torch on the CPU, nothing here imports the package.

    g = exp(-(d / 1.5)^2 / 2), d = -5 .. 5, over its sum; window w = g (x) g
    data_range = the given value, or max(pred.max - pred.min, truth.max - truth.min)
    c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2
    per channel and pixel, w-weighted over the 11 x 11 window: mu_p, mu_t, E[pp], E[tt], E[pt]
    s_p^2 = max(E[pp] - mu_p^2, 0), s_t^2 alike, s_pt = E[pt] - mu_p mu_t
    ssim = ((2 mu_p mu_t + c1)(2 s_pt + c2)) / ((mu_p^2 + mu_t^2 + c1)(s_p^2 + s_t^2 + c2))
    value = mean over the 3 channels and the pixels 5 <= y < H - 5, 5 <= x < W - 5

`ssim_valid` evaluates whole windows over the interior; `ssim_padded` is the package's own form: reflect-pad by 5, evaluate everywhere,
crop 5 -- the padding never reaches a kept pixel, so the two agree to round-off.  `ssim_f32_torch` is the padded form in fp32 (the
torch-operator route a user would otherwise take), for scale.  Inputs: [H,W,3] tensors or arrays."""
import torch
import torch.nn.functional as F

TAPS, R, SIGMA = 11, 5, 1.5


def gaussian(dtype=torch.float64) -> torch.Tensor:
    d = torch.arange(TAPS, dtype=dtype) - R
    g = torch.exp(-((d / SIGMA) ** 2) / 2)
    return g / g.sum()


def _chw(x, dtype) -> torch.Tensor:
    x = torch.as_tensor(x).detach().cpu().to(dtype)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"an [H,W,3] image, got {tuple(x.shape)}")
    return x.permute(2, 0, 1).contiguous()


def derived_range(pred, truth, dtype=torch.float64) -> float:
    p, t = torch.as_tensor(pred).to(dtype), torch.as_tensor(truth).to(dtype)
    return float(torch.maximum(p.max() - p.min(), t.max() - t.min()))


def _map(p, t, data_range, dtype):
    """The per-pixel ssim [3, h - 10, w - 10] of [3,h,w] images: every whole window."""
    if p.shape[1] < TAPS or p.shape[2] < TAPS:
        raise ValueError(f"a {p.shape[1]} x {p.shape[2]} image is smaller than the {TAPS} x {TAPS} window")
    g = gaussian(dtype)
    w = (g[:, None] * g[None, :]).expand(3, 1, TAPS, TAPS).contiguous()
    stack = torch.cat([p, t, p * p, t * t, p * t])[None]                         # [1,15,h,w]
    m = F.conv2d(stack, w.repeat(5, 1, 1, 1), groups=15)[0]
    mu_p, mu_t, e_pp, e_tt, e_pt = m[0:3], m[3:6], m[6:9], m[9:12], m[12:15]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    var_p, var_t = torch.clamp(e_pp - mu_p * mu_p, min=0), torch.clamp(e_tt - mu_t * mu_t, min=0)
    cov = e_pt - mu_p * mu_t
    return ((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2))


def ssim_valid(pred, truth, data_range=None, dtype=torch.float64) -> float:
    p, t = _chw(pred, dtype), _chw(truth, dtype)
    dr = derived_range(p, t, dtype) if data_range is None else float(data_range)
    return float(_map(p, t, dr, dtype).mean())


def ssim_padded(pred, truth, data_range=None, dtype=torch.float64) -> float:
    p, t = _chw(pred, dtype), _chw(truth, dtype)
    dr = derived_range(p, t, dtype) if data_range is None else float(data_range)
    pp, tp = (F.pad(x[None], (R, R, R, R), mode="reflect")[0] for x in (p, t))
    return float(_map(pp, tp, dr, dtype)[:, R:-R, R:-R].mean())


def ssim_f32_torch(pred, truth, data_range=None) -> float:
    return ssim_padded(pred, truth, data_range, dtype=torch.float32)


def ssim_single_window(pred, truth, data_range) -> float:
    """H = W = 11: one window per channel, written out as sums (no convolution)."""
    p, t = _chw(pred, torch.float64), _chw(truth, torch.float64)
    assert p.shape[1:] == (TAPS, TAPS)
    g = gaussian()
    w = g[:, None] * g[None, :]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vals = []
    for c in range(3):
        mu_p, mu_t = (w * p[c]).sum(), (w * t[c]).sum()
        var_p = max((w * p[c] * p[c]).sum() - mu_p * mu_p, 0.0)
        var_t = max((w * t[c] * t[c]).sum() - mu_t * mu_t, 0.0)
        cov = (w * p[c] * t[c]).sum() - mu_p * mu_t
        vals.append(((2 * mu_p * mu_t + c1) * (2 * cov + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (var_p + var_t + c2)))
    return float(sum(vals) / 3)
