"""An fp64 statement of "render a segmented object alone" (csrc/object.hip, NeRFRenderer.render_object) for the tests, with the fp32
round-off bounds that go with it.  Vectorised torch on the CPU; nothing here imports the package's kernels.

Definition.  One ray, the T samples of the last stage of the ordinary render: densities sigma_i, real bin edges b_0 .. b_T with
delta_i = b_{i+1} - b_i, mid-points t_i = (b_{i+1} + b_i) / 2, geometry channels geo_i in R^15, positions x_i.
  1. l_i = mask_mlp(cat[m_grid(x_i), geo_i]) in R^K;  label_i = the lowest index attaining max_k l_i,k
  2. g_i = (label_i in S) xor invert;  S = the set bits of a 32-bit keep mask; a label >= 32 (255 = "not evaluated") is in no S
  3. y_i = g_i ? delta_i sigma_i : 0 -- a select, not a product: a gated-out sigma = inf gives 0, not NaN.
     last_sample_opaque (opt.background == 'last_sample'): y_{T-1} = g_{T-1} ? +inf : 0
  4. alpha_i = 1 - exp(-y_i);  T_i = exp(-sum_{j<i} y_j);  w'_i = alpha_i T_i, NaN -> 0 as weights_from_sigma does
  5. weights_sum = sum w'_i;  depth = sum w'_i t_i;  f = [sum w'_i geo_i | (sum w'_i) SH4(d / |d|)] (31 values);
     object_image = sigmoid(view_mlp(f)) + (1 - sum w') bg
w'_i can be non-zero where the ordinary w_i is exactly 0 (the occluder in front is gated away).

Note on S = {} (nothing kept): every w' is 0, so f = 0 and object_image = sigmoid(view_mlp(0)) + bg.  For the bias-free view_mlp of the
reference network that is 0.5 + bg -- exactly what the ordinary render gives a ray that hits nothing (renderer.py:339-353) -- not bg.

Bounds (u = 2^-24; E = 2e-7, the relative error of the library's exp on normal results, pinned by test_oracle_identities; first-order
counts of what the text of k_object_composite performs, the library is built with -ffp-contract=off):
  y      delta is one rounded subtraction, delta sigma one rounded product: y_fp32 = y (1 + 2 u).
  alpha  1 - exp(-y):  exp(-y) moves by exp(-y) 2 u y with y and by exp(-y) E by itself, the subtraction rounds alpha once:
         e_alpha = exp(-y) (2 u y + E) + u alpha.   (y = +inf: alpha = 1 exactly.)
  T_i    the prefix is summed in fp64 from the fp32 y_j (2 u each) and rounded to fp32 once (u): the argument is within 3 u S_i of
         S_i = sum_{j<i} y_j, which is below the (i + 2) u S_i of a prefix summed in fp32 -- the bound used is the larger,
         max(3, i + 2) u S_i, so that a scan in fp32 would pass as well -- and exp adds E:
         e_T = T_i (expm1(max(3, i + 2) u S_i) + E) + 2^-149 (one step of the subnormal grid, where the relative statement ends).
  w'     one rounded product: e_w = e_alpha T + alpha e_T + u w'.
  sums   a chain of T fused multiply-adds from zero, each rounding a partial sum of at most the mass, the mid-point's own rounded
         addition for the depth: (T + 2) u sum |w' v| + sum e_w |v|.
  SH     f[15:31] = Y ws: encoders_ref64.head_sh_bound for the kernel's Y, |Y| e_ws, u |Y ws|.
"""
import math

import torch

import encoders_ref64 as er

U = 2.0 ** -24
EXP_REL = 2.0e-7
LABEL_SKIPPED = 255


def labels_from_logits(logits):
    """[..., K] -> the lowest index attaining the maximum, int64 (NaN never wins; a row of NaN / -inf gives 0)."""
    lg = logits.double()
    lg = torch.where(torch.isnan(lg), torch.full_like(lg, -math.inf), lg)
    mx = lg.max(dim=-1, keepdim=True).values
    K = lg.shape[-1]
    idx = torch.arange(K).expand_as(lg)
    return torch.where(lg == mx, idx, torch.full_like(idx, K)).min(dim=-1).values


def top_two_margin(logits):
    """[..., K] float64 -> top value minus the runner-up (inf for K = 1)."""
    lg = logits.double()
    if lg.shape[-1] == 1:
        return torch.full(lg.shape[:-1], math.inf, dtype=torch.float64)
    top = lg.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def gate(labels, keep_mask, invert):
    lab = labels.long()
    in_set = (lab < 32) & (((torch.tensor(int(keep_mask), dtype=torch.int64) >> lab.clamp(max=31)) & 1) != 0)
    return in_set != bool(invert)


def object_ref64(sigmas, real_bins, geo, rays_d, keep_mask, invert=False, last_sample_opaque=False, labels=None, logits=None,
                 view_weights=None, bg=None):
    """Steps 1-5 in float64.  sigmas [N,T], real_bins [N,T+1], geo [N,T,15], rays_d [N,3]; labels [N,T] integer or logits [N,T,K].
    view_weights: the bias-free view_mlp's weight matrices (ReLU between them) + bg (scalar or [N,3]) -> object_image as well.
    Returns the outputs and the absolute-term sums / error terms the bounds need (see the module docstring)."""
    if labels is None:
        labels = labels_from_logits(logits)
    sg, rb, gf = sigmas.double(), real_bins.double(), geo.double()
    N, T = sg.shape
    g = gate(labels, keep_mask, invert)
    delta = rb[:, 1:] - rb[:, :-1]
    y = torch.where(g, delta * sg, torch.zeros_like(sg))
    if last_sample_opaque:
        y[:, -1] = torch.where(g[:, -1], torch.full_like(y[:, -1], math.inf), torch.zeros_like(y[:, -1]))
    S = torch.cat([torch.zeros(N, 1, dtype=torch.float64), torch.cumsum(y, dim=-1)[:, :-1]], dim=-1)
    alpha = 1.0 - torch.exp(-y)
    tr = torch.exp(-S)
    w = (alpha * tr).nan_to_num(0.0, posinf=math.inf, neginf=-math.inf)
    tm = (rb[:, 1:] + rb[:, :-1]) / 2
    sh = er.sh_values(er.head_direction(rays_d), 4)
    ws = w.sum(-1)
    f = torch.cat([(w[:, :, None] * gf).sum(1), sh * ws[:, None]], dim=-1)
    out = dict(labels=labels, gate=g, y=y, weights=w, weights_sum=ws, depth=(w * tm).sum(-1), f_image=f, sh=sh)
    # ---- error terms
    yf = torch.where(torch.isinf(y), torch.zeros_like(y), y)
    e_alpha = torch.where(torch.isinf(y), torch.zeros_like(y), torch.exp(-yf) * (2 * U * yf + EXP_REL)) + U * alpha
    count = torch.arange(T, dtype=torch.float64).add(2).clamp(min=3)[None, :]
    Sf = torch.where(torch.isfinite(S), S, torch.zeros_like(S))
    e_T = torch.where(torch.isfinite(S), tr * (torch.expm1(count * U * Sf) + EXP_REL), torch.zeros_like(S)) + 2.0 ** -149
    e_w = (e_alpha * tr + alpha * e_T + U * w.abs()).nan_to_num(0.0)
    out["weights_bound"] = e_w
    out["weights_sum_bound"] = (T + 2) * U * w.abs().sum(-1) + e_w.sum(-1)
    out["depth_bound"] = (T + 2) * U * (w * tm).abs().sum(-1) + (e_w * tm.abs()).sum(-1)
    geo_bound = (T + 2) * U * (w[:, :, None] * gf).abs().sum(1) + (e_w[:, :, None] * gf.abs()).sum(1)
    sh_bound = ws.abs()[:, None] * er.head_sh_bound(rays_d) + sh.abs() * out["weights_sum_bound"][:, None] + U * (sh * ws[:, None]).abs()
    out["f_image_bound"] = torch.cat([geo_bound, sh_bound], dim=-1)
    if view_weights is not None:
        h = f
        for i, W in enumerate(view_weights):
            h = h @ W.double().t()
            if i + 1 < len(view_weights):
                h = torch.relu(h)
        bgt = bg.double() if torch.is_tensor(bg) else torch.tensor(float(bg), dtype=torch.float64)
        out["object_image"] = torch.sigmoid(h) + (1 - ws)[:, None] * bgt
    return out


def plain_weights64(sigmas, real_bins, last_sample_opaque):
    """renderer.py:308-325 (weights_from_sigma) in float64, stated independently of object_ref64."""
    sg, rb = sigmas.double(), real_bins.double()
    ds = (rb[:, 1:] - rb[:, :-1]) * sg
    if last_sample_opaque:
        ds = torch.cat([ds[:, :-1], torch.full_like(ds[:, -1:], math.inf)], dim=-1)
    trans = torch.exp(-torch.cat([torch.zeros_like(ds[:, :1]), torch.cumsum(ds[:, :-1], dim=-1)], dim=-1))
    return ((1 - torch.exp(-ds)) * trans).nan_to_num(0)


def skipped_tiles(live):
    """[N,T] -> bool [N,T]: the samples of the 128-sample tiles (rays 32 r .. 32 r + 31 x depth indices 4 p .. 4 p + 3, rays past N count
    as zeros) whose live values are all exactly 0 -- the tiles sn_rm_mask_point_labels skips."""
    N, T = live.shape
    nz = torch.zeros(((N + 31) // 32) * 32, T, dtype=torch.bool)
    nz[:N] = live.cpu() != 0
    tile_live = nz.view(-1, 32, T // 4, 4).any(dim=3).any(dim=1)             # [groups, T/4]
    return (~tile_live)[:, None, :, None].expand(-1, 32, -1, 4).reshape(-1, T)[:N]
