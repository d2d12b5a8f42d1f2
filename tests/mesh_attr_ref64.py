"""An fp64 statement of the surface probes that give an exported mesh its vertex colours and instance labels (csrc/mesh_attr.hip,
NeRFRenderer.vertex_attributes) for the tests, with the fp32 round-off bounds that go with it.  Vectorised torch on the CPU; nothing here
imports the package's kernels.

Definition.  A vertex v with mesh normal n (pointing out of the inside); K in {4, 8, 16, 32} probe samples, step h (an fp32 value > 0).
  1. d = -n / |n|;  (0, 0, -1) where |n| is 0 or not finite
  2. t_i = (i + 1/2 - K/2) h;  p_i = v + t_i d  (then the contraction, when the field is contracted)
  3. sigma_i, geo_i in R^15 = the main field at p_i;  label_i = the mask head at p_i.  A label >= 32 (255 = "not evaluated") is in no set.
  4. g_i = (label_i in S) xor invert, true without labels;  y_i = g_i ? h sigma_i : 0 -- a select, not a product
  5. w_i = (1 - exp(-y_i)) exp(-sum_{j<i} y_j), NaN -> 0 (object_ref64's weight without an opaque last sample)
  6. W = sum w_i (the coverage);  G = sum w_i geo_i;  g = G / W where W >= 2^-126, else the fallback (sum_i geo_i) / K, ungated
  7. f = [g | SH4(d / |d|)] (31 values);  colour = sigmoid(view_mlp(f))
  8. vote_l = sum_{i: label_i = l} w_i for l < 32;  vertex label = the lowest l attaining the maximum vote if that is > 0, else 255

Bounds (u = 2^-24; E = 2e-7, the relative error of the library's exp on normal results, pinned by test_oracle_identities; first-order counts
of what the text of k_vertex_probe_composite performs, the library is built with -ffp-contract=off).  The weight's terms are object_ref64's:
  y      one rounded product h sigma (object_ref64 allows two roundings, delta being a difference there; the same 2 u is kept here).
  alpha  e_alpha = exp(-y) (2 u y + E) + u alpha;  y = +inf: alpha = 1 exactly.
         y = 0: the library's exp(-0) is exactly 1 (k = 0, r = 0, the polynomial is 0 + 1), so alpha and the weight are EXACTLY 0 -- no E
         term.  Without this a gated-out vertex (W = 0 exactly, on the device as well) would count as "near the 2^-126 threshold".
  T_i    e_T = T_i (expm1(max(3, i + 2) u S_i) + E) + 2^-149, S_i the prefix (summed in fp64 on the device, rounded to fp32 once).
         S_i = +inf (an opaque sample in front): the library's exp(-inf) is exactly 0, and so is the weight -- no 2^-149 term either.
  w      e_w = e_alpha T + alpha e_T + u w.
  sums   W: K additions from zero, G: K fused multiply-adds from zero: (K + 2) u sum |w v| + sum e_w |v|  (v = 1 for W).
  g      the IEEE division G / W of two perturbed values: (e_G + |g| e_W) / W + u |g| (+ 2^-149, one step of the subnormal grid).
         First order in e_W / W; vertices whose W is within e_W of the 2^-126 threshold could take either branch and are reported apart.
  mean   the fallback: K - 1 additions in sample order, the factor 1/K is a power of two: (K - 1) u sum_i |geo_i| / K + 2^-149.
  SH     f[15:31] = Y: encoders_ref64.head_sh_bound for the kernel's Y (the direction is normalised again in fp32, as the per-ray head does).
  votes  vote_l: at most K additions of weights: (K + 2) u vote_l + sum_{label = l} e_w.  The vertex label is certain where the top vote
         beats every other by more than the two bounds involved and is itself above its bound -- or where no vote can be positive at all.
  d      probe_direction (csrc/mesh_attr.hip): s = n / m (u), the sum of squares (3 u on each square's argument and rounding, 2 additions:
         5 u), the root halves it and rounds (3 u), the division (u): 5 u |d_a|, taken as 6 u |d_a| + 2^-149.
"""
import math

import torch

import encoders_ref64 as er

U = 2.0 ** -24
EXP_REL = 2.0e-7
TINY = 2.0 ** -149
W_MIN = 2.0 ** -126
LABEL_NONE = 255
SAMPLES = (4, 8, 16, 32)


def probe_direction64(normals):
    """[V,3] -> d = -n / |n| in float64; (0, 0, -1) where |n| is 0 or not finite."""
    n = normals.double()
    m = n.abs().amax(-1, keepdim=True)
    ok = torch.isfinite(n).all(-1, keepdim=True) & (m > 0)
    s = n / torch.where(ok, m, torch.ones_like(m))                   # scaled first: fp64 squares of fp32 extremes stay finite anyway
    d = -s / s.pow(2).sum(-1, keepdim=True).sqrt()
    fallback = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).expand_as(d)
    return torch.where(ok, d, fallback)


def direction_bound(d64):
    return 6 * U * d64.abs() + TINY


def probe_offsets(K):
    """The exact factors i + 1/2 - K/2, float64 [K]."""
    return torch.arange(K, dtype=torch.float64) + 0.5 - K / 2


def probe_points32(vertices, dirs, K, h):
    """The fp32 restatement of step 2 from given fp32 directions: t = fl(c_i h), p = fl(v + fl(t d)).  [V,3], [V,3] -> [V,K,3] float32."""
    t = probe_offsets(K).float() * torch.tensor(h, dtype=torch.float32)
    return vertices.float()[:, None, :] + t[None, :, None] * dirs.float()[:, None, :]


def gate(labels, keep_mask, invert):
    lab = labels.long()
    in_set = (lab < 32) & (((torch.tensor(int(keep_mask), dtype=torch.int64) >> lab.clamp(max=31)) & 1) != 0)
    return in_set != bool(invert)


def vertex_probe_ref64(sigmas, geo, dirs, h, labels=None, keep_mask=0xFFFFFFFF, invert=False):
    """Steps 4-8 in float64 (but the perceptron).  sigmas [V,K], geo [V,K,15], dirs [V,3], h an fp32 value, labels [V,K] integer or None.
    Returns the outputs and the bounds of the module docstring."""
    sg, gf = sigmas.double(), geo.double()
    V, K = sg.shape
    h = float(torch.tensor(h, dtype=torch.float32))
    g = gate(labels, keep_mask, invert) if labels is not None else torch.ones(V, K, dtype=torch.bool)
    y = torch.where(g, h * sg, torch.zeros_like(sg))
    S = torch.cat([torch.zeros(V, 1, dtype=torch.float64), torch.cumsum(y, dim=-1)[:, :-1]], dim=-1)
    alpha = 1.0 - torch.exp(-y)
    tr = torch.exp(-S)
    w = (alpha * tr).nan_to_num(0.0, posinf=math.inf, neginf=-math.inf)
    W = w.sum(-1)
    G = (w[:, :, None] * gf).sum(1)
    mean = gf.sum(1) / K
    normal = W >= W_MIN
    gmean = torch.where(normal[:, None], G / torch.where(normal, W, torch.ones_like(W))[:, None], mean)
    sh = er.sh_values(er.head_direction(dirs), 4)
    out = dict(gate=g, y=y, weights=w, coverage=W, G=G, mean=mean, normal=normal, g=gmean, f=torch.cat([gmean, sh], dim=-1), sh=sh)
    # ---- error terms
    yf = torch.where(torch.isinf(y), torch.zeros_like(y), y)
    e_alpha = torch.where(torch.isinf(y) | (y == 0), torch.zeros_like(y), torch.exp(-yf) * (2 * U * yf + EXP_REL)) + U * alpha
    count = torch.arange(K, dtype=torch.float64).add(2).clamp(min=3)[None, :]
    Sf = torch.where(torch.isfinite(S), S, torch.zeros_like(S))
    e_T = torch.where(torch.isfinite(S), tr * (torch.expm1(count * U * Sf) + EXP_REL), torch.zeros_like(S)) + TINY
    e_w = (e_alpha * tr + alpha * e_T + U * w.abs()).nan_to_num(0.0)
    e_w = torch.where((y == 0) | (S == math.inf), torch.zeros_like(e_w), e_w)      # exactly 0 on the device as well
    e_W = (K + 2) * U * w.abs().sum(-1) + e_w.sum(-1)
    e_G = (K + 2) * U * (w[:, :, None] * gf).abs().sum(1) + (e_w[:, :, None] * gf.abs()).sum(1)
    Wd = torch.where(normal, W, torch.ones_like(W))[:, None]
    g_bound = torch.where(normal[:, None], (e_G + gmean.abs() * e_W[:, None]) / Wd + U * gmean.abs(), (K - 1) * U * gf.abs().sum(1) / K) + TINY
    out.update(weights_bound=e_w, coverage_bound=e_W, G_bound=e_G, g_bound=g_bound,
               f_bound=torch.cat([g_bound, er.head_sh_bound(dirs)], dim=-1),
               branch_certain=(W - W_MIN).abs() > e_W)
    if labels is not None:
        lab = labels.long()
        onehot = (lab[:, :, None] == torch.arange(32)[None, None, :]).double()                 # [V,K,32]; a label >= 32 votes nowhere
        votes = (w[:, :, None] * onehot).sum(1)
        e_votes = (K + 2) * U * votes + (e_w[:, :, None] * onehot).sum(1)
        top = votes.max(-1).values
        idx = torch.arange(32).expand_as(votes)
        arg = torch.where(votes == top[:, None], idx, torch.full_like(idx, 32)).min(-1).values
        vlabel = torch.where(top > 0, arg, torch.full_like(arg, LABEL_NONE))
        e_top = e_votes.gather(1, arg[:, None])[:, 0]
        others = torch.ones_like(votes, dtype=torch.bool).scatter(1, arg[:, None], False)
        rival = torch.where(others, votes + e_votes, torch.full_like(votes, -math.inf)).max(-1).values   # the most any other label can reach
        nothing = (votes + e_votes).max(-1).values == 0                                         # no vote can be positive: 255 for certain
        certain = nothing | ((top - e_top > rival) & (top - e_top > 0))
        out.update(votes=votes, votes_bound=e_votes, vertex_label=vlabel, label_certain=certain)
    return out


def random_case(V, K, mode, seed=0):
    """The inputs of the composite tests: sigmas log-uniform over 1e-3 .. 1e3 with zeros, +inf and NaN sprinkled in, geo ~ N(0,1), unit-ish
    directions, labels over 3 ids plus 255.  mode: "plain" (no labels), "keep" ({0, 2}), "invert" ({1} inverted).  One generator for the
    CPU and the GPU tests: the CPU test checks that the reference's own near-ties stay rare for exactly these inputs."""
    g = torch.Generator().manual_seed(1000 * seed + 37 * K + V)
    sg = torch.exp(torch.empty(V, K).uniform_(math.log(1e-3), math.log(1e3), generator=g))
    r = torch.rand(V, K, generator=g)
    sg = torch.where(r < 0.15, torch.zeros_like(sg), sg)
    sg = torch.where((r >= 0.15) & (r < 0.17), torch.full_like(sg, math.inf), sg)
    sg = torch.where((r >= 0.17) & (r < 0.18), torch.full_like(sg, math.nan), sg)
    geo = torch.randn(V, K, 15, generator=g)
    dirs = torch.randn(V, 3, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    lab = torch.randint(0, 4, (V, K), generator=g)
    labels = torch.where(lab == 3, torch.full_like(lab, LABEL_NONE), lab).to(torch.uint8)
    if V >= 17:
        labels[3] = 1                      # a vertex of one label: gated out entirely by "keep", kept entirely by neither
        labels[5] = LABEL_NONE             # nothing evaluated: no vote
        sg[7] = 0.0                        # empty space: W = 0 without any gate
    kw = {"plain": dict(labels=None), "keep": dict(labels=labels, keep_mask=0b101, invert=False),
          "invert": dict(labels=labels, keep_mask=0b010, invert=True)}[mode]
    return dict(sigmas=sg, geo=geo, dirs=dirs, h=0.013, **kw)
