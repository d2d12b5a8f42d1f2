"""Inputs of the object-render tests, built on the CPU from committed seeds (the GPU tests move them over), and their fp64 references."""
import functools
import math

import torch

import grid_ref64 as gref
import object_ref64 as oref

E = 15
LABEL_CASES = [(37, 4, 2, 16), (70, 32, 3, 16), (33, 128, 16, 16), (40, 8, 2, 6)]      # (N, T, K, L)
TAU_REL = 1e-4            # the project's bound for the 256-wide matrix-core kernels (test_gpu_heads.py:48): tau = 1e-4 max(1, max |ref|)
MARGIN_SHARE_MAX = 0.02   # evaluated samples whose fp64 top-two margin is within 2 tau: at most this share


@functools.lru_cache(maxsize=None)
def label_case(N, T, K, L):
    """The mask head of test_fused_mask_head_just_in_time_kernel_agrees (E = 15, positions partly outside the box) and a `live` array whose
    tails are zero on every second group of 32 rays (about a third of the rays): whole 128-sample tiles are skipped there; a fifth of the
    other values are zero one by one (evaluated samples with y == 0)."""
    from sanerf_hq_amd.gridencoder import GridEncoder
    from sanerf_hq_amd.nerf.network import SkipConnMLP
    torch.manual_seed(1000 * N + T)
    enc = GridEncoder(input_dim=3, num_levels=L, level_dim=8, base_resolution=16, log2_hashmap_size=15, desired_resolution=512)
    with torch.no_grad():
        enc.embeddings.uniform_(-1.0, 1.0)
    mlp = SkipConnMLP(L * 8 + E, K, 256, 3, skip_layers=[], bias=False)
    g = torch.Generator().manual_seed(N + 7 * T + K)
    xyz = torch.rand(N, T, 3, generator=g) * 2.2 - 1.1
    extra = torch.randn(N, T, E, generator=g)
    live = torch.rand(N, T, generator=g) + 0.01
    live[torch.rand(N, T, generator=g) < 0.2] = 0.0
    group = torch.arange(N) // 32
    live[group % 2 == 1, (T // 2 if T > 4 else 0):] = 0.0
    return enc, mlp, xyz, extra, live


@functools.lru_cache(maxsize=None)
def label_ref(N, T, K, L):
    """fp64 perceptron on the fp64 grid encoding: logits [N,T,K] float64, tau, labels, margin."""
    enc, mlp, xyz, extra, live = label_case(N, T, K, L)
    grid = gref.Grid(3, L, 8, 15, 16, desired=512)
    assert grid.offsets == [int(o) for o in enc.offsets.tolist()]
    x01 = ((xyz.reshape(-1, 3) + 1.0) * 0.5).float()              # grid.py:156 with bound = 1, the kernel's own first step (exact but for the addition)
    feat = gref.forward(grid, x01, enc.embeddings.detach())["y"].reshape(N * T, L * 8)
    h = torch.cat([feat, extra.reshape(-1, E).double()], dim=-1)
    layers = list(mlp.net)
    for i, lin in enumerate(layers):
        h = h @ lin.weight.detach().double().t()
        if i + 1 < len(layers):
            h = torch.nn.functional.leaky_relu(h, 0.01)
    logits = h.reshape(N, T, K)
    tau = TAU_REL * max(1.0, float(logits.abs().max()))
    return dict(logits=logits, tau=tau, labels=oref.labels_from_logits(logits), margin=oref.top_two_margin(logits))


def margin_share(N, T, K, L):
    """Share of the EVALUATED samples (not on a skipped tile) that the 2 tau margin leaves out."""
    live = label_case(N, T, K, L)[4]
    ref = label_ref(N, T, K, L)
    evaluated = ~oref.skipped_tiles(live)
    return float(((ref["margin"] <= 2 * ref["tau"]) & evaluated).sum()) / float(evaluated.sum())


COMPOSITE_K = 5


@functools.lru_cache(maxsize=None)
def composite_case(T, N=1000):
    """sigmas, real_bins, geo, rays_d, labels for N rays (smaller tests take the first rays): densities with exact zeros (label 255 on half
    of those: 'not evaluated'), one sigma = inf (ray 0) and one occluder of 1e30 (ray 1, and every 7th ray) in front of labelled samples."""
    g = torch.Generator().manual_seed(4242 + T)
    sig = torch.rand(N, T, generator=g) * 8.0
    sig[torch.rand(N, T, generator=g) < 0.25] = 0.0
    rb = 0.2 + torch.cumsum(torch.rand(N, T + 1, generator=g) * (2.0 / T) + 1e-3, dim=-1)
    geo = torch.randn(N, T, 15, generator=g)
    rd = torch.randn(N, 3, generator=g)
    labels = torch.randint(0, COMPOSITE_K, (N, T), generator=g)
    sig[0, 1] = math.inf
    labels[0, 1] = 2
    sig[1::7, 1] = 1e30
    labels[1::7, 1] = 3
    skipped = (sig == 0) & (torch.rand(N, T, generator=g) < 0.5)
    skipped[:, -1] = False            # (with last_sample the last sample's y is not delta * sigma: it always counts as evaluated)
    labels[skipped] = oref.LABEL_SKIPPED
    return sig, rb, geo, rd, labels.to(torch.uint8)
