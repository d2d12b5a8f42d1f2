"""numpy restatement of the generator behind sn_rm_jitter_tables (csrc/jitter.hip): Philox4x32-10 (Salmon, Moraes, Dror, Shaw,
"Parallel random numbers: as easy as 1, 2, 3", SC'11) and the counter layout of the jitter tables.

    element (stage k, global ray g = ray_base + n, column j):
        w       = philox4x32_10(counter = (g, (k << 24) | (j >> 2), draw_lo, draw_hi), key = (seed_lo, seed_hi))[j & 3]
        uniform = float32(w >> 8) * 2^-24
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                     # 32 x 32 -> 64: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def table_words(seed: int, draw: int, k: int, ray_base: int, N: int, T1: int) -> np.ndarray:
    """The 32-bit words behind rows ray_base .. ray_base + N - 1 of stage k's table: uint32 [N, T1]."""
    seed, draw = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF
    G = (T1 + 3) // 4
    g = (np.arange(N, dtype=np.uint64) + np.uint64(ray_base))[:, None]
    assert int(ray_base) + N <= 1 << 32 and T1 <= 1 << 26 and 0 <= k < 4
    q = np.arange(G, dtype=np.uint64)[None, :] | np.uint64(k << 24)
    out = philox4x32_10((g, q, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1).reshape(N, 4 * G)[:, :T1]


def table_uniforms(seed: int, draw: int, k: int, ray_base: int, N: int, T1: int) -> np.ndarray:
    """float32 [N, T1] in [0, 1): 24 bits each, exact."""
    return (table_words(seed, draw, k, ray_base, N, T1) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
