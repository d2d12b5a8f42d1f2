"""CPU: the numpy restatement of the jitter tables' generator (tests/philox_ref.py) against Random123's known answers, the statistical
conditions its counter layout has to meet, its chunk invariance -- and the host checks of sn_rm_jitter_tables, which answer before any
launch (there is no GPU here).  tests/test_gpu_jitter.py holds the kernel to this restatement bit for bit."""
import ctypes

import numpy as np
import pytest

import philox_ref as pr

# Random123's kat_vectors for philox4x32, 10 rounds: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox4x32_10_known_answers(counter, key, want):
    got = pr.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want


def test_philox_is_vectorised_over_counters():
    """An array of counters gives what the counters give one by one (the tables are computed as arrays)."""
    cs = np.array([k[0] for k in KAT], dtype=np.uint64).T
    for key in ((0, 0), (0xa4093822, 0x299f31d0)):
        got = np.stack(pr.philox4x32_10(tuple(cs), key), axis=-1)
        for i, (counter, _, _) in enumerate(KAT):
            assert got[i].tolist() == [int(x) for x in pr.philox4x32_10(counter, key)]


CASES = [(1234, 0, 1, 4096, 33), (1234, 0, 0, 4096, 129), (0x9E3779B97F4A7C15, 1 << 32, 2, 4096, 9), (1234, 1, 3, 257, 7)]


@pytest.mark.parametrize("seed,draw,k,N,T1", CASES)
def test_table_uniforms_meet_the_conditions_on_the_layout(seed, draw, k, N, T1):
    """Over the flattened table: |z| of the mean <= 4, 16-bin chi^2(15) <= 37.7 (the 0.1 % point), lag-1 correlation * sqrt(n) <= 4,
    every value in [0, 1)."""
    u = pr.table_uniforms(seed, draw, k, 0, N, T1)
    assert u.dtype == np.float32 and u.shape == (N, T1)
    x = u.astype(np.float64).ravel()
    n = x.size
    assert x.min() >= 0.0 and x.max() < 1.0
    z = (x.mean() - 0.5) / np.sqrt(1.0 / 12.0 / n)
    counts = np.bincount((x * 16).astype(np.int64), minlength=16)
    chi2 = float(((counts - n / 16.0) ** 2 / (n / 16.0)).sum())
    d = x - x.mean()
    lag = float((d[:-1] * d[1:]).sum() / (d * d).sum() * np.sqrt(n))
    print(f"seed={seed:#x} draw={draw} k={k} N={N} T1={T1}: z={z:+.2f} chi2={chi2:.1f} lag1*sqrt(n)={lag:+.2f}")
    assert abs(z) <= 4.0
    assert chi2 <= 37.7
    assert abs(lag) <= 4.0


def test_tables_differ_between_stages_draws_seeds_and_rays():
    base = pr.table_words(1234, 0, 1, 0, 64, 9)
    for other in (pr.table_words(1234, 0, 2, 0, 64, 9), pr.table_words(1234, 1, 1, 0, 64, 9), pr.table_words(1235, 0, 1, 0, 64, 9),
                  pr.table_words(1234, 1 << 32, 1, 0, 64, 9), pr.table_words(1234 + (1 << 32), 0, 1, 0, 64, 9), pr.table_words(1234, 0, 1, 64, 64, 9)):
        assert (base != other).mean() > 0.99
    assert len(np.unique(base)) == base.size                          # no two elements of a table share a (counter, lane)


def test_restatement_is_chunk_invariant():
    """257 rows at once = chunks of 100 + 157 with ray_base = 100; and a row does not depend on the row length's neighbours."""
    for k, T1 in ((0, 4), (1, 33), (2, 6), (3, 7)):
        whole = pr.table_uniforms(99, 7, k, 0, 257, T1)
        parts = np.concatenate([pr.table_uniforms(99, 7, k, 0, 100, T1), pr.table_uniforms(99, 7, k, 100, 157, T1)])
        assert np.array_equal(whole, parts)
    top = pr.table_uniforms(99, 7, 1, (1 << 32) - 257, 257, 5)        # the last rays of the 32-bit ray counter
    assert np.array_equal(top[-1:], pr.table_uniforms(99, 7, 1, (1 << 32) - 1, 1, 5))


def test_jitter_tables_entry_point_validates_its_arguments():
    """sn_rm_jitter_tables answers bad arguments with SN_ERR_INVALID before any launch; N == 0 is SN_OK; the ABI version stays 12."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    assert l.sn_abi_version() == 12 == _lib.ABI_VERSION and "sn_rm_jitter_tables" in _lib.EXPORTED_SYMBOLS
    INVALID = -1
    dummy = ctypes.c_void_p(64)
    steps = (ctypes.c_uint32 * 5)(128, 64, 32, 16, 8)
    u = (ctypes.c_void_p * 4)(None, 64, 64, 64)
    f = l.sn_rm_jitter_tables
    assert f(None, 4, 0, 3, steps, dummy, u, 1, None) == INVALID and b"NULL state" in l.sn_last_error()
    assert f(ctypes.c_void_p(72), 4, 0, 3, steps, dummy, u, 1, None) == INVALID and b"16-byte" in l.sn_last_error()
    assert f(dummy, 4, 0, 0, steps, dummy, u, 1, None) == INVALID and b"num_stages" in l.sn_last_error()
    assert f(dummy, 4, 0, 5, steps, dummy, u, 1, None) == INVALID and b"num_stages" in l.sn_last_error()
    assert f(dummy, 4, 0, 3, None, dummy, u, 1, None) == INVALID
    for bad in (1 << 26, (1 << 32) - 1, 0):                            # num_steps + 1 <= 2^26 (the column counter has 24 + 2 bits); and >= 1
        over = (ctypes.c_uint32 * 3)(128, bad, 32)
        assert f(dummy, 4, 0, 3, over, dummy, u, 1, None) == INVALID and b"num_steps[1]" in l.sn_last_error()
        assert f(dummy, 4, 0, 3, over, None, None, 0, None) == INVALID      # ... whether or not the stage's table is asked for
    assert f(dummy, 2, (1 << 32) - 1, 3, steps, dummy, u, 1, None) == INVALID and b"ray_base" in l.sn_last_error()
    assert f(dummy, (1 << 32) - 1, 2, 3, steps, dummy, u, 1, None) == INVALID and b"ray_base" in l.sn_last_error()
    assert f(dummy, 4, 0, 3, steps, ctypes.c_void_p(66), u, 1, None) == INVALID and b"4-byte" in l.sn_last_error()
    assert f(dummy, 0, 0, 3, steps, dummy, u, 1, None) == 0
    assert f(None, 0, 0, 0, None, None, None, 0, None) == 0
    assert f(dummy, 4, 0, 3, steps, None, None, 0, None) == 0          # no table, no advance: nothing to launch
