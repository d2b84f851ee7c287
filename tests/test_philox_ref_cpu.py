"""The NumPy reference of the per-row Philox latent draws (tests/philox_ref.py) on its own, without a GPU: the Random123
known-answer vectors of philox4x32-10, the uniforms, and the samplers' laws against scipy's truncated normal. (The device kernels
are held against this reference draw for draw in tests/test_gpu_philox_latent.py.)"""
import numpy as np
import pytest
from scipy import stats

from . import philox_ref as P


# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = P.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want
    # the same vector as one lane of an array of otherwise different counters
    c = [np.array([ctr[i], 1, 2], dtype=np.uint64) for i in range(4)]
    got = P.philox4x32_10(*c, *key)
    assert tuple(int(v[0]) for v in got) == want


def test_row_key_and_counter_words():
    # the key folds the high word of the global row into the seed; the counter carries (row, n, draw lo, draw hi)
    seed, draw = (5 << 32) + 77, (3 << 32) + 9
    rows = np.array([7, (1 << 32) + 7, (2 << 32) + 7], dtype=np.int64)
    g = P.RowRng(seed, draw, rows)
    for i, r in enumerate(rows):
        s = (seed ^ ((int(r) >> 32) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
        assert (int(g.k0[i]), int(g.k1[i]), int(g.row[i])) == (s & 0xFFFFFFFF, s >> 32, 7)
        x = P.philox4x32_10(7, 4, draw & 0xFFFFFFFF, draw >> 32, s & 0xFFFFFFFF, s >> 32)
        a, b = g.next2(4, np.array([i]))
        assert a[0] == ((int(x[0]) << 21 | int(x[1]) >> 11) + 0.5) / 2.0 ** 53
        assert b[0] == ((int(x[2]) << 21 | int(x[3]) >> 11) + 0.5) / 2.0 ** 53
    # same low word, different high word: different streams
    u = g.next2(0)[0]
    assert len(set(u.tolist())) == 3


def test_uniforms_in_open_interval():
    g = P.RowRng((1 << 40) + 3, (1 << 32) + 1, np.arange(1 << 18, dtype=np.int64))
    for n in range(4):
        a, b = g.next2(n)
        for u in (a, b):
            assert np.all(u > 0) and np.all(u < 1)
            assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
    # the ends of the map: 0.5 / 2^53 at the bottom; at the top (2^53 - 1) + 0.5 rounds to even, i.e. to 2^53, so the one largest
    # of the 2^53 words gives exactly 1.0 (probability 2^-53; the samplers then meet r = 0 or z = mu, both finite)
    assert P.to_uniform(0, 0) == 2.0 ** -54
    assert P.to_uniform(0xFFFFFFFF, 0xFFFFF7FF) < 1.0
    assert P.to_uniform(0xFFFFFFFF, 0xFFFFFFFF) == 1.0


def test_sincospi_reduction():
    u = np.concatenate([np.linspace(0, 1, 4097)[1:-1], np.random.default_rng(0).random(10000)])
    s, c = P.sincospi2(u)
    np.testing.assert_allclose(s, np.sin(2 * np.pi * u), rtol=0, atol=4e-15)
    np.testing.assert_allclose(c, np.cos(2 * np.pi * u), rtol=0, atol=4e-15)
    # exact at the quadrant points
    s, c = P.sincospi2(np.array([0.25, 0.5, 0.75]))
    assert s.tolist() == [1.0, 0.0, -1.0] and c.tolist() == [0.0, -1.0, 0.0]


# util.hpp:15-60: every branch of the three samplers
BRANCHES = [
    ("left", -1.3, None),
    ("left", 0.0, None),
    ("left", 2.5, None),
    ("left", 8.0, None),
    ("right", None, 0.7),
    ("right", None, -1.8),
    ("twoside", -0.8, 1.1),
    ("twoside", -3.0, -1.2),
    ("twoside", 0.9, 2.4),
    ("twoside", 30.0, 30.001),
]


@pytest.mark.parametrize("kind,lo,hi", BRANCHES)
def test_reference_samplers_follow_truncated_normal(kind, lo, hi):
    n = 200_000
    z, margin = P.tn_hook(kind, 0.0 if lo is None else lo, 0.0 if hi is None else hi, n, seed=(7 << 32) + 1, draw=2)
    a = -np.inf if lo is None else lo
    b = np.inf if hi is None else hi
    assert np.all(z > a) and np.all(z < b)
    assert np.all(margin > 0)
    dist = stats.truncnorm(a, b)
    # P(sqrt(n) D > 2.2) ~ 1e-4
    assert stats.kstest(z, dist.cdf).statistic < 2.2 / np.sqrt(n)
    assert abs(z.mean() - dist.mean()) < 5 * dist.std() / np.sqrt(n)


def test_fallback_after_max_tries():
    # the device gives up after TN_MAX_TRIES attempts; the reference mirrors the fall-back values (shown with a small cap)
    g = P.RowRng(3, 0, np.arange(20000, dtype=np.int64))
    z, _ = P.tn_twoside(g, 40.0, 100.0, max_tries=1)
    assert np.mean(z == 70.0) > 0.9 and np.all((z == 70.0) | ((z > 40) & (z < 100)))
    z, _ = P.tn_left(g, 5.0, max_tries=1)
    assert np.any(z == 5.0) and np.all(z >= 5.0)
    z, _ = P.tn_left(g, -0.5, max_tries=1)  # two candidates per attempt: both rejected with probability Phi(-0.5)^2
    assert np.any(z == 0.0) and np.all((z == 0.0) | (z > -0.5))
    z2, _ = P.tn_right(g, 0.5, max_tries=1)
    np.testing.assert_array_equal(z2, -z)
