"""The per-row Philox latent draws (csrc/mfm_tasks.hpp) held against the NumPy reference tests/philox_ref.py draw for draw: the
sampler test hook, k_tn_classification and k_oprobit_sample_z. These are the only latent draws a row-sharded fit makes, and a
distribution test cannot see a wrong row key, row offset or draw index.

Every comparison: |device - reference| <= 1e-13 (|reference| + scale), scale = the magnitude of the bounds / scores the draw was
computed from (z = lo + (hi - lo) u and e = score - (score + z) carry rounding of that size). Rows whose reference path passes an
accept / reject comparison closer than 1e-11 are left out, where device libm and glibc may decide differently; at most 1 row in
10^5 may be left out, so a systematic flip cannot hide there.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from . import philox_ref as P
from .test_gpu_task_kernels import TN_CASES

pytestmark = pytest.mark.gpu

SEED = (3 << 32) + 12345  # both key words matter
DRAWS = [0, 1, (1 << 32) + 1]  # both draw words of the counter matter
ROW_OFFSETS = [0, (1 << 31) - 7, (1 << 32) - 100, (5 << 32) + 11]  # (2^32 - 100: the rows cross the fold of the key)


@pytest.fixture(scope="module")
def capi():
    from myfm_amd import _capi

    if _capi.lib().mfm_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _capi


def _assert_draws(dev, ref, margin, scale, what):
    n = ref.shape[0]
    keep = margin >= 1e-11
    n_out = int(n - keep.sum())
    assert n_out * 100_000 <= n, "%s: %d of %d rows within 1e-11 of a decision" % (what, n_out, n)
    assert np.all(np.isfinite(dev))
    err = np.abs(dev - ref)[keep]
    tol = (1e-13 * (np.abs(ref) + scale))[keep]
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, "%s: %d rows differ, first %s: device %r, reference %r" % (
        what, bad.size, np.flatnonzero(keep)[bad[:5]], dev[keep][bad[:5]], ref[keep][bad[:5]])


EDGES = [
    ("left", 8.0, None),         # far bounds, exponential proposal
    ("left", 38.0, None),
    ("right", None, -8.0),
    ("right", None, -38.0),
    ("left", -8.0, None),        # (the same magnitudes on the N(0, 1) branch: accepted at once)
    ("right", None, 38.0),
    ("right", None, 0.0),        # -left(-0.0): -0.0 < 0 is false, the exponential proposal
    ("twoside", 0.0, 1.5),       # a bound of exactly 0 on the two-sided switch
    ("twoside", -1.5, 0.0),
    ("twoside", 30.0, 30.001),   # narrow, deep in the tail
    ("twoside", -1e-3, -1e-12),  # narrow, just below 0
    ("twoside", -60.0, 60.0),    # wide: ~50 attempts per draw
]


@pytest.mark.parametrize("kind,lo,hi", TN_CASES + EDGES)
def test_sampler_hook_draw_for_draw(capi, kind, lo, hi):
    lo_, hi_ = 0.0 if lo is None else lo, 0.0 if hi is None else hi
    scale = max(1.0, abs(lo_), abs(hi_))
    for k, draw in enumerate(DRAWS):
        n = 1_000_000 if k == 0 else 200_000
        dev = capi.device_truncated_normal(kind, lo_, hi_, n, seed=SEED, draw_index=draw)
        ref, margin = P.tn_hook(kind, lo_, hi_, n, SEED, draw)
        _assert_draws(dev, ref, margin, scale, "%s(%r, %r) draw %d" % (kind, lo, hi, draw))
        if lo is not None:
            assert np.all(dev > lo)
        if hi is not None:
            assert np.all(dev < hi)


def _classification_ctx(capi, n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(n, 1))
    X = sps.csr_matrix(x)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)  # labels of both signs, independent of the score
    c = capi.Context(X, y, rank=2)
    # scores from -40 to 40: both branches of tn_left on both sides of every label
    c.set_state(0.25, np.array([40.0]), rng.normal(size=(1, 2)) * 0.1)
    c.set_w0(0.25)
    c.score_train()
    scores = c.get_e()
    assert scores.min() < -39 and scores.max() > 39
    return c, y, scores


@pytest.mark.parametrize("row_offset", ROW_OFFSETS)
def test_classification_latent_draw_for_draw(capi, row_offset):
    n = 300_000
    c, y, scores = _classification_ctx(capi, n)
    capi.lib().mfm_set_row_offset(c.h, row_offset)
    for draw in (DRAWS[0], DRAWS[2]):
        c.update_e_classification(SEED, draw)
        dev = c.get_e()
        ref, margin = P.classification_e(scores, y, SEED, draw, row_offset)
        _assert_draws(dev, ref, margin, np.abs(scores) + 1.0, "classification offset %d draw %d" % (row_offset, draw))
        z = scores - dev  # the latent value: on the side of 0 its label says
        assert np.all(np.where(y > 0, z > -1e-12, z < 1e-12))
    # consecutive draw indices: a fresh draw in every row
    c.update_e_classification(SEED, 7)
    a = c.get_e()
    c.update_e_classification(SEED, 8)
    b = c.get_e()
    assert np.all(a != b)


def _gamma(n_class):
    return np.array([0.3]) if n_class == 2 else np.linspace(-4.0, 4.0, n_class - 1)


def _oprobit_table(n, n_class, seed):
    rng = np.random.default_rng(seed)
    X = sps.csr_matrix(rng.normal(size=(n, 1)))
    y = rng.integers(0, n_class, size=n).astype(np.float64)
    scores = rng.uniform(-40.0, 40.0, size=n)
    return X, y, scores, rng


@pytest.mark.parametrize("n_class", [2, 3, 9, 33, 70])
def test_oprobit_sample_z_whole_table(capi, n_class):
    n = 100_000
    X, y, scores, _ = _oprobit_table(n, n_class, seed=n_class)
    c = capi.Context(X, y, rank=0)
    g = c.oprobit_add_group(n_class)
    gamma = _gamma(n_class)
    for k, row_offset in enumerate(ROW_OFFSETS):
        draw = DRAWS[k % len(DRAWS)]
        capi.lib().mfm_set_row_offset(c.h, row_offset)
        c.set_e(scores)
        c.oprobit_sample_z(g, gamma, SEED, draw)
        ref, margin = P.oprobit_sample_z(scores, y, None, n_class, gamma, SEED, draw, row_offset)
        _assert_draws(c.get_e(), ref, margin, np.abs(scores) + 5.0, "oprobit %d classes offset %d" % (n_class, row_offset))


@pytest.mark.parametrize("n_class", [2, 3, 9, 33, 70])
def test_oprobit_sample_z_two_groups_scattered_rows(capi, n_class):
    # two cutpoint groups on one table: a scattered third of the rows with 3 classes, the rest with n_class; the stream of a row
    # is keyed by its TABLE row, not by its position in the group's list
    n = 100_000
    X, y, scores, rng = _oprobit_table(n, n_class, seed=100 + n_class)
    rows_a = np.sort(rng.choice(n, size=n // 3, replace=False))
    rows_b = np.setdiff1d(np.arange(n), rows_a)
    y[rows_a] = rng.integers(0, 3, size=rows_a.size)
    c = capi.Context(X, y, rank=0)
    ga, gb = c.oprobit_add_group(3, rows_a), c.oprobit_add_group(n_class, rows_b)
    gam_a, gam_b = np.array([-0.5, 0.8]), _gamma(n_class)
    out_a = np.ones(n, dtype=bool)
    out_a[rows_a] = False
    for k, row_offset in enumerate(ROW_OFFSETS):
        draw = DRAWS[(k + 1) % len(DRAWS)]
        capi.lib().mfm_set_row_offset(c.h, row_offset)
        c.set_e(scores)
        c.oprobit_sample_z(ga, gam_a, SEED, draw)
        dev = c.get_e()
        assert np.array_equal(dev[out_a], scores[out_a])  # rows outside the group keep their scores, bit for bit
        ref, margin = P.oprobit_sample_z(scores, y, rows_a, 3, gam_a, SEED, draw, row_offset)
        _assert_draws(dev[rows_a], ref[rows_a], margin, np.abs(scores[rows_a]) + 5.0, "group a offset %d" % row_offset)
        c.oprobit_sample_z(gb, gam_b, SEED, draw + 1)
        dev2 = c.get_e()
        assert np.array_equal(dev2[rows_a], dev[rows_a])
        ref2, margin2 = P.oprobit_sample_z(dev, y, rows_b, n_class, gam_b, SEED, draw + 1, row_offset)
        _assert_draws(dev2[rows_b], ref2[rows_b], margin2, np.abs(scores[rows_b]) + 5.0, "group b offset %d" % row_offset)
