"""predict_proba_dist / predict_expected_dist on the device: mean, standard deviation and quantiles over the kept
samples of the ordered-probit class probabilities p_c(score_s; cutpoints_s) and of the expected class index sum_c c p_c, from
host samples and from the device store, untiled and tiled, without and with relation blocks, through the estimator, the binding
and the C ABI.

The comparisons and their tolerances are those of tests/test_gpu_predict_dist.py; they carry over because p_c and the expected
index are 0.4 C-Lipschitz in the score, the std sum has the same length, and the expected index is a sum of at most 70 positive
terms (relative error <= 2 * 70 * 2^-52 < 1e-13):
  A  against the device's own per-sample values -- class probabilities: predict_proba of a one-sample predictor; expected index:
     predict_expected_dist(quantiles=()).mean of a one-sample predictor (a mean over one sample is v * 1.0). mean bit for bit
     against predict_proba (expected: rtol 1e-13); std rtol 1e-12; quantiles at an integer position (S - 1) p bit for bit
     against np.sort(...)[h], the others rtol 1e-13 / atol 1e-15. Only for S <= 257 (one device call per sample).
  B  against tests/dist_oprobit_ref.py on the closed-form NumPy scores: rtol 1e-9, atol 1e-10 on all three outputs."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import dist_oprobit_ref as orf

pytestmark = pytest.mark.gpu

D = 12
Q5 = (0.0, 0.05, 0.5, 0.95, 1.0)
Q32 = tuple(np.linspace(0.0, 1.0, 32))


def make_predictor(n_features, K, samples, cuts):
    """MyFMOrderedProbit around a Predictor restored through __setstate__ from (w0, w, V) samples and their cutpoints: the
    host-sample path"""
    import myfm_amd
    from myfm_amd import _myfm

    fms = []
    for (w0, w, V), c in zip(samples, cuts):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((float(w0), w, V, [np.asarray(c, dtype=np.float64)]))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, n_features, int(_myfm.TaskType.ORDERED), fms))
    est = myfm_amd.MyFMOrderedProbit(K)
    est.predictor_ = p
    return est


def one_sample(fm):
    import myfm_amd
    from myfm_amd import _myfm

    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((fm.V.shape[1], fm.w.shape[0], int(_myfm.TaskType.ORDERED), [fm]))
    est = myfm_amd.MyFMOrderedProbit(fm.V.shape[1])
    est.predictor_ = p
    return est


def normal_samples(rng, n_features, K, S, scale=0.5):
    """normal w and V, w0 in 16 steps (bounded, so that S = 4096 samples stay within reach of the cutpoints)"""
    return [(0.1 * (s % 16) - 0.3, rng.normal(size=n_features) * scale, rng.normal(size=(n_features, K)) * scale) for s in range(S)]


def design(kind, N, rng):
    if N == 0:
        return sps.csr_matrix((0, D))
    if kind == "ell":  # one-hot rows, unit values, equal length
        rows = np.repeat(np.arange(N), 2)
        cols = np.stack([rng.integers(0, 6, size=N), 6 + rng.integers(0, 6, size=N)], axis=1).reshape(-1)
        return sps.csr_matrix((np.ones(2 * N), (rows, cols)), shape=(N, D))
    dense = np.zeros((N, D))
    for t in range(N):
        n = int(rng.integers(0, 5)) if kind == "ragged" else int(rng.integers(1, 6))
        if kind == "ragged" and t % 5 == 1:
            n = 0  # empty rows
        cols = rng.choice(D, size=n, replace=False)
        dense[t, cols] = 1.0 if kind == "ragged" else rng.choice([1.0, -1.0, 2.0, -2.0, 0.5], size=n)
    return sps.csr_matrix(dense)


def device_values(est, X, rels, expected):
    """per-sample values as the device computes them: (S, N, C) class probabilities, or (S, N) expected indices"""
    out = []
    for fm in est.predictor_.samples:
        one = one_sample(fm)
        out.append(np.asarray(one.predict_expected_dist(X, rels, quantiles=()).mean if expected else one.predict_proba(X, rels)))
    return np.stack(out)


def check_A(got, vals, quantiles, expect_mean, expected):
    S = vals.shape[0]
    if expected:
        np.testing.assert_allclose(got.mean, expect_mean, rtol=1e-13, atol=0)
    else:
        assert np.array_equal(got.mean, expect_mean)
    np.testing.assert_allclose(got.std, vals.std(axis=0), rtol=1e-12, atol=0)
    srt = np.sort(vals, axis=0)
    assert got.quantiles.shape == (len(quantiles),) + vals.shape[1:]
    for i, p in enumerate(quantiles):
        h = (S - 1) * p
        if h == np.floor(h):
            assert np.array_equal(got.quantiles[i], srt[int(h)]), p
        else:
            np.testing.assert_allclose(got.quantiles[i], np.quantile(vals, p, axis=0), rtol=1e-13, atol=1e-15)


def check_B(got, samples, cuts, X_flat, quantiles, expected):
    p = orf.class_probs(orf.sample_scores(samples, X_flat), cuts)
    mean, std, qs = orf.summary(orf.expected_index(p) if expected else p, quantiles)
    for a, b in ((got.mean, mean), (got.std, std), (got.quantiles, qs)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-10)


def both(est, X, rels=(), quantiles=Q5):
    """(expected flag, summary) of the two methods"""
    return [(False, est.predict_proba_dist(X, list(rels), quantiles=quantiles)),
            (True, est.predict_expected_dist(X, list(rels), quantiles=quantiles))]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. host samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,S,C,kind,quantiles", [
    (0, 257, 1, 2, "ell", Q5),
    (1, 7, 2, 3, "ragged", Q5),
    (3, 257, 63, 5, "values", Q32),
    (8, 1, 64, 5, "ell", Q5),
    (33, 257, 65, 33, "ragged", Q5),
    (3, 7, 257, 70, "values", Q5),
    (3, 7, 4096, 5, "ell", Q5),
    (8, 0, 2, 5, "ragged", Q5),
    (1, 257, 64, 5, "values", ()),
])
def test_host_samples(K, N, S, C, kind, quantiles):
    """N = 257 and 7: a partial last workgroup at 32 rows per workgroup and at fewer; ell / ragged / values: the three row forms of
    the score pass; C = 33 crosses the class limit of predict_proba's one-pass form; S = 63, 64, 65 straddle a power of two;
    S = 257 (and the expected index of C = 33 at S = 65) reads the cutpoints from global memory, the smaller cases from LDS; at S = 4096 one row is all the LDS of
    a workgroup; quantiles = (): the direct form."""
    from myfm_amd.estimators import PredictiveSummary

    rng = np.random.default_rng(1000 * K + 10 * N + S)
    X = design(kind, N, rng)
    samples = normal_samples(rng, D, K, S)
    cuts = orf.sample_cutpoints(rng, S, C - 1)
    est = make_predictor(D, K, samples, cuts)
    proba = est.predict_proba(X)
    assert proba.shape == (N, C)
    for expected, got in both(est, X, quantiles=quantiles):
        tail = () if expected else (C,)
        assert isinstance(got, PredictiveSummary)
        assert got.mean.shape == (N,) + tail and got.std.shape == (N,) + tail and got.quantiles.shape == (len(quantiles), N) + tail
        if not expected:
            assert np.array_equal(got.mean, proba)
        if N == 0:
            continue
        check_B(got, samples, cuts, X, quantiles, expected)
        if S <= 257:
            vals = device_values(est, X, [], expected)
            check_A(got, vals, quantiles, vals.sum(axis=0) * (1.0 / S) if expected else proba, expected)
            if expected:
                np.testing.assert_allclose(got.mean, proba @ np.arange(C), rtol=1e-13, atol=0)
        if S == 1:
            assert np.all(got.std == 0.0)
        assert np.all(got.mean >= 0.0) and np.all(got.quantiles >= 0.0)
        again = (est.predict_expected_dist if expected else est.predict_proba_dist)(X, quantiles=quantiles)
        assert same(got, again)  # no atomics: a rerun is bit-identical


# ---- 2. tiling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expected", [False, True])
def test_tiles_and_chunks_do_not_change_a_bit(expected):
    """257 rows in tiles of 100 (two full ones and 57 rows), 65 samples in chunks of 7"""
    rng = np.random.default_rng(21)
    X = design("values", 257, rng)
    est = make_predictor(D, 3, normal_samples(rng, D, 3, 65), orf.sample_cutpoints(rng, 65, 4))
    p = est.predictor_
    q = np.array(Q5)
    base = p.predict_dist_oprobit(X, [], q, 0, expected)
    assert base[2].shape == ((5, 257) if expected else (5, 257, 5))
    tiled = p.predict_dist_oprobit(X, [], q, 0, expected, tile_rows=100, chunk_samples=7)
    assert same(base, tiled)
    assert same(base, (est.predict_expected_dist if expected else est.predict_proba_dist)(X, quantiles=Q5))
    direct = p.predict_dist_oprobit(X, [], np.array([]), 0, expected)  # the moments of the direct form are those of the LDS form
    direct_tiled = p.predict_dist_oprobit(X, [], np.array([]), 0, expected, tile_rows=100, chunk_samples=7)
    assert same(direct, direct_tiled)
    assert np.array_equal(direct[0], base[0]) and np.array_equal(direct[1], base[1])
    if not expected:
        assert np.array_equal(base[0], est.predict_proba(X))


# ---- 3. ties and saturation ----------------------------------------------------------------------------------------------------
def test_ties():
    rng = np.random.default_rng(31)
    X = design("values", 65, rng)
    sample = normal_samples(rng, D, 3, 1)[0]
    cut = orf.sample_cutpoints(rng, 1, 4)[0]
    est = make_predictor(D, 3, [sample] * 64, [cut] * 64)
    for expected, got in both(est, X):
        v = device_values(one_sample(est.predictor_.samples[0]), X, [], expected)[0]
        assert np.all(got.std == 0.0)
        assert all(np.array_equal(row, v) for row in got.quantiles)
        if not expected:
            assert np.array_equal(got.mean, est.predict_proba(X))


def test_saturation():
    """cutpoints more than 9 above every score: erf(> 9 / sqrt 2) is exactly 1, so p_0 = 1 and every other class is exactly 0"""
    rng = np.random.default_rng(32)
    X = design("values", 65, rng)
    samples = normal_samples(rng, D, 3, 7)
    top = np.abs(orf.sample_scores(samples, X)).max()
    cuts = top + 9.5 + np.sort(rng.random(size=(7, 4)), axis=1)
    est = make_predictor(D, 3, samples, cuts)
    (_, pr), (_, ex) = both(est, X)
    assert np.all(pr.mean[:, 0] == 1.0) and np.all(pr.mean[:, 1:] == 0.0)
    assert np.all(pr.std == 0.0)
    assert np.all(pr.quantiles[:, :, 0] == 1.0) and np.all(pr.quantiles[:, :, 1:] == 0.0)
    assert np.all(ex.mean == 0.0) and np.all(ex.std == 0.0) and np.all(ex.quantiles == 0.0)
    assert not np.any(np.signbit(pr.mean)) and not np.any(np.signbit(pr.quantiles)) and not np.any(np.signbit(ex.quantiles))
    assert np.array_equal(pr.mean, est.predict_proba(X))


# ---- 4. relation blocks --------------------------------------------------------------------------------------------------------
def _block_cases():
    from myfm_amd.utils.synthetic import block_design

    main, X_flat, blocks, _, _ = block_design()
    yield "block_design", main, blocks
    rng = np.random.default_rng(41)
    N = 37
    main2 = sps.csr_matrix(np.round(rng.normal(size=(N, 4)), 2) * (rng.random((N, 4)) < 0.5))
    b0 = sps.csr_matrix(np.round(rng.normal(size=(3, 5)), 2))
    b1 = sps.csr_matrix(np.eye(4)[:, :3] + 0.5 * (rng.random((4, 3)) < 0.3))
    yield "all_rows_at_block_row_0", main2, [(np.zeros(N, dtype=np.int64), b0), (rng.integers(0, 4, size=N).astype(np.int64), b1)]


@pytest.mark.parametrize("S", [2, 65])
@pytest.mark.parametrize("case", [0, 1])
def test_relation_blocks(case, S):
    import myfm_amd

    name, main, blocks = list(_block_cases())[case]
    X_flat = orf.expand(main, blocks)
    rels = [myfm_amd.RelationBlock(idx, B) for idx, B in blocks]
    rng = np.random.default_rng(40 + S)
    samples = normal_samples(rng, X_flat.shape[1], 3, S)
    cuts = orf.sample_cutpoints(rng, S, 4)
    est = make_predictor(X_flat.shape[1], 3, samples, cuts)
    proba, proba_flat = est.predict_proba(main, rels), est.predict_proba(X_flat)
    for (expected, got), (_, flat) in zip(both(est, main, rels), both(est, X_flat)):
        check_B(got, samples, cuts, X_flat, Q5, expected)
        # the exact parts of A hold for each call against its own path's per-sample values ...
        vals = device_values(est, main, rels, expected)
        check_A(got, vals, Q5, vals.sum(axis=0) * (1.0 / S) if expected else proba, expected)
        vals_flat = device_values(est, X_flat, [], expected)
        check_A(flat, vals_flat, Q5, vals_flat.sum(axis=0) * (1.0 / S) if expected else proba_flat, expected)
        # ... and across the two calls, whose scores differ in the last bit, A's floating-point tolerances
        np.testing.assert_allclose(got.std, flat.std, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(got.mean, flat.mean, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(got.quantiles, flat.quantiles, rtol=1e-13, atol=1e-15)


# ---- 5. device store -----------------------------------------------------------------------------------------------------------
def test_store_path():
    import myfm_amd

    rng = np.random.default_rng(51)
    n_users, n_items, n = 20, 15, 300
    users, items = rng.integers(0, n_users, size=n), rng.integers(0, n_items, size=n)
    X = sps.csr_matrix((np.ones(2 * n), (np.repeat(np.arange(n), 2), np.stack([users, n_users + items], axis=1).reshape(-1))),
                       shape=(n, n_users + n_items))
    bu, bi = rng.normal(size=n_users), rng.normal(size=n_items)
    y = np.clip(np.round(2.0 + bu[users] + bi[items] + 0.5 * rng.normal(size=n)), 0, 4).astype(np.int64)
    y[:5] = np.arange(5)  # every class occurs
    est = myfm_amd.MyFMOrderedProbit(rank=4).fit(X, y, n_iter=40, n_kept_samples=30)
    assert est.predictor_.resident and len(est.predictor_.samples) == 30
    restored = pickle.loads(pickle.dumps(est))
    assert not restored.predictor_.resident  # host samples
    proba = est.predict_proba(X)
    assert proba.shape == (n, 5)
    for (expected, got), (_, back) in zip(both(est, X), both(restored, X)):
        assert same(got, back)
        if not expected:
            assert np.array_equal(got.mean, proba)
    # the expected index of the pair rows is what predict_pairs scores (another, equivalent expression: sum_j Phi(score - cut_j))
    Xq = sps.csr_matrix((np.ones(n_users), (np.arange(n_users), np.arange(n_users))), shape=(n_users, n_users + n_items))
    Xc = sps.csr_matrix((np.ones(n_items), (np.arange(n_items), n_users + np.arange(n_items))), shape=(n_items, n_users + n_items))
    uu, ii = np.divmod(np.arange(n_users * n_items), n_items)
    rows = (Xq[uu] + Xc[ii]).tocsr()
    pairs = est.predict_pairs(Xq, Xc)
    np.testing.assert_allclose(est.predict_expected_dist(rows).mean.reshape(n_users, n_items), pairs, rtol=1e-12, atol=1e-12)


# ---- 6. the C ABI through ctypes -----------------------------------------------------------------------------------------------
def test_c_abi():
    from myfm_amd import _capi

    K, N, S, C = 3, 257, 63, 5
    rng = np.random.default_rng(1000 * K + 10 * N + S)
    X = design("values", N, rng)
    samples = normal_samples(rng, D, K, S)
    cuts = orf.sample_cutpoints(rng, S, C - 1)
    est = make_predictor(D, K, samples, cuts)
    dsg = _capi.Design(X)
    store = _capi.Store(D, K)
    for w0, w, V in samples:
        store.push(w0, w, V)
    for expected in (False, True):
        want = est.predictor_.predict_dist_oprobit(X, [], np.array(Q32), 0, expected)
        assert same(want, dsg.summary_oprobit(samples, cuts, expected, Q32))
        assert same(want, store.summary_oprobit(dsg, cuts, expected, Q32))
        bad = cuts.copy()
        bad[S // 2] = bad[S // 2][::-1]
        nan = cuts.copy()
        nan[S - 1, 2] = np.nan
        for refused in (np.empty((S, 0)), bad, nan):
            with pytest.raises(ValueError):  # MFM_ERR_INVALID
                dsg.summary_oprobit(samples, refused, expected, Q5)
            with pytest.raises(ValueError):
                store.summary_oprobit(dsg, refused, expected, Q5)
    store.close()
    dsg.close()
