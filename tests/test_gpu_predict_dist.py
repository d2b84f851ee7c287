"""predict_dist on the device: mean, standard deviation and quantiles over the kept samples, with and without
the noise mixture, from host samples and from the device store, untiled and tiled, without and with relation blocks.

The comparisons:
  A  against the per-sample values taken from the device (FM.predict_score, the scorer the predictors sum): mean bit for bit
     against predict() / predict_proba(); std rtol 1e-12 (a two-pass sum of S <= 4096 squares carries S 2^-53); quantiles at an
     integer position (S - 1) p bit for bit against np.sort(...)[h], the others rtol 1e-13 / atol 1e-15 (one interpolation).
  B  against the closed-form NumPy scores: atol 1e-10 with rtol 1e-9 on all three outputs (the summaries are 1-Lipschitz in the
     sup norm of the per-sample values; the project's bound for scores).
  C  mixture quantiles: |F(q) - p| <= 1e-12 with F evaluated in NumPy on the device's scores, and |q - q_brentq| <= 1e-9 max(1, |q|)."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import dist_ref as dr

pytestmark = pytest.mark.gpu

D = 12
Q5 = (0.0, 0.05, 0.5, 0.95, 1.0)
Q32 = tuple(np.linspace(0.0, 1.0, 32))


def make_predictor(task, n_features, K, samples):
    """an estimator around a Predictor restored through __setstate__ from (w0, w, V) samples: the host-sample path"""
    import myfm_amd
    from myfm_amd import _myfm

    fms = []
    for w0, w, V in samples:
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((float(w0), w, V, []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, n_features, int(task), fms))
    est = (myfm_amd.MyFMClassifier if task == _myfm.TaskType.CLASSIFICATION else myfm_amd.MyFMRegressor)(K)
    est.predictor_ = p
    return est


def normal_samples(rng, n_features, K, S, scale=0.5):
    """normal w and V, distinct w0"""
    return [(0.1 * s - 0.3, rng.normal(size=n_features) * scale, rng.normal(size=(n_features, K)) * scale) for s in range(S)]


def task_of(mode):
    from myfm_amd import _myfm

    return _myfm.TaskType.CLASSIFICATION if mode else _myfm.TaskType.REGRESSION


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


def device_values(est, X, rels, mode):
    """(S, N) per-sample values as the device computes them: FM.predict_score for a regressor; for a classifier the one-sample
    predictor's predict, Phi(score) * (1 / 1)"""
    from myfm_amd import _myfm

    p = est.predictor_
    if not mode:
        return np.stack([np.asarray(fm.predict_score(X, rels)) for fm in p.samples])
    out = []
    for fm in p.samples:
        one = _myfm.Predictor.__new__(_myfm.Predictor)
        one.__setstate__((fm.V.shape[1], fm.w.shape[0], int(_myfm.TaskType.CLASSIFICATION), [fm]))
        out.append(np.asarray(one.predict(X, rels)))
    return np.stack(out)


def check_A(got, vals, quantiles, expect_mean):
    S = vals.shape[0]
    assert np.array_equal(got.mean, expect_mean)
    np.testing.assert_allclose(got.std, vals.std(axis=0), rtol=1e-12, atol=0)
    srt = np.sort(vals, axis=0)
    assert got.quantiles.shape == (len(quantiles), vals.shape[1])
    for i, p in enumerate(quantiles):
        h = (S - 1) * p
        if h == np.floor(h):
            assert np.array_equal(got.quantiles[i], srt[int(h)]), p
        else:
            np.testing.assert_allclose(got.quantiles[i], np.quantile(vals, p, axis=0), rtol=1e-13, atol=1e-15)


def check_B(got, samples, X_flat, mode, quantiles):
    mean, std, qs = dr.summary(dr.values(dr.sample_scores(samples, X_flat), mode), quantiles)
    for a, b in ((got.mean, mean), (got.std, std), (got.quantiles, qs)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-10)


# ---- 1. host samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,S,kind,mode,quantiles", [
    (0, 257, 1, "ell", 0, Q5),
    (1, 7, 2, "ragged", 1, Q5),
    (3, 257, 63, "values", 0, Q32),
    (8, 1, 64, "ell", 1, Q5),
    (33, 257, 65, "ragged", 0, Q5),
    (3, 257, 95, "values", 1, Q5),
    (8, 7, 257, "ragged", 0, Q32),
    (3, 7, 4096, "ell", 0, Q5),
    (33, 7, 4096, "values", 1, Q32),
    (8, 0, 2, "ragged", 1, Q5),
    (0, 0, 4096, "values", 0, Q5),
    (1, 257, 64, "values", 0, ()),
])
def test_host_samples(K, N, S, kind, mode, quantiles):
    from myfm_amd.estimators import PredictiveSummary

    rng = np.random.default_rng(1000 * K + 10 * N + S)
    X = design(kind, N, rng)
    samples = normal_samples(rng, D, K, S)
    est = make_predictor(task_of(mode), D, K, samples)
    got = est.predict_dist(X, quantiles=quantiles)
    assert isinstance(got, PredictiveSummary)
    assert got.mean.shape == (N,) and got.std.shape == (N,) and got.quantiles.shape == (len(quantiles), N)
    expect_mean = est.predict_proba(X) if mode else est.predict(X)
    assert np.array_equal(got.mean, expect_mean)
    if N == 0:
        return
    check_B(got, samples, X, mode, quantiles)
    if S <= 257 or mode == 0:  # (one device call per sample: at the cap of 4096 samples for the regressor only)
        check_A(got, device_values(est, X, [], mode), quantiles, expect_mean)
    if S == 1:
        assert np.all(got.std == 0.0)
    again = est.predict_dist(X, quantiles=quantiles)  # no atomics: a rerun is bit-identical
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ---- 2. tiling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,noise,block", [
    pytest.param(0, False, False, id="0-False"), pytest.param(1, False, False, id="1-False"), pytest.param(0, True, False, id="0-True"),
    pytest.param(0, False, True, id="0-False-block")])
def test_tiles_and_chunks_do_not_change_a_bit(mode, noise, block):
    """257 rows in tiles of 64 (four full ones and a single row), 7 samples in chunks of 3, 3 and 1; block: the relation-block
    design of section 4 at 257 rows, whose tiles go through the per-sample pass"""
    rng = np.random.default_rng(21 + mode)
    if not block:
        X, rels, n_features = design("values", 257, rng), [], D
    else:
        import myfm_amd
        from myfm_amd.utils.synthetic import block_design

        X, X_flat, blocks, _, _ = block_design(257)
        rels, n_features = [myfm_amd.RelationBlock(idx, B) for idx, B in blocks], X_flat.shape[1]
    est = make_predictor(task_of(mode), n_features, 3, normal_samples(rng, n_features, 3, 7))
    q = np.array([0.05, 0.5, 0.77, 0.95]) if noise else np.array(Q5)
    prec = np.geomspace(0.25, 400.0, 7) if noise else None
    p = est.predictor_
    base = p.predict_dist(X, rels, q, prec)
    for kw in ({"tile_rows": 64}, {"chunk_samples": 3}, {"tile_rows": 64, "chunk_samples": 3}, {"tile_rows": 1000, "chunk_samples": 50}):
        got = p.predict_dist(X, rels, q, prec, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(base, got)), kw
    assert np.array_equal(base[0], est.predict_proba(X, rels) if mode else est.predict(X, rels))


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_ties(mode):
    rng = np.random.default_rng(31)
    X = design("values", 65, rng)
    a, b = normal_samples(rng, D, 3, 2)
    same = make_predictor(task_of(mode), D, 3, [a] * 5)
    vals = device_values(same, X, [], mode)
    got = same.predict_dist(X, quantiles=Q5)
    assert np.all(got.std == 0.0)
    assert all(np.array_equal(row, vals[0]) for row in got.quantiles)
    two = make_predictor(task_of(mode), D, 3, [a, b, a, a, b])
    vals = device_values(two, X, [], mode)
    q = (0.0, 0.25, 0.5, 0.75, 1.0, 0.6, 0.3)
    got = two.predict_dist(X, quantiles=q)
    check_A(got, vals, q, two.predict_proba(X) if mode else two.predict(X))
    lo, hi = np.minimum(vals[0], vals[1]), np.maximum(vals[0], vals[1])
    assert np.all((got.quantiles >= lo) & (got.quantiles <= hi))


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


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S", [2, 65])
@pytest.mark.parametrize("case", [0, 1])
def test_relation_blocks(case, S, mode):
    import myfm_amd

    name, main, blocks = list(_block_cases())[case]
    X_flat = dr.expand(main, blocks)
    rels = [myfm_amd.RelationBlock(idx, B) for idx, B in blocks]
    rng = np.random.default_rng(40 + S)
    samples = normal_samples(rng, X_flat.shape[1], 3, S)
    est = make_predictor(task_of(mode), X_flat.shape[1], 3, samples)
    got = est.predict_dist(main, rels, quantiles=Q5)
    check_B(got, samples, X_flat, mode, Q5)
    check_A(got, device_values(est, main, rels, mode), Q5, est.predict_proba(main, rels) if mode else est.predict(main, rels))
    flat = est.predict_dist(X_flat, quantiles=Q5)
    # The block scorer adds a block row's cached partial sums where the flat scorer adds term by term, so the two designs' scores
    # differ in the last bit (4.4e-16 seen at |score| ~ 1) and the summaries of the two calls cannot agree bit for bit. The
    # exact parts of comparison A hold against the block path's own scores (above) and the flat path's own scores (here); across
    # the two calls the floating-point tolerances of A apply: std rtol 1e-12, mean and quantiles rtol 1e-13 / atol 1e-15, and the
    # same atol for std (all three are 1-Lipschitz in the sup norm of the values, which differ by a few 2^-52 here).
    check_A(flat, device_values(est, X_flat, [], mode), Q5, est.predict_proba(X_flat) if mode else est.predict(X_flat))
    np.testing.assert_allclose(got.std, flat.std, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got.mean, flat.mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(got.quantiles, flat.quantiles, rtol=1e-13, atol=1e-15)


# ---- 5. device store -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    import myfm_amd
    from myfm_amd.utils.synthetic import onehot_mf

    X, y, shapes = onehot_mf(2000, 40, 30)
    reg = myfm_amd.MyFMRegressor(4).fit(X, y, n_iter=12, n_kept_samples=7)
    cls = myfm_amd.MyFMClassifier(4).fit(X, y > y.mean(), n_iter=12, n_kept_samples=7)
    return X[:300], reg, cls


@pytest.mark.parametrize("which", ["regressor", "classifier"])
def test_store_path(fitted, which):
    X, reg, cls = fitted
    est, mode = (reg, 0) if which == "regressor" else (cls, 1)
    assert est.predictor_.resident and len(est.predictor_.samples) == 7
    got = est.predict_dist(X, quantiles=Q5)
    expect_mean = est.predict_proba(X) if mode else est.predict(X)
    assert np.array_equal(got.mean, expect_mean)
    check_A(got, device_values(est, X, [], mode), Q5, expect_mean)
    restored = pickle.loads(pickle.dumps(est))
    assert not restored.predictor_.resident  # host samples
    back = restored.predict_dist(X, quantiles=Q5)
    assert all(np.array_equal(a, b) for a, b in zip(got, back))
    tiled = est.predictor_.predict_dist(X, [], np.array(Q5), None, tile_rows=128, chunk_samples=2)
    assert all(np.array_equal(a, b) for a, b in zip(got, tiled))


def check_C(quantiles_dev, scores, alphas, probs):
    for i, p in enumerate(probs):
        F = dr.mixture_cdf(quantiles_dev[i], scores, alphas)
        worst = np.abs(F - p).max()
        ref = np.array([dr.mixture_quantile(scores[:, t], alphas, p) for t in range(scores.shape[1])])
        dq = np.abs(quantiles_dev[i] - ref) / np.maximum(1.0, np.abs(ref))
        assert worst <= 1e-12, p
        assert dq.max() <= 1e-9, p


def test_store_path_noise(fitted):
    """noise=True takes the alphas of the last 7 iterations of history_"""
    X, reg, _ = fitted
    alphas = np.array([h.alpha for h in reg.history_.hypers[-7:]])
    assert len(reg.history_.hypers) == 12 and np.all(alphas > 0)
    probs = (0.05, 0.5, 0.95)
    got = reg.predict_dist(X, quantiles=probs, noise=True)
    scores = device_values(reg, X, [], 0)
    assert np.array_equal(got.mean, reg.predict(X))
    np.testing.assert_allclose(got.std, np.sqrt(scores.var(axis=0) + np.mean(1.0 / alphas)), rtol=1e-12, atol=0)
    check_C(got.quantiles, scores, alphas, probs)
    direct = reg.predictor_.predict_dist(X, [], np.array(probs), alphas)
    assert all(np.array_equal(a, b) for a, b in zip(got, direct))
    restored = pickle.loads(pickle.dumps(reg))
    restored.history_ = reg.history_
    back = restored.predict_dist(X, quantiles=probs, noise=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, back))


# ---- 6. noise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N", [(1, 257), (2, 257), (95, 257), (3000, 7), (4096, 7)])
def test_noise_mixture(S, N):
    """S = 3000: one row and the S values of sqrt(alpha) no longer fit the 48 KB that several rows share; S = 4096: they take
    more than 64 KB, the dynamic-LDS opt-in"""
    rng = np.random.default_rng(60 + S)
    X = design("values", N, rng)
    est = make_predictor(task_of(0), D, 3, normal_samples(rng, D, 3, S))
    alphas = rng.permutation(np.geomspace(0.25, 400.0, S)) if S > 1 else np.array([0.25])
    probs = np.array([0.001, 0.05, 0.5, 0.95, 0.999])
    mean, std, qs = est.predictor_.predict_dist(X, [], probs, alphas)
    scores = device_values(est, X, [], 0)
    assert np.array_equal(mean, est.predict(X))
    np.testing.assert_allclose(std, np.sqrt(scores.var(axis=0) + np.mean(1.0 / alphas)), rtol=1e-12, atol=0)
    check_C(qs, scores, alphas, probs)
    mean0, std0, q0 = est.predictor_.predict_dist(X, [], np.array([]), alphas)  # the moments alone
    assert np.array_equal(mean0, mean) and np.array_equal(std0, std) and q0.shape == (0, N)
