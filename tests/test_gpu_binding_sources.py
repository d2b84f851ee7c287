"""Both branches of the binding's sample dispatch: a fitted estimator's predictor reads the device store in place, the
same estimator after pickle.loads(pickle.dumps(.)) holds host samples that are packed for the call. The same kernels run over the
same numbers, so every device predictor must return the same bits either way. predict / predict_proba are left out: the host
flavour of mfm_design_predict streams one sample at a time by design and sums in another order than the one-pass store form."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_ROWS, RANK, N_KEPT, N_CLASS = 40, 30, 600, 3, 4, 5
D = N_USERS + N_ITEMS
QUANTILES = (0.05, 0.5, 0.95)


def onehot(cols, width=D):
    """one row per entry of `cols`, a row holding 1 in each of its columns"""
    cols = np.asarray(cols, dtype=np.int32).reshape(len(cols), -1)
    n, m = cols.shape
    X = sps.csr_matrix((np.ones(n * m), cols.ravel(), np.arange(0, n * m + 1, m, dtype=np.int64)), shape=(n, width))
    X.sort_indices()
    return X


def same(a, b):
    """a and b (arrays or tuples of arrays) are equal bit for bit"""
    a, b = (tuple(a), tuple(b)) if isinstance(a, tuple) else ((a,), (b,))
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module", params=["regressor", "classifier", "ordered"])
def sources(request):
    """(kind, the fitted estimator, the same restored from a pickle, the design rows of the fit): 600 of the 1200 (user, item)
    pairs of a 40 x 30 one-hot table, rank 3, the last 4 of 8 iterations kept"""
    import myfm_amd

    kind = request.param
    rng = np.random.default_rng(31)
    pair = rng.permutation(N_USERS * N_ITEMS)[:N_ROWS]
    u, i = pair // N_ITEMS, pair % N_ITEMS
    P, Q = rng.normal(size=(N_USERS, 2)), rng.normal(size=(N_ITEMS, 2))
    lat = 0.5 * rng.normal(size=N_USERS)[u] + (P[u] * Q[i]).sum(axis=1) + 0.5 * rng.normal(size=N_ROWS)
    X = onehot(np.stack([u, N_USERS + i], axis=1))
    cls, y = {"regressor": (myfm_amd.MyFMGibbsRegressor, lat), "classifier": (myfm_amd.MyFMGibbsClassifier, lat > 0),
              "ordered": (myfm_amd.MyFMOrderedProbit, np.digitize(lat, [-1.5, -0.5, 0.5, 1.5]))}[kind]
    est = cls(RANK, random_seed=5).fit(X, y, n_iter=8, n_kept_samples=N_KEPT, group_shapes=[N_USERS, N_ITEMS])
    restored = pickle.loads(pickle.dumps(est))
    assert est.predictor_.resident and len(est.predictor_.samples) == N_KEPT
    assert not restored.predictor_.resident and len(restored.predictor_.samples) == N_KEPT  # host samples
    return kind, est, restored, X


def test_pair_predictors(sources):
    _, est, restored, _ = sources
    Xq, Xc = onehot(np.arange(17)), onehot(N_USERS + np.arange(N_ITEMS))
    exclude = sps.csr_matrix(np.random.default_rng(2).random((17, N_ITEMS)) < 0.2)
    assert same(est.predict_pairs(Xq, Xc), restored.predict_pairs(Xq, Xc))
    assert same(est.predict_topk(Xq, Xc, 5, exclude=exclude), restored.predict_topk(Xq, Xc, 5, exclude=exclude))
    assert same(tuple(est.predict_pairs_dist(Xq, Xc)), tuple(restored.predict_pairs_dist(Xq, Xc)))
    # (5 < the 30 candidates less a row's exclusions: no NaN tail)
    assert same(tuple(est.predict_topk_ucb(Xq, Xc, 5, beta=1, exclude=exclude)),
                tuple(restored.predict_topk_ucb(Xq, Xc, 5, beta=1, exclude=exclude)))


def test_summaries(sources):
    kind, est, restored, X = sources
    rows = X[:257]
    if kind == "ordered":
        for name in ("predict_proba_dist", "predict_expected_dist"):
            assert same(tuple(getattr(est, name)(rows, quantiles=QUANTILES)), tuple(getattr(restored, name)(rows, quantiles=QUANTILES)))
        return
    assert same(tuple(est.predict_dist(rows, quantiles=QUANTILES)), tuple(restored.predict_dist(rows, quantiles=QUANTILES)))
    if kind == "regressor":
        assert same(tuple(est.predict_dist(rows, quantiles=QUANTILES, noise=True)),
                    tuple(restored.predict_dist(rows, quantiles=QUANTILES, noise=True)))


@pytest.mark.parametrize("draw", [False, True])
def test_fold_in(sources, draw):
    """3 new users with 4 observations each: the folded-in columns of every kept sample"""
    kind, est, restored, _ = sources
    rng = np.random.default_rng(9)
    entity = np.repeat(np.arange(3), 4)
    X_new = onehot(N_USERS + np.concatenate([rng.permutation(N_ITEMS)[:4] for _ in range(3)]))
    y_new = {"regressor": rng.normal(size=12), "classifier": rng.random(12) < 0.5, "ordered": rng.integers(0, N_CLASS, size=12)}[kind]
    name = "fold_in" if kind == "regressor" else "fold_in_gibbs"
    a = getattr(est, name)(X_new, y_new, entity, 0, draw=draw, random_seed=4)
    b = getattr(restored, name)(X_new, y_new, entity, 0, draw=draw, random_seed=4)
    assert a.w_samples.shape == (N_KEPT, D + 3) and a.V_samples.shape == (N_KEPT, D + 3, RANK)
    assert same(a.w_samples[:, D:], b.w_samples[:, D:]) and same(a.V_samples[:, D:], b.V_samples[:, D:])
