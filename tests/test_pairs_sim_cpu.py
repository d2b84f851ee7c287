"""The similarity forms without a device: the float64 twin of the kernels' operations against the longdouble
reference within the derived tolerance, the exact inputs, the invariance under per-sample rotations that is the reason for the
per-sample definition, the host-side argument checks, neighbour_table and the exported symbols."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_ref as pr
from tests import pairs_sim_ref as sr
from tests import pairs_ucb_ref as ur

HALVES = [1.0, -1.0, 2.0, -2.0, 0.5]


def _real_case(K, S, shared, U=12, I=40):
    rng = np.random.default_rng(100 + K + S + shared)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    if shared:
        Xq = Xc[:U]
    return Xq, Xc, pr.normal_samples(rng, D, K, S, scale=0.3)


@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("K,S", [(8, 5), (33, 7)])
def test_twin_within_tolerance(K, S, shared, metric):
    """the float64 restatement of the device's operations agrees with the longdouble reference within the tolerance the GPU tests
    use, with room to spare, and the inputs are well conditioned (the bracket stays below 100)"""
    Xq, Xc, samples = _real_case(K, S, shared)
    vals = sr.sample_values(samples, Xq, Xc, metric)
    rmean, rstd = ur.moments_ld(vals)
    assert sr.brackets(samples, Xq, Xc, "cosine").max() < 100.0  # (the condition is the cosine's; the inner product's bound is absolute)
    b_mean, b_std = sr.bounds(samples, Xq, Xc, metric, vals)
    for reverse in (False, True):
        mean, std = sr.twin_moments(samples, Xq, Xc, metric, reverse)
        use = float((np.abs(mean - rmean) / b_mean).max()), float((np.abs(std - rstd) / b_std).max())
        assert max(use) < 1e-2, use
    assert float(np.asarray(rstd, dtype=np.float64).max()) > 1e-2
    if metric == "cosine":
        assert float(np.abs(np.asarray(vals, dtype=np.float64)).max()) <= 1.0 + 1e-12
        if shared:  # a row against itself
            live = np.asarray(sr.inv_norm_ld(sr.embeddings_ld(samples, Xq)), dtype=np.float64).min(axis=0) > 0
            d = np.asarray(rmean, dtype=np.float64)[np.arange(Xq.shape[0]), np.arange(Xq.shape[0])]
            assert np.all(np.abs(d[live] - 1.0) < 1e-15) and np.all(d[~live] == 0.0)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
def test_exact_unit_samples_are_exact(K, S, shared):
    """float64 in two factor orders and longdouble agree bit for bit on the exact inputs, under both metrics; the values tie often"""
    rng = np.random.default_rng(7 + 10 * K + S)
    D = 20
    Xq, Xc = sr.unit_sides(rng, 17, 50, D, shared)
    samples = sr.exact_unit_samples(rng, D, K, S)
    for metric in sr.METRICS:
        rmean, rstd = (np.asarray(x, dtype=np.float64) for x in sr.moments(samples, Xq, Xc, metric))
        for reverse in (False, True):
            mean, std = sr.twin_moments(samples, Xq, Xc, metric, reverse)
            assert np.array_equal(mean, rmean) and np.array_equal(std, rstd)
        if S == 1:
            assert np.all(rstd == 0.0)
        if S == 2:
            v = np.asarray(sr.sample_values(samples, Xq, Xc, metric), dtype=np.float64)
            assert np.array_equal(rstd, np.abs(v[0] - v[1]) / 2)
        empty = np.diff(Xq.indptr) == 0
        assert empty.any() and np.all(rmean[empty] == 0.0) and np.all(rstd[empty] == 0.0)
        if metric == "cosine" and K >= 4:
            assert 3 <= np.unique(rmean).size <= 40


def test_rotation_invariance_and_the_averaged_V():
    """rotating each sample's V by its own orthogonal matrix leaves mean and std of the per-sample cosine where they were; the
    cosine of the averaged V moves: an average of factors that differ by rotations means nothing"""
    Xq, Xc, samples = _real_case(8, 5, True)
    turned = sr.rotated(np.random.default_rng(3), samples)
    for metric in sr.METRICS:
        vals = sr.sample_values(samples, Xq, Xc, metric)
        (m0, s0), (m1, s1) = ur.moments_ld(vals), sr.moments(turned, Xq, Xc, metric)
        b_mean, b_std = sr.bounds(samples, Xq, Xc, metric, vals)
        assert np.all(np.abs(np.asarray(m0 - m1, dtype=np.float64)) <= b_mean) and np.all(np.abs(np.asarray(s0 - s1, dtype=np.float64)) <= b_std)

    def of_average(ss):
        Vbar = np.mean([np.asarray(V) for _, _, V in ss], axis=0)
        return np.asarray(sr.sample_values([(0.0, None, Vbar)], Xq, Xc, "cosine")[0], dtype=np.float64)

    assert np.abs(of_average(samples) - of_average(turned)).max() > 0.1


# ---- the host-side argument checks: raised on a machine without a GPU --------------------------------------------------------------------
def _restored(cls, task, D=6, K=2, S=2):
    """an estimator around a Predictor restored through __setstate__ (no fit, no device)"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for _ in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), [np.array([-0.5, 0.5])] if task == "ORDERED" else []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(getattr(_myfm.TaskType, task)), fms))
    est = getattr(myfm_amd, cls)(K)
    est.predictor_ = p
    return est


@pytest.mark.parametrize("cls,task", [("MyFMRegressor", "REGRESSION"), ("MyFMClassifier", "CLASSIFICATION"), ("MyFMOrderedProbit", "ORDERED")])
def test_value_errors_without_a_device(cls, task):
    from myfm_amd import _myfm

    est = _restored(cls, task)
    X = sps.identity(6, format="csr")
    for name in ("predict_similar", "predict_similarity"):
        for bad in ("euclid", "", None, 0):
            with pytest.raises(ValueError, match="metric"):
                getattr(est, name)(X, metric=bad)
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            est.predict_similar(X, k=bad)
    for bad in (np.inf, np.nan, "1", None):
        with pytest.raises(ValueError, match="beta must be a finite"):
            est.predict_similar(X, k=3, beta=bad)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.predict_similar(X, k=3, exclude=sps.identity(5, format="csr"))
    with pytest.raises(ValueError, match="exclude_self"):
        est.predict_similar(X, X, k=3, exclude_self=True)
    with pytest.raises(ValueError, match="feature_size|Told to predict"):
        est.predict_similar(sps.identity(5, format="csr"), k=3)
    with pytest.raises(ValueError, match="2\\^24"):
        est.predict_similarity(sps.csr_matrix((5000, 6)), sps.csr_matrix((5000, 6)))
    # valid arguments, shared columns included: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        for call in (lambda: est.predict_similar(X, k=3), lambda: est.predict_similar(X, X[:4], k=3, metric="dot", beta=-1.0),
                     lambda: est.predict_similarity(X), lambda: est.predict_similarity(X[:2], X, metric="dot")):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_variational_estimators_have_no_such_method():
    import myfm_amd

    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_similar") and not hasattr(cls, "predict_similarity")
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit):
        assert hasattr(cls, "predict_similar") and hasattr(cls, "predict_similarity")


# ---- neighbour_table -------------------------------------------------------------------------------------------------------------------
def test_neighbour_table():
    from myfm_amd.utils.ranking import neighbour_table

    idx = np.array([[2, 0, -1], [1, 3, 0]])
    mean = np.array([[0.9, 0.4, np.nan], [0.8, 0.7, -0.2]])
    std = np.array([[0.05, 0.3, np.nan], [0.2, 0.01, 0.1]])
    res = (idx, mean + std, mean, std)
    assert neighbour_table(res) == [[(2, 0.9, 0.05), (0, 0.4, 0.3)], [(1, 0.8, 0.2), (3, 0.7, 0.01), (0, -0.2, 0.1)]]
    names = ["a", "b", "c", "d"]
    assert neighbour_table(res, names, min_mean=0.5) == [[("c", 0.9, 0.05)], [("b", 0.8, 0.2), ("d", 0.7, 0.01)]]
    assert neighbour_table(res, names, min_mean=0.5, max_std=0.1) == [[("c", 0.9, 0.05)], [("d", 0.7, 0.01)]]
    assert neighbour_table(res, max_std=0.0) == [[], []]
    with pytest.raises(ValueError, match="names has"):
        neighbour_table(res, names[:3])
    with pytest.raises(ValueError, match="\\(U, k\\)"):
        neighbour_table((idx[0], mean[0], mean[0], std[0]))


# ---- the library's symbols ----------------------------------------------------------------------------------------------------------------
def test_symbols_exported():
    from myfm_amd import _capi

    L = _capi.lib()
    for name in ("mfm_pairs_create_sim", "mfm_pairs_sim", "mfm_pairs_sim_store", "mfm_pairs_topk_sim", "mfm_pairs_topk_sim_store"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert _capi.SIM_METRICS == {"cosine": 0, "dot": 1}
    assert _capi._sim_metric("cosine") == 0 and _capi._sim_metric("dot") == 1 and _capi._sim_metric(np.int32(1)) == 1
    assert _capi._sim_metric(7) == 7  # (a number is the library's to refuse)
    for bad in ("euclid", "", None, 0.5, True):
        with pytest.raises(ValueError, match='"cosine" or "dot"'):
            _capi._sim_metric(bad)
