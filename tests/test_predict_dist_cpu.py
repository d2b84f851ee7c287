"""predict_dist, the parts that need no GPU: identities of the NumPy / SciPy reference (tests/dist_ref.py) that the device
tests compare against, the argument checks, which run on the host before the device is looked for, and the exports."""
import types

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.special import ndtri

from tests import dist_ref as dr


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.001, 0.05, 0.5, 0.95, 0.999])
def test_identical_components_have_the_normal_quantile(p):
    m, alpha = 1.75, 6.25
    q = dr.mixture_quantile(np.full(9, m), np.full(9, alpha), p)
    assert abs(q - (m + ndtri(p) / np.sqrt(alpha))) <= 1e-12


def test_bracket_property_on_random_inputs():
    """F(min_s y_s) <= p <= F(max_s y_s): every component's CDF at min_s y_s is at most p, at max_s y_s at least p"""
    rng = np.random.default_rng(11)
    for _ in range(200):
        S = int(rng.integers(1, 40))
        scores, alphas = rng.normal(size=S) * 3.0, np.exp(rng.uniform(np.log(0.25), np.log(400.0), size=S))
        p = float(rng.choice([0.001, 0.05, 0.3, 0.5, 0.95, 0.999]))
        lo, hi = dr.bracket(scores, alphas, p)
        assert dr.mixture_cdf(lo, scores, alphas) <= p + 1e-15 and dr.mixture_cdf(hi, scores, alphas) >= p - 1e-15
        q = dr.mixture_quantile(scores, alphas, p)
        assert lo <= q <= hi and abs(dr.mixture_cdf(q, scores, alphas) - p) <= 1e-12


@pytest.mark.parametrize("S", [1, 2, 7, 95])
def test_sharp_components_approach_the_empirical_bracket(S):
    """alpha -> 1e12: the mixture's CDF steps by 1 / S at every score, and its p-quantile lies between the two order statistics
    that np.quantile interpolates (within a few component widths, 1e-6 each)"""
    rng = np.random.default_rng(S)
    scores = rng.normal(size=S)
    srt = np.sort(scores)
    for p in (0.001, 0.05, 0.3, 0.5, 0.77, 0.95, 0.999):
        q = dr.mixture_quantile(scores, np.full(S, 1e12), p)
        lo = int(np.floor((S - 1) * p))
        assert srt[lo] - 1e-5 <= q <= srt[min(lo + 1, S - 1)] + 1e-5


def test_noise_summary_of_one_component():
    scores = np.array([[0.5, -2.0]])
    mean, std, qs = dr.noise_summary(scores, [4.0], [0.05, 0.5])
    assert np.array_equal(mean, scores[0]) and np.allclose(std, 0.5, rtol=1e-15)
    assert np.allclose(qs, scores + ndtri([0.05, 0.5])[:, None] / 2.0, rtol=0, atol=1e-13)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def _restored(cls, task, D=12, K=3, S=2):
    """an estimator around a Predictor restored through __setstate__ (no fit, no device)"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for _ in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(task), fms))
    est = getattr(myfm_amd, cls)(K)
    est.predictor_ = p
    return est


def _history(alphas):
    return types.SimpleNamespace(hypers=[types.SimpleNamespace(alpha=a) for a in alphas])


X3 = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, 12))


@pytest.mark.parametrize("cls,task", [("MyFMRegressor", "REGRESSION"), ("MyFMClassifier", "CLASSIFICATION"),
                                      ("MyFMGibbsRegressor", "REGRESSION"), ("MyFMGibbsClassifier", "CLASSIFICATION")])
def test_argument_checks_need_no_gpu(cls, task):
    import myfm_amd
    from myfm_amd import _myfm

    est = _restored(cls, getattr(_myfm.TaskType, task))
    with pytest.raises(ValueError, match="1-D"):
        est.predict_dist(X3, quantiles=[[0.5]])
    with pytest.raises(ValueError, match="1-D"):
        est.predict_dist(X3, quantiles=0.5)
    with pytest.raises(ValueError, match="at most 32"):
        est.predict_dist(X3, quantiles=np.linspace(0, 1, 33))
    for bad in (-0.1, 1.0000001, np.nan):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            est.predict_dist(X3, quantiles=[0.5, bad])
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        est.predict_dist(X3[:, :11])
    with pytest.raises(ValueError, match="X and X_rel have different shape"):
        est.predict_dist(X3[:, :8], [myfm_amd.RelationBlock([0, 1], sps.csr_matrix(np.eye(4)))])
    # the binding makes the same checks on what reaches it
    p = est.predictor_
    with pytest.raises(ValueError, match="1-D"):
        p.predict_dist(X3, [], np.zeros((2, 2)))
    with pytest.raises(ValueError, match="at most 32"):
        p.predict_dist(X3, [], np.linspace(0, 1, 33))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        p.predict_dist(X3, [], np.array([np.nan]))
    with pytest.raises(ValueError, match="non-negative"):
        p.predict_dist(X3, [], np.array([0.5]), tile_rows=-1)
    if task == "CLASSIFICATION":
        est.history_ = _history([1.0, 2.0])
        with pytest.raises(ValueError, match="classifier"):
            est.predict_dist(X3, noise=True)
        with pytest.raises(ValueError, match="regression only"):
            p.predict_dist(X3, [], np.array([0.5]), precisions=np.ones(2))
    else:
        for bad in (0.0, 1.0):
            with pytest.raises(ValueError, match="strictly inside"):
                est.predict_dist(X3, quantiles=[0.5, bad], noise=True)
        with pytest.raises(RuntimeError, match="history_"):  # no history at all
            est.predict_dist(X3, noise=True)
        est.history_ = _history([1.0])  # ... and one that is shorter than the two kept samples
        with pytest.raises(RuntimeError, match="history_"):
            est.predict_dist(X3, noise=True)
        with pytest.raises(ValueError, match="strictly inside"):
            p.predict_dist(X3, [], np.array([1.0]), precisions=np.ones(2))
        with pytest.raises(ValueError, match="one value per kept sample"):
            p.predict_dist(X3, [], np.array([0.5]), precisions=np.ones(3))
        with pytest.raises(ValueError, match="positive and finite"):
            p.predict_dist(X3, [], np.array([0.5]), precisions=np.array([1.0, 0.0]))
        est.history_ = _history([1.0, 2.0, 4.0])
    # valid arguments: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_dist(X3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_dist(X3, quantiles=())
        if task == "REGRESSION":
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.predict_dist(X3, noise=True)


def test_sample_limit_applies_to_quantiles_only():
    from myfm_amd import _myfm

    est = _restored("MyFMRegressor", _myfm.TaskType.REGRESSION, S=4097)
    with pytest.raises(ValueError, match="4096"):
        est.predict_dist(X3)
    with pytest.raises(ValueError, match="4096"):
        est.predictor_.predict_dist(X3, [], np.array([0.5]))
    if _myfm.device_count() == 0:  # mean and std have no limit: the call gets as far as the device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_dist(X3, quantiles=())


def test_out_of_scope_estimators_have_no_predict_dist():
    import myfm_amd

    for cls in (myfm_amd.MyFMOrderedProbit, myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_dist")
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        myfm_amd.MyFMRegressor(2).predict_dist(X3)


def test_new_symbols_are_exported():
    from myfm_amd import _capi

    L = _capi.lib()
    for name in ("mfm_design_summary_store", "mfm_design_summary"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert callable(_capi.Design.summary) and callable(_capi.Store.summary)
