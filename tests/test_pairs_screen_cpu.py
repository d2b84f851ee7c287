"""The screened top-k without a device: the exported symbols, the argument checks that come before the device is
looked for, and which estimators have the method."""
import numpy as np
import pytest
import scipy.sparse as sps


def test_symbols_exported():
    from myfm_amd import _capi

    L = _capi.lib()
    for name in ("mfm_pairs_topk_screened", "mfm_pairs_topk_screened_store", "mfm_pairs_screen_scores", "mfm_pairs_screen_scores_store"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    for name in ("topk_screened", "topk_screened_store", "screen_scores", "screen_scores_store"):
        assert hasattr(_capi.Pairs, name)


def test_value_errors_without_a_device():
    import myfm_amd
    from myfm_amd import _myfm

    D, K = 6, 2
    rng = np.random.default_rng(5)
    fms = []
    for _ in range(2):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(_myfm.TaskType.REGRESSION), fms))
    est = myfm_amd.MyFMRegressor(K)
    est.predictor_ = p
    X = sps.identity(D, format="csr")
    Xq, Xc = X[:2], X[2:]
    for bad in (0, 129, 256, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            est.predict_topk_screened(Xq, Xc, bad)
    with pytest.raises(ValueError, match="share column 1"):
        est.predict_topk_screened(Xq, X[1:], 3)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.predict_topk_screened(Xq, Xc, 3, exclude=sps.identity(3, format="csr"))
    with pytest.raises(ValueError, match="k must be"):  # (the binding's own check, for a caller that skips the estimator)
        p.predict_topk_screened(Xq, Xc, 129, None, [], [])
    if _myfm.device_count() == 0:  # valid arguments: the refusal of a machine without a GPU comes only now
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_topk_screened(Xq, Xc, 3)


def test_only_the_regressors_have_the_method():
    import myfm_amd

    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.VariationalFMRegressor):
        assert hasattr(cls, "predict_topk_screened")
    for cls in (myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_topk_screened")
