"""predict_proba_dist / predict_expected_dist of MyFMOrderedProbit, the parts that need no GPU: identities of the NumPy / SciPy
reference (tests/dist_oprobit_ref.py) that the device tests compare against, the surface, the argument checks, which run on the
host before the device is looked for, and the exports."""
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import dist_oprobit_ref as orf
from tests import dist_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mfm_design_summary_oprobit_store", "mfm_design_summary_oprobit")


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,C", [(1, 3, 2), (7, 11, 5), (65, 4, 33), (5, 3, 70)])
def test_reference_identities(S, N, C):
    rng = np.random.default_rng(100 * S + C)
    scores = rng.normal(size=(S, N)) * 1.5
    cuts = orf.sample_cutpoints(rng, S, C - 1)
    p = orf.class_probs(scores, cuts)
    assert p.shape == (S, N, C) and np.all(p >= 0.0)
    mean, std, qs = orf.summary(p, (0.05, 0.5, 0.95))
    assert mean.shape == (N, C) and std.shape == (N, C) and qs.shape == (3, N, C)
    np.testing.assert_allclose(mean.sum(axis=1), 1.0, rtol=0, atol=1e-15 * C)
    e = orf.expected_index(p)
    e_mean, e_std, e_qs = orf.summary(e, (0.05, 0.5, 0.95))
    assert e.shape == (S, N) and e_mean.shape == (N,) and e_std.shape == (N,) and e_qs.shape == (3, N)
    np.testing.assert_allclose(e_mean, mean @ np.arange(C), rtol=1e-13, atol=0)
    assert orf.summary(p, ())[2].shape == (0, N, C) and orf.summary(e, ())[2].shape == (0, N)


def test_one_cutpoint_is_the_classifier_of_the_shifted_score():
    """n_cut = 1: p_0 = Phi(cut - score), which is dist_ref's classifier value of the score shifted by the sample's cutpoint"""
    rng = np.random.default_rng(3)
    scores = rng.normal(size=(6, 9))
    cuts = rng.normal(size=(6, 1))
    p = orf.class_probs(scores, cuts)
    assert np.array_equal(p[:, :, 0], dr.values(cuts - scores, 1))
    assert np.array_equal(p[:, :, 1], 1.0 - dr.values(cuts - scores, 1))
    np.testing.assert_allclose(orf.expected_index(p), dr.values(scores - cuts, 1), rtol=0, atol=1e-15)


# ---- the surface ---------------------------------------------------------------------------------------------------------------
X3 = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, 12))


def test_surface():
    import myfm_amd

    for name in ("predict_proba_dist", "predict_expected_dist"):
        assert callable(getattr(myfm_amd.MyFMOrderedProbit, name))
        for cls in (myfm_amd.MyFMRegressor, myfm_amd.MyFMClassifier, myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier,
                    myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
            assert not hasattr(cls, name), (cls, name)
    assert not hasattr(myfm_amd.MyFMOrderedProbit, "predict_dist")
    for name in ("predict_proba_dist", "predict_expected_dist"):
        with pytest.raises(RuntimeError, match="Predictor called before fit"):
            getattr(myfm_amd.MyFMOrderedProbit(2), name)(X3)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def _restored(S=2, D=12, K=3, n_cut=4, cut_groups=1):
    """MyFMOrderedProbit around a Predictor restored through __setstate__ (no fit, no device)"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for s in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), [np.arange(n_cut) * 0.7 - 1.0 + 0.01 * (s % 7)] * cut_groups))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(_myfm.TaskType.ORDERED), fms))
    est = myfm_amd.MyFMOrderedProbit(K)
    est.predictor_ = p
    return est


@pytest.mark.parametrize("method,expected", [("predict_proba_dist", False), ("predict_expected_dist", True)])
def test_argument_checks_need_no_gpu(method, expected):
    import myfm_amd
    from myfm_amd import _myfm

    est = _restored()
    call = getattr(est, method)
    with pytest.raises(ValueError, match="1-D"):
        call(X3, quantiles=[[0.5]])
    with pytest.raises(ValueError, match="1-D"):
        call(X3, quantiles=0.5)
    with pytest.raises(ValueError, match="at most 32"):
        call(X3, quantiles=np.linspace(0, 1, 33))
    for bad in (-0.1, 1.0000001, np.nan):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            call(X3, quantiles=[0.5, bad])
    for bad in (1, -1, 7):
        with pytest.raises(ValueError, match="cutpoint_index"):
            call(X3, cutpoint_index=bad)
    with pytest.raises(ValueError, match="cutpoint_index"):
        call(X3, cutpoint_index=0.0)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        call(X3[:, :11])
    with pytest.raises(ValueError, match="X and X_rel have different shape"):
        call(X3[:, :8], [myfm_amd.RelationBlock([0, 1], sps.csr_matrix(np.eye(4)))])
    with pytest.raises(TypeError):
        call(X3, noise=True)  # y is discrete: there is no noise form
    # the binding makes the same checks on what reaches it
    p = est.predictor_
    with pytest.raises(ValueError, match="1-D"):
        p.predict_dist_oprobit(X3, [], np.zeros((2, 2)), 0, expected)
    with pytest.raises(ValueError, match="at most 32"):
        p.predict_dist_oprobit(X3, [], np.linspace(0, 1, 33), 0, expected)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        p.predict_dist_oprobit(X3, [], np.array([np.nan]), 0, expected)
    with pytest.raises(ValueError, match="non-negative"):
        p.predict_dist_oprobit(X3, [], np.array([0.5]), 0, expected, tile_rows=-1)
    for bad in (1, -1):
        with pytest.raises(ValueError, match="cutpoint_index"):
            p.predict_dist_oprobit(X3, [], np.array([0.5]), bad, expected)
    # Predictor.predict_dist keeps refusing an ordered model
    with pytest.raises(ValueError, match="not ordered probit"):
        p.predict_dist(X3, [], np.array([0.5]))
    # valid arguments: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(X3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(X3, quantiles=())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _restored(cut_groups=2).predict_proba_dist(X3, cutpoint_index=1)


def test_samples_must_agree_on_the_number_of_cutpoints():
    from myfm_amd import _myfm

    est = _restored(S=3)
    fms = list(est.predictor_.samples)
    odd = _myfm.FM.__new__(_myfm.FM)
    odd.__setstate__((0.5, np.zeros(12), np.zeros((12, 3)), [np.array([-1.0, 1.0])]))
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((3, 12, int(_myfm.TaskType.ORDERED), fms + [odd]))
    est.predictor_ = p
    for method, expected in (("predict_proba_dist", False), ("predict_expected_dist", True)):
        with pytest.raises(ValueError, match="different numbers of cutpoints"):
            getattr(est, method)(X3)
        with pytest.raises(ValueError, match="inconsistent cutpoint sizes"):
            p.predict_dist_oprobit(X3, [], np.array([0.5]), 0, expected)


@pytest.mark.parametrize("method,expected", [("predict_proba_dist", False), ("predict_expected_dist", True)])
def test_sample_limit_applies_to_quantiles_only(method, expected):
    from myfm_amd import _myfm

    est = _restored(S=4097)
    with pytest.raises(ValueError, match="4096"):
        getattr(est, method)(X3)
    with pytest.raises(ValueError, match="4096"):
        est.predictor_.predict_dist_oprobit(X3, [], np.array([0.5]), 0, expected)
    if _myfm.device_count() == 0:  # mean and std have no limit: the call gets as far as the device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(est, method)(X3, quantiles=())


# ---- the exports ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_and_exported():
    from myfm_amd import _capi

    with open(os.path.join(ROOT, "include", "myfm_hip.h")) as f:
        header = f.read()
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert callable(_capi.Design.summary_oprobit) and callable(_capi.Store.summary_oprobit)
