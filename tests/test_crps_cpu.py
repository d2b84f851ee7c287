"""predict_crps without a GPU: (a) the reference of tests/crps_ref.py against quadrature, closed forms and its mpmath
twin, (b) the host row functions of the library against the reference, (c) the refusals on the host, (d) crps_summary and the
exports."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.integrate import quad
from scipy.special import ndtr

from tests import crps_ref as cr

EPS = np.finfo(np.float64).eps


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,seed", [(1, 0), (2, 1), (5, 2), (9, 3), (17, 4)])
def test_reference_against_quadrature(S, seed):
    """CRPS = int (F(x) - 1[x >= y])^2 dx of the mixture's CDF, split at y and at the components' means"""
    f, y, prec, _ = cr.random_rows(0, S, 3, seed)
    got = cr.crps_mixture(f, y, prec)[0]
    sd = 1.0 / np.sqrt(prec)
    for n in range(3):
        F = lambda x: float(np.mean(ndtr((x - f[:, n]) / sd)))  # noqa: E731
        lo, hi = min(f[:, n].min(), y[n]) - 12 * sd.max(), max(f[:, n].max(), y[n]) + 12 * sd.max()
        pts = sorted(set(list(f[:, n]) + [y[n]]))
        below = quad(lambda x: F(x) ** 2, lo, y[n], points=[p for p in pts if lo < p < y[n]] or None, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        above = quad(lambda x: (F(x) - 1.0) ** 2, y[n], hi, points=[p for p in pts if y[n] < p < hi] or None, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        assert abs(got[n] - (below + above)) <= 1e-11


def test_one_sample_is_the_normal_closed_form():
    """S = 1: sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)], z = (y - mu) / sigma (Gneiting and Raftery 2007)"""
    f, y, prec, _ = cr.random_rows(0, 1, 40, 7, far=6.0)
    sigma = 1.0 / np.sqrt(prec[0])
    z = (y - f[0]) / sigma
    want = sigma * (z * (2 * ndtr(z) - 1) + 2 * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) - 1 / np.sqrt(np.pi))
    crps, accuracy, spread = cr.crps_mixture(f, y, prec)
    assert np.all(cr.deviation(crps, want) <= 16 * EPS)
    assert np.all(cr.deviation(spread, sigma / np.sqrt(np.pi)) <= 4 * EPS) and np.all(crps >= (1 - 1 / np.sqrt(2)) * accuracy * (1 - 8 * EPS))


def test_classifier_crps_is_the_brier_score():
    f, y, _, _ = cr.random_rows(1, 9, 50, 8, far=3.0)
    crps, accuracy, spread = cr.crps_classes(f, y)
    p = cr.class_probs(f)[:, 1]
    assert np.all(np.abs(crps - (p - y) ** 2) <= 8 * EPS)
    assert np.all(np.abs((accuracy - spread) - crps) <= 4 * EPS)


def test_ordered_crps_is_the_ranked_probability_score():
    f, y, _, cut = cr.random_rows(2, 9, 50, 9, far=2.0)
    crps, accuracy, spread = cr.crps_classes(f, y, cut)
    cdf = np.cumsum(cr.class_probs(f, cut), axis=1)[:, :-1]  # (N, n_cut): P(Y <= j)
    step = (y[:, None] <= np.arange(cut.shape[1])[None, :]).astype(np.float64)
    assert np.all(np.abs(crps - ((cdf - step) ** 2).sum(axis=1)) <= 16 * EPS)
    assert np.all(np.abs((accuracy - spread) - crps) <= 8 * EPS)
    assert np.all(crps >= 0) and np.all(spread >= 0)


def test_the_recorded_tolerance_is_the_measured_one():
    measured = cr.measured_deviation()
    print("float64 reference against mpmath over tolerance_cases(): %.3e" % measured)
    assert measured <= 1.05 * cr.CRPS_MEASURED_DEVIATION and cr.CRPS_RTOL == 8 * cr.CRPS_MEASURED_DEVIATION


# ---- (b) the library's host rows ---------------------------------------------------------------------------------------------------
def _rows(task):
    """random rows of one task: S = 1, 2, 9, 33, 200; targets up to 40 sigma away; equal samples"""
    cases = [cr.random_rows(task, S, 6, 10 * task + S) for S in (1, 2, 9, 33, 200)]
    cases.append(cr.random_rows(task, 9, 9, 10 * task + 5, far=40.0))
    cases.append(cr.random_rows(task, 33, 4, 10 * task + 6, equal=True))
    return cases


@pytest.mark.parametrize("task", [0, 1, 2])
def test_host_rows_match_the_reference(task):
    from myfm_amd import _capi, _myfm

    for f, y, prec, cut in _rows(task):
        want = np.stack(cr.crps(task, f, y, prec, cut))
        assert np.all(np.isfinite(want)) and np.all(want[0] >= 0)
        for n in range(f.shape[1]):
            a = _myfm.crps_row(task, float(y[n]), f[:, n], prec, cut)
            b = _capi.crps_row(task, y[n], f[:, n], prec, cut)
            assert a == b and all(np.isfinite(a)) and a[0] >= 0
            assert np.all(cr.deviation(a, want[:, n]) <= cr.CRPS_RTOL), (task, f.shape, n, a, want[:, n])


def test_saturated_terms_stay_finite():
    """a target 40 sigma away: erf = 1, the exp term underflows, accuracy = |y - mu| to the last bits"""
    from myfm_amd import _myfm

    crps, accuracy, spread = _myfm.crps_row(0, 40.0, np.zeros(3), np.ones(3), None)
    assert accuracy == 40.0 and abs(spread - 1 / np.sqrt(np.pi)) <= 4 * EPS and crps == accuracy - spread
    crps, accuracy, spread = _myfm.crps_row(1, 1.0, np.full(3, -40.0), None, None)
    assert accuracy == 1.0 and spread == 0.0 and crps == 1.0
    crps, accuracy, spread = _myfm.crps_row(1, 0.0, np.full(3, -30.0), None, None)
    assert 0.0 < accuracy < 1e-150 and crps == accuracy * accuracy  # (the small side, from erfc itself)


def test_host_row_refusals():
    from myfm_amd import _capi, _myfm

    f = np.zeros(2)
    for fn in (_myfm.crps_row, _capi.crps_row):
        with pytest.raises(ValueError, match="bad task"):
            fn(3, 0.0, f, None, None)
        with pytest.raises(ValueError, match="needs the noise precision"):
            fn(0, 0.0, f, None, None)
        with pytest.raises(ValueError, match="positive and finite"):
            fn(0, 0.0, f, np.array([1.0, 0.0]), None)
        with pytest.raises(ValueError, match="regression"):
            fn(1, 0.0, f, np.ones(2), None)
        with pytest.raises(ValueError, match="0 or 1"):
            fn(1, 2.0, f, None, None)
        with pytest.raises(ValueError, match="ordered probit"):
            fn(1, 1.0, f, None, np.zeros((2, 1)))
        with pytest.raises(ValueError, match="needs at least one cutpoint per sample"):
            fn(2, 1.0, f, None, None)
        with pytest.raises(ValueError, match="finite and ascending"):
            fn(2, 1.0, f, None, np.array([[0.0, 1.0], [1.0, 0.0]]))
        with pytest.raises(ValueError, match="integers in"):
            fn(2, 3.0, f, None, np.array([[0.0, 1.0], [0.0, 1.0]]))
        with pytest.raises(ValueError, match="finite"):
            fn(0, np.nan, f, np.ones(2), None)
        with pytest.raises(ValueError, match="one entry per score"):
            fn(0, 0.0, f, np.ones(3), None)
        with pytest.raises(ValueError, match="at most 1024 samples"):
            fn(0, 0.0, np.zeros(1025), np.ones(1025), None)
        assert np.isfinite(fn(0, 0.0, np.zeros(1024), np.ones(1024), None)[0])
        assert np.isfinite(fn(2, 1.0, np.zeros(1025), None, np.zeros((1025, 1)))[0])  # tasks 1, 2: no sample limit


# ---- (c) refusals on the host, before the device is looked for ------------------------------------------------------------------
D, K, S = 12, 3, 2
CUTS = [np.array([-1.0, 0.0, 1.5]), np.array([-0.5, 0.25, 2.0])]
X3 = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, D))


def _restored(cls, task, cuts=None, n_samples=S):
    """an estimator around a Predictor restored through __setstate__ (no fit, no device)"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for s in range(n_samples):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), [] if cuts is None else [cuts[s % len(cuts)]]))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(getattr(_myfm.TaskType, task)), fms))
    est = getattr(myfm_amd, cls)(K)
    est.predictor_ = p
    return est


def _history(alphas):
    return types.SimpleNamespace(hypers=[types.SimpleNamespace(alpha=a) for a in alphas])


def _no_device():
    from myfm_amd import _myfm

    return _myfm.device_count() == 0


def _common_refusals(est, task, y, **kw):
    """what every task refuses, at the estimator and at predictor_: the messages of predict_log_density"""
    p = est.predictor_
    with pytest.raises(ValueError, match="one value per row"):
        est.predict_crps(X3, y[:2])
    with pytest.raises(ValueError, match="one value per row"):
        p.predict_crps(X3, [], y[:2], task, **kw)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            est.predict_crps(X3, np.array([y[0], bad, y[2]]))
        with pytest.raises(ValueError, match="finite"):
            p.predict_crps(X3, [], np.array([y[0], bad, y[2]]), task, **kw)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        est.predict_crps(X3[:, :11], y)
    for bad_task in (-1, 3):
        with pytest.raises(ValueError, match="bad task"):
            p.predict_crps(X3, [], y, bad_task, **kw)
    with pytest.raises(ValueError, match="does not match"):
        p.predict_crps(X3, [], y, (task + 1) % 3, **kw)
    for name in ("tile_rows", "chunk_samples"):
        with pytest.raises(ValueError, match="non-negative"):
            p.predict_crps(X3, [], y, task, **kw, **{name: -1})


def test_regression_refusals_need_no_gpu():
    est = _restored("MyFMGibbsRegressor", "REGRESSION")
    p, y = est.predictor_, np.array([0.5, -1.0, 2.0])
    with pytest.raises(RuntimeError, match="history_"):
        est.predict_crps(X3, y)
    for bad in (0.0, -1.0, np.inf, np.nan):
        est.history_ = _history([1.0, bad])
        with pytest.raises(ValueError, match="positive and finite"):
            est.predict_crps(X3, y)
        with pytest.raises(ValueError, match="positive and finite"):
            p.predict_crps(X3, [], y, 0, precisions=np.array([1.0, bad]))
    with pytest.raises(ValueError, match="needs the noise precision"):
        p.predict_crps(X3, [], y, 0)
    with pytest.raises(ValueError, match="one value per kept sample"):
        p.predict_crps(X3, [], y, 0, precisions=np.ones(3))
    with pytest.raises(ValueError, match="ordered probit only"):
        p.predict_crps(X3, [], y, 0, precisions=np.ones(2), cutpoints=np.zeros((2, 1)))
    est.history_ = _history([9.0, 1.0, 2.0])
    _common_refusals(est, 0, y, precisions=np.array([1.0, 2.0]))
    if _no_device():  # valid arguments: the usual refusal of a machine without a GPU comes only now
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_crps(X3, y)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.predict_crps(X3, [], y, 0, precisions=np.array([1.0, 2.0]))


def test_the_sample_limit_is_the_regressors_alone():
    y = np.array([0.5, -1.0, 2.0])
    est = _restored("MyFMGibbsRegressor", "REGRESSION", n_samples=1025)
    est.history_ = _history(np.ones(1025))
    with pytest.raises(ValueError, match="at most 1024 kept samples, this model keeps 1025"):
        est.predict_crps(X3, y)
    with pytest.raises(ValueError, match="at most 1024 kept samples, this model keeps 1025"):
        est.predictor_.predict_crps(X3, [], y, 0, precisions=np.ones(1025))
    if _no_device():
        ok = _restored("MyFMGibbsRegressor", "REGRESSION", n_samples=1024)
        ok.history_ = _history(np.ones(1024))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ok.predict_crps(X3, y)
        many = _restored("MyFMOrderedProbit", "ORDERED", CUTS, n_samples=1025)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            many.predict_crps(X3, np.array([0, 3, 2]))


def test_classification_refusals_need_no_gpu():
    est = _restored("MyFMGibbsClassifier", "CLASSIFICATION")
    p, y = est.predictor_, np.array([0.0, 1.0, 1.0])
    for bad in (2.0, -1.0, 0.5):
        with pytest.raises(ValueError, match="0 or 1"):
            est.predict_crps(X3, np.array([0.0, bad, 1.0]))
        with pytest.raises(ValueError, match="0 or 1"):
            p.predict_crps(X3, [], np.array([0.0, bad, 1.0]), 1)
    with pytest.raises(ValueError, match="regression only"):
        p.predict_crps(X3, [], y, 1, precisions=np.ones(2))
    with pytest.raises(ValueError, match="ordered probit only"):
        p.predict_crps(X3, [], y, 1, cutpoints=np.zeros((2, 1)))
    with pytest.raises(TypeError):
        est.predict_crps(X3, y, cutpoint_index=0)
    _common_refusals(est, 1, y)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_crps(X3, np.array([False, True, True]))


def test_ordered_refusals_need_no_gpu():
    est = _restored("MyFMOrderedProbit", "ORDERED", CUTS)
    p, y = est.predictor_, np.array([0, 3, 2])
    for bad in (4, -1, 1.5):  # three cutpoints: the labels are 0 .. 3
        with pytest.raises(ValueError, match="integers in"):
            est.predict_crps(X3, np.array([0, bad, 1]))
        with pytest.raises(ValueError, match="integers in"):
            p.predict_crps(X3, [], np.array([0, bad, 1], dtype=np.float64), 2, cutpoints=0)
    with pytest.raises(ValueError, match="needs the samples' cutpoints"):
        p.predict_crps(X3, [], y, 2)
    with pytest.raises(ValueError, match="regression only"):
        p.predict_crps(X3, [], y, 2, precisions=np.ones(2), cutpoints=0)
    with pytest.raises(ValueError, match="out of range"):
        est.predict_crps(X3, y, cutpoint_index=1)
    with pytest.raises(ValueError, match="must be an integer"):
        est.predict_crps(X3, y, cutpoint_index=0.0)
    with pytest.raises(ValueError, match="finite and ascending"):
        p.predict_crps(X3, [], y, 2, cutpoints=np.array([[-1.0, 0.0, 1.0], [0.0, 2.0, 1.0]]))
    _common_refusals(est, 2, y.astype(np.float64), cutpoints=0)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_crps(X3, y)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.predict_crps(X3, [], y, 2, cutpoints=np.stack(CUTS))


# ---- (d) crps_summary, exports -------------------------------------------------------------------------------------------------------
def test_crps_summary_by_hand():
    from myfm_amd import CrpsScore
    from myfm_amd.utils.evaluation import crps_summary

    a = CrpsScore(np.array([1.0, 2.0, 3.0, 6.0]), np.array([2.0, 3.0, 4.0, 7.0]), np.array([1.0, 1.0, 1.0, 1.0]))
    out = crps_summary(a)
    assert out == {"crps": 3.0, "se": float(np.sqrt(3.5 / 4)), "accuracy": 4.0, "spread": 1.0}  # var = (4 + 1 + 0 + 9) / 4
    b = CrpsScore(np.array([2.0, 2.0, 4.0, 8.0]), None, None)
    out = crps_summary(a, b)
    assert out["skill"] == 1.0 - 3.0 / 4.0 and out["se_diff"] == float(np.sqrt(np.var([-1.0, 0.0, -1.0, -2.0]) / 4))
    assert crps_summary(a, b.crps) == out and crps_summary(a.crps)["crps"] == 3.0
    with pytest.raises(ValueError, match="same rows"):
        crps_summary(a, b.crps[:3])


def test_who_has_the_method():
    import myfm_amd

    assert myfm_amd.CrpsScore._fields == ("crps", "accuracy", "spread")
    assert "CrpsScore" in myfm_amd.__all__
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.MyFMRegressor,
                myfm_amd.MyFMClassifier):
        assert callable(cls.predict_crps)
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_crps")
    assert callable(myfm_amd._myfm.Predictor.predict_crps) and callable(myfm_amd._myfm.crps_row)
    assert not hasattr(myfm_amd._myfm.VariationalPredictor, "predict_crps")
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        myfm_amd.MyFMRegressor(2).predict_crps(sps.csr_matrix((1, 3)), [0.5])


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_design_crps_store", "mfm_design_crps", "mfm_crps_row"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.Design.crps) and callable(_capi.Store.crps) and callable(_capi.crps_row)
