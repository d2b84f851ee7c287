"""predict_log_density, the parts that need no GPU: identities of the NumPy / SciPy reference (tests/logdens_ref.py) that the device
tests compare against, the evaluation helpers, the value function of csrc/mfm_logdens.hpp run on the host (_myfm.log_density_value,
the code the kernel runs) against that reference, the argument checks, which run before the device is looked for, and the exports."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.special import log_ndtr, ndtr

from tests import logdens_ref as lr


# ---- (a) the reference and the evaluation helpers ----------------------------------------------------------------------------------
def test_classifier_lpd_is_the_log_of_the_mean_probability():
    rng = np.random.default_rng(1)
    f = rng.normal(size=(7, 50)) * 3.0
    lpd, _, _, pit = lr.summarise(lr.log_lik(f, np.ones(50), 1))
    assert pit is None and np.allclose(np.exp(lpd), ndtr(f).mean(axis=0), rtol=1e-13, atol=0)
    lpd0 = lr.summarise(lr.log_lik(f, np.zeros(50), 1))[0]
    assert np.allclose(np.exp(lpd) + np.exp(lpd0), 1.0, rtol=1e-13, atol=0)


def test_ordered_class_densities_sum_to_one():
    rng = np.random.default_rng(2)
    S, N = 5, 40
    f = rng.normal(size=(S, N)) * 2.0
    cut = np.sort(rng.normal(size=(S, 4)) * 1.5, axis=1)
    total = sum(np.exp(lr.summarise(lr.log_lik(f, np.full(N, c), 2, cutpoints=cut))[0]) for c in range(5))
    assert np.allclose(total, 1.0, rtol=1e-13, atol=0)


def test_one_sample_has_no_variance():
    rng = np.random.default_rng(3)
    f, y = rng.normal(size=(1, 9)), rng.normal(size=9)
    lpd, mean, var, pit = lr.summarise(lr.log_lik(f, y, 0, precisions=[2.5]), f, y, [2.5])
    assert np.array_equal(lpd, mean) and np.array_equal(var, np.zeros(9))
    assert np.allclose(pit, ndtr((y - f[0]) * np.sqrt(2.5)), rtol=1e-15)


def test_waic_by_hand():
    from myfm_amd.utils.evaluation import log_score, waic

    lpd, var = np.array([-1.0, -2.0, -0.5]), np.array([0.1, 0.5, 0.0])
    w = waic((lpd, None, var, None, None))
    assert w["lppd"] == -3.5 and abs(w["p_waic"] - 0.6) < 1e-15 and abs(w["elpd_waic"] + 4.1) < 1e-15 and abs(w["waic"] - 8.2) < 1e-14
    # the rows' elpd: -1.1, -2.5, -0.5; mean -4.1 / 3; se = sqrt(3 * population variance)
    e = np.array([-1.1, -2.5, -0.5])
    assert abs(w["se"] - np.sqrt(((e - e.mean()) ** 2).sum())) < 1e-14
    assert w["n_high_variance"] == 1 and set(w) == {"lppd", "p_waic", "elpd_waic", "waic", "se", "n_high_variance"}
    assert abs(log_score((lpd,)) - 3.5 / 3) < 1e-15


def test_pit_histogram_on_known_values():
    from myfm_amd.utils.evaluation import pit_histogram

    counts, chi2 = pit_histogram(np.array([0.0, 0.05, 0.15, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75, 0.85, 0.95, 1.0]), bins=4)
    assert list(counts) == [3, 3, 2, 4] and abs(chi2 - (0 + 0 + 1 + 1) / 3.0) < 1e-15
    uniform = (np.arange(100) + 0.5) / 100
    counts, chi2 = pit_histogram(types.SimpleNamespace(pit=uniform))
    assert list(counts) == [10] * 10 and chi2 == 0.0
    with pytest.raises(ValueError, match="regression only"):
        pit_histogram(types.SimpleNamespace(pit=None))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        pit_histogram(np.array([0.5, 1.5]))


# ---- (b) the value function on the host against the reference ----------------------------------------------------------------------
def _interval_value(lo, hi):
    """log(Phi(hi) - Phi(lo)) by the code under test: an ordered-probit value at score 0 whose class has the cutpoints lo, hi"""
    from myfm_amd import _myfm

    if np.isinf(lo):
        return _myfm.log_density_value(2, 0.0, 0.0, 0.0, 0.0, [hi, hi + 1.0])
    if np.isinf(hi):
        return _myfm.log_density_value(2, 2.0, 0.0, 0.0, 0.0, [lo - 1.0, lo])
    return _myfm.log_density_value(2, 1.0, 0.0, 0.0, 0.0, [lo, hi])


def test_value_function_on_the_regime_grid():
    lo, hi = lr.value_grid()
    ref, alt = lr.interval_log_prob(lo, hi), lr.alt_interval_log_prob(lo, hi)
    one_sided = np.isinf(lo) | np.isinf(hi)
    # the grid reaches every regime: A, B, C wide, C narrow (both ends within 0.5, one interval straddling 0), both one-sided labels
    two = ~one_sided
    narrow = two & (lo <= 0) & (hi >= 0) & (np.maximum(np.abs(lo), np.abs(hi)) < 0.5)
    assert (two & (lo > 0)).any() and (two & (hi < 0)).any() and narrow.any() and (narrow & (lo < 0) & (hi > 0)).any()
    assert (two & (lo <= 0) & (hi >= 0) & ~narrow).any() and np.isinf(lo).any() and np.isinf(hi).any()
    assert np.abs(lo[~np.isinf(lo)]).max() == 38.0 and np.abs(hi[~np.isinf(hi)]).max() == 38.0 and (hi - lo).min() >= 1e-3 * (1 - 1e-11)  # (38 + 1e-3 - 38)
    # the tolerance: 8 x the deviation of two independent float64 formulations on this grid, which the reference's own two-term form
    # must stay inside
    measured = lr.deviation(alt, ref).max()
    print("reference against the second formulation: %.3e (recorded %.3e)" % (measured, lr.LOGDENS_MEASURED_DEVIATION))
    assert measured <= 1.05 * lr.LOGDENS_MEASURED_DEVIATION and lr.LOGDENS_RTOL == 8 * lr.LOGDENS_MEASURED_DEVIATION
    got = np.array([_interval_value(a, b) for a, b in zip(lo, hi)])
    assert np.isfinite(got).all()
    dev = lr.deviation(got, ref)
    print("value function against the reference: %.3e, one-sided %.3e" % (dev.max(), dev[one_sided].max()))
    assert dev.max() <= lr.LOGDENS_RTOL


def test_log_phi_keeps_relative_accuracy_in_both_tails():
    """one-sided labels, |score| to 36 (beyond, Phi(-x) is a denormal): relative to |l| alone, also where l -> 0"""
    from myfm_amd import _myfm

    xs = np.concatenate([np.linspace(-36.0, 36.0, 1441), [-1e-300, 0.0, 1e-300]])
    for label in (1.0, 0.0):
        got = np.array([_myfm.log_density_value(1, label, x) for x in xs])
        ref = log_ndtr(xs if label else -xs)
        assert np.all(np.abs(got - ref) <= lr.LOGDENS_RTOL * np.abs(ref))
    for x in (-38.0, 38.0, -40.0, 40.0):  # finite where Phi underflows, and equal to log_ndtr within the tolerance
        got = _myfm.log_density_value(1, 1.0, x)
        assert np.isfinite(got) and lr.deviation(got, log_ndtr(x)) <= lr.LOGDENS_RTOL


def test_regression_and_ordered_values():
    from myfm_amd import _myfm

    rng = np.random.default_rng(4)
    for _ in range(50):
        y, f, alpha = rng.normal() * 3, rng.normal() * 3, float(np.exp(rng.uniform(-3, 6)))
        got = _myfm.log_density_value(0, y, f, 0.5 * np.log(alpha) - lr.HALF_LOG_2PI, np.sqrt(alpha))
        assert lr.deviation(got, lr.log_lik([[f]], [y], 0, [alpha])[0, 0]) <= lr.LOGDENS_RTOL
    cut = np.array([-1.5, -0.5, 0.5, 1.5])
    for f in (-31.5, -3.0, -0.2, 0.0, 0.7, 4.0, 31.5):  # (-31.5 with the top label: the score 30 below the lowest cutpoint)
        for label in range(5):
            got = _myfm.log_density_value(2, float(label), f, 0.0, 0.0, cut)
            assert np.isfinite(got) and lr.deviation(got, lr.log_lik([[f]], [label], 2, cutpoints=cut[None, :])[0, 0]) <= lr.LOGDENS_RTOL
    with pytest.raises(ValueError):
        _myfm.log_density_value(3, 0.0, 0.0)
    with pytest.raises(ValueError):
        _myfm.log_density_value(2, 5.0, 0.0, 0.0, 0.0, cut)


# ---- (c) refusals on the host ----------------------------------------------------------------------------------------------------------
D, K, S = 12, 3, 2
CUTS = [np.array([-1.0, 0.0, 1.5]), np.array([-0.5, 0.25, 2.0])]
X3 = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, D))


def _restored(cls, task, cuts=None):
    """an estimator around a Predictor restored through __setstate__ (no fit, no device)"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for s in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), [] if cuts is None else [cuts[s]]))
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
    """what every task refuses, at the estimator and at predictor_ (task: the integer, kw: a valid call's constants)"""
    import myfm_amd

    p = est.predictor_
    with pytest.raises(ValueError, match="one value per row"):
        est.predict_log_density(X3, y[:2])
    with pytest.raises(ValueError, match="one value per row"):
        est.predict_log_density(X3, np.stack([y, y]))
    with pytest.raises(ValueError, match="one value per row"):
        p.predict_log_density(X3, [], y[:2], task, **kw)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            est.predict_log_density(X3, np.array([y[0], bad, y[2]]))
        with pytest.raises(ValueError, match="finite"):
            p.predict_log_density(X3, [], np.array([y[0], bad, y[2]]), task, **kw)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        est.predict_log_density(X3[:, :11], y)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        p.predict_log_density(X3[:, :11], [], y, task, **kw)
    with pytest.raises(ValueError, match="X and X_rel have different shape"):
        est.predict_log_density(X3[:, :8], y, [myfm_amd.RelationBlock([0, 1], sps.csr_matrix(np.eye(4)))])
    for bad_task in (-1, 3):
        with pytest.raises(ValueError, match="bad task"):
            p.predict_log_density(X3, [], y, bad_task, **kw)
    with pytest.raises(ValueError, match="does not match"):
        p.predict_log_density(X3, [], y, (task + 1) % 3, **kw)
    for name in ("tile_rows", "chunk_samples"):
        with pytest.raises(ValueError, match="non-negative"):
            p.predict_log_density(X3, [], y, task, **kw, **{name: -1})


@pytest.mark.parametrize("cls", ["MyFMRegressor", "MyFMGibbsRegressor"])
def test_regression_refusals_need_no_gpu(cls):
    est = _restored(cls, "REGRESSION")
    p, y = est.predictor_, np.array([0.5, -1.0, 2.0])
    with pytest.raises(RuntimeError, match="history_"):  # no history at all: the RuntimeError of predict_dist(noise=True)
        est.predict_log_density(X3, y)
    est.history_ = _history([1.0])  # ... and one that is shorter than the two kept samples
    with pytest.raises(RuntimeError, match="history_"):
        est.predict_log_density(X3, y)
    for bad in (0.0, -1.0, np.inf, np.nan):
        est.history_ = _history([1.0, bad])
        with pytest.raises(ValueError, match="positive and finite"):
            est.predict_log_density(X3, y)
        with pytest.raises(ValueError, match="positive and finite"):
            p.predict_log_density(X3, [], y, 0, precisions=np.array([1.0, bad]))
    with pytest.raises(ValueError, match="needs the noise precision"):
        p.predict_log_density(X3, [], y, 0)
    with pytest.raises(ValueError, match="one value per kept sample"):
        p.predict_log_density(X3, [], y, 0, precisions=np.ones(3))
    with pytest.raises(ValueError, match="ordered probit only"):
        p.predict_log_density(X3, [], y, 0, precisions=np.ones(2), cutpoints=np.zeros((2, 1)))
    est.history_ = _history([9.0, 1.0, 2.0])  # (the last two are the kept samples')
    _common_refusals(est, 0, y, precisions=np.array([1.0, 2.0]))
    if _no_device():  # valid arguments: the usual refusal of a machine without a GPU comes only now
        for pointwise in (False, True):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.predict_log_density(X3, y, pointwise=pointwise)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.predict_log_density(X3, [], y, 0, precisions=np.array([1.0, 2.0]))


@pytest.mark.parametrize("cls", ["MyFMClassifier", "MyFMGibbsClassifier"])
def test_classification_refusals_need_no_gpu(cls):
    est = _restored(cls, "CLASSIFICATION")
    p, y = est.predictor_, np.array([0.0, 1.0, 1.0])
    for bad in (2.0, -1.0, 0.5):
        with pytest.raises(ValueError, match="0 or 1"):
            est.predict_log_density(X3, np.array([0.0, bad, 1.0]))
        with pytest.raises(ValueError, match="0 or 1"):
            p.predict_log_density(X3, [], np.array([0.0, bad, 1.0]), 1)
    with pytest.raises(ValueError, match="regression only"):
        p.predict_log_density(X3, [], y, 1, precisions=np.ones(2))
    with pytest.raises(ValueError, match="ordered probit only"):
        p.predict_log_density(X3, [], y, 1, cutpoints=np.zeros((2, 1)))
    with pytest.raises(TypeError):
        est.predict_log_density(X3, y, cutpoint_index=0)
    _common_refusals(est, 1, y)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_log_density(X3, np.array([False, True, True]))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.predict_log_density(X3, [], y, 1, pointwise=True)


def test_ordered_refusals_need_no_gpu():
    est = _restored("MyFMOrderedProbit", "ORDERED", CUTS)
    p, y = est.predictor_, np.array([0, 3, 2])
    for bad in (4, -1, 1.5):  # three cutpoints: the labels are 0 .. 3
        with pytest.raises(ValueError, match="integers in"):
            est.predict_log_density(X3, np.array([0, bad, 1]))
        with pytest.raises(ValueError, match="integers in"):
            p.predict_log_density(X3, [], np.array([0, bad, 1], dtype=np.float64), 2, cutpoints=0)
    with pytest.raises(ValueError, match="needs the samples' cutpoints"):
        p.predict_log_density(X3, [], y, 2)
    with pytest.raises(ValueError, match="regression only"):
        p.predict_log_density(X3, [], y, 2, precisions=np.ones(2), cutpoints=0)
    with pytest.raises(ValueError, match="out of range"):
        est.predict_log_density(X3, y, cutpoint_index=1)
    with pytest.raises(ValueError, match="must be an integer"):
        est.predict_log_density(X3, y, cutpoint_index=0.0)
    with pytest.raises(ValueError, match="shape"):
        p.predict_log_density(X3, [], y, 2, cutpoints=np.zeros((3, 3)))
    for bad in ([[-1.0, np.nan, 1.0], [0.0, 1.0, 2.0]], [[-1.0, 0.0, 1.0], [0.0, 2.0, 1.0]], [[-1.0, 0.0, np.inf], [0.0, 1.0, 2.0]]):
        with pytest.raises(ValueError, match="finite and ascending"):
            p.predict_log_density(X3, [], y, 2, cutpoints=np.array(bad))
    for cuts in ([CUTS[0], np.array([0.5, 0.25, 2.0])], [np.array([-1.0, np.nan, 1.5]), CUTS[1]]):  # ... and held by the model
        broken = _restored("MyFMOrderedProbit", "ORDERED", cuts)
        with pytest.raises(ValueError, match="finite and ascending"):
            broken.predict_log_density(X3, y)
    ragged = _restored("MyFMOrderedProbit", "ORDERED", [CUTS[0], CUTS[1][:2]])
    with pytest.raises(ValueError, match="inconsistent cutpoint sizes"):
        ragged.predict_log_density(X3, np.array([0, 1, 2]))
    _common_refusals(est, 2, y.astype(np.float64), cutpoints=0)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_log_density(X3, y, pointwise=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            p.predict_log_density(X3, [], y, 2, cutpoints=np.stack(CUTS))


# ---- (d) exports ---------------------------------------------------------------------------------------------------------------------------
def test_who_has_the_method():
    import myfm_amd

    assert myfm_amd.PointwiseDensity._fields == ("lpd", "log_lik_mean", "log_lik_var", "pit", "log_lik")
    assert "PointwiseDensity" in myfm_amd.__all__
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.MyFMRegressor,
                myfm_amd.MyFMClassifier):
        assert callable(cls.predict_log_density)
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_log_density")
    assert callable(myfm_amd._myfm.Predictor.predict_log_density) and callable(myfm_amd._myfm.log_density_value)
    assert not hasattr(myfm_amd._myfm.VariationalPredictor, "predict_log_density")
    for cls, y in ((myfm_amd.MyFMRegressor, [0.5]), (myfm_amd.MyFMClassifier, [1]), (myfm_amd.MyFMOrderedProbit, [1])):
        with pytest.raises(RuntimeError, match="Predictor called before fit"):
            cls(2).predict_log_density(sps.csr_matrix((1, 3)), y)


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_design_logdens_store", "mfm_design_logdens", "mfm_logdens_value"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.Design.log_density) and callable(_capi.Store.log_density)
