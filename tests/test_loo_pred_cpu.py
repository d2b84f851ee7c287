"""predict_loo_dist and predict_loo_crps, the parts that need no GPU: the host hooks _myfm.loo_summary_row and
_myfm.loo_crps_row (one row through the scalar pieces of the kernels, in their orders) against the NumPy reference of
tests/loo_pred_ref.py and its higher-precision twin, identities and edge rows, loo_residuals and crps_summary, the refusals that are
raised before the device is looked for, and the exports."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import loo_pred_ref as lr
from tests import psis_ref as pr
from tests.test_loo_cpu import CUTS, X3, _history, _no_device, _restored

Q = np.asarray(lr.QUANTILES)


def summary_row(v, lw, quantiles=Q, inv_alpha=None):
    from myfm_amd import _myfm

    return _myfm.loo_summary_row(v, lw, np.asarray(quantiles, dtype=np.float64), inv_alpha)


def crps_row(c, t, lw=None):
    from myfm_amd import _myfm

    return np.array(_myfm.loo_crps_row(c["task"], c["y"][t], c["f"][:, t], (c["lw"] if lw is None else lw)[:, t], c["prec"], c["cut"]))


# ---- (a) the reference, its twin and the host rows ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    return lr.measured_deviation()


def test_the_recorded_deviations_have_not_grown(measured):
    """float64 reference / twin over tolerance_cases() and summary_only_cases(); no more than 1 % of a case's quantile cells lie
    within NEAR of a running sum"""
    moments, moments_large, quantiles, crps, left_out = measured
    print("measured float64 / twin deviation: moments %.3g (S <= %d) and %.3g (above), quantiles %.3g, crps %.3g; cells left out at most %.3g"
          % (moments, lr.LOO_LARGE_S, moments_large, quantiles, crps, left_out))
    assert moments <= lr.LOO_MEASURED_DEVIATION_MOMENTS
    assert moments_large <= lr.LOO_MEASURED_DEVIATION_MOMENTS_LARGE
    assert quantiles <= lr.LOO_MEASURED_DEVIATION_QUANTILES
    assert crps <= lr.LOO_MEASURED_DEVIATION_CRPS
    assert left_out <= lr.MAX_LEFT_OUT


def test_the_host_rows_match_the_reference_and_its_twin():
    """every row of tolerance_cases(): weights from psis_ref.psis on the rows' own log likelihoods"""
    for c in lr.tolerance_cases():
        ia = lr.inv_alpha_of(c)
        refs = []
        for hp in (False, True):
            v = lr.values(c["task"], c["f"], c["cut"], hp)
            s = lr.summary(v, c["lw"], Q, ia, hp)
            k = lr.crps(c["task"], c["f"], c["lw"], c["y"], c["prec"], c["cut"], hp)
            refs.append(([None if a is None else np.asarray(a, dtype=np.float64) for a in s[:5]], s[5], np.stack(k).astype(np.float64)))
        v64 = lr.values(c["task"], c["f"], c["cut"])
        keep = ~(refs[0][1] | refs[1][1])
        for t in range(v64.shape[1]):
            mean, sd, q, sd_y, ess = summary_row(v64[:, t], c["lw"][:, t], Q, ia)
            got_k = crps_row(c, t)
            assert (sd_y is None) == (c["task"] != 0)
            for s, _, k in refs:
                for got, want in ((mean, s[0]), (sd, s[1]), (ess, s[4])) + (((sd_y, s[3]),) if sd_y is not None else ()):
                    assert lr.deviation(got, want[t]) <= lr.LOO_RTOL_MOMENTS, (c["task"], c["f"].shape, t)
                assert np.all(lr.deviation(q, s[2][:, t])[keep[:, t]] <= lr.LOO_RTOL_QUANTILES), (c["task"], c["f"].shape, t)
                assert np.all(lr.deviation(got_k, k[:, t]) <= lr.LOO_RTOL_CRPS), (c["task"], c["f"].shape, t)
            assert got_k[0] >= 0.0
            if c["task"] == 0:
                assert got_k[0] == got_k[1] - got_k[2]  # accuracy - spread == crps


def test_equal_weights_give_the_crps_of_predict_crps():
    """lw = -log S: the formula of predict_crps term for term"""
    from myfm_amd import _myfm

    for task in (0, 1, 2):
        for S in (1, 5, 33):
            c = lr.random_case(task, S, 4, 70 + task)
            lw = np.full((S, 4), -np.log(S))
            for t in range(4):
                want = np.array(_myfm.crps_row(task, c["y"][t], c["f"][:, t], c["prec"], c["cut"]))
                assert np.all(lr.deviation(crps_row(c, t, lw), want) <= lr.LOO_RTOL_CRPS), (task, S, t)


def test_equal_samples():
    """all samples alike: the summary is that value whatever the weights, std 0 up to the rounding of the mean; loo_crps_row equals
    crps_row"""
    from myfm_amd import _myfm

    for task in (0, 1, 2):
        c = lr.random_case(task, 9, 5, 80 + task, equal=True)
        v = lr.values(task, c["f"], c["cut"])
        for t in range(5):
            mean, sd, q, _, ess = summary_row(v[:, t], c["lw"][:, t])
            assert lr.deviation(mean, v[0, t]) <= lr.LOO_RTOL_MOMENTS and sd <= lr.LOO_RTOL_MOMENTS * max(1.0, abs(v[0, t]))
            assert np.all(q == v[0, t]) and lr.deviation(ess, 9.0) <= lr.LOO_RTOL_MOMENTS
            want = np.array(_myfm.crps_row(task, c["y"][t], c["f"][:, t], c["prec"], c["cut"]))
            assert np.all(lr.deviation(crps_row(c, t), want) <= lr.LOO_RTOL_CRPS)


def test_a_single_sample_row():
    from myfm_amd import _myfm

    mean, sd, q, sd_y, ess = summary_row(np.array([1.25]), np.array([0.0]), (0.0, 0.3, 1.0), np.array([4.0]))
    assert mean == 1.25 and sd == 0.0 and np.all(q == 1.25) and sd_y == 2.0 and ess == 1.0
    out = _myfm.loo_crps_row(0, 0.5, np.array([1.25]), np.array([0.0]), np.array([0.25]), None)
    assert out == _myfm.crps_row(0, 0.5, np.array([1.25]), np.array([0.25]), None)


def test_a_row_with_a_density_of_zero_is_nan_everywhere():
    ll = pr.normal_tails(40, 2, 1.0, 4)
    ll[7, 1] = -np.inf
    elpd, k, lw = pr.psis(ll)
    assert np.isposinf(k[1]) and np.all(np.isnan(lw[:, 1]))
    v = np.random.default_rng(1).normal(size=40)
    mean, sd, q, sd_y, ess = summary_row(v, lw[:, 1], Q, np.ones(40))
    assert np.isnan(mean) and np.isnan(sd) and np.all(np.isnan(q)) and np.isnan(sd_y) and np.isnan(ess)
    ref = lr.summary(v[:, None], lw[:, 1:], Q, np.ones(40))
    assert all(np.all(np.isnan(a)) for a in ref[:5])
    c = dict(task=0, y=np.zeros(1), f=v[:, None], prec=np.ones(40), cut=None, lw=lw[:, 1:])
    assert np.all(np.isnan(crps_row(c, 0)))
    mean, sd, q, sd_y, ess = summary_row(v, lw[:, 0], Q, np.ones(40))  # ... and its neighbour is finite
    assert np.isfinite(mean) and np.all(np.isfinite(q))


def test_the_quantile_rule_by_hand():
    """v = 3, 1, 2 with weights 0.5, 0.2, 0.3: ordered 1, 2, 3 with running sums 0.2, 0.5, 1"""
    v, w = np.array([3.0, 1.0, 2.0]), np.array([0.5, 0.2, 0.3])
    probs = (0.0, 0.1, 0.2, 0.35, 0.5, 0.75, 1.0)
    q = summary_row(v, np.log(w), probs)[2]
    c = np.cumsum(w[[1, 2, 0]])
    want = [1.0, 1.0, 1.0, 1.0 + (0.35 - c[0]) / (c[1] - c[0]), 2.0, 2.0 + (0.75 - c[1]) / (c[2] - c[1]), 3.0]
    assert np.all(np.abs(q - want) <= 4 * np.finfo(np.float64).eps * 3.0)
    assert q[0] == 1.0 and q[1] == 1.0  # p = 0 and any p below the first weight: the smallest value itself
    assert np.array_equal(summary_row(v, np.log(w), probs[::-1])[2], q[::-1])  # in the caller's order
    assert np.all(np.abs(lr.summary(v[:, None], np.log(w)[:, None], probs)[2][:, 0] - want) <= 4 * np.finfo(np.float64).eps * 3.0)


def test_ties_resolve_by_sample_index():
    """two equal values: the one with the smaller sample index comes first in the order, so its weight is the first step"""
    v = np.array([2.0, 1.0, 1.0, 0.0])
    for w in (np.array([0.1, 0.6, 0.1, 0.2]), np.array([0.1, 0.1, 0.6, 0.2])):
        lw = np.log(w)
        q = summary_row(v, lw, (0.25, 0.5, 0.85))[2]
        want = lr.summary(v[:, None], lw[:, None], (0.25, 0.5, 0.85))[2][:, 0]
        assert np.all(lr.deviation(q, want) <= lr.LOO_RTOL_QUANTILES)
    # order (0, s3), (1, s1), (1, s2), (2, s0); weights 0.2, 0.6, 0.1, 0.1: c = 0.2, 0.8, 0.9, 1; p = 0.25 falls in s1's step
    q = summary_row(v, np.log(np.array([0.1, 0.6, 0.1, 0.2])), (0.25,))[2]
    assert abs(q[0] - (0.25 - 0.2) / 0.6) <= 1e-15
    # weights 0.2, 0.1, 0.6, 0.1: c = 0.2, 0.3, 0.9, 1; p = 0.25 falls in s1's step of 0.1
    q = summary_row(v, np.log(np.array([0.1, 0.1, 0.6, 0.2])), (0.25,))[2]
    assert abs(q[0] - (0.25 - 0.2) / 0.1) <= 1e-14


# ---- (b) loo_residuals and crps_summary --------------------------------------------------------------------------------------------
def test_loo_residuals_on_hand_made_arrays():
    from myfm_amd import LooPredictive
    from myfm_amd.utils import evaluation as ev

    y = np.array([1.0, 2.0, 3.0, 6.0])
    mean = np.array([0.0, 2.0, 4.0, 4.0])
    quant = np.array([[0.5, 0.0, 3.5, 0.0], [1.0, 2.0, 4.0, 5.0], [1.5, 3.0, 5.0, 6.0]])
    res = LooPredictive(mean, np.ones(4), quant, np.array([1.0, 2.0, 0.5, 4.0]), np.full(4, 10.0), np.zeros(4))
    out = ev.loo_residuals(res, y, interval=(0, 2))
    r = np.array([1.0, 0.0, -1.0, 2.0])
    assert np.array_equal(out["residuals"], r) and out["rmse"] == np.sqrt(1.5) and out["mae"] == 1.0
    assert out["r2"] == 1.0 - np.var(r) / np.var(y)
    assert np.array_equal(out["standardized"], r / np.array([1.0, 2.0, 0.5, 4.0]))
    assert out["coverage"] == 0.75  # rows 0, 1, 3 inside, row 2 (3 < 3.5) outside
    plain = ev.loo_residuals(LooPredictive(mean, np.ones(4), quant, None, np.full(4, 10.0), np.zeros(4)), y)
    assert plain["standardized"] is None and plain["coverage"] is None and plain["rmse"] == out["rmse"]
    for bad in ((0, 3), (-1, 2), (0.0, 2), (True, 2)):
        with pytest.raises(ValueError, match="interval"):
            ev.loo_residuals(res, y, interval=bad)
    with pytest.raises(ValueError, match="one value per row"):
        ev.loo_residuals(res, y[:3])


def test_crps_summary_takes_a_loo_crps():
    from myfm_amd import CrpsScore, LooCrps
    from myfm_amd.utils.evaluation import crps_summary

    parts = (np.array([1.0, 2.0, 3.0, 6.0]), np.array([2.0, 3.0, 4.0, 7.0]), np.array([1.0, 1.0, 1.0, 1.0]))
    loo = LooCrps(*parts, np.array([0.1, 0.2, 0.8, np.inf]))
    assert crps_summary(loo) == crps_summary(CrpsScore(*parts))
    assert crps_summary(loo, CrpsScore(parts[0] * 2, None, None))["skill"] == 0.5


# ---- (c) refusals on the host ------------------------------------------------------------------------------------------------------
def _models():
    reg = _restored("MyFMGibbsRegressor", "REGRESSION")
    reg.history_ = _history([9.0, 1.0, 2.0])
    return [(reg, np.array([0.5, -1.0, 2.0]), {}), (_restored("MyFMGibbsClassifier", "CLASSIFICATION"), np.array([0.0, 1.0, 1.0]), {}),
            (_restored("MyFMOrderedProbit", "ORDERED", CUTS), np.array([0, 3, 2]), dict(cutpoint_index=0))]


def _same_error(est, method, args, kwargs):
    """the method raises what predict_loo raises for these arguments, with the same message"""
    with pytest.raises((ValueError, RuntimeError)) as want:
        est.predict_loo(*args, **kwargs)
    with pytest.raises(type(want.value)) as got:
        getattr(est, method)(*args, **kwargs)
    assert str(got.value) == str(want.value).replace("predict_loo", method)


@pytest.mark.parametrize("method", ["predict_loo_dist", "predict_loo_crps"])
def test_shared_refusals_are_predict_loos(method):
    for est, y, kw in _models():
        for bad in (0, 0.0, -1.0, np.nan, np.inf, True, "1", None, [1.0]):
            _same_error(est, method, (X3, y), dict(r_eff=bad, **kw))
        _same_error(est, method, (X3, y[:2]), kw)
        _same_error(est, method, (X3, np.array([y[0], np.nan, y[2]], dtype=np.float64)), kw)
        _same_error(est, method, (X3[:, :11], y), kw)
        p, task = est.predictor_, int(est._task_type)
        own = dict(precisions=np.ones(2) if task == 0 else None, cutpoints=0 if task == 2 else None)
        for name in ("tile_rows", "chunk_samples"):
            with pytest.raises(ValueError, match="non-negative"):
                getattr(p, method)(X3, [], np.asarray(y, dtype=np.float64), task, **own, **{name: -1})
        with pytest.raises(ValueError, match="does not match"):
            getattr(p, method)(X3, [], np.asarray(y, dtype=np.float64), (task + 1) % 3)
        with pytest.raises(ValueError, match="r_eff"):
            getattr(p, method)(X3, [], np.asarray(y, dtype=np.float64), task, r_eff=0.0, **own)
        if _no_device():  # valid arguments: the usual refusal of a machine without a GPU comes only now
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                getattr(est, method)(X3, y, r_eff=0.5, **kw)
    no_history = _restored("MyFMGibbsRegressor", "REGRESSION")
    with pytest.raises(RuntimeError, match="%s needs history_" % method):
        getattr(no_history, method)(X3, np.array([0.5, -1.0, 2.0]))
    with pytest.raises(TypeError):
        getattr(_models()[1][0], method)(X3, np.array([0.0, 1.0, 1.0]), cutpoint_index=0)


def test_bad_quantiles_are_refused_as_predict_dist_refuses_them():
    for est, y, kw in _models():
        p, task = est.predictor_, int(est._task_type)
        own = dict(precisions=np.ones(2) if task == 0 else None, cutpoints=0 if task == 2 else None)
        for bad, msg in (((0.5, 1.5), r"must lie in \[0, 1\]"), ((-0.1,), r"must lie in \[0, 1\]"), ((np.nan,), r"must lie in \[0, 1\]"),
                         (np.zeros((2, 2)), "1-D sequence"), (np.linspace(0, 1, 33), "at most 32 quantiles per call")):
            with pytest.raises(ValueError, match=msg):
                est.predict_loo_dist(X3, y, quantiles=bad, **kw)
            with pytest.raises(ValueError, match=msg):
                p.predict_loo_dist(X3, [], np.asarray(y, dtype=np.float64), task, quantiles=bad, **own)
        if _no_device():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.predict_loo_dist(X3, y, quantiles=np.linspace(0, 1, 32), **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.predict_loo_dist(X3, y, quantiles=(), **kw)


def test_the_sample_limits():
    y = np.array([0.0, 1.0, 1.0])
    many = _restored("MyFMGibbsClassifier", "CLASSIFICATION", n_samples=4097)
    for method in ("predict_loo_dist", "predict_loo_crps"):
        with pytest.raises(ValueError, match="at most 4096 kept samples, this model keeps 4097"):
            getattr(many, method)(X3, y)
        with pytest.raises(ValueError, match="at most 4096 kept samples, this model keeps 4097"):
            getattr(many.predictor_, method)(X3, [], y, 1)
    reg = _restored("MyFMGibbsRegressor", "REGRESSION", n_samples=1025)
    reg.history_ = _history(np.ones(1025))
    yr = np.array([0.5, -1.0, 2.0])
    with pytest.raises(ValueError, match="a regression CRPS is computed over at most 1024 kept samples, this model keeps 1025"):
        reg.predict_loo_crps(X3, yr)
    with pytest.raises(ValueError, match="a regression CRPS is computed over at most 1024 kept samples, this model keeps 1025"):
        reg.predictor_.predict_loo_crps(X3, [], yr, 0, precisions=np.ones(1025))
    if _no_device():  # the summary of 1025 samples and the class CRPS of 1025 are valid
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            reg.predict_loo_dist(X3, yr)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _restored("MyFMOrderedProbit", "ORDERED", [CUTS[0]] * 1025, n_samples=1025).predict_loo_crps(X3, np.array([0, 3, 2]))


def test_the_host_rows_refuse():
    from myfm_amd import _myfm

    v, lw = np.zeros(5), np.full(5, -np.log(5))
    with pytest.raises(ValueError, match="at most 32 quantiles"):
        _myfm.loo_summary_row(v, lw, np.linspace(0, 1, 33))
    with pytest.raises(ValueError, match="out of range"):
        _myfm.loo_summary_row(v, lw, np.array([1.5]))
    with pytest.raises(ValueError, match="4096"):
        _myfm.loo_summary_row(np.zeros(4097), np.zeros(4097))
    with pytest.raises(ValueError):
        _myfm.loo_summary_row(v, lw[:4])
    with pytest.raises(ValueError, match="finite"):
        _myfm.loo_summary_row(np.array([0.0, np.nan]), lw[:2])
    with pytest.raises(ValueError, match="at most 1024 samples, got 1025"):
        _myfm.loo_crps_row(0, 0.0, np.zeros(1025), np.zeros(1025), np.ones(1025), None)
    with pytest.raises(ValueError):
        _myfm.loo_crps_row(0, 0.0, v, lw[:4], np.ones(5), None)


# ---- (d) exports -------------------------------------------------------------------------------------------------------------------
def test_who_has_the_methods():
    import myfm_amd

    assert myfm_amd.LooPredictive._fields == ("mean", "std", "quantiles", "std_y", "ess", "pareto_k")
    assert myfm_amd.LooCrps._fields == ("crps", "accuracy", "spread", "pareto_k")
    assert "LooPredictive" in myfm_amd.__all__ and "LooCrps" in myfm_amd.__all__
    for name in ("predict_loo_dist", "predict_loo_crps"):
        for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.MyFMRegressor,
                    myfm_amd.MyFMClassifier):
            assert callable(getattr(cls, name))
        for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier, myfm_amd._myfm.VariationalPredictor):
            assert not hasattr(cls, name)
        assert callable(getattr(myfm_amd._myfm.Predictor, name))
        with pytest.raises(RuntimeError, match="Predictor called before fit"):
            getattr(myfm_amd.MyFMRegressor(2), name)(sps.csr_matrix((1, 3)), [0.5])
    assert callable(myfm_amd._myfm.loo_summary_row) and callable(myfm_amd._myfm.loo_crps_row)
    assert "np.quantile" in myfm_amd.MyFMGibbsRegressor.predict_loo_dist.__doc__


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_design_loo_summary_store", "mfm_design_loo_summary", "mfm_design_loo_crps_store", "mfm_design_loo_crps",
                 "mfm_loo_summary_row", "mfm_loo_crps_row"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    for cls in (_capi.Design, _capi.Store):
        assert callable(cls.loo_summary) and callable(cls.loo_crps)
