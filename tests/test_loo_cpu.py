"""predict_loo, the parts that need no GPU: identities of the NumPy reference (tests/psis_ref.py), the host hook
_myfm.psis_row (one row through the scalar pieces of the kernel) against that reference in longdouble, loo / compare of
myfm_amd.utils.evaluation, the refusals that are raised before the device is looked for, and the exports."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse as sps

from tests import psis_ref as pr


def lse(a):
    mx = np.max(a)
    return mx + np.log(np.sum(np.exp(a - mx)))


# ---- (a) identities of the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 20])
def test_a_short_tail_gives_the_harmonic_mean(S):
    """M = ceil(min(0.2 S, 3 sqrt S)) < 5 up to S = 20 (21 .. 24 give ceil(4.2 .. 4.8) = 5: fitted): the raw ratios"""
    assert pr.tail_len(S) < 5 and pr.tail_len(21) == 5 and pr.tail_len(24) == 5 and pr.tail_len(25) == 5 and pr.tail_len(26) == 6
    ll = pr.normal_tails(S, 3, 1.0, S)
    elpd, k, lw = pr.psis(ll)
    assert np.all(np.isposinf(k))
    want = np.array([-(lse(-ll[:, t]) - np.log(S)) for t in range(3)])
    assert np.all(pr.deviation(elpd, want) <= 4 * (S + 8) * np.finfo(np.float64).eps)  # (two log-sum-exps over S terms)


def test_tail_lengths():
    assert pr.tail_len(95) == 19 and pr.tail_len(4096) == 192 and pr.tail_len(4096, 0.05) == 820 and pr.tail_len(1000, 2.5) == 60
    assert 30 + int(np.sqrt(820)) == 58  # the widest grid: a grid point per lane of a wavefront


def test_the_weights_sum_to_one():
    for name, ll, r_eff in pr.cpu_cases():
        elpd, k, lw = pr.psis(ll, r_eff)
        ok = ~np.isnan(lw[0])
        assert np.all(np.abs(np.exp(lw[:, ok]).sum(axis=0) - 1.0) <= 64 * ll.shape[0] * np.finfo(np.float64).eps), name
        assert np.all(lw[:, ok] <= 0.0)


def test_a_constant_row_is_not_fitted():
    elpd, k, lw = pr.psis(np.full((101, 2), -1.25))
    assert np.all(np.isposinf(k)) and np.all(pr.deviation(elpd, -1.25) <= 64 * np.finfo(np.float64).eps)
    assert np.all(pr.deviation(lw, -np.log(101.0)) <= 64 * np.finfo(np.float64).eps)


def test_a_density_of_zero_under_one_sample():
    ll = pr.normal_tails(40, 2, 1.0, 4)
    ll[7, 1] = -np.inf
    elpd, k, lw = pr.psis(ll)
    assert np.isneginf(elpd[1]) and np.isposinf(k[1]) and np.all(np.isnan(lw[:, 1]))
    assert np.isfinite(elpd[0]) and np.isfinite(k[0]) and np.all(np.isfinite(lw[:, 0]))


def test_ties_are_broken_by_sample_index():
    """two equal ratios on either side of the cutoff: the one with the larger sample index belongs to the tail, as if its l were a
    hair smaller"""
    S = 101
    M = pr.tail_len(S)
    base = pr.normal_tails(S, 1, 1.0, 11)[:, 0]
    order = np.argsort(-base, kind="stable")  # ratios ascending
    a, b = sorted((int(order[S - M - 1]), int(order[S - M])))
    tie = base.copy()
    tie[a] = tie[b] = base[order[S - M - 1]]
    nudged = {}
    for which in (a, b):
        ll = tie.copy()
        ll[which] -= 1e-10  # the larger ratio: strictly inside the tail
        nudged[which] = pr.psis(ll[:, None])[2][:, 0]
    lw = pr.psis(tie[:, None])[2][:, 0]
    assert abs(nudged[b][a] - nudged[b][b]) > 1e-3  # the cutoff value and the smoothed first tail value differ visibly
    assert np.all(np.abs(lw - nudged[b]) < 1e-6) and abs(lw[a] - nudged[a][a]) > 1e-3


def test_an_exact_pareto_sample_returns_its_shape():
    """|k^ - k| <= 4 (1 + k) / sqrt(n) + |5 - 10 k| / (n + 10). The first term is four asymptotic standard deviations of the maximum
    likelihood estimate of the shape, (1 + k) / sqrt(n) (Smith 1987, Estimating tails of probability distributions, Ann. Statist. 15,
    for k > -1/2), which Zhang and Stephens (2009, Technometrics 51, section 4 and table 1) report their estimator to match in
    efficiency over k in [-0.5, 1]; the second is the shift of the loo package's prior (n k + 5) / (n + 10) away from k."""
    n = 820
    rng = np.random.default_rng(2024)
    for k in (-0.3, 0.0, 0.3, 0.7, 1.0):
        x = np.sort(pr.gpd_sample(k, 2.0, n, rng))[:, None]
        khat, sigma = pr.gpd_fit(x)
        assert abs(khat[0] - k) <= 4 * (1 + k) / np.sqrt(n) + abs(5 - 10 * k) / (n + 10), (k, khat)
        assert abs(sigma[0] - 2.0) <= 0.5


# ---- (b) the host hook against the longdouble reference ---------------------------------------------------------------------------
def test_psis_row_matches_the_longdouble_reference():
    """every row of cpu_cases(): S in {1, 5, 20, 21, 24, 25, 26, 95, 101, 1000, 4096} x r_eff in {1, 0.05, 2.5} x four spreads of the
    ratios, a tail of equal pairs, two degenerate tails, a constant row and a row with an l of -inf. The deviation between the
    float64 and the longdouble reference is measured again and has not grown past the recorded constants."""
    from myfm_amd import _myfm

    measured_e = measured_k = 0.0
    n_fitted = 0
    for name, ll, r_eff in pr.cpu_cases():
        e64, k64, w64 = pr.psis(ll, r_eff)
        eL, kL, wL = (np.asarray(v, dtype=np.float64) for v in pr.psis(ll, r_eff, np.longdouble))
        assert np.array_equal(np.isposinf(k64), np.isposinf(kL)) and np.array_equal(np.isnan(w64), np.isnan(wL)), name
        fin = np.isfinite(kL)
        n_fitted += int(fin.sum())
        ok = ~np.isnan(wL[0])
        measured_e = max(measured_e, pr.deviation(e64, eL).max(), pr.deviation(w64[:, ok], wL[:, ok]).max() if ok.any() else 0.0)
        measured_k = max(measured_k, pr.deviation(k64[fin], kL[fin]).max() if fin.any() else 0.0)
        for t in range(ll.shape[1]):
            elpd, k, lw = _myfm.psis_row(ll[:, t], r_eff)
            assert lw.shape == (ll.shape[0],)
            if not ok[t]:
                assert np.isneginf(elpd) and np.isposinf(k) and np.all(np.isnan(lw)), (name, t)
                continue
            assert np.isposinf(k) == np.isposinf(kL[t]), (name, t)
            assert pr.deviation(elpd, eL[t]) <= pr.PSIS_RTOL_ELPD, (name, t, elpd, eL[t])
            assert np.all(pr.deviation(lw, wL[:, t]) <= pr.PSIS_RTOL_ELPD), (name, t)
            if fin[t]:
                assert pr.deviation(k, kL[t]) <= pr.PSIS_RTOL_K, (name, t, k, kL[t])
    assert n_fitted == 8 * 3 * 8 + 1  # (the fit ran on every row of the eight S >= 21 and on the first of the edge rows)
    print("measured float64 / longdouble deviation: elpd and log weights %.3g, k %.3g" % (measured_e, measured_k))
    assert measured_e <= pr.PSIS_MEASURED_DEVIATION_ELPD and measured_k <= pr.PSIS_MEASURED_DEVIATION_K


def test_psis_row_edge_rows_take_the_branches_they_are_named_for():
    name, ll, r_eff = pr.cpu_cases()[-1]
    elpd, k, lw = pr.psis(ll, r_eff)
    assert name == "edge_rows" and np.isfinite(k[0]) and np.all(np.isposinf(k[1:])) and np.isneginf(elpd[4])
    assert np.unique(ll[:, 0]).size == ll.shape[0] - 6  # six equal pairs


def test_psis_row_refuses():
    from myfm_amd import _myfm

    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="r_eff"):
            _myfm.psis_row(np.zeros(30), bad)
    with pytest.raises(ValueError):
        _myfm.psis_row(np.zeros(0))
    with pytest.raises(ValueError):
        _myfm.psis_row(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="4096"):
        _myfm.psis_row(np.zeros(4097))


# ---- (c) loo and compare ---------------------------------------------------------------------------------------------------------
def test_loo_and_compare_on_hand_made_arrays():
    from myfm_amd import LooDensity
    from myfm_amd.utils import evaluation as ev

    elpd = np.array([-1.0, -2.0, -4.0, -1.0])
    k = np.array([0.1, 0.69, 0.71, np.inf])
    lpd = np.array([-0.5, -1.5, -3.0, -1.0])
    res = LooDensity(elpd, k, lpd, None, None)
    out = ev.loo(res, 4000)
    assert out["elpd_loo"] == -8.0 and out["p_loo"] == 2.0 and out["looic"] == 16.0
    assert out["se"] == pytest.approx(np.sqrt(4 * np.var(elpd)))
    assert out["pareto_k_threshold"] == 0.7 and out["n_bad_k"] == 2
    few = ev.loo(res, 100)  # 1 - 1 / log10(100) = 0.5
    assert few["pareto_k_threshold"] == pytest.approx(0.5) and few["n_bad_k"] == 3
    assert ev.pareto_k_threshold(2200) == 0.7 and ev.pareto_k_threshold(1000) == pytest.approx(2.0 / 3.0)
    assert ev.loo((elpd, k, lpd), 4000) == out
    other = LooDensity(elpd + np.array([0.5, -0.5, 1.0, 0.0]), k, lpd, None, None)
    cmp = ev.compare(other, res)
    assert cmp["elpd_diff"] == 1.0 and cmp["se_diff"] == pytest.approx(np.sqrt(4 * np.var([0.5, -0.5, 1.0, 0.0])))
    assert ev.compare(other.elpd_loo, res.elpd_loo) == cmp
    with pytest.raises(ValueError, match="same rows"):
        ev.compare(res, LooDensity(elpd[:3], k[:3], lpd[:3], None, None))
    with pytest.raises(ValueError, match="one length"):
        ev.loo((elpd, k[:3], lpd), 100)
    for bad in (1, 2.5, True):
        with pytest.raises(ValueError, match="n_samples"):
            ev.loo(res, bad)
    counts, chi2 = ev.pit_histogram(np.array([0.05, 0.15, 0.95, 0.5]), bins=2)  # a bare array, as result.loo_pit is
    assert counts.tolist() == [2, 2] and chi2 == 0.0


# ---- (d) refusals on the host ----------------------------------------------------------------------------------------------------
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


def _same_error(est, good_y, args, kwargs=None):
    """predict_loo raises what predict_log_density raises for these arguments, with the same message"""
    kwargs = kwargs or {}
    with pytest.raises((ValueError, RuntimeError)) as want:
        est.predict_log_density(*args, **kwargs)
    with pytest.raises(type(want.value)) as got:
        est.predict_loo(*args, **kwargs)
    assert str(got.value) == str(want.value)


def _own_refusals(est, y, **kw):
    for bad in (0, 0.0, -1.0, np.nan, np.inf, True, "1", None, [1.0]):
        with pytest.raises(ValueError, match="r_eff must be one finite positive number"):
            est.predict_loo(X3, y, r_eff=bad, **kw)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError, match="log_weights must be a bool"):
            est.predict_loo(X3, y, log_weights=bad, **kw)


def _shared_refusals(est, y):
    import myfm_amd

    _same_error(est, y, (X3, y[:2]))
    _same_error(est, y, (X3, np.stack([y, y])))
    for bad in (np.nan, np.inf):
        _same_error(est, y, (X3, np.array([y[0], bad, y[2]], dtype=np.float64)))
    _same_error(est, y, (X3[:, :11], y))
    _same_error(est, y, (X3[:, :8], y, [myfm_amd.RelationBlock([0, 1], sps.csr_matrix(np.eye(4)))]))
    p, task = est.predictor_, int(est._task_type)
    for name in ("tile_rows", "chunk_samples"):
        with pytest.raises(ValueError, match="non-negative"):
            p.predict_loo(X3, [], np.asarray(y, dtype=np.float64), task, precisions=np.ones(S) if task == 0 else None,
                          cutpoints=0 if task == 2 else None, **{name: -1})
    with pytest.raises(ValueError, match="does not match"):
        p.predict_loo(X3, [], np.asarray(y, dtype=np.float64), (task + 1) % 3)
    with pytest.raises(ValueError, match="r_eff"):
        p.predict_loo(X3, [], np.asarray(y, dtype=np.float64), task, precisions=np.ones(S) if task == 0 else None,
                      cutpoints=0 if task == 2 else None, r_eff=0.0)


@pytest.mark.parametrize("cls", ["MyFMRegressor", "MyFMGibbsRegressor"])
def test_regression_refusals_need_no_gpu(cls):
    est = _restored(cls, "REGRESSION")
    y = np.array([0.5, -1.0, 2.0])
    with pytest.raises(RuntimeError, match="predict_loo needs history_"):  # no history at all
        est.predict_loo(X3, y)
    for bad in (0.0, -1.0, np.inf, np.nan):
        est.history_ = _history([1.0, bad])
        _same_error(est, y, (X3, y))
    est.history_ = _history([9.0, 1.0, 2.0])
    _shared_refusals(est, y)
    _own_refusals(est, y)
    if _no_device():  # valid arguments: the usual refusal of a machine without a GPU comes only now
        for log_weights in (False, True):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.predict_loo(X3, y, log_weights=log_weights, r_eff=0.5)


@pytest.mark.parametrize("cls", ["MyFMClassifier", "MyFMGibbsClassifier"])
def test_classification_refusals_need_no_gpu(cls):
    est = _restored(cls, "CLASSIFICATION")
    y = np.array([0.0, 1.0, 1.0])
    for bad in (2.0, -1.0, 0.5):
        _same_error(est, y, (X3, np.array([0.0, bad, 1.0])))
    with pytest.raises(TypeError):
        est.predict_loo(X3, y, cutpoint_index=0)
    _shared_refusals(est, y)
    _own_refusals(est, y)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_loo(X3, np.array([False, True, True]))


def test_ordered_refusals_need_no_gpu():
    est = _restored("MyFMOrderedProbit", "ORDERED", CUTS)
    y = np.array([0, 3, 2])
    for bad in (4, -1, 1.5):
        _same_error(est, y, (X3, np.array([0, bad, 1])))
    _same_error(est, y, (X3, y), dict(cutpoint_index=1))
    _same_error(est, y, (X3, y), dict(cutpoint_index=0.0))
    for cuts in ([CUTS[0], np.array([0.5, 0.25, 2.0])], [np.array([-1.0, np.nan, 1.5]), CUTS[1]]):
        _same_error(_restored("MyFMOrderedProbit", "ORDERED", cuts), y, (X3, y))
    _same_error(_restored("MyFMOrderedProbit", "ORDERED", [CUTS[0], CUTS[1][:2]]), y, (X3, np.array([0, 1, 2])))
    _shared_refusals(est, y)
    _own_refusals(est, y, cutpoint_index=0)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_loo(X3, y, log_weights=True, cutpoint_index=0)


def test_more_than_4096_samples_are_refused():
    est = _restored("MyFMClassifier", "CLASSIFICATION", n_samples=4097)
    y = np.array([0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="at most 4096 kept samples, this model keeps 4097"):
        est.predict_loo(X3, y)
    with pytest.raises(ValueError, match="at most 4096 kept samples, this model keeps 4097"):
        est.predictor_.predict_loo(X3, [], y, 1)
    at_limit = _restored("MyFMClassifier", "CLASSIFICATION", n_samples=4096)
    if _no_device():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            at_limit.predict_loo(X3, y)


# ---- (e) exports -------------------------------------------------------------------------------------------------------------------
def test_who_has_the_method():
    import myfm_amd

    assert myfm_amd.LooDensity._fields == ("elpd_loo", "pareto_k", "lpd", "loo_pit", "log_weights")
    assert "LooDensity" in myfm_amd.__all__
    assert myfm_amd.PointwiseDensity._fields == ("lpd", "log_lik_mean", "log_lik_var", "pit", "log_lik")
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.MyFMRegressor,
                myfm_amd.MyFMClassifier):
        assert callable(cls.predict_loo)
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_loo")
    assert callable(myfm_amd._myfm.Predictor.predict_loo) and callable(myfm_amd._myfm.psis_row)
    assert not hasattr(myfm_amd._myfm.VariationalPredictor, "predict_loo")
    for cls, y in ((myfm_amd.MyFMRegressor, [0.5]), (myfm_amd.MyFMClassifier, [1]), (myfm_amd.MyFMOrderedProbit, [1])):
        with pytest.raises(RuntimeError, match="Predictor called before fit"):
            cls(2).predict_loo(sps.csr_matrix((1, 3)), y)


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_design_loo_store", "mfm_design_loo", "mfm_psis_row"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.Design.loo) and callable(_capi.Store.loo)
    assert _capi.psis_tail_len(4096, 0.05) == 820 and _capi.psis_tail_len(95) == 19
