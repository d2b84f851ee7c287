"""Chain diagnostics, the parts that need no GPU: identities of the NumPy reference (tests/ess_ref.py), the host hooks
_myfm.ess_row (one sequence through the scalar pieces of the kernel) and _myfm.rank_z_table against it, diagnostics_summary, the
refusals that are raised before the device is looked for, and the exports."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.special import ndtri

from tests import ess_ref as er
from tests.test_loo_cpu import CUTS, X3, _history, _no_device, _restored


# ---- (a) identities of the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [95, 1024])
def test_independent_draws_are_worth_about_s(S):
    x = np.random.default_rng(S).normal(size=(200, S))
    ess = er.E(x).ess
    assert abs(np.median(ess) - S) <= 0.15 * S
    assert np.all(ess <= S * np.log10(S))


@pytest.mark.parametrize("phi", [0.5, 0.9])
def test_ar1_rows_have_the_textbook_efficiency(phi):
    S = 4096
    out = er.E(er.ar1(np.random.default_rng(7), phi, 40, S))
    want = S * (1.0 - phi) / (1.0 + phi)
    print("phi %.1f: mean ess %.0f against %.0f" % (phi, out.ess.mean(), want))
    assert abs(out.ess.mean() - want) <= 0.10 * want
    assert np.all(out.rhat < 1.05)


def test_a_shifted_second_half_has_a_large_rhat():
    rng = np.random.default_rng(3)
    for S in (32, 95, 1024):
        x = rng.normal(size=(20, S))
        x[:, S // 2:] += 3.0
        table = er_table(S)
        assert np.all(er.E(x).rhat > 1.5)
        assert np.all(er.value_diagnostics(x, table).rhat > 1.5)


def er_table(S):
    from myfm_amd import _myfm

    return _myfm.rank_z_table(S)


def test_constant_rows_and_short_chains_give_nan():
    for S in (1, 2, 7):
        x = np.random.default_rng(S).normal(size=(3, S))
        out = er.E(x)
        assert np.all(np.isnan(out.ess)) and np.all(np.isnan(out.rhat)) and np.all(out.T == -1)
        assert all(np.all(np.isnan(o)) for o in er.value_diagnostics(x, np.zeros(2 * S - 1))[:4])
    for S in (8, 95):
        out = er.E(np.full((2, S), 0.25))
        assert np.all(np.isnan(out.ess)) and np.all(np.isnan(out.rhat))
        got = er.value_diagnostics(np.full((2, S), 0.25), er_table(S))
        assert all(np.all(np.isnan(o)) for o in got[:4])
    ll = np.random.default_rng(0).normal(size=(16, 3))
    ll[:, 1] = -np.inf  # a density of 0 under every sample
    ll[3, 2] = -np.inf  # ... and under one
    got = er.likelihood_diagnostics(ll, er_table(16))
    assert np.isnan(got.r_eff[1]) and np.isnan(got.rhat[1]) and np.isfinite(got.r_eff[0]) and np.isfinite(got.r_eff[2])


def test_the_fold_is_the_distance_to_numpys_median_and_symmetric_in_the_middle():
    rng = np.random.default_rng(5)
    for S in (8, 9, 32, 95):
        x = np.exp(rng.normal(size=(200, S)))
        med = np.quantile(x, 0.5, axis=1)
        assert np.array_equal(med, er.median_linear(x))
        f = er.folded(x)
        assert np.all(np.abs(f - np.abs(x - med[:, None])) <= 4 * np.finfo(np.float64).eps * np.abs(x).max(axis=1)[:, None])
        order = np.argsort(x, axis=1)
        r = np.arange(len(x))
        lo, hi = f[r, order[:, (S - 1) // 2]], f[r, order[:, S // 2]]
        assert np.array_equal(lo, hi)  # odd S: the median itself, 0; even S: the two middle draws, equally far
        assert np.all(lo == 0.0) if S % 2 else np.all(lo > 0.0)
        assert np.array_equal(f.min(axis=1), lo)


def test_the_ess_is_bounded_by_s_log10_s():
    rng = np.random.default_rng(11)
    for S in (8, 9, 16, 95):
        e = rng.normal(size=(300, S + 1))
        ess = er.E(e[:, 1:] - 0.9 * e[:, :-1]).ess  # (a negative lag-1 correlation: an ess above S, up to the floor of tau)
        assert np.all(ess <= S * np.log10(S) * (1 + 1e-12)) and (S < 16 or ess.max() > S)  # (S = 8, 9: every row sits on the floor, 7.22)


# ---- (b) the host hooks against the reference --------------------------------------------------------------------------------
def test_ess_row_matches_the_longdouble_reference():
    """every row of cpu_cases(): S in CPU_SIZES x {normal, AR(1) phi = 0.98, Phi-saturated with ties, clipped with heavy ties}, and
    per row the three sequences the kernel runs E on: v, Z(v) and Z(|v - med v|). A row flagged `near` is left out (at most 1 % of a
    case). The float64 / longdouble deviation of the reference is measured again and has not grown past the recorded constants.
    The raw saturated rows are ill-conditioned (their spread is 1e-6 and less of their value: v - mean cancels): they have
    constants of their own."""
    from myfm_amd import _myfm

    measured = {False: [0.0, 0.0], True: [0.0, 0.0]}
    n_compared = n_left_out = 0
    for name, S, v in er.cpu_cases():
        table = er_table(S)
        z = er.rank_z(v, table)
        zf = er.rank_z(er.folded(v), table)
        for which, x in (("v", v), ("Z(v)", z), ("Z(|v - med|)", zf)):
            r64, rL = er.E(x), er.E(x, np.longdouble)
            ill = name == "saturated" and which == "v"
            rtol_ess = er.ESS_RTOL_ESS_SATURATED if ill else er.ESS_RTOL_ESS
            rtol_rhat = er.ESS_RTOL_RHAT_SATURATED if ill else er.ESS_RTOL_RHAT
            ok = ~np.isnan(rL.ess)
            assert np.array_equal(np.isnan(r64.ess), ~ok) and np.array_equal(np.isnan(rL.rhat), ~ok), (name, S, which)
            left_out = r64.near | rL.near
            assert left_out.sum() <= er.MAX_EXCLUDED_SHARE * len(x), (name, S, which, int(left_out.sum()))
            n_left_out += int(left_out.sum())
            use = ok & ~left_out
            if use.any():
                m = measured[ill]
                m[0] = max(m[0], er.deviation(r64.ess[use], rL.ess[use]).max())
                m[1] = max(m[1], er.deviation(r64.rhat[use], rL.rhat[use]).max())
            for t in range(len(x)):
                ess, rhat = _myfm.ess_row(x[t])
                if not ok[t]:
                    assert np.isnan(ess) and np.isnan(rhat), (name, S, which, t)
                elif use[t]:
                    n_compared += 1
                    assert er.deviation(ess, rL.ess[t]) <= rtol_ess, (name, S, which, t, ess, rL.ess[t])
                    assert er.deviation(rhat, rL.rhat[t]) <= rtol_rhat, (name, S, which, t, rhat, rL.rhat[t])
    print("rows compared %d, left out as near a Geyer decision %d" % (n_compared, n_left_out))
    print("measured float64 / longdouble deviation: ess %.3g, rhat %.3g; raw saturated rows: ess %.3g, rhat %.3g"
          % (measured[False][0], measured[False][1], measured[True][0], measured[True][1]))
    assert n_left_out == 0  # (on these inputs the reference flags none)
    assert measured[False][0] <= er.ESS_MEASURED_DEVIATION_ESS and measured[False][1] <= er.ESS_MEASURED_DEVIATION_RHAT
    assert measured[True][0] <= er.ESS_MEASURED_DEVIATION_ESS_SATURATED and measured[True][1] <= er.ESS_MEASURED_DEVIATION_RHAT_SATURATED


def test_the_multi_batch_lags_are_reached_on_the_host():
    """the AR(1) rows at S >= 1024 truncate beyond lag 64, the kernel's first batch"""
    for name, S, v in er.cpu_cases():
        if name == "ar1" and S >= 1024:
            assert np.median(er.E(v).T) >= 64


def test_ess_row_refuses():
    from myfm_amd import _myfm

    with pytest.raises(ValueError):
        _myfm.ess_row(np.zeros(0))
    with pytest.raises(ValueError):
        _myfm.ess_row(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="4096"):
        _myfm.ess_row(np.zeros(4097))
    for bad in (0, 4097, -1):
        with pytest.raises(ValueError, match="4096"):
            _myfm.rank_z_table(bad)
    assert all(np.isnan(v) for v in _myfm.ess_row(np.arange(7.0)))
    row = np.arange(8.0)
    row[3] = np.inf
    assert all(np.isnan(v) for v in _myfm.ess_row(row))


@pytest.mark.parametrize("S", [1, 8, 95, 4096])
def test_the_rank_z_table_matches_ndtri(S):
    """table[j] = Phi^-1((1 + j / 2 - 3 / 8) / (S + 1 / 4)). The library bisects 0.5 erfc(-z / sqrt 2) down to neighbouring doubles: its
    z is off by the error of erfc and of p, a few eps p / phi(z) <= a few eps max(1, 1 / |z|)-ish; ndtri itself is good to about
    1e-15 relative. 1e-13 relative with 1e-15 absolute around z = 0 covers both."""
    from myfm_amd import _capi, _myfm

    table = _myfm.rank_z_table(S)
    j = np.arange(2 * S - 1)
    want = ndtri((1.0 + j / 2.0 - 0.375) / (S + 0.25))
    assert table.shape == (2 * S - 1,) and np.all(np.diff(table) > 0)
    print("S = %d: largest |table - ndtri| %.3g" % (S, np.abs(table - want).max()))
    assert np.all(np.abs(table - want) <= 1e-13 * np.abs(want) + 1e-15)
    assert np.array_equal(table, _capi.rank_z_table(S))
    assert table[S - 1] == pytest.approx(0.0, abs=1e-15)  # the middle rank
    assert np.allclose(table, -table[::-1], rtol=1e-13, atol=1e-15)


# ---- (c) diagnostics_summary -----------------------------------------------------------------------------------------------------
def test_diagnostics_summary_on_hand_made_arrays():
    from myfm_amd import ChainDiagnostics, LikelihoodDiagnostics
    from myfm_amd.utils import evaluation as ev

    rhat = np.array([1.0, 1.005, 1.02, np.nan, 1.3])
    bulk = np.array([400.0, 90.0, 150.0, np.nan, 20.0])
    res = ChainDiagnostics(rhat, bulk, bulk / 2, np.ones(5))
    out = ev.diagnostics_summary(res)
    assert out == {"rhat_max": 1.3, "n_high_rhat": 2, "ess_min": 20.0, "ess_median": 120.0, "n_low_ess": 2, "n_nan": 1}
    assert ev.diagnostics_summary(res, rhat_max=1.1, ess_min=50)["n_high_rhat"] == 1
    assert ev.diagnostics_summary(res, rhat_max=1.1, ess_min=50)["n_low_ess"] == 1
    lik = LikelihoodDiagnostics(np.array([0.5, 0.25, 1.5, np.nan, 0.75]), rhat, bulk, np.ones(5))
    out = ev.diagnostics_summary(lik)
    assert out["r_eff_min"] == 0.25 and out["r_eff_median"] == 0.625 and out["n_nan"] == 1 and out["rhat_max"] == 1.3
    empty = ev.diagnostics_summary(ChainDiagnostics(np.full(2, np.nan), np.full(2, np.nan), None, None))
    assert np.isnan(empty["rhat_max"]) and np.isnan(empty["ess_min"]) and empty["n_nan"] == 2 and empty["n_high_rhat"] == 0
    with pytest.raises(ValueError, match="one length"):
        ev.diagnostics_summary(ChainDiagnostics(rhat, bulk[:3], None, None))


# ---- (d) refusals on the host ----------------------------------------------------------------------------------------------------
def _same_error(call, reference_call):
    with pytest.raises((ValueError, RuntimeError)) as want:
        reference_call()
    with pytest.raises(type(want.value)) as got:
        call()
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_refusals_need_no_gpu(kind):
    cls, task, cuts, y = {"regressor": ("MyFMGibbsRegressor", "REGRESSION", None, np.array([0.5, -1.0, 2.0])),
                          "classifier": ("MyFMGibbsClassifier", "CLASSIFICATION", None, np.array([0.0, 1.0, 1.0])),
                          "ordered": ("MyFMOrderedProbit", "ORDERED", CUTS, np.array([0, 3, 2]))}[kind]
    est = _restored(cls, task, cuts)
    if kind == "regressor":
        with pytest.raises(RuntimeError, match="likelihood_diagnostics needs history_"):
            est.likelihood_diagnostics(X3, y)
        est.history_ = _history([9.0, 1.0, 2.0])
    # the wrong y shape: what predict_log_density raises for it
    _same_error(lambda: est.likelihood_diagnostics(X3, y[:2]), lambda: est.predict_log_density(X3, y[:2]))
    _same_error(lambda: est.likelihood_diagnostics(X3, np.stack([y, y])), lambda: est.predict_log_density(X3, np.stack([y, y])))
    _same_error(lambda: est.likelihood_diagnostics(X3[:, :11], y), lambda: est.predict_log_density(X3[:, :11], y))
    with pytest.raises(ValueError):
        est.predict_diagnostics(X3[:, :11])
    if kind == "ordered":
        for bad in (0.0, "0", True):
            _same_error(lambda: est.likelihood_diagnostics(X3, y, cutpoint_index=bad), lambda: est.predict_log_density(X3, y, cutpoint_index=bad))
            with pytest.raises(ValueError, match="cutpoint_index must be an integer"):
                est.predict_diagnostics(X3, cutpoint_index=bad)
        _same_error(lambda: est.likelihood_diagnostics(X3, y, cutpoint_index=1), lambda: est.predict_log_density(X3, y, cutpoint_index=1))
        with pytest.raises(ValueError, match="cutpoint_index 1 out of range"):
            est.predict_diagnostics(X3, cutpoint_index=1)
    else:
        with pytest.raises(TypeError):
            est.predict_diagnostics(X3, cutpoint_index=0)
    p, t = est.predictor_, int(est._task_type)
    dens = dict(precisions=np.ones(2) if t == 0 else None, cutpoints=0 if t == 2 else None)
    for name in ("tile_rows", "chunk_samples"):
        with pytest.raises(ValueError, match="non-negative"):
            p.predict_ess(X3, [], **{name: -1})
        with pytest.raises(ValueError, match="non-negative"):
            p.likelihood_ess(X3, [], np.asarray(y, dtype=np.float64), t, **dens, **{name: -1})
    with pytest.raises(ValueError, match="does not match"):
        p.likelihood_ess(X3, [], np.asarray(y, dtype=np.float64), (t + 1) % 3)
    # r_eff: "auto" is taken, every other string is still refused
    kw = dict(cutpoint_index=0) if kind == "ordered" else {}
    for bad in ("1", "Auto", "", None, True, 0.0, [1.0]):
        with pytest.raises(ValueError, match="r_eff must be one finite positive number"):
            est.predict_loo(X3, y, r_eff=bad, **kw)
    if _no_device():  # valid arguments: the usual refusal of a machine without a GPU comes only now
        for call in (lambda: est.predict_loo(X3, y, r_eff="auto", **kw), lambda: est.predict_diagnostics(X3, **kw),
                     lambda: est.likelihood_diagnostics(X3, y, **kw)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_more_than_4096_samples_are_refused():
    est = _restored("MyFMClassifier", "CLASSIFICATION", n_samples=4097)
    y = np.array([0.0, 1.0, 1.0])
    for call in (lambda: est.predict_diagnostics(X3), lambda: est.likelihood_diagnostics(X3, y), lambda: est.predictor_.predict_ess(X3, []),
                 lambda: est.predictor_.likelihood_ess(X3, [], y, 1), lambda: est.predict_loo(X3, y, r_eff="auto")):
        with pytest.raises(ValueError, match="at most 4096 kept samples, this model keeps 4097"):
            call()


# ---- (e) exports -----------------------------------------------------------------------------------------------------------------
def test_who_has_the_methods():
    import myfm_amd

    assert myfm_amd.ChainDiagnostics._fields == ("rhat", "ess_bulk", "ess_mean", "mcse_mean")
    assert myfm_amd.LikelihoodDiagnostics._fields == ("r_eff", "rhat", "ess_bulk", "mcse_lpd")
    assert "ChainDiagnostics" in myfm_amd.__all__ and "LikelihoodDiagnostics" in myfm_amd.__all__
    assert myfm_amd.LooDensity._fields == ("elpd_loo", "pareto_k", "lpd", "loo_pit", "log_weights")
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.MyFMRegressor,
                myfm_amd.MyFMClassifier):
        assert callable(cls.predict_diagnostics) and callable(cls.likelihood_diagnostics)
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_diagnostics") and not hasattr(cls, "likelihood_diagnostics")
    for name in ("predict_ess", "likelihood_ess"):
        assert callable(getattr(myfm_amd._myfm.Predictor, name)) and not hasattr(myfm_amd._myfm.VariationalPredictor, name)
    assert callable(myfm_amd._myfm.ess_row) and callable(myfm_amd._myfm.rank_z_table)
    assert callable(myfm_amd.utils.evaluation.diagnostics_summary)


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_design_ess_store", "mfm_design_ess", "mfm_ess_row", "mfm_rank_z_table"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.Design.ess) and callable(_capi.Store.ess)
    x = np.random.default_rng(2).normal(size=40)
    assert _capi.ess_row(x) == myfm_amd._myfm.ess_row(x)
