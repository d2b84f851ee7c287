"""Chain diagnostics of several chains, the parts that need no GPU: the NumPy reference of tests/ess_chains_ref.py
against tests/ess_ref.py at one chain, the host hook _myfm.ess_row(x, n_chains) against it, sequence_diagnostics and
hyper_diagnostics, the refusals that are raised on the host, combine_chains on restored models, and the exports."""
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

from tests import ess_chains_ref as cr
from tests import ess_ref as er
from tests.test_loo_cpu import CUTS, D, K, X3


def er_table(S):
    from myfm_amd import _myfm

    return _myfm.rank_z_table(S)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b)) and len(tuple(a)) == len(tuple(b))


# ---- (a) the reference at one chain is the single-chain reference ----------------------------------------------------------------
def test_the_reference_at_one_chain_gives_the_bits_of_ess_ref():
    from myfm_amd import _myfm

    for name, S, v in er.cpu_cases():
        table = er_table(S)
        hook = _myfm.ess_row(v[0], n_chains=1)  # (the library at one chain diagnoses what ess_ref.py diagnoses)
        assert np.isnan(hook[0]) == np.isnan(er.E(v[:1]).ess[0]) and np.isnan(hook[1]) == np.isnan(er.E(v[:1]).rhat[0]), (name, S)
        for dtype in (np.float64, np.longdouble):
            assert same_bits(cr.E(v, 1, dtype), er.E(v, dtype)), (name, S, dtype)
            assert same_bits(cr.E(er.rank_z(v, table), 1, dtype), er.E(er.rank_z(v, table), dtype)), (name, S, dtype)
            assert same_bits(cr.value_diagnostics(v, table, 1, dtype), er.value_diagnostics(v, table, dtype)), (name, S, dtype)
            ll = np.log(np.abs(v) + 1e-3).T  # (S, rows): any finite log likelihoods
            assert same_bits(cr.likelihood_diagnostics(ll, table, 1, dtype), er.likelihood_diagnostics(ll, table, dtype)), (name, S, dtype)


# ---- (b) the host hook against the reference -------------------------------------------------------------------------------------
def test_ess_row_of_several_chains_matches_the_longdouble_reference():
    """every row of cpu_cases(): (M, L) in CPU_SHAPES x {normal, AR(1) phi = 0.98, clipped with heavy ties, Phi-saturated with ties,
    chains 3 sd apart}, and per row the three sequences the kernel runs E on: v, Z(v) and Z(|v - med v|). A row flagged `near` is left
    out (at most 1 % of a case). The float64 / longdouble deviation of the reference is measured again and has not grown past the
    recorded constants; the raw saturated rows have constants of their own, as in tests/test_ess_cpu.py."""
    from myfm_amd import _myfm

    measured = {False: [0.0, 0.0], True: [0.0, 0.0]}
    n_compared = n_left_out = 0
    for name, M, L, v in cr.cpu_cases():
        table = er_table(M * L)
        z = cr.rank_z(v, table)
        zf = cr.rank_z(cr.folded(v), table)
        for which, x in (("v", v), ("Z(v)", z), ("Z(|v - med|)", zf)):
            r64, rL = cr.E(x, M), cr.E(x, M, np.longdouble)
            ill = name == "saturated" and which == "v"
            rtol_ess = cr.CHAINS_RTOL_ESS_SATURATED if ill else cr.CHAINS_RTOL_ESS
            rtol_rhat = cr.CHAINS_RTOL_RHAT_SATURATED if ill else cr.CHAINS_RTOL_RHAT
            ok = ~np.isnan(rL.ess)
            assert np.array_equal(np.isnan(r64.ess), ~ok) and np.array_equal(np.isnan(rL.rhat), ~ok), (name, M, L, which)
            left_out = r64.near | rL.near
            assert left_out.sum() <= cr.MAX_EXCLUDED_SHARE * len(x), (name, M, L, which, int(left_out.sum()))
            n_left_out += int(left_out.sum())
            use = ok & ~left_out
            if use.any():
                m = measured[ill]
                m[0] = max(m[0], cr.deviation(r64.ess[use], rL.ess[use]).max())
                m[1] = max(m[1], cr.deviation(r64.rhat[use], rL.rhat[use]).max())
            if name == "shifted" and which != "Z(|v - med|)":
                assert np.all(r64.rhat > 1.1), (name, M, L, which, r64.rhat.min())
            for t in range(len(x)):
                ess, rhat = _myfm.ess_row(x[t], n_chains=M)
                if not ok[t]:
                    assert np.isnan(ess) and np.isnan(rhat), (name, M, L, which, t)
                elif use[t]:
                    n_compared += 1
                    assert cr.deviation(ess, rL.ess[t]) <= rtol_ess, (name, M, L, which, t, ess, rL.ess[t])
                    assert cr.deviation(rhat, rL.rhat[t]) <= rtol_rhat, (name, M, L, which, t, rhat, rL.rhat[t])
        if name == "shifted":
            assert np.all(cr.value_diagnostics(v, table, M).rhat > 1.1), (M, L)
    print("rows compared %d, left out as near a Geyer decision %d" % (n_compared, n_left_out))
    print("measured float64 / longdouble deviation: ess %.3g, rhat %.3g; raw saturated rows: ess %.3g, rhat %.3g"
          % (measured[False][0], measured[False][1], measured[True][0], measured[True][1]))
    assert measured[False][0] <= cr.CHAINS_MEASURED_DEVIATION_ESS and measured[False][1] <= cr.CHAINS_MEASURED_DEVIATION_RHAT
    assert measured[True][0] <= cr.CHAINS_MEASURED_DEVIATION_ESS_SATURATED and measured[True][1] <= cr.CHAINS_MEASURED_DEVIATION_RHAT_SATURATED


def test_constant_chains_and_short_chains():
    from myfm_amd import _myfm

    rng = np.random.default_rng(4)
    # one chain of three is constant, the others vary: diagnosed
    x = rng.normal(size=(5, 3 * 16))
    x[:, 16:32] = 0.25
    want = cr.E(x, 3, np.longdouble)
    assert np.all(np.isfinite(np.asarray(want.ess, dtype=np.float64))) and np.all(np.isfinite(np.asarray(want.rhat, dtype=np.float64)))
    for t in range(len(x)):
        ess, rhat = _myfm.ess_row(x[t], n_chains=3)
        assert cr.deviation(ess, want.ess[t]) <= cr.CHAINS_RTOL_ESS and cr.deviation(rhat, want.rhat[t]) <= cr.CHAINS_RTOL_RHAT
    # every chain constant, each at its own value: W = 0, nothing to diagnose
    y = np.repeat([0.1, 0.7, -2.0], 16)
    assert all(np.isnan(o) for o in _myfm.ess_row(y, n_chains=3))
    assert np.all(np.isnan(cr.E(y, 3).ess)) and np.all(np.isnan(cr.E(y, 3).rhat))
    # two chains of seven draws: halves of three
    z = rng.normal(size=14)
    assert all(np.isnan(o) for o in _myfm.ess_row(z, n_chains=2))
    assert np.all(np.isnan(cr.E(z, 2).ess))
    assert all(np.all(np.isnan(o)) for o in cr.value_diagnostics(z, er_table(14), 2)[:4])
    # an odd chain length: the middle draw of every chain belongs to no sequence
    w = rng.normal(size=3 * 9)
    moved = w.copy()
    moved[[4, 13, 22]] += 100.0
    assert _myfm.ess_row(w, n_chains=3) == _myfm.ess_row(moved, n_chains=3)


def test_one_chain_through_the_new_argument_gives_the_old_bits():
    from myfm_amd import _capi, _myfm

    for name, S, v in er.cpu_cases():
        for x in v[:6]:
            a, b = _myfm.ess_row(x, 1), _myfm.ess_row(x)
            assert np.array_equal(a, b, equal_nan=True), (name, S)
            assert np.array_equal(_capi.ess_row(x, n_chains=1), b, equal_nan=True) and np.array_equal(_capi.ess_row(x), b, equal_nan=True)
    x = np.random.default_rng(1).normal(size=60)
    assert _capi.ess_row(x, 3) == _myfm.ess_row(x, n_chains=3) != _myfm.ess_row(x)


def test_bad_chain_counts_are_refused():
    from myfm_amd import _capi, _myfm

    x = np.random.default_rng(0).normal(size=66)
    for hook in (_myfm.ess_row, _capi.ess_row):
        with pytest.raises(ValueError, match="n_chains must be at least 1"):
            hook(x, 0)
        with pytest.raises(ValueError, match="at most 32 chains, got 33"):
            hook(x, 33)
        with pytest.raises(ValueError, match="66 samples are not a multiple of n_chains = 4"):
            hook(x, 4)
        assert np.isfinite(hook(x, 3)[0])


# ---- (c) the traces of scalars: sequence_diagnostics, hyper_diagnostics ----------------------------------------------------------
def test_sequence_diagnostics_matches_the_reference():
    from myfm_amd.utils import evaluation as ev

    for name, M, L, v in cr.cpu_cases():
        if M * L > 512 or name == "saturated":
            continue
        table = er_table(M * L)
        want = cr.value_diagnostics(v, table, M, np.longdouble)
        for t in range(0, len(v), 7):
            if want.near[t]:
                continue
            rhat, bulk, mean = ev.sequence_diagnostics(v[t], M)
            for g, w, tol in ((rhat, want.rhat[t], cr.CHAINS_RTOL_RHAT), (bulk, want.ess_bulk[t], cr.CHAINS_RTOL_ESS),
                              (mean, want.ess_mean[t], cr.CHAINS_RTOL_ESS)):
                assert (np.isnan(g) and np.isnan(w)) or cr.deviation(g, w) <= tol, (name, M, L, t, g, w)
    assert all(np.isnan(o) for o in ev.sequence_diagnostics(np.full(32, 0.5), 2))
    bad = np.arange(32.0)
    bad[5] = np.nan
    assert all(np.isnan(o) for o in ev.sequence_diagnostics(bad, 2))
    with pytest.raises(ValueError, match="not a multiple"):
        ev.sequence_diagnostics(np.arange(33.0), 2)
    with pytest.raises(ValueError, match="non-empty 1-D"):
        ev.sequence_diagnostics(np.zeros((4, 8)))


def _hyper(rng, alpha, G=2):
    from myfm_amd import _myfm

    h = _myfm.FMHyperParameters.__new__(_myfm.FMHyperParameters)
    h.__setstate__((alpha, rng.normal(size=G), np.exp(rng.normal(size=G)), rng.normal(size=(G, K)), np.exp(rng.normal(size=(G, K)))))
    return h


def _chain(cls, task, seed, cuts=None, n_samples=16, alpha=None):
    """an estimator around a Predictor restored through __setstate__ (as tests/test_loo_cpu.py builds one), its samples drawn from
    `seed`, with a history_ of n_samples + 3 entries and n_groups_ = 2: no fit, no device"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(seed)
    fms = []
    for s in range(n_samples):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((float(rng.normal()), rng.normal(size=D), rng.normal(size=(D, K)), [] if cuts is None else [cuts[s]]))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(getattr(_myfm.TaskType, task)), fms))
    est = getattr(myfm_amd, cls)(K)
    est.predictor_ = p
    est.history_ = _myfm.LearningHistory([_hyper(rng, float(np.exp(rng.normal())) if alpha is None else alpha) for _ in range(n_samples + 3)],
                                         list(rng.normal(size=n_samples + 3)), list(range(n_samples + 3)))
    est.n_groups_ = 2
    return est


def test_hyper_diagnostics_keys_and_a_constant_trace():
    import myfm_amd
    from myfm_amd.utils import evaluation as ev

    chains = [_chain("MyFMGibbsRegressor", "REGRESSION", 10 + c) for c in range(3)]
    both = myfm_amd.combine_chains(chains)
    out = ev.hyper_diagnostics(both)
    assert list(out) == ["alpha", "mu_w[0]", "mu_w[1]", "lambda_w[0]", "lambda_w[1]"]
    alpha = np.concatenate([[h.alpha for h in c.history_.hypers[3:]] for c in chains])
    assert out["alpha"] == ev.sequence_diagnostics(alpha, 3) and all(np.isfinite(out["alpha"]))
    lam1 = np.concatenate([[h.lambda_w[1] for h in c.history_.hypers[3:]] for c in chains])
    assert out["lambda_w[1]"] == ev.sequence_diagnostics(lam1, 3)
    single = ev.hyper_diagnostics(chains[0])
    assert single["alpha"] == ev.sequence_diagnostics(alpha[:16], 1)
    probit = myfm_amd.combine_chains([_chain("MyFMGibbsClassifier", "CLASSIFICATION", 20 + c, alpha=1.0) for c in range(2)])
    out = ev.hyper_diagnostics(probit)
    assert all(np.isnan(o) for o in out["alpha"]) and all(np.isfinite(o) for o in out["mu_w[0]"])
    with pytest.raises(RuntimeError, match="fitted"):
        ev.hyper_diagnostics(myfm_amd.MyFMGibbsRegressor(2))


# ---- (d) combine_chains on the host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_combine_chains_pools_the_samples_chain_after_chain(kind):
    import myfm_amd

    cls, task, cuts = {"regressor": ("MyFMGibbsRegressor", "REGRESSION", None), "classifier": ("MyFMGibbsClassifier", "CLASSIFICATION", None),
                       "ordered": ("MyFMOrderedProbit", "ORDERED", [CUTS[s % 2] for s in range(16)])}[kind]
    chains = [_chain(cls, task, 30 + c, cuts) for c in range(3)]
    chains[0].random_seed = 77
    before = [pickle.dumps((c.predictor_, c.history_)) for c in chains]
    both = myfm_amd.combine_chains(chains)
    assert type(both) is type(chains[0]) and both.n_chains_ == 3 and both.n_groups_ == 2 and both.random_seed == 77
    assert not hasattr(chains[0], "n_chains_") and [pickle.dumps((c.predictor_, c.history_)) for c in chains] == before
    assert len(both.predictor_.samples) == 48 and both.predictor_.feature_size == D and not both.predictor_.resident
    for name in ("w0_samples", "w_samples", "V_samples") + (("cutpoint_samples",) if kind == "ordered" else ()):
        assert np.array_equal(getattr(both, name), np.concatenate([getattr(c, name) for c in chains])), name
    assert len(both.history_.hypers) == 48
    kept = [h for c in chains for h in c.history_.hypers[3:]]
    assert [h.alpha for h in both.history_.hypers] == [h.alpha for h in kept]
    assert all(np.array_equal(a.mu_V, b.mu_V) and np.array_equal(a.lambda_w, b.lambda_w) for a, b in zip(both.history_.hypers, kept))
    assert list(both.history_.train_log_losses) == [v for c in chains for v in c.history_.train_log_losses[3:]]
    assert list(both.history_.n_mh_accept) == [v for c in chains for v in c.history_.n_mh_accept[3:]]
    again = pickle.loads(pickle.dumps(both))
    assert again.n_chains_ == 3 and np.array_equal(again.w_samples, both.w_samples) and len(again.history_.hypers) == 48
    assert myfm_amd.combine_chains(chains[:1]).n_chains_ == 1


def test_combine_chains_refuses_on_the_host():
    import myfm_amd

    reg = lambda seed, **kw: _chain("MyFMGibbsRegressor", "REGRESSION", seed, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="at least one"):
        myfm_amd.combine_chains([])
    with pytest.raises(ValueError, match="one class"):
        myfm_amd.combine_chains([reg(1), _chain("MyFMGibbsClassifier", "CLASSIFICATION", 2)])
    with pytest.raises(ValueError, match="keeps no samples"):
        myfm_amd.combine_chains([myfm_amd.VariationalFMRegressor(2), myfm_amd.VariationalFMRegressor(2)])
    with pytest.raises(ValueError, match="estimator 1 is not fitted"):
        myfm_amd.combine_chains([reg(1), myfm_amd.MyFMGibbsRegressor(K)])
    with pytest.raises(ValueError, match="estimator 1 is itself a combination"):
        myfm_amd.combine_chains([reg(1), myfm_amd.combine_chains([reg(2), reg(3)])])
    with pytest.raises(ValueError, match="at most 32 chains"):
        myfm_amd.combine_chains([reg(1)] * 33)
    with pytest.raises(ValueError, match="number of kept samples"):
        myfm_amd.combine_chains([reg(1), reg(2, n_samples=8)])
    other = reg(2)
    other.n_groups_ = 1
    with pytest.raises(ValueError, match="n_groups_"):
        myfm_amd.combine_chains([reg(1), other])
    other = reg(2)
    other.rank = K + 1
    with pytest.raises(ValueError, match="its rank"):
        myfm_amd.combine_chains([reg(1), other])
    other = reg(2)
    other.fold_in_columns_ = (D - 1, D)
    with pytest.raises(ValueError, match="fold_in_columns_"):
        myfm_amd.combine_chains([reg(1), other])
    ordered = lambda seed, cuts: _chain("MyFMOrderedProbit", "ORDERED", seed, cuts)  # noqa: E731
    with pytest.raises(ValueError, match="number of cutpoints"):
        myfm_amd.combine_chains([ordered(1, [CUTS[0]] * 16), ordered(2, [CUTS[0][:2]] * 16)])
    with pytest.raises(ValueError, match="keeps no samples"):
        myfm_amd.fit_chains(myfm_amd.VariationalFMRegressor(2), X3, np.zeros(3))
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="n_chains must be an integer"):
            myfm_amd.fit_chains(myfm_amd.MyFMGibbsRegressor(2), X3, np.zeros(3), n_chains=bad)
    for bad in ([1, 1], [1], [1, 2.5]):
        with pytest.raises(ValueError, match="seeds must hold"):
            myfm_amd.fit_chains(myfm_amd.MyFMGibbsRegressor(2), X3, np.zeros(3), n_chains=2, seeds=bad)


def test_the_chain_count_reaches_the_predictor_and_is_checked_by_the_library():
    """33 chains and a count that does not divide the samples are refused by the estimator's calls (the library's message), on a
    machine with a GPU and without: before the device is touched"""
    import myfm_amd

    both = myfm_amd.combine_chains([_chain("MyFMGibbsClassifier", "CLASSIFICATION", 40 + c) for c in range(2)])
    y = np.array([0.0, 1.0, 1.0])
    for n, match in ((5, "32 samples are not a multiple of n_chains = 5"), (33, "at most 32 chains, got 33"), (0, "n_chains must be at least 1")):
        both.n_chains_ = n
        for call in (lambda: both.predict_diagnostics(X3), lambda: both.likelihood_diagnostics(X3, y),
                     lambda: both.predict_loo(X3, y, r_eff="auto")):
            with pytest.raises(ValueError, match=match):
                call()


L_MAX = 32  # chains: the 64 half-chains of a row are the lanes of one wavefront


# ---- (e) exports -----------------------------------------------------------------------------------------------------------------
def test_the_new_names_exist():
    import inspect

    import myfm_amd
    from myfm_amd import _capi
    from myfm_amd.utils import evaluation as ev

    assert callable(myfm_amd.combine_chains) and callable(myfm_amd.fit_chains)
    assert "combine_chains" in myfm_amd.__all__ and "fit_chains" in myfm_amd.__all__
    assert callable(ev.sequence_diagnostics) and callable(ev.hyper_diagnostics)
    assert callable(myfm_amd._myfm.Predictor.concatenated)
    assert myfm_amd._myfm.ESS_MAX_CHAINS == L_MAX == _capi.lib().mfm_ess_max_chains()
    for f in (_capi.Design.ess, _capi.Store.ess, _capi.ess_row, myfm_amd.fit_chains):
        assert "n_chains" in inspect.signature(f).parameters
    assert inspect.signature(_capi.ess_row).parameters["n_chains"].default == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_design_ess_chains_store", "mfm_design_ess_chains", "mfm_ess_row_chains", "mfm_ess_check_chains", "mfm_ess_max_chains"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
