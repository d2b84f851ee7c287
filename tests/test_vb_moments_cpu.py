"""The analytic score moments of the variational estimators without a device: the two restatements of the reference
agree, the pair split equals the row form of the concatenated row, and the public surface is what the design states."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import vb_moments_ref as vr

ABSENT = ("predict_dist", "predict_proba_dist", "predict_expected_dist", "predict_pairs_dist", "predict_topk_ucb", "predict_topk_samples",
          "predict_topk_thompson", "predict_topk_prob", "predict_diagnostics", "likelihood_diagnostics", "predict_ess", "likelihood_ess",
          "predict_log_density", "predict_crps", "predict_loo", "fold_in", "fold_in_gibbs")
NEW_SYMBOLS = ("mfm_design_moments_vb", "mfm_pairs_moments_vb", "mfm_pairs_topk_bound_vb")


def _random_row(rng, D, nnz):
    cols = rng.choice(D, size=nnz, replace=False)
    vals = rng.choice([-1.5, -0.7, 0.3, 1.0, 2.5], size=nnz) * rng.uniform(0.5, 1.5, size=nnz)
    return cols, vals


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("nnz", [0, 1, 2, 3, 5, 6])
def test_closed_form_equals_brute_force(nnz, K):
    """random rows with non-unit values: the five-sum closed form and the enumeration over pairs of feature pairs agree within
    1e-15 of the closed form's scale (both are longdouble, eps 5e-20; the enumeration has up to 225 K terms)"""
    rng = np.random.default_rng(100 * nnz + K)
    D = 9
    for _ in range(4):
        model = vr.normal_model(rng, D, K, scale=0.8)
        cols, vals = _random_row(rng, D, nnz)
        X = sps.csr_matrix((vals, (np.zeros(nnz, dtype=int), cols)), shape=(1, D))
        mo = vr.closed_form(X, model, extra_var=0.25)
        bf = vr.brute_force_var(cols, vals, model, extra_var=0.25)
        assert abs(mo.var[0] - bf) <= 1e-15 * mo.scale[0], (mo.var[0], bf)
        assert mo.var[0] >= 0 and mo.scale[0] * (1 + 1e-15) >= mo.var[0]  # (scale is rounded to float64)
        if nnz <= 1:  # no feature pair: the linear part alone
            w0v, wv = model[1], model[3]
            assert abs(mo.var[0] - (vr.LD(w0v) + vr.LD(0.25) + sum(vr.LD(v) ** 2 * vr.LD(wv[c]) for c, v in zip(cols, vals)))) <= 1e-18


def test_mean_is_the_mean_models_score():
    from tests import pairs_ref as pr

    rng = np.random.default_rng(5)
    D, K = 12, 4
    model = vr.normal_model(rng, D, K)
    X = sps.random(20, D, density=0.3, random_state=np.random.RandomState(1), format="csr")
    mo = vr.closed_form(X, model)
    ref = pr._sample_scores(np.asarray(X.todense()), model[0], model[2], model[4])
    np.testing.assert_allclose(np.asarray(mo.mean, dtype=np.float64), ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("K", [0, 2, 5])
def test_pair_split_equals_the_row_form(K):
    """Var of the pair row a_u + b_i from its halves (what the device contracts) equals the closed form of the dense pair row"""
    from tests import pairs_ref as pr

    rng = np.random.default_rng(40 + K)
    Xq, Xc, D = pr.disjoint_sides(rng, 6, 7, 5, 6, [1.0, -1.0, 2.0, 0.5, -0.3], mean_nnz=2.5, empty_every=4)
    model = vr.normal_model(rng, D, K, scale=0.7)
    mo = vr.pairs_closed_form(Xq, Xc, model)
    A, B = np.asarray(Xq.todense()), np.asarray(Xc.todense())
    for u in range(6):
        for i in range(7):
            split = vr.pair_split_var(A[u], B[i], model)
            assert abs(split - mo.var[u, i]) <= 1e-15 * mo.scale[u, i], (u, i)


def test_exact_model_is_exact_in_fp64():
    """the exact-layout data of the GPU tests: the float64 evaluation of the closed form equals the longdouble one"""
    rng = np.random.default_rng(3)
    D, K = 15, 33
    model = vr.exact_model(rng, D, K)
    X = sps.random(30, D, density=0.3, random_state=np.random.RandomState(2), format="csr")
    X.data = rng.integers(1, 3, size=X.nnz) * rng.choice([-1.0, 1.0], size=X.nnz)
    mo = vr.closed_form(X, model)
    w0, w0v, w, wv, m, s = model
    Xd = np.asarray(X.todense())
    X2 = Xd * Xd
    M, A, B, C, E = Xd @ m, X2 @ s, (X2 * Xd) @ (s * m), (X2 * X2) @ (s * m * m), (X2 * X2) @ (s * s)
    var64 = w0v + X2 @ wv + (M * M * A - 2 * M * B + C + 0.5 * (A * A - E)).sum(axis=1)
    assert np.array_equal(var64, np.asarray(mo.var, dtype=np.float64))
    assert np.all(np.asarray(mo.var, dtype=np.float64) == mo.var)


def test_surface():
    import myfm_amd

    reg, cls = myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier
    for c in (reg, cls):
        for name in ("predict_moments", "predict_pairs_moments", "predict_topk_bound"):
            assert callable(getattr(c, name)), (c, name)
        for name in ABSENT:
            assert not hasattr(c, name), (c, name)
    assert callable(cls.predict_proba_marginal) and not hasattr(reg, "predict_proba_marginal")
    vp = myfm_amd._myfm.VariationalPredictor
    for name in ("predict_moments", "predict_pairs_moments", "predict_topk_bound"):
        assert callable(getattr(vp, name)) and not hasattr(myfm_amd._myfm.Predictor, name)
    for name in ABSENT:
        assert not hasattr(vp, name), name
    # the Gibbs estimators are what they were
    for c in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit):
        for name in ("predict_moments", "predict_pairs_moments", "predict_topk_bound", "predict_proba_marginal"):
            assert not hasattr(c, name), (c, name)
    assert "ScoreMoments" in myfm_amd.__all__ and myfm_amd.ScoreMoments._fields == ("mean", "std")
    assert "quantile of the probability" in cls.predict_topk_bound.__doc__


def test_unfitted_estimators_raise():
    import myfm_amd

    X = sps.identity(4, format="csr")
    for est in (myfm_amd.VariationalFMRegressor(2), myfm_amd.VariationalFMClassifier(2)):
        for call in (lambda: est.predict_moments(X), lambda: est.predict_pairs_moments(X, X), lambda: est.predict_topk_bound(X, X, 2),
                     lambda: est.predict_moments(X, noise=True)):
            with pytest.raises(RuntimeError, match="Predictor called before fit"):
                call()
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        myfm_amd.VariationalFMClassifier(2).predict_proba_marginal(X)


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.Design.moments_vb) and callable(_capi.Pairs.moments_vb) and callable(_capi.Pairs.topk_bound_vb)
