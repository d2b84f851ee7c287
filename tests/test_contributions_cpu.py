"""predict_contributions without a device: the reference's own identities, mfm_contrib_row -- the kernel's
arithmetic on the host -- against the reference within its bound on every shape the device tests run, the argument checks, the
utils.evaluation helpers and the public surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from tests import contrib_ref as cr
from tests import score_ref as sr

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(K, F, kind, S):
    fo = cr.grouping(F, kind)
    return fo, cr.design37(fo, F), cr.random_samples(cr.D_TEST, K, S)


# ---- the reference's identities ----
@pytest.mark.parametrize("F,kind", [(1, "contiguous"), (3, "contiguous"), (5, "interleaved"), (16, "interleaved")])
def test_components_add_up_to_the_score(F, kind):
    fo, X, samples = case(9, F, kind, 2)
    rows = sr.flat_rows(X)
    for w0, w, V in samples:
        c, _ = cr.components(rows, w, V, fo, F)
        want = sr.fm_score(X, (), w0, w, V)
        got = LD(w0) + c.sum(axis=0)
        M, _ = sr.fm_score_bound(X, (), w0, w, V)  # (relative to what the terms add up to in magnitude: the score may cancel)
        assert np.all(np.abs(got - want) <= 1e-17 * M)


def test_one_unit_entry_in_a_field_has_no_inner_interaction():
    fo, X, samples = case(9, 5, "contiguous", 2)
    rows = sr.flat_rows(X)
    for _, w, V in samples:
        c, _ = cr.components(rows, w, V, fo, 5)
        twin = cr.components_f64(rows, w, V, fo, 5)
        diag = [5 + i for i, (g, h) in enumerate(cr.pairs(5)) if g == h]
        assert np.all(twin[diag, 4] == 0.0) and np.all(twin[:, 0] == 0.0)  # the unit one-hot row, the empty row
        assert np.all(np.abs(c[diag, 4]) <= 2.0 ** -60)


def test_one_field_is_the_whole_score():
    fo, X, samples = case(9, 1, "contiguous", 1)
    w0, w, V = samples[0]
    c, _ = cr.components(sr.flat_rows(X), w, V, fo, 1)
    lin, pair = sr.fm_score_terms(X, (), w0, w, V)
    M, _ = sr.fm_score_bound(X, (), w0, w, V)  # (what the terms add up to in magnitude: a factor's term cancels inside)
    assert np.all(np.abs(c[0] - lin) <= 1e-17 * M)
    assert np.all(np.abs(c[1] - pair.sum(axis=1)) <= 1e-17 * M)


def test_permuting_the_fields_permutes_the_components():
    F = 4
    fo, X, samples = case(9, F, "interleaved", 1)
    _, w, V = samples[0]
    rows = sr.flat_rows(X)
    c, _ = cr.components(rows, w, V, fo, F)
    perm = np.array([2, 0, 3, 1])
    cp, _ = cr.components(rows, w, V, perm[fo], F)
    where = {gh: i for i, gh in enumerate(cr.pairs(F))}
    for g in range(F):
        assert np.array_equal(cp[perm[g]], c[g])
    for i, (g, h) in enumerate(cr.pairs(F)):
        a, b = sorted((int(perm[g]), int(perm[h])))
        assert np.all(np.abs(cp[F + where[(a, b)]] - c[F + i]) <= 2.0 ** -60 * np.maximum(np.abs(c[F + i]), 1e-300))


# ---- the kernel's arithmetic on the host ----
@pytest.mark.parametrize("K,F,kind,S", cr.shape_cases(), ids=lambda v: str(v))
def test_contrib_row_matches_the_reference(K, F, kind, S):
    from myfm_amd import _capi

    fo, X, samples = case(K, F, kind, S)
    ref = cr.Reference(X, (), samples, fo, F)
    mean, std = np.empty((F + len(cr.pairs(F)), 37)), np.empty((F + len(cr.pairs(F)), 37))
    for t in range(37):
        lo, hi = X.indptr[t], X.indptr[t + 1]
        mean[:, t], std[:, t] = _capi.contrib_row(X.indices[lo:hi], X.data[lo:hi], samples, F, fo)
    (lin, inter), (lin_std, inter_std) = ref.split(mean), ref.split(std)
    ref.check((float(ref.bias), float(ref.bias_std), lin, lin_std, inter, inter_std), "contrib_row K=%d F=%d %s S=%d" % (K, F, kind, S))
    # the float64 twin takes the kernel's orders: the host entry gives its bits
    assert np.array_equal(mean, ref.twin_mean) and np.array_equal(std, ref.twin_std)
    assert np.all(mean[:, 0] == 0.0) and np.all(std[:, 0] == 0.0)  # the empty row
    diag = [F + i for i, (g, h) in enumerate(cr.pairs(F)) if g == h]
    assert np.all(mean[diag, 4] == 0.0) and np.all(std[diag, 4] == 0.0)  # one unit entry per field
    if S == 1:
        assert np.all(std == 0.0)


def test_contrib_row_through_the_binding_is_the_same():
    from myfm_amd import _capi, _myfm

    fo, X, samples = case(9, 3, "interleaved", 5)
    ws = np.stack([s[1] for s in samples])
    Vs = np.stack([np.ascontiguousarray(s[2].T) for s in samples])
    lo, hi = X.indptr[3], X.indptr[4]
    a = _myfm.contrib_row(X.indices[lo:hi], X.data[lo:hi], ws, Vs, 3, fo)
    b = _capi.contrib_row(X.indices[lo:hi], X.data[lo:hi], samples, 3, fo)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- argument checks ----
def test_contrib_row_argument_checks():
    from myfm_amd import _capi

    fo, X, samples = case(3, 3, "contiguous", 2)
    idx, val = X.indices[X.indptr[3]:X.indptr[4]], X.data[X.indptr[3]:X.indptr[4]]
    with pytest.raises(Exception, match="field_of holds one field per column of the design: 69 expected, got 68"):
        _capi.contrib_row(idx, val, samples, 3, fo[:-1])
    with pytest.raises(Exception, match=r"field_of\[8\] = 1 lies outside \[0, 1\)"):
        _capi.contrib_row(idx, val, samples, 1, fo)
    bad = fo.copy()
    bad[5] = 3
    with pytest.raises(Exception, match=r"field_of\[5\] = 3 lies outside \[0, 3\)"):
        _capi.contrib_row(idx, val, samples, 3, bad)
    for F in (0, 17):
        with pytest.raises(Exception, match=r"the number of fields must lie in \[1, 16\], got %d" % F):
            _capi.contrib_row(idx, val, samples, F, np.zeros(cr.D_TEST, dtype=np.int32))


def fake_fitted(cls, D=6, with_grouping=True):
    """an estimator that passes for fitted as far as the host-side checks of predict_contributions go"""
    est = cls(2)

    class P:
        feature_size = D

        def predict_contributions(self, *a):
            raise AssertionError("the checks let the call through")

    est.predictor_ = P()
    if with_grouping:
        est.grouping_ = None
    return est


def test_estimator_argument_checks():
    import myfm_amd

    X = sps.identity(6, format="csr")
    est = fake_fitted(myfm_amd.MyFMGibbsRegressor)
    with pytest.raises(ValueError, match="give grouping or group_shapes, not both"):
        est.predict_contributions(X, grouping=[0] * 6, group_shapes=[6])
    with pytest.raises(ValueError, match="one field per column: 6 expected"):
        est.predict_contributions(X, grouping=[0] * 5)
    with pytest.raises(ValueError, match="one field per column: 6 expected"):
        est.predict_contributions(X, group_shapes=[3, 2])
    with pytest.raises(ValueError, match="negative field"):
        est.predict_contributions(X, grouping=[0, 0, -1, 0, 0, 0])
    with pytest.raises(ValueError, match="serves 1 to 16 fields, got 17"):
        est.predict_contributions(X, grouping=[0, 0, 16, 0, 0, 0])
    with pytest.raises(ValueError, match="serves 1 to 16 fields, got 0"):
        est.predict_contributions(X, group_shapes=[])
    old = fake_fitted(myfm_amd.MyFMGibbsClassifier, with_grouping=False)
    with pytest.raises(ValueError, match="no grouping_.*pass grouping or group_shapes"):
        old.predict_contributions(X)
    with pytest.raises(AssertionError, match="the checks let the call through"):
        old.predict_contributions(X, group_shapes=[4, 2])


def test_public_surface():
    import myfm_amd

    assert "ScoreContributions" in myfm_amd.__all__
    assert myfm_amd.ScoreContributions._fields == ("bias", "bias_std", "linear", "linear_std", "interaction", "interaction_std", "pairs")
    for name in ("MyFMGibbsRegressor", "MyFMGibbsClassifier", "MyFMOrderedProbit", "MyFMRegressor", "MyFMClassifier"):
        cls = getattr(myfm_amd, name)
        assert callable(getattr(cls, "predict_contributions"))
        assert "score scale" in cls.predict_contributions.__doc__.lower()
        with pytest.raises(RuntimeError, match="Predictor called before fit"):
            cls(2).predict_contributions(sps.identity(3, format="csr"))
    for name in ("VariationalFMRegressor", "VariationalFMClassifier"):
        assert not hasattr(getattr(myfm_amd, name), "predict_contributions")


def test_symbols_are_declared_listed_and_exported():
    from myfm_amd import _build, _capi

    header = open(os.path.join(ROOT, "include", "myfm_hip.h")).read()
    lib = ctypes.CDLL(_build.HIP_LIB)
    for name in ("mfm_design_contrib_store", "mfm_design_contrib", "mfm_contrib_row"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
        assert getattr(lib, name)
    assert callable(_capi.Design.contributions) and callable(_capi.Store.contributions) and callable(_capi.contrib_row)


# ---- utils.evaluation ----
def hand_made():
    import myfm_amd

    lin = np.array([[1.0, -2.0], [0.5, 0.0]])
    lin_std = np.array([[0.1, 2.0], [0.5, 0.0]])
    inter = np.array([[0.0, 0.0], [3.0, -1.0], [0.25, 0.5]])
    inter_std = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.1]])
    return myfm_amd.ScoreContributions(10.0, 0.5, lin, lin_std, inter, inter_std, np.array([[0, 0], [0, 1], [1, 1]]))


def test_contribution_total():
    from myfm_amd.utils.evaluation import contribution_total

    assert np.array_equal(contribution_total(hand_made()), np.array([10 + 1.5 + 3.25, 10 - 2.0 - 0.5]))


def test_contribution_matrix():
    from myfm_amd.utils.evaluation import contribution_matrix

    mean, std = contribution_matrix(hand_made(), 1)
    assert np.array_equal(mean, np.array([[0.0, -1.0], [-1.0, 0.5]]))
    assert np.array_equal(std, np.array([[0.0, 1.0], [1.0, 0.1]]))


def test_contribution_summary():
    from myfm_amd.utils.evaluation import contribution_summary

    out = contribution_summary(hand_made())
    assert np.array_equal(out["linear"]["magnitude"], [1.5, 0.25])
    assert np.array_equal(out["interaction"]["magnitude"], [0.0, 2.0, 0.375])
    total = 1.5 + 0.25 + 2.0 + 0.375
    assert np.allclose(out["linear"]["share"], np.array([1.5, 0.25]) / total, rtol=1e-15)
    assert np.allclose(out["interaction"]["share"], np.array([0.0, 2.0, 0.375]) / total, rtol=1e-15)
    assert np.array_equal(out["linear"]["significant"], [0.5, 0.0])       # |1| > 0.2; |-2| > 4 no; 0.5 > 1 no; 0 > 0 no
    assert np.array_equal(out["interaction"]["significant"], [0.0, 0.5, 0.5])  # 3 > 2; 1 > 2 no; .25 > 1 no; .5 > .2
    assert np.array_equal(out["pairs"], [[0, 0], [0, 1], [1, 1]])
