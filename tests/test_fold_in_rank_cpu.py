"""Ranking under a new entity's own posterior, the parts that need no GPU: the reference of
tests/fold_in_rank_ref.py against fold_in_ref and score_ref, the prior closed form, the float64 twin's error against the
longdouble reference (the figure TWIN_C records), the host argument checks and the exported symbols."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import fold_in_rank_ref as rr
from tests import fold_in_ref as fr
from tests.test_fold_in_cpu import _restored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mfm_foldin_rank_set_candidates", "mfm_foldin_rank_set_exclude", "mfm_foldin_rank_dist_store", "mfm_foldin_rank_dist",
               "mfm_foldin_rank_topk_store", "mfm_foldin_rank_topk")
COUNTS = (0, 1, 2, 65, 0)


def _problem(K, fit_linear, S=3, I=9, D=20):
    rng = np.random.default_rng(900 + 2 * K + fit_linear)
    p = fr.problem(rng, D, K, S, len(COUNTS), counts=COUNTS)
    return p, fr.context_rows(rng, I, D)


@pytest.mark.parametrize("K,fit_linear", [(0, True), (3, True), (5, False)])
def test_mean_is_the_folded_models_score_and_the_prior_is_closed_form(K, fit_linear):
    """mean = the mean over the samples of the FM score of the D + U wide pair rows under fold_in_ref's posterior means; an entity
    without rows has v = sum_j z_j^2 / lambda_j and m = f + z . mu"""
    p, Xc = _problem(K, fit_linear)
    m, v, ref = rr.per_sample(p, Xc, fit_linear)
    U, I, o = p["U"], Xc.shape[0], 0 if fit_linear else 1
    w_new, V_new = fr.split(ref["theta"], fit_linear, K)
    rows = sps.hstack([sps.vstack([Xc] * U), sps.kron(sps.identity(U), np.ones((I, 1)))]).tocsr()
    for s in range(p["S"]):
        ext = fr.extend_sample(p["samples"][s], w_new[s].astype(np.float64), V_new[s].astype(np.float64))
        direct = fr.mean_score([ext], rows).reshape(U, I)
        assert np.all(np.abs(direct - m[s].astype(np.float64)) <= 1e-12 * (1 + np.abs(direct)))
        z, f = rr.candidate_terms(p["samples"][s], Xc, fit_linear)
        for u in np.flatnonzero(p["counts"] == 0):
            want_v = (z * z / ref["lam"][s]).sum(axis=1)
            assert np.all(np.abs(v[s, u] - want_v) <= 1e-17 * (1 + want_v))
            assert np.all(np.abs(m[s, u] - (f + np.dot(z, ref["mu"][s]))) <= 1e-17 * (1 + np.abs(m[s, u])))
    out = rr.summarise(m, v, p["alpha"])
    assert np.all(out["std"] >= out["std_within"]) and (K + fit_linear == 0 or np.all(out["std_within"] > 0))


@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 14, 15, 16, 31, 32, 63, 64])
def test_float64_twin_stays_within_the_recorded_constant(K, fit_linear):
    """the twin's largest error / unit bound over this grid is what TWIN_C records (the device gets 8 times that)"""
    p, Xc = _problem(K, fit_linear, S=2, I=17, D=40)
    want, bound, cond = rr.summary(p, Xc, fit_linear)
    assert cond.max() <= 1e5
    w = rr.worst(rr.summary_f64(p, Xc, fit_linear), want, bound)
    print("fold-in rank twin K=%d fit_linear=%d: error / bound = %.4f" % (K, fit_linear, w))
    assert w <= rr.TWIN_C


def test_argument_checks_need_no_gpu():
    import myfm_amd
    from myfm_amd import _myfm

    est = _restored()
    X, Xc = sps.csr_matrix(np.eye(4, 6)), sps.csr_matrix(np.eye(5, 6))
    y, ent = np.arange(4.0), np.array([1, 0, 1, 2])
    for call in (lambda **kw: est.fold_in_topk(kw.pop("X", X), y, ent, 0, kw.pop("Xc", Xc), kw.pop("k", 2), **kw),
                 lambda **kw: est.fold_in_pairs_dist(kw.pop("X", X), y, ent, 0, kw.pop("Xc", Xc))):
        with pytest.raises(ValueError, match="X has 5 columns but the fitted feature size is 6"):  # fold_in's own checks, first
            call(X=sps.csr_matrix((4, 5)))
        with pytest.raises(ValueError, match="X_cand has 7 columns"):
            call(Xc=sps.csr_matrix((5, 7)))
    for k in (0, 257, 1.5):
        with pytest.raises(ValueError, match=r"k must be an integer in \[1, 256\]"):
            est.fold_in_topk(X, y, ent, 0, Xc, k)
    with pytest.raises(ValueError, match="by must be 'ucb' or 'gain'"):
        est.fold_in_topk(X, y, ent, 0, Xc, 2, by="mean")
    for beta in (np.nan, np.inf, "1"):
        with pytest.raises(ValueError, match="beta must be a finite real number"):
            est.fold_in_topk(X, y, ent, 0, Xc, 2, beta=beta)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.fold_in_topk(X, y, ent, 0, Xc, 2, exclude=sps.csr_matrix((3, 4)))
    with pytest.raises(ValueError, match="2\\^24 pairs"):
        est.fold_in_pairs_dist(X, y, ent, 0, sps.csr_matrix((1 << 23, 6)))
    if _myfm.device_count() == 0:  # valid arguments: the refusal of a machine without a GPU comes only now
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fold_in_topk(X, y, ent, 0, Xc, 2, by="gain", exclude=sps.csr_matrix((3, 5)))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fold_in_pairs_dist(X, y, ent, 1, Xc)


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi, _myfm

    with open(os.path.join(ROOT, "include", "myfm_hip.h")) as f:
        declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", f.read()))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(_capi.lib(), name), name
    assert myfm_amd.ColdStartRanking._fields == ("indices", "value", "mean", "std", "gain")
    assert myfm_amd.ColdStartSummary._fields == ("mean", "std", "std_within", "gain")
    assert hasattr(_myfm.Predictor, "fold_in_topk") and hasattr(_myfm.Predictor, "fold_in_pairs_dist")
