"""Ranking by an upper confidence bound, the parts that need no GPU: the float64 twin of the kernels' moment
recurrence against longdouble, the exact cases, the argument checks of predict_pairs_dist / predict_topk_ucb, which run on the
host before the device is looked for, and the exports."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests import pairs_ucb_ref as ur

HALVES = [1.0, -1.0, 2.0, -2.0, 0.5]
NEW_SYMBOLS = ("mfm_pairs_moments_store", "mfm_pairs_moments", "mfm_pairs_topk_ucb_store", "mfm_pairs_topk_ucb")


@pytest.mark.parametrize("mode,n_cut", [(0, 0), (1, 0), (2, 1), (2, 4)])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_twin_meets_the_recurrence_term(K, S, mode, n_cut):
    """On the GPU test's real-valued cases (fewer candidates) the float64 twin, fed the float64 per-sample values, differs from
    the longdouble moments of the same values by less than the recurrence's share of the std tolerance, 4 S 2^-53 rms(v), and in
    the mean by less than S 2^-53 max|v|."""
    rng = np.random.default_rng(31 + K + S + n_cut)
    Xq, Xc, D = pr.disjoint_sides(rng, 37, 200, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    cuts = rr.sorted_cuts(rng, S, n_cut) if mode == 2 else None
    v64 = np.asarray(ur.sample_values(samples, Xq, Xc, mode, cuts), dtype=np.float64)
    mean, std = ur.welford_twin(v64)
    rmean, rstd = ur.moments_ld(v64)
    term = ur.recurrence_term(v64) + 1e-300
    use_std = float((np.abs(std - rstd) / term).max())
    use_mean = float((np.abs(mean - rmean) / (S * ur.EPS * np.abs(v64).max(axis=0) + 1e-300)).max())
    print("K %d S %d mode %d n_cut %d: twin uses %.3g of the std term, %.3g of S eps max|v| in the mean" % (K, S, mode, n_cut, use_std, use_mean))
    assert use_std <= 1.0 and use_mean <= 1.0


def test_twin_keeps_a_common_offset_and_a_tiny_spread():
    """values 1e8 + small: the shifted problem's std comes out to the recurrence's term (relative to the values, as the tolerance
    is), where the raw sums of v and v^2 would lose it altogether"""
    rng = np.random.default_rng(3)
    small = rng.normal(size=(37, 500)) * 1e-3
    vals = 1e8 + small
    mean, std = ur.welford_twin(vals)
    rmean, rstd = ur.moments_ld(vals)
    assert np.all(np.abs(std - rstd) <= ur.recurrence_term(vals))
    raw = np.sqrt(np.maximum((vals ** 2).mean(axis=0) - vals.mean(axis=0) ** 2, 0.0))
    assert np.abs(raw - np.asarray(rstd, dtype=np.float64)).max() > 1e3 * np.abs(std - rstd).max()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_identical_samples_and_one_sample_give_zero_std(mode):
    rng = np.random.default_rng(8 + mode)
    Xq, Xc, D = pr.disjoint_sides(rng, 17, 60, 19, 27, HALVES, mean_nnz=3.0)
    one = pr.normal_samples(rng, D, 8, 1)
    cuts = rr.sorted_cuts(rng, 1, 3)
    for S in (1, 3):
        v64 = np.asarray(ur.sample_values(one * S, Xq, Xc, mode, np.repeat(cuts, S, axis=0)), dtype=np.float64)
        mean, std = ur.welford_twin(v64)
        assert np.all(std == 0.0) and np.array_equal(mean, v64[0])


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("K", [0, 3, 33])
def test_exact_data_claim(K, S):
    """small integers and halves with S <= 2: every v_s, the mean and var = (a - b)^2 / 4 are exact in fp64 and std = |a - b| / 2
    is an exact square root, so the twin equals longdouble bit for bit -- the claim the GPU test's exact layout rests on"""
    rng = np.random.default_rng(1000 + K + 7 * S)
    Xq, Xc, D = pr.disjoint_sides(rng, 37, 250, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    vals = ur.sample_values(pr.exact_samples(rng, D, K, S), Xq, Xc, 0)
    mean, std = ur.welford_twin(vals)
    rmean, rstd = ur.moments_ld(vals)
    assert np.array_equal(mean.astype(ur.LD), rmean) and np.array_equal(std.astype(ur.LD), rstd)
    for beta in (1.0, -2.0, 0.5):
        assert np.array_equal((mean + beta * std).astype(ur.LD), rmean + ur.LD(beta) * rstd)
    if K and S == 2:
        assert np.unique(std).size > 5 and np.unique(mean).size > 50


def _restored(cls, task, D=12, K=3, S=2):
    """an estimator around a Predictor restored through __setstate__ (no fit, no device)"""
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for _ in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(task), fms))
    est = getattr(myfm_amd, cls)(K)
    est.predictor_ = p
    return est


@pytest.mark.parametrize("cls,task", [("MyFMRegressor", "REGRESSION"), ("MyFMClassifier", "CLASSIFICATION")])
def test_ucb_argument_checks_need_no_gpu(cls, task):
    from myfm_amd import _myfm

    est = _restored(cls, getattr(_myfm.TaskType, task))
    Xq = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, 12))
    Xc = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 7, 8])), shape=(4, 12))
    shared = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 2, 8])), shape=(4, 12))
    with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
        est.predict_topk_ucb(Xq, shared, 2)
    with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
        est.predict_pairs_dist(Xq, shared)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        est.predict_topk_ucb(Xq[:, :11], Xc[:, :11], 2)
    with pytest.raises(ValueError, match="Told to predict for 13"):
        est.predict_pairs_dist(Xq, sps.csr_matrix((4, 13)))
    for k in (0, 257, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            est.predict_topk_ucb(Xq, Xc, k)
    for beta in (np.inf, -np.inf, np.nan, 1j, "1", None, [1.0]):
        with pytest.raises(ValueError, match="beta must be a finite"):
            est.predict_topk_ucb(Xq, Xc, 2, beta=beta)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.predict_topk_ucb(Xq, Xc, 2, exclude=sps.csr_matrix((4, 3)))
    big_q, big_c = sps.csr_matrix((4097, 12)), sps.csr_matrix((4096, 12))
    with pytest.raises(ValueError, match="predict_topk_ucb"):
        est.predict_pairs_dist(big_q, big_c)
    # valid arguments (a negative beta and beta = 0 among them): the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        for beta in (1.0, -2.0, 0, np.float32(0.5)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.predict_topk_ucb(Xq, Xc, 2, beta=beta)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_pairs_dist(Xq, Xc)


def test_who_has_the_methods():
    import myfm_amd

    assert myfm_amd.PairSummary._fields == ("mean", "std")
    assert myfm_amd.RankedSummary._fields == ("indices", "value", "mean", "std")
    assert "PairSummary" in myfm_amd.__all__ and "RankedSummary" in myfm_amd.__all__
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit):
        assert callable(cls.predict_pairs_dist) and callable(cls.predict_topk_ucb)
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_pairs_dist") and not hasattr(cls, "predict_topk_ucb")
        assert callable(cls.predict_topk)
    assert not hasattr(myfm_amd._myfm.VariationalPredictor, "predict_topk_ucb")
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        myfm_amd.MyFMOrderedProbit(2).predict_topk_ucb(sps.csr_matrix((1, 3)), sps.csr_matrix((1, 3)), 1)


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
    for m in ("moments", "moments_store", "topk_ucb", "topk_ucb_store"):
        assert callable(getattr(_capi.Pairs, m))
