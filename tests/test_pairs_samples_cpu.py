"""Ranking under each kept sample, the parts that need no GPU: the reference vote against a brute-force count,
the exports, and the argument checks of predict_topk_samples / predict_topk_thompson / predict_topk_prob, which run on the
host before the device is looked for."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_samples_ref as sref
from tests.test_pairs_ucb_cpu import _restored

NEW_SYMBOLS = ("mfm_pairs_topk_samples_store", "mfm_pairs_topk_samples", "mfm_pairs_topk_prob_store", "mfm_pairs_topk_prob")
METHODS = ("predict_topk_samples", "predict_topk_thompson", "predict_topk_prob")


@pytest.mark.parametrize("S,U,k,I", [(1, 3, 4, 9), (5, 7, 10, 12), (37, 4, 16, 20), (8, 5, 6, 3)])
def test_vote_against_a_brute_force_count(S, U, k, I):
    """random lists without repeats within a list, with tails where the candidates run out (I < k) or at random, and few
    candidates so that the counts tie heavily: a dict count sorted by (-count, index) must give the same entries"""
    rng = np.random.default_rng(S + 10 * k)
    idx = np.full((S, U, k), -1, dtype=np.int64)
    for s in range(S):
        for u in range(U):
            n = min(k, I) if (s + u) % 3 else int(rng.integers(0, min(k, I) + 1))
            idx[s, u, :n] = rng.choice(I, size=n, replace=False)
    for n_top in (1, k, 256):
        got_i, got_p = sref.vote(idx, n_top)
        assert got_i.shape == (U, n_top) and got_p.shape == (U, n_top) and got_i.dtype == np.int64
        for u in range(U):
            count = {}
            for s in range(S):
                for c in idx[s, u]:
                    if c >= 0:
                        count[int(c)] = count.get(int(c), 0) + 1
            best = sorted(count.items(), key=lambda t: (-t[1], t[0]))[:n_top]
            assert [c for c, _ in best] == list(got_i[u, :len(best)])
            assert [n / S for _, n in best] == list(got_p[u, :len(best)])
            assert np.all(got_i[u, len(best):] == -1) and np.all(got_p[u, len(best):] == 0.0)
    # every list complete and I >= k: a row's probabilities add up to k when every candidate is returned
    if I >= k:
        full = np.stack([np.stack([rng.choice(I, size=k, replace=False) for _ in range(U)]) for _ in range(S)])
        _, p = sref.vote(full, 256)
        assert np.allclose(p.sum(axis=1), k)


def test_thompson_samples_is_the_documented_draw():
    assert np.array_equal(sref.thompson_samples(7, 13, 50), np.random.default_rng(7).integers(0, 13, size=50))
    assert sref.thompson_samples(0, 1, 9).tolist() == [0] * 9


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    header = open(os.path.join(root, "include", "myfm_hip.h")).read()
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", header))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    for m in ("topk_samples", "topk_samples_store", "topk_prob", "topk_prob_store"):
        assert callable(getattr(_capi.Pairs, m))
    # the vote's limit: one number in the header, in _capi and in the estimators, and enough for 95 samples x k = 256
    limit = int(re.search(r"#define MFM_PAIRS_VOTE_MAX (\d+)", header).group(1))
    assert limit == _capi.PAIRS_VOTE_MAX == myfm_amd.estimators.TOPK_PROB_MAX_VOTES and limit >= 24320


def test_who_has_the_methods():
    import myfm_amd

    assert myfm_amd.SampleRankings._fields == ("indices", "value")
    assert myfm_amd.ThompsonRanking._fields == ("indices", "value", "sample")
    assert myfm_amd.TopKProbability._fields == ("indices", "probability")
    for name in ("SampleRankings", "ThompsonRanking", "TopKProbability"):
        assert name in myfm_amd.__all__
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.MyFMRegressor,
                myfm_amd.MyFMClassifier):
        for m in METHODS:
            assert callable(getattr(cls, m)), (cls, m)
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier, myfm_amd._myfm.VariationalPredictor):
        for m in METHODS:
            assert not hasattr(cls, m), (cls, m)
    for m in METHODS:
        assert hasattr(myfm_amd._myfm.Predictor, m)
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        myfm_amd.MyFMOrderedProbit(2).predict_topk_prob(sps.csr_matrix((1, 3)), sps.csr_matrix((1, 3)), 1)


@pytest.mark.parametrize("cls,task", [("MyFMRegressor", "REGRESSION"), ("MyFMClassifier", "CLASSIFICATION")])
def test_argument_checks_need_no_gpu(cls, task):
    from myfm_amd import _myfm

    est = _restored(cls, getattr(_myfm.TaskType, task))
    Xq = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, 12))
    Xc = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 7, 8])), shape=(4, 12))
    shared = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 2, 8])), shape=(4, 12))
    calls = [getattr(est, m) for m in METHODS]
    # what predict_topk_ucb refuses for the same sides, k and exclude, with its messages
    for call in calls:
        with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
            call(Xq, shared, 2)
        with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
            call(Xq[:, :11], Xc[:, :11], 2)
        for k in (0, 257, -1, 2.5):
            with pytest.raises(ValueError, match="k must be"):
                call(Xq, Xc, k)
        with pytest.raises(ValueError, match="exclude must have shape"):
            call(Xq, Xc, 2, exclude=sps.csr_matrix((4, 3)))
    # the methods' own
    for seed in (-1, True, 1.5, "0", None, [0]):
        with pytest.raises(ValueError, match="random_seed must be a non-negative integer"):
            est.predict_topk_thompson(Xq, Xc, 2, random_seed=seed)
    for n_top in (0, 257, -3, True, 2.5, "3"):
        with pytest.raises(ValueError, match="n_top must be an integer in"):
            est.predict_topk_prob(Xq, Xc, 2, n_top=n_top)
    many = _restored(cls, getattr(_myfm.TaskType, task), S=129)  # 129 * 256 = 33024 list entries per query
    with pytest.raises(ValueError, match="at most 32768 list entries per query"):
        many.predict_topk_prob(Xq, Xc, 256)
    with pytest.raises(ValueError, match="k must be"):
        many.predict_topk_prob(Xq, Xc, 257)
    # valid arguments: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        for call, kw in ((calls[0], {}), (calls[1], {"random_seed": 3}), (calls[1], {"random_seed": np.int64(0)}), (calls[2], {}),
                         (calls[2], {"n_top": 256}), (calls[2], {"n_top": np.int32(1)})):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(Xq, Xc, 2, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            many.predict_topk_prob(Xq, Xc, 254)
