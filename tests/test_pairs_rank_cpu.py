"""Ranks of held-out pairs, the parts that need no GPU: the brute-force rank reference on a hand-checked case,
ranking_metrics against a direct computation from the dense score matrix, the argument checks of predict_rank, which run on the
host before the device is looked for, and the exports."""
import os
import re
import subprocess
from collections import namedtuple

import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_rank_ref as kr

Result = namedtuple("Result", ["rank", "value", "n_candidates"])


def _pattern(rows, U, I):
    r = [u for u, cols in rows.items() for _ in cols]
    c = [j for cols in rows.values() for j in cols]
    return sps.csr_matrix((np.ones(len(r)), (r, c)), shape=(U, I))


# ---- a case small enough to count by hand: U = 6, I = 9 -------------------------------------------------------------------------
def hand_case():
    down = np.arange(9, 0, -1.0)  # column j holds 9 - j: the order of the columns is the ranking
    scores = np.stack([down, down, np.full(9, 5.0), down, np.asarray([0, 3, 0, 0, 0, 7, 0, 0, 0.0]), down])
    targets = _pattern({0: [0], 1: [2, 4, 8], 2: [3], 4: [1, 5], 5: [8]}, 6, 9)  # (row 3 has none)
    exclude = _pattern({4: [0, 2, 3, 4, 6, 7, 8], 5: [0, 1]}, 6, 9)           # (row 4: everything but its targets)
    return scores, targets, exclude


def test_rank_ref_on_the_hand_case():
    scores, targets, exclude = hand_case()
    for ref in (kr.rank_ref, kr.rank_ref_fast):
        rank, value, n_cand = ref(scores, targets, exclude)
        # row 1: the targets at columns 2, 4, 8 have 2, 4, 8 better columns (other targets count); row 2: all values tie and the
        # three smaller indices win; row 4: nothing but the two targets is left, 7 > 3; row 5: 8 better columns, two excluded
        assert rank.tolist() == [0, 2, 4, 8, 3, 1, 0, 6]
        assert value.tolist() == [9.0, 7.0, 5.0, 1.0, 5.0, 3.0, 7.0, 1.0]
        assert n_cand.tolist() == [9, 9, 9, 9, 2, 7]
    rank, _, _ = kr.rank_ref(scores, targets)
    assert rank.tolist() == [0, 2, 4, 8, 3, 1, 0, 8]  # (without exclusions: row 4's zeros lose to both targets, row 5 has 8 ahead)


def test_metrics_on_the_hand_case():
    from myfm_amd.utils.ranking import ranking_metrics

    scores, targets, exclude = hand_case()
    got = ranking_metrics(Result(*kr.rank_ref(scores, targets, exclude)), targets, k=3)
    l3 = 1.0 / np.log2(3.0)
    want = {
        "hit_rate@3": 3 / 5,                                   # min r = 0, 2, 3, 0, 6
        "recall@3": (1 + 1 / 3 + 0 + 1 + 0) / 5,
        "ndcg@3": (1 + 0.5 / (1 + l3 + 0.5) + 0 + 1 + 0) / 5,  # row 1: only rank 2 is inside, ideal 1 + 1/log2(3) + 1/2
        "mrr": (1 + 1 / 3 + 1 / 4 + 1 + 1 / 7) / 5,
        "mean_rank": (0 + (2 + 3 + 6) + 3 + (0 + 0) + 6) / 8,  # r': the rank among the non-targets
        "auc": (1 + (1 - 11 / 18) + (1 - 3 / 8) + 0) / 4,      # (row 4 has no non-target left and stays out)
        "n_queries": 5,
    }
    assert set(got) == set(want)
    for name in want:
        assert got[name] == pytest.approx(want[name], rel=1e-14, abs=0), name
    ref = kr.metrics_ref(scores, targets, exclude, k=3)
    for name in want:
        assert ref[name] == pytest.approx(want[name], rel=1e-14, abs=0), name


@pytest.mark.parametrize("k", [1, 3, 10])
@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_metrics_match_the_direct_computation(seed, tied, k):
    """U = 6, I = 9; 0, 1 or 3 targets per row; with `tied` the scores take three values only, so the index order decides most
    comparisons; one row has everything but its targets excluded"""
    from myfm_amd.utils.ranking import ranking_metrics

    rng = np.random.default_rng(seed)
    U, I = 6, 9
    scores = rng.integers(0, 3, size=(U, I)).astype(np.float64) if tied else rng.normal(size=(U, I))
    targets = kr.draw_targets(rng, U, I, [0, 1, 3], ties_from=scores)
    exclude = kr.exclude_without(rng, U, I, 0.3, targets).tolil()
    full = 2  # (a row with three targets)
    exclude[full, :] = 1.0
    exclude[full, targets[full].indices] = 0.0
    exclude = sps.csr_matrix(exclude)
    exclude.eliminate_zeros()
    for ex in (None, exclude):
        res = Result(*kr.rank_ref(scores, targets, ex))
        got, want = ranking_metrics(res, targets, k=k), kr.metrics_ref(scores, targets, ex, k=k)
        assert set(got) == set(want)
        for name in want:
            assert got[name] == pytest.approx(want[name], rel=1e-13, abs=1e-15), (name, ex is None)
    assert set(res.rank[targets.indptr[full]:targets.indptr[full + 1]].tolist()) == {0, 1, 2}  # only the targets are left in that row


def test_auc_of_a_perfect_and_a_reversed_ranking():
    from myfm_amd.utils.ranking import ranking_metrics

    U, I = 4, 9
    scores = np.tile(np.arange(I, 0, -1.0), (U, 1))
    best = _pattern({0: [0], 1: [0, 1, 2], 3: [0, 1]}, U, I)
    worst = _pattern({0: [8], 1: [6, 7, 8], 3: [7, 8]}, U, I)
    for targets, auc in ((best, 1.0), (worst, 0.0)):
        got = ranking_metrics(Result(*kr.rank_ref(scores, targets)), targets)
        assert got["auc"] == auc and got["n_queries"] == 3
        assert kr.metrics_ref(scores, targets)["auc"] == auc
    assert ranking_metrics(Result(*kr.rank_ref(scores, best)), best)["mean_rank"] == 0.0
    assert ranking_metrics(Result(*kr.rank_ref(scores, best)), best, k=3)["ndcg@3"] == 1.0


def test_metrics_without_any_target_and_bad_arguments():
    from myfm_amd.utils.ranking import ranking_metrics

    empty = sps.csr_matrix((3, 5))
    got = ranking_metrics(Result(np.empty(0, dtype=np.int64), np.empty(0), np.full(3, 5)), empty)
    assert got["n_queries"] == 0 and np.isnan(got["mrr"]) and np.isnan(got["auc"]) and np.isnan(got["hit_rate@10"])
    one = _pattern({1: [2]}, 3, 5)
    with pytest.raises(ValueError, match="does not belong"):
        ranking_metrics(Result(np.zeros(2, dtype=np.int64), np.zeros(2), np.full(3, 5)), one)
    for k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            ranking_metrics(Result(np.zeros(1, dtype=np.int64), np.zeros(1), np.full(3, 5)), one, k=k)


# ---- the argument checks of predict_rank -------------------------------------------------------------------------------------------
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
def test_rank_argument_checks_need_no_gpu(cls, task):
    from myfm_amd import _myfm

    est = _restored(cls, getattr(_myfm.TaskType, task))
    Xq = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, 12))
    Xc = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 7, 8])), shape=(4, 12))
    shared = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 2, 8])), shape=(4, 12))
    targets = _pattern({0: [1], 2: [0, 3]}, 3, 4)
    with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
        est.predict_rank(Xq, shared, targets)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        est.predict_rank(Xq[:, :11], Xc[:, :11], targets)
    for bad in (sps.csr_matrix((4, 3)), sps.csr_matrix((3, 5)), None, np.zeros((3, 4))):
        with pytest.raises(ValueError, match="targets must"):
            est.predict_rank(Xq, Xc, bad)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.predict_rank(Xq, Xc, targets, exclude=sps.csr_matrix((4, 3)))
    with pytest.raises(ValueError, match=r"query row 2, candidate 3\) is also excluded"):
        est.predict_rank(Xq, Xc, targets, exclude=_pattern({0: [0], 2: [1, 3]}, 3, 4))
    # the binding checks its own arguments, whoever calls it
    p = est.predictor_
    with pytest.raises(ValueError, match=r"query row 2, candidate 3\) is also excluded"):
        p.predict_rank(Xq, Xc, targets, _pattern({2: [3]}, 3, 4))
    with pytest.raises(ValueError, match="targets must have shape"):
        p.predict_rank(Xq, Xc, sps.csr_matrix((3, 5)))
    unsorted = sps.csr_matrix((np.ones(2), np.asarray([3, 0], dtype=np.int32), np.asarray([0, 0, 0, 2])), shape=(3, 4))
    with pytest.raises(ValueError, match="query row 2 must be sorted and unique"):
        p.predict_rank(Xq, Xc, unsorted)
    wide_c = sps.csr_matrix((70, 12))
    with pytest.raises(ValueError, match="query row 1 has 65 targets, a call takes at most 64"):
        p.predict_rank(Xq, wide_c, _pattern({1: list(range(65))}, 3, 70))
    # valid arguments -- 65 targets in a row among them, which the estimator splits: the usual refusal of a machine without a
    # GPU comes only now
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_rank(Xq, Xc, targets, exclude=_pattern({0: [0], 2: [1]}, 3, 4))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_rank(Xq, wide_c, _pattern({1: list(range(65))}, 3, 70))


def test_who_has_the_method():
    import myfm_amd

    assert myfm_amd.TargetRanks._fields == ("rank", "value", "n_candidates")
    assert "TargetRanks" in myfm_amd.__all__
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit, myfm_amd.VariationalFMRegressor,
                myfm_amd.VariationalFMClassifier):
        assert callable(cls.predict_rank) and callable(cls.predict_topk)
    assert callable(myfm_amd._myfm.Predictor.predict_rank) and callable(myfm_amd._myfm.VariationalPredictor.predict_rank)
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        myfm_amd.MyFMOrderedProbit(2).predict_rank(sps.csr_matrix((1, 3)), sps.csr_matrix((1, 3)), sps.csr_matrix((1, 1)))


def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(myfm_amd.__file__)))
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", open(os.path.join(root, "include", "myfm_hip.h")).read()))
    L = _capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in ("mfm_pairs_set_targets", "mfm_pairs_rank_store", "mfm_pairs_rank"):
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    for m in ("rank", "rank_store"):
        assert callable(getattr(_capi.Pairs, m))
