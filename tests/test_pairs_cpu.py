"""Query x candidate scoring, the parts that need no GPU: the algebra of the decomposition against the direct
pair-row reference, and the argument checks of predict_pairs / predict_topk, which run on the host before the device is
looked for."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_ref as pr


@pytest.mark.parametrize("K,S,mode", [(0, 2, 0), (3, 1, 0), (8, 4, 0), (8, 4, 1), (33, 3, 1)])
def test_decomposition_equals_direct_pair_rows(K, S, mode):
    """w0 + A[u] + B[i] + P[u] . Q[i] is the FM score of the row a_u + b_i when the sides share no column: the cross term
    sum_j V[k, j]^2 a_uj b_ij of the squares vanishes. 1e-12 relative to the sum of absolute terms (Phi is 0.4-Lipschitz)."""
    rng = np.random.default_rng(100 + K + S)
    Xq, Xc, D = pr.disjoint_sides(rng, 23, 41, 19, 27, [1.0, -1.0, 2.0, -2.0, 0.5], mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    ref = pr.pair_scores(samples, Xq, Xc, mode)
    got = pr.decomposed_scores(samples, Xq, Xc, mode)
    bound = 1e-12 * pr.pair_scores_abs(samples, Xq, Xc)
    assert np.all(np.abs(got - ref) <= bound)
    # ... and it is the cross term that makes the difference: with a shared column the two disagree
    Xc2 = Xc.tolil()
    Xc2[0, 0] = 1.0
    Xq2 = Xq.tolil()
    Xq2[0, 0] = 1.0
    if K:
        d = pr.decomposed_scores(samples, Xq2.tocsr(), Xc2.tocsr(), 0)[0, 0] - pr.pair_scores(samples, Xq2.tocsr(), Xc2.tocsr(), 0)[0, 0]
        assert abs(d) > 1e-6


def test_reference_topk_order_and_tail():
    s = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    idx, val = pr.topk(s, 4)
    assert idx.tolist() == [[1, 2, 4, 3], [0, 1, 2, 3]] and val[0].tolist() == [3.0, 3.0, 3.0, 2.0]
    ex = sps.csr_matrix(np.array([[0, 1, 0, 0, 1], [1, 1, 1, 1, 0]]))
    idx, val = pr.topk(s, 4, ex)
    assert idx.tolist() == [[2, 3, 0, -1], [4, -1, -1, -1]] and val[1, 1] == -np.inf


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
def test_pair_argument_checks_need_no_gpu(cls, task):
    from myfm_amd import _capi, _myfm

    est = _restored(cls, getattr(_myfm.TaskType, task))
    Xq = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, 12))
    Xc = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 7, 8])), shape=(4, 12))
    shared = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 2, 8])), shape=(4, 12))
    with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
        est.predict_topk(Xq, shared, 2)
    with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
        est.predict_pairs(Xq, shared)
    with pytest.raises(ValueError, match="Told to predict for 11 but this->feature_size is 12"):
        est.predict_topk(Xq[:, :11], Xc[:, :11], 2)
    with pytest.raises(ValueError, match="Told to predict for 13"):
        est.predict_pairs(Xq, sps.csr_matrix((4, 13)))
    for k in (0, 257, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            est.predict_topk(Xq, Xc, k)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.predict_topk(Xq, Xc, 2, exclude=sps.csr_matrix((4, 3)))
    big_q, big_c = sps.csr_matrix((4097, 12)), sps.csr_matrix((4096, 12))
    with pytest.raises(ValueError, match="predict_topk"):
        est.predict_pairs(big_q, big_c)
    # the C ABI makes the same checks before it looks for a device
    with pytest.raises(ValueError, match="X_query and X_cand share column 2"):
        _capi.Pairs(Xq, shared)
    # valid arguments: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_topk(Xq, Xc, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_pairs(Xq, Xc)


def test_variational_predictor_has_the_methods():
    from myfm_amd import VariationalFMClassifier, VariationalFMRegressor, _myfm

    for cls in (VariationalFMRegressor, VariationalFMClassifier):
        assert callable(cls.predict_pairs) and callable(cls.predict_topk)
    assert hasattr(_myfm.VariationalPredictor, "predict_topk") and hasattr(_myfm.VariationalPredictor, "predict_pairs")
    with pytest.raises(RuntimeError, match="Predictor called before fit"):
        VariationalFMRegressor(2).predict_topk(sps.csr_matrix((1, 3)), sps.csr_matrix((1, 3)), 1)
