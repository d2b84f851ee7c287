"""The diversified top-k without a device: the reference's own identities, the conditioning of the inputs the GPU
tests use, the host-side refusals and the exports."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_diverse_ref as dr
from tests import pairs_ref as pr
from tests.test_pairs_sim_cpu import _restored


@pytest.mark.parametrize("K,S", [(8, 5), (33, 5), (8, 37), (33, 37)])
def test_reference_identities_and_seeds(K, S):
    """on the GPU tests' real-valued inputs: the spread and the brackets they rely on; the reference's list passes its own replay with
    nothing used of the tolerance; lam = 1 is the pool's head; a wrong pick and a wrong objective are caught"""
    samples, Xq, Xc, ex = dr.real_case(K, S)
    sim, b_sim = dr.similarity(samples, Xc)  # (asserts the brackets)
    b_v = dr.value_bound(samples, Xq, Xc)
    for M in (32, 128):
        dr.assert_spread(samples, Xq, Xc, ex, M)
        pool = pr.topk(pr.pair_scores(samples, Xq, Xc, 0), M, ex)
        for lam in (1.0, 0.7, 0.3):
            res = tuple(np.stack(x) for x in zip(*[dr.greedy(pool[0][u], pool[1][u], sim, lam, M // 2) for u in range(Xq.shape[0])]))
            assert dr.check_replay(res, pool, sim, b_sim, b_v, lam) < 1e-3
            head = np.array_equal(res[0], pool[0][:, :M // 2]) and np.array_equal(res[1], pool[1][:, :M // 2])
            assert head == (lam == 1.0)  # (lam = 1 is the pool's head; diversification changes the list)
        bad = tuple(x.copy() for x in res)
        bad[2][0, 3] += 1e-6
        with pytest.raises(AssertionError):
            dr.check_replay(bad, pool, sim, b_sim, b_v, 0.3)
        bad = tuple(x.copy() for x in res)
        bad[0][0, 2] = bad[0][0, 1]  # (a candidate twice)
        with pytest.raises(AssertionError):
            dr.check_replay(bad, pool, sim, b_sim, b_v, 0.3)
    assert [dr.default_pool(k) for k in (1, 8, 10, 32, 100)] == [32, 32, 40, 128, 128]


@pytest.mark.parametrize("cls,task", [("MyFMRegressor", "REGRESSION"), ("MyFMClassifier", "CLASSIFICATION"), ("MyFMOrderedProbit", "ORDERED")])
def test_value_errors_without_a_device(cls, task):
    from myfm_amd import _myfm

    est = _restored(cls, task)
    Xq, Xc = sps.csr_matrix(([1.0, 1.0], ([0, 1], [0, 1])), shape=(2, 6)), sps.csr_matrix(([1.0, 1.0, 1.0], ([0, 1, 2], [3, 4, 5])), shape=(3, 6))
    for kw, what in ((dict(k=0), "k must be"), (dict(k=2.5), "k must be"), (dict(k=9, pool=8), "k must be"), (dict(k=129), "k must be"),
                     (dict(k=1, pool=0), "pool must be"), (dict(k=1, pool=129), "pool must be"), (dict(k=1, pool=2.0), "pool must be"),
                     (dict(k=1, lam=-0.1), "lam must be"), (dict(k=1, lam=1.5), "lam must be"), (dict(k=1, lam=np.nan), "lam must be"),
                     (dict(k=1, lam=np.inf), "lam must be"), (dict(k=1, lam="1"), "lam must be"),
                     (dict(k=1, exclude=sps.identity(5, format="csr")), "exclude must have shape")):
        with pytest.raises(ValueError, match=what):
            est.predict_topk_diverse(Xq, Xc, **kw)
    for bad in ((0, 0.5, 8), (9, 0.5, 8), (1, 0.5, 129), (1, np.nan, 8), (1, 1.5, 8)):  # (the binding's own checks, before the device is looked for)
        with pytest.raises(ValueError, match="must be"):
            est.predictor_.predict_topk_diverse(Xq, Xc, *bad)
    with pytest.raises(ValueError, match="share column"):
        est.predict_topk_diverse(Xq, Xq, k=1)
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.predict_topk_diverse(Xq, Xc, k=2)


def test_exports_and_intra_list_similarity():
    import myfm_amd
    from myfm_amd import _capi
    from myfm_amd.utils.ranking import intra_list_similarity

    L = _capi.lib()
    for name in ("mfm_pairs_topk_diverse", "mfm_pairs_topk_diverse_store"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert myfm_amd.DiverseRanking._fields == ("indices", "value", "objective", "redundancy") and "DiverseRanking" in myfm_amd.__all__
    assert _capi.diverse_pool(10) == dr.default_pool(10) == 40
    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_topk_diverse")
    for cls in (myfm_amd.MyFMGibbsRegressor, myfm_amd.MyFMGibbsClassifier, myfm_amd.MyFMOrderedProbit):
        assert hasattr(cls, "predict_topk_diverse")
    sim = np.array([[1.0, 0.5, 0.1], [0.5, 1.0, 0.3], [0.1, 0.3, 1.0]])
    idx = np.array([[0, 1, 2], [2, 0, -1], [1, -1, -1]])
    got = intra_list_similarity(myfm_amd.DiverseRanking(idx, None, None, None), sim)
    assert np.allclose(got[:2], [(0.5 + 0.1 + 0.3) / 3, 0.1]) and np.isnan(got[2])
    assert np.allclose(intra_list_similarity(idx, sim)[:2], got[:2])
