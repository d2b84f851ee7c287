"""The diversified top-k on the device: k_div_pack and k_div_select behind mfm_pairs_topk_diverse against the
longdouble replay of tests/pairs_diverse_ref.py -- every step of the device's own list is judged given its earlier picks (no search,
nothing skipped; the tolerance is derived in that file). The pool must equal a separate topk call bit for bit in every case.

Largest used share of the tolerance over the real-valued cases, as printed by test_real_valued: see DESIGN 4.13.6."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_diverse_ref as dr
from tests import pairs_ref as pr
from tests import pairs_sim_ref as sr
from tests.test_gpu_pairs_sim import _block_sides, _fit, _one_hot, tiny_table, N_ITEMS, N_USERS  # noqa: F401

pytestmark = pytest.mark.gpu


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _check(P, samples, k, lam, pool, sim, b_sim=0.0, b_v=0.0, mode=0):
    """one call under the replay; lam = 1 must be topk(k), bit for bit"""
    got = P.topk_diverse(samples, k, lam, pool, mode)
    assert got[0].dtype == np.int64 and all(x.shape == (P.U, k) for x in got)
    used = dr.check_replay(got, P.topk(samples, pool, mode), sim, b_sim, b_v, lam)
    if lam == 1.0:
        assert _same(got[:2], P.topk(samples, k, mode))
    return got, used


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("K", [0, 1, 3, 33])
@pytest.mark.parametrize("pool", [1, 15, 16, 17, 33, 128])
def test_exact_layout(pool, K, S):
    """exact_unit_samples and unit sides: every norm is a power of two, the cosines and their mean over S <= 2 samples are exact, so
    the similarity's tolerance is 0 and only ROUND is left for the relevance's division. Partial tiles, an inner length that is no
    multiple of the staged chunk (K = 33, S = 1: 36 -> 40; K <= 3: 4 -> 8), K = 0 (every sim 0: topk's list), a pool larger than the
    candidate set (tail entries)."""
    from myfm_amd import _capi

    rng = np.random.default_rng(100 * pool + 10 * K + S)
    D = 20
    samples = sr.exact_unit_samples(rng, D, K, S)
    for I in sorted({pool - 3, pool, 250} - set(range(-3, 1))):
        Xq, Xc = sr.unit_sides(rng, 5, I, D, shared=False)
        sim = sr.moments(samples, Xc, Xc, "cosine")[0]
        for U in (1, 5):
            P = _capi.Pairs(Xq[:U], Xc)
            for k in sorted({1, pool}):
                for lam in (0.0, 0.5, 1.0):
                    got, _ = _check(P, samples, k, lam, pool, sim)
                    if K == 0:
                        assert _same(got[:2], P.topk(samples, k)) and np.all(got[3][got[0] >= 0] == 0.0)
                    assert np.all(got[0][:, min(I, k):] == -1) and np.all(got[0][:, :min(I, k)] >= 0)
            P.close()


@pytest.mark.parametrize("pool", [32, 128])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued(K, S, pool):
    """normal samples, multi-hot sides, 5 % of the pairs excluded; the input's conditioning is asserted on the reference alone"""
    from myfm_amd import _capi

    samples, Xq, Xc, ex = dr.real_case(K, S)
    dr.assert_spread(samples, Xq, Xc, ex, pool)
    sim, b_sim = dr.similarity(samples, Xc)
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    for lam in (0.3, 0.7):
        got, used = _check(P, samples, pool // 2, lam, pool, sim, b_sim, dr.value_bound(samples, Xq, Xc))
        print("K %d S %d pool %d lam %.1f: %.3g of the tolerance" % (K, S, pool, lam, used))
        assert not any(ex[u, i] for u in range(P.U) for i in got[0][u])
    P.close()


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_exact_ties(lam):
    """every candidate row twice, at i and i + I: twins tie exactly in value and in every Gram entry, so the lower index goes first at
    every step. The duplicate's similarity with its chosen twin is 1, the largest there is, so it directly follows its twin only when
    nothing better is live: every other unchosen pool entry is then itself the duplicate of a chosen one (late in a list that takes the
    whole pool). A property of these inputs for lam > 0, so it is asserted on the reference's own list too."""
    from myfm_amd import _capi

    samples, Xq, Xc, _ = dr.real_case(8, 5, I=100)
    I, X2, pool = Xc.shape[0], sps.vstack([Xc, Xc], format="csr"), 64
    sim, b_sim = dr.similarity(samples, X2)
    P = _capi.Pairs(Xq, X2)
    got, _ = _check(P, samples, pool, lam, pool, sim, b_sim, dr.value_bound(samples, Xq, X2))
    pidx, pval = P.topk(samples, pool)
    for idx in (got[0], np.stack([dr.greedy(pidx[u], pval[u], sim, lam, pool)[0] for u in range(P.U)])):
        for u in range(P.U):
            at = {int(i): t for t, i in enumerate(idx[u])}
            for i, t in at.items():
                if i >= I and i - I in at:
                    assert at[i - I] < t, (u, i)
                    if t - at[i - I] == 1:
                        assert all((int(j) + I) % (2 * I) in at and at[(int(j) + I) % (2 * I)] < t for j in idx[u, t + 1:]), (u, i, t)
    P.close()


def test_exclude_chunks_blocks_and_empty_rows():
    """exclusions down to fewer than k candidates; a forced 64-row chunk gives identical output; a relation-block candidate side
    against the same side expanded on the host; a candidate with an empty row (a zero embedding: its sim with everything is 0)"""
    from myfm_amd import _capi

    samples, Xq, Xc, _ = dr.real_case(8, 5, U=150, I=120)
    U, I, k, pool = 150, 120, 10, 32
    assert np.any(np.diff(Xc.indptr) == 0)
    ex = sps.lil_matrix((U, I))
    ex[0, :I - 3] = 1  # (query 0 keeps 3 candidates)
    ex[1, :] = 1       # (query 1 keeps none)
    ex = sps.csr_matrix(ex + sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr"))
    sim, b_sim = dr.similarity(samples, Xc)
    one, many = _capi.Pairs(Xq, Xc, exclude=ex), _capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=1)
    got, _ = _check(one, samples, k, 0.5, pool, sim, b_sim, dr.value_bound(samples, Xq, Xc))
    assert np.all(got[0][0, 3:] == -1) and np.all(got[0][0, :3] >= I - 3) and np.all(got[0][1] == -1) and np.all(np.isnan(got[2][1]))
    assert _same(got, many.topk_diverse(samples, k, 0.5, pool))
    one.close()
    many.close()
    rng = np.random.default_rng(23)
    Xq, Xc, rq, rc, Fq, Fc, D = _block_sides(rng, 37, 250, exact=False)
    Fq, rq = Fq[:, :23 + 6], [rq[0]]  # (the queries keep the user block alone: the sides of a scoring handle share no column)
    Fq = sps.hstack([Fq, sps.csr_matrix((37, D - Fq.shape[1]))], format="csr")
    samples = pr.normal_samples(rng, D, 8, 5, scale=0.3)
    sim, b_sim = dr.similarity(samples, Fc)
    for P in (_capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc), _capi.Pairs(Fq, Fc)):
        _check(P, samples, k, 0.5, pool, sim, b_sim, dr.value_bound(samples, Fq, Fc))
        P.close()


def test_refusals():
    from myfm_amd import _capi

    rng = np.random.default_rng(2)
    Xq, Xc, D = pr.disjoint_sides(rng, 5, 20, 9, 11, [1.0, 0.5])
    samples = pr.normal_samples(rng, D, 4, 2)
    P = _capi.Pairs(Xq, Xc)
    for k, pool, what in ((0, 8, "k must be"), (9, 8, "k must be"), (200, None, "k must be"), (1, 0, "pool must be"), (1, 129, "pool must be")):
        with pytest.raises(ValueError, match=what):
            P.topk_diverse(samples, k, 0.5, pool)
    for lam in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="lam must be"):
            P.topk_diverse(samples, 3, lam)
    P.close()
    S = _capi.Pairs(Xq, Xc, similarity=True)
    with pytest.raises(ValueError, match="similarity handle"):
        S.topk_diverse(samples, 3)
    S.close()


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_estimator_boundary(kind, tiny_table):  # noqa: F811
    """the three estimators on a tiny fitted table, after pickling, and the regressor after fold_in: the pool is predict_topk's bit for
    bit and the list passes the replay against the reference computed from the estimator's own samples"""
    X, y, shapes = tiny_table
    D = N_USERS + N_ITEMS
    est = _fit(kind, X, y, shapes)
    Xq, Xc = _one_hot(np.arange(7), D), _one_hot(N_USERS + np.arange(N_ITEMS), D)
    ests = [(est, Xq, Xc), (pickle.loads(pickle.dumps(est)), Xq, Xc)]
    if kind == "regressor":
        seen = np.asarray([0, 3, 5, 7, 1, 2, 4, 9])
        new = est.fold_in(_one_hot(N_USERS + seen, D), np.linspace(-1.0, 1.0, seen.size), np.repeat(np.arange(2), 4), 0)
        ests.append((new, _one_hot(D + np.arange(2), D + 2), _one_hot(N_USERS + np.arange(N_ITEMS), D + 2)))
    for e, xq, xc in ests:
        samples = [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in e.predictor_.samples]
        sim, b_sim = dr.similarity(samples, xc)
        r = e.predict_topk_diverse(xq, xc, k=5, lam=0.5, pool=16)
        assert type(r).__name__ == "DiverseRanking" and r.indices.dtype == np.int64
        # (test_gpu_pairs.mode_bound: Phi's Lipschitz constant 0.4 and its own rounding; the class index sums one Phi per cutpoint, 4 here)
        b_v = dr.value_bound(samples, xq, xc)
        b_v = {"regressor": b_v, "classifier": 0.4 * b_v + 1e-14, "ordered": 4 * (0.4 * b_v + 1e-14)}[kind]
        dr.check_replay(tuple(r), e.predict_topk(xq, xc, 16), sim, b_sim, b_v, 0.5)
        assert _same(tuple(e.predict_topk_diverse(xq, xc, k=5, lam=1.0))[:2], e.predict_topk(xq, xc, 5))
