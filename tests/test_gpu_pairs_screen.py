"""The screened top-k on the device: the same list as topk, bit for bit and certified, on exact data whose values
are spread wider than the bf16 path's bound; clustered values, which must fall back; the bound itself against longdouble; and the
estimator boundary."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import datasets as ds
from tests import pairs_ref as pr

pytestmark = pytest.mark.gpu

HALVES = [1.0, -1.0, 2.0, -2.0, 0.5]
DQ, DC = 9, 11
BLK = DQ + DC  # the three columns that neither side's main matrix stores: a relation block's


def k_short(k):
    return min(256, max(64, 2 * k))


def spread_case(rng, U, I, K, S, spacing=64.0):
    """exact data (small integers and halves: every sum is exact in fp64, so pr.pair_scores is the longdouble result) whose
    candidates carry an identity column with the linear weight -spacing * (a permutation): consecutive values lie further apart
    than the interaction terms move them"""
    Xq, Xc, D0 = pr.disjoint_sides(rng, U, I, DQ, DC, HALVES, mean_nnz=2.0, empty_every=5)
    D = D0 + I
    Xq = sps.csr_matrix((Xq.data, Xq.indices, Xq.indptr), shape=(U, D))
    Xc = sps.csr_matrix((Xc.data, Xc.indices, Xc.indptr), shape=(I, D))
    Xc = sps.csr_matrix(Xc + sps.csr_matrix((np.ones(I), (np.arange(I), D0 + np.arange(I))), shape=(I, D)))
    samples = pr.exact_samples(rng, D, K, S)
    order = rng.permutation(I)
    for _, w, _ in samples:
        w[D0:] = -spacing * order
    return Xq, Xc, D, samples


def exclusions(rng, U, I):
    """a tenth of the pairs, and the last of several rows keeps three candidates: fewer than k are left"""
    ex = sps.random(U, I, density=0.1, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="lil")
    if U > 1:
        ex[U - 1, :] = 1.0
        ex[U - 1, rng.choice(I, size=min(3, I), replace=False)] = 0.0
    ex = sps.csr_matrix(ex)
    ex.eliminate_zeros()
    return ex


def check_same_list(P, src, ref, ex, E, ks_of=k_short):
    """topk_screened == topk == the reference's ranking for k = 1, 10, 33, 128 (k_s = 64, 64, 66, 256: the three tile shapes, and a
    shortlist that ends inside a rescoring group of 16), every row certified; before that, from the reference: the k-th value
    clears the k_s-th (t_u is bounded by it; the k_s + 1-th is further away still) by more than 2 E_u"""
    topk, screened = (P.topk_store, P.topk_screened_store) if hasattr(src, "push") else (P.topk, P.topk_screened)
    for k in (1, 10, 33, 128):
        ks = ks_of(k)
        ridx, rval = pr.topk(ref, ks, ex)
        full = ridx[:, ks - 1] >= 0
        assert np.all(rval[full, k - 1] - rval[full, ks - 1] > 2 * E[full]), k
        idx, val, cert = screened(src, k)
        tidx, tval = topk(src, k)
        assert np.array_equal(idx, tidx) and np.array_equal(val, tval), k
        assert np.array_equal(idx, ridx[:, :k]) and np.array_equal(val, rval[:, :k]), k
        assert cert.dtype == bool and cert.all(), (k, np.flatnonzero(~cert))


# ---- 1. the same list ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,S", [(0, 2), (1, 1), (5, 3), (33, 2)])
@pytest.mark.parametrize("I", [1, 63, 257, 300])
@pytest.mark.parametrize("U", [1, 65])
def test_same_list_certified(U, I, K, S):
    """every tile shape (k_s = 64, 64, 66, 256), KS padding, L = S KS off the multiples of 32, one and several stripes, I below and above
    k_s; host samples and, for the odd I, the device store"""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S)
    Xq, Xc, D, samples = spread_case(rng, U, I, K, S)
    ex = exclusions(rng, U, I)
    ref = pr.pair_scores(samples, Xq, Xc, 0)
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    src, stored = samples, I % 2 == 1 and K > 0
    if stored:
        src = _capi.Store(D, K)
        for s in samples:
            src.push(*s)
    E = (P.screen_scores_store(src) if stored else P.screen_scores(src))[1]
    check_same_list(P, src, ref, ex, E)
    P.close()


@pytest.mark.parametrize("side", [0, 1])
def test_same_list_with_a_relation_block(side):
    """a block of 4 rows x 3 columns on the query side or on the candidate side: the packed operands come from the gathered embedding"""
    from myfm_amd import _capi

    rng = np.random.default_rng(50 + side)
    U, I, K, S = 65, 300, 5, 3
    Xq, Xc, D, samples = spread_case(rng, U, I, K, S)
    B = sps.csr_matrix(rng.choice(HALVES + [0.0], size=(4, 3)))
    o2b = rng.integers(0, 4, size=(U, I)[side])
    gathered = sps.csr_matrix(sps.hstack([sps.csr_matrix((o2b.size, BLK)), B[o2b], sps.csr_matrix((o2b.size, D - BLK - 3))]))
    full = [Xq, Xc]
    full[side] = sps.csr_matrix(full[side] + gathered)
    ref = pr.pair_scores(samples, full[0], full[1], 0)
    ex = exclusions(rng, U, I)
    rel = {("rel_query", "rel_cand")[side]: [(BLK, o2b, B)]}
    P = _capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=1, **rel)  # (one 64-row tile per chunk: two chunks)
    check_same_list(P, samples, ref, ex, P.screen_scores(samples)[1])
    P.close()


# ---- 2. clustered values -----------------------------------------------------------------------------------------------------------
def clustered_case(U, I, K, S):
    """one-hot candidates with one linear weight and factor rows that differ by 1e-8, the upper half exact copies of the lower:
    every value of a row within 1e-6 of every other, the differences all in the contraction, far below what bf16 separates"""
    rng = np.random.default_rng(3)
    Xq, _, D0 = pr.disjoint_sides(rng, U, I, DQ, I, HALVES, mean_nnz=2.0, empty_every=0)
    Xc = sps.csr_matrix((np.ones(I), (np.arange(I), DQ + np.arange(I))), shape=(I, D0))
    samples = pr.normal_samples(rng, D0, K, S)
    for _, w, V in samples:
        noise = rng.normal(size=(I // 2, K))
        w[DQ:DQ + I] = 0.25
        V[DQ:DQ + I] = rng.normal(size=K) + 1e-8 * np.concatenate([noise, noise[: I - I // 2]])
    return Xq, Xc, samples


def test_clustered_values_fall_back():
    from myfm_amd import _capi

    U, I, K, S = 17, 300, 8, 3
    Xq, Xc, samples = clustered_case(U, I, K, S)
    ref = pr.pair_scores(samples, Xq, Xc, 0)
    assert np.all(ref.max(axis=1) - ref.min(axis=1) < 1e-6)
    P = _capi.Pairs(Xq, Xc)
    for k in (10, 128):
        idx, val, cert = P.topk_screened(samples, k)
        tidx, tval = P.topk(samples, k)
        assert np.array_equal(idx[cert], tidx[cert]) and np.array_equal(val[cert], tval[cert]), k
        assert not cert.all(), k
        assert np.abs(np.take_along_axis(ref, tidx, 1) - tval).max() < 1e-12
        # the duplicates tie exactly on the device too: the lower index first
        pos = {int(i): j for j, i in enumerate(tidx[0])}
        for i in range(I // 2):
            if i in pos and i + I // 2 in pos:
                assert pos[i] < pos[i + I // 2] and tval[0, pos[i]] == tval[0, pos[i + I // 2]]
    P.close()


# ---- 3. the bound ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,S", [(32, 1), (32, 128)])
def test_the_bound_holds(K, S):
    """all-positive operands (nothing cancels), L = 32 and L = 4096: |r~ - r| <= S E_u against longdouble, element by element. The
    kernel's E_u takes bf16's unit roundoff as 2^-8; half of it is (to first order) the figure with 2^-9, asserted as well. The
    printed ratios are DESIGN 4.13.5's: the whole error over the bound, and the accumulation's share -- r~ against the longdouble
    product of the operands as bf16 holds them -- per n 2^-24 sum |p q|, the constant c_acc stands for."""
    from myfm_amd import _capi

    rng = np.random.default_rng(K + S)
    U, I = 16, 64
    D = U + I
    Xq = sps.csr_matrix((np.ones(U), (np.arange(U), np.arange(U))), shape=(U, D))
    Xc = sps.csr_matrix((np.ones(I), (np.arange(I), U + np.arange(I))), shape=(I, D))
    samples = [(0.0, rng.uniform(0, 1, size=D), rng.uniform(0.25, 1.0, size=(D, K))) for _ in range(S)]
    P = _capi.Pairs(Xq, Xc)
    r, E = P.screen_scores(samples)
    P.close()
    ld = np.longdouble
    Pm = np.concatenate([V[:U] for _, _, V in samples], axis=1).astype(ld)   # one-hot sides: the embeddings are V's rows
    Qm = np.concatenate([V[U:] for _, _, V in samples], axis=1).astype(ld)
    bsum = sum(w[U:].astype(ld) for _, w, _ in samples)  # (a one-hot row's bias is its linear weight: sum P^2 equals sum V^2 x^2)
    exact = bsum[None, :] + Pm @ Qm.T
    err = np.abs(r.astype(ld) - exact)
    print("L %d: max |r~ - r| / (S E_u) = %.4g" % (K * S, float((err / (S * E[:, None])).max())))

    def bf16(x):  # round to nearest even at 8 significand bits
        m, e = np.frexp(x.astype(np.float64))
        return np.ldexp(np.rint(m * 256.0) / 256.0, e).astype(ld)

    at_bf16 = bsum[None, :] + bf16(Pm) @ bf16(Qm).T
    n = -(-K * S // 32) * 32
    acc = np.abs(r.astype(ld) - at_bf16) / (n * ld(2.0) ** -24 * (bf16(Pm) @ bf16(Qm).T))
    print("L %d: accumulation error / (n 2^-24 sum |p q|) = %.4g" % (K * S, float(acc.max())))
    assert np.all(err <= S * E[:, None])
    assert np.all(err <= 0.5 * S * E[:, None])


# ---- 4. the estimator boundary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gibbs", "variational"])
def test_estimator_boundary(kind):
    """predict_topk_screened equals predict_topk, tails and all, from the device store and after a pickle round trip (host samples);
    on the clustered model some rows are answered by the fallback and the result is still predict_topk's"""
    import myfm_amd

    n_users, n_items = 45, 70
    X, y, shapes = ds.onehot_mf(2500, n_users, n_items, rank_true=4, seed=2)
    D = n_users + n_items
    Xq = sps.csr_matrix((np.ones(n_users), (np.arange(n_users), np.arange(n_users))), shape=(n_users, D))
    Xc = sps.csr_matrix((np.ones(n_items), (np.arange(n_items), n_users + np.arange(n_items))), shape=(n_items, D))
    X = sps.csr_matrix(X)
    X.sort_indices()
    seen = sps.csr_matrix((np.ones(X.shape[0]), (X.indices[0::2], X.indices[1::2] - n_users)), shape=(n_users, n_items))
    if kind == "gibbs":
        est = myfm_amd.MyFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=30, n_kept_samples=10, group_shapes=shapes)
    else:
        est = myfm_amd.VariationalFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=30, group_shapes=shapes)
    for e in (est, pickle.loads(pickle.dumps(est))):
        for k, ex in ((10, seen), (128, None)):
            got = e.predict_topk_screened(Xq, Xc, k, exclude=ex)
            idx, val = e.predict_topk(Xq, Xc, k, exclude=ex)
            assert np.array_equal(got.indices, idx) and np.array_equal(got.value, val), (kind, k)
            assert got.certified.dtype == bool and got.certified.shape == (n_users,)
    if kind == "gibbs":
        from myfm_amd import _myfm

        Xq, Xc, samples = clustered_case(17, 300, 8, 3)
        fms = []
        for w0, w, V in samples:
            fm = _myfm.FM.__new__(_myfm.FM)
            fm.__setstate__((w0, w, V, []))
            fms.append(fm)
        p = _myfm.Predictor.__new__(_myfm.Predictor)
        p.__setstate__((8, Xq.shape[1], int(_myfm.TaskType.REGRESSION), fms))
        clustered = myfm_amd.MyFMRegressor(8)
        clustered.predictor_ = p
        got = clustered.predict_topk_screened(Xq, Xc, 10)
        idx, val = clustered.predict_topk(Xq, Xc, 10)
        assert np.array_equal(got.indices, idx) and np.array_equal(got.value, val)
        assert not got.certified.all()
