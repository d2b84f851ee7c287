"""Query x candidate scoring on the device: the MFMA tile layout with exact data, real-valued data against the
direct pair-row reference, k and the exclusions, the estimator boundary against predict() on the materialised pair rows, and
the chunking of the queries."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import datasets as ds
from tests import pairs_ref as pr

pytestmark = pytest.mark.gpu

HALVES = [1.0, -1.0, 2.0, -2.0, 0.5]


def check_topk(idx, val, ref, bound, k, exclude=None):
    """the top-k properties that hold whatever near-ties do: a prefix of valid entries of the right length, values equal to the
    reference's at the returned indices within the bound and non-increasing, no index twice, none excluded, and every candidate
    left out no better than the row's last returned value + bound"""
    U, I = ref.shape
    assert idx.shape == (U, k) and val.shape == (U, k) and idx.dtype == np.int64
    E = None if exclude is None else sps.csr_matrix(exclude)
    for u in range(U):
        allowed = np.ones(I, dtype=bool)
        if E is not None:
            allowed[E.indices[E.indptr[u]:E.indptr[u + 1]]] = False
        n = min(k, int(allowed.sum()))
        ii = idx[u, :n]
        assert np.all(idx[u, n:] == -1) and np.all(val[u, n:] == -np.inf), u
        assert np.all((ii >= 0) & (ii < I)) and np.unique(ii).size == n and np.all(allowed[ii]), u
        assert np.all(np.abs(val[u, :n] - ref[u, ii]) <= bound[u, ii]), u
        assert np.all(np.diff(val[u, :n]) <= 0), u
        rest = allowed.copy()
        rest[ii] = False
        if rest.any():
            assert np.all(ref[u, rest] <= val[u, n - 1] + bound[u, rest]), u


def mode_bound(samples, Xq, Xc, mode):
    """n eps with n <= 1e4 terms is about 1e-12 of the sum of absolute terms; a factor 100 for the different association.
    Mode 1: times Phi's Lipschitz constant 0.4, plus 1e-14 for Phi's own rounding."""
    b = 1e-10 * pr.pair_scores_abs(samples, Xq, Xc)
    return b if mode == 0 else 0.4 * b + 1e-14


# ---- 1. exact layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
@pytest.mark.parametrize("I", [5, 16, 250])
@pytest.mark.parametrize("U", [1, 17, 37])
def test_exact_layout(U, I, K, S):
    """small integers and halves: every sum is exact in fp64, so the dense scores equal the reference bit for bit whatever the
    association -- a misplaced MFMA operand or result cannot hide. The values tie often, so the top-k (all three tile shapes:
    k <= 64, <= 128, <= 256) exercises the index order and must equal the reference's exactly."""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    samples = pr.exact_samples(rng, D, K, S)
    ref = pr.pair_scores(samples, Xq, Xc, 0)
    P = _capi.Pairs(Xq, Xc)
    got = P.scores(samples, mode=0)
    assert got.shape == (U, I)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    for k in (10, 100, 256):
        idx, val = P.topk(samples, k, mode=0)
        ridx, rval = pr.topk(ref, k)
        assert np.array_equal(idx, ridx) and np.array_equal(val, rval), k
    P.close()


# ---- 2. real values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued(K, S, mode):
    """normal samples, multi-hot sides with values +-1, +-2, 0.5 and empty rows; 1000 candidates span several stripes; S = 37
    is a long sample loop (mode 1 finishes a tile per sample)"""
    from myfm_amd import _capi

    rng = np.random.default_rng(31 + K + S)
    U, I = 37, 1000
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    ref = pr.pair_scores(samples, Xq, Xc, mode)
    bound = mode_bound(samples, Xq, Xc, mode)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    got = P.scores(samples, mode=mode)
    err = np.abs(got - ref)
    print("K %d S %d mode %d: max |device - ref| / bound = %.3g" % (K, S, mode, (err / bound).max()))
    assert np.all(err <= bound)
    for k in (10, 100, 256):
        idx, val = P.topk(samples, k, mode=mode)
        check_topk(idx, val, ref, bound, k, ex)
    P.close()


# ---- 3. k and exclude -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 256])
def test_k_and_exclude(k):
    from myfm_amd import _capi

    rng = np.random.default_rng(77)
    U, I, K, S = 20, 250, 8, 3
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0, empty_every=0)
    samples = pr.normal_samples(rng, D, K, S)
    ref = pr.pair_scores(samples, Xq, Xc, 0)
    bound = mode_bound(samples, Xq, Xc, 0)
    top10, _ = pr.topk(ref, 10)
    ex = sps.random(U, I, density=0.1, random_state=np.random.RandomState(5), format="lil")
    ex[0, :] = 1.0  # everything excluded
    ex[1, :] = 0.0  # nothing excluded
    ex[2, :] = 0.0
    ex[2, top10[2]] = 1.0  # exactly its top 10
    ex = sps.csr_matrix(ex)
    ex.eliminate_zeros()
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    idx, val = P.topk(samples, k, mode=0)
    check_topk(idx, val, ref, bound, k, ex)
    assert np.all(idx[0] == -1) and np.all(val[0] == -np.inf)
    n1 = min(k, I)
    assert np.all(idx[1, :n1] >= 0) and np.all(idx[1, n1:] == -1)  # (k = 256 > I = 250: the -1 / -inf tail)
    assert not np.intersect1d(idx[2], top10[2]).size
    # without exclusions
    P2 = _capi.Pairs(Xq, Xc)
    idx, val = P2.topk(samples, k, mode=0)
    check_topk(idx, val, ref, bound, k)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="k must be"):
            P2.topk(samples, bad)
    P.close()
    P2.close()


# ---- 4. the estimator boundary ---------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS = 45, 70


@pytest.fixture(scope="module")
def table():
    X, y, shapes = ds.onehot_mf(2500, N_USERS, N_ITEMS, rank_true=4, seed=2)
    D = N_USERS + N_ITEMS
    Xq = sps.csr_matrix((np.ones(N_USERS), (np.arange(N_USERS), np.arange(N_USERS))), shape=(N_USERS, D))
    Xc = sps.csr_matrix((np.ones(N_ITEMS), (np.arange(N_ITEMS), N_USERS + np.arange(N_ITEMS))), shape=(N_ITEMS, D))
    u, i = np.repeat(np.arange(N_USERS), N_ITEMS), np.tile(np.arange(N_ITEMS), N_USERS)
    Xpairs = sps.csr_matrix((np.ones(2 * u.size), (np.repeat(np.arange(u.size), 2), np.stack([u, N_USERS + i], 1).ravel())),
                            shape=(u.size, D))
    X = sps.csr_matrix(X)
    X.sort_indices()
    seen = sps.csr_matrix((np.ones(X.shape[0]), (X.indices[0::2], X.indices[1::2] - N_USERS)), shape=(N_USERS, N_ITEMS))
    seen.sum_duplicates()
    return X, y, shapes, Xq, Xc, Xpairs, seen


def _boundary_checks(est, mode, samples_of, table):
    X, y, shapes, Xq, Xc, Xpairs, seen = table
    got = est.predict_pairs(Xq, Xc)
    idx, val = est.predict_topk(Xq, Xc, 10, exclude=seen)
    direct = est.predict_proba(Xpairs) if mode == 1 else est.predict(Xpairs)
    ref = np.asarray(direct, dtype=np.float64).reshape(N_USERS, N_ITEMS)
    bound = mode_bound(samples_of(est), Xq, Xc, mode)
    assert got.shape == ref.shape and np.all(np.abs(got - ref) <= bound), np.abs(got - ref).max()
    check_topk(idx, val, ref, bound, 10, seen)


def _gibbs_samples(est):
    return [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in est.predictor_.samples]


def _vb_samples(est):
    return [(est.w0_mean, np.asarray(est.w_mean), np.asarray(est.V_mean))]


@pytest.mark.parametrize("kind", ["regressor", "classifier", "variational"])
def test_estimator_boundary(kind, table):
    """predict_pairs equals predict() on the materialised pair rows (the independent path), predict_topk with the training
    pairs excluded passes the top-k check against it -- from the device store, and after a pickle round trip from host samples"""
    import myfm_amd

    X, y, shapes = table[:3]
    if kind == "regressor":
        est = myfm_amd.MyFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=30, n_kept_samples=10, group_shapes=shapes)
        mode, samples_of = 0, _gibbs_samples
    elif kind == "classifier":
        est = myfm_amd.MyFMClassifier(rank=8, random_seed=3).fit(X, y > np.median(y), n_iter=30, n_kept_samples=10,
                                                                 group_shapes=shapes)
        mode, samples_of = 1, _gibbs_samples
    else:
        est = myfm_amd.VariationalFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=30, group_shapes=shapes)
        mode, samples_of = 0, _vb_samples
    _boundary_checks(est, mode, samples_of, table)
    _boundary_checks(pickle.loads(pickle.dumps(est)), mode, samples_of, table)


# ---- 5. splitting ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_query_chunks_give_identical_output(mode):
    """a scratch bound of one byte leaves one 64-row tile per chunk: 150 queries take three chunks, the default bound one; the
    value of a pair does not depend on its tile and the order is total, so the outputs are identical"""
    from myfm_amd import _capi

    rng = np.random.default_rng(9)
    U, I, K, S = 150, 300, 8, 3
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    one, many = _capi.Pairs(Xq, Xc, exclude=ex), _capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=1)
    assert np.array_equal(one.scores(samples, mode), many.scores(samples, mode))
    for k in (10, 256):
        a, b = one.topk(samples, k, mode), many.topk(samples, k, mode)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ref = pr.pair_scores(samples, Xq, Xc, mode)
    check_topk(*many.topk(samples, 10, mode), ref, mode_bound(samples, Xq, Xc, mode), 10, ex)
    one.close()
    many.close()


# ---- 6. stripes of several workgroup steps ---------------------------------------------------------------------------------------
# The host cuts the candidates into min(ceil(512 / query tiles), steps, 64) stripes, so a stripe is longer than one workgroup step
# (128 / 256 / 512 candidates for k <= 64 / 128 / 256) only with more than 64 steps or with many query tiles. That is the
# production shape: the threshold and the buffers are carried from step to step, the operand offsets move, and the last step is
# clipped inside the stripe.
def test_long_stripe_few_queries():
    """3 queries x 9000 candidates, k = 10: 71 steps on 64 stripes at the most, so stripes of 2 steps; exact data must give the
    reference's lists exactly, real-valued data pass the top-k check; with exclusions"""
    from myfm_amd import _capi

    rng = np.random.default_rng(611)
    U, I, K, S = 3, 9000, 8, 3
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 12, 40, HALVES, mean_nnz=3.0)
    ex = sps.random(U, I, density=0.02, random_state=np.random.RandomState(2), format="csr")
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    exact = pr.exact_samples(rng, D, K, S)
    ref = pr.pair_scores(exact, Xq, Xc, 0)
    assert np.array_equal(P.scores(exact, 0), ref)
    idx, val = P.topk(exact, 10, 0)
    ridx, rval = pr.topk(ref, 10, ex)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    for mode in (0, 1):
        samples = pr.normal_samples(rng, D, K, S, scale=0.3)
        ref = pr.pair_scores(samples, Xq, Xc, mode)
        bound = mode_bound(samples, Xq, Xc, mode)
        assert np.all(np.abs(P.scores(samples, mode) - ref) <= bound)
        check_topk(*P.topk(samples, 10, mode), ref, bound, 10, ex)
    P.close()


@pytest.fixture(scope="module")
def many_tiles():
    """2000 queries x 3000 candidates of exact data: 32 / 63 / 125 query tiles for the three tile shapes give 16 / 9 / 5 stripes
    of 24 / 12 / 6 steps, i.e. 2 steps per stripe (the last one clipped at candidate 3000); the reference, computed once"""
    rng = np.random.default_rng(612)
    U, I = 2000, 3000
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    samples = pr.exact_samples(rng, D, 4, 2)
    ref = np.vstack([pr.pair_scores(samples, Xq[a:a + 250], Xc, 0) for a in range(0, U, 250)])
    ex = sps.random(U, I, density=0.01, random_state=np.random.RandomState(4), format="csr")
    return Xq, Xc, samples, ref, ex


@pytest.mark.parametrize("k", [10, 100, 256])
def test_long_stripes_many_query_tiles(k, many_tiles):
    from myfm_amd import _capi

    Xq, Xc, samples, ref, ex = many_tiles
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    idx, val = P.topk(samples, k, 0)
    ridx, rval = pr.topk(ref, k, ex)
    assert np.array_equal(idx, ridx) and np.array_equal(val, rval)
    if k == 10:
        assert np.array_equal(P.scores(samples, 0), ref)
    P.close()
