"""Query x candidate scoring with relation-block sides and the ordered-probit mode on the device: the block tables
and their gather with exact data, real-valued data in modes 0, 1 and 2 against the direct pair rows of the expanded sides, the
chunking of the queries (o2b keeps its absolute index), calls without blocks, the estimator boundary against predict() on the
materialised pair rows with relation blocks, and the errors of the new C entry points."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import datasets as ds
from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests.test_gpu_pairs import N_ITEMS, N_USERS, check_topk, mode_bound

pytestmark = pytest.mark.gpu

HALVES = rr.HALVES


def pairs_of(sd, **kw):
    from myfm_amd import _capi

    Xq, Xc, rq, rc = rr.capi_args(sd)
    return _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, **kw)


def mode2_bound(samples, Fq, Fc, n_cut):
    """n_cut values of Phi summed, each 0.4-Lipschitz in the score (bound b of mode 0) and rounded itself (1e-14)"""
    return n_cut * (0.4 * mode_bound(samples, Fq, Fc, 0) + 1e-14)


# ---- 3. exact layout with blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [(1, 0), (0, 1), (2, 2)])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [0, 1, 4, 33])
@pytest.mark.parametrize("I", [5, 250])
@pytest.mark.parametrize("U", [1, 17, 37])
def test_exact_layout_with_blocks(U, I, K, S, nb):
    """small integers and halves: every sum is exact, so tables, gather and contraction equal the direct reference on the expanded
    sides bit for bit whatever the association. (2, 2) has the one-row block on both sides and None entries; (1, 0) / (0, 1)
    leave the other side without blocks, so it takes the plain embedding kernel."""
    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S + 100000 * nb[0] + 200000 * nb[1])
    sd = rr.block_sides(rng, U, I, 9, 11, nb[0], nb[1], mean_nnz=2.0, empty_every=5, with_none=False)
    samples = pr.exact_samples(rng, sd["D"], K, S)
    Fq, Fc = rr.flat_sides(sd)
    ref = pr.pair_scores(samples, Fq, Fc, 0)
    P = pairs_of(sd)
    got = P.scores(samples, mode=0)
    assert got.shape == (U, I)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    for k in (10, 256):
        idx, val = P.topk(samples, k, mode=0)
        ridx, rval = pr.topk(ref, k)
        assert np.array_equal(idx, ridx) and np.array_equal(val, rval), k
    P.close()


# ---- 4. real values, modes 0, 1 and 2 --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_sides():
    """U = 37, I = 1000, two blocks per side, exclusions: the sides and their expansion, made once"""
    rng = np.random.default_rng(41)
    sd = rr.block_sides(rng, 37, 1000, 40, 60, 2, 2, mean_nnz=3.0)
    ex = sps.random(37, 1000, density=0.05, random_state=np.random.RandomState(3), format="csr")
    return sd, rr.flat_sides(sd), ex


@pytest.mark.parametrize("mode,n_cut", [(0, 0), (1, 0), (2, 1), (2, 4)])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued_with_blocks(K, S, mode, n_cut, real_sides):
    sd, (Fq, Fc), ex = real_sides
    rng = np.random.default_rng(31 + K + S + n_cut)
    samples = pr.normal_samples(rng, sd["D"], K, S, scale=0.3)
    cuts = rr.sorted_cuts(rng, S, n_cut) if mode == 2 else None
    ref = rr.pair_scores_mode(samples, Fq, Fc, mode, cuts)
    bound = mode2_bound(samples, Fq, Fc, n_cut) if mode == 2 else mode_bound(samples, Fq, Fc, mode)
    P = pairs_of(sd, exclude=ex, cutpoints=cuts)
    got = P.scores(samples, mode=mode)
    err = np.abs(got - ref)
    print("K %d S %d mode %d n_cut %d: max |device - ref| / bound = %.3g" % (K, S, mode, n_cut, (err / bound).max()))
    assert np.all(err <= bound)
    for k in (10, 100, 256):
        idx, val = P.topk(samples, k, mode=mode)
        check_topk(idx, val, ref, bound, k, ex)
    P.close()


@pytest.mark.parametrize("n_cut", [1, 4])
def test_mode2_without_blocks(n_cut):
    from myfm_amd import _capi

    rng = np.random.default_rng(57 + n_cut)
    U, I, K, S = 37, 1000, 8, 5
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    cuts = rr.sorted_cuts(rng, S, n_cut)
    ref = rr.pair_scores_mode(samples, Xq, Xc, 2, cuts)
    bound = mode2_bound(samples, Xq, Xc, n_cut)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    P = _capi.Pairs(Xq, Xc, exclude=ex, cutpoints=cuts)
    got = P.scores(samples, mode=2)
    assert np.all(np.abs(got - ref) <= bound)
    assert got.min() >= 0.0 and got.max() <= n_cut
    for k in (10, 100, 256):
        check_topk(*P.topk(samples, k, mode=2), ref, bound, k, ex)
    P.close()


# ---- 5. chunks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
def test_query_chunks_with_blocks_give_identical_output(mode):
    """scratch_bound=1 leaves one 64-row tile per chunk: 150 queries take three chunks. The query side's tables are built once
    and o2b is read at the absolute row, so the second and third chunk gather what the single chunk gathers."""
    rng = np.random.default_rng(9)
    U, I, K, S = 150, 300, 8, 3
    sd = rr.block_sides(rng, U, I, 30, 50, 1, 1, mean_nnz=3.0)
    # (the generated o2b repeats its values everywhere; make the chunks differ so that a re-based index cannot pass)
    o2b = sd["bq"][0][0]
    assert not np.array_equal(o2b[:64], o2b[64:128]) and not np.array_equal(o2b[:22], o2b[128:150])
    samples = pr.normal_samples(rng, sd["D"], K, S)
    cuts = rr.sorted_cuts(rng, S, 4) if mode == 2 else None
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    one, many = pairs_of(sd, exclude=ex, cutpoints=cuts), pairs_of(sd, exclude=ex, cutpoints=cuts, scratch_bound=1)
    assert np.array_equal(one.scores(samples, mode), many.scores(samples, mode))
    for k in (10, 256):
        a, b = one.topk(samples, k, mode), many.topk(samples, k, mode)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    Fq, Fc = rr.flat_sides(sd)
    ref = rr.pair_scores_mode(samples, Fq, Fc, mode, cuts)
    bound = mode2_bound(samples, Fq, Fc, 4) if mode == 2 else mode_bound(samples, Fq, Fc, 0)
    assert np.all(np.abs(many.scores(samples, mode) - ref) <= bound)
    check_topk(*many.topk(samples, 10, mode), ref, bound, 10, ex)
    one.close()
    many.close()


# ---- 6. calls without blocks ---------------------------------------------------------------------------------------------------
def test_block_call_against_expanded_call():
    """Pairs(expand(...)) has no blocks and takes the plain embedding kernel. Exact data: the block call equals it bit for bit.
    Real data: the two associate the sums differently, so they agree within the bound (both also with the reference)."""
    from myfm_amd import _capi

    rng = np.random.default_rng(23)
    sd = rr.block_sides(rng, 37, 250, 9, 11, 2, 2, mean_nnz=2.0)
    Fq, Fc = rr.flat_sides(sd)
    blocked, flat = pairs_of(sd), _capi.Pairs(Fq, Fc)
    exact = pr.exact_samples(rng, sd["D"], 4, 3)
    a, b = blocked.scores(exact, 0), flat.scores(exact, 0)
    assert np.array_equal(a, b) and np.array_equal(b, pr.pair_scores(exact, Fq, Fc, 0))
    ta, tb = blocked.topk(exact, 10, 0), flat.topk(exact, 10, 0)
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    for mode in (0, 1):
        samples = pr.normal_samples(rng, sd["D"], 8, 5, scale=0.3)
        bound = mode_bound(samples, Fq, Fc, mode)
        a, b = blocked.scores(samples, mode), flat.scores(samples, mode)
        ref = pr.pair_scores(samples, Fq, Fc, mode)
        assert np.all(np.abs(a - b) <= bound) and np.all(np.abs(a - ref) <= bound) and np.all(np.abs(b - ref) <= bound)
    blocked.close()
    flat.close()


# ---- 7. the estimator boundary ----------------------------------------------------------------------------------------------------
N_SIDE = 5  # multi-hot side columns behind each identity


@pytest.fixture(scope="module")
def rel_table():
    """the 45 x 70 table of test_gpu_pairs.py as a relation-block design: user block = identity + 5 multi-hot side columns, item
    block likewise; everything the checks need, made once"""
    X, y, _ = ds.onehot_mf(2500, N_USERS, N_ITEMS, rank_true=4, seed=2)
    X = sps.csr_matrix(X)
    X.sort_indices()
    u_row, i_row = X.indices[0::2].astype(np.int64), X.indices[1::2].astype(np.int64) - N_USERS
    rng = np.random.default_rng(12)

    def block(n):
        side = sps.random(n, N_SIDE, density=0.4, random_state=np.random.RandomState(n), format="csr")
        side.data[:] = rng.choice(HALVES, size=side.nnz)
        return sps.hstack([sps.identity(n, format="csr"), side], format="csr")

    UB, IB = block(N_USERS), block(N_ITEMS)
    u, i = np.repeat(np.arange(N_USERS), N_ITEMS), np.tile(np.arange(N_ITEMS), N_USERS)
    seen = sps.csr_matrix((np.ones(u_row.size), (u_row, i_row)), shape=(N_USERS, N_ITEMS))
    seen.sum_duplicates()
    edges = np.quantile(y, [0.2, 0.4, 0.6, 0.8])
    y5 = np.searchsorted(edges, y, side="right").astype(np.int64)  # 5 classes
    return dict(y=y, y5=y5, UB=UB, IB=IB, u_row=u_row, i_row=i_row, u=u, i=i, seen=seen)


def _rel_fit(kind, t, bias):
    import myfm_amd

    N = t["y"].size
    RB = myfm_amd.RelationBlock
    X = sps.csr_matrix(np.ones((N, 1))) if bias else sps.csr_matrix((N, 0))
    rels = [RB(t["u_row"], t["UB"]), RB(t["i_row"], t["IB"])]
    shapes = ([1] if bias else []) + [t["UB"].shape[1], t["IB"].shape[1]]
    if kind == "regressor":
        return myfm_amd.MyFMRegressor(rank=8, random_seed=3).fit(X, t["y"], X_rel=rels, n_iter=30, n_kept_samples=10, group_shapes=shapes)
    if kind == "classifier":
        return myfm_amd.MyFMClassifier(rank=8, random_seed=3).fit(X, t["y"] > np.median(t["y"]), X_rel=rels, n_iter=30,
                                                                 n_kept_samples=10, group_shapes=shapes)
    if kind == "variational":
        return myfm_amd.VariationalFMRegressor(rank=8, random_seed=3).fit(X, t["y"], X_rel=rels, n_iter=30, group_shapes=shapes)
    return myfm_amd.MyFMOrderedProbit(rank=8, random_seed=3).fit(X, t["y5"], X_rel=rels, n_iter=30, n_kept_samples=10,
                                                                 group_shapes=shapes)


def _samples_of(kind, est):
    if kind == "variational":
        return [(est.w0_mean, np.asarray(est.w_mean), np.asarray(est.V_mean))]
    return [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in est.predictor_.samples]


def _rel_boundary_checks(kind, est, t, bias):
    import myfm_amd

    RB = myfm_amd.RelationBlock
    m = 1 if bias else 0
    Xq = sps.csr_matrix(np.ones((N_USERS, 1))) if bias else sps.csr_matrix((N_USERS, 0))  # the bias-like column: the query side's
    Xc = sps.csr_matrix((N_ITEMS, m))
    rq = [RB(np.arange(N_USERS), t["UB"]), None]
    rc = [None, RB(np.arange(N_ITEMS), t["IB"])]
    got = est.predict_pairs(Xq, Xc, X_rel_query=rq, X_rel_cand=rc)
    idx, val = est.predict_topk(Xq, Xc, 10, exclude=t["seen"], X_rel_query=rq, X_rel_cand=rc)
    # the independent path: the U * I pair rows through the estimator's own prediction with relation blocks
    Xp = sps.csr_matrix(np.ones((t["u"].size, 1))) if bias else sps.csr_matrix((t["u"].size, 0))
    rp = [RB(t["u"], t["UB"]), RB(t["i"], t["IB"])]
    Fq = rr.expand(Xq, [(np.arange(N_USERS), t["UB"]), None], [t["UB"].shape[1], t["IB"].shape[1]])
    Fc = rr.expand(Xc, [None, (np.arange(N_ITEMS), t["IB"])], [t["UB"].shape[1], t["IB"].shape[1]])
    samples = _samples_of(kind, est)
    if kind == "ordered":
        direct = est.predict_proba(Xp, rp) @ np.arange(5)
        bound = mode2_bound(samples, Fq, Fc, 4)
    elif kind == "classifier":
        direct, bound = est.predict_proba(Xp, rp), mode_bound(samples, Fq, Fc, 1)
    else:
        direct, bound = est.predict(Xp, rp), mode_bound(samples, Fq, Fc, 0)
    ref = np.asarray(direct, dtype=np.float64).reshape(N_USERS, N_ITEMS)
    assert got.shape == ref.shape and np.all(np.abs(got - ref) <= bound), (np.abs(got - ref) / bound).max()
    assert np.ptp(ref) > 1e-3
    check_topk(idx, val, ref, bound, 10, t["seen"])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("kind", ["regressor", "classifier", "variational", "ordered"])
def test_estimator_boundary_with_blocks(kind, bias, rel_table):
    """predict_pairs with X_rel_query=[ub, None], X_rel_cand=[None, ib] equals predict / predict_proba (ordered probit:
    predict_proba @ arange(5)) on the materialised pair rows given as relation blocks of U * I rows; predict_topk with the
    training pairs excluded passes the top-k check -- from the device store, and after a pickle round trip from host samples"""
    est = _rel_fit(kind, rel_table, bias)
    _rel_boundary_checks(kind, est, rel_table, bias)
    _rel_boundary_checks(kind, pickle.loads(pickle.dumps(est)), rel_table, bias)


def test_ordered_probit_on_the_onehot_table():
    """MyFMOrderedProbit without blocks: both sides in the full feature space"""
    import myfm_amd

    X, y, shapes = ds.onehot_mf(2500, N_USERS, N_ITEMS, rank_true=4, seed=2)
    D = N_USERS + N_ITEMS
    y5 = np.searchsorted(np.quantile(y, [0.2, 0.4, 0.6, 0.8]), y, side="right").astype(np.int64)
    est = myfm_amd.MyFMOrderedProbit(rank=8, random_seed=3).fit(X, y5, n_iter=30, n_kept_samples=10, group_shapes=shapes)
    Xq = sps.csr_matrix((np.ones(N_USERS), (np.arange(N_USERS), np.arange(N_USERS))), shape=(N_USERS, D))
    Xc = sps.csr_matrix((np.ones(N_ITEMS), (np.arange(N_ITEMS), N_USERS + np.arange(N_ITEMS))), shape=(N_ITEMS, D))
    u, i = np.repeat(np.arange(N_USERS), N_ITEMS), np.tile(np.arange(N_ITEMS), N_USERS)
    Xpairs = sps.csr_matrix((np.ones(2 * u.size), (np.repeat(np.arange(u.size), 2), np.stack([u, N_USERS + i], 1).ravel())),
                            shape=(u.size, D))
    for e in (est, pickle.loads(pickle.dumps(est))):
        ref = (e.predict_proba(Xpairs) @ np.arange(5)).reshape(N_USERS, N_ITEMS)
        bound = mode2_bound(_samples_of("ordered", e), Xq, Xc, 4)
        got = e.predict_pairs(Xq, Xc)
        assert np.all(np.abs(got - ref) <= bound), (np.abs(got - ref) / bound).max()
        check_topk(*e.predict_topk(Xq, Xc, 10), ref, bound, 10)


# ---- 8. errors of the C entry points -----------------------------------------------------------------------------------------------
def test_capi_errors():
    from myfm_amd import _capi

    rng = np.random.default_rng(2)
    D = 20
    Xq = sps.csr_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, D))
    Xc = sps.csr_matrix((np.ones(4), ([0, 1, 2, 3], [5, 6, 7, 8])), shape=(4, D))
    B = sps.csr_matrix(np.array([[1.0, 0, 2.0], [0, 0.5, 0]]))
    good = (10, [1, 0, 1], B)
    with pytest.raises(ValueError, match=r"X_rel_query\[0\]: row 1 maps to block row 2, the block has 2"):
        _capi.Pairs(Xq, Xc, rel_query=[(10, [1, 2, 1], B)])
    with pytest.raises(ValueError, match=r"X_rel_cand\[0\]: row 3 maps to block row -1"):
        _capi.Pairs(Xq, Xc, rel_cand=[(10, [1, 0, 1, -1], B)])
    with pytest.raises(ValueError, match=r"X_rel_query\[1\]: columns \[18, 18 \+ 3\) exceed the feature size 20"):
        _capi.Pairs(Xq, Xc, rel_query=[good, (18, [1, 0, 1], B)])
    # an overlapping column: with the other side's main matrix, with the other side's earlier block (a row nothing points at)
    with pytest.raises(ValueError, match="X_query and X_cand share column 7$"):
        _capi.Pairs(Xq, Xc, rel_query=[(7, [1, 1, 1], sps.csr_matrix(np.array([[1.0, 0, 0], [0, 0, 0]])))])
    with pytest.raises(ValueError, match="X_query and X_cand share column 12$"):
        _capi.Pairs(Xq, Xc, rel_query=[good], rel_cand=[(12, [1, 1, 1, 1], B)])
    with pytest.raises(ValueError, match="o2b must have one entry per row"):
        _capi.Pairs(Xq, Xc, rel_query=[(10, [1, 0], B)])
    samples = pr.normal_samples(rng, D, 4, 3)
    P = _capi.Pairs(Xq, Xc, rel_query=[good])
    with pytest.raises(ValueError, match="mode 2 needs the samples' cutpoints"):
        P.scores(samples, mode=2)
    with pytest.raises(ValueError, match="bad prediction mode .*2: mean expected class index"):
        P.scores(samples, mode=3)
    P.close()
    P = _capi.Pairs(Xq, Xc, rel_query=[good], cutpoints=rr.sorted_cuts(rng, 2, 3))
    with pytest.raises(ValueError, match="cutpoints were set for 2 samples, the call has 3"):
        P.topk(samples, 2, mode=2)
    assert P.scores(samples[:2], mode=2).shape == (3, 4)  # ... and the right count passes
    P.close()
    with pytest.raises(ValueError, match="at least one sample and one cutpoint"):
        _capi.Pairs(Xq, Xc, cutpoints=np.zeros((3, 0)))
