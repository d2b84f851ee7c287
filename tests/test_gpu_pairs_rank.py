"""Ranks of given pairs among all candidates on the device, through _capi.Pairs and the estimators: values bit for bit
those of the dense scores, ranks exactly the brute-force count under the total order, whatever the chunking and the stripes."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import datasets as ds
from tests import pairs_rank_ref as kr
from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests.test_gpu_pairs import HALVES, mode_bound
from tests.test_gpu_pairs_rel import _rel_fit, mode2_bound, rel_table  # noqa: F401  (rel_table is a fixture)

pytestmark = pytest.mark.gpu

COUNTS = [5, 0, 64, 1]  # targets per row, by row index modulo 4 (clipped to the number of candidates)


def check_against_scores(rank, value, scores, targets, exclude):
    """value bit for bit the dense scores at the targets, rank exactly the brute-force count on those scores"""
    rrank, rvalue, _ = kr.rank_ref_fast(scores, targets, exclude)
    assert rank.dtype == np.int64 and rank.shape == rrank.shape and value.shape == rvalue.shape
    assert np.array_equal(value, rvalue), np.flatnonzero(value != rvalue)[:8]
    assert np.array_equal(rank, rrank), (np.flatnonzero(rank != rrank)[:8], rank[rank != rrank][:8], rrank[rank != rrank][:8])


# ---- 1. exact layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [0, 3, 33])
@pytest.mark.parametrize("I", [5, 129, 1000])
@pytest.mark.parametrize("U", [1, 17, 65])
def test_exact_layout(U, I, K, S):
    """small integers and halves: every sum is exact in fp64, so the values equal the NumPy reference bit for bit and tie often --
    a misplaced MFMA result, a dropped stripe or a lost count cannot hide, and the index order decides many comparisons. 0, 1, 5
    and 64 targets per row, columns 0 and I - 1 among them and (where the row has them) two targets of equal value; with and
    without 10 % of the other pairs excluded"""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    samples = pr.exact_samples(rng, D, K, S)
    ref = pr.pair_scores(samples, Xq, Xc, 0)
    targets = kr.draw_targets(rng, U, I, COUNTS, ties_from=ref)
    assert targets[:, 0].nnz and targets[:, I - 1].nnz
    if U >= 17 and I >= 129:
        tied = [np.unique(ref[u, targets[u].indices]).size < targets[u].nnz for u in range(U)]
        assert any(tied)
    exclude = kr.exclude_without(rng, U, I, 0.1, targets)
    for ex in (None, exclude):
        P = _capi.Pairs(Xq, Xc, exclude=ex, targets=targets)
        rank, value = P.rank(samples, mode=0)
        check_against_scores(rank, value, ref, targets, ex)
        P.close()


# ---- 2. real values, all three modes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued(K, S, mode):
    """normal samples, 37 queries x 1000 candidates (several stripes), mode 2 with 4 cutpoints per sample. The values are those of
    the dense form bit for bit -- the same expression, nothing contracted -- so the ranks are exactly the count on the dense
    scores; against the NumPy reference, whose association differs, the rank lies between the counts of the candidates that win
    and that may win within the rounding bound b of both values"""
    from myfm_amd import _capi

    rng = np.random.default_rng(31 + K + S + mode)
    U, I, n_cut = 37, 1000, 4
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    cuts = rr.sorted_cuts(rng, S, n_cut) if mode == 2 else None
    ref = rr.pair_scores_mode(samples, Xq, Xc, mode, cuts)
    bound = mode2_bound(samples, Xq, Xc, n_cut) if mode == 2 else mode_bound(samples, Xq, Xc, mode)
    targets = kr.draw_targets(rng, U, I, COUNTS)
    exclude = kr.exclude_without(rng, U, I, 0.05, targets)
    P = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets, cutpoints=cuts)
    dense = P.scores(samples, mode=mode)
    rank, value = P.rank(samples, mode=mode)
    P.close()
    check_against_scores(rank, value, dense, targets, exclude)
    p = 0
    for u in range(U):
        allowed = np.ones(I, dtype=bool)
        allowed[exclude[u].indices] = False
        for i in targets[u].indices:
            v = value[p]
            assert abs(v - ref[u, i]) <= bound[u, i]
            lo = np.count_nonzero((ref[u] > v + bound[u]) & allowed)
            hi = np.count_nonzero((ref[u] >= v - bound[u]) & allowed)
            assert lo <= rank[p] <= hi, (u, i, lo, rank[p], hi)
            p += 1
    assert p == rank.size


# ---- 3. consistency with the top-k ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_ranks_of_a_topk_list_are_its_positions(mode):
    from myfm_amd import _capi

    rng = np.random.default_rng(77 + mode)
    U, I, K, S, k = 50, 700, 8, 3, 10
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    exclude = sps.random(U, I, density=0.1, random_state=np.random.RandomState(5), format="csr")
    top = _capi.Pairs(Xq, Xc, exclude=exclude)
    idx, val = top.topk(samples, k, mode=mode)
    top.close()
    assert np.all(idx >= 0)
    targets = sps.csr_matrix((np.ones(U * k), (np.repeat(np.arange(U), k), idx.ravel())), shape=(U, I))
    targets.sort_indices()
    P = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets)
    rank, value = P.rank(samples, mode=mode)
    P.close()
    # the outputs follow the sorted columns of a row: position j of the list is found at the place of idx[u, j] among them
    place = np.argsort(np.argsort(idx, axis=1), axis=1) + k * np.arange(U)[:, None]
    assert np.array_equal(rank[place], np.tile(np.arange(k), (U, 1)))
    assert np.array_equal(value[place], val)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_forms_finish_the_same_value(mode):
    """the dense form, the three selecting tile shapes (k = 10, 100, 256) and the rank form's two passes finish one pair's value
    with the same code, so they agree bit for bit: 65 queries x 600 candidates (two 64-row tiles, two steps of the 512-wide
    shape), rank 33 (KS = 36), 3 samples, real-valued sides, 5 exclusions per row, mode 2 with 4 cutpoints per sample"""
    from myfm_amd import _capi

    rng = np.random.default_rng(123 + mode)
    U, I, K, S, n_cut = 65, 600, 33, 3, 4
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, list(rng.normal(size=7)), mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    cuts = rr.sorted_cuts(rng, S, n_cut) if mode == 2 else None
    ex_cols = np.stack([rng.choice(I - 1, size=5, replace=False) for _ in range(U)])  # (never the last candidate: it is a target)
    exclude = sps.csr_matrix((np.ones(U * 5), (np.repeat(np.arange(U), 5), ex_cols.ravel())), shape=(U, I))
    top = _capi.Pairs(Xq, Xc, exclude=exclude, cutpoints=cuts)
    scores = top.scores(samples, mode=mode)
    lists = {k: top.topk(samples, k, mode=mode) for k in (10, 100, 256)}
    top.close()
    for k, (idx, val) in lists.items():
        assert idx.shape == (U, k) and np.all(idx >= 0)
        assert np.array_equal(val, np.take_along_axis(scores, idx, axis=1)), k
    idx10 = lists[10][0]
    cols = [np.union1d(idx10[u], [I - 1]) for u in range(U)]  # sorted and unique
    indptr = np.concatenate([[0], np.cumsum([c.size for c in cols])])
    t_cols = np.concatenate(cols)
    targets = sps.csr_matrix((np.ones(t_cols.size), t_cols, indptr), shape=(U, I))
    P = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets, cutpoints=cuts)
    rank, value = P.rank(samples, mode=mode)
    P.close()
    assert np.array_equal(value, scores[np.repeat(np.arange(U), np.diff(indptr)), t_cols])
    place = np.stack([indptr[u] + np.searchsorted(cols[u], idx10[u]) for u in range(U)])
    assert np.array_equal(rank[place], np.tile(np.arange(10), (U, 1)))


# ---- 4. independence of chunking and stripes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_query_chunks_give_identical_output(mode):
    """a scratch bound of one byte leaves one 64-row tile per chunk: 200 queries take four chunks, the default bound one"""
    from myfm_amd import _capi

    rng = np.random.default_rng(9 + mode)
    U, I, K, S = 200, 300, 8, 3
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    targets = kr.draw_targets(rng, U, I, COUNTS)
    targets = sps.csr_matrix(sps.diags((np.arange(U) // 64 != 1).astype(np.float64)) @ targets)  # (the second chunk has no target)
    targets.eliminate_zeros()
    targets.sort_indices()
    exclude = kr.exclude_without(rng, U, I, 0.05, targets)
    one = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets)
    many = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets, scratch_bound=1)
    a, b = one.rank(samples, mode), many.rank(samples, mode)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check_against_scores(*b, one.scores(samples, mode), targets, exclude)
    one.close()
    many.close()


def test_long_stripes_few_queries():
    """2 queries x 20 000 candidates: 157 steps on 64 stripes at the most, so stripes of 3 steps whose counters are carried from
    step to step and the last of which is clipped; exact data (ties) and real-valued data, with exclusions"""
    from myfm_amd import _capi

    rng = np.random.default_rng(611)
    U, I, K, S = 2, 20000, 8, 3
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 12, 40, HALVES, mean_nnz=3.0, empty_every=0)
    targets = kr.draw_targets(rng, U, I, [64, 5])
    exclude = kr.exclude_without(rng, U, I, 0.02, targets)
    P = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets)
    small = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets, scratch_bound=1)
    for samples in (pr.exact_samples(rng, D, K, S), pr.normal_samples(rng, D, K, S, scale=0.3)):
        rank, value = P.rank(samples, 0)
        check_against_scores(rank, value, P.scores(samples, 0), targets, exclude)
        again = small.rank(samples, 0)
        assert np.array_equal(again[0], rank) and np.array_equal(again[1], value)
    P.close()
    small.close()


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------
def test_edges():
    from myfm_amd import _capi

    rng = np.random.default_rng(5)
    U, I, K, S = 9, 70, 4, 2
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 12, 20, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    # no targets at all: none given, and an empty pattern
    for t in (None, sps.csr_matrix((U, I))):
        P = _capi.Pairs(Xq, Xc, targets=t)
        rank, value = P.rank(samples)
        assert rank.shape == (0,) and rank.dtype == np.int64 and value.shape == (0,)
        P.close()
    # rows whose every non-target candidate is excluded: one target has rank 0, three targets have ranks 0, 1, 2
    targets = sps.csr_matrix((np.ones(5), ([2, 4, 4, 4, 7], [69, 0, 33, 50, 10])), shape=(U, I))
    exclude = sps.lil_matrix((U, I))
    exclude[2, :69] = 1.0
    exclude[4, :] = 1.0
    exclude[4, [0, 33, 50]] = 0.0
    exclude = sps.csr_matrix(exclude)
    exclude.eliminate_zeros()
    P = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets)
    rank, value = P.rank(samples)
    check_against_scores(rank, value, P.scores(samples), targets, exclude)
    assert rank[0] == 0 and sorted(rank[1:4].tolist()) == [0, 1, 2]
    P.close()
    # 65 targets in one row; a target that is excluded; unsorted input is sorted by the wrapper
    many = sps.csr_matrix((np.ones(65), (np.full(65, 3), np.arange(65))), shape=(U, I))
    with pytest.raises(ValueError, match="query row 3 has 65 targets"):
        _capi.Pairs(Xq, Xc, targets=many)
    with pytest.raises(ValueError, match=r"query row 4, candidate 33\) is also excluded"):
        _capi.Pairs(Xq, Xc, exclude=sps.csr_matrix(([1.0], ([4], [33])), shape=(U, I)), targets=targets)
    with pytest.raises(ValueError, match="targets must have shape"):
        _capi.Pairs(Xq, Xc, targets=sps.csr_matrix((U, I + 1)))
    # no candidates
    P = _capi.Pairs(Xq, sps.csr_matrix((0, D)), targets=sps.csr_matrix((U, 0)))
    rank, value = P.rank(samples)
    assert rank.shape == (0,) and value.shape == (0,)
    P.close()


def test_store_and_host_samples_agree():
    from myfm_amd import _capi

    rng = np.random.default_rng(15)
    U, I, K, S = 20, 300, 8, 4
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 12, 20, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    store = _capi.Store(D, K)
    for s in samples:
        store.push(*s)
    targets = kr.draw_targets(rng, U, I, COUNTS)
    P = _capi.Pairs(Xq, Xc, targets=targets)
    a, b = P.rank(samples, 1), P.rank_store(store, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = P.rank_store(store, 1, first=1, count=2)
    check_against_scores(*c, P.scores(samples[1:3], 1), targets, None)
    P.close()
    store.close()


# ---- 6. the estimator boundary -------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS = 40, 130


@pytest.fixture(scope="module")
def table():
    X, y, shapes = ds.onehot_mf(2500, N_USERS, N_ITEMS, rank_true=4, seed=2)
    D = N_USERS + N_ITEMS
    Xq = sps.csr_matrix((np.ones(N_USERS), (np.arange(N_USERS), np.arange(N_USERS))), shape=(N_USERS, D))
    Xc = sps.csr_matrix((np.ones(N_ITEMS), (np.arange(N_ITEMS), N_USERS + np.arange(N_ITEMS))), shape=(N_ITEMS, D))
    X = sps.csr_matrix(X)
    X.sort_indices()
    seen = sps.csr_matrix((np.ones(X.shape[0]), (X.indices[0::2], X.indices[1::2] - N_USERS)), shape=(N_USERS, N_ITEMS))
    seen.sum_duplicates()
    rng = np.random.default_rng(4)
    targets = kr.draw_targets(rng, N_USERS, N_ITEMS, [3, 0, 1, 100, 7])  # (100 targets in a row: more than one device call)
    return X, y, shapes, Xq, Xc, _without(seen, targets), targets


def _without(seen, targets):
    """the seen pairs that are no targets, as a pattern"""
    T = sps.csr_matrix((np.ones(targets.nnz), targets.indices, targets.indptr), shape=targets.shape)
    E = sps.csr_matrix(seen - seen.multiply(T))
    E.eliminate_zeros()
    return E


def _rank_checks(est, Xq, Xc, exclude, targets, **rel):
    from myfm_amd.utils.ranking import ranking_metrics

    dense = est.predict_pairs(Xq, Xc, **rel)
    for ex in (exclude, None):
        res = est.predict_rank(Xq, Xc, targets, exclude=ex, **rel)
        rrank, rvalue, rn = kr.rank_ref_fast(dense, targets, ex)
        assert res.rank.dtype == np.int64 and np.array_equal(res.rank, rrank)
        assert np.array_equal(res.value, rvalue) and np.array_equal(res.n_candidates, rn)
        got, want = ranking_metrics(res, targets, k=10), kr.metrics_ref(dense, targets, ex, k=10)
        assert set(got) == set(want)
        for name in want:
            assert got[name] == pytest.approx(want[name], rel=1e-12, abs=1e-15), name


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered", "variational"])
def test_estimator_boundary(kind, table):
    """predict_rank equals the brute-force count on predict_pairs of the same estimator, values bit for bit, and ranking_metrics
    the metrics computed from that dense matrix -- from the device store, and after a pickle round trip from host samples; one row
    has 100 targets, which the estimator serves in two device calls"""
    import myfm_amd

    X, y, shapes, Xq, Xc, exclude, targets = table
    if kind == "regressor":
        est = myfm_amd.MyFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=30, n_kept_samples=10, group_shapes=shapes)
    elif kind == "classifier":
        est = myfm_amd.MyFMClassifier(rank=8, random_seed=3).fit(X, y > np.median(y), n_iter=30, n_kept_samples=10, group_shapes=shapes)
    elif kind == "ordered":
        y5 = np.searchsorted(np.quantile(y, [0.2, 0.4, 0.6, 0.8]), y, side="right").astype(np.int64)
        est = myfm_amd.MyFMOrderedProbit(rank=8, random_seed=3).fit(X, y5, n_iter=30, n_kept_samples=10, group_shapes=shapes)
    else:
        est = myfm_amd.VariationalFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=30, group_shapes=shapes)
    assert np.diff(targets.indptr).max() == 100
    _rank_checks(est, Xq, Xc, exclude, targets)
    _rank_checks(pickle.loads(pickle.dumps(est)), Xq, Xc, exclude, targets)


def test_estimator_boundary_with_blocks(rel_table):  # noqa: F811
    """a regressor fitted with relation blocks, the sides given as X_rel_query=[ub, None], X_rel_cand=[None, ib]; a row with 66 of
    the 70 candidates as targets makes the second device call run over a subset of the query rows and of the block's map"""
    import myfm_amd

    t = rel_table
    RB = myfm_amd.RelationBlock
    U, I = t["seen"].shape
    est = _rel_fit("regressor", t, True)
    Xq, Xc = sps.csr_matrix(np.ones((U, 1))), sps.csr_matrix((I, 1))
    rel = dict(X_rel_query=[RB(np.arange(U), t["UB"]), None], X_rel_cand=[None, RB(np.arange(I), t["IB"])])
    targets = kr.draw_targets(np.random.default_rng(8), U, I, [2, 0, 66, 1, 5])
    exclude = _without(t["seen"], targets)
    _rank_checks(est, Xq, Xc, exclude, targets, **rel)
    _rank_checks(pickle.loads(pickle.dumps(est)), Xq, Xc, exclude, targets, **rel)
