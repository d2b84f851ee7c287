"""Ranking under each kept sample on the device: the per-sample selecting form of the tile kernel behind its two
plans (every sample's list, the list of a row's own sample), the vote that turns the lists into top-k inclusion probabilities,
the slicing of the plan, relation-block sides, the estimator boundary and the errors of the C entry points. The shapes are
test_gpu_pairs.py's."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests import pairs_samples_ref as sref
from tests import pairs_ucb_ref as ur
from tests.test_gpu_pairs import HALVES, N_ITEMS, N_USERS, check_topk, mode_bound, table  # noqa: F401  (table: the fixture)

pytestmark = pytest.mark.gpu


def sample_bound(sample, Xq, Xc, mode, n_cut):
    """b_s of pairs_ucb_ref.bounds: the bound of the value of every pair under the one sample"""
    return n_cut * (0.4 * mode_bound([sample], Xq, Xc, 0) + 1e-14) if mode == 2 else mode_bound([sample], Xq, Xc, mode)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. exact layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
@pytest.mark.parametrize("I", [5, 16, 250])
@pytest.mark.parametrize("U", [1, 17, 37])
def test_exact_layout(U, I, K, S):
    """small integers and halves: every v_s is exact in fp64 and ties are frequent, so indices and values of every sample's list
    equal the reference's bit for bit under the total order, on all three tile shapes; and the vote equals the reference vote of
    those lists bit for bit -- I < k included, where the tails carry no vote and the missing entries are -1 / 0.0."""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    samples = pr.exact_samples(rng, D, K, S)
    vals = ur.sample_values(samples, Xq, Xc, 0)
    P = _capi.Pairs(Xq, Xc)
    for k in (10, 100, 256):
        ridx, rval = sref.sample_lists(vals, k)
        idx, val = P.topk_samples(samples, k, mode=0)
        assert idx.shape == (S, U, k) and idx.dtype == np.int64 and val.shape == (S, U, k)
        assert np.array_equal(idx, ridx) and np.array_equal(val, rval), k
        for n_top in (1, k, 256):
            pidx, prob = P.topk_prob(samples, k, n_top, mode=0)
            assert pidx.dtype == np.int64
            assert _same((pidx, prob), sref.vote(ridx, n_top)), (k, n_top)
    P.close()


# ---- 2. the same value as the other forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_cut", [(0, 0), (1, 0), (2, 1), (2, 4)])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued(K, mode, n_cut):
    """normal samples, 1000 candidates over several stripes, 5 % of the pairs excluded. Sample s's list is bit for bit the
    reference top k of the moments form's mean over that one sample (the value of a pair under a sample is finished by the
    same code in both forms), and meets check_topk against the longdouble per-sample values under the single-sample bound b_s."""
    from myfm_amd import _capi

    S = 5
    rng = np.random.default_rng(31 + K + S + n_cut)
    U, I = 37, 1000
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    cuts = rr.sorted_cuts(rng, S, n_cut) if mode == 2 else None
    vals = np.asarray(ur.sample_values(samples, Xq, Xc, mode, cuts), dtype=np.float64)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    P = _capi.Pairs(Xq, Xc, exclude=ex, cutpoints=cuts)
    lists = {k: P.topk_samples(samples, k, mode=mode) for k in (10, 100, 256)}
    worst = 0.0
    for s in range(S):
        P1 = _capi.Pairs(Xq, Xc, exclude=ex, cutpoints=None if cuts is None else cuts[s:s + 1])
        one_mean, one_std = P1.moments(samples[s:s + 1], mode=mode)
        P1.close()
        assert np.all(one_std == 0.0)
        b_s = sample_bound(samples[s], Xq, Xc, mode, n_cut)
        for k, (idx, val) in lists.items():
            assert _same((idx[s], val[s]), pr.topk(one_mean, k, ex)), (s, k)
            check_topk(idx[s], val[s], vals[s], b_s, k, ex)
            ok = idx[s] >= 0
            worst = max(worst, float((np.abs(val[s][ok] - ur.at(vals[s], idx[s])[ok]) / ur.at(b_s, idx[s])[ok]).max()))
    print("K %d mode %d n_cut %d: per-sample lists, largest |value - ref| / tolerance = %.3g" % (K, mode, n_cut, worst))
    P.close()


# ---- 3. the vote on real data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 37])
def test_vote_on_real_data(S):
    """topk_prob equals the reference vote applied to the device's own topk_samples lists, bit for bit (37 samples x k = 256:
    9472 votes per row, a sort of 16384)"""
    from myfm_amd import _capi

    rng = np.random.default_rng(500 + S)
    U, I, K = 37, 1000, 8
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    for k in (10, 100, 256):
        idx, _ = P.topk_samples(samples, k, mode=1)
        for n_top in (1, k, 256):
            got = P.topk_prob(samples, k, n_top, mode=1)
            assert _same(got, sref.vote(idx, n_top)), (k, n_top)
            assert np.all(np.diff(got[1], axis=1) <= 0) and got[1].max() <= 1.0
        if S > 1 and k == 10:
            assert 0.0 < P.topk_prob(samples, k, 256, mode=1)[1][:, 10:].max() < 1.0  # (the samples do not agree on their lists)
    P.close()


# ---- 4. Thompson: the list of a row's own sample --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("S,U", [(2, 150), (37, 17), (1, 37)])
def test_rows_own_sample(S, U, k):
    """row u's list under sample row_sample[u] equals every-sample's list [row_sample[u], u] bit for bit. S = 2, U = 150: a group
    spans more than one 64-row tile; S = 37, U = 17: most groups are empty, the rest hold one or two rows; S = 1: one group."""
    from myfm_amd import _capi

    rng = np.random.default_rng(40 + S + U)
    I, K = 300, 8
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    for seed in (0, 11):
        rs = sref.thompson_samples(seed, S, U)
        for mode in (0, 1):
            P = _capi.Pairs(Xq, Xc, exclude=ex)
            idx, val = P.topk_samples(samples, k, mode=mode)
            tidx, tval = P.topk_samples(samples, k, mode=mode, row_sample=rs)
            assert tidx.shape == (U, k) and tidx.dtype == np.int64
            rows = np.arange(U)
            assert _same((tidx, tval), (idx[rs, rows], val[rs, rows])), (seed, mode)
            P.close()
    if S > 1:
        assert np.unique(sref.thompson_samples(0, S, U)).size > 1


# ---- 5. slicing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 256])
def test_slices_give_identical_output(k):
    """150 queries x 1000 candidates, 5 samples. The default bound takes the plan in one launch. A bound of one byte leaves one
    64-row chunk and one entry per slice: cuts between query chunks, between samples and (k = 256, 16-row tiles) inside a
    sample's tiles. 250 000 and 600 000 bytes keep all rows in one chunk of the every-sample calls and give slices of 2 of its
    15 entries (k = 10) or of 1 and 3 of its 50 (k = 256): cuts inside a sample's row tiles and across samples. All outputs of
    the three calls are identical."""
    from myfm_amd import _capi

    rng = np.random.default_rng(90)
    U, I, K, S = 150, 1000, 8, 5
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    rs = sref.thompson_samples(5, S, U)

    def outputs(P):
        out = P.topk_samples(samples, k, mode=1) + P.topk_samples(samples, k, mode=1, row_sample=rs)
        for n_top in (1, k, 256):
            out = out + P.topk_prob(samples, k, n_top, mode=1)
        P.close()
        return out

    whole = outputs(_capi.Pairs(Xq, Xc, exclude=ex))
    assert _same(whole[4:6], sref.vote(whole[0], 1)) and _same(whole[8:10], sref.vote(whole[0], 256))
    for bound in (1, 250_000, 600_000, 5_000_000):
        assert _same(whole, outputs(_capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=bound))), bound


# ---- 6. relation-block sides ----------------------------------------------------------------------------------------------------
def test_relation_block_sides():
    """two blocks per side (test_gpu_pairs_rel.py's construction) against the sides expanded on the host: with exact data all
    three outputs are equal bit for bit; with real-valued data both calls meet check_topk under the single-sample bound, and
    each call's vote is the reference vote of its own lists"""
    from myfm_amd import _capi

    rng = np.random.default_rng(23)
    U, I, S, k = 37, 250, 5, 10
    sd = rr.block_sides(rng, U, I, 9, 11, 2, 2, mean_nnz=2.0)
    Fq, Fc = rr.flat_sides(sd)
    Xq, Xc, rq, rc = rr.capi_args(sd)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    rs = sref.thompson_samples(2, S, U)
    rows = np.arange(U)
    for exact in (True, False):
        samples = pr.exact_samples(rng, sd["D"], 8, S) if exact else pr.normal_samples(rng, sd["D"], 8, S, scale=0.3)
        vals = np.asarray(ur.sample_values(samples, Fq, Fc, 0), dtype=np.float64)
        got = []
        for P in (_capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, exclude=ex), _capi.Pairs(Fq, Fc, exclude=ex)):
            lists, own, prob = P.topk_samples(samples, k), P.topk_samples(samples, k, row_sample=rs), P.topk_prob(samples, k, 20)
            P.close()
            for s in range(S):
                check_topk(lists[0][s], lists[1][s], vals[s], sample_bound(samples[s], Fq, Fc, 0, 0), k, ex)
            assert _same(own, (lists[0][rs, rows], lists[1][rs, rows]))
            assert _same(prob, sref.vote(lists[0], 20))
            got.append(lists + own + prob)
        if exact:
            assert _same(got[0], got[1])
            assert _same(got[0][:2], sref.sample_lists(vals, k, ex))


# ---- 7. the estimator boundary ---------------------------------------------------------------------------------------------------
def _fit(kind, X, y, shapes):
    import myfm_amd

    kw = dict(n_iter=30, n_kept_samples=10, group_shapes=shapes)
    if kind == "regressor":
        return myfm_amd.MyFMRegressor(rank=8, random_seed=3).fit(X, y, **kw)
    if kind == "classifier":
        return myfm_amd.MyFMClassifier(rank=8, random_seed=3).fit(X, y > np.median(y), **kw)
    y5 = np.searchsorted(np.quantile(y, [0.2, 0.4, 0.6, 0.8]), y, side="right").astype(np.int64)
    return myfm_amd.MyFMOrderedProbit(rank=8, random_seed=3).fit(X, y5, **kw)


def _one_sample(est, s):
    """the estimator with kept sample s alone (host samples)"""
    one = pickle.loads(pickle.dumps(est))
    rank, D, task, fms = one.predictor_.__getstate__()
    p = type(one.predictor_).__new__(type(one.predictor_))
    p.__setstate__((rank, D, task, [fms[s]]))
    one.predictor_ = p
    return one


def _boundary_checks(kind, est, Xq, Xc, seen):
    mode = {"regressor": 0, "classifier": 1, "ordered": 2}[kind]
    fms = est.predictor_.samples
    samples = [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in fms]
    n_cut = len(fms[0].cutpoints[0]) if mode == 2 else 0
    S, U, k = len(fms), Xq.shape[0], 10
    r = est.predict_topk_samples(Xq, Xc, k, exclude=seen)
    assert type(r).__name__ == "SampleRankings" and r.indices.shape == (S, U, k) and r.indices.dtype == np.int64
    for s in range(S):
        d = _one_sample(est, s).predict_pairs_dist(Xq, Xc)
        assert np.all(d.std == 0.0)
        check_topk(r.indices[s], r.value[s], d.mean, sample_bound(samples[s], Xq, Xc, mode, n_cut), k, seen)
    assert len({r.indices[s].tobytes() for s in range(S)}) > 1  # (the samples rank differently)
    for n_top in (None, 5, 256):
        p = est.predict_topk_prob(Xq, Xc, k, n_top=n_top, exclude=seen)
        assert type(p).__name__ == "TopKProbability" and p.indices.dtype == np.int64
        assert _same(tuple(p), sref.vote(r.indices, k if n_top is None else n_top)), n_top
    t = est.predict_topk_thompson(Xq, Xc, k, random_seed=4, exclude=seen)
    assert type(t).__name__ == "ThompsonRanking" and t.sample.dtype == np.int64
    assert np.array_equal(t.sample, sref.thompson_samples(4, S, U))
    rows = np.arange(U)
    assert _same((t.indices, t.value), (r.indices[t.sample, rows], r.value[t.sample, rows]))
    assert _same(tuple(t), tuple(est.predict_topk_thompson(Xq, Xc, k, random_seed=4, exclude=seen)))
    other = est.predict_topk_thompson(Xq, Xc, k, random_seed=5, exclude=seen)
    assert not np.array_equal(other.sample, t.sample) and not np.array_equal(other.indices, t.indices)


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_estimator_boundary(kind, table):  # noqa: F811
    """predict_topk_samples[s] against predict_pairs_dist of the estimator that keeps sample s alone, predict_topk_prob against the
    reference vote of predict_topk_samples, predict_topk_thompson against both and its documented draw; from the device store,
    after a pickle round trip (host samples) and on a fold_in result (three new users, queried through their new columns)."""
    X, y, shapes, Xq, Xc, Xpairs, seen = table
    est = _fit(kind, X, y, shapes)
    _boundary_checks(kind, est, Xq, Xc, seen)
    _boundary_checks(kind, pickle.loads(pickle.dumps(est)), Xq, Xc, seen)
    D, n_new, per = N_USERS + N_ITEMS, 3, 6
    rng = np.random.default_rng(5)
    items = np.concatenate([rng.choice(N_ITEMS, size=per, replace=False) for _ in range(n_new)])
    entity = np.repeat(np.arange(n_new), per)
    ctx = sps.csr_matrix((np.ones(items.size), (np.arange(items.size), N_USERS + items)), shape=(items.size, D))
    if kind == "regressor":
        new = est.fold_in(ctx, rng.normal(size=items.size), entity, 0)
    elif kind == "classifier":
        new = est.fold_in_gibbs(ctx, rng.integers(0, 2, size=items.size), entity, 0)
    else:
        new = est.fold_in_gibbs(ctx, rng.integers(0, 5, size=items.size), entity, 0)
    Xq2 = sps.csr_matrix((np.ones(n_new), (np.arange(n_new), D + np.arange(n_new))), shape=(n_new, D + n_new))
    Xc2 = sps.csr_matrix((np.ones(N_ITEMS), (np.arange(N_ITEMS), N_USERS + np.arange(N_ITEMS))), shape=(N_ITEMS, D + n_new))
    seen2 = sps.csr_matrix((np.ones(items.size), (entity, items)), shape=(n_new, N_ITEMS))
    _boundary_checks(kind, new, Xq2, Xc2, seen2)


# ---- 8. errors of the C entry points ---------------------------------------------------------------------------------------------
def test_capi_errors():
    """every refusal leaves the result buffers as they were"""
    from myfm_amd import _capi

    rng = np.random.default_rng(2)
    U, I = 5, 20
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES)
    samples = pr.normal_samples(rng, D, 4, 3)
    P = _capi.Pairs(Xq, Xc)
    src = _capi._host(samples)
    idx, val = np.full(3 * U * 256, -7, dtype=np.int64), np.full(3 * U * 256, 123.0)

    def refused(symbol, source, *tail):
        rc = source.call(symbol, P.h, *tail, _capi._p(idx), _capi._p(val))
        assert rc != 0 and np.all(idx == -7) and np.all(val == 123.0), (symbol, tail)
        return _capi.lib().mfm_pairs_last_error(P.h).decode()

    for at, bad in ((0, 3), (4, -1), (2, 100)):
        rs = np.zeros(U, dtype=np.int32)
        rs[at] = bad
        msg = refused("mfm_pairs_topk_samples", src, 0, 4, _capi._p(rs))
        assert "row_sample: query row %d asks for sample %d" % (at, bad) in msg
    for k in (0, 257):
        assert "k must be in [1, 256]" in refused("mfm_pairs_topk_samples", src, 0, k, None)
        assert "k must be in [1, 256]" in refused("mfm_pairs_topk_prob", src, 0, k, 4)
    for n_top in (0, 257):
        assert "n_top must be in [1, 256]" in refused("mfm_pairs_topk_prob", src, 0, 4, n_top)
    assert "mode 2 needs the samples' cutpoints" in refused("mfm_pairs_topk_samples", src, 2, 4, None)
    assert "mode 2 needs the samples' cutpoints" in refused("mfm_pairs_topk_prob", src, 2, 4, 4)
    many = _capi._host(pr.normal_samples(rng, D, 2, 129))  # 129 * 256 = 33024 > MFM_PAIRS_VOTE_MAX
    assert 129 * 256 > _capi.PAIRS_VOTE_MAX >= 128 * 256
    assert "at most %d list entries per query row" % _capi.PAIRS_VOTE_MAX in refused("mfm_pairs_topk_prob", many, 0, 256, 10)
    # the wrappers raise, and what is allowed works: 128 samples x k = 256 is the limit itself
    with pytest.raises(ValueError, match="n_top must be"):
        P.topk_prob(samples, 4, 0)
    with pytest.raises(ValueError, match="one entry per query row"):
        P.topk_samples(samples, 4, row_sample=np.zeros(U + 1, dtype=np.int32))
    limit = pr.normal_samples(rng, D, 2, 128)
    assert _same(P.topk_prob(limit, 256, 256), sref.vote(P.topk_samples(limit, 256)[0], 256))
    P.close()
