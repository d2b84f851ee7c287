"""Similar rows under each kept sample on the device: the similarity forms of the tile kernel and k_pairs_moments_at
behind them with exact data on every tile edge, real-valued data against the longdouble reference of tests/pairs_sim_ref.py, the
same-set call, identical samples, the chunking, relation-block sides, the refusals and the estimator boundary. The shapes are
test_gpu_pairs.py's.

Tolerance (first order, pairs_sim_ref.bounds): b_s = 1e-10 * bracket_s + 1e-15 per sample, the mean's bound mean_s b_s, the std's
max_s b_s + 4 S 2^-53 rms_s(c_s) + 1e-300, the value's the mean's + |beta| the std's. The bracket of the cosine must stay below
100 for every pair of the real-valued inputs, or the bound would hide an ill-conditioned cosine: asserted on the reference alone."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import datasets as ds
from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests import pairs_sim_ref as sr
from tests import pairs_ucb_ref as ur
from tests.test_gpu_pairs import HALVES
from tests.test_gpu_pairs_ucb import check_ranked

pytestmark = pytest.mark.gpu


def _f64(pair):
    return tuple(np.asarray(x, dtype=np.float64) for x in pair)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _reference(samples, Xa, Xb, metric):
    """(mean, std longdouble, mean's bound, std's bound); the conditioning of the inputs is asserted here, on the reference alone"""
    assert sr.brackets(samples, Xa, Xb, "cosine").max() < 100.0
    vals = sr.sample_values(samples, Xa, Xb, metric)
    return ur.moments_ld(vals) + sr.bounds(samples, Xa, Xb, metric, vals)


# ---- 1. exact layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
@pytest.mark.parametrize("I", [5, 16, 250])
@pytest.mark.parametrize("U", [1, 17, 37])
def test_exact_layout(U, I, K, S):
    """pairs_sim_ref.exact_unit_samples and unit sides, S <= 2: every norm is a power of two, so r, the cosine, the inner product,
    the mean and std = |a - b| / 2 are exact in fp64 under any association (tests/test_pairs_sim_cpu.py). Dense mean and std and
    value / mean / std of the lists equal the reference bit for bit, the index lists (ties are frequent) equal the reference's
    under the total order -- all three selecting tile shapes and k_pairs_moments_at behind each; sides with shared columns (a
    similarity handle) and with disjoint ones (either kind of handle); empty rows give 0 under both metrics."""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S)
    D = 20
    samples = sr.exact_unit_samples(rng, D, K, S)
    for shared in (True, False):
        Xq, Xc = sr.unit_sides(rng, U, I, D, shared)
        handles = [_capi.Pairs(Xq, Xc, similarity=True)] + ([] if shared else [_capi.Pairs(Xq, Xc)])
        for metric in sr.METRICS:
            rmean, rstd = _f64(sr.moments(samples, Xq, Xc, metric))
            empty_q, empty_c = np.diff(Xq.indptr) == 0, np.diff(Xc.indptr) == 0
            for P in handles:
                mean, std = P.sim(samples, metric)
                assert mean.shape == (U, I) and std.shape == (U, I)
                assert np.array_equal(mean, rmean), (shared, metric, np.argwhere(mean != rmean)[:8])
                assert np.array_equal(std, rstd), (shared, metric, np.argwhere(std != rstd)[:8])
                assert np.all(mean[empty_q] == 0.0) and np.all(mean[:, empty_c] == 0.0)
                if S == 1:
                    assert np.all(std == 0.0)
            for beta in (0.0, 1.0, -2.0):
                ref = rmean + beta * rstd
                for k in (10, 100, 256):
                    ridx, rval = pr.topk(ref, k)
                    want = (ridx, rval, ur.at(rmean, ridx), ur.at(rstd, ridx))
                    for P in handles:
                        assert _same(P.topk_sim(samples, k, metric, beta), want), (shared, metric, beta, k)
        for P in handles:
            P.close()


# ---- 2. real values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sr.METRICS)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued(K, S, shared, metric):
    """normal samples, multi-hot sides, 1000 candidates over several stripes; `shared`: the queries are the first 37 candidates
    (every column shared, a similarity handle) and 5 % of the pairs are excluded. The checks are test_gpu_pairs_ucb.check_ranked's."""
    from myfm_amd import _capi

    rng = np.random.default_rng(31 + K + S)
    U, I = 37, 1000
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    ex = None
    if shared:
        Xq = Xc[:U]
        ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    rmean, rstd, b_mean, b_std = _reference(samples, Xq, Xc, metric)
    P = _capi.Pairs(Xq, Xc, exclude=ex, similarity=shared)
    mean, std = P.sim(samples, metric)
    use_mean = float((np.abs(mean - rmean) / b_mean).max())
    use_std = float((np.abs(std - rstd) / b_std).max())
    print("K %d S %d shared %d %s: dense mean %.3g, dense std %.3g of the tolerance" % (K, S, shared, metric, use_mean, use_std))
    assert use_mean <= 1.0 and use_std <= 1.0
    assert float(np.asarray(rstd, dtype=np.float64).max()) > 1e-2  # (there is a spread to rank by)
    if metric == "cosine":
        assert np.abs(mean).max() <= 1.0 + 1e-9
    worst = np.zeros(4)
    for beta in (0.0, 1.0, -0.5):
        for k in (10, 100, 256):
            worst = np.maximum(worst, check_ranked(P.topk_sim(samples, k, metric, beta), k, beta, rmean, rstd, b_mean, b_std, ex))
    print("   ranked: value %.3g, mean %.3g, std %.3g, value - (mean + beta std) %.3g of the tolerance" % tuple(worst))
    P.close()


# ---- 3. the same set on both sides ---------------------------------------------------------------------------------------------------
def test_same_set():
    """items against themselves. With the diagonal excluded no row lists itself; without, every row with a nonzero embedding has
    itself or an exact duplicate at the head, with a cosine mean within the tolerance of 1."""
    from myfm_amd import _capi

    rng = np.random.default_rng(77)
    R, D, K, S = 150, 30, 8, 5
    rows = []
    for r in range(R):
        if r % 9 == 8:
            rows.append({})  # an empty row
        elif r % 11 == 10:
            rows.append(dict(rows[r - 3]))  # an exact duplicate of an earlier row
        else:
            cols = rng.choice(D, size=int(rng.integers(2, 5)), replace=False)
            rows.append({int(c): float(rng.choice(HALVES)) for c in cols})
    X = sps.csr_matrix(([v for row in rows for v in row.values()], ([r for r, row in enumerate(rows) for _ in row], [c for row in rows for c in row])),
                       shape=(R, D))
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    rmean, rstd, b_mean, b_std = _reference(samples, X, X, "cosine")
    twins = [{v for v in range(R) if rows[v] == rows[u]} for u in range(R)]
    # the inputs: apart from a row's duplicates nothing is parallel to it (asserted on the reference)
    for u in range(R):
        if rows[u]:
            others = np.asarray([v for v in range(R) if v not in twins[u]])
            assert float(np.asarray(rmean, dtype=np.float64)[u, others].max()) < 1.0 - 1e-6
    k = 10
    with_diag = _capi.Pairs(X, X, similarity=True)
    idx, val, mean, std = with_diag.topk_sim(samples, k, "cosine", 0.0)
    check_ranked((idx, val, mean, std), k, 0.0, rmean, rstd, b_mean, b_std)
    for u in range(R):
        if rows[u]:
            assert int(idx[u, 0]) in twins[u], u
            assert abs(mean[u, 0] - 1.0) <= b_mean[u, idx[u, 0]] and std[u, 0] <= b_std[u, idx[u, 0]], u
        else:
            assert np.all(val[u] == 0.0) and np.array_equal(idx[u], np.arange(k))  # (all ties at 0: the smallest indices)
    with_diag.close()
    diag = sps.identity(R, format="csr")
    no_diag = _capi.Pairs(X, X, exclude=diag, similarity=True)
    got = no_diag.topk_sim(samples, k, "cosine", 0.0)
    assert not np.any(got[0] == np.arange(R)[:, None])
    check_ranked(got, k, 0.0, rmean, rstd, b_mean, b_std, diag)
    no_diag.close()


# ---- 4. identical samples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sr.METRICS)
def test_identical_samples(metric):
    """one sample pushed three times: d = c - mean is 0 from the second sample on, so std == 0.0 everywhere, with real values"""
    from myfm_amd import _capi

    rng = np.random.default_rng(64)
    U, I, K = 37, 250, 8
    _, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    Xq = Xc[:U]
    samples = pr.normal_samples(rng, D, K, 1, scale=0.3) * 3
    P = _capi.Pairs(Xq, Xc, similarity=True)
    mean, std = P.sim(samples, metric)
    assert np.all(std == 0.0)
    one_mean, one_std = P.sim(samples[:1], metric)
    assert np.array_equal(mean, one_mean) and np.all(one_std == 0.0)
    for k, beta in ((10, 1.0), (100, -2.0), (256, 0.5)):
        idx, val, m, s = P.topk_sim(samples, k, metric, beta)
        ok = idx >= 0
        assert np.all(s[ok] == 0.0)
        assert np.array_equal(val, np.where(ok, ur.at(mean, idx), -np.inf))
    P.close()


# ---- 5. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sr.METRICS)
def test_query_chunks_give_identical_output(metric):
    """a scratch bound of one byte leaves one 64-row tile per chunk: 150 queries take three chunks, the default bound one"""
    from myfm_amd import _capi

    rng = np.random.default_rng(9)
    U, I, K, S = 150, 300, 8, 3
    _, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    Xq = Xc[:U]
    samples = pr.normal_samples(rng, D, K, S)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    one, many = _capi.Pairs(Xq, Xc, exclude=ex, similarity=True), _capi.Pairs(Xq, Xc, exclude=ex, similarity=True, scratch_bound=1)
    assert _same(one.sim(samples, metric), many.sim(samples, metric))
    for k, beta in ((10, 1.0), (100, -0.5), (256, 0.0)):
        assert _same(one.topk_sim(samples, k, metric, beta), many.topk_sim(samples, k, metric, beta)), k
    rmean, rstd, b_mean, b_std = _reference(samples, Xq, Xc, metric)
    check_ranked(many.topk_sim(samples, 10, metric, 1.0), 10, 1.0, rmean, rstd, b_mean, b_std, ex)
    one.close()
    many.close()


# ---- 6. relation-block sides -----------------------------------------------------------------------------------------------------
def _block_sides(rng, U, I, exact):
    """a user block on the query side (position 0) and one item block on both sides (position 1) behind main matrices of width D0.
    exact: every side row holds one stored entry in total -- the main part is empty and only the item block's rows (one entry
    each) are pointed at, the user block's rows being empty."""
    D0, wu, wi = 23, 6, 7
    if exact:
        Xq, Xc = sps.csr_matrix((U, D0)), sps.csr_matrix((I, D0))
        Bu = sps.csr_matrix((3, wu))
        Bi = sps.csr_matrix((rng.choice(sr.UNIT_VALUES, size=wi), (np.arange(wi), rng.permutation(wi))), shape=(wi, wi))
        ou, oq, oc = rng.integers(0, 3, size=U), rng.integers(0, wi, size=U), rng.integers(0, wi, size=I)
    else:
        Xq, Xc, _ = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0)
        (ou, Bu), (oq, Bi) = rr.make_block(rng, U, wu), rr.make_block(rng, U, wi)
        oc = rng.integers(0, Bi.shape[0], size=I)
    D = D0 + wu + wi
    pad = lambda X: sps.hstack([X, sps.csr_matrix((X.shape[0], wu + wi))], format="csr")
    rq, rc = [(D0, ou, Bu), (D0 + wu, oq, Bi)], [(D0 + wu, oc, Bi)]
    Fq, Fc = rr.expand(Xq, [(ou, Bu), (oq, Bi)]), rr.expand(Xc, [None, (oc, Bi)], [wu, wi])
    return pad(Xq), pad(Xc), rq, rc, Fq, Fc, D


@pytest.mark.parametrize("metric", sr.METRICS)
def test_relation_block_sides(metric):
    """block sides against the sides expanded on the host (a call without blocks) and against the reference, within the tolerance;
    exact data with one stored entry per side row in total bit for bit"""
    from myfm_amd import _capi

    rng = np.random.default_rng(23)
    U, I = 37, 250
    Xq, Xc, rq, rc, Fq, Fc, D = _block_sides(rng, U, I, exact=False)
    samples = pr.normal_samples(rng, D, 8, 5, scale=0.3)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    blocked = _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, exclude=ex, similarity=True)
    flat = _capi.Pairs(Fq, Fc, exclude=ex, similarity=True)
    rmean, rstd, b_mean, b_std = _reference(samples, Fq, Fc, metric)
    (ma, sa), (mb, sb) = blocked.sim(samples, metric), flat.sim(samples, metric)
    for m, s in ((ma, sa), (mb, sb)):
        assert np.all(np.abs(m - rmean) <= b_mean) and np.all(np.abs(s - rstd) <= b_std)
    assert np.all(np.abs(ma - mb) <= b_mean) and np.all(np.abs(sa - sb) <= b_std)
    for P in (blocked, flat):
        check_ranked(P.topk_sim(samples, 10, metric, 1.0), 10, 1.0, rmean, rstd, b_mean, b_std, ex)
        P.close()
    # a column twice in one side is still refused on a similarity handle
    with pytest.raises(ValueError, match="already stored in this side"):
        _capi.Pairs(Xq, Xc, rel_query=[rq[1], rq[1]], similarity=True)
    with pytest.raises(ValueError, match="X_query and X_cand share column"):
        _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc)

    Xq, Xc, rq, rc, Fq, Fc, D = _block_sides(rng, U, I, exact=True)
    assert np.all(np.diff(Fq.indptr) == 1) and np.all(np.diff(Fc.indptr) == 1)
    samples = sr.exact_unit_samples(rng, D, 4, 2)
    blocked, flat = _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, similarity=True), _capi.Pairs(Fq, Fc, similarity=True)
    want = _f64(sr.moments(samples, Fq, Fc, metric))
    assert _same(blocked.sim(samples, metric), want) and _same(flat.sim(samples, metric), want)
    for k, beta in ((10, 1.0), (100, -2.0), (256, 0.0)):
        ridx, rval = pr.topk(want[0] + beta * want[1], k)
        full = (ridx, rval, ur.at(want[0], ridx), ur.at(want[1], ridx))
        assert _same(blocked.topk_sim(samples, k, metric, beta), full) and _same(flat.topk_sim(samples, k, metric, beta), full), k
    blocked.close()
    flat.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from myfm_amd import _capi

    rng = np.random.default_rng(2)
    Xq, Xc, D = pr.disjoint_sides(rng, 5, 20, 9, 11, HALVES)
    samples = pr.normal_samples(rng, D, 4, 2)
    P = _capi.Pairs(Xq, Xc, similarity=True)
    for call in (lambda: P.scores(samples), lambda: P.topk(samples, 3), lambda: P.topk_ucb(samples, 3), lambda: P.moments(samples),
                 lambda: P.topk_samples(samples, 3), lambda: P.topk_prob(samples, 3), lambda: P.rank(samples),
                 lambda: P.moments_vb((0.0, 0.0, np.zeros(D), np.zeros(D), np.zeros((D, 2)), np.zeros((D, 2)))),
                 lambda: P.topk_bound_vb((0.0, 0.0, np.zeros(D), np.zeros(D), np.zeros((D, 2)), np.zeros((D, 2))), 3, 1.0)):
        with pytest.raises(ValueError, match="similarity handle"):
            call()
    for bad in (0, 257):
        with pytest.raises(ValueError, match="k must be"):
            P.topk_sim(samples, bad)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="beta must be a finite"):
            P.topk_sim(samples, 3, beta=bad)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="bad similarity metric"):
            P.topk_sim(samples, 3, metric=bad)
        with pytest.raises(ValueError, match="bad similarity metric"):
            P.sim(samples, metric=bad)
    # both entry points work on a plain handle too, and its own forms go on working
    Q = _capi.Pairs(Xq, Xc)
    assert _same(Q.sim(samples, "dot"), P.sim(samples, "dot")) and _same(Q.topk_sim(samples, 3), P.topk_sim(samples, 3))
    assert Q.scores(samples).shape == (5, 20)
    # the tail: 20 candidates, k = 30
    idx, val, mean, std = P.topk_sim(samples, 30)
    assert np.all(idx[:, 20:] == -1) and np.all(val[:, 20:] == -np.inf) and np.all(np.isnan(mean[:, 20:])) and np.all(np.isnan(std[:, 20:]))
    assert np.all(idx[:, :20] >= 0)
    P.close()
    Q.close()
    big = _capi.Pairs(sps.csr_matrix((4097, D)), sps.csr_matrix((4096, D)), similarity=True)  # 4097 * 4096 > 2^24
    with pytest.raises(ValueError, match="more than 2\\^24 pairs"):
        big.sim(samples)
    big.close()


# ---- 8. the estimator boundary ---------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS, RANK = 30, 20, 4


@pytest.fixture(scope="module")
def tiny_table():
    X, y, shapes = ds.onehot_mf(500, N_USERS, N_ITEMS, rank_true=3, seed=4)
    return X, y, shapes


def _fit(kind, X, y, shapes, seed=3):
    import myfm_amd

    kw = dict(n_iter=12, n_kept_samples=6, group_shapes=shapes)
    if kind == "regressor":
        return myfm_amd.MyFMRegressor(rank=RANK, random_seed=seed).fit(X, y, **kw)
    if kind == "classifier":
        return myfm_amd.MyFMClassifier(rank=RANK, random_seed=seed).fit(X, y > np.median(y), **kw)
    y5 = np.searchsorted(np.quantile(y, [0.2, 0.4, 0.6, 0.8]), y, side="right").astype(np.int64)
    return myfm_amd.MyFMOrderedProbit(rank=RANK, random_seed=seed).fit(X, y5, **kw)


def _one_hot(cols, D):
    return sps.csr_matrix((np.ones(len(cols)), (np.arange(len(cols)), cols)), shape=(len(cols), D))


def _boundary_checks(est, Xq, Xc=None, n_samples=None):
    """predict_similarity and predict_similar of an estimator against the reference computed from its V_samples"""
    fms = est.predictor_.samples
    samples = [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in fms]
    assert n_samples is None or len(samples) == n_samples
    Xb = Xq if Xc is None else Xc
    U, I = Xq.shape[0], Xb.shape[0]
    for metric in sr.METRICS:
        rmean, rstd, b_mean, b_std = _reference(samples, Xq, Xb, metric)
        got = est.predict_similarity(Xq, Xc, metric=metric)
        assert type(got).__name__ == "PairSummary" and got.mean.shape == (U, I) and got.std.shape == (U, I)
        use = float((np.abs(got.mean - rmean) / b_mean).max()), float((np.abs(got.std - rstd) / b_std).max())
        assert max(use) <= 1.0, (metric, use)
        assert float(np.asarray(rstd, dtype=np.float64).max()) > 1e-4
        for beta in (0.0, 1.0):
            r = est.predict_similar(Xq, Xc, k=5, metric=metric, beta=beta)
            assert type(r).__name__ == "RankedSummary" and r.indices.dtype == np.int64
            check_ranked(tuple(r), 5, beta, rmean, rstd, b_mean, b_std, sps.identity(U, format="csr") if Xc is None else None)
            if Xc is None:
                assert not np.any(r.indices == np.arange(U)[:, None])
                full = est.predict_similar(Xq, k=5, metric=metric, beta=beta, exclude_self=False)
                check_ranked(tuple(full), 5, beta, rmean, rstd, b_mean, b_std)


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_estimator_boundary(kind, tiny_table):
    """the items' neighbours from the device store, after a pickle round trip (host samples), on combine_chains of two fits (the
    chains' factors are rotated against each other) and, after fold_in of three new users, the new users' neighbours among the
    fitted users"""
    import myfm_amd

    X, y, shapes = tiny_table
    D = N_USERS + N_ITEMS
    items = _one_hot(N_USERS + np.arange(N_ITEMS), D)
    est = _fit(kind, X, y, shapes)
    _boundary_checks(est, items, n_samples=6)
    _boundary_checks(est, items[:7], items)
    _boundary_checks(pickle.loads(pickle.dumps(est)), items, n_samples=6)
    _boundary_checks(myfm_amd.combine_chains([est, _fit(kind, X, y, shapes, seed=11)]), items, n_samples=12)
    n_new, per = 3, 6
    rng = np.random.default_rng(5)
    seen = np.concatenate([rng.choice(N_ITEMS, size=per, replace=False) for _ in range(n_new)])
    entity = np.repeat(np.arange(n_new), per)
    ctx = _one_hot(N_USERS + seen, D)
    if kind == "regressor":
        new = est.fold_in(ctx, rng.normal(size=seen.size), entity, 0)
    elif kind == "classifier":
        new = est.fold_in_gibbs(ctx, rng.integers(0, 2, size=seen.size), entity, 0)
    else:
        new = est.fold_in_gibbs(ctx, rng.integers(0, 5, size=seen.size), entity, 0)
    _boundary_checks(new, _one_hot(D + np.arange(n_new), D + n_new), _one_hot(np.arange(N_USERS), D + n_new), n_samples=6)
