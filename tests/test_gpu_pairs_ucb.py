"""Ranking by an upper confidence bound on the device: the moments form of the tile kernel and k_pairs_moments_at
with exact data on every tile edge, real-valued data against the longdouble moments of the direct pair rows, identical samples,
the chunking, relation-block sides and the estimator boundary against predict_dist / predict_expected_dist on the pair rows.
The shapes are test_gpu_pairs.py's."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests import pairs_ucb_ref as ur
from tests.test_gpu_pairs import HALVES, N_ITEMS, N_USERS, check_topk, mode_bound, table  # noqa: F401  (table: the fixture)

pytestmark = pytest.mark.gpu


def check_ranked(got, k, beta, ref_mean, ref_std, b_mean, b_std, exclude=None):
    """check_topk's properties of (indices, value) against mean + beta * std under the value's bound; mean and std of the returned
    entries against the reference within theirs; value against mean + beta * std of the same entry within the value's bound;
    tails -1 / -inf / NaN / NaN. Returns the largest error / tolerance of (value, mean, std, value - (mean + beta std))."""
    idx, val, mean, std = got
    b_val = b_mean + abs(beta) * b_std
    ref_val = np.asarray(ref_mean + ur.LD(beta) * ref_std, dtype=np.float64)
    check_topk(idx, val, ref_val, b_val, k, exclude)
    assert mean.shape == idx.shape and std.shape == idx.shape
    ok = idx >= 0
    assert np.all(np.isnan(mean[~ok])) and np.all(np.isnan(std[~ok]))
    use = []
    for g, r_at, b in ((val, ur.at(ref_val, idx), b_val), (mean, ur.at(ref_mean, idx), b_mean), (std, ur.at(ref_std, idx), b_std),
                       (val, mean + beta * std, b_val)):
        use.append(float((np.abs(g[ok] - r_at[ok]) / ur.at(b, idx)[ok]).max()) if ok.any() else 0.0)
    assert max(use) <= 1.0, use
    assert np.all(std[ok] >= 0.0)
    return use


# ---- 1. exact layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
@pytest.mark.parametrize("I", [5, 16, 250])
@pytest.mark.parametrize("U", [1, 17, 37])
def test_exact_layout(U, I, K, S):
    """small integers and halves, S <= 2: every v_s, the mean, var = (a - b)^2 / 4 and std = |a - b| / 2 are exact in fp64
    (tests/test_pairs_ucb_cpu.py), so dense mean and std, and value / mean / std of the top-k, equal the reference bit for bit
    whatever the association, and the index lists (ties are frequent) equal the reference's under the total order -- all three
    tile shapes of the selecting kernel, and k_pairs_moments_at behind each."""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K + 7 * S)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    samples = pr.exact_samples(rng, D, K, S)
    rmean, rstd = (np.asarray(x, dtype=np.float64) for x in ur.moments_ld(ur.sample_values(samples, Xq, Xc, 0)))
    P = _capi.Pairs(Xq, Xc)
    mean, std = P.moments(samples, mode=0)
    assert mean.shape == (U, I) and std.shape == (U, I)
    assert np.array_equal(mean, rmean), np.argwhere(mean != rmean)[:8]
    assert np.array_equal(std, rstd), np.argwhere(std != rstd)[:8]
    if S == 1:
        assert np.all(std == 0.0)
    for beta in (1.0, -2.0, 0.5):
        ref = rmean + beta * rstd
        for k in (10, 100, 256):
            idx, val, m, s = P.topk_ucb(samples, k, beta, mode=0)
            ridx, rval = pr.topk(ref, k)
            assert np.array_equal(idx, ridx) and np.array_equal(val, rval), (beta, k)
            assert np.array_equal(m, ur.at(rmean, ridx), equal_nan=True) and np.array_equal(s, ur.at(rstd, ridx), equal_nan=True), (beta, k)
    P.close()


# ---- 2. real values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_cut", [(0, 0), (1, 0), (2, 1), (2, 4)])
@pytest.mark.parametrize("S", [5, 37])
@pytest.mark.parametrize("K", [8, 33])
def test_real_valued(K, S, mode, n_cut):
    """normal samples, multi-hot sides, 1000 candidates over several stripes, 5 % of the pairs excluded. Tolerances, from b =
    test_gpu_pairs.mode_bound of all samples and b_s of the single sample s: mean b; std max_s b_s + 4 S 2^-53 rms_s(v_s) + 1e-300
    (std is 1-Lipschitz in the sup norm of the values; the second term is the recurrence's own rounding, of which the float64
    twin uses at most 0.11, tests/test_pairs_ucb_cpu.py); value mean's + |beta| std's."""
    from myfm_amd import _capi

    rng = np.random.default_rng(31 + K + S + n_cut)
    U, I = 37, 1000
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S, scale=0.3)
    cuts = rr.sorted_cuts(rng, S, n_cut) if mode == 2 else None
    vals = ur.sample_values(samples, Xq, Xc, mode, cuts)
    rmean, rstd = ur.moments_ld(vals)
    b_mean, b_std = ur.bounds(samples, Xq, Xc, mode, n_cut, vals, mode_bound)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    P = _capi.Pairs(Xq, Xc, exclude=ex, cutpoints=cuts)
    mean, std = P.moments(samples, mode=mode)
    use_mean = float((np.abs(mean - rmean) / b_mean).max())
    use_std = float((np.abs(std - rstd) / b_std).max())
    print("K %d S %d mode %d n_cut %d: dense mean %.3g, dense std %.3g of the tolerance" % (K, S, mode, n_cut, use_mean, use_std))
    assert use_mean <= 1.0 and use_std <= 1.0
    assert float(np.asarray(rstd, dtype=np.float64).max()) > 1e-2  # (there is a spread to rank by)
    worst = np.zeros(4)
    for beta in (1.0, -0.5):
        for k in (10, 100, 256):
            worst = np.maximum(worst, check_ranked(P.topk_ucb(samples, k, beta, mode=mode), k, beta, rmean, rstd, b_mean, b_std, ex))
    print("   ranked: value %.3g, mean %.3g, std %.3g, value - (mean + beta std) %.3g of the tolerance" % tuple(worst))
    P.close()


# ---- 3. identical samples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_identical_samples(mode):
    """one sample pushed three times: d = v - mean is 0 from the second sample on, so std == 0.0 everywhere and the value the
    selection compares is the tile's mean bit for bit (beta * 0 added), with real-valued data. The returned mean is recomputed by
    k_pairs_moments_at in another association: it equals the value within the bound with real-valued data and bit for bit with
    exact data, where no association rounds."""
    from myfm_amd import _capi

    rng = np.random.default_rng(64 + mode)
    U, I, K = 37, 250, 8
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    cuts = np.repeat(rr.sorted_cuts(rng, 1, 3), 3, axis=0) if mode == 2 else None
    P = _capi.Pairs(Xq, Xc, cutpoints=cuts)
    P1 = _capi.Pairs(Xq, Xc, cutpoints=cuts[:1]) if mode == 2 else P  # (the cutpoints are set per sample of the call)
    real, exact = pr.normal_samples(rng, D, K, 1, scale=0.3) * 3, pr.exact_samples(rng, D, K, 1) * 3
    for samples, is_exact in ((real, False), (exact, True)):
        if is_exact and mode != 0:
            continue  # (Phi rounds)
        mean, std = P.moments(samples, mode=mode)
        assert np.all(std == 0.0)
        one_mean, one_std = P1.moments(samples[:1], mode=mode)
        assert np.array_equal(mean, one_mean) and np.all(one_std == 0.0)
        for k, beta in ((10, 1.0), (100, -2.0), (256, 0.5)):
            idx, val, m, s = P.topk_ucb(samples, k, beta, mode=mode)
            ok = idx >= 0
            assert np.all(s[ok] == 0.0)
            assert np.array_equal(val, np.where(ok, ur.at(mean, idx), -np.inf))
            if is_exact:
                assert np.array_equal(val[ok], m[ok])
            else:
                b = 3 * (0.4 * mode_bound(samples, Xq, Xc, 0) + 1e-14) if mode == 2 else mode_bound(samples, Xq, Xc, mode)
                assert np.all(np.abs(val[ok] - m[ok]) <= ur.at(b, idx)[ok])
    P.close()
    P1.close()


# ---- 4. chunking -----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_query_chunks_give_identical_output(mode):
    """a scratch bound of one byte leaves one 64-row tile per chunk: 150 queries take three chunks, the default bound one"""
    from myfm_amd import _capi

    rng = np.random.default_rng(9)
    U, I, K, S = 150, 300, 8, 3
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    samples = pr.normal_samples(rng, D, K, S)
    cuts = rr.sorted_cuts(rng, S, 4) if mode == 2 else None
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    one, many = _capi.Pairs(Xq, Xc, exclude=ex, cutpoints=cuts), _capi.Pairs(Xq, Xc, exclude=ex, cutpoints=cuts, scratch_bound=1)
    assert _same(one.moments(samples, mode), many.moments(samples, mode))
    for k, beta in ((10, 1.0), (100, -0.5), (256, 1.0)):
        assert _same(one.topk_ucb(samples, k, beta, mode), many.topk_ucb(samples, k, beta, mode)), k
    vals = ur.sample_values(samples, Xq, Xc, mode, cuts)
    rmean, rstd = ur.moments_ld(vals)
    b_mean, b_std = ur.bounds(samples, Xq, Xc, mode, 4, vals, mode_bound)
    check_ranked(many.topk_ucb(samples, 10, 1.0, mode), 10, 1.0, rmean, rstd, b_mean, b_std, ex)
    one.close()
    many.close()


def test_long_stripe_few_queries():
    """3 queries x 9000 candidates: more steps than the 64 stripes a launch can have, so stripes of several steps (threshold and
    buffers carried, the last step clipped); exact data with S = 2 must give the reference's lists exactly, one k per tile shape"""
    from myfm_amd import _capi

    rng = np.random.default_rng(611)
    U, I, K, S = 3, 9000, 8, 2
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 12, 40, HALVES, mean_nnz=3.0)
    ex = sps.random(U, I, density=0.02, random_state=np.random.RandomState(2), format="csr")
    one, many = _capi.Pairs(Xq, Xc, exclude=ex), _capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=1)
    samples = pr.exact_samples(rng, D, K, S)
    rmean, rstd = (np.asarray(x, dtype=np.float64) for x in ur.moments_ld(ur.sample_values(samples, Xq, Xc, 0)))
    mean, std = one.moments(samples, 0)
    assert np.array_equal(mean, rmean) and np.array_equal(std, rstd)
    for k, beta in ((10, 1.0), (100, -2.0), (256, 0.5)):
        got = one.topk_ucb(samples, k, beta, 0)
        ridx, rval = pr.topk(rmean + beta * rstd, k, ex)
        assert _same(got, (ridx, rval, ur.at(rmean, ridx), ur.at(rstd, ridx))), k
        assert _same(got, many.topk_ucb(samples, k, beta, 0)), k
    one.close()
    many.close()


@pytest.fixture(scope="module")
def many_tiles():
    rng = np.random.default_rng(612)
    U, I = 2000, 3000
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, HALVES, mean_nnz=2.0, empty_every=5)
    samples = pr.normal_samples(rng, D, 4, 3, scale=0.3)
    ex = sps.random(U, I, density=0.01, random_state=np.random.RandomState(4), format="csr")
    return Xq, Xc, samples, ex


@pytest.mark.parametrize("k", [10, 100, 256])
def test_long_stripes_many_query_tiles(k, many_tiles):
    """2000 queries x 3000 candidates: 32 / 63 / 125 query tiles give 16 / 9 / 5 stripes of several steps in one chunk, and a chunk
    of one 64-row tile takes up to 47 stripes of one step: identical output (real-valued data; the exclusions apply)"""
    from myfm_amd import _capi

    Xq, Xc, samples, ex = many_tiles
    one, many = _capi.Pairs(Xq, Xc, exclude=ex), _capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=1)
    a, b = one.topk_ucb(samples, k, 1.0, 0), many.topk_ucb(samples, k, 1.0, 0)
    assert _same(a, b)
    assert np.all(a[0] >= 0) and np.all(np.diff(a[1], axis=1) <= 0)
    E = ex.tocsr()
    for u in (0, 63, 64, 1999):
        assert not np.intersect1d(a[0][u], E.indices[E.indptr[u]:E.indptr[u + 1]]).size
    if k == 10:
        assert _same(one.moments(samples, 0), many.moments(samples, 0))
    one.close()
    many.close()


# ---- 5. relation-block sides -----------------------------------------------------------------------------------------------------
def test_relation_block_sides():
    """two blocks per side against the sides expanded on the host (a call without blocks) and against the reference"""
    from myfm_amd import _capi

    rng = np.random.default_rng(23)
    sd = rr.block_sides(rng, 37, 250, 9, 11, 2, 2, mean_nnz=2.0)
    Fq, Fc = rr.flat_sides(sd)
    Xq, Xc, rq, rc = rr.capi_args(sd)
    samples = pr.normal_samples(rng, sd["D"], 8, 5, scale=0.3)
    ex = sps.random(37, 250, density=0.05, random_state=np.random.RandomState(3), format="csr")
    blocked, flat = _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, exclude=ex), _capi.Pairs(Fq, Fc, exclude=ex)
    for mode in (0, 1):
        vals = ur.sample_values(samples, Fq, Fc, mode)
        rmean, rstd = ur.moments_ld(vals)
        b_mean, b_std = ur.bounds(samples, Fq, Fc, mode, 0, vals, mode_bound)
        (ma, sa), (mb, sb) = blocked.moments(samples, mode), flat.moments(samples, mode)
        for m, s in ((ma, sa), (mb, sb)):
            assert np.all(np.abs(m - rmean) <= b_mean) and np.all(np.abs(s - rstd) <= b_std)
        assert np.all(np.abs(ma - mb) <= b_mean) and np.all(np.abs(sa - sb) <= b_std)
        for P in (blocked, flat):
            check_ranked(P.topk_ucb(samples, 10, 1.0, mode), 10, 1.0, rmean, rstd, b_mean, b_std, ex)
    blocked.close()
    flat.close()


# ---- 6. the estimator boundary ---------------------------------------------------------------------------------------------------
def _fit(kind, X, y, shapes):
    import myfm_amd

    kw = dict(n_iter=30, n_kept_samples=10, group_shapes=shapes)
    if kind == "regressor":
        return myfm_amd.MyFMRegressor(rank=8, random_seed=3).fit(X, y, **kw)
    if kind == "classifier":
        return myfm_amd.MyFMClassifier(rank=8, random_seed=3).fit(X, y > np.median(y), **kw)
    y5 = np.searchsorted(np.quantile(y, [0.2, 0.4, 0.6, 0.8]), y, side="right").astype(np.int64)
    return myfm_amd.MyFMOrderedProbit(rank=8, random_seed=3).fit(X, y5, **kw)


def _boundary_checks(kind, est, Xq, Xc, Xpairs, seen):
    mode = {"regressor": 0, "classifier": 1, "ordered": 2}[kind]
    fms = est.predictor_.samples
    samples = [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in fms]
    cuts = np.asarray([fm.cutpoints[0] for fm in fms]) if mode == 2 else None
    n_cut = cuts.shape[1] if mode == 2 else 0
    U, I = Xq.shape[0], Xc.shape[0]
    got = est.predict_pairs_dist(Xq, Xc)
    direct = est.predict_expected_dist(Xpairs, quantiles=()) if mode == 2 else est.predict_dist(Xpairs, quantiles=())
    dmean, dstd = np.asarray(direct.mean).reshape(U, I), np.asarray(direct.std).reshape(U, I)
    b_mean, b_std = ur.bounds(samples, Xq, Xc, mode, n_cut, ur.sample_values(samples, Xq, Xc, mode, cuts), mode_bound)
    assert type(got).__name__ == "PairSummary" and got.mean.shape == (U, I) and got.std.shape == (U, I)
    use = float((np.abs(got.mean - dmean) / b_mean).max()), float((np.abs(got.std - dstd) / b_std).max())
    print("%s: predict_pairs_dist against predict_dist on the pair rows: mean %.3g, std %.3g of the tolerance" % ((kind,) + use))
    assert max(use) <= 1.0
    assert np.ptp(dmean) > 1e-3 and dstd.max() > 1e-4
    for beta in (1.0, -0.5):
        r = est.predict_topk_ucb(Xq, Xc, 10, beta=beta, exclude=seen)
        assert type(r).__name__ == "RankedSummary" and r.indices.dtype == np.int64
        check_ranked(tuple(r), 10, beta, got.mean, got.std, b_mean, b_std, seen)


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_estimator_boundary(kind, table):  # noqa: F811
    """predict_pairs_dist equals predict_dist (ordered probit: predict_expected_dist) on the materialised pair rows -- two device
    paths that share no kernel -- and predict_topk_ucb returns entries whose mean and std are that matrix's at the returned
    indices; from the device store, after a pickle round trip (host samples) and on a fold_in result (three new users, queried
    through their new columns)."""
    X, y, shapes, Xq, Xc, Xpairs, seen = table
    est = _fit(kind, X, y, shapes)
    _boundary_checks(kind, est, Xq, Xc, Xpairs, seen)
    _boundary_checks(kind, pickle.loads(pickle.dumps(est)), Xq, Xc, Xpairs, seen)
    # three new users with 6 observations each: their context rows are item one-hots
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
    u, i = np.repeat(np.arange(n_new), N_ITEMS), np.tile(np.arange(N_ITEMS), n_new)
    Xp2 = sps.csr_matrix((np.ones(2 * u.size), (np.repeat(np.arange(u.size), 2), np.stack([N_USERS + i, D + u], 1).ravel())),
                         shape=(u.size, D + n_new))
    seen2 = sps.csr_matrix((np.ones(items.size), (entity, items)), shape=(n_new, N_ITEMS))
    _boundary_checks(kind, new, Xq2, Xc2, Xp2, seen2)


def test_variational_estimators_have_no_such_method():
    import myfm_amd

    for cls in (myfm_amd.VariationalFMRegressor, myfm_amd.VariationalFMClassifier):
        assert not hasattr(cls, "predict_topk_ucb") and not hasattr(cls, "predict_pairs_dist")


# ---- 7. errors of the C entry points ---------------------------------------------------------------------------------------------
def test_capi_errors():
    from myfm_amd import _capi

    rng = np.random.default_rng(2)
    Xq, Xc, D = pr.disjoint_sides(rng, 5, 20, 9, 11, HALVES)
    samples = pr.normal_samples(rng, D, 4, 2)
    P = _capi.Pairs(Xq, Xc)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="k must be"):
            P.topk_ucb(samples, bad)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="beta must be a finite"):
            P.topk_ucb(samples, 3, beta=bad)
    with pytest.raises(ValueError, match="mode 2 needs the samples' cutpoints"):
        P.moments(samples, mode=2)
    # beta = 0 ranks by the mean through this path
    vals = ur.sample_values(samples, Xq, Xc, 0)
    rmean, rstd = ur.moments_ld(vals)
    b_mean, b_std = ur.bounds(samples, Xq, Xc, 0, 0, vals, mode_bound)
    check_ranked(P.topk_ucb(samples, 3, beta=0.0), 3, 0.0, rmean, rstd, b_mean, b_std)
    P.close()
