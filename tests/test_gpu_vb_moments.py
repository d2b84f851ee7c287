"""Analytic score moments of the variational estimators on the device: the row pass and its relation-block tables,
the five-pseudo-sample pair form with fused top-k, the estimator boundary and the C-ABI errors, against tests/vb_moments_ref.py.

Exactness: the device's sqrt is IEEE (correctly rounded), so on data whose variance is exact in fp64 "std^2 equals the reference"
is tested as std == sqrt(var_ref) bit for bit, with var_ref checked to be a float64."""
import ctypes as C
import pickle

import numpy as np
import pytest
import scipy.sparse as sps
from scipy import special

from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests import pairs_ucb_ref as ur
from tests import vb_moments_ref as vr
from tests.test_gpu_pairs import HALVES, N_ITEMS, N_USERS, mode_bound, table  # noqa: F401  (table: the fixture)
from tests.test_gpu_pairs_ucb import check_ranked

pytestmark = pytest.mark.gpu

INTS = [-2.0, -1.0, 1.0, 2.0]


def _f64(a):
    out = np.asarray(a, dtype=np.float64)
    assert np.all(out == a)  # (the longdouble value is a float64: the data are exact)
    return out


def _rows(rng, N, D, values, lens=(0, 1, 2, 7)):
    """CSR (N, D): row t has lens[t % len(lens)] entries in distinct columns, values drawn from `values`"""
    ptr, idx, val = [0], [], []
    for t in range(N):
        n = lens[t % len(lens)]
        idx.extend(np.sort(rng.choice(D, size=n, replace=False)))
        val.extend(rng.choice(values, size=n))
        ptr.append(len(idx))
    return sps.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(idx, dtype=np.int32), np.asarray(ptr, dtype=np.int64)), shape=(N, D))


def _two_blocks(rng, N, values):
    """a block with a single block row that every design row shares, and one of 4 rows of which row 3 is never pointed at"""
    b0 = (np.zeros(N, dtype=np.int64), _rows(rng, 1, 3, values, lens=(2,)))
    b1 = (np.arange(N, dtype=np.int64) % 3, _rows(rng, 4, 5, values, lens=(2, 0, 3, 5)))
    return [b0, b1]


def _expanded(X, blocks):
    return sps.hstack([X] + [B[mp] for mp, B in blocks]).tocsr()


# ---- 1. rows, exact layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_rows_exact_layout(N, K):
    """x in {-2, ..., 2}, integer means, variances in {1/4, 1/2, 1}: every product and sum is exact in fp64, so mean and variance
    equal the reference whatever the association -- a misplaced factor, lane or block row cannot hide. Rows of 0, 1, 2 and 7
    entries; with two relation blocks (a shared single block row, an unreferenced block row) against the host-expanded design;
    the forced row tile changes nothing."""
    from myfm_amd import _capi

    rng = np.random.default_rng(100 * N + K)
    D0 = 12
    X = _rows(rng, N, D0, INTS)
    blocks = _two_blocks(rng, N, INTS)
    Xe = _expanded(X, blocks)
    for design_args, Xref, D in (((X,), X, D0), ((X, blocks), Xe, Xe.shape[1]), ((Xe,), Xe, Xe.shape[1])):
        model = vr.exact_model(np.random.default_rng(K + 1), D, K)
        mo = vr.closed_form(Xref, model, extra_var=0.5)
        rmean, rvar = _f64(mo.mean), _f64(mo.var)
        d = _capi.Design(*design_args)
        mean, std = d.moments_vb(model, extra_var=0.5)
        assert mean.shape == (N,) and std.shape == (N,)
        assert np.array_equal(mean, rmean), np.flatnonzero(mean != rmean)[:8]
        assert np.array_equal(std, np.sqrt(rvar)), np.flatnonzero(std != np.sqrt(rvar))[:8]
        mean64, std64, prob64 = d.moments_vb(model, extra_var=0.5, want_prob=True, tile_rows=64)
        assert np.array_equal(mean64, mean) and np.array_equal(std64, std)
        assert np.array_equal(prob64, d.moments_vb(model, extra_var=0.5, want_prob=True)[2])
        again = d.moments_vb(model, extra_var=0.5)
        assert np.array_equal(again[0], mean) and np.array_equal(again[1], std)  # (no atomics: a rerun is bit-identical)
        d.close()


# ---- 2. rows, real values ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 33])
def real_rows(request):
    K = request.param
    rng = np.random.default_rng(7 + K)
    N, D = 130, 40
    X = _rows(rng, N, D, [-1.5, -0.7, 0.3, 1.0, 2.5], lens=(3, 1, 0, 7, 2, 12))
    model = vr.normal_model(rng, D, K)
    return K, X, model, vr.closed_form(X, model), vr.closed_form(X, model, extra_var=0.37)


def _check_var(std, mo):
    b2, _ = vr.std_bounds(mo)
    err = np.abs(std * std - np.asarray(mo.var, dtype=np.float64))
    use = float((err / np.maximum(b2, 1e-300)).max())
    print("std^2 against the reference: %.3g of the bound (n + 8) eps scale + 2 eps var" % use)
    assert np.all(err <= b2), use
    assert np.all(std >= 0.0)


def test_rows_real_valued(real_rows):
    """multi-hot rows with non-unit values: |std^2 - var_ref| <= (n + 8) eps scale + 2 eps var_ref with n and scale from the
    reference; the mean is predict()'s score bit for bit; a single-entry row has std == sqrt(w0_var + x^2 wv) exactly; a model
    with all variances 0 has std == 0.0 exactly"""
    from myfm_amd import _capi

    K, X, model, mo, _ = real_rows
    w0, w0v, w, wv, V, Vv = model
    d = _capi.Design(X)
    mean, std = d.moments_vb(model)
    assert np.array_equal(mean, d.predict([(w0, w, V)], mode=0))
    _check_var(std, mo)
    assert float(np.asarray(mo.var, dtype=np.float64).min()) > 0 and float(std.max()) > 1e-2
    single = np.flatnonzero(np.diff(X.indptr) == 1)
    assert single.size > 10
    x, j = X.data[X.indptr[single]], X.indices[X.indptr[single]]
    assert np.array_equal(std[single], np.sqrt(w0v + (x * x) * wv[j]))
    empty = np.flatnonzero(np.diff(X.indptr) == 0)
    assert np.array_equal(std[empty], np.full(empty.size, np.sqrt(w0v))) and np.all(mean[empty] == w0)
    zmean, zstd = d.moments_vb((w0, 0.0, w, np.zeros_like(wv), V, np.zeros_like(Vv)))
    assert np.array_equal(zmean, mean) and np.all(zstd == 0.0) and not np.any(np.signbit(zstd))
    d.close()


def test_rows_real_valued_with_blocks():
    """relation blocks against the host-expanded design within the bound, both against the reference"""
    from myfm_amd import _capi

    rng = np.random.default_rng(17)
    N, K = 130, 8
    vals = [-1.5, -0.7, 0.3, 1.0, 2.5]
    X = _rows(rng, N, 20, vals, lens=(3, 1, 0, 7))
    blocks = _two_blocks(rng, N, vals)
    Xe = _expanded(X, blocks)
    model = vr.normal_model(rng, Xe.shape[1], K)
    mo = vr.closed_form(Xe, model, n_parts=3)
    blocked, flat = _capi.Design(X, blocks), _capi.Design(Xe)
    (mb, sb), (mf, sf) = blocked.moments_vb(model), flat.moments_vb(model)
    _check_var(sb, mo)
    _check_var(sf, mo)
    assert np.all(np.abs(mb - np.asarray(mo.mean, dtype=np.float64)) <= vr.mean_bound(mo))
    assert np.array_equal(mf, flat.predict([(model[0], model[2], model[4])], mode=0))
    assert np.all(np.abs(sb * sb - sf * sf) <= 2 * vr.std_bounds(mo)[0])
    blocked.close()
    flat.close()


def test_noise_adds_extra_var(real_rows):
    """extra_var is added under the square root: against the reference evaluated with it"""
    from myfm_amd import _capi

    K, X, model, mo, mo_noise = real_rows
    d = _capi.Design(X)
    mean, std = d.moments_vb(model, extra_var=0.37)
    assert np.array_equal(mean, d.moments_vb(model)[0])
    _check_var(std, mo_noise)
    assert np.all(std * std > 0.37 - 1e-12)
    d.close()


def test_proba_marginal(real_rows):
    """Phi(mean / sqrt(1 + Var)) against scipy's ndtr of the reference moments. Bound: Phi is 0.4-Lipschitz and is rounded itself
    (test_gpu_pairs.mode_bound's mode 1, taken for the mean by scoring the rows as pairs with one empty candidate), and
    z = m / sqrt(1 + v) moves by at most dm / sqrt(1 + v) + |m| dv / (2 (1 + v)^1.5) <= dm + |m| dv / 2."""
    from myfm_amd import _capi

    K, X, model, mo, _ = real_rows
    d = _capi.Design(X)
    mean, std, prob = d.moments_vb(model, want_prob=True)
    m, v = np.asarray(mo.mean, dtype=np.float64), np.asarray(mo.var, dtype=np.float64)
    ref = special.ndtr(m / np.sqrt(1.0 + v))
    none = sps.csr_matrix((1, X.shape[1]))
    b = mode_bound([(model[0], model[2], model[4])], X, none, 1)[:, 0] + 0.4 * np.abs(m) * vr.var_bound(mo) / 2
    use = float((np.abs(prob - ref) / b).max())
    print("predict_proba_marginal: %.3g of the bound" % use)
    assert use <= 1.0
    assert np.abs(prob - special.ndtr(m)).max() > 1e-3  # (it is not the mean model's Phi(mean))
    d.close()


# ---- 3. consistency with training -------------------------------------------------------------------------------------------------
def test_variance_sum_is_the_trainers():
    """mfm_vb_update_e's variance-sum slot (update_e_and_var of the reference's trainer, with N w0_var) equals the sum over the same
    train rows of std^2, within the summed per-row bounds of both kernels plus the sums' own rounding"""
    from myfm_amd import _capi
    from tests.test_gpu_variational import _VB

    rng = np.random.default_rng(4)
    N, D, K = 300, 30, 5
    X = _rows(rng, N, D, [-1.5, -0.7, 0.3, 1.0, 2.5], lens=(3, 1, 4, 7))
    model = vr.normal_model(rng, D, K)
    vb = _VB(X, rng.normal(size=N), np.zeros(D, dtype=np.int32), K)
    vb.set_state(*model)
    trainer = vb.update_e(0)[2]
    d = _capi.Design(X)
    _, std = d.moments_vb(model)
    d.close()
    mo = vr.closed_form(X, model)
    total = float((std * std).sum())
    bound = 2 * float(vr.std_bounds(mo)[0].sum()) + 2 * N * vr.EPS * total
    print("trainer %.17g, sum of std^2 %.17g, reference %.17g, bound %.3g" % (trainer, total, float(mo.var.sum()), bound))
    assert abs(trainer - total) <= bound
    assert abs(total - float(mo.var.sum())) <= bound


# ---- 4. pairs, exact layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 3, 4, 33])
@pytest.mark.parametrize("I", [5, 16, 250])
@pytest.mark.parametrize("U", [1, 17, 37])
def test_pairs_exact_layout(U, I, K):
    """the grid of test_gpu_pairs_ucb.test_exact_layout on exact data: the dense mean is mfm_pairs_scores' bit for bit, the variance
    the dense-row reference's exactly, and the lists for beta in {-1, 0, 2}, k in {1, 10, I + 3} are the reference's, tail included;
    duplicated candidate rows tie and resolve by ascending index"""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 * U + 10 * I + K)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 9, 11, INTS, mean_nnz=2.0, empty_every=5)
    Xc = sps.csr_matrix(Xc).tolil()
    for a, b in ((1, 3), (2, I - 1)):  # planted ties
        Xc[b] = Xc[a]
    Xc = Xc.tocsr()
    model = vr.exact_model(rng, D, K)
    mo = vr.pairs_closed_form(Xq, Xc, model)
    rmean, rvar = _f64(mo.mean), _f64(mo.var)
    rstd = np.sqrt(rvar)
    P = _capi.Pairs(Xq, Xc)
    mean, std = P.moments_vb(model)
    assert mean.shape == (U, I) and std.shape == (U, I)
    assert np.array_equal(mean, P.scores([(model[0], model[2], model[4])], mode=0))
    assert np.array_equal(mean, rmean), np.argwhere(mean != rmean)[:8]
    assert np.array_equal(std, rstd), np.argwhere(std != rstd)[:8]
    for beta in (-1.0, 0.0, 2.0):
        ref = rmean + beta * rstd
        for k in (1, 10, I + 3):
            idx, val, m, s = P.topk_bound_vb(model, k, beta)
            ridx, rval = pr.topk(ref, k)
            assert np.array_equal(idx, ridx) and np.array_equal(val, rval), (beta, k)
            assert np.array_equal(m, ur.at(rmean, ridx), equal_nan=True) and np.array_equal(s, ur.at(rstd, ridx), equal_nan=True), (beta, k)
            if k == I + 3:
                assert np.all(idx[:, I:] == -1) and np.all(val[:, I:] == -np.inf) and np.all(np.isnan(m[:, I:])) and np.all(np.isnan(s[:, I:]))
                for u in range(U):  # the planted ties keep their index order
                    pos = {int(c): j for j, c in enumerate(idx[u, :I])}
                    assert pos[1] < pos[3] and pos[2] < pos[I - 1]
    P.close()


# ---- 5. pairs, real values -------------------------------------------------------------------------------------------------------
def _pair_bounds(mo):
    return vr.mean_bound(mo), vr.std_bounds(mo)[1]


@pytest.mark.parametrize("K", [8, 33])
def test_pairs_real_valued(K):
    """normal posterior, multi-hot sides, 1100 candidates (a stripe longer than one workgroup step), 5 % of the pairs and one whole
    query row excluded; k up to 256. Bounds from the reference's scale: mean (n + 8) eps mean_scale, std from the variance's."""
    from myfm_amd import _capi

    rng = np.random.default_rng(31 + K)
    U, I = 37, 1100
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, HALVES, mean_nnz=3.0)
    model = vr.normal_model(rng, D, K)
    mo = vr.pairs_closed_form(Xq, Xc, model)
    rstd = np.sqrt(np.maximum(mo.var, 0))
    b_mean, b_std = _pair_bounds(mo)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="lil")
    ex[5] = np.ones(I)
    ex = ex.tocsr()
    P = _capi.Pairs(Xq, Xc, exclude=ex)
    mean, std = P.moments_vb(model)
    assert np.array_equal(mean, P.scores([(model[0], model[2], model[4])], mode=0))
    use_mean = float((np.abs(mean - np.asarray(mo.mean, dtype=np.float64)) / b_mean).max())
    use_std = float((np.abs(std - np.asarray(rstd, dtype=np.float64)) / b_std).max())
    print("K %d: dense mean %.3g, dense std %.3g of the tolerance" % (K, use_mean, use_std))
    assert use_mean <= 1.0 and use_std <= 1.0
    assert float(std.min()) > 1e-2
    worst = np.zeros(4)
    for beta in (1.0, -0.5):
        for k in (10, 100, 256):
            got = P.topk_bound_vb(model, k, beta)
            assert np.all(got[0][5] == -1) and np.all(got[1][5] == -np.inf) and np.all(np.isnan(got[2][5]))
            worst = np.maximum(worst, check_ranked(got, k, beta, mo.mean, rstd, b_mean, b_std, ex))
    print("   ranked: value %.3g, mean %.3g, std %.3g, value - (mean + beta std) %.3g of the tolerance" % tuple(worst))
    P.close()


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_pairs_query_chunks_give_identical_output():
    """a scratch bound of one byte leaves one 64-row tile per chunk: 150 queries take three chunks, the default bound one"""
    from myfm_amd import _capi

    rng = np.random.default_rng(9)
    U, I, K = 150, 300, 8
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 30, 50, HALVES, mean_nnz=3.0)
    model = vr.normal_model(rng, D, K)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(1), format="csr")
    one, many = _capi.Pairs(Xq, Xc, exclude=ex), _capi.Pairs(Xq, Xc, exclude=ex, scratch_bound=1)
    assert _same(one.moments_vb(model), many.moments_vb(model))
    for k, beta in ((10, 1.0), (100, -0.5), (256, 1.0)):
        assert _same(one.topk_bound_vb(model, k, beta), many.topk_bound_vb(model, k, beta)), k
    mo = vr.pairs_closed_form(Xq, Xc, model)
    check_ranked(many.topk_bound_vb(model, 10, 1.0), 10, 1.0, mo.mean, np.sqrt(np.maximum(mo.var, 0)), *_pair_bounds(mo), ex)
    one.close()
    many.close()


def test_pairs_relation_block_sides():
    """two blocks per side ([ub, None] / [None, ib] positions) against the sides expanded on the host and against the reference"""
    from myfm_amd import _capi

    rng = np.random.default_rng(23)
    sd = rr.block_sides(rng, 37, 250, 9, 11, 2, 2, mean_nnz=2.0)
    Fq, Fc = rr.flat_sides(sd)
    Xq, Xc, rq, rc = rr.capi_args(sd)
    model = vr.normal_model(rng, sd["D"], 8)
    mo = vr.pairs_closed_form(Fq, Fc, model, n_parts=6)
    rmean, rstd = np.asarray(mo.mean, dtype=np.float64), np.asarray(np.sqrt(np.maximum(mo.var, 0)), dtype=np.float64)
    b_mean, b_std = _pair_bounds(mo)
    ex = sps.random(37, 250, density=0.05, random_state=np.random.RandomState(3), format="csr")
    blocked, flat = _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, exclude=ex), _capi.Pairs(Fq, Fc, exclude=ex)
    (ma, sa), (mb, sb) = blocked.moments_vb(model), flat.moments_vb(model)
    for m, s in ((ma, sa), (mb, sb)):
        assert np.all(np.abs(m - rmean) <= b_mean) and np.all(np.abs(s - rstd) <= b_std)
    assert np.all(np.abs(ma - mb) <= b_mean) and np.all(np.abs(sa - sb) <= b_std)
    assert np.array_equal(ma, blocked.scores([(model[0], model[2], model[4])], mode=0))
    for P in (blocked, flat):
        check_ranked(P.topk_bound_vb(model, 10, 1.0), 10, 1.0, mo.mean, np.sqrt(np.maximum(mo.var, 0)), b_mean, b_std, ex)
    blocked.close()
    flat.close()


# ---- 6. the estimator boundary ---------------------------------------------------------------------------------------------------
def _model_of(est):
    return (est.w0_mean, est.w0_var, np.asarray(est.w_mean), np.asarray(est.w_var), np.asarray(est.V_mean), np.asarray(est.V_var))


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_estimator_boundary(kind, table):  # noqa: F811
    """both estimators, fitted for 5 iterations: the four methods against the reference evaluated on the fitted posterior, identical
    arrays after a pickle round trip, and bad arguments refused on the host"""
    import myfm_amd

    X, y, shapes, Xq, Xc, Xpairs, seen = table
    if kind == "regressor":
        est = myfm_amd.VariationalFMRegressor(rank=8, random_seed=3).fit(X, y, n_iter=5, group_shapes=shapes)
    else:
        est = myfm_amd.VariationalFMClassifier(rank=8, random_seed=3).fit(X, y > np.median(y), n_iter=5, group_shapes=shapes)
    model = _model_of(est)
    rows = X[:200]
    mo = vr.closed_form(rows, model)

    def call_all(e):
        out = [e.predict_moments(rows), e.predict_pairs_moments(Xq, Xc), e.predict_topk_bound(Xq, Xc, 10, beta=1.5, exclude=seen)]
        out.append((e.predict_moments(rows, noise=True),) if kind == "regressor" else (e.predict_proba_marginal(rows),))
        return [np.asarray(a) for r in out for a in r]

    got = call_all(est)
    rm = est.predict_moments(rows)
    assert type(rm).__name__ == "ScoreMoments" and rm.mean.shape == (200,) and rm.std.shape == (200,)
    _check_var(rm.std, mo)
    if kind == "regressor":
        assert np.array_equal(rm.mean, est.predict(rows))
        assert np.array_equal(est.predict_pairs_moments(Xq, Xc).mean, est.predict_pairs(Xq, Xc))
        alpha = est.history_.hypers.alpha
        _check_var(est.predict_moments(rows, noise=True).std, vr.closed_form(rows, model, extra_var=1.0 / alpha))
    else:
        assert np.array_equal(special.ndtr(rm.mean) > 0.5, est.predict(rows))
        p = est.predict_proba_marginal(rows)
        m, v = np.asarray(mo.mean, dtype=np.float64), np.asarray(mo.var, dtype=np.float64)
        assert p.shape == (200,) and np.abs(p - special.ndtr(m / np.sqrt(1 + v))).max() < 1e-9
        with pytest.raises(ValueError, match="not available on a classifier"):
            est.predict_moments(rows, noise=True)
    pm = vr.pairs_closed_form(Xq, Xc, model)
    b_mean, b_std = _pair_bounds(pm)
    ps = est.predict_pairs_moments(Xq, Xc)
    assert type(ps).__name__ == "PairSummary" and ps.mean.shape == (N_USERS, N_ITEMS)
    rstd = np.sqrt(np.maximum(pm.var, 0))
    assert np.all(np.abs(ps.mean - np.asarray(pm.mean, dtype=np.float64)) <= b_mean)
    assert np.all(np.abs(ps.std - np.asarray(rstd, dtype=np.float64)) <= b_std) and float(ps.std.min()) > 0
    r = est.predict_topk_bound(Xq, Xc, 10, beta=1.5, exclude=seen)
    assert type(r).__name__ == "RankedSummary" and r.indices.dtype == np.int64
    check_ranked(tuple(r), 10, 1.5, pm.mean, rstd, b_mean, b_std, seen)
    again = call_all(pickle.loads(pickle.dumps(est)))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))
    # bad arguments: ValueError from the host checks
    for bad_k in (0, 257, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            est.predict_topk_bound(Xq, Xc, bad_k)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="beta must be a finite"):
            est.predict_topk_bound(Xq, Xc, 3, beta=bad)
    with pytest.raises(ValueError, match="share column"):
        est.predict_pairs_moments(Xq, Xq)
    with pytest.raises(ValueError, match="share column"):
        est.predict_topk_bound(Xq, Xq, 3)
    with pytest.raises(ValueError, match="exclude must have shape"):
        est.predict_topk_bound(Xq, Xc, 3, exclude=seen[:, :5])
    with pytest.raises(ValueError, match="this->feature_size"):
        est.predict_moments(rows[:, :10])


# ---- 7. errors of the C entry points ---------------------------------------------------------------------------------------------
def test_capi_errors():
    from myfm_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(2)
    Xq, Xc, D = pr.disjoint_sides(rng, 5, 20, 9, 11, HALVES)
    K = 4
    model = vr.normal_model(rng, D, K)
    K_, head, keep = _capi._pack_vb_model(model)
    out = [np.empty(5 * 20) for _ in range(3)]
    idx = np.empty(5 * 3, dtype=np.int64)
    p = [a.ctypes.data_as(C.c_void_p) for a in out]
    d, P = _capi.Design(Xq), _capi.Pairs(Xq, Xc)
    INV = _capi.MFM_ERR_INVALID
    # null outputs
    assert L.mfm_design_moments_vb(d.h, K, *head, 0.0, 0, 0, None, p[1], None) == INV and b"no output" in L.mfm_design_last_error(d.h)
    assert L.mfm_design_moments_vb(d.h, K, *head, 0.0, 1, 0, p[0], p[1], None) == INV and b"no output" in L.mfm_design_last_error(d.h)
    assert L.mfm_pairs_moments_vb(P.h, K, *head, 0.0, p[0], None) == INV and b"no output" in L.mfm_pairs_last_error(P.h)
    assert L.mfm_pairs_topk_bound_vb(P.h, K, *head, 0.0, 3, 1.0, idx.ctypes.data_as(C.c_void_p), p[0], p[1], None) == INV
    assert b"no output" in L.mfm_pairs_last_error(P.h)
    # negative rank, bad variances, bad tiling
    assert L.mfm_design_moments_vb(d.h, -1, *head, 0.0, 0, 0, p[0], p[1], None) == INV and b"rank" in L.mfm_design_last_error(d.h)
    assert L.mfm_pairs_moments_vb(P.h, -1, *head, 0.0, p[0], p[1]) == INV and b"rank" in L.mfm_pairs_last_error(P.h)
    assert L.mfm_pairs_topk_bound_vb(P.h, -1, *head, 0.0, 3, 1.0, idx.ctypes.data_as(C.c_void_p), p[0], p[1], p[2]) == INV
    assert L.mfm_design_moments_vb(d.h, K, *head, -1.0, 0, 0, p[0], p[1], None) == INV and b"extra_var" in L.mfm_design_last_error(d.h)
    assert L.mfm_design_moments_vb(d.h, K, *head, 0.0, 0, -5, p[0], p[1], None) == INV and b"tiling" in L.mfm_design_last_error(d.h)
    # no handle
    assert L.mfm_design_moments_vb(None, K, *head, 0.0, 0, 0, p[0], p[1], None) == INV and b"no design" in L.mfm_design_last_error(None)
    assert L.mfm_pairs_moments_vb(None, K, *head, 0.0, p[0], p[1]) == INV and b"no pair design" in L.mfm_pairs_last_error(None)
    assert L.mfm_pairs_topk_bound_vb(None, K, *head, 0.0, 3, 1.0, idx.ctypes.data_as(C.c_void_p), p[0], p[1], p[2]) == INV
    # through the wrappers: k and beta
    for bad in (0, 257):
        with pytest.raises(ValueError, match="k must be"):
            P.topk_bound_vb(model, bad, 1.0)
    for bad in (np.inf, np.nan):
        with pytest.raises(ValueError, match="beta must be a finite"):
            P.topk_bound_vb(model, 3, bad)
    # and the handles still work
    mean, std = P.moments_vb(model)
    assert np.array_equal(mean, P.scores([(model[0], model[2], model[4])], mode=0)) and np.all(std > 0)
    d.close()
    P.close()
