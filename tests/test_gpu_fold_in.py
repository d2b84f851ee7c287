"""Fold-in of new one-hot entities on the device: the kernel against the longdouble reference of
tests/fold_in_ref.py at every rank shape, row count and chunking, posterior draws against the per-row Philox stream, the
invariance of a result under everything but the entity's own rows, and MyFMGibbsRegressor.fold_in end to end.

The tolerance of cases 1 and 2, per (sample, entity), against the longdouble reference:
    |theta - theta_ref|_inf <= 16 (K + 1 + n_u) 2^-52 cond_2(Lambda_ref) max(|theta_ref|_inf, |mu|_inf)
(fold_in_ref.tolerance; tests/test_fold_in_cpu.py holds the float64 NumPy restatement to the same bound, where it reaches 0.04 of it).
On one MI355X the kernel's largest error / bound was 0.078 for the means and 0.34 for the draws, both at rank 0."""
import functools
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import fold_in_ref as fr

pytestmark = pytest.mark.gpu

D = 40
RANKS = [0, 1, 3, 4, 15, 16, 17, 31, 33, 63, 64]
SHAPES = [(U, S) for U in (1, 5, 70) for S in (1, 2, 7)]
SEEDS = (5, 0x9E3779B97F4A7C15)


@functools.lru_cache(maxsize=1)
def _cases(K, fit_linear):
    """the problems of one (rank, fit_linear) over every (U, S), each with its longdouble reference: computed once, shared by the
    mean and the draw test (which run next to each other)"""
    out = []
    for U, S in SHAPES:
        p = fr.problem(np.random.default_rng(10000 * K + 100 * U + 2 * S + fit_linear), D, K, S, U)
        out.append((p, fr.posterior(p, fit_linear)))
    return out


def _solve(p, fit_linear, draw=False, seed=0, scratch_bound=None):
    from myfm_amd import _capi

    h = _capi.FoldIn(p["X"], p["y"], p["entity"], p["U"], fit_linear, scratch_bound=scratch_bound)
    try:
        return h.solve(p["samples"], p["alpha"], p["mu"], p["lam"], draw=draw, seed=seed)
    finally:
        h.close()


def _check_shapes(p, w, V, fit_linear):
    assert w.shape == (p["S"], p["U"]) and V.shape == (p["S"], p["U"], p["K"])
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V))
    if not fit_linear:
        assert not w.any()  # exactly 0


# ---- 1., 2. the kernel against the longdouble reference, means and draws ---------------------------------------------------------
@pytest.mark.parametrize("draw", [False, True])
@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("K", RANKS)
def test_kernel_matches_longdouble_reference(K, fit_linear, draw):
    """U in {1, 5, 70} x S in {1, 2, 7}; rows per entity from {0, 1, 2, 63, 64, 65, 257} (one pass, the pass edge, several passes);
    context rows empty, one-hot and multi-hot with values {0.5, 1, 2}; shuffled entity; empty entities at the front, in the middle
    and at the end. draw: theta_mean + L^-T eps with the reference's L and the normals of tests/philox_ref.py, two seeds."""
    worst = 0.0
    for p, ref in _cases(K, fit_linear):
        M = ref["theta"].shape[-1]
        empty = p["counts"] == 0
        if M:
            assert ref["cond"].max() <= 1e5  # (stayed below 5e3 on the CPU: the tolerance cannot go slack)
        for seed in (SEEDS if draw else (0,)):
            w, V = _solve(p, fit_linear, draw=draw, seed=seed)
            _check_shapes(p, w, V, fit_linear)
            if M == 0:
                continue
            got = fr.join(w, V, fit_linear)
            want = fr.drawn(ref, fr.normals(seed, p["S"], p["U"], M)) if draw else ref["theta"]
            tol = fr.tolerance(ref, K, want)
            err = np.abs(got - want).max(axis=-1).astype(np.float64)
            ratio = float((err / tol).max())
            worst = max(worst, ratio)
            assert np.all(err <= tol), (p["U"], p["S"], seed, ratio, np.unravel_index(np.argmax(err / tol), err.shape))
            if not draw and empty.any():  # the prior, bit for bit
                assert np.array_equal(got[:, empty], np.broadcast_to(ref["mu"][:, None, :].astype(np.float64), got[:, empty].shape))
    print("fold-in K=%d fit_linear=%d draw=%d: largest error / bound = %.4f" % (K, fit_linear, draw, worst))


def test_draw_stream_is_keyed_by_s_U_plus_u():
    """the same observations as entity 3 of 5 and as entity 1 of 7: under sample 1 both read stream row 8 = 1 * 5 + 3 = 1 * 7 + 1 and
    give the same bits; under sample 0 the rows are 3 and 1 and the draws differ. The posterior means agree under both."""
    rng = np.random.default_rng(77)
    base = fr.problem(rng, D, 6, 2, 1, counts=[70])

    def placed(U, u):
        q = dict(base)
        q.update(U=U, entity=np.full(70, u, dtype=np.int64), counts=np.bincount([u] * 70, minlength=U))
        return q

    a, b = placed(5, 3), placed(7, 1)
    (wa, Va), (wb, Vb) = _solve(a, True, draw=True, seed=9), _solve(b, True, draw=True, seed=9)
    assert wa[1, 3] == wb[1, 1] and np.array_equal(Va[1, 3], Vb[1, 1])
    assert wa[0, 3] != wb[0, 1] and not np.array_equal(Va[0, 3], Vb[0, 1])
    (ma, MVa), (mb, MVb) = _solve(a, True), _solve(b, True)
    assert np.array_equal(ma[:, 3], mb[:, 1]) and np.array_equal(MVa[:, 3], MVb[:, 1])
    # against the reference, the streams recomputed for each U
    for q, u, w, V in ((a, 3, wa, Va), (b, 1, wb, Vb)):
        ref = fr.posterior(q, True)
        want = fr.drawn(ref, fr.normals(9, 2, q["U"], 7))
        err = np.abs(fr.join(w, V, True) - want).max(axis=-1).astype(np.float64)
        assert np.all(err <= fr.tolerance(ref, 6, want))


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,fit_linear", [(17, True), (4, False), (0, True)])
def test_result_depends_on_the_entity_alone(K, fit_linear):
    """an entity computed alone, among 70 others, and under scratch bounds that force several chunks of entities and of samples:
    identical bits. A store-resident model and the same samples as host arrays: identical bits, for a sub-range of the store too."""
    from myfm_amd import _capi

    S, U, me = 7, 71, 37
    p = fr.problem(np.random.default_rng(31 + K), D, K, S, U)
    p["counts"][me] = 129  # (three passes; the generator may have drawn fewer)
    p = fr.problem(np.random.default_rng(31 + K), D, K, S, U, counts=p["counts"])
    w, V = _solve(p, fit_linear)
    mine = p["entity"] == me
    alone = dict(p)
    alone.update(U=1, X=p["X"][mine], y=p["y"][mine], entity=np.zeros(int(mine.sum()), dtype=np.int64), counts=np.array([129]))
    w1, V1 = _solve(alone, fit_linear)
    assert np.array_equal(w1[:, 0], w[:, me]) and np.array_equal(V1[:, 0], V[:, me])
    cell = (K + 1) * 8
    for bound in (1, 3 * cell, 20 * cell, 7 * 30 * cell + 5):  # one (entity, sample); 3 samples; 2 entities; 30 entities
        for draw in (False, True):
            wd, Vd = (w, V) if not draw else _solve(p, fit_linear, draw=True, seed=4)
            wc, Vc = _solve(p, fit_linear, draw=draw, seed=4, scratch_bound=bound)
            assert np.array_equal(wc, wd) and np.array_equal(Vc, Vd), (bound, draw)
    # the store
    st = _capi.Store(D, K)
    h = _capi.FoldIn(p["X"], p["y"], p["entity"], U, fit_linear, scratch_bound=50 * cell)
    try:
        for w0, ws, Vs in p["samples"]:
            st.push(w0, ws, Vs)
        ws_, Vs_ = h.solve_store(st, p["alpha"], p["mu"], p["lam"])
        assert np.array_equal(ws_, w) and np.array_equal(Vs_, V)
        wr, Vr = h.solve_store(st, p["alpha"][2:5], p["mu"][2:5], p["lam"][2:5], first=2, count=3)
        assert np.array_equal(wr, w[2:5]) and np.array_equal(Vr, V[2:5])
        wd, Vd = h.solve_store(st, p["alpha"], p["mu"], p["lam"], draw=True, seed=4)
        wh, Vh = h.solve(p["samples"], p["alpha"], p["mu"], p["lam"], draw=True, seed=4)
        assert np.array_equal(wd, wh) and np.array_equal(Vd, Vh)
    finally:
        h.close()
        st.close()


def test_bad_precisions_and_models_are_errors_not_nans():
    from myfm_amd import _capi

    p = fr.problem(np.random.default_rng(2), D, 3, 2, 4, counts=[0, 5, 70, 1])
    for name, bad in (("lam", -1.0), ("lam", 0.0), ("lam", np.nan), ("lam", np.inf), ("alpha", -2.0), ("alpha", np.nan), ("mu", np.inf)):
        q = dict(p)
        q[name] = p[name].copy()
        q[name][(1,) if name == "alpha" else (1, 2)] = bad
        with pytest.raises(ValueError, match="not positive and finite|not finite"):
            _solve(q, True)
    # component 0 is not read without the linear term
    q = dict(p)
    q["lam"] = p["lam"].copy()
    q["lam"][:, 0] = -1.0
    _solve(q, False)
    # a model value that is not finite makes the pivot test fail on the device: an error through the handle
    q = dict(p)
    w0, w, V = p["samples"][1]
    V = V.copy()
    V[:, 1] = np.nan
    q["samples"] = [p["samples"][0], (w0, w, V)]
    with pytest.raises(ValueError, match="not positive definite"):
        _solve(q, True)
    big = fr.problem(np.random.default_rng(3), 5, 65, 1, 1, counts=[2])
    with pytest.raises(ValueError, match="ranks up to 64"):
        _solve(big, True)
    assert _capi.lib().mfm_foldin_max_rank() == 64


# ---- 4., 5. the estimator ----------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS, OLD_USERS, OLD_ITEMS, RANK = 200, 100, 160, 95, 4


def _rows(cols_a, cols_b, width):
    """one-hot pairs: row t stores columns cols_a[t] and cols_b[t]"""
    n = len(cols_a)
    idx = np.empty(2 * n, dtype=np.int32)
    idx[0::2], idx[1::2] = cols_a, cols_b
    X = sps.csr_matrix((np.ones(2 * n), idx, np.arange(0, 2 * n + 1, 2, dtype=np.int64)), shape=(n, width))
    X.sort_indices()
    return X


def _onehot(cols, width):
    n = len(cols)
    return sps.csr_matrix((np.ones(n), np.asarray(cols, dtype=np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, width))


def _host_mean(est, X):
    w0, w, V = est.w0_samples, est.w_samples, est.V_samples
    return fr.mean_score([(w0[s], w[s], V[s]) for s in range(w0.shape[0])], X)


@pytest.fixture(scope="module")
def fitted():
    """200 users x 100 items, about a third of the pairs rated; the model is fitted on users [0, 160) x items [0, 95); the last 40
    users and the last 5 items are new"""
    from myfm_amd import MyFMGibbsRegressor

    rng = np.random.default_rng(12)
    bu, bi = rng.normal(size=N_USERS) * 0.5, rng.normal(size=N_ITEMS) * 0.5
    P, Q = rng.normal(size=(N_USERS, 3)) * 0.7, rng.normal(size=(N_ITEMS, 3)) * 0.7
    u, i = np.nonzero(rng.random((N_USERS, N_ITEMS)) < 0.33)
    y = 3.0 + bu[u] + bi[i] + (P[u] * Q[i]).sum(axis=1) + rng.normal(size=u.shape[0]) * 0.3
    old = (u < OLD_USERS) & (i < OLD_ITEMS)
    Dm = OLD_USERS + OLD_ITEMS
    fm = MyFMGibbsRegressor(RANK, random_seed=3)
    fm.fit(_rows(u[old], OLD_USERS + i[old], Dm), y[old], n_iter=60, n_kept_samples=40, group_shapes=[OLD_USERS, OLD_ITEMS])
    # the new users' ratings of old items, halved at random
    nu = (u >= OLD_USERS) & (i < OLD_ITEMS)
    half = rng.random(int(nu.sum())) < 0.5
    seen = dict(u=u[nu][half] - OLD_USERS, i=i[nu][half], y=y[nu][half])
    rest = dict(u=u[nu][~half] - OLD_USERS, i=i[nu][~half], y=y[nu][~half])
    ni = i >= OLD_ITEMS  # the new items' ratings, by old and new users
    items = dict(u=u[ni], i=i[ni] - OLD_ITEMS, y=y[ni])
    return dict(fm=fm, D=Dm, seen=seen, rest=rest, items=items)


def _fold_users(f, n_entities=N_USERS - OLD_USERS, **kw):
    s = f["seen"]
    return f["fm"].fold_in(_onehot(OLD_USERS + s["i"], f["D"]), s["y"], s["u"], 0, n_entities=n_entities, **kw)


def test_estimator_fold_in(fitted):
    from myfm_amd import MyFMGibbsRegressor

    fm, Dm, seen = fitted["fm"], fitted["D"], fitted["seen"]
    U = N_USERS - OLD_USERS + 1  # one more entity than there are new users: the last has no rows
    X_old = _rows(np.arange(50) % OLD_USERS, OLD_USERS + np.arange(50) % OLD_ITEMS, Dm)
    before = fm.predict(X_old)
    fm2 = _fold_users(fitted, n_entities=U)
    assert isinstance(fm2, MyFMGibbsRegressor) and fm2 is not fm and fm2.fold_in_columns_ == (Dm, Dm + U)
    assert fm2.predictor_.feature_size == Dm + U and fm.predictor_.feature_size == Dm and not hasattr(fm, "fold_in_columns_")
    assert fm2.history_ is fm.history_ and fm2.n_groups_ == 2 and fm2.rank == RANK and fm2.random_seed == 3
    assert fm2.w_samples.shape == (40, Dm + U) and fm2.V_samples.shape == (40, Dm + U, RANK)
    # the receiver: untouched, bit for bit; the old columns of the result: the receiver's
    assert np.array_equal(fm.predict(X_old), before)
    assert np.array_equal(fm2.w_samples[:, :Dm], fm.w_samples) and np.array_equal(fm2.V_samples[:, :Dm], fm.V_samples)
    wide = sps.csr_matrix((X_old.data, X_old.indices, X_old.indptr), shape=(50, Dm + U))
    assert np.array_equal(fm2.predict(wide), before)
    # the new columns against the longdouble reference under the hyper-parameters of the users' group
    kept = fm.history_.hypers[-40:]
    p = dict(D=Dm, K=RANK, S=40, U=U, X=_onehot(OLD_USERS + seen["i"], Dm), y=seen["y"], entity=seen["u"],
             samples=[(fm.w0_samples[s], fm.w_samples[s], fm.V_samples[s]) for s in range(40)],
             alpha=np.array([h.alpha for h in kept]), counts=np.bincount(seen["u"], minlength=U),
             mu=np.array([np.append(h.mu_w[0], h.mu_V[0]) for h in kept]), lam=np.array([np.append(h.lambda_w[0], h.lambda_V[0]) for h in kept]))
    ref = fr.posterior(p, True)
    got = fr.join(fm2.w_samples[:, Dm:], fm2.V_samples[:, Dm:], True)
    err = np.abs(got - ref["theta"]).max(axis=-1).astype(np.float64)
    assert np.all(err <= fr.tolerance(ref, RANK))
    # an entity without rows: the prior mean, bit for bit
    assert p["counts"][U - 1] == 0 and np.array_equal(got[:, U - 1], p["mu"])
    # predict on rows that carry column D + u: the host evaluation of the extended samples
    rest = fitted["rest"]
    Xn = _rows(OLD_USERS + rest["i"], Dm + rest["u"], Dm + U)
    pred = fm2.predict(Xn)
    np.testing.assert_allclose(pred, _host_mean(fm2, Xn), rtol=1e-12, atol=1e-12)
    dist = fm2.predict_dist(Xn, quantiles=(0.5,), noise=True)
    assert np.array_equal(dist.mean, pred) and np.all(dist.std > 0)
    # ranking the old items for the new users
    Xq, Xc = _onehot(Dm + np.arange(U), Dm + U), _onehot(OLD_USERS + np.arange(OLD_ITEMS), Dm + U)
    full = np.stack([_host_mean(fm2, _rows(OLD_USERS + np.arange(OLD_ITEMS), np.full(OLD_ITEMS, Dm + uu), Dm + U)) for uu in range(U)])
    np.testing.assert_allclose(fm2.predict_pairs(Xq, Xc), full, rtol=1e-12, atol=1e-12)
    idx, val = fm2.predict_topk(Xq, Xc, 10)
    assert np.array_equal(idx, np.argsort(-full, axis=1, kind="stable")[:, :10])
    np.testing.assert_allclose(val, np.take_along_axis(full, idx, axis=1), rtol=1e-12, atol=1e-12)
    # pickling
    fm2b = pickle.loads(pickle.dumps(fm2))
    assert fm2b.fold_in_columns_ == (Dm, Dm + U) and np.array_equal(fm2b.predict(Xn), pred)
    # a draw differs from the mean, and is reproducible
    d1, d2 = _fold_users(fitted, draw=True, random_seed=8), _fold_users(fitted, draw=True, random_seed=8)
    assert np.array_equal(d1.w_samples, d2.w_samples) and not np.array_equal(d1.w_samples[:, Dm:], fm2.w_samples[:, Dm:Dm + U - 1])


def test_fold_in_composes(fitted):
    """users, then items whose raters are old and new users alike (rows in the first result's feature space)"""
    Dm, it = fitted["D"], fitted["items"]
    U, I = N_USERS - OLD_USERS, N_ITEMS - OLD_ITEMS
    fm2 = _fold_users(fitted)
    ucol = np.where(it["u"] < OLD_USERS, it["u"], Dm + it["u"] - OLD_USERS)
    fm3 = fm2.fold_in(_onehot(ucol, Dm + U), it["y"], it["i"], 1)
    assert fm3.fold_in_columns_ == (Dm + U, Dm + U + I) and fm2.fold_in_columns_ == (Dm, Dm + U)
    assert np.array_equal(fm3.w_samples[:, :Dm + U], fm2.w_samples) and np.array_equal(fm3.V_samples[:, :Dm + U], fm2.V_samples)
    X = _rows(ucol, Dm + U + it["i"], Dm + U + I)
    pred = fm3.predict(X)
    np.testing.assert_allclose(pred, _host_mean(fm3, X), rtol=1e-12, atol=1e-12)
    # the items' posterior saw these very ratings: it fits them far better than the items' prior mean does
    prior = fm2.fold_in(sps.csr_matrix((0, Dm + U)), np.zeros(0), np.zeros(0, dtype=np.int64), 1, n_entities=I)
    rm = lambda e: float(np.sqrt(np.mean((e.predict(X) - it["y"]) ** 2)))  # noqa: E731
    assert rm(fm3) < rm(prior)


def test_fold_in_helps(fitted):
    """40 users held out of the fit, folded in with half of their ratings: the RMSE on their other half is strictly below the RMSE
    of the same rows scored with the prior mean theta = (mu_w, mu_V) -- the fold-in of no observations"""
    fm, Dm, rest = fitted["fm"], fitted["D"], fitted["rest"]
    U = N_USERS - OLD_USERS
    fm2 = _fold_users(fitted)
    prior = fm.fold_in(sps.csr_matrix((0, Dm)), np.zeros(0), np.zeros(0, dtype=np.int64), 0, n_entities=U)
    X = _rows(OLD_USERS + rest["i"], Dm + rest["u"], Dm + U)
    rmse_fold = float(np.sqrt(np.mean((fm2.predict(X) - rest["y"]) ** 2)))
    rmse_prior = float(np.sqrt(np.mean((prior.predict(X) - rest["y"]) ** 2)))
    print("fold-in RMSE %.4f, prior-mean RMSE %.4f on %d held-out ratings" % (rmse_fold, rmse_prior, X.shape[0]))
    assert rmse_fold < rmse_prior
