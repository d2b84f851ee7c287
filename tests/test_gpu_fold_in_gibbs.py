"""Fold-in for the probit estimators on the device: the chain kernel against the longdouble reference of
tests/fold_in_gibbs_ref.py at every rank shape, row count, task and chain length, the invariance of a result under the chunking, the
special values, and MyFMGibbsClassifier.fold_in_gibbs / MyFMOrderedProbit.fold_in_gibbs end to end.

The tolerance, per (sample, entity), against the longdouble chain with the same draws:
    |theta - theta_ref|_inf <= 16 T (M + n_u) 2^-52 cond_2(Lambda_ref) max(|theta_ref|_inf, |mu|_inf),   T = n_burn + n_inner
(fold_in_gibbs_ref.tolerance; tests/test_fold_in_gibbs_cpu.py holds the float64 twin to the same bound, where it reaches 0.045 of
it). A cell whose chain has a margin below 1e-9 (a draw within rounding of a decision of its sampler) is left out; a case asserts
that at most 1 % of its cells are. On one MI355X the largest error / bound was 0.060 for the means and 0.083 for the draws, both at
rank 1 without the linear term, and no cell was left out."""
import functools
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import fold_in_gibbs_ref as gr
from tests import fold_in_ref as fr

pytestmark = pytest.mark.gpu

D = 40
RANKS = [0, 1, 3, 16, 17, 33, 64]
TASKS = [0, 2, 3, 5]  # 0: the classifier; else the classes of ordered probit
# (U, S) and the rows of every entity: ROW_CHOICES in turn, so that 0, 1, 63, 64, 65 and 257 rows (no pass, one row, the edges of the
# setup pass of 64 and a second sweep pass of 256) all occur, with empty entities at the front, in the middle and at the end
SHAPES = [((1, 1), [64]), ((5, 2), [0, 1, 65, 2, 0]), ((9, 3), [0, 257, 63, 64, 0, 65, 1, 2, 0])]
CHAINS = ((0, 1), (1, 1), (2, 3))
MARGIN = 1e-9
assert set(fr.ROW_CHOICES) == set(c for _, cnt in SHAPES for c in cnt)


def _task(n_class):
    return "classifier" if n_class == 0 else "ordered"


def _solve(p, fit_linear, n_burn, n_inner, draw=False, seed=0, scratch_bound=None):
    from myfm_amd import _capi

    h = _capi.FoldIn(p["X"], p["y"], p["entity"], p["U"], fit_linear, scratch_bound=scratch_bound)
    try:
        return h.solve_gibbs(p["samples"], p["mu"], p["lam"], _task(p["n_class"]), p["cut"], n_burn=n_burn, n_inner=n_inner, draw=draw,
                             seed=seed)
    finally:
        h.close()


def _compare(p, r, fit_linear, chains, seed):
    """the device against the views of the run r for every chain length, means and draws: (largest error / bound of the means and
    of the draws, cells, left out)"""
    worst, cells, left = np.zeros(2), 0, 0
    for n_burn, n_inner in chains:
        ref = gr.view(r, n_burn, n_inner)
        M = ref["last"].shape[-1]
        keep = ref["margin"] >= MARGIN
        empty = p["counts"] == 0
        for draw in (False, True):
            w, V = _solve(p, fit_linear, n_burn, n_inner, draw=draw, seed=seed)
            assert w.shape == (p["S"], p["U"]) and V.shape == (p["S"], p["U"], p["K"])
            assert np.all(np.isfinite(w)) and np.all(np.isfinite(V))
            if not fit_linear:
                assert not w.any()  # exactly 0
            if M == 0:
                continue
            got = fr.join(w, V, fit_linear)
            want = ref["last" if draw else "mean"]
            tol = gr.tolerance(ref, want, n_burn + n_inner)
            err = np.abs(got - want).max(axis=-1).astype(np.float64)
            cells += keep.size
            left += int((~keep).sum())
            ratio = float((err / tol)[keep].max()) if keep.any() else 0.0
            worst[int(draw)] = max(worst[int(draw)], ratio)
            assert np.all(err[keep] <= tol[keep]), (p["U"], p["S"], n_burn, n_inner, draw, ratio)
            if empty.any():  # the prior bit for bit; the draw: the chain's last step from it, in float64 as the kernel takes it
                mu, lam = ref["mu"].astype(np.float64), ref["lam"].astype(np.float64)
                e = r["eps"][n_burn + n_inner - 1][:, empty]
                want_e = mu[:, None, :] + e / np.sqrt(lam)[:, None, :] if draw else np.broadcast_to(mu[:, None, :], e.shape)
                if draw:
                    np.testing.assert_allclose(got[:, empty], want_e, rtol=0, atol=1e-13 * (1 + np.abs(want_e).max()))
                else:
                    assert np.array_equal(got[:, empty], want_e)
    return worst, cells, left


# ---- the kernel against the longdouble reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_class", TASKS)
@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("K", RANKS)
def test_kernel_matches_longdouble_reference(K, fit_linear, n_class):
    """(U, S) in {(1, 1), (5, 2), (9, 3)} x (n_burn, n_inner) in {(0, 1), (1, 1), (2, 3)} x {mean, draw}; context rows empty, one-hot
    and multi-hot; shuffled entity. One reference run of 5 sweeps per problem holds the three chains."""
    worst, cells, left = np.zeros(2), 0, 0
    for (U, S), counts in SHAPES:
        p = gr.problem(np.random.default_rng(10000 * K + 100 * U + 10 * n_class + fit_linear), D, K, S, U, n_class, counts=counts)
        r = gr.run(p, fit_linear, 5, 11)
        assert r["cond"].max() <= 1e5  # (the tolerance cannot go slack)
        w, c, l = _compare(p, r, fit_linear, CHAINS, 11)
        worst, cells, left = np.maximum(worst, w), cells + c, left + l
    assert left <= 0.01 * cells, (left, cells)
    print("fold-in chain K=%d fit_linear=%d n_class=%d: largest error / bound = %.4f (means) %.4f (draws), %d of %d cells left out"
          % (K, fit_linear, n_class, worst[0], worst[1], left, cells))


@pytest.mark.parametrize("n_class", [0, 4])
def test_long_chain_stays_within_the_bound(n_class):
    """20 + 200 sweeps at rank 3: the chain contracts, so the error does not grow beyond the T of the bound"""
    p = gr.problem(np.random.default_rng(91 + n_class), D, 3, 2, 5, n_class, counts=[0, 1, 65, 2, 0])
    worst, cells, left = _compare(p, gr.run(p, True, 220, 3), True, ((20, 200),), 3)
    assert left <= 0.01 * cells, (left, cells)
    print("fold-in chain (20, 200) n_class=%d: largest error / bound = %.4f (means) %.4f (draws), %d of %d cells left out"
          % (n_class, worst[0], worst[1], left, cells))


@pytest.mark.parametrize("n_class", [0, 3])
def test_many_entities_and_samples(n_class):
    """U = 70, S = 7 at rank 16, rows per entity cycling ROW_CHOICES from a random start"""
    p = gr.problem(np.random.default_rng(17 + n_class), D, 16, 7, 70, n_class)
    worst, cells, left = _compare(p, gr.run(p, True, 5, 0x9E3779B97F4A7C15), True, ((2, 3),), 0x9E3779B97F4A7C15)
    assert left <= 0.01 * cells, (left, cells)
    print("fold-in chain U=70 S=7 n_class=%d: largest error / bound = %.4f (means) %.4f (draws), %d of %d cells left out"
          % (n_class, worst[0], worst[1], left, cells))


# ---- invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,fit_linear,n_class", [(17, True, 0), (4, False, 3), (0, True, 5)])
def test_result_does_not_depend_on_the_chunking(K, fit_linear, n_class):
    """scratch bounds that hold one cell, a few samples of one entity, two entities and everything: identical bits, means and draws.
    A store-resident model and the same samples as host arrays: identical bits, for a sub-range of the store too."""
    from myfm_amd import _capi

    S, U = 5, 12
    p = gr.problem(np.random.default_rng(31 + K), D, K, S, U, n_class, counts=[3, 0, 129, 64, 1, 257, 0, 65, 2, 63, 300, 5])
    M = K + (1 if fit_linear else 0)
    cell = (129 * (M + 1) + K + 1) * 8  # the scratch of one cell of entity 2
    full = {draw: _solve(p, fit_linear, 2, 3, draw=draw, seed=4) for draw in (False, True)}
    for bound in (1, 3 * cell, 2 * S * cell, 5 * S * cell + 8):
        for draw in (False, True):
            wc, Vc = _solve(p, fit_linear, 2, 3, draw=draw, seed=4, scratch_bound=bound)
            assert np.array_equal(wc, full[draw][0]) and np.array_equal(Vc, full[draw][1]), (bound, draw)
    st = _capi.Store(D, K)
    h = _capi.FoldIn(p["X"], p["y"], p["entity"], U, fit_linear, scratch_bound=7 * cell)
    try:
        for w0, ws, Vs in p["samples"]:
            st.push(w0, ws, Vs)
        kw = dict(cutpoints=p["cut"], n_burn=2, n_inner=3, seed=4)
        for draw in (False, True):
            ws_, Vs_ = h.solve_gibbs_store(st, p["mu"], p["lam"], _task(n_class), draw=draw, **kw)
            assert np.array_equal(ws_, full[draw][0]) and np.array_equal(Vs_, full[draw][1])
        # samples [1, 4) of the store are samples 0 .. 2 of their call: the streams are keyed by the call's sample index
        sub = dict(p, S=3, samples=p["samples"][1:4], mu=p["mu"][1:4], lam=p["lam"][1:4], cut=None if n_class == 0 else p["cut"][1:4])
        wh, Vh = _solve(sub, fit_linear, 2, 3, seed=4)
        wr, Vr = h.solve_gibbs_store(st, sub["mu"], sub["lam"], _task(n_class), first=1, count=3, **dict(kw, cutpoints=sub["cut"]))
        assert np.array_equal(wr, wh) and np.array_equal(Vr, Vh)
    finally:
        h.close()
        st.close()


def test_streams_on_the_device_are_keyed_as_documented():
    """the same rows as entity 3 of 5 and as entity 1 of 7: sample 1 reads eps row 8 in both (and the same latent rows, the entity
    being alone): the same bits; sample 0 reads eps rows 3 and 1: other draws"""
    base = gr.problem(np.random.default_rng(77), D, 6, 2, 1, 0, counts=[70])

    def placed(U, u):
        return dict(base, U=U, entity=np.full(70, u, dtype=np.int64), counts=np.bincount([u] * 70, minlength=U))

    for draw in (False, True):
        (wa, Va), (wb, Vb) = _solve(placed(5, 3), True, 1, 2, draw=draw, seed=9), _solve(placed(7, 1), True, 1, 2, draw=draw, seed=9)
        assert wa[1, 3] == wb[1, 1] and np.array_equal(Va[1, 3], Vb[1, 1])
        assert wa[0, 3] != wb[0, 1] and not np.array_equal(Va[0, 3], Vb[0, 1])
        (wc, Vc) = _solve(placed(5, 3), True, 1, 2, draw=draw, seed=10)
        assert not np.array_equal(wc, wa) and not np.array_equal(Vc, Va)


# ---- special values ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_model_values_that_are_not_finite():
    from myfm_amd import _capi

    p = gr.problem(np.random.default_rng(2), D, 3, 2, 4, 4, counts=[0, 5, 70, 1])
    for name, bad in (("lam", -1.0), ("lam", 0.0), ("lam", np.nan), ("lam", np.inf), ("mu", np.inf), ("mu", np.nan)):
        q = dict(p)
        q[name] = p[name].copy()
        q[name][1, 2] = bad
        with pytest.raises(ValueError, match="not positive and finite"):
            _solve(q, True, 1, 1)
    q = dict(p, lam=p["lam"].copy())
    q["lam"][:, 0] = -1.0  # component 0 is not read without the linear term
    _solve(q, False, 1, 1)
    for bad, msg in ((np.nan, "cutpoint that is not finite"), (np.inf, "cutpoint that is not finite"), (-9.0, "not non-decreasing")):
        q = dict(p, cut=p["cut"].copy())
        q["cut"][1, 2] = bad
        with pytest.raises(ValueError, match=msg):
            _solve(q, True, 1, 1)
    for bad in (4.0, -1.0, 1.5):
        q = dict(p, y=p["y"].copy())
        q["y"][3] = bad
        with pytest.raises(ValueError, match=r"not an integer in \[0, 4\)"):
            _solve(q, True, 1, 1)
    for n_burn, n_inner, msg in ((1, 0, "n_inner must be at least 1"), (-1, 1, "n_burn must not be negative"), (65535, 1, "must not exceed 65535")):
        with pytest.raises(ValueError, match=msg):
            _solve(p, True, n_burn, n_inner)
    with pytest.raises(ValueError, match="ranks up to 64"):
        _solve(gr.problem(np.random.default_rng(3), 5, 65, 1, 1, 0, counts=[2]), True, 1, 1)
    # a model value that is not finite: an error through the handle and zeros in the result, never a NaN. In V it spoils Lambda (the
    # pivot test), in w only f (the truncation bounds).
    h = _capi.FoldIn(p["X"], p["y"], p["entity"], p["U"], True)
    try:
        for where in ("V", "w"):
            w0, w, V = p["samples"][1]
            w, V = w.copy(), V.copy()
            if where == "V":
                V[:, 1] = np.nan
            else:
                w[:] = np.inf
            K, S, w0s, ws, Vs = _capi._pack_samples([p["samples"][0], (w0, w, V)])
            w_new, V_new = np.full((S, p["U"]), 7.0), np.full((S, p["U"], K), 7.0)
            rc = _capi.lib().mfm_foldin_gibbs_solve(h.h, K, S, _capi._p(w0s), _capi._p(ws), _capi._p(Vs), 1, 4, _capi._p(p["cut"]),
                                                    _capi._p(p["mu"]), _capi._p(p["lam"]), 1, 2, 0, 0, _capi._p(w_new), _capi._p(V_new))
            assert rc == _capi.MFM_ERR_INVALID and b"not positive definite" in _capi.lib().mfm_foldin_last_error(h.h)
            assert np.all(np.isfinite(w_new)) and np.all(np.isfinite(V_new))
            rows = p["counts"] > 0
            assert not w_new[1, rows].any() and not V_new[1, rows].any()  # the spoilt sample's cells with rows: zeros
    finally:
        h.close()


@pytest.mark.parametrize("n_class", [0, 3])
def test_latents_implied_by_the_result_are_finite(n_class):
    """one more sweep from the returned state on the host: every row mean f + z theta is finite, and so is every latent drawn from it"""
    p = gr.problem(np.random.default_rng(8 + n_class), D, 5, 2, 5, n_class, counts=[0, 1, 65, 2, 0])
    w, V = _solve(p, True, 3, 4, draw=True, seed=1)
    theta = fr.join(w, V, True)
    Xg, yg, off = fr.grouped(p["X"], p["y"], p["entity"], 5)
    ent = np.repeat(np.arange(5), np.diff(off))
    m = np.stack([(lambda zf: zf[1] + (zf[0] * theta[s][ent]).sum(axis=-1))(gr.z_and_f(p["samples"][s], Xg, np.float64)) for s in range(2)])
    d, _ = gr.latent_draws(dict(p, yg=yg), m, 7, 1)
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(d)) and np.all(np.abs(m + d) < 40)


# ---- the estimators ----------------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS, OLD_USERS, OLD_ITEMS, RANK, SEEN = 60, 40, 45, 36, 4, 15
N_KEPT = 30


def _rows(cols_a, cols_b, width):
    n = len(cols_a)
    idx = np.empty(2 * n, dtype=np.int32)
    idx[0::2], idx[1::2] = cols_a, cols_b
    X = sps.csr_matrix((np.ones(2 * n), idx, np.arange(0, 2 * n + 1, 2, dtype=np.int64)), shape=(n, width))
    X.sort_indices()
    return X


def _onehot(cols, width):
    n = len(cols)
    return sps.csr_matrix((np.ones(n), np.asarray(cols, dtype=np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, width))


@functools.lru_cache(maxsize=None)
def _fitted(task):
    """60 users x 40 items, every pair labelled; the model is fitted on users [0, 45) x items [0, 36). Each of the 15 new users is
    folded in with 15 of the old items and scored on the other 21; the 4 new items are rated by old and new users alike."""
    from myfm_amd import MyFMGibbsClassifier, MyFMOrderedProbit

    rng = np.random.default_rng(12)
    bu, bi = rng.normal(size=N_USERS), rng.normal(size=N_ITEMS) * 0.5
    P, Q = rng.normal(size=(N_USERS, 2)) * 0.8, rng.normal(size=(N_ITEMS, 2)) * 0.8
    u, i = np.nonzero(np.ones((N_USERS, N_ITEMS), dtype=bool))
    lat = bu[u] + bi[i] + (P[u] * Q[i]).sum(axis=1) + rng.normal(size=u.shape[0])
    y = (lat > 0).astype(np.int64) if task == "classifier" else np.digitize(lat, [-1.2, 0.0, 1.2])
    old = (u < OLD_USERS) & (i < OLD_ITEMS)
    Dm = OLD_USERS + OLD_ITEMS
    fm = (MyFMGibbsClassifier if task == "classifier" else MyFMOrderedProbit)(RANK, random_seed=3)
    fm.fit(_rows(u[old], OLD_USERS + i[old], Dm), y[old], n_iter=50, n_kept_samples=N_KEPT, group_shapes=[OLD_USERS, OLD_ITEMS])
    nu = (u >= OLD_USERS) & (i < OLD_ITEMS)
    order = np.argsort(np.argsort(rng.random((N_USERS, OLD_ITEMS)), axis=1), axis=1)  # per user a random order of the old items
    seen = nu & (order[u, np.minimum(i, OLD_ITEMS - 1)] < SEEN)
    seen_d = dict(u=u[seen] - OLD_USERS, i=i[seen], y=y[seen])
    rest = nu & ~seen
    rest_d = dict(u=u[rest] - OLD_USERS, i=i[rest], y=y[rest])
    ni = i >= OLD_ITEMS
    return dict(fm=fm, D=Dm, seen=seen_d, rest=rest_d, items=dict(u=u[ni], i=i[ni] - OLD_ITEMS, y=y[ni]), task=task)


def _fold_users(f, n_entities=N_USERS - OLD_USERS, **kw):
    s = f["seen"]
    return f["fm"].fold_in_gibbs(_onehot(OLD_USERS + s["i"], f["D"]), s["y"], s["u"], 0, n_entities=n_entities, **kw)


def _log_loss(est, X, y, task):
    p = est.predict_proba(X)
    if task == "classifier":
        return float(-np.mean(np.log(np.where(y > 0, p, 1 - p))))
    return float(-np.mean(np.log(p[np.arange(y.shape[0]), y])))


@pytest.mark.parametrize("task", ["classifier", "ordered"])
def test_estimator_fold_in_gibbs(task):
    f = _fitted(task)
    fm, Dm = f["fm"], f["D"]
    U = N_USERS - OLD_USERS + 1  # one more entity than there are new users: the last has no rows
    X_old = _rows(np.arange(50) % OLD_USERS, OLD_USERS + np.arange(50) % OLD_ITEMS, Dm)
    before = fm.predict_proba(X_old)
    fm2 = _fold_users(f, n_entities=U)
    assert type(fm2) is type(fm) and fm2 is not fm and fm2.fold_in_columns_ == (Dm, Dm + U)
    assert fm2.predictor_.feature_size == Dm + U and fm.predictor_.feature_size == Dm and not hasattr(fm, "fold_in_columns_")
    assert fm2.history_ is fm.history_ and fm2.n_groups_ == 2 and fm2.rank == RANK and fm2.random_seed == 3
    assert fm2.w_samples.shape == (N_KEPT, Dm + U) and fm2.V_samples.shape == (N_KEPT, Dm + U, RANK)
    assert np.all(np.isfinite(fm2.w_samples)) and np.all(np.isfinite(fm2.V_samples))
    # the receiver: untouched; the old columns of the result: the receiver's
    assert np.array_equal(fm.predict_proba(X_old), before)
    assert np.array_equal(fm2.w_samples[:, :Dm], fm.w_samples) and np.array_equal(fm2.V_samples[:, :Dm], fm.V_samples)
    wide = sps.csr_matrix((X_old.data, X_old.indices, X_old.indptr), shape=(50, Dm + U))
    np.testing.assert_allclose(fm2.predict_proba(wide), before, rtol=1e-12, atol=1e-14)
    # the entity without rows: the prior mean of the users' group, bit for bit
    kept = fm.history_.hypers[-N_KEPT:]
    assert np.array_equal(fm2.w_samples[:, Dm + U - 1], np.array([h.mu_w[0] for h in kept]))
    assert np.array_equal(fm2.V_samples[:, Dm + U - 1], np.array([h.mu_V[0] for h in kept]))
    # every device predictor on rows that carry column D + u
    rest = f["rest"]
    Xn = _rows(OLD_USERS + rest["i"], Dm + rest["u"], Dm + U)
    proba = fm2.predict_proba(Xn)
    assert np.all(np.isfinite(proba)) and np.all(proba >= 0) and np.all(proba <= 1)
    if task == "classifier":
        dist = fm2.predict_dist(Xn, quantiles=(0.5,))
        assert np.array_equal(dist.mean, proba) and np.all(dist.std >= 0)
    else:
        assert proba.shape == (Xn.shape[0], 4) and np.array_equal(fm2.cutpoint_samples, fm.cutpoint_samples)
        dist = fm2.predict_proba_dist(Xn, quantiles=(0.5,))
        np.testing.assert_allclose(dist.mean, proba, rtol=1e-12, atol=1e-14)
        exp = fm2.predict_expected_dist(Xn, quantiles=())
        np.testing.assert_allclose(exp.mean, proba @ np.arange(4), rtol=1e-10, atol=1e-12)
    Xq, Xc = _onehot(Dm + np.arange(U), Dm + U), _onehot(OLD_USERS + np.arange(OLD_ITEMS), Dm + U)
    idx, val = fm2.predict_topk(Xq, Xc, 5)
    assert idx.shape == (U, 5) and np.all((idx >= 0) & (idx < OLD_ITEMS)) and np.all(np.diff(val, axis=1) <= 0)
    fm2b = pickle.loads(pickle.dumps(fm2))
    assert fm2b.fold_in_columns_ == (Dm, Dm + U) and np.array_equal(fm2b.predict_proba(Xn), proba)
    # the same seed: the same result; another seed: another; a draw differs from the mean
    same, other = _fold_users(f, n_entities=U), _fold_users(f, n_entities=U, random_seed=8)
    assert np.array_equal(same.w_samples, fm2.w_samples) and np.array_equal(same.V_samples, fm2.V_samples)
    assert not np.array_equal(other.w_samples[:, Dm:Dm + U - 1], fm2.w_samples[:, Dm:Dm + U - 1])
    d1, d2 = _fold_users(f, draw=True, random_seed=8), _fold_users(f, draw=True, random_seed=8)
    assert np.array_equal(d1.w_samples, d2.w_samples) and not np.array_equal(d1.w_samples[:, Dm:], other.w_samples[:, Dm:Dm + U - 1])


@pytest.mark.parametrize("task", ["classifier", "ordered"])
def test_fold_in_gibbs_composes_and_helps(task):
    """users, then items whose raters are old and new users alike (rows in the first result's feature space). The held-out
    log-loss of the folded-in users is below that of the same users folded in with no observations, the prior -- a comparison,
    not a threshold; the items' posterior fits the labels it saw better than the items' prior does."""
    f = _fitted(task)
    fm, Dm, rest, it = f["fm"], f["D"], f["rest"], f["items"]
    U, I = N_USERS - OLD_USERS, N_ITEMS - OLD_ITEMS
    fm2 = _fold_users(f)
    none = (sps.csr_matrix((0, Dm)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    prior = fm.fold_in_gibbs(*none, 0, n_entities=U)
    X = _rows(OLD_USERS + rest["i"], Dm + rest["u"], Dm + U)
    ll_fold, ll_prior = _log_loss(fm2, X, rest["y"], task), _log_loss(prior, X, rest["y"], task)
    print("%s: held-out log-loss %.4f folded in, %.4f with the prior, on %d labels" % (task, ll_fold, ll_prior, X.shape[0]))
    assert ll_fold < ll_prior
    ucol = np.where(it["u"] < OLD_USERS, it["u"], Dm + it["u"] - OLD_USERS)
    fm3 = fm2.fold_in_gibbs(_onehot(ucol, Dm + U), it["y"], it["i"], 1)
    assert type(fm3) is type(fm) and fm3.fold_in_columns_ == (Dm + U, Dm + U + I) and fm2.fold_in_columns_ == (Dm, Dm + U)
    assert np.array_equal(fm3.w_samples[:, :Dm + U], fm2.w_samples) and np.array_equal(fm3.V_samples[:, :Dm + U], fm2.V_samples)
    Xi = _rows(ucol, Dm + U + it["i"], Dm + U + I)
    iprior = fm2.fold_in_gibbs(sps.csr_matrix((0, Dm + U)), none[1], none[2], 1, n_entities=I)
    assert _log_loss(fm3, Xi, it["y"], task) < _log_loss(iprior, Xi, it["y"], task)
