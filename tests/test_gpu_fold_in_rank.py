"""Ranking under a new entity's own posterior on the device: the dense form against the longdouble reference of
tests/fold_in_rank_ref.py at every tile and k-step edge, the lists against the reference's order, the invariance under the entity
chunking, and MyFMGibbsRegressor.fold_in_topk / fold_in_pairs_dist against the folded model's own predictors.

Tolerance: DEVICE_C = 8 TWIN_C times the unit bounds of fold_in_rank_ref (derived there); cond_2(Lambda_ref) <= 1e5 is asserted.
On one MI355X the largest error / unit bound was 0.61 (rank 0 without the linear term; below 0.012 from rank 14 on)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from tests import fold_in_rank_ref as rr
from tests import fold_in_ref as fr

pytestmark = pytest.mark.gpu

D = 40
ROWS = (0, 1, 2, 65)
# (rank, U, S, I): every rank of the 4-wide k-step and 16-row tile edges (M = rank + fit_linear, the mean is row M) with both
# fit_linear, the candidate counts around the 16-column tile and the 256-candidate step, the entity counts around the block of 8
DENSE = [(0, 5, 2, 17), (1, 1, 1, 1), (3, 5, 7, 15), (4, 17, 2, 16), (14, 5, 2, 64), (15, 33, 1, 65), (16, 5, 7, 257), (31, 17, 2, 17),
         (32, 5, 2, 64), (63, 5, 1, 65), (64, 17, 2, 257)]


def _handle(p, Xc, fit_linear, exclude=None, scratch_bound=None):
    from myfm_amd import _capi

    h = _capi.FoldIn(p["X"], p["y"], p["entity"], p["U"], fit_linear, scratch_bound=scratch_bound)
    h.set_candidates(Xc)
    if exclude is not None:
        h.set_exclude(exclude)
    return h


def _dist(p, Xc, fit_linear, **kw):
    h = _handle(p, Xc, fit_linear, **kw)
    try:
        return dict(zip(rr.FIELDS, h.rank_dist(p["samples"], p["alpha"], p["mu"], p["lam"])))
    finally:
        h.close()


@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("K,U,S,I", DENSE)
def test_dense_form_matches_longdouble_reference(K, U, S, I, fit_linear):
    rng = np.random.default_rng(7000 + 100 * K + 2 * U + fit_linear)
    p = fr.problem(rng, D, K, S, U, counts=fr.entity_counts(rng, U, ROWS))
    Xc = fr.context_rows(rng, I, D)
    want, bound, cond = rr.summary(p, Xc, fit_linear)
    assert cond.max() <= 1e5
    got = _dist(p, Xc, fit_linear)
    w = rr.worst(got, want, bound)
    print("fold-in rank K=%d fit_linear=%d U=%d S=%d I=%d: error / bound = %.4f" % (K, fit_linear, U, S, I, w))
    assert w <= rr.DEVICE_C
    # std_within is 0 only where z is: an all-zero q without the linear term (an empty context row; the reference has an exact 0 too)
    assert np.array_equal(got["std_within"] > 0, want["std_within"] > 0) and np.all(got["std"] >= got["std_within"])
    if fit_linear:
        assert np.all(got["std_within"] > 0)


# ---- the lists ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _list_case():
    """5 entities x 300 candidates with real-valued multi-hot contexts (no two candidates alike), rank 9, 3 samples; the exclusion
    pattern leaves entity 1 with 7 candidates and takes a third of the others'"""
    rng = np.random.default_rng(41)
    p = fr.problem(rng, D, 9, 3, 5, counts=(0, 1, 2, 65, 7))
    Xc = sps.random(300, D, density=0.1, random_state=np.random.RandomState(3), data_rvs=lambda n: rng.uniform(0.5, 2.0, n)).tolil()
    Xc[:, 0] = rng.uniform(0.5, 2.0, 300)[:, None]
    Xc = Xc.tocsr()
    ex = rng.random((5, 300)) < 0.33
    ex[1] = np.arange(300) >= 7
    want, bound, _ = rr.summary(p, Xc, True)
    return p, Xc, sps.csr_matrix(ex.astype(np.float64)), want, bound


@pytest.mark.parametrize("excluded", [False, True])
@pytest.mark.parametrize("by", ["ucb", "gain"])
@pytest.mark.parametrize("k", [1, 10, 64, 65, 256])
def test_lists_match_the_reference_order(k, by, excluded):
    p, Xc, ex, want, bound = _list_case()
    beta = 1.5
    tol = rr.DEVICE_C * (bound["gain"] if by == "gain" else bound["mean"] + beta * bound["std"])
    ref_idx, ref_val = rr.ranked(want, by, beta, k, ex if excluded else None)
    # the reference's own order is decided by gaps the tolerance cannot close
    live = ref_idx >= 0
    with np.errstate(invalid="ignore"):
        gaps = (ref_val[:, :-1] - ref_val[:, 1:])[live[:, 1:]].astype(np.float64)
    assert gaps.size and gaps.min() > 4 * tol.max()
    h = _handle(p, Xc, True, exclude=ex if excluded else None)
    try:
        idx, value, mean, std, gain = h.rank_topk(p["samples"], p["alpha"], p["mu"], p["lam"], k, by=by, beta=beta)
    finally:
        h.close()
    assert np.array_equal(idx, ref_idx[:, :k])
    hit = idx >= 0
    assert np.all(np.isneginf(value[~hit])) and np.all(np.isnan(mean[~hit]) & np.isnan(std[~hit]) & np.isnan(gain[~hit]))
    if excluded:
        assert hit[1].sum() == min(k, 7)  # k above the live candidates: a tail
    u = np.nonzero(hit)[0]
    for got, name in ((mean, "mean"), (std, "std"), (gain, "gain")):
        err = np.abs(got[hit].astype(rr.LD) - want[name][u, idx[hit]]).astype(np.float64)
        assert np.all(err <= rr.DEVICE_C * bound[name][u, idx[hit]]), name
    assert np.all(np.abs(value[hit].astype(rr.LD) - ref_val[:, :k][hit]).astype(np.float64) <= tol[u, idx[hit]])
    assert np.all(np.abs(value[hit] - (gain[hit] if by == "gain" else mean[hit] + beta * std[hit])) <= 2 * tol[u, idx[hit]])


def test_results_do_not_depend_on_the_entity_chunks():
    """scratch bounds that hold all 33 entities, 24 of them (two chunks) and one block of 8 (five chunks): identical bits"""
    rng = np.random.default_rng(77)
    K, S, U, I = 16, 2, 33, 65
    p = fr.problem(rng, D, K, S, U, counts=fr.entity_counts(rng, U, ROWS))
    Xc = fr.context_rows(rng, I, D)
    ex = sps.csr_matrix((rng.random((U, I)) < 0.2).astype(np.float64))
    per_entity = S * (2 * 5 * 64 + K + 1) * 8  # (the kept operand at M = 17: 2 row tiles x 5 k-steps x 64 doubles; csrc/mfm_foldin_rank.hip)
    base, base_list = None, None
    for chunk in (None, 24, 1):
        dense_b = None if chunk is None else chunk * (per_entity + 4 * I * 8) + 64
        list_b = None if chunk is None else chunk * (per_entity + I * 8 + 3 * 4 + 65 * 10 * 12 + 280) + 64
        got = _dist(p, Xc, True, scratch_bound=dense_b)
        h = _handle(p, Xc, True, exclude=ex, scratch_bound=list_b)
        try:
            lists = h.rank_topk(p["samples"], p["alpha"], p["mu"], p["lam"], 10)
        finally:
            h.close()
        if base is None:
            base, base_list = got, lists
        assert all(np.array_equal(got[n], base[n]) for n in rr.FIELDS)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(lists, base_list))


# ---- the estimator ----------------------------------------------------------------------------------------------------------------
def test_estimator_agrees_with_the_folded_model():
    """mean is fold_in(...).predict_pairs on one-hot queries, std is never below that model's predict_pairs_dist std (which lacks the
    within-sample term), the lists are the dense outputs' order, and folding items into a model that holds folded-in users works"""
    from myfm_amd import MyFMGibbsRegressor

    rng = np.random.default_rng(5)
    nu, ni, U = 30, 20, 6
    u, i = np.nonzero(rng.random((nu, ni)) < 0.5)
    y = 3.0 + rng.normal(size=nu)[u] * 0.5 + rng.normal(size=ni)[i] * 0.5 + rng.normal(size=u.size) * 0.3
    Dm = nu + ni
    onehot = lambda cols, width: sps.csr_matrix((np.ones(len(cols)), (np.arange(len(cols)), cols)), shape=(len(cols), width))  # noqa: E731
    fm = MyFMGibbsRegressor(3, random_seed=1)
    fm.fit(onehot(u, Dm) + onehot(nu + i, Dm), y, n_iter=30, n_kept_samples=12, group_shapes=[nu, ni])
    ent = rng.integers(0, U - 1, size=14)  # (the last entity has no rows)
    X, yy = onehot(nu + rng.integers(0, ni, size=14), Dm), rng.normal(size=14) + 3.0
    Xc = onehot(nu + np.arange(ni), Dm)
    dist = fm.fold_in_pairs_dist(X, yy, ent, 0, Xc, n_entities=U)
    fm2 = fm.fold_in(X, yy, ent, 0, n_entities=U)
    wide = sps.csr_matrix((Xc.data, Xc.indices, Xc.indptr), shape=(ni, Dm + U))
    Xq = onehot(Dm + np.arange(U), Dm + U)
    np.testing.assert_allclose(dist.mean, fm2.predict_pairs(Xq, wide), rtol=1e-12, atol=1e-12)
    folded = fm2.predict_pairs_dist(Xq, wide)
    assert np.all(dist.std >= folded.std) and np.all(dist.std_within > 0) and np.all(dist.gain > 0)
    np.testing.assert_allclose(dist.std ** 2, dist.std_within ** 2 + folded.std ** 2, rtol=1e-9)
    for by, full in (("ucb", dist.mean + 2.0 * dist.std), ("gain", dist.gain)):
        top = fm.fold_in_topk(X, yy, ent, 0, Xc, 5, by=by, beta=2.0, n_entities=U)
        assert np.array_equal(top.indices, np.argsort(-full, axis=1, kind="stable")[:, :5])
        np.testing.assert_allclose(top.value, np.take_along_axis(full, top.indices, axis=1), rtol=1e-12)
    # items folded into the model that holds the folded-in users: the candidates name the new users' columns
    it = rng.integers(0, 3, size=10)
    items = fm2.fold_in_pairs_dist(onehot(Dm + rng.integers(0, U, size=10), Dm + U), rng.normal(size=10) + 3.0, it, 1, Xq)
    assert items.mean.shape == (3, U) and np.all(np.isfinite(items.mean)) and np.all(items.std_within > 0)
