"""predict_contributions on the device against the longdouble reference of tests/contrib_ref.py, within the bounds
derived there (gamma_n M_c per component and sample; the recurrence term is measured on each case's own inputs and printed).

The lane map of k_contrib changes shape at ranks 4 | 5, 16 | 17, 32 | 33 (lanes per row), 64 | 65 and 128 | 129 (walks of the row),
and the buckets of fields end at 2, 4, 8 and 16: contrib_ref.RANKS and contrib_ref.FIELDS hold these edges and the edge plus one,
in the place of the issue's rank list, whose edges (8 | 9, 130) are kept as well."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import contrib_ref as cr
from tests import score_ref as sr
from tests import test_gpu_crps as tc

pytestmark = pytest.mark.gpu
LD = np.longdouble


def same(a, b):
    """two results are equal bit for bit (bias, bias_std and the four arrays)"""
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(tuple(a)[:6], tuple(b)[:6]))


def run(X, blocks, samples, F, fo, **kw):
    from myfm_amd import _capi

    d = _capi.Design(X, blocks)
    try:
        return d.contributions(samples, F, fo, **kw)
    finally:
        d.close()


def check_exact_rows(got, F, S):
    """the rows of design37 whose values are exact: row 0 is empty, row 4 holds one unit entry per field"""
    _, _, lin, lin_std, inter, inter_std = got[:6]
    for a in (lin, lin_std, inter, inter_std):
        assert np.all(a[:, 0] == 0.0)
    diag = [i for i, (g, h) in enumerate(cr.pairs(F)) if g == h]
    assert np.all(inter[diag, 4] == 0.0) and np.all(inter_std[diag, 4] == 0.0)
    if S == 1:
        assert got[1] == 0.0 and np.all(lin_std == 0.0) and np.all(inter_std == 0.0)


@pytest.fixture(scope="module")
def cases():
    """every host-sample case's inputs and reference, computed once"""
    out = {}
    for K, F, kind, S in cr.shape_cases():
        fo = cr.grouping(F, kind)
        X, samples = cr.design37(fo, F), cr.random_samples(cr.D_TEST, K, S)
        out[(K, F, kind, S)] = (fo, X, samples, cr.Reference(X, (), samples, fo, F))
    return out


@pytest.mark.parametrize("K,F,kind,S", cr.shape_cases(), ids=lambda v: str(v))
def test_host_samples_match_the_reference(cases, K, F, kind, S):
    fo, X, samples, ref = cases[(K, F, kind, S)]
    got = run(X, (), samples, F, fo)
    ref.check(got, "device K=%d F=%d %s S=%d" % (K, F, kind, S))
    check_exact_rows(got, F, S)


@pytest.mark.parametrize("key", [(9, 3, "interleaved", 5), (65, 5, "contiguous", 5)], ids=str)
def test_sample_chunk_and_row_tile_do_not_change_a_bit(cases, key):
    fo, X, samples, _ = cases[key]
    F = key[1]
    base = run(X, (), samples, F, fo)
    for chunk in (1, 2, 3):
        assert same(base, run(X, (), samples, F, fo, chunk_samples=chunk)), chunk
    for tile in (1, 7, 36, 37, 38):
        assert same(base, run(X, (), samples, F, fo, tile_rows=tile)), tile
    assert same(base, run(X, (), samples, F, fo, tile_rows=7, chunk_samples=2))


# ---- relation blocks: read in place, against the same rows expanded into a main matrix ----
N_B, N_U, N_I = 37, 12, 9


def block_designs():
    rng = np.random.default_rng(3)
    u, i = rng.integers(0, N_U, size=N_B), rng.integers(0, N_I, size=N_B)  # (random maps: not monotone)
    assert np.any(np.diff(i) < 0) and np.any(np.diff(u) < 0)
    users = tc.onehot(u, N_U)
    items = sps.hstack([sps.identity(N_I, format="csr"), sps.csr_matrix(rng.normal(size=(N_I, 2)))], format="csr")
    people = sps.hstack([sps.identity(N_U, format="csr"), sps.csr_matrix(rng.normal(size=(N_U, 1)))], format="csr")
    f_items = [1] * N_I + [2, 2]  # the block's columns span two fields
    return {
        "two-fields": (users, [(i, items)], np.array([0] * N_U + f_items), 3),
        "two-blocks": (sps.csr_matrix(rng.normal(size=(N_B, 2))), [(u, people), (i, items)], np.array([0, 0] + [1] * N_U + [3] + f_items), 4),
        "no-main-columns": (sps.csr_matrix((N_B, 0)), [(i, items)], np.array(f_items) - 1, 2),
        "interleaved": (users, [(i, items)], np.arange(N_U + N_I + 2) % 3, 3),
    }


@pytest.mark.parametrize("name", ["two-fields", "two-blocks", "no-main-columns", "interleaved"])
@pytest.mark.parametrize("K", [3, 33])
def test_relation_blocks_match_the_expanded_rows(name, K):
    X, blocks, fo, F = block_designs()[name]
    fo = fo.astype(np.int32)
    D = fo.shape[0]
    samples = cr.random_samples(D, K, 5)
    ref = cr.Reference(X, blocks, samples, fo, F)
    got = run(X, blocks, samples, F, fo)
    ref.check(got, "blocks %s K=%d" % (name, K))
    expanded = sps.hstack([X] + [sps.csr_matrix(B)[mp] for mp, B in blocks], format="csr")
    ref.check(run(expanded, (), samples, F, fo), "expanded %s K=%d" % (name, K))
    assert same(got, run(X, blocks, samples, F, fo, tile_rows=7, chunk_samples=2))


# ---- fitted estimators: the tiny models of test_gpu_crps.py ----
fitted = tc.fitted


def model_grouping(m):
    shapes = [tc.N_USERS] + ([tc.N_ITEMS] if not m["rels"] else [r.feature_size for r in m["rels"]])
    return shapes, np.repeat(np.arange(len(shapes)), shapes).astype(np.int32)


def test_fitted_model_matches_the_reference_and_adds_up(fitted):
    import myfm_amd
    from myfm_amd.utils.evaluation import contribution_total

    m = fitted
    est, samples = m["est"], tc.host_samples(m["est"])
    shapes, fo = model_grouping(m)
    assert np.array_equal(est.grouping_, fo)
    got = est.predict_contributions(m["X"], m["rels"])
    assert isinstance(got, myfm_amd.ScoreContributions)
    assert got.linear.shape == got.linear_std.shape == (2, tc.N_ROWS) and got.interaction.shape == got.interaction_std.shape == (3, tc.N_ROWS)
    assert np.array_equal(got.pairs, [[0, 0], [0, 1], [1, 1]])
    blocks = tc.capi_blocks(m["rels"])
    ref = cr.Reference(m["X"], blocks, samples, fo, 2)
    ref.check(got, "%s%s" % (m["kind"], "-block" if m["block"] else ""))
    if not m["block"]:
        assert np.all(got.interaction[[0, 2]] == 0.0)  # one unit entry per field
    # the components add up to the mean of the per-sample scores of the single-sample scorer
    total = contribution_total(got)
    score_tol = np.mean([sr.fm_score_bound(m["X"], blocks, *s)[1] for s in samples], axis=0)
    mag = abs(LD(got.bias)) + np.abs(got.linear).sum(axis=0) + np.abs(got.interaction).sum(axis=0) + np.abs(m["f"]).mean(axis=0)
    tol = ref.tol_mean.sum(axis=0) + ref.tol_bias + score_tol + cr.gamma(5 + len(samples) + 2) * mag
    dev = np.abs(total.astype(LD) - m["f"].astype(LD).mean(axis=0))
    print("total against the mean score: worst deviation / bound %.3f" % float((dev / tol).max()))
    assert np.all(dev <= tol)
    # the default grouping is the fit's: passing it again gives the same bits, in both spellings
    assert same(got, est.predict_contributions(m["X"], m["rels"], group_shapes=shapes))
    assert same(got, est.predict_contributions(m["X"], m["rels"], grouping=fo))


def test_store_host_and_pickle_give_the_same_bits(fitted):
    from myfm_amd import _capi

    m = fitted
    est = m["est"]
    _, fo = model_grouping(m)
    got = est.predict_contributions(m["X"], m["rels"])
    assert est.predictor_.resident
    back = pickle.loads(pickle.dumps(est))
    assert np.array_equal(back.grouping_, fo) and not back.predictor_.resident
    assert same(got, back.predict_contributions(m["X"], m["rels"]))
    assert same(got, run(m["X"], tc.capi_blocks(m["rels"]), tc.host_samples(est), 2, fo))


def test_a_model_without_grouping_must_be_given_one(fitted):
    m = fitted
    back = pickle.loads(pickle.dumps(m["est"]))
    del back.grouping_
    with pytest.raises(ValueError, match="no grouping_"):
        back.predict_contributions(m["X"], m["rels"])
    shapes, _ = model_grouping(m)
    assert same(m["est"].predict_contributions(m["X"], m["rels"]), back.predict_contributions(m["X"], m["rels"], group_shapes=shapes))


def test_fold_in_extends_the_grouping():
    X, rels, lat = tc.make_data(False)
    est = tc.fit("regressor", X, rels, lat)
    rng = np.random.default_rng(2)
    U, n = 3, 12
    ctx = tc.onehot(tc.N_USERS + rng.integers(0, tc.N_ITEMS, size=n).reshape(-1, 1))  # new users' observations: the item's one-hot
    ext = est.fold_in(ctx, rng.normal(size=n), rng.integers(0, U, size=n), group=0, n_entities=U)
    D = tc.D
    assert ext.grouping_.shape == (D + U,) and np.all(ext.grouping_[D:] == 0) and np.array_equal(ext.grouping_[:D], est.grouping_)
    q = tc.onehot(np.array([[D + 1, tc.N_USERS + 4]]), D + U)  # new user 1 with item 4
    got = ext.predict_contributions(q)
    samples = tc.host_samples(ext)
    cr.Reference(q, (), samples, ext.grouping_, 2).check(got, "fold_in")
    w = np.asarray([s[1] for s in samples])
    assert abs(got.linear[0, 0] - w[:, D + 1].mean()) <= 4 * np.spacing(np.abs(w[:, D + 1]).max())
    assert np.all(got.interaction[[0, 2], 0] == 0.0) and got.interaction[1, 0] != 0.0


def test_combined_chains_equal_the_concatenated_samples():
    import myfm_amd

    X, rels, lat = tc.make_data(True)
    a = tc.fit("regressor", X, rels, lat)
    b = type(a)(tc.RANK, random_seed=6).fit(X, lat, X_rel=rels, n_iter=8, n_kept_samples=tc.N_KEPT, group_shapes=[tc.N_USERS, rels[0].feature_size])
    both = myfm_amd.combine_chains([a, b])
    assert np.array_equal(both.grouping_, a.grouping_)
    got = both.predict_contributions(X, rels)
    want = run(X, tc.capi_blocks(rels), tc.host_samples(a) + tc.host_samples(b), 2, a.grouping_)
    assert same(got, want)
