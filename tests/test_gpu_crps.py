"""predict_crps on the device against the NumPy / SciPy reference of tests/crps_ref.py.

The per-sample scores (S, N) the reference starts from are taken from the existing single-sample scorer (mfm_design_predict, one
sample, mode 0), so the comparison isolates the new kernels. Two values a, b are compared by |a - b| / max(1, |b|) <= CRPS_RTOL
(crps_ref.py, where the constant is derived); with a relation-block design 2 max_s ulp(score_s) is added per row for a last-bit
difference of the scores (|dA/dm| <= 1 in both terms of the energy form, |d Phi / dt| < 1 per cut likewise).

CRPS_BLOCK = 4 is the register block of k_row_crps_mix (csrc/mfm_crps.hpp): the host-sample cases run S = 3, 4 and 5 around it."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import crps_ref as cr

pytestmark = pytest.mark.gpu

CRPS_BLOCK = 4
N_USERS, N_ITEMS, N_ROWS, RANK, N_KEPT, N_CLASS = 40, 30, 600, 3, 4, 5
D = N_USERS + N_ITEMS
TASK = {"regressor": 0, "classifier": 1, "ordered": 2}


def onehot(cols, width=D):
    cols = np.asarray(cols, dtype=np.int32).reshape(len(cols), -1)
    n, m = cols.shape
    X = sps.csr_matrix((np.ones(n * m), cols.ravel(), np.arange(0, n * m + 1, m, dtype=np.int64)), shape=(n, width))
    X.sort_indices()
    return X


def same(a, b):
    """two result tuples are equal bit for bit"""
    a, b = tuple(a), tuple(b)
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def host_samples(est):
    return [(fm.w0, np.asarray(fm.w), np.asarray(fm.V)) for fm in est.predictor_.samples]


def capi_blocks(rels):
    return [(np.asarray(r.original_to_block_array), r.data) for r in rels]


def device_scores(X, rels, samples):
    """(S, N): every sample's scores from the single-sample scorer"""
    from myfm_amd import _capi

    d = _capi.Design(X, capi_blocks(rels))
    out = np.stack([d.predict([s], 0) for s in samples])
    d.close()
    return out


def constants(kind, est):
    """(precisions, cutpoints) of the kept samples, None where the task has none"""
    S = len(est.predictor_.samples)
    if kind == "regressor":
        return np.array([h.alpha for h in est.history_.hypers[-S:]]), None
    if kind == "ordered":
        return None, np.stack([np.asarray(fm.cutpoints[0]) for fm in est.predictor_.samples])
    return None, None


def check_against_reference(kind, got, f, y, prec, cut, block=False):
    """all three outputs of `got` against the reference on the scores f; crps >= 0"""
    want = cr.crps(TASK[kind], f, np.asarray(y, dtype=np.float64), prec, cut)
    extra = 2 * np.spacing(np.abs(f)).max(axis=0) if block else 0.0
    for name, a, b in zip(("crps", "accuracy", "spread"), got, want):
        assert a.shape == b.shape and np.all(np.isfinite(a)), name
        dev = np.abs(a - b) - extra
        worst = (dev / np.maximum(1.0, np.abs(b))).max() if len(b) else 0.0
        print("%s %s S=%d N=%d: worst deviation %.3e (bound %.3e)" % (kind, name, f.shape[0], f.shape[1], worst, cr.CRPS_RTOL))
        assert np.all(dev <= cr.CRPS_RTOL * np.maximum(1.0, np.abs(b))), (name, worst)
    assert np.all(got[0] >= 0)


def make_data(block):
    rng = np.random.default_rng(31)
    pair = rng.permutation(N_USERS * N_ITEMS)[:N_ROWS]
    u, i = pair // N_ITEMS, pair % N_ITEMS
    P, Q = rng.normal(size=(N_USERS, 2)), rng.normal(size=(N_ITEMS, 2))
    lat = 0.5 * rng.normal(size=N_USERS)[u] + (P[u] * Q[i]).sum(axis=1) + 0.5 * rng.normal(size=N_ROWS)
    if not block:
        return onehot(np.stack([u, N_USERS + i], axis=1)), [], lat
    import myfm_amd

    # the items through a relation block: their one-hot and one real-valued item feature, D = 40 + 31
    item = sps.hstack([sps.identity(N_ITEMS, format="csr"), sps.csr_matrix(rng.normal(size=(N_ITEMS, 1)))], format="csr")
    return onehot(u, N_USERS), [myfm_amd.RelationBlock(i.astype(np.int64), item)], lat


def targets(kind, lat):
    return {"regressor": lat, "classifier": (lat > 0).astype(np.float64), "ordered": np.digitize(lat, [-1.5, -0.5, 0.5, 1.5])}[kind]


def fit(kind, X, rels, y, n_kept=N_KEPT, n_iter=8):
    import myfm_amd

    cls = {"regressor": myfm_amd.MyFMGibbsRegressor, "classifier": myfm_amd.MyFMGibbsClassifier, "ordered": myfm_amd.MyFMOrderedProbit}[kind]
    shapes = [N_USERS] + ([N_ITEMS] if not rels else [r.feature_size for r in rels])
    return cls(RANK, random_seed=5).fit(X, y, X_rel=rels, n_iter=n_iter, n_kept_samples=n_kept, group_shapes=shapes)


@pytest.fixture(scope="module", params=[(k, b) for b in (False, True) for k in ("regressor", "classifier", "ordered")],
                ids=lambda p: p[0] + ("-block" if p[1] else ""))
def fitted(request):
    """the three tiny models of test_gpu_log_density.py (40 x 30 one-hot, 600 rows, rank 3, 4 kept of 8 iterations), and the same
    three with the items in a relation block; the per-sample scores of the fit's rows, computed once"""
    kind, block = request.param
    X, rels, lat = make_data(block)
    y = targets(kind, lat)
    est = fit(kind, X, rels, y)
    assert est.predictor_.resident and len(est.predictor_.samples) == N_KEPT
    prec, cut = constants(kind, est)
    return dict(kind=kind, block=block, est=est, X=X, rels=rels, y=np.asarray(y, dtype=np.float64), prec=prec, cut=cut,
                f=device_scores(X, rels, host_samples(est)))


def test_all_outputs_match_the_reference(fitted):
    from myfm_amd import CrpsScore

    m = fitted
    got = m["est"].predict_crps(m["X"], m["y"], m["rels"])
    assert isinstance(got, CrpsScore) and got.crps.shape == got.accuracy.shape == got.spread.shape == (N_ROWS,)
    check_against_reference(m["kind"], got, m["f"], m["y"], m["prec"], m["cut"], m["block"])


def test_discrete_scores_follow_from_predict_proba(fitted):
    """classifier: the Brier score of predict_proba; ordered probit: the ranked probability score of its class probabilities"""
    m = fitted
    if m["kind"] == "regressor":
        return
    got = m["est"].predict_crps(m["X"], m["y"], m["rels"])
    proba = m["est"].predict_proba(m["X"], m["rels"])
    if m["kind"] == "classifier":
        want = (proba - m["y"]) ** 2
    else:
        cdf = np.cumsum(proba, axis=1)[:, :-1]
        want = ((cdf - (m["y"][:, None] <= np.arange(N_CLASS - 1)[None, :])) ** 2).sum(axis=1)
    print("%s crps against predict_proba: worst relative deviation %.3e" % (m["kind"], (np.abs(got.crps - want) / np.maximum(want, 1e-300)).max()))
    np.testing.assert_allclose(got.crps, want, rtol=1e-12, atol=0)


def test_the_pickle_round_trip_gives_the_same_bits(fitted):
    """the resident store read in place and the restored model's host samples, packed for the call"""
    m = fitted
    restored = pickle.loads(pickle.dumps(m["est"]))
    assert not restored.predictor_.resident
    rows, y = m["X"][:257], m["y"][:257]
    rels = [type(r)(np.asarray(r.original_to_block_array)[:257], r.data) for r in m["rels"]]
    assert same(m["est"].predict_crps(rows, y, rels), restored.predict_crps(rows, y, rels))


def test_tilings_do_not_change_a_bit(fitted):
    """N = 257 through _capi: tile_rows 64 (last tile 1 row), 257, 1; chunk_samples 1, 3 (ragged over the 4 samples); the host
    flavour and the store"""
    from myfm_amd import _capi

    m = fitted
    task = TASK[m["kind"]]
    rows, y = m["X"][:257], m["y"][:257]
    blocks = [(mp[:257], B) for mp, B in capi_blocks(m["rels"])]
    samples = host_samples(m["est"])
    d = _capi.Design(rows, blocks)
    st = _capi.Store(d.D, RANK)
    for w0, w, V in samples:
        st.push(w0, w, V)
    kw = dict(precisions=m["prec"], cutpoints=m["cut"])
    want = st.crps(d, task, y, **kw)
    assert same(want, m["est"].predict_crps(rows, y, [type(r)(np.asarray(r.original_to_block_array)[:257], r.data) for r in m["rels"]]))
    assert same(want, d.crps(samples, task, y, **kw))
    for tile_rows in (64, 257, 1):
        for chunk_samples in (1, 3):
            assert same(want, st.crps(d, task, y, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (tile_rows, chunk_samples)
    assert same(want, d.crps(samples, task, y, tile_rows=64, chunk_samples=3, **kw))
    st.close()
    d.close()


def random_call(kind, S, N, seed, n_cut=N_CLASS - 1):
    """(rows, samples, y, precisions, cutpoints) of a valid call on random host samples: no fit"""
    rng = np.random.default_rng(seed)
    rows = onehot(np.stack([rng.integers(0, N_USERS, size=N), N_USERS + rng.integers(0, N_ITEMS, size=N)], axis=1).reshape(N, 2))
    samples = [(0.1 * rng.normal(), rng.normal(size=D) * 0.5, rng.normal(size=(D, RANK)) * 0.5) for _ in range(S)]
    prec = np.exp(rng.uniform(-1.0, 2.0, size=S)) if kind == "regressor" else None
    cut = cr.spaced_cutpoints(rng, S, n_cut) if kind == "ordered" else None
    y = {"regressor": rng.normal(size=N), "classifier": (rng.random(N) < 0.5).astype(np.float64),
         "ordered": rng.integers(0, n_cut + 1, size=N).astype(np.float64)}[kind]
    return rows, samples, y, prec, cut


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_the_library_refuses_before_it_computes(kind):
    """the checks of the C entry points: those of the log density, message for message, and the sample limit"""
    import ctypes as C

    from myfm_amd import _capi

    task = TASK[kind]
    rows, samples, y, prec, cut = random_call(kind, 3, 5, 1)
    d = _capi.Design(rows)
    kw = dict(precisions=prec, cutpoints=cut)
    with pytest.raises(ValueError, match="negative tiling"):
        d.crps(samples, task, y, tile_rows=-1, **kw)
    with pytest.raises(ValueError, match="bad task"):
        d.crps(samples, 3, y, **kw)
    with pytest.raises(ValueError, match="y must be finite"):
        d.crps(samples, task, np.array([np.nan] + list(y[1:])), **kw)
    narrow = _capi.Store(D - 1, RANK)  # a store of another feature size
    for w0, w, V in samples:
        narrow.push(w0, w[:-1], V[:-1])
    with pytest.raises(ValueError, match="feature size mismatch"):
        narrow.crps(d, task, y, **kw)
    narrow.close()
    K, S, w0s, ws, Vs = _capi._pack_samples(samples)
    out = [np.empty(5) for _ in range(3)]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _capi.lib().mfm_design_crps(d.h, K, S, p(w0s), p(ws), p(Vs), task, p(y), p(prec), 0 if cut is None else cut.shape[1], p(cut),
                                     0, 0, p(out[0]), None, p(out[2]))
    assert rc == _capi.MFM_ERR_INVALID and b"three output arrays" in _capi.lib().mfm_design_last_error(d.h)
    if task != 0:
        with pytest.raises(ValueError, match="noise precisions apply to regression"):
            d.crps(samples, task, y, precisions=np.ones(3), cutpoints=cut)
    else:
        with pytest.raises(ValueError, match="needs the noise precision"):
            d.crps(samples, task, y)
        with pytest.raises(ValueError, match="positive and finite"):
            d.crps(samples, task, y, precisions=np.array([1.0, -1.0, 1.0]))
    if task != 2:
        with pytest.raises(ValueError, match="cutpoints apply to ordered probit"):
            d.crps(samples, task, y, precisions=prec, cutpoints=np.zeros((3, 1)))
    else:
        with pytest.raises(ValueError, match="integers in"):
            d.crps(samples, task, np.full(5, float(N_CLASS)), **kw)
        with pytest.raises(ValueError, match="finite and ascending"):
            d.crps(samples, task, y, cutpoints=cut[:, ::-1])
    if task == 1:
        with pytest.raises(ValueError, match="0 or 1"):
            d.crps(samples, task, np.full(5, 2.0))
    # ... and a valid call still runs on this design afterwards
    got = d.crps(samples, task, y, **kw)
    check_against_reference(kind, got, np.stack([d.predict([s], 0) for s in samples]), y, prec, cut)
    d.close()


def test_a_wavefront_of_mixed_labels():
    """ordered probit, 5 classes, 64 consecutive rows whose labels cycle 0 1 2 3 4: every lane of the wavefront takes its own
    side of every cut"""
    X, rels, lat = make_data(False)
    est = fit("ordered", X, rels, targets("ordered", lat))
    rows, y = X[:64], (np.arange(64) % N_CLASS).astype(np.float64)
    _, cut = constants("ordered", est)
    check_against_reference("ordered", est.predict_crps(rows, y), device_scores(rows, [], host_samples(est)), y, None, cut)


def test_one_kept_sample_and_no_rows():
    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat, n_kept=1, n_iter=3)
    assert len(est.predictor_.samples) == 1
    got = est.predict_crps(X, lat)
    prec, _ = constants("regressor", est)
    # one normal: the spread is sigma / sqrt(pi) for every row, from the table's diagonal entry alone
    assert np.all(np.abs(got.spread - 1.0 / np.sqrt(np.pi * prec[0])) <= 4 * np.finfo(np.float64).eps)
    check_against_reference("regressor", got, device_scores(X, [], host_samples(est)), lat, prec, None)
    none = est.predict_crps(X[:0], lat[:0])  # N = 0 through the estimator
    assert none.crps.shape == none.accuracy.shape == none.spread.shape == (0,)


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_no_rows(kind):
    from myfm_amd import _capi

    rows, samples, y, prec, cut = random_call(kind, 3, 4, 2)
    d = _capi.Design(rows[:0])
    got = d.crps(samples, TASK[kind], y[:0], precisions=prec, cutpoints=cut)
    assert all(o.shape == (0,) for o in got)
    d.close()


# N = 130: three wavefronts, the last one partial. Regression: S at CRPS_BLOCK - 1, CRPS_BLOCK and CRPS_BLOCK + 1 (the diagonal block alone;
# a full block; a full block and a partial one), S = 33 and 257 (many blocks, the last one of one sample). Ordered probit: the
# cutpoints are staged in LDS while they fit 48 KB = 6144 doubles -- S = 600 with 4 cutpoints: 2400 doubles, staged; with 11: 6600, global.
@pytest.mark.parametrize("kind,S,n_cut", [("regressor", CRPS_BLOCK - 1, 0), ("regressor", CRPS_BLOCK, 0), ("regressor", CRPS_BLOCK + 1, 0),
                                          ("regressor", 33, 0), ("regressor", 257, 0), ("classifier", 33, 0), ("ordered", 600, 4),
                                          ("ordered", 600, 11)])
def test_host_samples_at_the_block_and_staging_boundaries(kind, S, n_cut):
    from myfm_amd import _capi

    N = 130
    rows, samples, y, prec, cut = random_call(kind, S, N, S + n_cut, n_cut=max(n_cut, 1))
    if kind == "ordered":
        assert (S * n_cut * 8 <= 48 * 1024) == (n_cut == 4)
    d = _capi.Design(rows)
    f = np.stack([d.predict([s], 0) for s in samples])
    got = d.crps(samples, TASK[kind], y, precisions=prec, cutpoints=cut)
    assert same(got, d.crps(samples, TASK[kind], y, precisions=prec, cutpoints=cut, tile_rows=64, chunk_samples=97))
    d.close()
    check_against_reference(kind, got, f, y, prec, cut)


def test_the_sample_limit_is_regressions_alone():
    """S = 1024 on 5 rows runs (524 800 pair terms a row); 1025 is refused for regression and runs for ordered probit"""
    from myfm_amd import _capi

    rows, samples, y, prec, cut = random_call("regressor", 1025, 5, 77)
    d = _capi.Design(rows)
    f = np.stack([d.predict([s], 0) for s in samples])
    with pytest.raises(ValueError, match="at most 1024 samples, got 1025"):
        d.crps(samples, 0, y, precisions=prec)
    got = d.crps(samples[:1024], 0, y, precisions=prec[:1024])
    check_against_reference("regressor", got, f[:1024], y, prec[:1024], None)
    rng = np.random.default_rng(78)
    cut = cr.spaced_cutpoints(rng, 1025, 2)
    labels = rng.integers(0, 3, size=5).astype(np.float64)
    check_against_reference("ordered", d.crps(samples, 2, labels, cutpoints=cut), f, labels, None, cut)
    d.close()


def test_a_folded_in_regressor_answers_for_a_new_user():
    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat)
    rng = np.random.default_rng(9)
    items = rng.permutation(N_ITEMS)[:4]
    folded = est.fold_in(onehot(N_USERS + items), rng.normal(size=4), np.zeros(4, dtype=np.int64), 0)
    query = onehot(np.stack([np.full(3, D), N_USERS + rng.permutation(N_ITEMS)[:3]], axis=1), D + 1)  # the new user's column, an item
    y = rng.normal(size=3)
    got = folded.predict_crps(query, y)
    assert got.crps.shape == (3,)
    prec, _ = constants("regressor", folded)
    check_against_reference("regressor", got, device_scores(query, [], host_samples(folded)), y, prec, None)
