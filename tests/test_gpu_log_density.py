"""predict_log_density on the device against the NumPy / SciPy reference of tests/logdens_ref.py.

The per-sample scores (S, N) the reference starts from are taken from the existing single-sample scorer (mfm_design_predict, one
sample, mode 0), so the comparison isolates the new kernel. Two log densities a, b are compared by |a - b| / max(1, |b|) <=
LOGDENS_RTOL (logdens_ref.py, where the constant is derived); with a relation-block design |dl/df| ulp(f) is added for a last-bit
difference of the score. lpd and log_lik_mean are 1-Lipschitz in the sup norm of a row's l and take the same bound; the variance
takes the bound that follows from it (var_bound); pit is compared at rtol 1e-13 (the rounding of z = (y - f) sqrt(alpha), |z| < 20,
in Phi's tail) with atol 1e-16."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.special import log_ndtr, logsumexp

from tests import logdens_ref as lr

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_ROWS, RANK, N_KEPT, N_CLASS = 40, 30, 600, 3, 4, 5
D = N_USERS + N_ITEMS
TASK = {"regressor": 0, "classifier": 1, "ordered": 2}
EPS = np.finfo(np.float64).eps


def onehot(cols, width=D):
    cols = np.asarray(cols, dtype=np.int32).reshape(len(cols), -1)
    n, m = cols.shape
    X = sps.csr_matrix((np.ones(n * m), cols.ravel(), np.arange(0, n * m + 1, m, dtype=np.int64)), shape=(n, width))
    X.sort_indices()
    return X


def same(a, b):
    """two result tuples are equal bit for bit (None where the other has None)"""
    a, b = tuple(a), tuple(b)
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and x.shape == y.shape and np.array_equal(x, y))
                                    for x, y in zip(a, b))


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


def dl_df(kind, ll, f, y, prec, cut):
    """|dl/df| (S, N): how far a last-bit difference of the score moves l"""
    if kind == "regressor":
        return prec[:, None] * np.abs(y[None, :] - f)
    phi = lambda t: np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi)  # noqa: E731
    if kind == "classifier":
        return phi(f) / np.exp(ll)
    ext = np.concatenate([np.full((cut.shape[0], 1), -np.inf), cut, np.full((cut.shape[0], 1), np.inf)], axis=1)
    lab = y.astype(np.int64)
    return np.abs(phi(ext[:, lab + 1] - f) - phi(ext[:, lab] - f)) / np.exp(ll)


def var_bound(ll, e):
    """|var' - var| when every l of a row moves by at most e: each deviation from the mean moves by at most 2 e, so
    |d var| <= (4 e sum_s |d_s| + 4 e^2 S) / (S - 1) <= 4 e sd sqrt(S / (S - 1)) + 4 e^2 S / (S - 1)"""
    S = ll.shape[0]
    if S == 1:
        return np.zeros(ll.shape[1])
    sd = ll.std(axis=0, ddof=1)
    return 4 * e * sd * np.sqrt(S / (S - 1)) + 4 * e * e * S / (S - 1)


def check_against_reference(kind, got, f, y, prec, cut, block=False):
    """all five outputs of `got` (pointwise=True) against the reference on the scores f"""
    y = np.asarray(y, dtype=np.float64)
    ll = lr.log_lik(f, y, TASK[kind], prec, cut)
    lpd, mean, var, pit = lr.summarise(ll, f, y, prec)
    tol = lr.LOGDENS_RTOL * np.maximum(1.0, np.abs(ll))  # absolute, per value
    if block:
        tol = tol + dl_df(kind, ll, f, y, prec, cut) * np.spacing(np.abs(f))
    assert got.log_lik.shape == ll.shape and np.all(np.isfinite(got.log_lik))
    assert np.all(np.abs(got.log_lik - ll) <= tol)
    e = tol.max(axis=0)
    assert np.all(np.abs(got.lpd - lpd) <= e + 8 * EPS * np.maximum(1.0, np.abs(lpd)))
    assert np.all(np.abs(got.log_lik_mean - mean) <= e + 8 * EPS * np.abs(ll).max(axis=0))
    assert np.all(np.abs(got.log_lik_var - var) <= var_bound(ll, e) + 64 * EPS * np.maximum(var, EPS))
    if kind == "regressor":
        np.testing.assert_allclose(got.pit, pit, rtol=1e-13, atol=1e-16)
    else:
        assert got.pit is None


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
    """the three tiny models of test_gpu_binding_sources.py (40 x 30 one-hot, 600 rows, rank 3, 4 kept of 8 iterations), and the
    same three with the items in a relation block; the per-sample scores of the fit's rows, computed once"""
    kind, block = request.param
    X, rels, lat = make_data(block)
    y = targets(kind, lat)
    est = fit(kind, X, rels, y)
    assert est.predictor_.resident and len(est.predictor_.samples) == N_KEPT
    prec, cut = constants(kind, est)
    return dict(kind=kind, block=block, est=est, X=X, rels=rels, y=np.asarray(y, dtype=np.float64), prec=prec, cut=cut,
                f=device_scores(X, rels, host_samples(est)))


def test_all_outputs_match_the_reference(fitted):
    from myfm_amd import PointwiseDensity

    m = fitted
    got = m["est"].predict_log_density(m["X"], m["y"], m["rels"], pointwise=True)
    assert isinstance(got, PointwiseDensity) and got.lpd.shape == (N_ROWS,) and got.log_lik.shape == (N_KEPT, N_ROWS)
    check_against_reference(m["kind"], got, m["f"], m["y"], m["prec"], m["cut"], m["block"])
    lean = m["est"].predict_log_density(m["X"], m["y"], m["rels"])
    assert lean.log_lik is None and same(tuple(lean)[:4], tuple(got)[:4])  # KEEP changes nothing but the matrix


def test_outputs_are_consistent_with_the_returned_matrix(fitted):
    m = fitted
    got = m["est"].predict_log_density(m["X"], m["y"], m["rels"], pointwise=True)
    ll = got.log_lik
    S = ll.shape[0]
    peak = np.abs(ll).max(axis=0)
    # the streaming log-sum-exp adds S terms and three more roundings at the magnitude of the largest |l|
    assert np.all(np.abs(got.lpd - (logsumexp(ll, axis=0) - np.log(S))) <= (S + 8) * EPS * np.maximum(1.0, peak))
    assert np.all(np.abs(got.log_lik_mean - ll.mean(axis=0)) <= 4 * np.spacing(peak))
    if m["kind"] == "classifier":
        proba = m["est"].predict_proba(m["X"], m["rels"])
        ones = m["est"].predict_log_density(m["X"], np.ones(N_ROWS), m["rels"])
        np.testing.assert_allclose(np.exp(ones.lpd), proba, rtol=1e-12, atol=0)


def test_the_pickle_round_trip_gives_the_same_bits(fitted):
    """the resident store read in place and the restored model's host samples, packed for the call"""
    m = fitted
    restored = pickle.loads(pickle.dumps(m["est"]))
    assert not restored.predictor_.resident
    rows, y = m["X"][:257], m["y"][:257]
    rels = [type(r)(np.asarray(r.original_to_block_array)[:257], r.data) for r in m["rels"]]
    assert same(m["est"].predict_log_density(rows, y, rels, pointwise=True), restored.predict_log_density(rows, y, rels, pointwise=True))


def test_tilings_do_not_change_a_bit(fitted):
    """N = 257 through _capi: tile_rows 64 (last tile 1 row), 257, 1; chunk_samples 1, 3 (ragged over the 4 samples); the host
    flavour and the store; the pointwise matrix included"""
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
    kw = dict(precisions=m["prec"], cutpoints=m["cut"], pointwise=True)
    want = st.log_density(d, task, y, **kw)
    assert want[4].shape == (N_KEPT, 257) and (want[3] is None) == (task != 0)
    assert same(want, d.log_density(samples, task, y, **kw))
    for tile_rows in (64, 257, 1):
        for chunk_samples in (1, 3):
            assert same(want, st.log_density(d, task, y, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (tile_rows, chunk_samples)
    assert same(want, d.log_density(samples, task, y, tile_rows=64, chunk_samples=3, **kw))
    assert same(want[:4], st.log_density(d, task, y, precisions=m["prec"], cutpoints=m["cut"], tile_rows=64)[:4])
    part = st.log_density(d, task, y, first=1, count=3, precisions=None if m["prec"] is None else m["prec"][1:],
                          cutpoints=None if m["cut"] is None else m["cut"][1:], pointwise=True)
    assert np.array_equal(part[4], want[4][1:])
    st.close()
    d.close()


def spaced_cutpoints(rng, S, n_cut):
    """(S, n_cut) ascending cutpoints with spacings in [0.05, 0.8]: LOGDENS_RTOL holds for intervals of 1e-3 and wider (the
    reference's own two-term form cancels below that, see logdens_ref.value_grid)"""
    return -2.0 + rng.normal(size=(S, 1)) * 0.5 + np.cumsum(rng.uniform(0.05, 0.8, size=(S, n_cut)), axis=1)


def random_call(kind, S, N, seed):
    """(rows, samples, y, precisions, cutpoints) of a valid call on random host samples: no fit"""
    rng = np.random.default_rng(seed)
    n_cut = N_CLASS - 1
    rows = onehot(np.stack([rng.integers(0, N_USERS, size=N), N_USERS + rng.integers(0, N_ITEMS, size=N)], axis=1).reshape(N, 2))
    samples = [(0.1 * rng.normal(), rng.normal(size=D) * 0.5, rng.normal(size=(D, RANK)) * 0.5) for _ in range(S)]
    prec = np.exp(rng.uniform(-1.0, 2.0, size=S)) if kind == "regressor" else None
    cut = spaced_cutpoints(rng, S, n_cut) if kind == "ordered" else None
    y = {"regressor": rng.normal(size=N), "classifier": (rng.random(N) < 0.5).astype(np.float64),
         "ordered": rng.integers(0, n_cut + 1, size=N).astype(np.float64)}[kind]
    return rows, samples, y, prec, cut


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_the_library_refuses_before_it_computes(kind):
    """the checks of the C entry points, those that the binding cannot reach among them (it allocates pit by the task itself)"""
    import ctypes as C

    from myfm_amd import _capi

    task = TASK[kind]
    rows, samples, y, prec, cut = random_call(kind, 3, 5, 1)
    d = _capi.Design(rows)
    kw = dict(precisions=prec, cutpoints=cut)
    with pytest.raises(ValueError, match="negative tiling"):
        d.log_density(samples, task, y, tile_rows=-1, **kw)
    with pytest.raises(ValueError, match="bad task"):
        d.log_density(samples, 3, y, **kw)
    with pytest.raises(ValueError, match="finite"):
        d.log_density(samples, task, np.array([np.nan] + list(y[1:])), **kw)
    narrow = _capi.Store(D - 1, RANK)  # a store of another feature size
    for w0, w, V in samples:
        narrow.push(w0, w[:-1], V[:-1])
    with pytest.raises(ValueError, match="feature size mismatch"):
        narrow.log_density(d, task, y, **kw)
    narrow.close()
    if task != 0:
        with pytest.raises(ValueError, match="regression"):
            d.log_density(samples, task, y, precisions=np.ones(3), cutpoints=cut)
        K, S, w0s, ws, Vs = _capi._pack_samples(samples)
        out = [np.empty(5) for _ in range(4)]
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = _capi.lib().mfm_design_logdens(d.h, K, S, p(w0s), p(ws), p(Vs), task, p(y), None, 0 if cut is None else cut.shape[1], p(cut),
                                            0, 0, p(out[0]), p(out[1]), p(out[2]), p(out[3]), None)
        assert rc == _capi.MFM_ERR_INVALID and b"regression" in _capi.lib().mfm_design_last_error(d.h)
    else:
        with pytest.raises(ValueError, match="needs the noise precision"):
            d.log_density(samples, task, y)
    if task != 2:
        with pytest.raises(ValueError, match="ordered probit"):
            d.log_density(samples, task, y, precisions=prec, cutpoints=np.zeros((3, 1)))
    else:
        with pytest.raises(ValueError, match="integers in"):
            d.log_density(samples, task, np.full(5, float(N_CLASS)), **kw)
        with pytest.raises(ValueError, match="finite and ascending"):
            d.log_density(samples, task, y, cutpoints=cut[:, ::-1])
    if task == 1:
        with pytest.raises(ValueError, match="0 or 1"):
            d.log_density(samples, task, np.full(5, 2.0))
    # ... and a valid call still runs on this design afterwards
    assert np.all(np.isfinite(d.log_density(samples, task, y, **kw)[0]))
    d.close()


def test_a_wavefront_of_mixed_labels():
    """ordered probit, 5 classes, 64 consecutive rows whose labels cycle 0 1 2 3 4: every lane of the wavefront takes another
    class, the one-sided ones included"""
    X, rels, lat = make_data(False)
    est = fit("ordered", X, rels, targets("ordered", lat))
    rows, y = X[:64], (np.arange(64) % N_CLASS).astype(np.float64)
    _, cut = constants("ordered", est)
    got = est.predict_log_density(rows, y, pointwise=True)
    check_against_reference("ordered", got, device_scores(rows, [], host_samples(est)), y, None, cut)


def restored_with_w0(est, kind, w0s):
    """the model rebuilt from its state with the samples' w0 replaced: host samples"""
    from myfm_amd import _myfm

    fms = []
    for fm, w0 in zip(est.predictor_.samples, w0s):
        new = _myfm.FM.__new__(_myfm.FM)
        new.__setstate__((float(w0), np.asarray(fm.w), np.asarray(fm.V), [np.asarray(c) for c in fm.cutpoints]))
        fms.append(new)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((RANK, D, TASK[kind], fms))
    out = type(est)(RANK)
    out.predictor_ = p
    return out


@pytest.mark.parametrize("w0", [40.0, -40.0])
def test_classifier_tails_stay_finite(w0):
    """scores near +-40, where Phi underflows: lpd is finite and equals log_ndtr within the tolerance, for both labels"""
    X, rels, lat = make_data(False)
    est = restored_with_w0(fit("classifier", X, rels, targets("classifier", lat)), "classifier", [w0] * N_KEPT)
    rows = X[:130]
    f = device_scores(rows, [], host_samples(est))
    assert np.abs(f).min() > 30.0
    for label in (1.0, 0.0):
        y = np.full(130, label)
        got = est.predict_log_density(rows, y, pointwise=True)
        assert np.all(np.isfinite(got.lpd)) and np.all(np.isfinite(got.log_lik))
        assert np.all(lr.deviation(got.log_lik, log_ndtr(f if label else -f)) <= lr.LOGDENS_RTOL)
        check_against_reference("classifier", got, f, y, None, None)


def test_ordered_top_label_far_below_the_cutpoints():
    """every score 30 and more below the lowest cutpoint, asked for the top label: log(1 - Phi(cut - f)) without forming Phi"""
    X, rels, lat = make_data(False)
    fitted_est = fit("ordered", X, rels, targets("ordered", lat))
    _, cut = constants("ordered", fitted_est)
    est = restored_with_w0(fitted_est, "ordered", [cut.min() - 36.0] * N_KEPT)
    rows = X[:130]
    f = device_scores(rows, [], host_samples(est))
    assert (cut.min() - f).min() >= 30.0
    y = np.full(130, N_CLASS - 1.0)
    got = est.predict_log_density(rows, y, pointwise=True)
    assert np.all(np.isfinite(got.lpd)) and np.all(got.lpd < -400.0)
    check_against_reference("ordered", got, f, y, None, cut)


def test_one_kept_sample():
    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat, n_kept=1, n_iter=3)
    assert len(est.predictor_.samples) == 1
    got = est.predict_log_density(X, lat, pointwise=True)
    assert np.array_equal(got.log_lik_var, np.zeros(N_ROWS)) and not np.signbit(got.log_lik_var).any()
    assert np.array_equal(got.lpd, got.log_lik_mean) and np.array_equal(got.lpd, got.log_lik[0])
    prec, _ = constants("regressor", est)
    check_against_reference("regressor", got, device_scores(X, [], host_samples(est)), lat, prec, None)
    none = est.predict_log_density(X[:0], lat[:0], pointwise=True)  # N = 0 through the estimator
    assert none.lpd.shape == none.pit.shape == (0,) and none.log_lik.shape == (1, 0)


# The per-sample constants are staged in LDS while they fit 48 KB = 6144 doubles, and read from global memory beyond:
#   ordered, S = 600, 4 cutpoints:   2400 doubles, staged      ordered, S = 600, 11 cutpoints:  6600 doubles, global
#   regression, S = 600:             1200 doubles, staged      regression, S = 3100:            6200 doubles, global
@pytest.mark.parametrize("kind,S,n_cut", [("ordered", 600, 4), ("ordered", 600, 11), ("regressor", 600, 0), ("regressor", 3100, 0)])
def test_many_host_samples_on_both_sides_of_the_staging_boundary(kind, S, n_cut):
    from myfm_amd import _capi

    rng = np.random.default_rng(S + n_cut)
    N = 130  # three wavefronts, the last one partial
    rows = onehot(np.stack([rng.integers(0, N_USERS, size=N), N_USERS + rng.integers(0, N_ITEMS, size=N)], axis=1))
    samples = [(0.1 * rng.normal(), rng.normal(size=D) * 0.5, rng.normal(size=(D, RANK)) * 0.5) for _ in range(S)]
    prec = np.exp(rng.uniform(-1.0, 2.0, size=S)) if kind == "regressor" else None
    cut = spaced_cutpoints(rng, S, n_cut) if kind == "ordered" else None
    y = rng.normal(size=N) if kind == "regressor" else rng.integers(0, n_cut + 1, size=N).astype(np.float64)
    n_aux = 2 * S if kind == "regressor" else S * n_cut
    assert (n_aux * 8 <= 48 * 1024) == ((kind, S, n_cut) in (("ordered", 600, 4), ("regressor", 600, 0)))
    d = _capi.Design(rows)
    f = np.stack([d.predict([s], 0) for s in samples])
    from myfm_amd import PointwiseDensity

    got = PointwiseDensity(*d.log_density(samples, TASK[kind], y, precisions=prec, cutpoints=cut, pointwise=True))
    assert same(got, d.log_density(samples, TASK[kind], y, precisions=prec, cutpoints=cut, pointwise=True, tile_rows=64, chunk_samples=97))
    d.close()
    check_against_reference(kind, got, f, y, prec, cut)


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_no_rows(kind):
    from myfm_amd import _capi

    rows, samples, y, prec, cut = random_call(kind, 3, 4, 2)
    d = _capi.Design(rows[:0])
    lpd, mean, var, pit, ll = d.log_density(samples, TASK[kind], y[:0], precisions=prec, cutpoints=cut, pointwise=True)
    assert lpd.shape == mean.shape == var.shape == (0,) and ll.shape == (3, 0) and (pit is None) == (kind != "regressor")
    d.close()


def test_a_folded_in_regressor_answers_for_a_new_user():
    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat)
    rng = np.random.default_rng(9)
    items = rng.permutation(N_ITEMS)[:4]
    folded = est.fold_in(onehot(N_USERS + items), rng.normal(size=4), np.zeros(4, dtype=np.int64), 0)
    query = onehot(np.stack([np.full(3, D), N_USERS + rng.permutation(N_ITEMS)[:3]], axis=1), D + 1)  # the new user's column, an item
    y = rng.normal(size=3)
    got = folded.predict_log_density(query, y, pointwise=True)
    assert got.lpd.shape == (3,) and np.all(np.isfinite(got.lpd)) and np.all((got.pit > 0) & (got.pit < 1))
    prec, _ = constants("regressor", folded)
    check_against_reference("regressor", got, device_scores(query, [], host_samples(folded)), y, prec, None)
