"""predict_loo_dist and predict_loo_crps on the device against the NumPy reference of tests/loo_pred_ref.py.

The reference is fed the device's own per-sample scores (the single-sample scorer, mfm_design_predict) and the device's own
predict_loo(log_weights=True) weights, so the comparison isolates the new third stage. Two values are compared by |a - b| /
max(1, |b|) against the bounds of loo_pred_ref.py (8 x the measured deviation of the reference from its twin); with a
relation-block design 2 max_s ulp(score_s) is added per row for a last-bit difference of the scores (every value and every CRPS term
moves by less than the score does, a weighted mean or a quantile by no more than its values). A quantile cell within NEAR of a
running sum is left out, at most 1 % of a case's cells. pareto_k equals predict_loo's bit for bit.

LOO_CRPS_BLOCK = 4 is the register block of k_row_loo_crps_mix (csrc/mfm_loo_pred.hpp): the host-sample cases run S = 1 .. 5 around it."""
import pickle

import numpy as np
import pytest

from tests import loo_pred_ref as lr
from tests.test_gpu_log_density import (D, N_ITEMS, N_ROWS, N_USERS, RANK, TASK, capi_blocks, constants, device_scores, fit, host_samples,
                                        make_data, onehot, same, targets)
from tests.test_gpu_loo import N_KEPT, synthetic_call

pytestmark = pytest.mark.gpu

Q = np.asarray(lr.QUANTILES)


def check_summary(task, got, f, lw, prec, cut, quantiles=Q, block=False):
    """(mean, std, quantiles, std_y, ess) of `got` against the reference on the scores f (S, N) and the log weights lw (S, N)"""
    want = lr.summary(lr.values(task, f, cut), lw, quantiles, None if prec is None else 1.0 / prec)
    extra = 2 * np.spacing(np.abs(f)).max(axis=0) if block else 0.0
    assert (got[3] is None) == (task != 0)
    rtol = lr.rtol_moments(f.shape[0])
    for name, i in (("mean", 0), ("std", 1), ("std_y", 3), ("ess", 4)):
        if got[i] is None:
            continue
        a, b = got[i], want[i]
        assert a.shape == b.shape and np.all(np.isfinite(a)), name
        dev = (np.abs(a - b) - extra) / np.maximum(1.0, np.abs(b))
        print("task %d %s S=%d N=%d: worst deviation %.3e (bound %.3e)" % (task, name, f.shape[0], f.shape[1], dev.max(), rtol))
        assert np.all(dev <= rtol), name
    a, b, keep = got[2], want[2], ~want[5]
    assert a.shape == b.shape == (len(quantiles), f.shape[1]) and np.all(np.isfinite(a))
    if keep.size:
        assert 1.0 - keep.mean() <= lr.MAX_LEFT_OUT
        dev = (np.abs(a - b) - extra) / np.maximum(1.0, np.abs(b))
        print("task %d quantiles S=%d N=%d: worst deviation %.3e (bound %.3e), %d cells left out"
              % (task, f.shape[0], f.shape[1], dev[keep].max(), lr.LOO_RTOL_QUANTILES, (~keep).sum()))
        assert np.all(dev[keep] <= lr.LOO_RTOL_QUANTILES)


def check_crps(task, got, f, lw, y, prec, cut, block=False):
    want = lr.crps(task, f, lw, np.asarray(y, dtype=np.float64), prec, cut)
    extra = 2 * np.spacing(np.abs(f)).max(axis=0) if block else 0.0
    for name, a, b in zip(("crps", "accuracy", "spread"), got, want):
        assert a.shape == b.shape and np.all(np.isfinite(a)), name
        dev = (np.abs(a - b) - extra) / np.maximum(1.0, np.abs(b))
        print("task %d %s S=%d N=%d: worst deviation %.3e (bound %.3e)" % (task, name, f.shape[0], f.shape[1], dev.max(), lr.LOO_RTOL_CRPS))
        assert np.all(dev <= lr.LOO_RTOL_CRPS), name
    assert np.all(got[0] >= 0)


@pytest.fixture(scope="module", params=[(k, b) for b in (False, True) for k in ("regressor", "classifier", "ordered")],
                ids=lambda p: p[0] + ("-block" if p[1] else ""))
def fitted(request):
    """the tiny models of test_gpu_loo.py (40 x 30 one-hot, 600 rows, rank 3, 32 samples kept of 40 iterations); the device's own
    scores and leave-one-out weights of the fit's rows, computed once"""
    kind, block = request.param
    X, rels, lat = make_data(block)
    y = np.asarray(targets(kind, lat), dtype=np.float64)
    est = fit(kind, X, rels, y, n_kept=N_KEPT, n_iter=40)
    assert est.predictor_.resident and len(est.predictor_.samples) == N_KEPT
    prec, cut = constants(kind, est)
    loo = est.predict_loo(X, y, rels, log_weights=True)
    f = device_scores(X, rels, host_samples(est))
    return dict(kind=kind, block=block, est=est, X=X, rels=rels, y=y, prec=prec, cut=cut, loo=loo, f=f)


def test_all_outputs_match_the_reference(fitted):
    from myfm_amd import LooCrps, LooPredictive
    from myfm_amd.utils import evaluation as ev

    m = fitted
    task = TASK[m["kind"]]
    ok = np.isfinite(m["loo"].elpd_loo)
    assert ok.all()  # (no row of these models has a density of 0)
    got = m["est"].predict_loo_dist(m["X"], m["y"], m["rels"], quantiles=Q)
    assert isinstance(got, LooPredictive) and got.mean.shape == (N_ROWS,) and got.quantiles.shape == (len(Q), N_ROWS)
    assert np.array_equal(got.pareto_k, m["loo"].pareto_k)
    check_summary(task, got, m["f"], m["loo"].log_weights, m["prec"], m["cut"], block=m["block"])
    if task == 0:  # the mean is sum w score, from the weights the caller can have
        w = np.exp(m["loo"].log_weights)
        direct = np.cumsum(w * m["f"], axis=0)[-1]
        extra = 2 * np.spacing(np.abs(m["f"])).max(axis=0) if m["block"] else 0.0
        assert np.all(np.abs(got.mean - direct) - extra <= lr.LOO_RTOL_MOMENTS * np.maximum(1.0, np.abs(direct)))
        res = ev.loo_residuals(got, m["y"], interval=(2, 1))  # the 5 % and the 95 % quantile of the score (not of y: no noise in them)
        assert 0.0 <= res["coverage"] <= 1.0 and res["r2"] < 1.0 and res["standardized"].shape == (N_ROWS,)
    assert np.all(got.quantiles[2] <= got.quantiles[3]) and np.all(got.quantiles[3] <= got.quantiles[0]) and np.all(got.quantiles[0] <= got.quantiles[1])
    assert np.all((got.ess >= 1.0 - 1e-12) & (got.ess <= N_KEPT * (1 + 1e-12)))
    lean = m["est"].predict_loo_dist(m["X"], m["y"], m["rels"], quantiles=())  # no sort: the same moments
    assert lean.quantiles.shape == (0, N_ROWS) and same((lean.mean, lean.std, lean.std_y, lean.ess, lean.pareto_k),
                                                        (got.mean, got.std, got.std_y, got.ess, got.pareto_k))
    crps = m["est"].predict_loo_crps(m["X"], m["y"], m["rels"])
    assert isinstance(crps, LooCrps) and np.array_equal(crps.pareto_k, m["loo"].pareto_k)
    check_crps(task, crps[:3], m["f"], m["loo"].log_weights, m["y"], m["prec"], m["cut"], m["block"])
    assert ev.crps_summary(crps)["crps"] == float(np.mean(crps.crps))
    if m["kind"] == "ordered":
        assert same(tuple(got), tuple(m["est"].predict_loo_dist(m["X"], m["y"], m["rels"], quantiles=Q, cutpoint_index=0)))


def capi_case(kind, S, N, seed, n_cut=None):
    """a design on random host samples, its scores and its leave-one-out log weights"""
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call(kind, S, N, seed)
    if kind == "ordered" and n_cut is not None:
        cut = cut[:, :n_cut]
        y = np.minimum(y, n_cut)
    d = _capi.Design(rows)
    kw = dict(precisions=prec, cutpoints=cut)
    lw = d.loo(samples, TASK[kind], y, log_weights=True, **kw)
    f = np.stack([d.predict([s], 0) for s in samples]) if S <= 200 else None
    return d, samples, y, prec, cut, kw, lw, f


# S = 1 .. 5 around the register block; 20 and 21: the last S without and the first with a fitted tail; 33, 95, 200: P = 64, 128, 256
# N = 1, 63, 64, 65, 257: rows around a wavefront and a workgroup of the row-per-thread kernels, and around the R rows of the LDS form
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 20, 21, 33, 95, 200])
def test_the_c_abi_on_synthetic_host_samples(S, N):
    for kind in ("regressor", "classifier", "ordered"):
        for n_cut in ((1, 4) if kind == "ordered" else (None,)):
            task = TASK[kind]
            d, samples, y, prec, cut, kw, loo, f = capi_case(kind, S, N, 100 * S + N + task, n_cut)
            got = d.loo_summary(samples, task, y, quantiles=Q, **kw)
            assert np.array_equal(got[5], loo[1])
            check_summary(task, got, f, loo[4], prec, cut)
            crps = d.loo_crps(samples, task, y, **kw)
            assert np.array_equal(crps[3], loo[1])
            check_crps(task, crps[:3], f, loo[4], y, prec, cut)
            d.close()


def scores_of(d, samples):
    """(S, N) by the mean scorer over one sample at a time, in chunks that keep the test quick: mode 0 of one sample is its score"""
    return np.stack([d.predict([s], 0) for s in samples])


@pytest.mark.parametrize("kind,S", [("regressor", 1024), ("ordered", 1025), ("regressor", 4096), ("classifier", 4096), ("ordered", 4096)])
def test_the_sample_limits_on_the_device(kind, S):
    """S = 1024: the largest regression CRPS; 1025: ordered probit beyond it; 4096: a summary with quantiles, one row per workgroup
    in 81 944 B of LDS. The scores of that many samples, one scorer call each, are taken for 8 rows only."""
    from myfm_amd import _capi

    task = TASK[kind]
    N = 8
    rows, samples, y, prec, cut = synthetic_call(kind, S, N, 7 * S + task)
    d = _capi.Design(rows)
    kw = dict(precisions=prec, cutpoints=cut)
    loo = d.loo(samples, task, y, log_weights=True, **kw)
    f = scores_of(d, samples)
    if S == 4096 or kind == "ordered":
        got = d.loo_summary(samples, task, y, quantiles=Q, **kw)
        assert np.array_equal(got[5], loo[1])
        check_summary(task, got, f, loo[4], prec, cut)
    if S <= 1025:
        crps = d.loo_crps(samples, task, y, **kw)
        assert np.array_equal(crps[3], loo[1])
        check_crps(task, crps[:3], f, loo[4], y, prec, cut)
    elif kind == "regressor":
        with pytest.raises(ValueError, match="at most 1024 samples, got 4096"):
            d.loo_crps(samples, task, y, **kw)
    d.close()


def test_the_library_refuses_before_it_computes():
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call("classifier", 1, 5, 3)
    d = _capi.Design(rows)
    with pytest.raises(ValueError, match="at most 4096 samples, got 4097"):
        d.loo_summary(samples * 4097, 1, y)
    with pytest.raises(ValueError, match="at most 4096 samples, got 4097"):
        d.loo_crps(samples * 4097, 1, y)
    with pytest.raises(ValueError, match="at most 32 quantiles"):
        d.loo_summary(samples * 3, 1, y, quantiles=np.linspace(0, 1, 33))
    with pytest.raises(ValueError, match="out of range"):
        d.loo_summary(samples * 3, 1, y, quantiles=(0.5, 1.5))
    K, S, w0s, ws, Vs = _capi._pack_samples(samples * 3)
    out = [np.empty(5) for _ in range(4)]
    p = _capi._p
    for tail_len in (-1, 3):
        rc = _capi.lib().mfm_design_loo_crps(d.h, K, S, p(w0s), p(ws), p(Vs), 1, p(y), None, 0, None, 0, 0, tail_len, *[p(o) for o in out])
        assert rc == _capi.MFM_ERR_INVALID and b"tail_len" in _capi.lib().mfm_design_last_error(d.h)
    rc = _capi.lib().mfm_design_loo_summary(d.h, K, S, p(w0s), p(ws), p(Vs), 1, p(y), None, 0, None, 0, 0, 0, 0, None, p(out[0]), p(out[1]), None,
                                            p(out[2]), p(out[3]), p(out[3]))
    assert rc == _capi.MFM_ERR_INVALID and b"regression" in _capi.lib().mfm_design_last_error(d.h)  # std_y of a classifier
    assert np.all(np.isfinite(d.loo_crps(samples * 3, 1, y)[0]))  # ... and a valid call still runs on this design afterwards
    d.close()


def test_tilings_sources_and_the_pickle_round_trip_do_not_change_a_bit(fitted):
    """N = 257 through _capi: tile_rows 7 and chunk_samples 3, the store against host samples; then the unpickled estimator"""
    from myfm_amd import _capi

    m = fitted
    task = TASK[m["kind"]]
    N = 257
    rows, y = m["X"][:N], m["y"][:N]
    rels = [type(r)(np.asarray(r.original_to_block_array)[:N], r.data) for r in m["rels"]]
    samples = host_samples(m["est"])
    d = _capi.Design(rows, [(mp[:N], B) for mp, B in capi_blocks(m["rels"])])
    st = _capi.Store(d.D, RANK)
    for w0, w, V in samples:
        st.push(w0, w, V)
    kw = dict(precisions=m["prec"], cutpoints=m["cut"])
    want_s = st.loo_summary(d, task, y, quantiles=Q, **kw)
    want_c = st.loo_crps(d, task, y, **kw)
    assert same(want_s, d.loo_summary(samples, task, y, quantiles=Q, **kw)) and same(want_c, d.loo_crps(samples, task, y, **kw))
    for tile_rows, chunk_samples in ((7, 3), (64, 0), (0, 3)):
        assert same(want_s, st.loo_summary(d, task, y, quantiles=Q, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (tile_rows, chunk_samples)
        assert same(want_c, st.loo_crps(d, task, y, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (tile_rows, chunk_samples)
    assert same(want_s, d.loo_summary(samples, task, y, quantiles=Q, tile_rows=7, chunk_samples=3, **kw))
    lean = st.loo_summary(d, task, y, tile_rows=7, **kw)  # without quantiles: no sort, the same moments
    assert lean[2].shape == (0, N) and same(want_s[:2] + want_s[3:], lean[:2] + lean[3:])
    st.close()
    d.close()
    restored = pickle.loads(pickle.dumps(m["est"]))
    assert not restored.predictor_.resident
    assert same(want_s, tuple(m["est"].predict_loo_dist(rows, y, rels, quantiles=Q)))
    assert same(want_s, tuple(restored.predict_loo_dist(rows, y, rels, quantiles=Q)))
    assert same(want_c, tuple(restored.predict_loo_crps(rows, y, rels)))
    # predict_loo itself after the new calls on the same predictor: its bits as before
    assert same(tuple(m["loo"]), tuple(m["est"].predict_loo(m["X"], m["y"], m["rels"], log_weights=True)))


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_duplicated_samples_give_the_crps_of_predict_crps(kind):
    """all S samples alike: every weight is 1 / S up to rounding, and the weighted form is predict_crps'"""
    from myfm_amd import _capi

    from tests import crps_ref as cr

    rows, samples, y, prec, cut = synthetic_call(kind, 1, 65, 12)
    S = 24
    kw = dict(precisions=None if prec is None else np.repeat(prec, S), cutpoints=None if cut is None else np.repeat(cut, S, axis=0))
    d = _capi.Design(rows)
    got = d.loo_crps(samples * S, TASK[kind], y, **kw)
    want = d.crps(samples * S, TASK[kind], y, **kw)
    for a, b in zip(got[:3], want):
        assert np.all(cr.deviation(a, b) <= lr.LOO_RTOL_CRPS)
    assert np.all(np.isposinf(got[3]))  # a constant row is not fitted
    d.close()


def test_a_folded_in_regressor_combined_chains_and_no_rows():
    import myfm_amd

    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat, n_kept=N_KEPT, n_iter=40)
    rng = np.random.default_rng(9)
    items = rng.permutation(N_ITEMS)[:4]
    folded = est.fold_in(onehot(N_USERS + items), rng.normal(size=4), np.zeros(4, dtype=np.int64), 0)
    query = onehot(np.stack([np.full(3, D), N_USERS + rng.permutation(N_ITEMS)[:3]], axis=1), D + 1)  # the new user's column, an item
    y = rng.normal(size=3)
    loo = folded.predict_loo(query, y, log_weights=True)
    prec, _ = constants("regressor", folded)
    f = device_scores(query, [], host_samples(folded))
    got = folded.predict_loo_dist(query, y, quantiles=Q)
    assert np.array_equal(got.pareto_k, loo.pareto_k)
    check_summary(0, got, f, loo.log_weights, prec, None)
    check_crps(0, folded.predict_loo_crps(query, y)[:3], f, loo.log_weights, y, prec, None)
    other = myfm_amd.MyFMGibbsRegressor(RANK, random_seed=6).fit(X, lat, n_iter=40, n_kept_samples=N_KEPT, group_shapes=[N_USERS, N_ITEMS])
    both = myfm_amd.combine_chains([est, other])
    loo = both.predict_loo(X[:65], lat[:65], log_weights=True)
    got = both.predict_loo_dist(X[:65], lat[:65], quantiles=Q)
    prec, _ = constants("regressor", both)
    f = device_scores(X[:65], [], host_samples(both))
    assert got.mean.shape == (65,) and np.array_equal(got.pareto_k, loo.pareto_k)
    check_summary(0, got, f, loo.log_weights, prec, None)
    check_crps(0, both.predict_loo_crps(X[:65], lat[:65])[:3], f, loo.log_weights, lat[:65], prec, None)
    none = est.predict_loo_dist(X[:0], lat[:0], quantiles=Q)  # N = 0 through the estimator
    assert none.mean.shape == none.std.shape == none.std_y.shape == none.ess.shape == none.pareto_k.shape == (0,)
    assert none.quantiles.shape == (len(Q), 0)
    none = est.predict_loo_crps(X[:0], lat[:0])
    assert none.crps.shape == none.accuracy.shape == none.spread.shape == none.pareto_k.shape == (0,)
