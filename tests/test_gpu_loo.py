"""predict_loo on the device against the NumPy reference of tests/psis_ref.py.

The reference is fed the device's own predict_log_density(pointwise=True).log_lik, so the comparison isolates the new kernel: the
ratios it sorts are bit for bit the reference's, and the orders agree. elpd_loo and the log weights are compared by
deviation(a, b) = |a - b| / max(1, |b|) <= PSIS_RTOL_ELPD, the finite k by the same form <= PSIS_RTOL_K, infinite k must be infinite
on both sides, lpd equals predict_log_density's bit for bit. Each test also runs the reference in longdouble on its own inputs and
checks that the float64 / longdouble deviation stays within the recorded figures the two tolerances are 8 x of.

loo_pit = sum_s w_s Phi(z_s): a log weight off by e_s = PSIS_RTOL_ELPD max(1, |lw_s|) moves w_s by the factor exp(e_s), Phi(z_s) is
compared at predict_log_density's rtol 1e-13 (atol 1e-16), and the sum of S positive terms in sample order carries S eps:
|d pit| <= sum_s e_s w_s Phi_s + (1e-13 + S eps) pit + 1e-16."""
import pickle

import numpy as np
import pytest

from tests import psis_ref as pr
from tests.test_gpu_log_density import (D, N_CLASS, N_ITEMS, N_ROWS, N_USERS, RANK, TASK, capi_blocks, constants, device_scores, fit, host_samples,
                                        make_data, onehot, same, spaced_cutpoints, targets)

pytestmark = pytest.mark.gpu

N_KEPT = 32  # M = ceil(min(6.4, 17)) = 7: the fit runs
EPS = np.finfo(np.float64).eps


def check_against_reference(got, ll, r_eff=1.0, pit_args=None):
    """elpd_loo, pareto_k and log_weights of `got` against the reference on the log likelihoods ll (S, N); every row is compared"""
    elpd, k, lw = pr.psis(ll, r_eff)
    eL, kL, wL = (np.asarray(v, dtype=np.float64) for v in pr.psis(ll, r_eff, np.longdouble))
    fin = np.isfinite(k)
    assert np.array_equal(fin, np.isfinite(kL)) and np.all(np.isfinite(wL))
    own_e = max(pr.deviation(elpd, eL).max(), pr.deviation(lw, wL).max())
    own_k = pr.deviation(k[fin], kL[fin]).max() if fin.any() else 0.0
    print("float64 / longdouble deviation of the reference on these inputs: elpd and log weights %.3g, k %.3g" % (own_e, own_k))
    assert own_e <= pr.PSIS_MEASURED_DEVIATION_ELPD and own_k <= pr.PSIS_MEASURED_DEVIATION_K
    got_elpd, got_k, got_lw = got[0], got[1], got[4]
    assert got_elpd.shape == elpd.shape and got_k.shape == k.shape and got_lw.shape == lw.shape
    assert np.array_equal(np.isposinf(got_k), ~fin) and np.all(np.isfinite(got_k[fin]))
    print("device / reference: elpd %.3g, log weights %.3g, k %.3g" % (pr.deviation(got_elpd, elpd).max(), pr.deviation(got_lw, lw).max(),
                                                                    pr.deviation(got_k[fin], k[fin]).max() if fin.any() else 0.0))
    assert np.all(pr.deviation(got_elpd, elpd) <= pr.PSIS_RTOL_ELPD)
    assert np.all(pr.deviation(got_lw, lw) <= pr.PSIS_RTOL_ELPD)
    assert np.all(pr.deviation(got_k[fin], k[fin]) <= pr.PSIS_RTOL_K)
    n_compared = int(fin.sum()) + int(np.isposinf(got_k).sum())
    assert n_compared == ll.shape[1]  # the share of rows left out of the comparison is zero
    if pit_args is not None:
        from scipy.special import ndtr

        f, y, prec = pit_args
        S = ll.shape[0]
        phi = ndtr((y[None, :] - f) * np.sqrt(prec)[:, None])
        w = np.exp(lw)
        pit = (w * phi).sum(axis=0)
        bound = (pr.PSIS_RTOL_ELPD * np.maximum(1.0, np.abs(lw)) * w * phi).sum(axis=0) + (1e-13 + S * EPS) * pit + 1e-16
        assert np.all(np.abs(got[3] - pit) <= bound)
        assert np.all((got[3] >= 0.0) & (got[3] <= 1.0 + S * EPS))
    else:
        assert got[3] is None
    return fin


@pytest.fixture(scope="module", params=[(k, b) for b in (False, True) for k in ("regressor", "classifier", "ordered")],
                ids=lambda p: p[0] + ("-block" if p[1] else ""))
def fitted(request):
    """the tiny models of test_gpu_log_density.py (40 x 30 one-hot, 600 rows, rank 3) with 32 samples kept of 40 iterations; the
    device's own log likelihoods of the fit's rows and, for the pit, the per-sample scores, computed once"""
    kind, block = request.param
    X, rels, lat = make_data(block)
    y = np.asarray(targets(kind, lat), dtype=np.float64)
    est = fit(kind, X, rels, y, n_kept=N_KEPT, n_iter=40)
    assert est.predictor_.resident and len(est.predictor_.samples) == N_KEPT
    prec, cut = constants(kind, est)
    density = est.predict_log_density(X, y, rels, pointwise=True)
    f = device_scores(X, rels, host_samples(est)) if kind == "regressor" else None
    return dict(kind=kind, block=block, est=est, X=X, rels=rels, y=y, prec=prec, cut=cut, density=density, f=f)


def test_all_outputs_match_the_reference(fitted):
    from myfm_amd import LooDensity
    from myfm_amd.utils import evaluation as ev

    m = fitted
    got = m["est"].predict_loo(m["X"], m["y"], m["rels"], log_weights=True)
    assert isinstance(got, LooDensity) and got.elpd_loo.shape == (N_ROWS,) and got.log_weights.shape == (N_KEPT, N_ROWS)
    assert np.array_equal(got.lpd, m["density"].lpd)
    fin = check_against_reference(got, m["density"].log_lik, 1.0, (m["f"], m["y"], m["prec"]) if m["kind"] == "regressor" else None)
    assert fin.sum() > N_ROWS // 2  # (the fit ran on most rows)
    lean = m["est"].predict_loo(m["X"], m["y"], m["rels"])
    assert lean.log_weights is None and same(tuple(lean)[:4], tuple(got)[:4])  # KEEP_W changes nothing but the matrix
    out = ev.loo(got, N_KEPT)
    assert np.isfinite(out["elpd_loo"]) and out["p_loo"] > 0.0 and out["elpd_loo"] < m["density"].lpd.sum()
    if m["kind"] == "regressor":
        counts, _ = ev.pit_histogram(got.loo_pit)
        assert counts.sum() == N_ROWS


def synthetic_call(kind, S, N, seed):
    """(rows, samples, y, precisions, cutpoints) of a valid call on random host samples of rank 2: no fit"""
    rng = np.random.default_rng(seed)
    n_cut = N_CLASS - 1
    rows = onehot(np.stack([rng.integers(0, N_USERS, size=N), N_USERS + rng.integers(0, N_ITEMS, size=N)], axis=1).reshape(N, 2))
    mean = (0.1, rng.normal(size=D) * 0.5, rng.normal(size=(D, 2)) * 0.5)  # a posterior around one model, 0.15 wide
    samples = [(mean[0] + 0.15 * rng.normal(), mean[1] + 0.15 * rng.normal(size=D), mean[2] + 0.15 * rng.normal(size=(D, 2))) for _ in range(S)]
    prec = np.exp(rng.uniform(-0.5, 0.5, size=S)) if kind == "regressor" else None
    cut = spaced_cutpoints(rng, S, n_cut) if kind == "ordered" else None
    y = {"regressor": rng.normal(size=N), "classifier": (rng.random(N) < 0.5).astype(np.float64),
         "ordered": rng.integers(0, n_cut + 1, size=N).astype(np.float64)}[kind]
    return rows, samples, y, prec, cut


# S = 1: no fit (M = 0). 24, 25: M = 5, the shortest tail that is fitted. 33: M = 7, P = 64. 64: a power of two, 95 and 101 above one
# (P = 128). 1024: two rows per workgroup. 4096: one row per workgroup, 114 744 B of LDS, at r_eff = 0.05 the widest tail and grid
# (M = 820, m = 58).
@pytest.mark.parametrize("r_eff", [1.0, 0.05])
@pytest.mark.parametrize("S", [1, 24, 25, 33, 64, 95, 101, 1024, 4096])
def test_the_c_abi_on_synthetic_host_samples(S, r_eff):
    from myfm_amd import _capi

    N = 64
    for kind in ("regressor", "classifier", "ordered"):
        rows, samples, y, prec, cut = synthetic_call(kind, S, N, 100 * S + TASK[kind])
        d = _capi.Design(rows)
        kw = dict(precisions=prec, cutpoints=cut)
        density = d.log_density(samples, TASK[kind], y, pointwise=True, **kw)
        got = d.loo(samples, TASK[kind], y, log_weights=True, r_eff=r_eff, **kw)
        assert np.array_equal(got[2], density[0])
        pit_args = None
        if kind == "regressor" and S <= 101:
            pit_args = (np.stack([d.predict([s], 0) for s in samples]), y, prec)
        elif kind == "regressor":  # (the scores of that many samples, one call each, would take the test's time: the range only)
            assert got[3].shape == (N,) and np.all((got[3] > 0.0) & (got[3] < 1.0))
            got = got[:3] + (None,) + got[4:]
        fin = check_against_reference(got, density[4], r_eff, pit_args)
        assert fin.any() == (pr.tail_len(S, r_eff) >= 5)
        d.close()


def test_more_than_4096_samples_are_refused_by_the_library():
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call("classifier", 1, 5, 3)
    d = _capi.Design(rows)
    with pytest.raises(ValueError, match="at most 4096 samples, got 4097"):
        d.loo(samples * 4097, 1, y)
    K, S, w0s, ws, Vs = _capi._pack_samples(samples * 3)
    out = [np.empty(5) for _ in range(3)]
    p = _capi._p
    for tail_len in (-1, 3):
        rc = _capi.lib().mfm_design_loo(d.h, K, S, p(w0s), p(ws), p(Vs), 1, p(y), None, 0, None, 0, 0, tail_len, p(out[0]), p(out[1]), p(out[2]),
                                        None, None)
        assert rc == _capi.MFM_ERR_INVALID and b"tail_len" in _capi.lib().mfm_design_last_error(d.h)
    assert np.all(np.isfinite(d.loo(samples * 3, 1, y)[0]))  # ... and a valid call still runs on this design afterwards
    d.close()


def test_tilings_sources_and_ranges_do_not_change_a_bit(fitted):
    """N = 257 through _capi: tile_rows 64, 100 (last tiles of 1 and 57 rows), 257; chunk_samples 3 and 97; the host flavour and the
    store; a sub-range of the store; with and without the log weights"""
    from myfm_amd import _capi

    m = fitted
    task = TASK[m["kind"]]
    N = 257
    rows, y = m["X"][:N], m["y"][:N]
    blocks = [(mp[:N], B) for mp, B in capi_blocks(m["rels"])]
    samples = host_samples(m["est"])
    d = _capi.Design(rows, blocks)
    st = _capi.Store(d.D, RANK)
    for w0, w, V in samples:
        st.push(w0, w, V)
    kw = dict(precisions=m["prec"], cutpoints=m["cut"], log_weights=True)
    want = st.loo(d, task, y, **kw)
    assert want[4].shape == (N_KEPT, N) and (want[3] is None) == (task != 0)
    assert same(want, d.loo(samples, task, y, **kw))
    for tile_rows in (64, 100, N):
        for chunk_samples in (3, 97):
            assert same(want, st.loo(d, task, y, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (tile_rows, chunk_samples)
    assert same(want, d.loo(samples, task, y, tile_rows=64, chunk_samples=3, **kw))
    assert same(want[:4], st.loo(d, task, y, precisions=m["prec"], cutpoints=m["cut"], tile_rows=100)[:4])
    sub = dict(precisions=None if m["prec"] is None else m["prec"][3:30], cutpoints=None if m["cut"] is None else m["cut"][3:30], log_weights=True)
    part = st.loo(d, task, y, first=3, count=27, **sub)
    assert part[4].shape == (27, N) and same(part, d.loo(samples[3:30], task, y, **sub))
    other = st.loo(d, task, y, r_eff=0.5, **kw)  # M = 7 as well: min(6.4, 24)
    assert same(want, other)
    st.close()
    d.close()


def test_the_pickle_round_trip_gives_the_same_bits(fitted):
    m = fitted
    restored = pickle.loads(pickle.dumps(m["est"]))
    assert not restored.predictor_.resident
    rows, y = m["X"][:257], m["y"][:257]
    rels = [type(r)(np.asarray(r.original_to_block_array)[:257], r.data) for r in m["rels"]]
    assert same(m["est"].predict_loo(rows, y, rels, log_weights=True), restored.predict_loo(rows, y, rels, log_weights=True))


def test_a_folded_in_regressor_and_no_rows():
    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat, n_kept=N_KEPT, n_iter=40)
    rng = np.random.default_rng(9)
    items = rng.permutation(N_ITEMS)[:4]
    folded = est.fold_in(onehot(N_USERS + items), rng.normal(size=4), np.zeros(4, dtype=np.int64), 0)
    query = onehot(np.stack([np.full(3, D), N_USERS + rng.permutation(N_ITEMS)[:3]], axis=1), D + 1)  # the new user's column, an item
    y = rng.normal(size=3)
    got = folded.predict_loo(query, y, log_weights=True)
    density = folded.predict_log_density(query, y, pointwise=True)
    assert np.array_equal(got.lpd, density.lpd)
    prec, _ = constants("regressor", folded)
    check_against_reference(got, density.log_lik, 1.0, (device_scores(query, [], host_samples(folded)), y, prec))
    none = est.predict_loo(X[:0], lat[:0], log_weights=True)  # N = 0 through the estimator
    assert none.elpd_loo.shape == none.pareto_k.shape == none.lpd.shape == none.loo_pit.shape == (0,) and none.log_weights.shape == (N_KEPT, 0)


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_duplicated_samples_follow_the_tie_rule(kind):
    """every host sample passed twice, S = 2 x 21: every ratio has an equal partner 21 samples on. M = 9 and S - M = 33 is odd, so one
    pair lies across the cutoff (x_0 = 0) and four inside the tail, where the order decides which of the two gets which smoothed
    value"""
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call(kind, 21, 64, 77)
    d = _capi.Design(rows)
    kw = dict(precisions=None if prec is None else np.concatenate([prec, prec]))
    density = d.log_density(samples + samples, TASK[kind], y, pointwise=True, **kw)
    assert np.array_equal(density[4][:21], density[4][21:])
    got = d.loo(samples + samples, TASK[kind], y, log_weights=True, **kw)
    fin = check_against_reference(got[:3] + (None,) + got[4:], density[4])
    assert fin.all()
    lw = got[4]
    assert np.any(lw[:21] != lw[21:])  # equal ratios, different smoothed values: the order mattered
    d.close()
