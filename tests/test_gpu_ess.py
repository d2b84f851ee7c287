"""predict_diagnostics / likelihood_diagnostics on the device against the NumPy reference of tests/ess_ref.py.

The reference is fed the device's own per-sample values, so the comparison isolates the new kernel: for the likelihood kind
predict_log_density(pointwise=True).log_lik, for the prediction kind every sample's value from a one-sample summary call (the mean
over one sample is that sample's value, through the stage 1 the diagnostics read). The rank-normalised values come from the
library's own table. Effective sample sizes and Monte Carlo errors are compared by deviation(a, b) = |a - b| / max(1, |b|) <=
ESS_RTOL_ESS, rhat by the same form <= ESS_RTOL_RHAT, NaN must be NaN on both sides. Each comparison also runs the reference in
longdouble on its own inputs and checks that its float64 / longdouble deviation stays within the recorded figures the tolerances
are 8 x of. A row the reference flags as near a Geyer decision is left out, at most 1 % of a case's rows; the count is printed."""
import pickle

import numpy as np
import pytest

from tests import ess_ref as er
from tests.test_gpu_log_density import (D, N_ROWS, RANK, TASK, capi_blocks, constants, fit, host_samples, make_data, same, targets)
from tests.test_gpu_loo import synthetic_call

pytestmark = pytest.mark.gpu

N_KEPT = 32
KINDS = ("regressor", "classifier", "ordered")


def per_sample_values(kind, design, samples, cut):
    """(N, S): the value of every row under every sample as the device computes it, one one-sample summary call per sample"""
    if kind == "ordered":
        cols = [design.summary_oprobit([s], cut[k:k + 1], expected=True, quantiles=())[0] for k, s in enumerate(samples)]
    else:
        cols = [design.summary([s], mode=TASK[kind], quantiles=())[0] for s in samples]
    return np.stack(cols, axis=1)


def compare(what, got, want, wantL):
    """the four outputs `got` against the reference's `want` (float64) and `wantL` (longdouble); returns the rows compared"""
    n = len(want.near)
    left_out = want.near | wantL.near
    print("%s: %d of %d rows left out as near a Geyer decision" % (what, int(left_out.sum()), n))
    assert left_out.sum() <= er.MAX_EXCLUDED_SHARE * n
    use = ~left_out
    worst = {"ess": 0.0, "rhat": 0.0}
    own = {"ess": 0.0, "rhat": 0.0}
    for name, g in zip(want._fields[:4], got):
        w, wL = getattr(want, name), np.asarray(getattr(wantL, name), dtype=np.float64)
        assert g.shape == w.shape == (n,)
        fin = ~np.isnan(w)
        assert np.array_equal(np.isnan(wL), ~fin) and np.array_equal(np.isnan(g[use]), ~fin[use]), name
        sel = use & fin
        if not sel.any():
            continue
        key = "rhat" if name == "rhat" else "ess"
        own[key] = max(own[key], er.deviation(w[sel], wL[sel]).max())
        worst[key] = max(worst[key], er.deviation(g[sel], w[sel]).max())
        assert np.all(er.deviation(g[sel], w[sel]) <= (er.ESS_RTOL_RHAT if key == "rhat" else er.ESS_RTOL_ESS)), name
    print("%s: float64 / longdouble deviation of the reference on these inputs: ess %.3g, rhat %.3g; device / reference: ess %.3g, rhat %.3g"
          % (what, own["ess"], own["rhat"], worst["ess"], worst["rhat"]))
    assert own["ess"] <= er.ESS_MEASURED_DEVIATION_ESS and own["rhat"] <= er.ESS_MEASURED_DEVIATION_RHAT
    return use


def check_values(what, got, values):
    from myfm_amd import _myfm

    table = _myfm.rank_z_table(values.shape[1])
    want = er.value_diagnostics(values, table)
    compare(what, got, want, er.value_diagnostics(values, table, np.longdouble))
    return want


def check_likelihood(what, got, log_lik):
    """got: (r_eff, rhat, ess_bulk, mcse_lpd), the order of LikelihoodDiagnostics"""
    from myfm_amd import _myfm

    table = _myfm.rank_z_table(log_lik.shape[0])
    want = er.likelihood_diagnostics(log_lik, table)
    compare(what, got, want, er.likelihood_diagnostics(log_lik, table, np.longdouble))
    return want


@pytest.fixture(scope="module", params=[(k, b) for b in (False, True) for k in KINDS], ids=lambda p: p[0] + ("-block" if p[1] else ""))
def fitted(request):
    """the tiny models of test_gpu_log_density.py (40 x 30 one-hot, 600 rows, rank 3) with 32 samples kept of 40 iterations; the
    device's own log likelihoods and per-sample values of the fit's rows, computed once"""
    from myfm_amd import _capi

    kind, block = request.param
    X, rels, lat = make_data(block)
    y = np.asarray(targets(kind, lat), dtype=np.float64)
    est = fit(kind, X, rels, y, n_kept=N_KEPT, n_iter=40)
    assert est.predictor_.resident and len(est.predictor_.samples) == N_KEPT
    prec, cut = constants(kind, est)
    density = est.predict_log_density(X, y, rels, pointwise=True)
    d = _capi.Design(X, capi_blocks(rels))
    values = per_sample_values(kind, d, host_samples(est), cut)
    d.close()
    return dict(kind=kind, block=block, est=est, X=X, rels=rels, y=y, prec=prec, cut=cut, density=density, values=values)


def test_both_methods_match_the_reference(fitted):
    from myfm_amd import ChainDiagnostics, LikelihoodDiagnostics
    from myfm_amd.utils import evaluation as ev

    m = fitted
    got = m["est"].predict_diagnostics(m["X"], m["rels"])
    assert isinstance(got, ChainDiagnostics) and all(o.shape == (N_ROWS,) for o in got)
    want = check_values("prediction", got, m["values"])
    assert np.isfinite(want.ess_mean).sum() > N_ROWS // 2
    lik = m["est"].likelihood_diagnostics(m["X"], m["y"], m["rels"])
    assert isinstance(lik, LikelihoodDiagnostics) and all(o.shape == (N_ROWS,) for o in lik)
    want = check_likelihood("likelihood", lik, m["density"].log_lik)
    assert np.isfinite(want.r_eff).sum() > N_ROWS // 2
    for res in (got, lik):
        out = ev.diagnostics_summary(res)
        assert out["n_nan"] == int(np.isnan(res.rhat).sum()) and out["rhat_max"] >= 1.0 - 1e-12 and out["ess_min"] > 1.0
        assert out["ess_median"] <= N_KEPT * np.log10(N_KEPT)
    assert np.all(lik.r_eff[np.isfinite(lik.r_eff)] <= np.log10(N_KEPT) * (1 + 1e-12))


def test_resident_restored_and_host_samples_give_the_same_bits(fitted):
    from myfm_amd import _capi

    m = fitted
    rows, y = m["X"][:257], m["y"][:257]
    rels = [type(r)(np.asarray(r.original_to_block_array)[:257], r.data) for r in m["rels"]]
    restored = pickle.loads(pickle.dumps(m["est"]))
    assert not restored.predictor_.resident
    kw = dict(cutpoint_index=0) if m["kind"] == "ordered" else {}
    want_v, want_l = m["est"].predict_diagnostics(rows, rels, **kw), m["est"].likelihood_diagnostics(rows, y, rels, **kw)
    assert same(want_v, restored.predict_diagnostics(rows, rels, **kw))
    assert same(want_l, restored.likelihood_diagnostics(rows, y, rels, **kw))
    d = _capi.Design(rows, [(mp[:257], B) for mp, B in capi_blocks(m["rels"])])
    samples = host_samples(m["est"])
    assert same(want_v, d.ess(samples, 0, TASK[m["kind"]], cutpoints=m["cut"]))
    rhat, bulk, r_eff, mcse = d.ess(samples, 1, TASK[m["kind"]], y, precisions=m["prec"], cutpoints=m["cut"])
    assert same(want_l, (r_eff, rhat, bulk, mcse))
    d.close()


def test_tilings_do_not_change_a_bit(fitted):
    """N = 257 through _capi: tile_rows 1, 7 (a last tile of 5 rows) and automatic; chunk_samples 1, 5 (ragged over the 32 samples)
    and automatic; the host flavour and the store; a sub-range of the store"""
    from myfm_amd import _capi

    m = fitted
    task = TASK[m["kind"]]
    N = 257
    rows, y = m["X"][:N], m["y"][:N]
    d = _capi.Design(rows, [(mp[:N], B) for mp, B in capi_blocks(m["rels"])])
    st = _capi.Store(d.D, RANK)
    samples = host_samples(m["est"])
    for w0, w, V in samples:
        st.push(w0, w, V)
    calls = {"prediction": dict(kind=0, mode_or_task=task, cutpoints=m["cut"]),
             "likelihood": dict(kind=1, mode_or_task=task, y=y, precisions=m["prec"], cutpoints=m["cut"])}
    for name, kw in calls.items():
        want = st.ess(d, **kw)
        assert all(o.shape == (N,) for o in want)
        assert same(want, d.ess(samples, **kw)), name
        for tile_rows in (1, 7, 0):
            for chunk_samples in (1, 5, 0):
                assert same(want, st.ess(d, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (name, tile_rows, chunk_samples)
        assert same(want, d.ess(samples, tile_rows=7, chunk_samples=5, **kw)), name
    sub = dict(kind=1, mode_or_task=task, y=y, precisions=None if m["prec"] is None else m["prec"][3:30],
               cutpoints=None if m["cut"] is None else m["cut"][3:30])
    assert same(st.ess(d, first=3, count=27, **sub), d.ess(samples[3:30], **sub))
    st.close()
    d.close()


def test_r_eff_auto_is_the_mean_of_the_rows_estimates(fitted):
    m = fitted
    kw = dict(cutpoint_index=0) if m["kind"] == "ordered" else {}
    lik = m["est"].likelihood_diagnostics(m["X"], m["y"], m["rels"], **kw)
    r_eff = float(np.nanmean(lik.r_eff))
    assert 0.0 < r_eff <= np.log10(N_KEPT)
    auto = m["est"].predict_loo(m["X"], m["y"], m["rels"], log_weights=True, r_eff="auto", **kw)
    assert same(auto, m["est"].predict_loo(m["X"], m["y"], m["rels"], log_weights=True, r_eff=r_eff, **kw))
    assert np.array_equal(auto.lpd, m["density"].lpd)


def ar1_samples(kind, S, N, seed, phi=0.98):
    """synthetic_call with the samples an AR(1) sequence in the sample index around one model, 0.15 wide; a sample's cutpoints move
    with it, by one AR(1) shift for all of them (synthetic_call's are independent from sample to sample)"""
    rows, samples, y, prec, cut = synthetic_call(kind, S, N, seed)
    rng = np.random.default_rng(seed + 1)
    n_par = 1 + D + 2 * D
    path = er.ar1(rng, phi, n_par + 1, S) * np.sqrt(1.0 - phi * phi)  # (unit variance)
    if cut is not None:
        cut = np.linspace(-1.5, 1.5, cut.shape[1])[None, :] + 0.15 * path[n_par][:, None]
    mean = np.concatenate([[0.1], rng.normal(size=D) * 0.5, rng.normal(size=2 * D) * 0.5])
    theta = mean[:, None] + 0.15 * path[:n_par]
    samples = [(theta[0, s], theta[1:1 + D, s].copy(), theta[1 + D:, s].reshape(D, 2).copy()) for s in range(S)]
    return rows, samples, y, prec, cut


# S = 1, 7: NaN. 8, 9: the shortest halves, even and odd. 16, 17, 32, 33: P a power of two and one above. 95: the flagship. 128, 129,
# 130: n = 64 (one lag batch) against n = 65 (a second one). 1024: two rows per workgroup. 4096: one row per workgroup, 114 784 B of
# LDS. The rows: 64 up to S = 130, 37 above (the per-sample values cost a call per sample).
SIZES = [1, 7, 8, 9, 16, 17, 32, 33, 95, 128, 129, 130, 1024, 4096]
CASES = [(S, False) for S in SIZES] + [(S, True) for S in (130, 1024, 4096)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,ar", CASES, ids=lambda v: ("ar1" if v else "iid") if isinstance(v, bool) else str(v))
def test_the_c_abi_on_synthetic_host_samples(S, ar, kind):
    from myfm_amd import _capi

    N = 64 if S <= 130 else 37
    seed = 100 * S + TASK[kind] + (7 if ar else 0)
    rows, samples, y, prec, cut = (ar1_samples if ar else synthetic_call)(kind, S, N, seed)
    d = _capi.Design(rows)
    task = TASK[kind]
    got_v = d.ess(samples, 0, task, cutpoints=cut)
    rhat, bulk, r_eff, mcse = d.ess(samples, 1, task, y, precisions=prec, cutpoints=cut)
    if S < 8:
        assert all(np.all(np.isnan(o)) and o.shape == (N,) for o in got_v + (rhat, bulk, r_eff, mcse))
        d.close()
        return
    want_v = check_values("prediction", got_v, per_sample_values(kind, d, samples, cut))
    log_lik = d.log_density(samples, task, y, precisions=prec, cutpoints=cut, pointwise=True)[4]
    want_l = check_likelihood("likelihood", (r_eff, rhat, bulk, mcse), log_lik)
    d.close()
    assert np.all(np.isfinite(want_v.ess_mean)) and np.all(np.isfinite(want_l.r_eff))
    if ar and S >= 1024:  # the multi-batch path really runs: Geyer's loop goes beyond the first 64 lags on at least half the rows
        print("truncation lags of the prediction value: median %d, of the likelihood: median %d" % (np.median(want_v.T), np.median(want_l.T)))
        assert (want_v.T >= 64).sum() >= N / 2
    if not ar:
        assert np.median(want_v.T) < 64


def test_more_than_4096_samples_and_bad_arguments_are_refused_by_the_library():
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call("classifier", 1, 5, 3)
    d = _capi.Design(rows)
    with pytest.raises(ValueError, match="at most 4096 samples, got 4097"):
        d.ess(samples * 4097, 0, 1)
    with pytest.raises(ValueError, match="at most 4096 samples, got 4097"):
        d.ess(samples * 4097, 1, 1, y)
    with pytest.raises(ValueError, match="bad kind"):
        d.ess(samples * 9, 2, 1, y)
    with pytest.raises(ValueError, match="bad mode"):
        d.ess(samples * 9, 0, 3)
    with pytest.raises(ValueError, match="do not apply to the prediction value"):
        d.ess(samples * 9, 0, 0, precisions=np.ones(9))
    with pytest.raises(ValueError, match="cutpoints apply to the expected class index"):
        d.ess(samples * 9, 0, 1, cutpoints=np.zeros((9, 2)))
    with pytest.raises(ValueError, match="at least one cutpoint per sample"):
        d.ess(samples * 9, 0, 2)
    with pytest.raises(ValueError, match="labels must be 0 or 1"):
        d.ess(samples * 9, 1, 1, y + 0.5)
    with pytest.raises(ValueError, match="negative tiling"):
        d.ess(samples * 9, 0, 1, tile_rows=-1)
    out = d.ess(samples * 9, 0, 1)  # equal samples: nothing varies, and a valid call still runs on this design afterwards
    assert all(np.all(np.isnan(o)) for o in out)
    d.close()


def test_a_folded_in_regressor_and_no_rows():
    from myfm_amd import _capi
    from tests.test_gpu_log_density import N_ITEMS, N_USERS, onehot

    X, rels, lat = make_data(False)
    est = fit("regressor", X, rels, lat, n_kept=N_KEPT, n_iter=40)
    rng = np.random.default_rng(9)
    items = rng.permutation(N_ITEMS)[:4]
    folded = est.fold_in(onehot(N_USERS + items), rng.normal(size=4), np.zeros(4, dtype=np.int64), 0)
    query = onehot(np.stack([np.full(3, D), N_USERS + rng.permutation(N_ITEMS)[:3]], axis=1), D + 1)  # the new user's column, an item
    y = rng.normal(size=3)
    d = _capi.Design(query)
    check_values("folded-in prediction", folded.predict_diagnostics(query), per_sample_values("regressor", d, host_samples(folded), None))
    d.close()
    check_likelihood("folded-in likelihood", folded.likelihood_diagnostics(query, y), folded.predict_log_density(query, y, pointwise=True).log_lik)
    none = est.predict_diagnostics(X[:0])  # N = 0 through the estimator
    assert all(o.shape == (0,) for o in none)
    assert all(o.shape == (0,) for o in est.likelihood_diagnostics(X[:0], lat[:0]))
