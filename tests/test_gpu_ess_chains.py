"""Chain diagnostics of several chains on the device against the NumPy reference of tests/ess_chains_ref.py, and the
estimators that combine_chains / fit_chains make.

As in tests/test_gpu_ess.py the reference is fed the device's own per-sample values (one one-sample summary call per sample) and log
likelihoods (predict_log_density's pointwise matrix), and the library's own table of rank-normalised values: the comparison isolates
the kernel. Effective sample sizes and Monte Carlo errors are compared by deviation(a, b) = |a - b| / max(1, |b|) <= CHAINS_RTOL_ESS,
rhat by the same form <= CHAINS_RTOL_RHAT, NaN must be NaN on both sides. Each comparison also runs the reference in longdouble on its
own inputs and checks that its float64 / longdouble deviation stays within the recorded figures the tolerances are 8 x of. A row the
reference flags as near a Geyer decision is left out, at most 1 % of a case's rows; the count is printed."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.special import logsumexp

from tests import ess_chains_ref as cr
from tests.test_gpu_ess import ar1_samples, per_sample_values
from tests.test_gpu_log_density import (D, N_ITEMS, N_ROWS, N_USERS, RANK, TASK, constants, device_scores, fit, host_samples, make_data, onehot,
                                        same, targets)
from tests.test_gpu_loo import synthetic_call

pytestmark = pytest.mark.gpu

KINDS = ("regressor", "classifier", "ordered")


def compare(what, got, want, wantL):
    """the four outputs `got` against the reference's `want` (float64) and `wantL` (longdouble); returns the rows compared"""
    n = len(want.near)
    left_out = want.near | wantL.near
    print("%s: %d of %d rows left out as near a Geyer decision" % (what, int(left_out.sum()), n))
    assert left_out.sum() <= cr.MAX_EXCLUDED_SHARE * n
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
        own[key] = max(own[key], cr.deviation(w[sel], wL[sel]).max())
        worst[key] = max(worst[key], cr.deviation(g[sel], w[sel]).max())
        assert np.all(cr.deviation(g[sel], w[sel]) <= (cr.CHAINS_RTOL_RHAT if key == "rhat" else cr.CHAINS_RTOL_ESS)), name
    print("%s: float64 / longdouble deviation of the reference on these inputs: ess %.3g, rhat %.3g; device / reference: ess %.3g, rhat %.3g"
          % (what, own["ess"], own["rhat"], worst["ess"], worst["rhat"]))
    assert own["ess"] <= cr.CHAINS_MEASURED_DEVIATION_ESS and own["rhat"] <= cr.CHAINS_MEASURED_DEVIATION_RHAT
    return use


def check_values(what, got, values, M):
    from myfm_amd import _myfm

    table = _myfm.rank_z_table(values.shape[1])
    want = cr.value_diagnostics(values, table, M)
    compare(what, got, want, cr.value_diagnostics(values, table, M, np.longdouble))
    return want


def check_likelihood(what, got, log_lik, M):
    """got: (r_eff, rhat, ess_bulk, mcse_lpd), the order of LikelihoodDiagnostics"""
    from myfm_amd import _myfm

    table = _myfm.rank_z_table(log_lik.shape[0])
    want = cr.likelihood_diagnostics(log_lik, table, M)
    compare(what, got, want, cr.likelihood_diagnostics(log_lik, table, M, np.longdouble))
    return want


def design_of(rows, block):
    """the design of synthetic_call's rows (a user and an item one-hot); block: the items through a relation block instead"""
    from myfm_amd import _capi

    if not block:
        return _capi.Design(rows)
    rows = sps.csr_matrix(rows)
    rows.sort_indices()
    item = rows.indices[rows.indptr[:-1] + 1] - N_USERS
    return _capi.Design(sps.csr_matrix(rows[:, :N_USERS]), [(item.astype(np.int64), sps.identity(N_ITEMS, format="csr"))])


# ---- through the C ABI -----------------------------------------------------------------------------------------------------------
# (chains, draws per chain, AR(1)): the shortest chains, even and odd (the middle draw of a chain of 9 or 19 is in no sequence); five
# chains: C = 10 lanes add up means; 32 chains of 8: C = 64 fills the wavefront, S = 256; four chains of 1024 autocorrelated draws:
# several batches of lags, S = 4096, one row per workgroup and the opt-in LDS size; 32 chains of 128: C = 64 at S = 4096.
SHAPES = [(2, 8, False), (3, 9, False), (5, 19, False), (32, 8, False), (4, 1024, True), (32, 128, False)]


@pytest.mark.parametrize("block", [False, True], ids=["plain", "block"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,L,ar", SHAPES, ids=lambda v: ("ar1" if v else "iid") if isinstance(v, bool) else str(v))
def test_the_c_abi_on_synthetic_host_samples(M, L, ar, kind, block):
    S = M * L
    N = 64 if S <= 256 else 37
    seed = 1000 * M + 10 * L + TASK[kind] + (5 if block else 0)
    rows, samples, y, prec, cut = (ar1_samples if ar else synthetic_call)(kind, S, N, seed)
    d = design_of(rows, block)
    task = TASK[kind]
    got_v = d.ess(samples, 0, task, cutpoints=cut, n_chains=M)
    rhat, bulk, r_eff, mcse = d.ess(samples, 1, task, y, precisions=prec, cutpoints=cut, n_chains=M)
    want_v = check_values("prediction", got_v, per_sample_values(kind, d, samples, cut), M)
    log_lik = d.log_density(samples, task, y, precisions=prec, cutpoints=cut, pointwise=True)[4]
    want_l = check_likelihood("likelihood", (r_eff, rhat, bulk, mcse), log_lik, M)
    d.close()
    assert np.all(np.isfinite(want_v.ess_mean)) and np.all(np.isfinite(want_l.r_eff))
    if ar:  # the multi-batch path really runs: Geyer's loop goes beyond the first 64 lags on at least half the rows
        print("truncation lags of the prediction value: median %d, of the likelihood: median %d" % (np.median(want_v.T), np.median(want_l.T)))
        assert (want_v.T >= 64).sum() >= N / 2
    else:
        assert np.median(want_v.T) < 64


def test_chains_too_short_give_nan():
    rows, samples, y, prec, cut = synthetic_call("regressor", 14, 9, 2)
    d = design_of(rows, False)
    out = d.ess(samples, 0, 0, n_chains=2) + d.ess(samples, 1, 0, y, precisions=prec, n_chains=2)  # two chains of 7
    assert all(o.shape == (9,) and np.all(np.isnan(o)) for o in out)
    assert all(np.all(np.isfinite(o)) for o in d.ess(samples, 0, 0))  # one chain of 14
    d.close()


# ---- bits --------------------------------------------------------------------------------------------------------------------
def old_entry(d, src, kind, task, y=None, precisions=None, cutpoints=None):
    """mfm_design_ess / mfm_design_ess_store, the entries without a chain count, called as _capi.Design._ess calls the new ones"""
    from myfm_amd import _capi

    y_, prec, n_cut, cp = d._log_density_args(np.zeros(d.N) if kind == 0 else y, precisions, cutpoints)
    out = [np.empty(d.N) for _ in range(4)]
    d._ck(src.call("mfm_design_ess", d.h, kind, task, _capi._p(y_ if kind == 1 else None), _capi._p(prec), n_cut, _capi._p(cp), 0, 0,
                   *[_capi._p(o) for o in out]))
    return tuple(out)


@pytest.fixture(scope="module", params=KINDS)
def fitted(request):
    """the tiny models of tests/test_gpu_log_density.py (40 x 30 one-hot, 600 rows, rank 3) with 32 samples kept of 40 iterations"""
    kind = request.param
    X, rels, lat = make_data(False)
    y = np.asarray(targets(kind, lat), dtype=np.float64)
    est = fit(kind, X, rels, y, n_kept=32, n_iter=40)
    assert est.predictor_.resident and len(est.predictor_.samples) == 32
    prec, cut = constants(kind, est)
    return dict(kind=kind, est=est, X=X, y=y, prec=prec, cut=cut)


def test_one_chain_through_the_new_entries_gives_the_bits_of_the_old_ones(fitted):
    from myfm_amd import _capi

    m = fitted
    task = TASK[m["kind"]]
    rows, y = m["X"][:257], m["y"][:257]
    d = _capi.Design(rows)
    samples = host_samples(m["est"])
    st = _capi.Store(d.D, RANK)
    for w0, w, V in samples:
        st.push(w0, w, V)
    for kw in (dict(kind=0, task=task, cutpoints=m["cut"]), dict(kind=1, task=task, y=y, precisions=m["prec"], cutpoints=m["cut"])):
        new = dict(kw, mode_or_task=kw["task"], n_chains=1)
        del new["task"]
        old_host, old_store = old_entry(d, _capi._host(samples), **kw), old_entry(d, _capi._resident(st, 0, None), **kw)
        assert same(old_host, d.ess(samples, **new)) and same(old_store, st.ess(d, **new)) and same(old_host, old_store)
        # ... and two chains over the same 32 samples: the store's entry and the host's agree, and say something else
        two = dict(new, n_chains=2)
        assert same(st.ess(d, **two), d.ess(samples, **two)) and not same(st.ess(d, **two), old_store)
    st.close()
    d.close()


@pytest.mark.parametrize("kind", KINDS)
def test_tilings_do_not_change_a_bit_of_three_chains(kind):
    """N = 257, three chains of 9: tile_rows 1, 7 (a last tile of 5 rows) and automatic; chunk_samples 1, 5 (ragged over the 27
    samples) and automatic; the host flavour and the store"""
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call(kind, 27, 257, 77 + TASK[kind])
    d = _capi.Design(rows)
    st = _capi.Store(d.D, 2)
    for w0, w, V in samples:
        st.push(w0, w, V)
    task = TASK[kind]
    for name, kw in (("prediction", dict(kind=0, mode_or_task=task, cutpoints=cut, n_chains=3)),
                     ("likelihood", dict(kind=1, mode_or_task=task, y=y, precisions=prec, cutpoints=cut, n_chains=3))):
        want = st.ess(d, **kw)
        assert all(o.shape == (257,) and np.all(np.isfinite(o)) for o in want)
        assert same(want, d.ess(samples, **kw)), name
        for tile_rows in (1, 7, 0):
            for chunk_samples in (1, 5, 0):
                assert same(want, st.ess(d, tile_rows=tile_rows, chunk_samples=chunk_samples, **kw)), (name, tile_rows, chunk_samples)
        assert same(want, d.ess(samples, tile_rows=7, chunk_samples=5, **kw)), name
        assert not same(want, st.ess(d, **dict(kw, n_chains=1)))
    st.close()
    d.close()


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_chains_that_sit_apart_have_a_large_rhat(kind):
    """three chains of 16 draws around one model; shifted: chain m's intercept moved by 1.5 m, some five standard deviations of a row's
    score (0.15 wide in every parameter: about 0.3).
    Every row whose value varies has rhat > 1.1 then, and the same chains unshifted stay below that row's shifted figure."""
    M, L, N = 3, 16, 64
    rows, samples, y, prec, cut = synthetic_call(kind, M * L, N, 41 + TASK[kind])
    shifted = [(w0 + 1.5 * (s // L), w, V) for s, (w0, w, V) in enumerate(samples)]
    d = design_of(rows, False)
    task = TASK[kind]
    plain, apart = d.ess(samples, 0, task, n_chains=M), d.ess(shifted, 0, task, n_chains=M)
    values = per_sample_values(kind, d, shifted, None)
    d.close()
    check_values("shifted prediction", apart, values, M)
    varies = np.ptp(values, axis=1) > 0
    print("%d of %d rows vary; shifted rhat: min %.3f; unshifted rhat: max %.3f" % (varies.sum(), N, np.nanmin(apart[0]), np.nanmax(plain[0])))
    assert varies.sum() >= N // 2 and np.all(np.isfinite(plain[0]))
    assert np.all(apart[0][varies] > 1.1) and np.all(plain[0][varies] < apart[0][varies])
    assert np.all(np.isnan(apart[0][~varies]))


def test_bad_chain_counts_are_refused_before_any_launch():
    from myfm_amd import _capi

    rows, samples, y, prec, cut = synthetic_call("classifier", 1, 5, 3)
    d = _capi.Design(rows)
    st = _capi.Store(d.D, 2)
    for _ in range(18):
        st.push(*samples[0])
    for call in (lambda **kw: d.ess(samples * 18, 0, 1, **kw), lambda **kw: d.ess(samples * 18, 1, 1, y, **kw),
                 lambda **kw: st.ess(d, 0, 1, **kw), lambda **kw: st.ess(d, 1, 1, y, **kw)):
        with pytest.raises(ValueError, match="n_chains must be at least 1, got 0"):
            call(n_chains=0)
        with pytest.raises(ValueError, match="at most 32 chains, got 33"):
            call(n_chains=33)
        with pytest.raises(ValueError, match="18 samples are not a multiple of n_chains = 4"):
            call(n_chains=4)
    with pytest.raises(ValueError, match="at most 4096 samples, got 4128"):
        d.ess(samples * 4128, 0, 1, n_chains=32)
    out = d.ess(samples * 18, 0, 1, n_chains=2)  # equal samples: nothing varies, and a valid call still runs on this design afterwards
    assert all(np.all(np.isnan(o)) for o in out)
    st.close()
    d.close()


# ---- the estimators ----------------------------------------------------------------------------------------------------------
N_KEPT, N_ITER, SEED = 16, 20, 5
SHAPES_KW = dict(group_shapes=[N_USERS, N_ITEMS])


@pytest.fixture(scope="module", params=KINDS)
def chains(request):
    """fit_chains of three chains of the tiny model (16 kept of 20 iterations), the three single fits from the same seeds, and the
    per-sample scores of the pooled samples from the one-sample scorer"""
    import myfm_amd

    kind = request.param
    cls = {"regressor": myfm_amd.MyFMGibbsRegressor, "classifier": myfm_amd.MyFMGibbsClassifier, "ordered": myfm_amd.MyFMOrderedProbit}[kind]
    X, rels, lat = make_data(False)
    y = np.asarray(targets(kind, lat), dtype=np.float64)
    proto = cls(RANK, random_seed=SEED)
    both = myfm_amd.fit_chains(proto, X, y, n_chains=3, n_iter=N_ITER, n_kept_samples=N_KEPT, **SHAPES_KW)
    assert proto.predictor_ is None
    singles = [cls(RANK, random_seed=SEED + c).fit(X, y, n_iter=N_ITER, n_kept_samples=N_KEPT, **SHAPES_KW) for c in range(3)]
    return dict(kind=kind, both=both, singles=singles, X=X, y=y, f=device_scores(X, [], host_samples(both)))


def test_fit_chains_pools_the_fits_of_its_seeds(chains):
    import myfm_amd

    m = chains
    both, singles = m["both"], m["singles"]
    assert type(both) is type(singles[0]) and both.n_chains_ == 3 and len(both.predictor_.samples) == 48 and not both.predictor_.resident
    assert both.n_groups_ == 2 and len(both.history_.hypers) == 48
    plain = fit(m["kind"], m["X"], [], m["y"], n_kept=N_KEPT, n_iter=N_ITER)  # (seed 5: chain 0)
    for name in ("w0_samples", "w_samples", "V_samples"):
        assert np.array_equal(getattr(both, name)[:N_KEPT], getattr(plain, name)), name
        assert np.array_equal(getattr(both, name), np.concatenate([getattr(s, name) for s in singles])), name
    assert [h.alpha for h in both.history_.hypers] == [h.alpha for s in singles for h in s.history_.hypers[-N_KEPT:]]
    predict = (lambda e: e.predict_proba(m["X"])) if m["kind"] != "regressor" else (lambda e: e.predict(m["X"]))
    np.testing.assert_allclose(predict(both), np.mean([predict(s) for s in singles], axis=0), rtol=0, atol=1e-12)
    seeded = myfm_amd.fit_chains(singles[0], m["X"], m["y"], n_chains=2, seeds=[SEED + 2, SEED], n_iter=N_ITER, n_kept_samples=N_KEPT, **SHAPES_KW)
    assert np.array_equal(seeded.w_samples, np.concatenate([singles[2].w_samples, singles[0].w_samples]))
    assert same(tuple(myfm_amd.combine_chains(singles).predict_diagnostics(m["X"])), tuple(both.predict_diagnostics(m["X"])))


def test_the_predictors_work_on_the_pooled_samples(chains):
    m = chains
    both, kind, X, y, f = m["both"], m["kind"], m["X"], m["y"], m["f"]
    kw = dict(cutpoint_index=0) if kind == "ordered" else {}
    alpha = np.array([h.alpha for s in m["singles"] for h in s.history_.hypers[-N_KEPT:]])
    if kind == "regressor":
        dist = both.predict_dist(X, quantiles=(0.1, 0.9), noise=True)
        np.testing.assert_allclose(dist.mean, f.mean(axis=0), rtol=0, atol=1e-12)
        np.testing.assert_allclose(dist.std, np.sqrt(f.var(axis=0) + np.mean(1.0 / alpha)), rtol=1e-12)
        assert np.all(dist.quantiles[0] < dist.mean) and np.all(dist.mean < dist.quantiles[1])
        ll = 0.5 * np.log(alpha / (2 * np.pi))[:, None] - 0.5 * alpha[:, None] * (y[None, :] - f) ** 2
    elif kind == "classifier":
        dist = both.predict_dist(X, quantiles=())
        from scipy.special import log_ndtr, ndtr

        np.testing.assert_allclose(dist.mean, ndtr(f).mean(axis=0), rtol=0, atol=1e-12)
        np.testing.assert_allclose(dist.std, ndtr(f).std(axis=0), rtol=0, atol=1e-12)
        ll = log_ndtr((2 * y[None, :] - 1) * f)
    else:
        ll = None
    density = both.predict_log_density(X, y, pointwise=True, **kw)
    assert density.log_lik.shape == (48, N_ROWS) and np.all(np.isfinite(density.lpd))
    if ll is not None:
        np.testing.assert_allclose(density.lpd, logsumexp(ll, axis=0) - np.log(48), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(density.lpd, logsumexp(density.log_lik, axis=0) - np.log(48), rtol=1e-12, atol=1e-12)
    lik = both.likelihood_diagnostics(X, y, **kw)
    auto = both.predict_loo(X, y, r_eff="auto", **kw)
    assert same(auto, both.predict_loo(X, y, r_eff=float(np.nanmean(lik.r_eff)), **kw)) and np.array_equal(auto.lpd, density.lpd)
    crps = both.predict_crps(X, y, **kw)
    assert crps.crps.shape == (N_ROWS,) and np.all(crps.crps >= 0.0) and np.all(np.isfinite(crps.crps))
    Xq, Xc = onehot(np.arange(5)), onehot(N_USERS + np.arange(N_ITEMS))
    idx, score = both.predict_topk(Xq, Xc, 3)
    pairs = np.mean([s.predict_pairs(Xq, Xc) for s in m["singles"]], axis=0)
    np.testing.assert_allclose(score, -np.sort(-pairs, axis=1)[:, :3], rtol=0, atol=1e-12)
    assert idx.shape == (5, 3)
    restored = pickle.loads(pickle.dumps(both))
    assert restored.n_chains_ == 3 and len(restored.history_.hypers) == 48
    assert same(tuple(restored.predict_diagnostics(X, **kw)), tuple(both.predict_diagnostics(X, **kw)))
    assert same(tuple(restored.predict_log_density(X, y, **kw))[:3], tuple(density)[:3])


def test_the_diagnostics_of_a_combined_model_compare_its_chains(chains):
    from myfm_amd import ChainDiagnostics, LikelihoodDiagnostics, _capi

    m = chains
    both, kind, X, y = m["both"], m["kind"], m["X"], m["y"]
    kw = dict(cutpoint_index=0) if kind == "ordered" else {}
    prec, cut = constants(kind, both)
    d = _capi.Design(X)
    samples = host_samples(both)
    task = TASK[kind]
    got = both.predict_diagnostics(X, **kw)
    assert isinstance(got, ChainDiagnostics) and same(tuple(got), d.ess(samples, 0, task, cutpoints=cut, n_chains=3))
    assert not same(tuple(got), d.ess(samples, 0, task, cutpoints=cut, n_chains=1))
    lik = both.likelihood_diagnostics(X, y, **kw)
    rhat, bulk, r_eff, mcse = d.ess(samples, 1, task, y, precisions=prec, cutpoints=cut, n_chains=3)
    assert isinstance(lik, LikelihoodDiagnostics) and same(tuple(lik), (r_eff, rhat, bulk, mcse))
    assert not np.array_equal(lik.rhat, d.ess(samples, 1, task, y, precisions=prec, cutpoints=cut, n_chains=1)[0], equal_nan=True)
    check_values("combined prediction", got, per_sample_values(kind, d, samples, cut), 3)
    d.close()
    one = m["singles"][0]
    assert not hasattr(one, "n_chains_")
    d1 = _capi.Design(X)
    p1, c1 = constants(kind, one)
    assert same(tuple(one.predict_diagnostics(X, **kw)), d1.ess(host_samples(one), 0, task, cutpoints=c1, n_chains=1))  # a plain fit: one chain
    d1.close()


def test_folding_in_keeps_the_chains(chains):
    """fold_in of a regressor, fold_in_gibbs of a classifier and of an ordered probit"""
    m = chains
    both, kind = m["both"], m["kind"]
    rng = np.random.default_rng(9)
    items = rng.permutation(N_ITEMS)[:4]
    ctx, entity = onehot(N_USERS + items), np.zeros(4, dtype=np.int64)
    labels = {"regressor": rng.normal(size=4), "classifier": np.array([1, 0, 1, 1]), "ordered": np.array([1, 0, 2, 3])}[kind]

    def fold(est):
        if kind == "regressor":
            return est.fold_in(ctx, labels, entity, 0)
        return est.fold_in_gibbs(ctx, labels, entity, 0, n_burn=3, n_inner=5)

    folded = fold(both)
    assert folded.n_chains_ == 3 and len(folded.predictor_.samples) == 48 and folded.fold_in_columns_ == (D, D + 1)
    assert both.predictor_.feature_size == D and folded.predictor_.feature_size == D + 1
    query = onehot(np.stack([np.full(3, D), N_USERS + rng.permutation(N_ITEMS)[:3]], axis=1), D + 1)
    pred = folded.predict(query) if kind == "regressor" else folded.predict_proba(query)
    assert pred.shape[0] == 3 and np.all(np.isfinite(pred))
    out = folded.predict_diagnostics(query)
    assert all(o.shape == (3,) and np.all(np.isfinite(o)) for o in out)
    assert not hasattr(fold(m["singles"][0]), "n_chains_")
