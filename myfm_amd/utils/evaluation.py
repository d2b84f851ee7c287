"""Model evaluation from the pointwise log predictive density (predict_log_density) and from Pareto-smoothed
leave-one-out (predict_loo), a digest of the chain diagnostics and of the continuous ranked
probability score (predict_crps), and the residuals of the leave-one-out predictions (predict_loo_dist).
Pure NumPy."""
import numpy as np

WAIC_HIGH_VARIANCE = 0.4  # a row whose log-likelihood variance exceeds this makes WAIC unreliable (Vehtari, Gelman, Gabry 2017)


def waic(result):
    """The widely applicable information criterion of a PointwiseDensity `result` (or any tuple that starts with lpd,
    log_lik_mean, log_lik_var), after Vehtari, Gelman and Gabry (2017). Returns a dict:

        lppd             sum_t lpd_t, the log pointwise predictive density
        p_waic           sum_t log_lik_var_t, the effective number of parameters
        elpd_waic        lppd - p_waic
        waic             -2 elpd_waic
        se               sqrt(N var_t(lpd_t - log_lik_var_t)), the standard error of elpd_waic (population variance over the rows)
        n_high_variance  the number of rows with log_lik_var > 0.4, the usual warning threshold"""
    lpd = np.asarray(result[0], dtype=np.float64)
    var = np.asarray(result[2], dtype=np.float64)
    if lpd.ndim != 1 or lpd.shape != var.shape:
        raise ValueError("lpd and log_lik_var must be 1-D arrays of one length")
    lppd, p_waic = float(lpd.sum()), float(var.sum())
    elpd = lppd - p_waic
    n = lpd.shape[0]
    se = float(np.sqrt(n * np.var(lpd - var))) if n else float("nan")
    return {"lppd": lppd, "p_waic": p_waic, "elpd_waic": elpd, "waic": -2.0 * elpd, "se": se,
            "n_high_variance": int(np.count_nonzero(var > WAIC_HIGH_VARIANCE))}


def log_score(result):
    """The mean negative log predictive density, -mean_t lpd_t (lower is better)."""
    lpd = np.asarray(result[0], dtype=np.float64)
    return float(-lpd.mean())


def pit_histogram(result, bins=10):
    """Calibration of a regression model from the probability integral transform: (counts, chi2), the counts of pit in `bins`
    equal cells of [0, 1] and the chi-square statistic sum (count - N / bins)^2 / (N / bins) against the uniform distribution
    (bins - 1 degrees of freedom). `result`: a PointwiseDensity of a regressor, or the pit values themselves -- for the
    leave-one-out transform of predict_loo pass result.loo_pit."""
    pit = getattr(result, "pit", result)
    if pit is None:
        raise ValueError("the probability integral transform exists for regression only")
    pit = np.asarray(pit, dtype=np.float64).reshape(-1)
    if isinstance(bins, bool) or int(bins) != bins or bins < 1:
        raise ValueError("bins must be a positive integer")
    if pit.shape[0] == 0 or not np.all((pit >= 0.0) & (pit <= 1.0)):
        raise ValueError("pit must be a non-empty array of values in [0, 1]")
    counts, _ = np.histogram(pit, bins=int(bins), range=(0.0, 1.0))
    expected = pit.shape[0] / int(bins)
    return counts, float(((counts - expected) ** 2).sum() / expected)


def pareto_k_threshold(n_samples):
    """Above this k the PSIS estimate of a row is unreliable at S draws: min(1 - 1 / log10(S), 0.7) (Vehtari et al. 2024)"""
    return min(1.0 - 1.0 / np.log10(n_samples), 0.7)


def loo(result, n_samples):
    """Leave-one-out cross-validation from a LooDensity `result` of predict_loo (or any tuple that starts with elpd_loo, pareto_k,
    lpd) over `n_samples` kept samples, after Vehtari, Gelman and Gabry (2017). Returns a dict:

        elpd_loo            sum_t elpd_loo_t, the expected log pointwise predictive density
        p_loo               sum_t (lpd_t - elpd_loo_t), the effective number of parameters
        looic               -2 elpd_loo
        se                  sqrt(N var_t elpd_loo_t), the standard error of elpd_loo (population variance over the rows)
        pareto_k_threshold  min(1 - 1 / log10(S), 0.7)
        n_bad_k             the number of rows whose k exceeds the threshold (+inf, where no fit was made, counts)

    For a regressor, pit_histogram(result.loo_pit) gives the calibration of the leave-one-out predictive distributions."""
    elpd = np.asarray(result[0], dtype=np.float64)
    k = np.asarray(result[1], dtype=np.float64)
    lpd = np.asarray(result[2], dtype=np.float64)
    if elpd.ndim != 1 or elpd.shape != k.shape or elpd.shape != lpd.shape:
        raise ValueError("elpd_loo, pareto_k and lpd must be 1-D arrays of one length")
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or n_samples < 2:
        raise ValueError("n_samples must be an integer of at least 2")
    total = float(elpd.sum())
    n = elpd.shape[0]
    threshold = pareto_k_threshold(int(n_samples))
    return {"elpd_loo": total, "p_loo": float((lpd - elpd).sum()), "looic": -2.0 * total,
            "se": float(np.sqrt(n * np.var(elpd))) if n else float("nan"), "pareto_k_threshold": threshold,
            "n_bad_k": int(np.count_nonzero(k > threshold))}


def compare(a, b):
    """The difference of two models' expected log predictive densities over the same rows: `a` and `b` are LooDensity results (or
    the pointwise elpd arrays themselves). Returns a dict: elpd_diff = sum_t (a_t - b_t), positive where `a` predicts better, and
    se_diff = sqrt(N var_t(a_t - b_t)) (population variance over the rows)."""
    ea = np.asarray(getattr(a, "elpd_loo", a), dtype=np.float64)
    eb = np.asarray(getattr(b, "elpd_loo", b), dtype=np.float64)
    if ea.ndim != 1 or eb.ndim != 1 or ea.shape != eb.shape:
        raise ValueError("the two results must hold one value per row of the same rows")
    d = ea - eb
    n = d.shape[0]
    return {"elpd_diff": float(d.sum()), "se_diff": float(np.sqrt(n * np.var(d))) if n else float("nan")}


def diagnostics_summary(result, rhat_max=1.01, ess_min=100):
    """What a ChainDiagnostics or LikelihoodDiagnostics `result` (predict_diagnostics, likelihood_diagnostics) says
    about the rows as a whole, with the thresholds of Vehtari et al. (2021). Returns a dict:

        rhat_max      the largest rhat over the rows (NaN rows left out; NaN where there is no other)
        n_high_rhat   the number of rows with rhat > `rhat_max`
        ess_min       the smallest ess_bulk over the rows
        ess_median    the median ess_bulk over the rows
        n_low_ess     the number of rows with ess_bulk < `ess_min`
        n_nan         the number of rows without a diagnosis (fewer than 8 kept samples, a constant or non-finite value)

    A LikelihoodDiagnostics adds r_eff_min and r_eff_median, the smallest and the median relative efficiency."""
    rhat = np.asarray(result.rhat, dtype=np.float64)
    ess = np.asarray(result.ess_bulk, dtype=np.float64)
    if rhat.ndim != 1 or rhat.shape != ess.shape:
        raise ValueError("rhat and ess_bulk must be 1-D arrays of one length")
    nan = float("nan")
    missing = np.isnan(rhat) | np.isnan(ess)
    r, e = rhat[~missing], ess[~missing]
    out = {"rhat_max": float(r.max()) if r.size else nan, "n_high_rhat": int(np.count_nonzero(r > rhat_max)),
           "ess_min": float(e.min()) if e.size else nan, "ess_median": float(np.median(e)) if e.size else nan,
           "n_low_ess": int(np.count_nonzero(e < ess_min)), "n_nan": int(np.count_nonzero(missing))}
    if hasattr(result, "r_eff"):
        f = np.asarray(result.r_eff, dtype=np.float64)
        f = f[np.isfinite(f)]
        out["r_eff_min"] = float(f.min()) if f.size else nan
        out["r_eff_median"] = float(np.median(f)) if f.size else nan
    return out


def sequence_diagnostics(x, n_chains=1):
    """(rhat, ess_bulk, ess_mean) of one scalar trace x (S,), `n_chains` chains of equal length one after another, as
    predict_diagnostics computes them per row, on the host: the library's own sequence estimator and table of
    rank-normalised values, ties sharing the average rank. rhat is the larger of the split R-hat of the rank-normalised draws and of
    the rank-normalised |x - median x|, ess_bulk the effective sample size of the rank-normalised draws, ess_mean that of the draws
    themselves. NaN for chains of fewer than 8 draws and for a trace that does not vary or is not finite."""
    from scipy.stats import rankdata

    from .. import _myfm

    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 1 or x.shape[0] < 1:
        raise ValueError("x must be a non-empty 1-D array")
    S = x.shape[0]
    ess_mean, _ = _myfm.ess_row(x, n_chains=int(n_chains))  # (refuses a chain count that does not divide S)
    nan = float("nan")
    if not np.all(np.isfinite(x)):
        return nan, nan, nan
    table = np.asarray(_myfm.rank_z_table(S))

    def z(v):
        return np.ascontiguousarray(table[np.rint(2.0 * rankdata(v, method="average") - 2.0).astype(np.int64)])

    ess_bulk, r_bulk = _myfm.ess_row(z(x), n_chains=int(n_chains))
    xs = np.sort(x)
    lo, hi = xs[(S - 1) // 2], xs[S // 2]
    h = (hi - lo) * 0.5
    _, r_folded = _myfm.ess_row(z(np.where(x >= hi, (x - hi) + h, (lo - x) + h)), n_chains=int(n_chains))
    rhat = nan if np.isnan(r_bulk) or np.isnan(r_folded) else max(r_bulk, r_folded)
    return float(rhat), float(ess_bulk), float(ess_mean)


def hyper_diagnostics(est):
    """sequence_diagnostics of the hyper-parameter trace of a fitted Gibbs estimator over its kept samples (the last S entries of
    history_.hypers; for a model of combine_chains / fit_chains its n_chains_ chains): a dict from "alpha", "mu_w[g]" and
    "lambda_w[g]" (g in range(n_groups_)) to (rhat, ess_bulk, ess_mean). These are the identified hyper-parameters; mu_V and
    lambda_V belong to single factors, which are identified up to sign and order only, and are left out. A constant trace (the
    alpha of the probit models) gives NaN."""
    predictor, history = getattr(est, "predictor_", None), getattr(est, "history_", None)
    if predictor is None or history is None:
        raise RuntimeError("hyper_diagnostics needs a fitted Gibbs estimator")
    S = len(predictor.samples)
    hypers = history.hypers
    if S < 1 or len(hypers) < S:
        raise RuntimeError("hyper_diagnostics needs history_ with the hyper-parameters of every kept sample")
    kept = hypers[len(hypers) - S:]
    n_chains = int(getattr(est, "n_chains_", 1))
    G = int(est.n_groups_ or 0)
    traces = {"alpha": [h.alpha for h in kept]}
    for g in range(G):
        traces["mu_w[%d]" % g] = [np.asarray(h.mu_w)[g] for h in kept]
    for g in range(G):
        traces["lambda_w[%d]" % g] = [np.asarray(h.lambda_w)[g] for h in kept]
    return {name: sequence_diagnostics(np.asarray(t, dtype=np.float64), n_chains) for name, t in traces.items()}


def crps_summary(result, reference=None):
    """What a CrpsScore `result` (predict_crps) says about the rows as a whole. Returns a dict:

        crps       the mean crps over the rows, in the units of y (smaller is better)
        se         its standard error sqrt(var_t(crps_t) / N) (population variance over the rows)
        accuracy   the mean of E|Y - y|
        spread     the mean of E|Y - Y'| / 2

    With `reference`, a CrpsScore of another model on the same rows (or the pointwise crps array itself), it adds skill =
    1 - crps / crps of the reference (positive where `result` predicts better), and se_diff, the paired standard error
    sqrt(var_t(crps_t - ref_t) / N) of the mean difference."""
    c = np.asarray(getattr(result, "crps", result), dtype=np.float64)
    if c.ndim != 1:
        raise ValueError("crps must hold one value per row")
    n = c.shape[0]
    nan = float("nan")

    def mean_of(name):
        v = getattr(result, name, None)
        return float(np.mean(np.asarray(v, dtype=np.float64))) if v is not None and n else nan

    out = {"crps": float(c.mean()) if n else nan, "se": float(np.sqrt(np.var(c) / n)) if n else nan,
           "accuracy": mean_of("accuracy"), "spread": mean_of("spread")}
    if reference is not None:
        r = np.asarray(getattr(reference, "crps", reference), dtype=np.float64)
        if r.ndim != 1 or r.shape != c.shape:
            raise ValueError("the two results must hold one value per row of the same rows")
        out["skill"] = 1.0 - float(c.mean()) / float(r.mean()) if n else nan
        out["se_diff"] = float(np.sqrt(np.var(c - r) / n)) if n else nan
    return out


def loo_residuals(result, y, interval=None):
    """What a LooPredictive `result` (predict_loo_dist) says about the targets y (N,) of the rows it was computed on,
    each predicted without itself. Returns a dict:

        residuals      y - mean (N,)
        rmse, mae      sqrt(mean_t residual_t^2), mean_t |residual_t|
        r2             1 - var_t(residual_t) / var_t(y_t), the leave-one-out R^2 (population variances over the rows)
        standardized   (y - mean) / std_y (N,), for a regressor (std_y is None otherwise: None)
        coverage       with interval = (lo_index, hi_index) into the quantile axis of `result`, the share of rows with
                       quantiles[lo_index] <= y <= quantiles[hi_index] (else None)

    Rows whose prediction is NaN (a target of density 0 under some sample) make the means NaN: drop them first."""
    y = np.asarray(y, dtype=np.float64)
    mean = np.asarray(result.mean, dtype=np.float64)
    if y.ndim != 1 or mean.ndim != 1 or y.shape != mean.shape:
        raise ValueError("y must hold one value per row of the result")
    res = y - mean
    n = y.shape[0]
    nan = float("nan")
    var_y = float(np.var(y)) if n else nan
    out = {"residuals": res, "rmse": float(np.sqrt(np.mean(res * res))) if n else nan, "mae": float(np.mean(np.abs(res))) if n else nan,
           "r2": 1.0 - float(np.var(res)) / var_y if n and var_y > 0.0 else nan,
           "standardized": None if result.std_y is None else res / np.asarray(result.std_y, dtype=np.float64), "coverage": None}
    if interval is not None:
        q = np.asarray(result.quantiles, dtype=np.float64)
        lo, hi = interval
        if isinstance(lo, bool) or isinstance(hi, bool) or not all(isinstance(i, (int, np.integer)) for i in (lo, hi)):
            raise ValueError("interval must be two indices into the quantile axis")
        if q.ndim != 2 or q.shape[1] != n or not (0 <= lo < q.shape[0] and 0 <= hi < q.shape[0]):
            raise ValueError("interval must be two indices into the quantile axis")
        out["coverage"] = float(np.mean((q[lo] <= y) & (y <= q[hi]))) if n else nan
    return out


def _contribution_arrays(result):
    lin, lin_std = np.asarray(result.linear, dtype=np.float64), np.asarray(result.linear_std, dtype=np.float64)
    inter, inter_std = np.asarray(result.interaction, dtype=np.float64), np.asarray(result.interaction_std, dtype=np.float64)
    F = lin.shape[0]
    if lin.ndim != 2 or inter.ndim != 2 or inter.shape != (F * (F + 1) // 2, lin.shape[1]) or lin_std.shape != lin.shape or inter_std.shape != inter.shape:
        raise ValueError("linear must be (F, N) and interaction (F (F + 1) / 2, N), each with a standard deviation of its shape")
    return F, lin, lin_std, inter, inter_std


def contribution_total(result):
    """bias + sum_g linear[g] + sum_p interaction[p] of a ScoreContributions `result` (predict_contributions), shape
    (N,): the posterior mean score of every row, the fields' terms added in their order."""
    _, lin, _, inter, _ = _contribution_arrays(result)
    return float(result.bias) + lin.sum(axis=0) + inter.sum(axis=0)


def contribution_matrix(result, row):
    """(mean, std), each a symmetric (F, F) matrix, of the interactions of row `row` of a ScoreContributions `result`: entry
    (g, h) = (h, g) is the pair's interaction, the diagonal the interactions inside a field."""
    F, _, _, inter, inter_std = _contribution_arrays(result)
    mean, std = np.zeros((F, F)), np.zeros((F, F))
    for p, (g, h) in enumerate(np.asarray(result.pairs).reshape(-1, 2)):
        mean[g, h] = mean[h, g] = inter[p, row]
        std[g, h] = std[h, g] = inter_std[p, row]
    return mean, std


def contribution_summary(result):
    """What a ScoreContributions `result` says about the rows as a whole. Returns a dict of two dicts, "linear" and "interaction",
    each with one array entry per component (F and P long):

        magnitude     the mean over the rows of |mean contribution|
        share         magnitude / the sum of the magnitudes of ALL components, linear and interaction (0 where that sum is 0)
        significant   the share of rows whose |mean| exceeds 2 std over the kept samples

    and "pairs", the (P, 2) field pairs of the interaction entries."""
    _, lin, lin_std, inter, inter_std = _contribution_arrays(result)
    n = lin.shape[1]

    def part(m, s):
        if n == 0:
            return np.zeros(m.shape[0]), np.zeros(m.shape[0])
        return np.abs(m).mean(axis=1), (np.abs(m) > 2.0 * s).mean(axis=1)

    lm, ls = part(lin, lin_std)
    im, is_ = part(inter, inter_std)
    total = float(lm.sum() + im.sum())
    scale = 1.0 / total if total > 0.0 else 0.0
    return {"linear": {"magnitude": lm, "share": lm * scale, "significant": ls},
            "interaction": {"magnitude": im, "share": im * scale, "significant": is_},
            "pairs": np.asarray(result.pairs).reshape(-1, 2)}
