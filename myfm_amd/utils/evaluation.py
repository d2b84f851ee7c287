"""Model evaluation from the pointwise log predictive density (predict_log_density). Pure NumPy."""
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
    (bins - 1 degrees of freedom). `result`: a PointwiseDensity of a regressor, or the pit values themselves."""
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
