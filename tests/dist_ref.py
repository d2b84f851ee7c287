"""NumPy / SciPy restatement of predict_dist, shared by tests/test_predict_dist_cpu.py and
tests/test_gpu_predict_dist.py: per-sample scores by the closed form, the empirical summaries by np.mean / np.std / np.quantile,
the mixture CDF by scipy.special.ndtr and its quantile by scipy.optimize.brentq on the bracket of per-component quantiles."""
import numpy as np
import scipy.sparse as sps
from scipy.optimize import brentq
from scipy.special import ndtr, ndtri

from myfm_amd.utils.synthetic import fm_score


def expand(X, blocks):
    """the flat design [X | B_0[idx_0] | B_1[idx_1] ...] of a main matrix and (index, block) pairs"""
    return sps.hstack([sps.csr_matrix(X)] + [sps.csr_matrix(B)[np.asarray(idx)] for idx, B in blocks]).tocsr()


def sample_scores(samples, X_flat):
    """(S, N) scores of the samples (w0, w[D], V[D, K]) on a flat design"""
    X_flat = sps.csr_matrix(X_flat)
    return np.stack([np.asarray(fm_score(X_flat, w0, w, V), dtype=np.float64).reshape(-1) for w0, w, V in samples])


def values(scores, mode):
    """the per-sample quantity that is summarised: the score (mode 0) or Phi(score) (mode 1)"""
    return ndtr(scores) if mode else np.asarray(scores, dtype=np.float64)


def summary(vals, quantiles):
    """(mean[N], std[N], quantiles[Q, N]) of (S, N) per-sample values"""
    q = np.asarray(quantiles, dtype=np.float64)
    qs = np.quantile(vals, q, axis=0) if q.size else np.empty((0, vals.shape[1]))
    return vals.mean(axis=0), vals.std(axis=0), qs


def mixture_cdf(y, scores, alphas):
    """mean_s Phi((y - score_s) sqrt(alpha_s)); scores (S,) or (S, N), y scalar or (N,)"""
    sa = np.sqrt(np.asarray(alphas, dtype=np.float64))
    sa = sa.reshape((-1,) + (1,) * (np.ndim(scores) - 1))
    return ndtr((y - scores) * sa).mean(axis=0)


def bracket(scores, alphas, p):
    """[min_s y_s, max_s y_s] of the per-component quantiles y_s = score_s + Phi^-1(p) / sqrt(alpha_s): F(lo) <= p <= F(hi)"""
    ys = np.asarray(scores) + ndtri(p) / np.sqrt(np.asarray(alphas, dtype=np.float64))
    return float(ys.min()), float(ys.max())


def mixture_quantile(scores, alphas, p):
    """the p-quantile of the mixture of one row ((S,) scores)"""
    lo, hi = bracket(scores, alphas, p)
    f = lambda y: float(mixture_cdf(y, scores, alphas)) - p  # noqa: E731
    if not lo < hi or f(lo) >= 0.0:
        return lo
    if f(hi) <= 0.0:
        return hi
    return brentq(f, lo, hi, xtol=1e-13)


def noise_summary(scores, alphas, quantiles):
    """(mean[N], std[N], quantiles[Q, N]) of the mixture mean_s N(score_s, 1 / alpha_s), scores (S, N)"""
    alphas = np.asarray(alphas, dtype=np.float64)
    std = np.sqrt(scores.var(axis=0) + np.mean(1.0 / alphas))
    qs = np.array([[mixture_quantile(scores[:, t], alphas, p) for t in range(scores.shape[1])] for p in quantiles]).reshape(
        len(quantiles), scores.shape[1])
    return scores.mean(axis=0), std, qs
