"""NumPy / SciPy restatement of the ordered-probit summaries predict_proba_dist / predict_expected_dist, shared by
tests/test_predict_dist_oprobit_cpu.py and tests/test_gpu_predict_dist_oprobit.py: class probabilities as differences of
scipy.special.ndtr, the expected class index, and their summaries by np.mean / np.std / np.quantile. Scores and designs come
from tests/dist_ref.py."""
import numpy as np
from scipy.special import ndtr

from tests.dist_ref import expand, sample_scores  # noqa: F401  (re-exported for the tests)


def sample_cutpoints(rng, S, n_cut):
    """(S, n_cut) cutpoints, ascending and distinct within a sample, shifted from sample to sample (by less than one: no class
    probability comes near underflow however many samples there are)"""
    return np.stack([np.sort(rng.normal(size=n_cut)) * 1.5 + 0.05 * (s % 16) for s in range(S)])


def class_probs(scores, cuts):
    """(S, N, C) probabilities of the C = n_cut + 1 classes: p_c = Phi(cut_c - score) - Phi(cut_{c-1} - score) with
    Phi(cut_{-1} - .) = 0 and Phi(cut_{n_cut} - .) = 1; scores (S, N), cuts (S, n_cut)"""
    scores, cuts = np.asarray(scores, dtype=np.float64), np.asarray(cuts, dtype=np.float64)
    S, N = scores.shape
    cdf = ndtr(cuts[:, None, :] - scores[:, :, None])
    cdf = np.concatenate([np.zeros((S, N, 1)), cdf, np.ones((S, N, 1))], axis=2)
    return np.diff(cdf, axis=2)


def expected_index(probs):
    """(S, N) expected class index sum_c c p_c of (S, N, C) class probabilities"""
    return probs @ np.arange(probs.shape[2], dtype=np.float64)


def summary(vals, quantiles):
    """(mean, std, quantiles) over axis 0 of per-sample values (S, N) or (S, N, C): shapes vals.shape[1:] and (Q,) + vals.shape[1:]"""
    q = np.asarray(quantiles, dtype=np.float64)
    qs = np.quantile(vals, q, axis=0) if q.size else np.empty((0,) + vals.shape[1:])
    return vals.mean(axis=0), vals.std(axis=0), qs
