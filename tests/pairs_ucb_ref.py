"""Reference of the moments form of the query x candidate scorer: the per-sample value of every pair from
pairs_ref's direct pair rows, mean and population standard deviation over the samples in np.longdouble, the float64 twin of the
recurrence the kernels run, and the tolerances the tests hold the device to."""
import numpy as np

from tests import pairs_ref as pr
from tests import score_ref as sr

LD = np.longdouble
EPS = 2.0 ** -53


def sample_values(samples, Xq, Xc, mode, cuts=None):
    """(S, U, I) longdouble: v_s of every pair. The score is pairs_ref's float64 pair-row formula; mode 1 is Phi(score), mode 2
    sum_j Phi(score - cuts[s][j]) with score_ref.phi (scipy's erf on the float64 argument, the rest in longdouble); mode 0
    values are the float64 scores themselves."""
    X, U, I = pr._pair_rows(Xq, Xc)
    out = np.empty((len(samples), U * I), dtype=LD)
    for s, (w0, w, V) in enumerate(samples):
        sc = pr._sample_scores(X, w0, w, V)
        if mode == 0:
            out[s] = sc
        elif mode == 1:
            out[s] = sr.phi(sc)
        else:
            acc = np.zeros(U * I, dtype=LD)
            for c in np.asarray(cuts[s], dtype=np.float64):
                acc = acc + sr.phi(sc - c)
            out[s] = acc
    return out.reshape(len(samples), U, I)


def moments_ld(vals):
    """(mean, std) over axis 0 in longdouble, ddof = 0, two passes"""
    vals = np.asarray(vals, dtype=LD)
    mean = vals.sum(axis=0) / LD(vals.shape[0])
    std = np.sqrt(((vals - mean) ** 2).sum(axis=0) / LD(vals.shape[0]))
    return mean, std


def welford_twin(vals):
    """float64 twin of the kernels' recurrence, operation for operation (the device build does not contract a * b + c):
    d = v - mean; mean += d * (1 / n); M2 += d * (v - mean); std = sqrt(M2 / S). Returns (mean, std) float64."""
    vals = np.asarray(vals, dtype=np.float64)
    mean = np.zeros(vals.shape[1:])
    m2 = np.zeros(vals.shape[1:])
    for s in range(vals.shape[0]):
        rn = np.float64(1.0) / np.float64(s + 1)
        d = vals[s] - mean
        mean = mean + d * rn
        m2 = m2 + d * (vals[s] - mean)
    return mean, np.sqrt(m2 / np.float64(vals.shape[0]))


def recurrence_term(vals):
    """4 S 2^-53 rms_s(v_s): the moment recurrence's own rounding in the std (each of the S steps rounds a few quantities of
    the values' size)"""
    v = np.asarray(vals, dtype=np.float64)
    return 4.0 * v.shape[0] * EPS * np.sqrt((v ** 2).mean(axis=0))


def bounds(samples, Xq, Xc, mode, n_cut, vals, score_bound):
    """(mean's bound, std's bound), each (U, I). score_bound(samples, Xq, Xc, mode) is test_gpu_pairs.mode_bound, b for all the
    samples and b_s for the single sample s (mode 2: n_cut values of Phi, each 0.4-Lipschitz in the score and rounded itself, as
    test_gpu_pairs_rel.mode2_bound). std is 1-Lipschitz in the sup norm of the values: max_s b_s, plus the recurrence's term."""
    def b_of(ss):
        return n_cut * (0.4 * score_bound(ss, Xq, Xc, 0) + 1e-14) if mode == 2 else score_bound(ss, Xq, Xc, mode)

    b_mean = b_of(samples)
    b_max = np.max([b_of([s]) for s in samples], axis=0)
    return b_mean, b_max + recurrence_term(vals) + 1e-300


def at(matrix, idx):
    """matrix[u, idx[u, j]] with NaN where idx is -1"""
    out = np.full(idx.shape, np.nan)
    ok = idx >= 0
    rows = np.broadcast_to(np.arange(idx.shape[0])[:, None], idx.shape)
    out[ok] = np.asarray(matrix, dtype=np.float64)[rows[ok], idx[ok]]
    return out
