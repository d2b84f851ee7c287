"""NumPy / SciPy reference of the pointwise log predictive density (predict_log_density), from the per-sample scores
(S, N). Deliberately not the three-regime erfcx form of csrc/mfm_logdens.hpp: log Phi comes from scipy.special.log_ndtr, a two-sided
class from log_ndtr(hi) + log1p(-exp(log_ndtr(lo) - log_ndtr(hi))), mirrored to the other tail when lo > 0."""
import numpy as np
from scipy.special import erfcx, log_ndtr, logsumexp, ndtr

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# How two values of a log density are compared: |a - b| / max(1, |b|). A log density enters sums over rows (lppd) and exp(): an
# absolute error e in l is a relative error e in the density itself, so below |l| = 1 the deviation is absolute; above, relative.
#
# LOGDENS_RTOL bounds that deviation between the code under test and this reference. It is 8 x the largest deviation, on
# value_grid(), between this reference and a second independent float64 formulation (alt_interval_log_prob): the device and the
# host libm may each round exp / log / erf a few ulp differently. Measured: 1.75e-13 (at (lo, hi) = (-0.002, -0.001), the narrowest
# intervals of the grid, 1e-3 wide, where Phi(hi) - Phi(lo) cancels in either formulation; 2.4e-14 at width 1e-2, 6.7e-16 on the
# one-sided labels); tests/test_log_density_cpu.py measures it again and checks that it has not grown.
LOGDENS_MEASURED_DEVIATION = 1.75e-13
LOGDENS_RTOL = 8 * LOGDENS_MEASURED_DEVIATION


def deviation(a, b):
    """|a - b| / max(1, |b|), elementwise; 0 where both are the same infinity"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return np.where(a == b, 0.0, d)


def interval_log_prob(lo, hi):
    """log(Phi(hi) - Phi(lo)), lo < hi, lo = -inf and hi = +inf allowed"""
    lo, hi = np.broadcast_arrays(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    flip = lo > 0  # Phi(hi) - Phi(lo) = Phi(-lo) - Phi(-hi): both ends into the lower tail, where log_ndtr is relative
    a, b = np.where(flip, -hi, lo), np.where(flip, -lo, hi)
    la, lb = log_ndtr(a), log_ndtr(b)
    with np.errstate(divide="ignore"):
        return lb + np.log1p(-np.exp(la - lb))


def alt_interval_log_prob(lo, hi):
    """the same by a second formulation: log(ndtr(hi) - ndtr(lo)) where Phi(hi) > 0.1, else from scipy's erfcx,
    log(erfcx(-hi / sqrt 2) / 2 - exp((hi^2 - lo^2) / 2) erfcx(-lo / sqrt 2) / 2) - hi^2 / 2; mirrored as above"""
    lo, hi = np.broadcast_arrays(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    flip = lo > 0
    a, b = np.where(flip, -hi, lo), np.where(flip, -lo, hi)
    r2 = np.sqrt(2.0)
    with np.errstate(all="ignore"):
        body = np.log(ndtr(b) - ndtr(a))
        bt = np.minimum(b, 0.0)  # (the tail form is used for b < 0 only)
        at = np.minimum(a, bt)
        low = np.where(np.isinf(at), 0.0, np.exp((bt * bt - at * at) / 2) * erfcx(-at / r2) / 2)
        tail = np.log(erfcx(-bt / r2) / 2 - low) - bt * bt / 2
    return np.where(ndtr(b) > 0.1, body, tail)


def value_grid():
    """(lo, hi) pairs that cover every regime of the code under test: both one-sided labels at |x| up to 38; regime A (lo > 0) and
    B (hi < 0) out to 38; regime C (lo <= 0 <= hi) wide, and narrow on both sides of the 0.5 switch, an interval straddling 0
    among them. Widths from 1e-3 (the narrowest spacing at which the reference's two-term form keeps LOGDENS_RTOL) to 30."""
    xs = np.concatenate([-np.array([38.0, 37.5, 30.0, 20.0, 12.0, 8.0, 5.0, 3.0, 2.0, 1.0, 0.6, 0.5, 0.49, 0.3, 0.1, 1e-3]), [0.0],
                         np.array([1e-3, 0.1, 0.3, 0.49, 0.5, 0.6, 1.0, 2.0, 3.0, 5.0, 8.0, 12.0, 20.0, 30.0, 37.5, 38.0])])
    widths = np.array([1e-3, 1e-2, 0.1, 0.3, 0.45, 0.5, 0.55, 0.9, 1.0, 1.1, 2.0, 5.0, 30.0])
    lo, hi = [], []
    for x in xs:  # one-sided: (-inf, x) and (x, +inf)
        lo += [-np.inf, x]
        hi += [x, np.inf]
    for x in xs:
        for w in widths:
            for a in (x, x - w, x - w / 2):  # the interval starting at, ending at and centred on x
                if abs(a) <= 38.0 and abs(a + w) <= 38.0:
                    lo.append(a)
                    hi.append(a + w)
    return np.array(lo), np.array(hi)


def log_lik(scores, y, task, precisions=None, cutpoints=None):
    """l[s, t] = log p(y_t | sample s). scores (S, N); task 0: precisions (S,); 1: y in {0, 1}; 2: cutpoints (S, n_cut), y labels"""
    f = np.asarray(scores, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if task == 0:
        alpha = np.asarray(precisions, dtype=np.float64)[:, None]
        return 0.5 * np.log(alpha) - HALF_LOG_2PI - 0.5 * alpha * (y[None, :] - f) ** 2
    if task == 1:
        return log_ndtr(np.where(y[None, :] > 0.5, f, -f))
    cut = np.asarray(cutpoints, dtype=np.float64)
    S = cut.shape[0]
    ext = np.concatenate([np.full((S, 1), -np.inf), cut, np.full((S, 1), np.inf)], axis=1)
    label = y.astype(np.int64)
    return interval_log_prob(ext[:, label] - f, ext[:, label + 1] - f)


def summarise(ll, scores=None, y=None, precisions=None):
    """(lpd, log_lik_mean, log_lik_var, pit or None) of l (S, N); pit with scores, y and precisions (regression)"""
    S = ll.shape[0]
    lpd = logsumexp(ll, axis=0) - np.log(S)
    var = np.var(ll, axis=0, ddof=1) if S > 1 else np.zeros(ll.shape[1])
    pit = None
    if precisions is not None:
        sq = np.sqrt(np.asarray(precisions, dtype=np.float64))[:, None]
        pit = ndtr((np.asarray(y, dtype=np.float64)[None, :] - scores) * sq).mean(axis=0)
    return lpd, ll.mean(axis=0), var, pit
