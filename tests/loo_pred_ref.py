"""NumPy / SciPy reference of the leave-one-out predictions (predict_loo_dist, predict_loo_crps), from the per-sample
scores (S, N) and the normalised log weights (S, N) of predict_loo, and its higher-precision twin.

The float64 form is vectorised over the rows and adds in the orders the device defines (np.cumsum: sequential, not .sum()'s pairwise
order). With w = exp(lw) and v the per-sample value (the score; Phi(score); the expected class index under the sample's cutpoints):
  mean = sum_s w_s v_s, std = sqrt(sum_s w_s (v_s - mean)^2), std_y = sqrt(std^2 + sum_s w_s / alpha_s), ess = 1 / sum_s w_s^2
  quantile at p: the samples ordered by (v_s, s) (a stable argsort), c_i the running sum of the weights in that order; v_(0) if
      c_0 >= p, else for the first i with c_i >= p  v_(i-1) + (v_(i) - v_(i-1)) clip((p - c_(i-1)) / (c_i - c_(i-1)), 0, 1), else v_(S-1)
  regression CRPS: accuracy = sum_s w_s A(y - mu_s, v_s), p_s = sum_{u < s} w_u A(mu_s - mu_u, v_s + v_u) + w_s g(2 v_s) / 2,
      spread = sum_s w_s p_s, crps = accuracy - spread  (A, g of tests/crps_ref.py)
  classes: d_j = sum_s w_s Phi(+-(cut_sj - score_s)), accuracy = sum_j d_j, spread = sum_j d_j (1 - d_j), crps = sum_j d_j^2
A row whose log weights are NaN has NaN everywhere.

The twin (hp=True) keeps every sum, the ordering and the quantile walk in longdouble and takes erf / erfc / exp from mpmath at 40
digits (rounded to longdouble as a pair of doubles).

How two values are compared: deviation(a, b) = |a - b| / max(1, |b|). Each bound is 8 x the largest deviation of the float64
reference from its twin over tolerance_cases() -- rows drawn as the tests draw theirs: all three tasks, S = 1, 2, 3, 5, 21, 33, 95 and
200 (the summaries also 1025 and 4096), weights from tests/psis_ref.py on the rows' own log likelihoods, targets up to 6 sigma
away, equal samples. The 8 is the project's margin for a device erf / exp that rounds a few ulp differently from libm. Measured:
  mean, std, std_y, ess     %(moments)s up to S = 1025 (3.3e-15: the mean of a regression row at S = 1025; 9.6e-16 and less up to S = 200)
                            %(moments_large)s above (3.9e-14: ess of a regression row at S = 4096, a sequential sum of 4096 squares);
                            rtol_moments(S) gives the bound of a case
  quantiles                 %(quantiles)s  (9.5e-15: classification at S = 1025)
  crps, accuracy, spread    %(crps)s  (7.2e-16)
tests/test_loo_pred_cpu.py measures them again and checks that none has grown.

A quantile cell (p, row) is left out of a comparison when some running sum c_i lies within NEAR of p: which step the walk stops at
is then decided by the last bits of the sum. tolerance_cases() and the probabilities QUANTILES leave out no more than 1 %% of a case's
cells (asserted in the CPU test)."""
import numpy as np
from scipy.special import erf, erfc, log_ndtr, ndtr

from tests import crps_ref as cr
from tests import psis_ref as pr
from tests.crps_ref import deviation  # noqa: F401  (the one way two values are compared)

LOO_MEASURED_DEVIATION_MOMENTS = 3.4e-15        # S <= LOO_LARGE_S
LOO_MEASURED_DEVIATION_MOMENTS_LARGE = 4.0e-14  # S > LOO_LARGE_S
LOO_LARGE_S = 1025
LOO_MEASURED_DEVIATION_QUANTILES = 1.0e-14
LOO_MEASURED_DEVIATION_CRPS = 7.4e-16
__doc__ = __doc__ % dict(moments=LOO_MEASURED_DEVIATION_MOMENTS, moments_large=LOO_MEASURED_DEVIATION_MOMENTS_LARGE, quantiles=LOO_MEASURED_DEVIATION_QUANTILES, crps=LOO_MEASURED_DEVIATION_CRPS)
LOO_RTOL_MOMENTS = 8 * LOO_MEASURED_DEVIATION_MOMENTS
LOO_RTOL_MOMENTS_LARGE = 8 * LOO_MEASURED_DEVIATION_MOMENTS_LARGE
LOO_RTOL_QUANTILES = 8 * LOO_MEASURED_DEVIATION_QUANTILES
LOO_RTOL_CRPS = 8 * LOO_MEASURED_DEVIATION_CRPS



def rtol_moments(S):
    """the bound of mean, std, std_y and ess of a case over S samples: the sums are sequential, their error grows with S"""
    return LOO_RTOL_MOMENTS if S <= LOO_LARGE_S else LOO_RTOL_MOMENTS_LARGE


NEAR = 1e-9
MAX_LEFT_OUT = 0.01
QUANTILES = (0.5, 0.95, 0.05, 0.25)  # in no order: the results come back in the caller's (p = 0 lies on the sum before the first
# weight, within NEAR of a small one: the tests check it exactly instead)
INV_SQRT2 = 0.70710678118654752440
LD = np.longdouble


# ---- the elementary functions, float64 or the twin's -----------------------------------------------------------------------------
def _mp_map(name, x):
    """mpmath's `name` at 40 digits of every element of the longdouble array x, rounded to longdouble"""
    import mpmath as mp

    x = np.asarray(x, dtype=LD)
    out = np.empty(x.shape, dtype=LD)
    flat_in, flat_out = x.reshape(-1), out.reshape(-1)
    with mp.workdps(40):
        fn = getattr(mp, name)
        for i in range(flat_in.shape[0]):
            xi = flat_in[i]
            if np.isnan(xi):
                flat_out[i] = np.nan
                continue
            hi = float(xi)
            r = fn(mp.mpf(hi) + mp.mpf(float(xi - LD(hi))))
            rh = float(r)
            flat_out[i] = LD(rh) + LD(float(r - mp.mpf(rh)))
    return out


def _fn(name, hp):
    if hp:
        return lambda x: _mp_map(name, x)
    return {"erf": erf, "erfc": erfc, "exp": np.exp}[name]


def _as(x, hp):
    return None if x is None else np.asarray(x, dtype=np.float64).astype(LD if hp else np.float64)


def _last(a):
    """the sequential sum along axis 0"""
    return np.cumsum(a, axis=0)[-1]


# ---- the values and the log likelihoods ------------------------------------------------------------------------------------------
def values(task, scores, cutpoints=None, hp=False):
    """the per-sample value v (S, N) that the summaries are taken of"""
    f = _as(scores, hp)
    dt = f.dtype.type
    if task == 0:
        return f
    e = _fn("erf", hp)
    if task == 1:
        return (e(f * dt(INV_SQRT2)) + dt(1)) / dt(2)
    cut = _as(cutpoints, hp)
    n_cut = cut.shape[1]
    prev, out = np.zeros_like(f), np.zeros_like(f)
    for c in range(n_cut):
        cdf = (dt(1) + e((cut[:, c][:, None] - f) * dt(INV_SQRT2))) / dt(2)
        if c > 0:
            out = out + dt(c) * (cdf - prev)
        prev = cdf
    return out + dt(n_cut) * (dt(1) - prev)


def log_lik(task, scores, y, precisions=None, cutpoints=None):
    """l (S, N) = log p(y | sample s), float64: what the weights of a test are made from"""
    f = np.asarray(scores, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if task == 0:
        z = (y[None, :] - f) * np.sqrt(precisions)[:, None]
        return 0.5 * np.log(precisions)[:, None] - 0.91893853320467274178 - 0.5 * z * z
    if task == 1:
        return log_ndtr(np.where(y[None, :] > 0.5, f, -f))
    S, N = f.shape
    ext = np.concatenate([np.full((S, 1), -np.inf), cutpoints, np.full((S, 1), np.inf)], axis=1)
    lab = y.astype(np.int64)
    return np.log(ndtr(ext[:, lab + 1] - f) - ndtr(ext[:, lab] - f))


# ---- the summary -------------------------------------------------------------------------------------------------------------------
def summary(v, lw, quantiles=(), inv_alpha=None, hp=False):
    """(mean (N,), std (N,), quantiles (Q, N), std_y (N,) or None, ess (N,), near (Q, N)) of the values v (S, N) under the log
    weights lw (S, N); near: the cells whose probability lies within NEAR of a running sum"""
    v, lw = _as(v, hp), _as(lw, hp)
    dt = v.dtype.type
    S, N = v.shape
    w = _fn("exp", hp)(lw)
    bad = np.isnan(w[0]) if N else np.zeros(0, dtype=bool)
    mean = _last(w * v)
    e = v - mean[None, :]
    m2 = _last(w * (e * e))
    ess = dt(1) / _last(w * w)
    std_y = None
    if inv_alpha is not None:
        std_y = np.sqrt(m2 + _last(w * _as(inv_alpha, hp)[:, None]))
    probs = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    q = np.empty((probs.shape[0], N), dtype=v.dtype)
    near = np.zeros((probs.shape[0], N), dtype=bool)
    if probs.shape[0] and N:
        order = np.argsort(v, axis=0, kind="stable")
        vs, ws = np.take_along_axis(v, order, axis=0), np.take_along_axis(w, order, axis=0)
        c = np.cumsum(ws, axis=0)
        cols = np.arange(N)
        for k, p in enumerate(probs):
            p = dt(p)
            ge = c >= p
            has, i = ge.any(axis=0), ge.argmax(axis=0)
            i1 = np.maximum(i, 1)
            v_prev, v_i, c_prev, c_i = vs[i1 - 1, cols], vs[i, cols], c[i1 - 1, cols], c[i, cols]
            with np.errstate(divide="ignore", invalid="ignore"):
                f = np.clip((p - c_prev) / (c_i - c_prev), dt(0), dt(1))
            x = np.where(i == 0, vs[0], v_prev + (v_i - v_prev) * f)
            q[k] = np.where(bad, np.nan, np.where(has, x, vs[-1]))
            near[k] = (np.abs(c - p) < NEAR).any(axis=0)
    return mean, np.sqrt(m2), q, std_y, ess, near


# ---- the CRPS ----------------------------------------------------------------------------------------------------------------------
def crps(task, scores, lw, y, precisions=None, cutpoints=None, hp=False):
    """(crps, accuracy, spread), (N,) each, of y under the predictive distribution of the samples reweighted by exp(lw)"""
    f, lw, y = _as(scores, hp), _as(lw, hp), _as(y, hp)
    dt = f.dtype.type
    S, N = f.shape
    ex, er = _fn("exp", hp), _fn("erf", hp)
    w = ex(lw)
    if task == 0:
        # (h, g) as the device's table holds them: float64 (crps_table_fill), whatever the sums are kept in
        v64 = 1.0 / np.asarray(precisions, dtype=np.float64)

        def A(m, h, g):
            z = m * h
            return m * er(z) + g * ex(-(z * z))

        h, g = (_as(a, hp) for a in cr.constants(v64))
        acc, total = np.zeros(N, dtype=f.dtype), np.zeros(N, dtype=f.dtype)
        for s in range(S):
            acc = acc + w[s] * A(y - f[s], h[s], g[s])
            p = np.zeros(N, dtype=f.dtype)
            if s > 0:
                hp_, gp_ = (_as(a, hp) for a in cr.constants(v64[s] + v64[:s]))
                p = p + _last(w[:s] * A(f[s][None, :] - f[:s], hp_[:, None], gp_[:, None]))
            p = p + w[s] * (dt(0.5) * dt(cr.constants(v64[s] + v64[s])[1]))
            total = total + w[s] * p
        return acc - total, acc, total
    ec = _fn("erfc", hp)
    cut = np.zeros((S, 1), dtype=f.dtype) if task == 1 else _as(cutpoints, hp)
    accuracy, spread, out = (np.zeros(N, dtype=f.dtype) for _ in range(3))
    for j in range(cut.shape[1]):
        t = cut[:, j][:, None] - f
        d = _last(w * (dt(0.5) * ec(np.where((y > j)[None, :], -t, t) * dt(INV_SQRT2))))
        accuracy = accuracy + d
        spread = spread + d * (dt(1) - d)
        out = out + d * d
    return out, accuracy, spread


# ---- the inputs of the tests -------------------------------------------------------------------------------------------------------
def random_case(task, S, N, seed, far=0.0, equal=False, n_cut=4, r_eff=1.0):
    """dict(task, f (S, N), y, prec, cut, lw (S, N), r_eff): random rows as tests/crps_ref.random_rows draws them and the Pareto-smoothed
    log weights of their own log likelihoods (tests/psis_ref.py)"""
    f, y, prec, cut = cr.random_rows(task, S, N, seed, far=far, equal=equal, n_cut=n_cut)
    lw = pr.psis(log_lik(task, f, y, prec, cut), r_eff)[2]
    return dict(task=task, f=f, y=y, prec=prec, cut=cut, lw=lw, r_eff=r_eff)


def tolerance_cases():
    """the inputs the constants are measured on (with summary_only_cases())"""
    cases = []
    for task in (0, 1, 2):
        for S, N in ((1, 6), (2, 6), (3, 6), (5, 6), (21, 8), (33, 8), (95, 6), (200, 2 if task == 0 else 4)):
            cases.append(random_case(task, S, N, 1000 * task + S))
        cases.append(random_case(task, 33, 6, 1000 * task + 51, far=6.0))
        cases.append(random_case(task, 9, 6, 1000 * task + 52, equal=True))
    return cases


def summary_only_cases():
    """further inputs of the summaries alone (a regression CRPS at these S would take the twin minutes)"""
    return [random_case(task, S, 3, 1000 * task + S) for task in (0, 1, 2) for S in (1025, 4096)]


def inv_alpha_of(case):
    return None if case["prec"] is None else 1.0 / case["prec"]


def measured_deviation():
    """(moments up to LOO_LARGE_S samples, moments above, quantiles, crps, share of quantile cells left out at most): the largest
    deviations of the float64 reference from its twin over tolerance_cases() and summary_only_cases()"""
    worst = [0.0, 0.0, 0.0]
    large = 0.0
    left_out = 0.0
    both = [(c, True) for c in tolerance_cases()] + [(c, False) for c in summary_only_cases()]
    for c, with_crps in both:
        out = []
        for hp in (False, True):
            v = values(c["task"], c["f"], c["cut"], hp)
            out.append(summary(v, c["lw"], QUANTILES, inv_alpha_of(c), hp))
        a, b = out
        for i in (0, 1, 3, 4):
            if a[i] is not None:
                dev = float(deviation(a[i], np.asarray(b[i], dtype=np.float64)).max())
                if c["f"].shape[0] <= LOO_LARGE_S:
                    worst[0] = max(worst[0], dev)
                else:
                    large = max(large, dev)
        keep = ~(a[5] | b[5])
        left_out = max(left_out, 1.0 - keep.mean())
        worst[1] = max(worst[1], float(deviation(a[2], np.asarray(b[2], dtype=np.float64))[keep].max()))
        if with_crps:
            got = np.stack(crps(c["task"], c["f"], c["lw"], c["y"], c["prec"], c["cut"]))
            twin = np.stack(crps(c["task"], c["f"], c["lw"], c["y"], c["prec"], c["cut"], hp=True)).astype(np.float64)
            worst[2] = max(worst[2], float(deviation(got, twin).max()))
    return worst[0], large, worst[1], worst[2], left_out
