"""NumPy reference of Pareto-smoothed importance-sampling leave-one-out (predict_loo), from the per-sample log
likelihoods l (S, N): Vehtari, Gelman and Gabry (2017), with the generalized Pareto fit of Zhang and Stephens (2009) under the loo
package's priors (Vehtari et al. 2024). Vectorised over the rows, a stable argsort for the tie rule (equal values keep their sample
order); `dtype` float64 or longdouble.

Per row, with M = tail_len(S, r_eff):
  r_s = -l_s - max_s(-l_s); any l_s = -inf: elpd_loo = -inf, k = +inf, log weights NaN
  M < 5: no smoothing, k = +inf
  sorted by (r_s, s): cutoff c at position S - M - 1, the tail the last M, x_i = exp(r_(i)) - exp(c) ascending;
      x at index floor(M / 4 + 0.5) - 1 (x*) <= 0: no smoothing, k = +inf
  m = 30 + floor(sqrt M) grid points b_j = 1 / x_M + (1 - sqrt(m / (j - 0.5))) / (3 x*), k_j = mean_i log1p(-b_j x_i),
      L_j = M (log(-b_j / k_j) - k_j - 1), w_j = 1 / sum_i exp(L_i - L_j), b = sum_j b_j w_j, k = mean_i log1p(-b x_i), sigma = -k / b,
      k^ = (M k + 5) / (M + 10)
  tail element i <- min(0, log(exp(c) + sigma expm1(-k^ log1p(-p_i)) / k^)), p_i = (i + 0.5) / M (k^ = 0: -sigma log1p(-p_i))
  lw_s = r_s - logsumexp_s r_s; elpd_loo = logsumexp_s(lw_s + l_s); loo_pit = sum_s exp(lw_s) Phi(z_s)

Two values are compared as tests/logdens_ref.py compares log densities: deviation(a, b) = |a - b| / max(1, |b|), for elpd_loo, the
log weights and the finite k^; infinities must agree exactly.

PSIS_RTOL_ELPD and PSIS_RTOL_K bound that deviation between the code under test and this reference in float64. Each is 8 x the
largest deviation between the float64 and the longdouble run of this reference over the inputs the tests use: cpu_cases() below,
and in tests/test_gpu_loo.py the device's own log likelihoods of the six tiny models, of the folded-in model and of the synthetic
host samples. The 8 covers the device and the host libm each rounding exp / log / log1p / expm1 a few ulp differently. Measured:
  elpd_loo and the log weights   3.64e-13 on cpu_cases() (S = 4096, r_eff = 0.05, M = 820, in a log weight); on the device's inputs
                                 at most 2.61e-13 (the ordered-probit model), 1.05e-13 on the synthetic samples (S = 4096)
  the finite k                   4.55e-11 on the rows of the ordered-probit model of tests/test_gpu_loo.py (32 samples, M = 7); on
                                 every other input at most 2.08e-12 (cpu_cases(), S = 24, M = 5, the shortest tail that is fitted)
tests/test_loo_cpu.py and every comparison of tests/test_gpu_loo.py measure the deviation on their inputs again and check that it
has not grown past the constants below."""
import numpy as np

from tests.logdens_ref import deviation  # noqa: F401  (the one way two values are compared)

PSIS_MEASURED_DEVIATION_ELPD = 3.7e-13
PSIS_MEASURED_DEVIATION_K = 4.6e-11
PSIS_RTOL_ELPD = 8 * PSIS_MEASURED_DEVIATION_ELPD
PSIS_RTOL_K = 8 * PSIS_MEASURED_DEVIATION_K


def tail_len(S, r_eff=1.0):
    """M = ceil(min(0.2 S, 3 sqrt(S / r_eff)))"""
    return int(np.ceil(min(0.2 * S, 3.0 * np.sqrt(S / float(r_eff)))))


def _lse(a):
    mx = a.max(axis=0)
    return mx + np.log(np.exp(a - mx).sum(axis=0))


def gpd_fit(x):
    """x (M, n) ascending per column, x* > 0: (k^, sigma) per column"""
    dt = x.dtype.type
    M = x.shape[0]
    q = int(np.floor(M / 4 + 0.5)) - 1
    m = 30 + int(np.floor(np.sqrt(M)))
    j = np.arange(1, m + 1).astype(dt)
    b = dt(1) / x[-1][None, :] + (dt(1) - np.sqrt(dt(m) / (j - dt(0.5))))[:, None] / (dt(3) * x[q])[None, :]  # (m, n)
    kj = np.empty_like(b)
    for g in range(m):  # (a grid point at a time: (M, n) temporaries)
        kj[g] = np.log1p(-b[g][None, :] * x).sum(axis=0) / dt(M)
    L = dt(M) * (np.log(-b / kj) - kj - dt(1))
    with np.errstate(over="ignore"):  # (a grid point far below the best one: weight 1 / inf = 0)
        w = dt(1) / np.exp(L[:, None, :] - L[None, :, :]).sum(axis=0)
    bh = (b * w).sum(axis=0)
    k = np.log1p(-bh[None, :] * x).sum(axis=0) / dt(M)
    sigma = -k / bh
    return (dt(M) * k + dt(5)) / (dt(M) + dt(10)), sigma


def psis(ll, r_eff=1.0, dtype=np.float64):
    """(elpd_loo (N,), pareto_k (N,), log_weights (S, N)) of the log likelihoods ll (S, N)"""
    dt = np.dtype(dtype).type
    ll = np.asarray(ll, dtype=np.float64).astype(dtype)
    S, N = ll.shape
    M = tail_len(S, r_eff)
    bad = np.isneginf(ll).any(axis=0)
    lc = np.where(bad[None, :], dt(0), ll)
    r = -lc
    r = r - r.max(axis=0)
    khat = np.full(N, np.inf)
    if M >= 5 and N > 0:
        order = np.argsort(r, axis=0, kind="stable")
        rs = np.take_along_axis(r, order, axis=0)
        ce = np.exp(rs[S - M - 1])
        x = np.exp(rs[S - M:]) - ce[None, :]
        q = int(np.floor(M / 4 + 0.5)) - 1
        cols = np.nonzero((x[q] > 0) & ~bad)[0]
        if cols.size:
            xf = x[:, cols]
            kh, sigma = gpd_fit(xf)
            p = (np.arange(M).astype(dtype) + dt(0.5)) / dt(M)
            l1 = np.log1p(-p)[:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                qq = np.where(kh[None, :] == 0, -sigma[None, :] * l1, sigma[None, :] * np.expm1(-kh[None, :] * l1) / kh[None, :])
            new = np.minimum(dt(0), np.log(ce[cols][None, :] + qq))
            sub = r[:, cols]
            np.put_along_axis(sub, order[S - M:, cols], new, axis=0)
            r[:, cols] = sub
            khat[cols] = kh.astype(np.float64)
    lw = r - _lse(r)[None, :]
    elpd = _lse(lw + lc)
    lw[:, bad] = np.nan
    elpd[bad] = -np.inf
    return elpd, khat, lw


def loo_pit(lw, scores, y, precisions):
    """sum_s exp(lw_s) Phi((y - score_s) sqrt(alpha_s)), float64"""
    from scipy.special import ndtr

    z = (np.asarray(y, dtype=np.float64)[None, :] - scores) * np.sqrt(np.asarray(precisions, dtype=np.float64))[:, None]
    return (np.exp(np.asarray(lw, dtype=np.float64)) * ndtr(z)).sum(axis=0)


def gpd_sample(k, sigma, n, rng):
    """n draws of the generalized Pareto distribution (location 0) by inversion"""
    u = rng.random(n)
    return sigma * np.expm1(-k * np.log1p(-u)) / k if k != 0 else -sigma * np.log1p(-u)


def normal_tails(S, n_rows, spread, seed):
    """(S, n_rows) log likelihoods of a normal model at targets `spread` posterior standard deviations wide: the importance ratios
    exp(-l) have a light tail for a small spread and a heavy one for a large"""
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(S, n_rows)) * spread
    y = rng.normal(size=n_rows) * (1.0 + spread)
    return -0.5 * (y[None, :] - mu) ** 2 - 0.9189385332046727


def cpu_cases():
    """[(name, ll (S, n), r_eff)]: what tests/test_loo_cpu.py runs _myfm.psis_row on, and what the constants above are measured on"""
    out = []
    for S in (1, 5, 20, 21, 24, 25, 26, 95, 101, 1000, 4096):  # (20: the last S with M < 5, 21: the first fitted)
        for r_eff in (1.0, 0.05, 2.5):
            rows = [normal_tails(S, 2, spread, 7 * S + i) for i, spread in enumerate((0.05, 0.5, 2.0, 6.0))]
            out.append(("S%d_reff%g" % (S, r_eff), np.concatenate(rows, axis=1), r_eff))
    rng = np.random.default_rng(3)
    base = normal_tails(101, 1, 1.0, 11)[:, 0]
    tied = base.copy()
    tied[np.argsort(base)[:12]] = np.repeat(np.sort(base)[:12:2], 2)  # the largest ratios in equal pairs
    degenerate = base.copy()
    degenerate[np.argsort(base)[:30]] = base.min()  # the cutoff and all of the tail one value: x = 0
    half = base.copy()
    half[np.argsort(base)[10:30]] = np.sort(base)[10]  # the cutoff equals the tail's lower half (x* = 0), the top ten differ
    const = np.full(101, -1.25)
    hole = base.copy()
    hole[rng.integers(0, 101)] = -np.inf
    out.append(("edge_rows", np.stack([tied, degenerate, half, const, hole], axis=1), 1.0))
    return out
