"""NumPy reference of the chain diagnostics of DESIGN 4.9.4 (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021), runnable in
float64 and in longdouble, vectorised over rows. Sums over samples are taken in sample order (cumsum) and sums over lags in lag
order, as the library takes them. The rank-normalised values come from a table the caller passes (the library's own: its last bits
are then no part of a comparison).

E(x) -> Sequence(ess, rhat, T, near): T is Geyer's truncation lag (-1 where there is no diagnosis), `near` is set where a decision of
Geyer's loops -- re + ro against 0, or the monotone comparison -- came within NEAR of equality: such a row may legitimately take
the other branch in another arithmetic, and is left out of comparisons (at most MAX_EXCLUDED_SHARE of a case's rows)."""
from collections import namedtuple

import numpy as np
from scipy.stats import rankdata

NEAR = 1e-9
MAX_EXCLUDED_SHARE = 0.01

# The largest float64 / longdouble deviation |a - b| / max(1, |b|) of this reference over the inputs of tests/test_ess_cpu.py and
# tests/test_gpu_ess.py, measured on the CPU (every comparison re-measures it on its own inputs and asserts it stays below), and the
# tolerances, 8 x these figures. Measured over cpu_cases(): ess 2.7e-14 (the AR(1) rows with phi = 0.98 at S = 4096, whose tau adds
# up a few hundred correlations; independent rows stay below 7e-15), rhat 1.6e-15. Over the inputs of tests/test_gpu_ess.py: ess
# 2.4e-13 (the regression likelihood of the AR(1) samples at S = 4096, whose prediction values reach 8.2e-14; everything up to
# S = 1024 stays below 3.3e-14), rhat 9.8e-16.
ESS_MEASURED_DEVIATION_ESS = 3e-13
ESS_MEASURED_DEVIATION_RHAT = 2e-15
ESS_RTOL_ESS = 8 * ESS_MEASURED_DEVIATION_ESS
ESS_RTOL_RHAT = 8 * ESS_MEASURED_DEVIATION_RHAT
# E on the raw Phi-saturated rows of cpu_cases() (not on their ranks): the values lie within 1e-6 and less of one another and many
# are equal, so what float64 has rounded away of the input is a large share of its spread. The deviation is the input's condition,
# largest at the smallest S, where a half holds four values. Measured: ess 1.2e-12, rhat 9.0e-9.
ESS_MEASURED_DEVIATION_ESS_SATURATED = 2e-12
ESS_MEASURED_DEVIATION_RHAT_SATURATED = 1e-8
ESS_RTOL_ESS_SATURATED = 8 * ESS_MEASURED_DEVIATION_ESS_SATURATED
ESS_RTOL_RHAT_SATURATED = 8 * ESS_MEASURED_DEVIATION_RHAT_SATURATED

Sequence = namedtuple("Sequence", ["ess", "rhat", "T", "near"])
ValueDiagnostics = namedtuple("ValueDiagnostics", ["rhat", "ess_bulk", "ess_mean", "mcse_mean", "T", "near"])
LikelihoodDiagnostics = namedtuple("LikelihoodDiagnostics", ["r_eff", "rhat", "ess_bulk", "mcse_lpd", "T", "near"])


def deviation(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return np.asarray(np.abs(a - b) / np.maximum(1.0, np.abs(b)), dtype=np.float64)


def _sum(m):
    """the sum along axis 1 in index order"""
    return np.cumsum(m, axis=1)[:, -1] if m.shape[1] else np.zeros(m.shape[0], dtype=m.dtype)


def E(x, dtype=np.float64):
    """(ess, rhat, T, near) per row of x (rows, S)"""
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    rows, S = x.shape
    n = S // 2
    nan = np.full(rows, np.nan, dtype=dtype)
    if n < 4:
        return Sequence(nan, nan.copy(), np.full(rows, -1), np.zeros(rows, dtype=bool))
    nn = dtype(n)
    a, b = x[:, :n], x[:, S - n:]
    with np.errstate(all="ignore"):
        # the halves about their first draws (a half of equal values is 0 exactly): d = (x - x_0) - m, mu = x_0 + m
        sa, sb = a - a[:, :1], b - b[:, :1]
        m_a, m_b = _sum(sa) / nn, _sum(sb) / nn
        da, db = sa - m_a[:, None], sb - m_b[:, None]
        mu_a, mu_b = a[:, 0] + m_a, b[:, 0] + m_b

        def A(t, sel):
            return (_sum(da[sel, :n - t] * da[sel, t:]) / nn + _sum(db[sel, :n - t] * db[sel, t:]) / nn) / dtype(2)

        everyone = np.ones(rows, dtype=bool)
        A0 = A(0, everyone)
        W = A0 * nn / dtype(n - 1)
        g = (mu_a + mu_b) / dtype(2)
        V = A0 + ((mu_a - g) ** 2 + (mu_b - g) ** 2)
        ok = (W > 0) & np.isfinite(W)
        rhat = np.where(ok, np.sqrt(V / W), nan)

        def rho_of(At, sel):
            return dtype(1) - (W[sel] - At) / V[sel]

        rho = np.zeros((rows, n + 2), dtype=dtype)
        re, ro = np.ones(rows, dtype=dtype), rho_of(A(1, everyone), everyone)
        rho[:, 0], rho[:, 1] = re, ro
        T = np.zeros(rows, dtype=np.int64)
        near = np.zeros(rows, dtype=bool)
        active = ok.copy()
        t = 0
        while t < n - 5:
            s = re + ro
            near |= active & (np.abs(s) < NEAR)
            active &= s > 0
            if not active.any():
                break
            t += 2
            re[active], ro[active] = rho_of(A(t, active), active), rho_of(A(t + 1, active), active)
            T[active] = t
            s = re + ro
            near |= active & (np.abs(s) < NEAR)
            keep = active & (s >= 0)
            rho[keep, t], rho[keep, t + 1] = re[keep], ro[keep]
        r = np.arange(rows)
        pos = ok & (re > 0)
        rho[r[pos], T[pos]] = re[pos]
        for t in range(2, int(T.max()) - 1, 2):  # t <= T - 2
            sel = ok & (t <= T - 2)
            prev, cur = rho[:, t - 2] + rho[:, t - 1], rho[:, t] + rho[:, t + 1]
            near |= sel & (np.abs(cur - prev) < NEAR)
            fix = sel & (cur > prev)
            rho[fix, t] = rho[fix, t + 1] = prev[fix] / dtype(2)
        below = np.arange(n + 2)[None, :] < T[:, None]
        tau = dtype(-1) + dtype(2) * _sum(np.where(below, rho, dtype(0))) + rho[r, T]
        tau = np.maximum(tau, dtype(1) / np.log10(dtype(2 * n)))
        ess = np.where(ok, dtype(2 * n) / tau, nan)
    return Sequence(ess, rhat, np.where(ok, T, -1), near & ok)


def rank_z(x, table):
    """the rank-normalised values of the rows of x (float64): ties share the average rank r, z = table[2r - 2]"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    x = np.where(np.all(np.isfinite(x), axis=1)[:, None], x, 0.0)  # (a row with a non-finite value has no ranks: its outputs are NaN)
    r = rankdata(x, method="average", axis=1)
    return np.asarray(table)[np.rint(2 * r - 2).astype(np.int64)]


def median_linear(x):
    """np.quantile(x, 0.5, axis=1) under the "linear" rule, as its _lerp computes it"""
    x = np.sort(np.atleast_2d(np.asarray(x, dtype=np.float64)), axis=1)
    S = x.shape[1]
    x0, x1 = x[:, (S - 1) // 2], x[:, S // 2]
    return x0 if S % 2 else x1 - (x1 - x0) * 0.5


def folded(x):
    """|x - median_linear(x)| per row (float64), evaluated from the two middle order statistics lo <= med <= hi as the library
    evaluates it: a draw is <= lo or >= hi, and its distance to the median is its distance to that neighbour plus h = (hi - lo) / 2.
    For even S the two middle draws, equally far from the median, then get equal values in floating point too; the rounded
    |x - med| makes them a tie or not by the last bit of the draws, and Z a rank apart. Odd S: the plain difference."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    xs = np.sort(x, axis=1)
    S = x.shape[1]
    lo, hi = xs[:, (S - 1) // 2][:, None], xs[:, S // 2][:, None]
    h = (hi - lo) * 0.5
    with np.errstate(all="ignore"):
        return np.where(x >= hi, (x - hi) + h, (lo - x) + h)


def _bulk_and_rhat(v, table, dtype):
    table = np.asarray(table, dtype=dtype)
    bulk = E(rank_z(v, table), dtype)
    with np.errstate(all="ignore"):
        folded_z = E(rank_z(folded(v), table), dtype)
        rhat = np.where(np.isnan(bulk.rhat) | np.isnan(folded_z.rhat), np.nan, np.maximum(bulk.rhat, folded_z.rhat))
    return bulk, rhat


def _sd(v, dtype):
    v = np.asarray(v, dtype=dtype)
    S = v.shape[1]
    mean = _sum(v) / dtype(S)
    return mean, np.sqrt(_sum((v - mean[:, None]) ** 2) / dtype(S - 1))


def value_diagnostics(v, table, dtype=np.float64):
    """rows of per-sample values v (rows, S) -> (rhat, ess_bulk, ess_mean, mcse_mean, T of v, near of v or Z(v))"""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    S = v.shape[1]
    if S < 8:
        nan = np.full(v.shape[0], np.nan)
        return ValueDiagnostics(nan, nan, nan, nan, np.full(v.shape[0], -1), np.zeros(v.shape[0], dtype=bool))
    with np.errstate(all="ignore"):
        plain = E(v, dtype)
        bulk, rhat = _bulk_and_rhat(v, table, dtype)
        _, sd = _sd(v, dtype)
        mcse = sd / np.sqrt(plain.ess)
    bad = ~np.all(np.isfinite(v), axis=1)
    out = [np.where(bad, np.nan, o) for o in (rhat, bulk.ess, plain.ess, mcse)]
    return ValueDiagnostics(*out, plain.T, plain.near | bulk.near)


def likelihood_diagnostics(log_lik, table, dtype=np.float64):
    """log_lik (S, N) as predict_log_density(pointwise=True) returns it -> per row (r_eff, rhat, ess_bulk, mcse_lpd, T of u, near)"""
    ll = np.asarray(log_lik, dtype=np.float64).T
    S = ll.shape[1]
    if S < 8:
        nan = np.full(ll.shape[0], np.nan)
        return LikelihoodDiagnostics(nan, nan, nan, nan, np.full(ll.shape[0], -1), np.zeros(ll.shape[0], dtype=bool))
    with np.errstate(all="ignore"):
        u = np.exp(ll - ll.max(axis=1)[:, None])  # (float64: the values themselves are the device's)
        plain = E(u, dtype)
        bulk, rhat = _bulk_and_rhat(u, table, dtype)
        mean, sd = _sd(u, dtype)
        mcse = sd / (mean * np.sqrt(plain.ess))
    bad = ~np.all(np.isfinite(u), axis=1)
    out = [np.where(bad, np.nan, o) for o in (plain.ess / dtype(S), rhat, bulk.ess, mcse)]
    return LikelihoodDiagnostics(*out, plain.T, plain.near | bulk.near)


CPU_SIZES = (8, 9, 10, 11, 16, 17, 95, 101, 130, 1024, 4096)


def ar1(rng, phi, rows, S):
    """stationary AR(1) rows with unit innovations"""
    e = rng.normal(size=(rows, S))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, S):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


def cpu_cases():
    """[(name, S, rows (n, S))]: per S independent normal rows, AR(1) rows with phi = 0.98, Phi-saturated rows with ties
    (ndtr(6 + 3 normal): most values within 1e-9 of 1, many equal to it) and clipped rows with heavy ties (three values)"""
    from scipy.special import ndtr

    out = []
    for S in CPU_SIZES:
        rng = np.random.default_rng(1000 + S)
        n = 40 if S <= 130 else 12
        out.append(("normal", S, rng.normal(size=(n, S))))
        out.append(("ar1", S, ar1(rng, 0.98, n, S)))
        out.append(("saturated", S, ndtr(6.0 + 3.0 * rng.normal(size=(n, S)))))
        out.append(("clipped", S, np.clip(np.rint(rng.normal(size=(n, S))), -1.0, 1.0)))
    return out
