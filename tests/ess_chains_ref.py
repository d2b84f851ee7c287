"""NumPy reference of the chain diagnostics of several chains (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021),
the generalisation of tests/ess_ref.py from the two halves of one chain to the 2M halves of M chains, runnable in float64 and in
longdouble, vectorised over rows. A row's S draws are M chains of L = S / M draws, chain after chain; n = L // 2; sequence 2m is
x[mL : mL + n], sequence 2m + 1 is x[mL + L - n : mL + L]. Sums over samples are taken in sample order (cumsum), sums over
sequences in sequence order and sums over lags in lag order, as the library takes them. The rank-normalised values come from a table
the caller passes (the library's own: its last bits are then no part of a comparison); ranks, the median, the mean and the standard
deviation are taken over all S draws.

E(x, n_chains) -> Sequence(ess, rhat, T, near) as ess_ref.E: `near` is set where a decision of Geyer's loops came within NEAR of
equality; such a row is left out of comparisons (at most MAX_EXCLUDED_SHARE of a case's rows). With n_chains = 1 every function here
returns the bits of its namesake in ess_ref.py."""
import numpy as np

from tests import ess_ref as er
from tests.ess_ref import (MAX_EXCLUDED_SHARE, NEAR, LikelihoodDiagnostics, Sequence, ValueDiagnostics, ar1, deviation,  # noqa: F401
                           folded, rank_z)

# The largest float64 / longdouble deviation |a - b| / max(1, |b|) of this reference over the inputs of tests/test_ess_chains_cpu.py
# and tests/test_gpu_ess_chains.py, measured on the CPU (every comparison re-measures it on its own inputs and asserts it stays
# below), and the tolerances, 8 x these figures. Measured over cpu_cases(): ess 1.53e-14 (the AR(1) rows of four chains of 1024),
# rhat 5.9e-16. Over the inputs of tests/test_gpu_ess_chains.py, with the per-sample values and log likelihoods that NumPy gives for
# its synthetic samples standing in for the device's (they differ in last bits): ess 3.2e-14 (the classifier's values of the four
# AR(1) chains of 1024; everything else stays below 3e-15), rhat 4.3e-16; re-measured by the device tests on the device's own
# values: ess 3.1e-14, rhat 4.3e-16. Recorded are the largest of these, rounded up in their last digit. Sums over a chain are a
# quarter as long as ess_ref.py's at S = 4096, and the figures are smaller than its 3e-13 and 2e-15 accordingly.
CHAINS_MEASURED_DEVIATION_ESS = 4e-14
CHAINS_MEASURED_DEVIATION_RHAT = 6e-16
CHAINS_RTOL_ESS = 8 * CHAINS_MEASURED_DEVIATION_ESS
CHAINS_RTOL_RHAT = 8 * CHAINS_MEASURED_DEVIATION_RHAT
# E on the raw Phi-saturated rows of cpu_cases() (not on their ranks), as in ess_ref.py: what float64 has rounded away of the input
# is a large share of its spread, largest where a half holds four values. Measured: ess 4.9e-15, rhat 2.2e-12 (pooling 2M halves
# averages the halves' condition: ess_ref.py's single pair of halves of four reaches 9.0e-9).
CHAINS_MEASURED_DEVIATION_ESS_SATURATED = 5e-15
CHAINS_MEASURED_DEVIATION_RHAT_SATURATED = 3e-12
CHAINS_RTOL_ESS_SATURATED = 8 * CHAINS_MEASURED_DEVIATION_ESS_SATURATED
CHAINS_RTOL_RHAT_SATURATED = 8 * CHAINS_MEASURED_DEVIATION_RHAT_SATURATED

_sum = er._sum


def sequences(x, n_chains):
    """the C = 2 n_chains half-chains of the rows of x (rows, S), each (rows, n), in sequence order"""
    S = x.shape[1]
    L = S // n_chains
    n = L // 2
    out = []
    for m in range(n_chains):
        out.append(x[:, m * L:m * L + n])
        out.append(x[:, m * L + L - n:m * L + L])
    return out


def E(x, n_chains=1, dtype=np.float64):
    """(ess, rhat, T, near) per row of x (rows, S), S a multiple of n_chains"""
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    rows, S = x.shape
    assert n_chains >= 1 and S % n_chains == 0
    C = 2 * n_chains
    n = (S // n_chains) // 2
    nan = np.full(rows, np.nan, dtype=dtype)
    if n < 4:
        return Sequence(nan, nan.copy(), np.full(rows, -1), np.zeros(rows, dtype=bool))
    nn = dtype(n)
    with np.errstate(all="ignore"):
        # the sequences about their first draws (a sequence of equal values is 0 exactly): d = (x - x_0) - m, mu = x_0 + m
        d, mu = [], []
        for q in sequences(x, n_chains):
            s = q - q[:, :1]
            m = _sum(s) / nn
            d.append(s - m[:, None])
            mu.append(q[:, 0] + m)

        def A(t, sel):
            acc = _sum(d[0][sel, :n - t] * d[0][sel, t:]) / nn
            for c in range(1, C):
                acc = acc + _sum(d[c][sel, :n - t] * d[c][sel, t:]) / nn
            return acc / dtype(C)

        everyone = np.ones(rows, dtype=bool)
        A0 = A(0, everyone)
        W = A0 * nn / dtype(n - 1)
        g = mu[0]
        for c in range(1, C):
            g = g + mu[c]
        g = g / dtype(C)
        B = (mu[0] - g) ** 2
        for c in range(1, C):
            B = B + (mu[c] - g) ** 2
        V = A0 + B / dtype(C - 1)
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
        tau = np.maximum(tau, dtype(1) / np.log10(dtype(C * n)))
        ess = np.where(ok, dtype(C * n) / tau, nan)
    return Sequence(ess, rhat, np.where(ok, T, -1), near & ok)


def _bulk_and_rhat(v, table, n_chains, dtype):
    table = np.asarray(table, dtype=dtype)
    bulk = E(rank_z(v, table), n_chains, dtype)
    with np.errstate(all="ignore"):
        folded_z = E(rank_z(folded(v), table), n_chains, dtype)
        rhat = np.where(np.isnan(bulk.rhat) | np.isnan(folded_z.rhat), np.nan, np.maximum(bulk.rhat, folded_z.rhat))
    return bulk, rhat


def value_diagnostics(v, table, n_chains=1, dtype=np.float64):
    """rows of per-sample values v (rows, S) -> (rhat, ess_bulk, ess_mean, mcse_mean, T of v, near of v or Z(v))"""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    S = v.shape[1]
    if S // n_chains < 8:
        nan = np.full(v.shape[0], np.nan)
        return ValueDiagnostics(nan, nan, nan, nan, np.full(v.shape[0], -1), np.zeros(v.shape[0], dtype=bool))
    with np.errstate(all="ignore"):
        plain = E(v, n_chains, dtype)
        bulk, rhat = _bulk_and_rhat(v, table, n_chains, dtype)
        _, sd = er._sd(v, dtype)
        mcse = sd / np.sqrt(plain.ess)
    bad = ~np.all(np.isfinite(v), axis=1)
    out = [np.where(bad, np.nan, o) for o in (rhat, bulk.ess, plain.ess, mcse)]
    return ValueDiagnostics(*out, plain.T, plain.near | bulk.near)


def likelihood_diagnostics(log_lik, table, n_chains=1, dtype=np.float64):
    """log_lik (S, N) as predict_log_density(pointwise=True) returns it -> per row (r_eff, rhat, ess_bulk, mcse_lpd, T of u, near)"""
    ll = np.asarray(log_lik, dtype=np.float64).T
    S = ll.shape[1]
    if S // n_chains < 8:
        nan = np.full(ll.shape[0], np.nan)
        return LikelihoodDiagnostics(nan, nan, nan, nan, np.full(ll.shape[0], -1), np.zeros(ll.shape[0], dtype=bool))
    with np.errstate(all="ignore"):
        u = np.exp(ll - ll.max(axis=1)[:, None])  # (float64: the values themselves are the device's)
        plain = E(u, n_chains, dtype)
        bulk, rhat = _bulk_and_rhat(u, table, n_chains, dtype)
        mean, sd = er._sd(u, dtype)
        mcse = sd / (mean * np.sqrt(plain.ess))
    bad = ~np.all(np.isfinite(u), axis=1)
    out = [np.where(bad, np.nan, o) for o in (plain.ess / dtype(S), rhat, bulk.ess, mcse)]
    return LikelihoodDiagnostics(*out, plain.T, plain.near | bulk.near)


# (chains, draws per chain): one chain; the shortest chains, even and odd; odd counts of odd lengths; 64 sequences, a full wavefront,
# at the shortest length and at S = 4096; four long chains, several batches of lags
CPU_SHAPES = ((1, 32), (2, 8), (3, 9), (5, 19), (7, 13), (32, 8), (32, 128), (4, 1024))
SHIFT_SD = 3.0  # how far apart, in standard deviations, the chains of the "shifted" rows sit


def cpu_cases():
    """[(name, M, L, rows (n, M L))]: per shape independent normal rows, AR(1) rows with phi = 0.98 (every chain its own stationary
    sequence), clipped rows with heavy ties (three values), Phi-saturated rows with ties (ndtr(6 + 3 normal)), and stationary chains
    whose means differ by SHIFT_SD standard deviations from one chain to the next (a single chain: its second half is shifted)"""
    from scipy.special import ndtr

    out = []
    for M, L in CPU_SHAPES:
        S = M * L
        rng = np.random.default_rng(7000 + 100 * M + L)
        n = 40 if S <= 256 else 12
        out.append(("normal", M, L, rng.normal(size=(n, S))))
        out.append(("ar1", M, L, ar1(rng, 0.98, n * M, L).reshape(n, S)))
        out.append(("clipped", M, L, np.clip(np.rint(rng.normal(size=(n, S))), -1.0, 1.0)))
        out.append(("saturated", M, L, ndtr(6.0 + 3.0 * rng.normal(size=(n, S)))))
        shift = SHIFT_SD * (np.repeat(np.arange(M), L) if M > 1 else (np.arange(L) >= L // 2).astype(np.float64))
        out.append(("shifted", M, L, rng.normal(size=(n, S)) + shift[None, :]))
    return out
