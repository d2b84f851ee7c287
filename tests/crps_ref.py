"""NumPy / SciPy reference of the continuous ranked probability score (predict_crps), from the per-sample scores
(S, N), and its mpmath twin at 40 digits.

The float64 form is vectorised over the rows and adds in the orders the device defines: regression, the pair terms of sample s over
t = 0 .. s - 1 into one sum per s (np.cumsum along the t axis: sequential, not .sum()'s pairwise order), then those sums in s order;
classification and ordered probit, the samples in order per cut, then the cuts in order. So the summation error of the device is
the reference's own, and what is left between the two is how erf / erfc / exp round on either side.

How two values are compared: |a - b| / max(1, |b|). CRPS_RTOL bounds that deviation between the code under test and this reference.
It is 8 x the largest deviation of this float64 reference from the mpmath twin over tolerance_cases() -- rows drawn as the tests
draw theirs (all three tasks; S = 1, 2, 9, 33 and 200; targets up to 40 sigma away; equal samples): the factor is the project's
margin for a device erf / exp that rounds a few ulp differently from libm, the measured part carries the
sequential sums. Measured: 7.4e-16 (the regression crps at S = 200; at most 4.5e-16 on every other case, 3.4e-16 at S <= 33 of the random rows);
tests/test_crps_cpu.py measures it again and checks that it has not grown."""
import numpy as np
from scipy.special import erf, erfc, ndtr

CRPS_MEASURED_DEVIATION = 7.4e-16
CRPS_RTOL = 8 * CRPS_MEASURED_DEVIATION

INV_SQRT2 = 0.70710678118654752440


def deviation(a, b):
    """|a - b| / max(1, |b|), elementwise"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def constants(v):
    """(h, g) of A(., v): h = 1 / sqrt(2 v), g = sqrt(2 v / pi)"""
    v2 = 2.0 * np.asarray(v, dtype=np.float64)
    return 1.0 / np.sqrt(v2), np.sqrt(v2 / np.pi)


def abs_normal(m, h, g):
    """A(m, v) = E|N(m, v)| = m erf(m h) + g exp(-(m h)^2)"""
    z = m * h
    return m * erf(z) + g * np.exp(-(z * z))


def crps_mixture(scores, y, precisions):
    """(crps, accuracy, spread), (N,) each, of y under mean_s N(scores[s], 1 / precisions[s]); scores (S, N)"""
    f = np.asarray(scores, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    v = 1.0 / np.asarray(precisions, dtype=np.float64)
    S, N = f.shape
    inv_S = 1.0 / S
    h, g = constants(v)
    acc, total = np.zeros(N), np.zeros(N)
    for s in range(S):
        acc = acc + abs_normal(y - f[s], h[s], g[s])
        p = np.zeros(N)
        if s > 0:
            hp, gp = constants(v[s] + v[:s])
            p = p + np.cumsum(abs_normal(f[s][None, :] - f[:s], hp[:, None], gp[:, None]), axis=0)[-1]
        p = p + 0.5 * constants(v[s] + v[s])[1]
        total = total + p
    accuracy, spread = acc * inv_S, (total * inv_S) * inv_S
    return accuracy - spread, accuracy, spread


def crps_classes(scores, y, cutpoints=None):
    """(crps, accuracy, spread), (N,) each, of the class index y under the posterior mean class probabilities; cutpoints (S, n_cut),
    None for a classifier (one cutpoint 0, y in {0, 1})"""
    f = np.asarray(scores, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    S, N = f.shape
    cut = np.zeros((S, 1)) if cutpoints is None else np.asarray(cutpoints, dtype=np.float64)
    inv_S = 1.0 / S
    accuracy, spread, crps = np.zeros(N), np.zeros(N), np.zeros(N)
    for j in range(cut.shape[1]):
        t = cut[:, j][:, None] - f
        d = np.cumsum(0.5 * erfc(np.where((y > j)[None, :], -t, t) * INV_SQRT2), axis=0)[-1] * inv_S
        accuracy = accuracy + d
        spread = spread + d * (1.0 - d)
        crps = crps + d * d
    return crps, accuracy, spread


def crps(task, scores, y, precisions=None, cutpoints=None):
    """task 0 regression, 1 classification, 2 ordered probit"""
    return crps_mixture(scores, y, precisions) if task == 0 else crps_classes(scores, y, cutpoints if task == 2 else None)


def class_probs(scores, cutpoints=None):
    """(N, C) posterior mean class probabilities, as differences of ndtr; a classifier: C = 2"""
    f = np.asarray(scores, dtype=np.float64)
    S = f.shape[0]
    cut = np.zeros((S, 1)) if cutpoints is None else np.asarray(cutpoints, dtype=np.float64)
    cdf = np.concatenate([np.zeros((S, 1, f.shape[1])), ndtr(cut[:, :, None] - f[:, None, :]), np.ones((S, 1, f.shape[1]))], axis=1)
    return np.diff(cdf, axis=1).mean(axis=0).T


def crps_mp(task, scores, y, precisions=None, cutpoints=None, dps=40):
    """the same three values at `dps` digits (mpmath), row by row: (3, N) float64 of the rounded results. About 0.03 s per row at
    S = 33 and 1.2 s at S = 200."""
    import mpmath as mp

    f = np.asarray(scores, dtype=np.float64)
    S, N = f.shape
    out = np.empty((3, N))
    with mp.workdps(dps):
        half, two = mp.mpf(1) / 2, mp.mpf(2)

        def A(m, v):
            return m * mp.erf(m / mp.sqrt(two * v)) + mp.sqrt(two * v / mp.pi) * mp.exp(-m * m / (two * v))

        for n in range(N):
            yn = mp.mpf(float(y[n]))
            fs = [mp.mpf(float(x)) for x in f[:, n]]
            if task == 0:
                v = [1 / mp.mpf(float(p)) for p in precisions]
                acc = sum(A(yn - fs[s], v[s]) for s in range(S)) / S
                spr = sum(sum(A(fs[s] - fs[t], v[s] + v[t]) for t in range(s)) + mp.sqrt(two * two * v[s] / mp.pi) / 2 for s in range(S)) / (S * S)
                res = (acc - spr, acc, spr)
            else:
                n_cut = cutpoints.shape[1] if task == 2 else 1
                crps_, acc, spr = mp.mpf(0), mp.mpf(0), mp.mpf(0)
                for j in range(n_cut):
                    F = sum(half * mp.erfc(-((mp.mpf(float(cutpoints[s, j])) if task == 2 else 0) - fs[s]) / mp.sqrt(two)) for s in range(S)) / S
                    d = F if float(y[n]) > j else 1 - F
                    acc, spr, crps_ = acc + d, spr + d * (1 - d), crps_ + d * d
                res = (crps_, acc, spr)
            out[:, n] = [float(r) for r in res]
    return out


def spaced_cutpoints(rng, S, n_cut):
    """(S, n_cut) ascending cutpoints with spacings in [0.05, 0.8]"""
    return -2.0 + rng.normal(size=(S, 1)) * 0.5 + np.cumsum(rng.uniform(0.05, 0.8, size=(S, n_cut)), axis=1)


def random_rows(task, S, N, seed, far=0.0, equal=False, n_cut=4):
    """(scores (S, N), y, precisions, cutpoints) of N random rows over S samples, drawn as the GPU tests draw their host samples
    (scores of standard deviation 0.8, precisions exp(U(-1, 2)), spaced cutpoints). far: the targets (regression) or the scores
    (classification, ordered probit) are moved up to `far` standard deviations of the noise away; equal: all samples alike."""
    rng = np.random.default_rng(seed)
    f = 0.8 * rng.normal(size=(S, N))
    prec = np.exp(rng.uniform(-1.0, 2.0, size=S)) if task == 0 else None
    cut = spaced_cutpoints(rng, S, n_cut) if task == 2 else None
    if equal:
        f = np.repeat(f[:1], S, axis=0)
        prec = None if prec is None else np.repeat(prec[:1], S)
        cut = None if cut is None else np.repeat(cut[:1], S, axis=0)
    shift = far * np.linspace(-1.0, 1.0, N)
    if task == 0:
        y = rng.normal(size=N) + shift / np.sqrt(prec.min())
    else:
        f = f + shift[None, :]
        y = (rng.random(N) < 0.5).astype(np.float64) if task == 1 else rng.integers(0, n_cut + 1, size=N).astype(np.float64)
    return f, y, prec, cut


def tolerance_cases():
    """the inputs CRPS_MEASURED_DEVIATION is measured on: (task, scores, y, precisions, cutpoints)"""
    cases = []
    for task in (0, 1, 2):
        for S, N in ((1, 12), (2, 12), (9, 12), (33, 12), (200, 2 if task == 0 else 4)):
            cases.append((task,) + random_rows(task, S, N, 100 * task + S))
        cases.append((task,) + random_rows(task, 9, 9, 100 * task + 50, far=40.0))
        cases.append((task,) + random_rows(task, 33, 6, 100 * task + 51, far=8.0))
        cases.append((task,) + random_rows(task, 9, 6, 100 * task + 52, equal=True))
    return cases


def measured_deviation():
    """the largest deviation of the float64 reference from the mpmath twin over tolerance_cases(), all three outputs"""
    worst = 0.0
    for task, f, y, prec, cut in tolerance_cases():
        got = np.stack(crps(task, f, y, prec, cut))
        worst = max(worst, float(deviation(got, crps_mp(task, f, y, prec, cut)).max()))
    return worst
