"""Reference of the analytic score moments of the variational estimators, in np.longdouble. Posterior: w0 ~ N(w0,
w0_var), w_j ~ N(w_j, wv_j), V_jk ~ N(m_jk, s_jk), all independent; model = (w0, w0_var, w[D], w_var[D], V[D, K], V_var[D, K]).

Two independent restatements of Var[score] of a row:
  closed_form  the five sums per factor, M = sum x m, A = sum x^2 s, B = sum x^3 s m, C = sum x^4 s m^2, E = sum x^4 s^2:
               Var = w0_var + sum x^2 wv + sum_k [M^2 A - 2 M B + C + (A^2 - E) / 2]_k
  brute_force  the score's pair part is sum over feature pairs p = (i < j) and factors k of a_pk = x_i x_j V_ik V_jk; its variance
               is sum_{p, q} E[a_pk a_qk] - E[a_pk] E[a_qk] over all pairs of pairs (factors are independent), every expectation
               a product of first and second moments of the V involved. O(nnz^4) per factor: rows of at most 6 entries.
and the dense-row helper for (query, candidate) pairs: the pair row a_u + b_i is built and handed to the closed form.

Error model of the closed form in fp64, used by the GPU tests as |got - ref| <= (n + 8) eps scale:
  scale  the same expression with every term replaced by its absolute value (M -> sum |x m|, B -> sum |x^3 s m|, minus -> plus):
         it bounds every intermediate of any association, the per-side and cross terms of the pair split included;
  n      the additions on the longest path: each of the five sums takes nnz (+ one per extra part of the row) additions and a term
         is a product of at most three sums, so 3 (nnz + parts + 2); the factors and the lanes' partial sums add K + 8 more (the
         pair form adds its contraction of length 4 K). The 8 of (n + 8) are the roundings inside one term.
"""
import itertools
from collections import Counter, namedtuple

import numpy as np
import scipy.sparse as sps

LD = np.longdouble
EPS = 2.0 ** -53

Moments = namedtuple("Moments", ["mean", "var", "scale", "n", "mean_scale"])


def _model_ld(model):
    w0, w0_var, w, w_var, V, V_var = model
    V = np.asarray(V, dtype=LD)
    return LD(w0), LD(w0_var), np.asarray(w, dtype=LD), np.asarray(w_var, dtype=LD), V, np.asarray(V_var, dtype=LD).reshape(V.shape)


def closed_form(X, model, extra_var=0.0, n_parts=1, contraction=0):
    """Moments(mean, var, scale, n, mean_scale), arrays over the rows of X (sparse or dense (R, D)); mean and var longdouble, scale
    and mean_scale float64, n int64. n_parts: the parts a row is summed from (main table + relation blocks); contraction: extra
    additions of the pair form."""
    w0, w0v, w, wv, m, s = _model_ld(model)
    X = np.asarray(X.todense() if sps.issparse(X) else X, dtype=LD)
    X2 = X * X
    X3, X4 = X2 * X, X2 * X2
    aX = np.abs(X)
    K = m.shape[1]
    M, A, B = X @ m, X2 @ s, X3 @ (s * m)
    C, E, S2 = X4 @ (s * m * m), X4 @ (s * s), X2 @ (m * m)
    lin, lv = X @ w, X2 @ wv
    mean = w0 + lin + LD(0.5) * (M * M - S2).sum(axis=1)
    var = w0v + LD(extra_var) + lv + (M * M * A - 2 * M * B + C + LD(0.5) * (A * A - E)).sum(axis=1)
    Mb, Bb = aX @ np.abs(m), (aX * X2) @ (s * np.abs(m))
    scale = w0v + LD(extra_var) + lv + (Mb * Mb * A + 2 * Mb * Bb + C + LD(0.5) * (A * A + E)).sum(axis=1)
    mean_scale = abs(w0) + aX @ np.abs(w) + LD(0.5) * (Mb * Mb + S2).sum(axis=1)
    nnz = np.asarray((X != 0).sum(axis=1)).ravel().astype(np.int64)
    n = 3 * (nnz + n_parts + 2) + K + 8 + contraction
    return Moments(mean, var, np.asarray(scale, dtype=np.float64), n, np.asarray(mean_scale, dtype=np.float64))


def brute_force_var(cols, vals, model, extra_var=0.0):
    """Var[score] of ONE row with entries (cols, vals), at most 6 of them, by enumeration over all pairs of feature pairs"""
    w0, w0v, w, wv, m, s = _model_ld(model)
    cols = [int(c) for c in cols]
    x = [LD(v) for v in vals]
    assert len(cols) <= 6 and len(set(cols)) == len(cols)
    var = w0v + LD(extra_var)
    for c, v in zip(cols, x):
        var += v * v * wv[c]
    pairs = list(itertools.combinations(range(len(cols)), 2))
    for k in range(m.shape[1]):
        first = {p: m[cols[p[0]], k] * m[cols[p[1]], k] for p in pairs}
        for p in pairs:
            for q in pairs:
                e = LD(1.0)
                for f, c in Counter(p + q).items():
                    mf, sf = m[cols[f], k], s[cols[f], k]
                    e *= mf if c == 1 else mf * mf + sf
                var += x[p[0]] * x[p[1]] * x[q[0]] * x[q[1]] * (e - first[p] * first[q])
    return var


def pair_rows(Xq, Xc):
    """dense (U * I, D): row u * I + i = Xq[u] + Xc[i] (the sides store disjoint columns)"""
    A = np.asarray(sps.csr_matrix(Xq, dtype=np.float64).todense())
    B = np.asarray(sps.csr_matrix(Xc, dtype=np.float64).todense())
    return (A[:, None, :] + B[None, :, :]).reshape(A.shape[0] * B.shape[0], A.shape[1])


def pairs_closed_form(Xq, Xc, model, extra_var=0.0, n_parts=2):
    """Moments with (U, I) arrays: the closed form of every dense pair row"""
    U, I = Xq.shape[0], Xc.shape[0]
    K = np.asarray(model[4]).shape[1]
    r = closed_form(pair_rows(Xq, Xc), model, extra_var, n_parts=n_parts, contraction=4 * K)
    return Moments(*(np.asarray(a).reshape(U, I) for a in r))


def pair_split_var(aq, ac, model):
    """Var[score] of one pair from its halves aq, ac (dense (D,) rows with disjoint support): the per-side closed forms plus the
    contraction of the query tables (Mq^2, Mq Aq - Bq, Mq, Aq) with the candidate tables (Ac, 2 Mc, 2 Mc Ac - 2 Bc, Mc^2 + Ac)"""
    w0, w0v, w, wv, m, s = _model_ld(model)

    def sums(a):
        a = np.asarray(a, dtype=LD)
        a2 = a * a
        return a @ m, a2 @ s, (a2 * a) @ (s * m), (a2 * a2) @ (s * m * m), (a2 * a2) @ (s * s), a2 @ wv

    def bracket(M, A, B, C, E):
        return (M * M * A - 2 * M * B + C + LD(0.5) * (A * A - E)).sum()

    Mq, Aq, Bq, Cq, Eq, lq = sums(aq)
    Mc, Ac, Bc, Cc, Ec, lc = sums(ac)
    cross = (Mq * Mq * Ac + (Mq * Aq - Bq) * 2 * Mc + Mq * (2 * Mc * Ac - 2 * Bc) + Aq * (Mc * Mc + Ac)).sum()
    return (w0v + lq + bracket(Mq, Aq, Bq, Cq, Eq)) + (lc + bracket(Mc, Ac, Bc, Cc, Ec)) + cross


def exact_model(rng, D, K):
    """means in small integers, variances in {1/4, 1/2, 1}: with x in {-2, ..., 2} every product and sum of the moments is exact
    in fp64 (the largest term, x^4 s m^2 summed over a few entries and factors, stays far below 2^53 quarter units)"""
    iv = lambda shape: rng.integers(-2, 3, size=shape).astype(np.float64)  # noqa: E731
    vv = lambda shape: rng.choice([0.25, 0.5, 1.0], size=shape)  # noqa: E731
    return float(rng.integers(-2, 3)), float(rng.choice([0.25, 0.5, 1.0])), iv(D), vv(D), iv((D, K)), vv((D, K))


def normal_model(rng, D, K, scale=0.3):
    return (float(rng.normal()), float(rng.uniform(0.01, 0.1)), rng.normal(size=D) * scale, rng.uniform(0.01, 0.1, size=D),
            rng.normal(size=(D, K)) * scale, rng.uniform(0.005, 0.1, size=(D, K)))


def var_bound(mo):
    """(n + 8) eps scale: the forward bound of the closed form in fp64"""
    return (mo.n + 8) * EPS * mo.scale


def mean_bound(mo):
    return (mo.n + 8) * EPS * mo.mean_scale


def std_bounds(mo):
    """the bound on std^2 (the variance bound plus the square root's and the squaring's own roundings) and, from it, on std:
    |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(max(a, b)) and <= sqrt(|a - b|)"""
    var = np.maximum(np.asarray(mo.var, dtype=np.float64), 0.0)
    b2 = var_bound(mo) + 2 * EPS * var
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.minimum(np.sqrt(b2), np.where(var > 0, b2 / np.sqrt(var), np.inf)) + EPS * np.sqrt(var)
    return b2, b
