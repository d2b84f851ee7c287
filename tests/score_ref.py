"""The FM score in np.longdouble, the running-error bound of a float64 evaluation of it, and the ordered-probit class
probabilities as the kernels define them: the reference of tests/test_gpu_score_shapes.py (proved in
tests/test_score_ref_cpu.py).

The score of a row of the flat design (main CSR and the relation blocks' rows side by side, FM.hpp:47-136) is

    w0 + sum_j x_j w_j + 1/2 sum_f [ (sum_j x_j v_jf)^2 - sum_j x_j^2 v_jf^2 ]

Only the columns a row touches are gathered, so the width of the design costs nothing.

np.longdouble is the x87 80-bit format on the machines this project runs on (64-bit mantissa: 2^11 times finer than the
float64 under test). `fm_score_f64` is the float64 counterpart in the orders a kernel may take; it is what the bound is held
against on the CPU.
"""
import numpy as np
import scipy.sparse as sps
from scipy import special

LD = np.longdouble
U = 2.0 ** -53  # unit roundoff of float64
SQRT_HALF = LD(1) / np.sqrt(LD(2))
PHI_SLOPE = 0.3990  # >= max Phi' = 1 / sqrt(2 pi) = 0.39894...


def flat_rows(X, blocks=()):
    """The rows of the flat design, padded to the longest: (idx[N, L] int64, x[N, L] float64 with 0 in the padding, cnt[N]
    stored entries per flat row). Block b's columns follow the main table's and the earlier blocks'."""
    parts = [sps.csr_matrix(X, dtype=np.float64)]
    for mp, B in blocks:
        parts.append(sps.csr_matrix(B, dtype=np.float64)[np.asarray(mp, dtype=np.int64)])
    F = sps.hstack(parts, format="csr") if len(parts) > 1 else parts[0]
    cnt = np.diff(F.indptr).astype(np.int64)
    L = max(int(cnt.max()) if cnt.size else 0, 1)
    live = np.arange(L)[None, :] < cnt[:, None]
    idx = np.zeros((F.shape[0], L), dtype=np.int64)
    x = np.zeros((F.shape[0], L))
    idx[live] = F.indices
    x[live] = F.data
    return idx, x, cnt


def _gather(rows, w, V):
    idx, x, _ = rows
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError("V must be (D, K)")
    return x.astype(LD), np.asarray(w)[idx].astype(LD), V[idx].astype(LD)  # (N, L), (N, L), (N, L, K)


def fm_score_terms(X, blocks, w0, w, V, rows=None):
    """(linear[N], pair[N, K]) in longdouble: the score is w0 + linear + sum_f pair[:, f]; dropping column f of `pair` is
    the score with factor f zeroed. `rows`: flat_rows(X, blocks) when the caller has them (x may be edited)."""
    x, wl, Vl = _gather(flat_rows(X, blocks) if rows is None else rows, w, V)
    xv = x[:, :, None] * Vl
    s = xv.sum(axis=1)
    return (x * wl).sum(axis=1), (s * s - (xv * xv).sum(axis=1)) / 2


def fm_score(X, blocks, w0, w, V, rows=None):
    """FM::predict_score of every row of (main CSR X, relation blocks [(map, B), ...]) in longdouble."""
    lin, pair = fm_score_terms(X, blocks, w0, w, V, rows)
    return LD(w0) + lin + pair.sum(axis=1)


def fm_score_bound(X, blocks, w0, w, V, rows=None):
    """(M[N], tol[N]) in longdouble. M = |w0| + sum |x w| + 1/2 sum_f [(sum |x v_f|)^2 + sum x^2 v_f^2] is what the score's
    terms add up to in magnitude; tol = gamma_n M with gamma_n = n u / (1 - n u), u = 2^-53, is the running-error bound of a
    float64 evaluation in ANY fixed order of n operations per result (Higham, Accuracy and Stability of Numerical
    Algorithms, ch. 3-4). n = 2 (entries of the flat row) + 16: a sum over the row's entries has a relative error of
    gamma_entries, its square twice that, and 16 covers what follows whatever the rank: at most 6 butterfly steps, at most 4
    pairs per lane, the additions of the blocks' caches and the final `w0 +`."""
    rows = flat_rows(X, blocks) if rows is None else rows
    x, wl, Vl = _gather(rows, w, V)
    xv = np.abs(x[:, :, None] * Vl)
    s = xv.sum(axis=1)
    M = abs(LD(w0)) + np.abs(x * wl).sum(axis=1) + ((s * s).sum(axis=1) + (xv * xv).sum(axis=(1, 2))) / 2
    n = (2 * rows[2] + 16).astype(LD)
    return M, n * LD(U) / (1 - n * LD(U)) * M


def phi(z):
    """Phi(z) = (1 + erf(z / sqrt 2)) / 2 as the kernels write it: erf (scipy's) on the float64 argument, the rest in longdouble"""
    arg = np.asarray(np.asarray(z, dtype=LD) * SQRT_HALF, dtype=np.float64)
    return (1 + special.erf(arg).astype(LD)) / 2


def class_probs(score, cut):
    """Ordered-probit class probabilities (FM.hpp:150-161) of score[N] under the cutpoints cut[n_cut], (N, n_cut + 1):
    differences of adjacent CDFs Phi(cut_c - score), 1 - the last CDF for the last class."""
    score = np.asarray(score, dtype=LD)
    cut = np.asarray(cut, dtype=LD)
    cdf = phi(cut[None, :] - score[:, None])
    out = np.empty((score.shape[0], cut.shape[0] + 1), dtype=LD)
    out[:, 0] = cdf[:, 0]
    out[:, 1:-1] = cdf[:, 1:] - cdf[:, :-1]
    out[:, -1] = 1 - cdf[:, -1]
    return out


def score_shape(K):
    """(GS lanes per row, SPL factor pairs per lane) of the scorer at rank K: csrc/mfm_hip.hip score_shape"""
    for top, shape in ((8, (4, 1)), (16, (8, 1)), (32, (16, 1)), (64, (32, 1)), (128, (64, 1)), (256, (64, 2)), (512, (64, 4))):
        if K <= top:
            return shape
    raise ValueError("rank > 512 is not supported")


def fm_score_f64(X, blocks, w0, w, V, order, rows=None):
    """The score in float64, every addition in a stated order. `order`: 'ascending' / 'descending' add the factors' terms
    one by one in that order of f, the entries of a row in stored / reverse order; 'tree' is k_score's: lane l of GS owns
    the factor pairs l, l + GS, ..., adds their squares, subtracts its share of sum x^2 v^2 (added entry by entry), lane 0
    takes the linear term, and the lanes' parts meet in a butterfly."""
    idx, x, _ = flat_rows(X, blocks) if rows is None else rows
    w, V = np.asarray(w, dtype=np.float64), np.asarray(V, dtype=np.float64)
    N, L = x.shape
    K = V.shape[1]
    entries = range(L - 1, -1, -1) if order == "descending" else range(L)
    if order in ("ascending", "descending"):
        a, b, lin = np.zeros((N, K)), np.zeros((N, K)), np.zeros(N)
        for l in entries:
            xl, vl = x[:, l], V[idx[:, l]]
            lin += xl * w[idx[:, l]]
            a += xl[:, None] * vl
            b += (xl * xl)[:, None] * (vl * vl)
        t = a * a - b
        s = np.zeros(N)
        for f in (range(K - 1, -1, -1) if order == "descending" else range(K)):
            s += t[:, f]
        return w0 + (0.5 * s + lin)
    if order != "tree":
        raise ValueError(order)
    GS, SPL = score_shape(K)
    Vp = np.zeros((V.shape[0], 2 * GS * SPL))
    Vp[:, :K] = V
    Vp = Vp.reshape(V.shape[0], SPL, GS, 2)  # [j][s][lane][x | y]: pair s * GS + lane
    a = np.zeros((N, SPL, GS, 2))
    b, lin = np.zeros((N, GS)), np.zeros(N)
    for l in entries:
        xl, vl = x[:, l], Vp[idx[:, l]]
        x2 = xl * xl
        lin += xl * w[idx[:, l]]
        a += xl[:, None, None, None] * vl
        for s in range(SPL):
            b += x2[:, None] * (vl[:, s, :, 0] * vl[:, s, :, 0])
            b += x2[:, None] * (vl[:, s, :, 1] * vl[:, s, :, 1])
    part = np.zeros((N, GS))
    for s in range(SPL):
        part += a[:, s, :, 0] * a[:, s, :, 0] + a[:, s, :, 1] * a[:, s, :, 1]
    part = 0.5 * (part - b)
    part[:, 0] += lin
    m = GS // 2
    while m >= 1:  # (lane 0's view of the butterfly: the sum of lanes l and l + m, halving)
        part = part[:, :m] + part[:, m:2 * m]
        m //= 2
    return w0 + part[:, 0]
