"""NumPy fp64 reference of the query x candidate scorer, computed the direct way: every pair row
X_query[u] + X_cand[i] is built and the FM formula is applied to it per sample. A sample is (w0, w[D], V[D, K])."""
import numpy as np
import scipy.sparse as sps
from scipy import special


def _pair_rows(Xq, Xc):
    """dense (U * I, D): row u * I + i = Xq[u] + Xc[i]"""
    A = np.asarray(sps.csr_matrix(Xq, dtype=np.float64).todense())
    B = np.asarray(sps.csr_matrix(Xc, dtype=np.float64).todense())
    U, I = A.shape[0], B.shape[0]
    return (A[:, None, :] + B[None, :, :]).reshape(U * I, A.shape[1]), U, I


def _sample_scores(X, w0, w, V):
    """w0 + X w + 1/2 sum_k [ (X V)_k^2 - (X^2 V^2)_k ] per row of the dense X"""
    w, V = np.asarray(w, dtype=np.float64), np.asarray(V, dtype=np.float64)
    s = w0 + X @ w
    if V.shape[1]:
        s = s + 0.5 * (((X @ V) ** 2).sum(axis=1) - ((X ** 2) @ (V ** 2)).sum(axis=1))
    return s


def pair_scores(samples, Xq, Xc, mode):
    """(U, I): mode 0 the mean over the samples of the score, mode 1 of Phi(score); summed in sample order, then divided"""
    X, U, I = _pair_rows(Xq, Xc)
    acc = np.zeros(U * I)
    for w0, w, V in samples:
        s = _sample_scores(X, w0, w, V)
        acc = acc + ((1.0 + special.erf(s * np.sqrt(0.5))) / 2.0 if mode == 1 else s)
    return (acc / len(samples)).reshape(U, I)


def pair_scores_abs(samples, Xq, Xc):
    """(U, I): the mean over the samples of the same sums with every term replaced by its absolute value, including the
    pieces the decomposition adds and cancels -- the scale of the rounding error of any association of them"""
    X, U, I = _pair_rows(Xq, Xc)
    X = np.abs(X)
    acc = np.zeros(U * I)
    for w0, w, V in samples:
        w, V = np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(V, dtype=np.float64))
        s = abs(w0) + X @ w
        if V.shape[1]:
            s = s + 0.5 * (((X @ V) ** 2).sum(axis=1) + ((X ** 2) @ (V ** 2)).sum(axis=1))
        acc = acc + s
    return (acc / len(samples)).reshape(U, I)


def topk(scores, k, exclude=None):
    """(indices int64 (U, k), values (U, k)) under (value descending, index ascending); excluded pairs (stored positions of
    the sparse `exclude`) left out; tail index -1 / value -inf"""
    scores = np.asarray(scores, dtype=np.float64)
    U, I = scores.shape
    idx = np.full((U, k), -1, dtype=np.int64)
    val = np.full((U, k), -np.inf)
    E = None if exclude is None else sps.csr_matrix(exclude)
    for u in range(U):
        keep = np.ones(I, dtype=bool)
        if E is not None:
            keep[E.indices[E.indptr[u]:E.indptr[u + 1]]] = False
        cand = np.flatnonzero(keep)
        order = cand[np.lexsort((cand, -scores[u, cand]))][:k]
        idx[u, :order.size] = order
        val[u, :order.size] = scores[u, order]
    return idx, val


def decomposed_scores(samples, Xq, Xc, mode):
    """the decomposition the device computes, restated: per-side embeddings P, Q and biases A, B, then
    w0 + A[u] + B[i] + P[u] . Q[i] per sample"""
    A_ = sps.csr_matrix(Xq, dtype=np.float64)
    B_ = sps.csr_matrix(Xc, dtype=np.float64)
    A2, B2 = A_.multiply(A_), B_.multiply(B_)
    acc = np.zeros((A_.shape[0], B_.shape[0]))
    for w0, w, V in samples:
        w, V = np.asarray(w, dtype=np.float64), np.asarray(V, dtype=np.float64)
        P, Q = A_ @ V, B_ @ V
        a = A_ @ w + 0.5 * ((P ** 2).sum(axis=1) - (A2 @ (V ** 2)).sum(axis=1))
        b = B_ @ w + 0.5 * ((Q ** 2).sum(axis=1) - (B2 @ (V ** 2)).sum(axis=1))
        s = w0 + a[:, None] + b[None, :] + P @ Q.T
        acc = acc + ((1.0 + special.erf(s * np.sqrt(0.5))) / 2.0 if mode == 1 else s)
    return acc / len(samples)


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
def disjoint_sides(rng, U, I, Dq, Dc, values, mean_nnz=2.5, empty_every=7):
    """multi-hot sides over disjoint column ranges of a D = Dq + Dc + 3 feature space (the last 3 columns are in neither),
    values drawn from `values`, every `empty_every`-th row empty"""
    D = Dq + Dc + 3

    def side(R, lo, n):
        rows, cols, vals = [], [], []
        for r in range(R):
            if empty_every and r % empty_every == empty_every - 1:
                continue
            m = min(n, 1 + rng.poisson(mean_nnz - 1))
            c = rng.choice(n, size=m, replace=False)
            rows += [r] * m
            cols += list(lo + c)
            vals += list(rng.choice(values, size=m))
        return sps.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(R, D))

    return side(U, 0, Dq), side(I, Dq, Dc), D


def exact_samples(rng, D, K, S):
    """samples of small integers and halves: with side values from the same set every sum of the scorer is exact in fp64"""
    out = []
    for _ in range(S):
        w0 = float(rng.integers(-4, 5)) / 2
        w = rng.integers(-4, 5, size=D) / 2.0
        V = rng.integers(-2, 3, size=(D, K)) / 2.0
        out.append((w0, w, V))
    return out


def normal_samples(rng, D, K, S, scale=0.4):
    return [(float(rng.normal()), rng.normal(size=D) * scale, rng.normal(size=(D, K)) * scale) for _ in range(S)]
