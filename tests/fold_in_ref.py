"""Fold-in of new one-hot entities (csrc/mfm_foldin.hpp) restated on the host: the reference of
tests/test_gpu_fold_in.py, proved in tests/test_fold_in_cpu.py.

A new feature u with value 1 in its rows enters the score linearly,

    score_s(x + e_u) = f_s(x) + w_u + sum_k V_uk q_sk(x),    q_sk(x) = sum_j V_s[j, k] x_j,

so under kept sample s, theta_u = (w_u, V_u1 .. V_uK) has the Gaussian posterior

    Lambda = diag(lambda) + alpha_s sum_i z_i z_i^T,   b = diag(lambda) mu + alpha_s sum_i z_i r_i,   z_i = (1, q_s(x_i)),
    r_i = y_i - f_s(x_i),   theta_mean = Lambda^-1 b,   a draw: theta_mean + L^-T eps with Lambda = L L^T.

`posterior` does this in np.longdouble with a hand-written Cholesky factorisation and triangular solves (the x87 80-bit format:
2^11 times finer than the float64 under test), `posterior_f64` in float64 with np.linalg.cholesky. A model without the linear
term drops component 0 (theta = V_u). `normals` are the draw's eps from the per-row Philox stream (tests/philox_ref.py).
"""
import numpy as np
import scipy.sparse as sps

from tests import philox_ref as ph
from tests import score_ref as sr

LD = np.longdouble
FOLDIN_DRAW_TAG = 0x464F4C44494E  # csrc/mfm_foldin.hpp
ROW_CHOICES = (0, 1, 2, 63, 64, 65, 257)
VALUES = (0.5, 1.0, 2.0)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def context_rows(rng, n, D):
    """n context rows over D columns: empty, one-hot and multi-hot (2 to 4 entries, values from VALUES) in turn"""
    indptr, indices, data = [0], [], []
    for i in range(n):
        kind = (i + int(rng.integers(3))) % 3
        m = 0 if kind == 0 else 1 if kind == 1 else int(rng.integers(2, 5))
        cols = np.sort(rng.choice(D, size=m, replace=False))
        indices.extend(int(c) for c in cols)
        data.extend([1.0] * m if kind == 1 else [float(v) for v in rng.choice(VALUES, size=m)])
        indptr.append(len(indices))
    return sps.csr_matrix((np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)),
                          shape=(n, D))


def entity_counts(rng, U, choices=ROW_CHOICES):
    """rows per entity: the choices in turn from a random start; with 5 or more entities the first, the middle and the last are empty"""
    start = int(rng.integers(len(choices)))
    cnt = np.asarray([choices[(start + u) % len(choices)] for u in range(U)], dtype=np.int64)
    if U >= 5:
        cnt[[0, U // 2, U - 1]] = 0
    return cnt


def problem(rng, D, K, S, U, scale=0.5, alpha=1.7, counts=None):
    """A fold-in problem: samples [(w0, w[D], V[D, K])] with factor scale `scale`, shuffled observations (X, y, entity), per-sample
    alpha (S,), mu and lam (S, K + 1) with the precisions in [0.5, 5]"""
    samples = [(float(rng.normal()), rng.normal(size=D) * scale, rng.normal(size=(D, K)) * scale) for _ in range(S)]
    cnt = entity_counts(rng, U) if counts is None else np.asarray(counts, dtype=np.int64)
    entity = np.repeat(np.arange(U, dtype=np.int64), cnt)
    rng.shuffle(entity)
    n = entity.shape[0]
    return dict(D=D, K=K, S=S, U=U, samples=samples, X=context_rows(rng, n, D), y=rng.normal(size=n) * 1.5 + 0.5, entity=entity,
                alpha=np.full(S, alpha), mu=rng.normal(size=(S, K + 1)) * 0.5, lam=rng.uniform(0.5, 5.0, size=(S, K + 1)),
                counts=cnt)


def grouped(X, y, entity, U):
    """the observations grouped by entity with a stable sort: (X, y, offsets (U + 1,))"""
    order = np.argsort(np.asarray(entity, dtype=np.int64), kind="stable")
    off = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(entity, dtype=np.int64), minlength=U), out=off[1:])
    return sps.csr_matrix(X)[order], np.asarray(y)[order], off


# ---- z and the residual --------------------------------------------------------------------------------------------------------
def z_and_residual(sample, X, y, dtype=LD):
    """(z (n, K + 1) with z[:, 0] = 1, r (n,)) of the rows of X under one sample, in `dtype`"""
    w0, w, V = sample
    idx, x, _ = sr.flat_rows(X)
    x, wl, Vl = x.astype(dtype), np.asarray(w)[idx].astype(dtype), np.asarray(V)[idx].astype(dtype)
    xv = x[:, :, None] * Vl
    q = xv.sum(axis=1)
    f = dtype(w0) + (x * wl).sum(axis=1) + ((q * q - (xv * xv).sum(axis=1)) / 2).sum(axis=1)
    z = np.concatenate([np.ones((X.shape[0], 1), dtype=dtype), q], axis=1)
    return z, np.asarray(y).astype(dtype) - f


def systems(p, fit_linear=True, dtype=LD):
    """(Lam (S, U, M, M), b (S, U, M), mu (S, M), lam (S, M)) in `dtype`; M = K + 1, or K without the linear term"""
    S, U, K = p["S"], p["U"], p["K"]
    o = 0 if fit_linear else 1
    M = K + 1 - o
    Xg, yg, off = grouped(p["X"], p["y"], p["entity"], U)
    mu, lam = p["mu"][:, o:].astype(dtype), p["lam"][:, o:].astype(dtype)
    Lam = np.zeros((S, U, M, M), dtype=dtype)
    b = np.zeros((S, U, M), dtype=dtype)
    for s in range(S):
        z, r = z_and_residual(p["samples"][s], Xg, yg, dtype)
        z = z[:, o:]
        a = dtype(p["alpha"][s])
        for u in range(U):
            zu, ru = z[off[u]:off[u + 1]], r[off[u]:off[u + 1]]
            Lam[s, u] = np.diag(lam[s]) + a * np.dot(zu.T, zu)
            b[s, u] = lam[s] * mu[s] + a * np.dot(zu.T, ru)
    return Lam, b, mu, lam


def cholesky_ld(A):
    """L with A = L L^T for a stack A (..., M, M), written out (no LAPACK in longdouble): column by column"""
    A = np.array(A, dtype=LD)
    M = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(M):
        d = A[..., j, j] - (L[..., j, :j] * L[..., j, :j]).sum(axis=-1)
        if not np.all(d > 0):
            raise np.linalg.LinAlgError("not positive definite")
        L[..., j, j] = np.sqrt(d)
        if j + 1 < M:
            L[..., j + 1:, j] = (A[..., j + 1:, j] - (L[..., j + 1:, :j] * L[..., j:j + 1, :j]).sum(axis=-1)) / L[..., j:j + 1, j]
    return L


def solve_lower(L, b):
    """x with L x = b (forward substitution), stacks"""
    x = np.zeros_like(b)
    for j in range(b.shape[-1]):
        x[..., j] = (b[..., j] - (L[..., j, :j] * x[..., :j]).sum(axis=-1)) / L[..., j, j]
    return x


def solve_upper_t(L, b):
    """x with L^T x = b (back substitution on the transpose), stacks"""
    x = np.zeros_like(b)
    for j in range(b.shape[-1] - 1, -1, -1):
        x[..., j] = (b[..., j] - (L[..., j + 1:, j] * x[..., j + 1:]).sum(axis=-1)) / L[..., j, j]
    return x


def posterior(p, fit_linear=True):
    """The longdouble reference: dict(theta (S, U, M) the posterior means, L (S, U, M, M), cond (S, U) = cond_2(Lambda) in
    float64, mu (S, M), lam (S, M), counts (U,)). An entity without rows has theta = mu exactly."""
    Lam, b, mu, lam = systems(p, fit_linear, LD)
    M = Lam.shape[-1]
    if M == 0:
        return dict(theta=np.zeros(b.shape, dtype=LD), L=Lam, cond=np.ones(b.shape[:2]), mu=mu, lam=lam, counts=p["counts"])
    L = cholesky_ld(Lam)
    theta = solve_upper_t(L, solve_lower(L, b))
    empty = p["counts"] == 0
    theta[:, empty] = mu[:, None, :]
    return dict(theta=theta, L=L, cond=np.linalg.cond(Lam.astype(np.float64)), mu=mu, lam=lam, counts=p["counts"])


def drawn(ref, eps):
    """theta_mean + L^-T eps in longdouble (eps (S, U, M) float64); an entity without rows: mu_j + eps_j / sqrt(lambda_j)"""
    if ref["theta"].shape[-1] == 0:
        return ref["theta"].copy()
    return ref["theta"] + solve_upper_t(ref["L"], np.asarray(eps).astype(LD))


def posterior_f64(p, fit_linear=True, eps=None):
    """The same in float64 NumPy: np.linalg.cholesky and two solves per (sample, entity); with eps, the draw"""
    Lam, b, mu, lam = systems(p, fit_linear, np.float64)
    if Lam.shape[-1] == 0:
        return np.zeros(b.shape)
    L = np.linalg.cholesky(Lam)
    Lt = np.swapaxes(L, -1, -2)
    yv = np.linalg.solve(L, b[..., None])
    if eps is not None:
        yv = yv + np.asarray(eps)[..., None]
    theta = np.linalg.solve(Lt, yv)[..., 0]
    empty = p["counts"] == 0
    theta[:, empty] = mu[:, None, :] if eps is None else mu[:, None, :] + np.asarray(eps)[:, empty] / np.sqrt(lam)[:, None, :]
    return theta


def tolerance(ref, K, theta=None):
    """(S, U): 16 (K + 1 + n_u) 2^-52 cond_2(Lambda_ref) max(|theta_ref|_inf, |mu|_inf) -- the forward bound of a Cholesky solve plus
    the summation error of the Gram sums, against the longdouble reference (`theta`: the reference draw instead of the mean)"""
    theta = np.asarray(ref["theta"] if theta is None else theta, dtype=np.float64)
    if theta.shape[-1] == 0:
        return np.zeros(theta.shape[:2])
    scale = np.maximum(np.abs(theta).max(axis=-1), np.abs(ref["mu"].astype(np.float64)).max(axis=-1)[:, None])
    return 16.0 * (K + 1 + ref["counts"][None, :]) * 2.0 ** -52 * ref["cond"] * scale


def split(theta, fit_linear, K):
    """theta (S, U, M) -> (w_new (S, U), V_new (S, U, K)) as the entry points write them (w_new = 0 without the linear term)"""
    theta = np.asarray(theta)
    if fit_linear:
        return theta[..., 0], theta[..., 1:]
    return np.zeros(theta.shape[:2], dtype=theta.dtype), theta


def join(w_new, V_new, fit_linear):
    return np.concatenate([w_new[..., None], V_new], axis=-1) if fit_linear else np.asarray(V_new)


# ---- the draw's normals ----------------------------------------------------------------------------------------------------------
def normals(seed, S, U, M):
    """eps (S, U, M): component j of (sample s, entity u) is the Box-Muller value of counter word j >> 1 of the stream keyed
    (seed, FOLDIN_DRAW_TAG, row = s U + u): r cos for even j, r sin for odd j"""
    rows = (np.arange(S, dtype=np.int64)[:, None] * U + np.arange(U, dtype=np.int64)[None, :]).ravel()
    g = ph.RowRng(seed, FOLDIN_DRAW_TAG, rows)
    eps = np.zeros((S * U, M + 1))
    for n in range((M + 1) // 2):
        ux, uy = g.next2(n)
        r = np.sqrt(-2.0 * np.log(ux))
        s, c = ph.sincospi2(uy)
        eps[:, 2 * n], eps[:, 2 * n + 1] = r * c, r * s
    return eps[:, :M].reshape(S, U, M)


# ---- the extended model ----------------------------------------------------------------------------------------------------------
def extend_sample(sample, w_new_s, V_new_s):
    """(w0, w[D + U], V[D + U, K]) of one sample extended by w_new_s (U,), V_new_s (U, K)"""
    w0, w, V = sample
    return w0, np.concatenate([w, w_new_s]), np.concatenate([V, V_new_s], axis=0)


def mean_score(samples, X):
    """mean over the samples of the float64 FM score of the rows of X (what predict returns, up to rounding)"""
    X = sps.csr_matrix(X, dtype=np.float64)
    out = np.zeros(X.shape[0])
    for w0, w, V in samples:
        q = X @ V
        out += w0 + X @ w + 0.5 * ((q * q).sum(axis=1) - (X.multiply(X) @ (V * V)).sum(axis=1))
    return out / len(samples)
