"""Reference of the similarity forms of the query x candidate family: per kept sample the embeddings P_s = X V_s of
two sets of side rows, their normalisation r and the cosine (or inner product) of every pair in np.longdouble; the float64 twin
that restates the device's operations in their order; the first-order tolerance the tests hold the device to; and exact inputs
on which every quantity is exact in fp64 under any association. A sample is (w0, w[D], V[D, K]); w0 and w play no part."""
import numpy as np
import scipy.sparse as sps

from tests import pairs_ucb_ref as ur

LD = np.longdouble
METRICS = ("cosine", "dot")


def _dense(X, dtype):
    return np.asarray(sps.csr_matrix(X, dtype=np.float64).todense()).astype(dtype)


# ---- the longdouble reference -------------------------------------------------------------------------------------------------------
def embeddings_ld(samples, X):
    """(S, R, K) longdouble: P_s[r, k] = sum_j V_s[j, k] x_rj"""
    A = _dense(X, LD)
    return np.stack([A @ np.asarray(V, dtype=np.float64).astype(LD) for _, _, V in samples]) if samples else np.zeros((0,) + A.shape[:1] + (0,), LD)


def inv_norm_ld(P):
    """(S, R) longdouble: r = 1 / sqrt(sum_k P_k^2), 0 where the sum is 0"""
    sq = (P * P).sum(axis=-1)
    r = np.zeros(sq.shape, dtype=LD)
    np.divide(LD(1), np.sqrt(sq), out=r, where=sq > 0)
    return r


def sample_values(samples, Xa, Xb, metric):
    """(S, U, I) longdouble: c_s of every pair"""
    assert metric in METRICS
    P, Q = embeddings_ld(samples, Xa), embeddings_ld(samples, Xb)
    c = np.einsum("suk,sik->sui", P, Q)
    if metric == "cosine":
        c = c * inv_norm_ld(P)[:, :, None] * inv_norm_ld(Q)[:, None, :]
    return c


def moments(samples, Xa, Xb, metric):
    """(mean, std) longdouble (U, I) over the samples, ddof = 0"""
    return ur.moments_ld(sample_values(samples, Xa, Xb, metric))


# ---- the float64 twin: the device's operations in their order ----------------------------------------------------------------------------
def _embed_twin(V, X):
    """(P (R, K), r (R,)) float64: per row and factor a += x * v over the row's entries in CSR order; sq += a * a in factor order;
    r = 1 / sqrt(sq), 0 where sq is 0 (k_pairs_embed)"""
    X = sps.csr_matrix(X, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    R, K = X.shape[0], V.shape[1]
    P, sq = np.zeros((R, K)), np.zeros(R)
    for r in range(R):
        for k in range(K):
            a = np.float64(0.0)
            for p in range(X.indptr[r], X.indptr[r + 1]):
                a = a + X.data[p] * V[X.indices[p], k]
            P[r, k] = a
            sq[r] = sq[r] + a * a
    rn = np.zeros(R)
    np.divide(1.0, np.sqrt(sq), out=rn, where=sq > 0)
    return P, rn


def twin_sample_values(samples, Xa, Xb, metric, reverse=False):
    """(S, U, I) float64: per sample the inner product summed factor by factor (k_pairs_moments_at's order; `reverse`: from the last
    factor down, another association), then (dot * r_a) * r_b"""
    out = []
    for _, _, V in samples:
        P, ra = _embed_twin(V, Xa)
        Q, rb = _embed_twin(V, Xb)
        if metric == "dot":
            ra, rb = np.ones_like(ra), np.ones_like(rb)
        dot = np.zeros((P.shape[0], Q.shape[0]))
        ks = range(P.shape[1] - 1, -1, -1) if reverse else range(P.shape[1])
        for k in ks:
            dot = dot + P[:, k][:, None] * Q[:, k][None, :]
        out.append((dot * ra[:, None]) * rb[None, :])
    return np.asarray(out).reshape(len(samples), Xa.shape[0], Xb.shape[0])


def twin_moments(samples, Xa, Xb, metric, reverse=False):
    """(mean, std) float64 by the kernels' Welford recurrence in sample order"""
    return ur.welford_twin(twin_sample_values(samples, Xa, Xb, metric, reverse))


# ---- the tolerance (first order) ------------------------------------------------------------------------------------------------------
def brackets(samples, Xa, Xb, metric):
    """(S, U, I) float64: the condition of c_s against rounding of the embeddings' terms. With pbar = |a| |V| the embedding of
    absolute terms,
        cosine: sum_k (pbar_k |q_k| + |p_k| qbar_k) / (|p| |q|) + |c| (sum_k pbar_k |p_k| / |p|^2 + sum_k qbar_k |q_k| / |q|^2)
        dot:    sum_k (pbar_k |q_k| + |p_k| qbar_k)
    0 where a norm is 0 (the value is exactly 0 there)."""
    A, B = np.abs(_dense(Xa, np.float64)), np.abs(_dense(Xb, np.float64))
    P, Q = embeddings_ld(samples, Xa).astype(np.float64), embeddings_ld(samples, Xb).astype(np.float64)
    out = np.zeros((len(samples), A.shape[0], B.shape[0]))
    for s, (_, _, V) in enumerate(samples):
        Va = np.abs(np.asarray(V, dtype=np.float64))
        Pb, Qb, p, q = A @ Va, B @ Va, np.abs(P[s]), np.abs(Q[s])
        num = Pb @ q.T + p @ Qb.T
        if metric == "dot":
            out[s] = num
            continue
        n2p, n2q = (p * p).sum(axis=1), (q * q).sum(axis=1)
        ok = (n2p[:, None] > 0) & (n2q[None, :] > 0)
        sp, sq_ = np.where(n2p > 0, n2p, 1.0), np.where(n2q > 0, n2q, 1.0)
        c = np.abs(P[s] @ Q[s].T) / np.sqrt(sp[:, None] * sq_[None, :])
        own = ((Pb * p).sum(axis=1) / sp)[:, None] + ((Qb * q).sum(axis=1) / sq_)[None, :]
        out[s] = np.where(ok, num / np.sqrt(sp[:, None] * sq_[None, :]) + c * own, 0.0)
    return out


def bounds(samples, Xa, Xb, metric, vals):
    """(mean's bound, std's bound), each (U, I): b_s = 1e-10 * bracket_s + 1e-15 (the constant is test_gpu_pairs.mode_bound's: n <=
    1e4 terms, times 100 for the association); mean: mean_s b_s; std: max_s b_s + 4 S 2^-53 rms_s(c_s) + 1e-300."""
    b = 1e-10 * brackets(samples, Xa, Xb, metric) + 1e-15
    return b.mean(axis=0), b.max(axis=0) + ur.recurrence_term(vals) + 1e-300


# ---- exact inputs -----------------------------------------------------------------------------------------------------------------------
def exact_unit_samples(rng, D, K, S):
    """every column of V holds n in {0, 1, 4, 16} (n <= K) nonzero factors of one magnitude 2^e, e in [-2, 2], with random signs:
    with side rows of at most one stored entry from {0.5, 1, 2} every norm is a power of two, so r, the cosine and the inner
    product are exact in fp64 under any association, and with S <= 2 so are the mean and std = |a - b| / 2"""
    out = []
    for _ in range(S):
        V = np.zeros((D, K))
        for j in range(D):
            n = int(rng.choice([n for n in (0, 1, 4, 16) if n <= K]))
            if n:
                at = rng.choice(K, size=n, replace=False)
                V[j, at] = rng.choice([-1.0, 1.0], size=n) * 2.0 ** int(rng.integers(-2, 3))
        out.append((float(rng.integers(-4, 5)) / 2, rng.integers(-4, 5, size=D) / 2.0, V))
    return out


UNIT_VALUES = (0.5, 1.0, 2.0)


def unit_sides(rng, U, I, D, shared, empty_every=5):
    """side rows of at most one stored entry from UNIT_VALUES, every `empty_every`-th row empty. shared: both sides draw their
    columns from all of [0, D) and the candidates' first rows are the queries themselves (the candidates are a superset of the
    queries when I >= U); else the queries use the first half of the columns and the candidates the second."""
    def side(R, lo, hi):
        rows = [r for r in range(R) if not (empty_every and r % empty_every == empty_every - 1)]
        cols = rng.integers(lo, hi, size=len(rows))
        vals = rng.choice(UNIT_VALUES, size=len(rows))
        return sps.csr_matrix((vals, (rows, cols)), shape=(R, D))

    if not shared:
        return side(U, 0, D // 2), side(I, D // 2, D)
    Xq, Xc = side(U, 0, D), side(I, 0, D)
    n = min(U, I)
    Xc = sps.vstack([Xq[:n], Xc[n:]], format="csr")
    return Xq, Xc


def rotated(rng, samples):
    """every sample's V times its own random orthogonal matrix (K, K): the embeddings rotate, inner products and norms do not"""
    out = []
    for w0, w, V in samples:
        K = np.asarray(V).shape[1]
        V = np.asarray(V, dtype=np.float64)
        out.append((w0, w, V @ np.linalg.qr(rng.normal(size=(K, K)))[0] if K else V))
    return out
