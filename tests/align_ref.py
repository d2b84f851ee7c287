"""Reference of aligned_factors: the same rounds in NumPy float64 (np.linalg.svd), a twin with the contraction in
longdouble and the SVD from mpmath (40 digits), the cases both test files use, and the tolerance.

The tolerance is a bound on |computed - exact| of ANY float64 evaluation of the rounds, worked out per case from the reference's
own quantities; u = 2^-53, gamma_n = n u / (1 - n u), all norms Frobenius, d_ref the bound on the round's reference (0 in round 0,
the previous round's d_mean after):
  M_s      e_M = gamma_{D+4} || |V_s| C |ref|^T || + ||V_s C|| d_ref      (a sum of D products in any order, plus the chunks' sums)
  R_s      d_R = 2 e_M / (sigma_K + sigma_{K-1}) + e_J                    (Li 1995, the polar factor of a perturbed matrix)
           e_J = 12 u K^{3/2} SWEEPS: a plane rotation perturbs a column by 6 u of its length, a column meets K - 1 rotations per
           sweep, K columns, U and W each; the product U W^T adds K u, which the constant covers. SWEEPS is the device's cap.
  Y_s      d_Y = (d_R + gamma_{K+2} sqrt(K)) ||V_s||
  mean     d_mean = mean_s d_Y + 4 S u max_s ||V_s||                      (Welford's divisions and sums)
  std      d_std = max_s d_Y + 4 S u max_s ||V_s||                        (the deviation norm is 1-Lipschitz in every y_s)
  align_s  (sqrt(K) e_M + e_J sum sigma) / den + align_s (2 gamma_{D+4} + d_ref / ||ref C^1/2|| + 8 u)   (Mirsky for sum sigma)
"""
import numpy as np

U_ROUND = 2.0 ** -53
SWEEPS = 30  # (ALIGN_SWEEPS of csrc/mfm_align.hpp)

# the real-valued cases: (K, S, D, n_refine, weighted). Every K of {3, 16, 33, 64}, S of {2, 37}, D of {200, 5000} (3 chunks),
# n_refine of {0, 2} and both weight settings occurs; S = 37 only below rank 33 and rank 64 in one round, because the twin's
# 40-digit SVD takes 0.2 s at rank 16 and 12 s at rank 64.
REAL_CASES = [(3, 37, 5000, 2, True), (16, 2, 5000, 2, False), (16, 37, 200, 0, True), (33, 2, 200, 0, True), (64, 2, 5000, 0, False)]


def gamma(n):
    return n * U_ROUND / (1.0 - n * U_ROUND)


def jacobi_term(K):
    return 12.0 * U_ROUND * K ** 1.5 * SWEEPS


def real_case(K, S, D, weighted, seed=0):
    """Vs (S, K, D) = Q_s^T V_0 + 0.1 noise with random orthogonal Q_s, every other one a reflection; weights (D,) or None with a
    third of the entries zero"""
    rng = np.random.default_rng([seed, K, S, D])
    V0 = rng.standard_normal((K, D))
    Vs = np.empty((S, K, D))
    for s in range(S):
        Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
        if (np.linalg.det(Q) < 0) != (s % 2 == 1):
            Q[:, 0] = -Q[:, 0]
        Vs[s] = Q.T @ V0 + 0.1 * rng.standard_normal((K, D))
    weights = None
    if weighted:
        weights = rng.uniform(0.5, 1.5, D)
        weights[::3] = 0.0
    return Vs, weights


def samples_of(Vs):
    """the (w0, w, V (D, K)) list the library's host entry points take"""
    return [(0.0, np.zeros(V.shape[1]), np.ascontiguousarray(V.T)) for V in Vs]


def _svd_mp(M):
    import mpmath as mp

    with mp.workdps(40):
        U, s, Vt = mp.svd_r(mp.matrix([[mp.mpf(float(x)) + mp.mpf(float(x - np.longdouble(float(x)))) for x in row] for row in M]))
        R = U * Vt
        K = M.shape[0]
        return (np.array([[np.longdouble(float(R[i, j])) + np.longdouble(float(R[i, j] - mp.mpf(float(R[i, j])))) for j in range(K)] for i in range(K)]),
                np.array([float(x) for x in s]))


def align_ref(Vs, reference=-1, n_refine=1, weights=None, twin=False):
    """-> dict(mean (D, K), std (D, K), rotations (S, K, K), alignment (S,), M (S, K, K) and sigma (S, K) of the last round,
    min_gap: the least (sigma_K + sigma_{K-1}) / sigma_1 over samples and rounds (K >= 2), tol: dict of the bounds above)"""
    ft = np.longdouble if twin else np.float64
    Vs = np.asarray(Vs, dtype=np.float64)
    S, K, D = Vs.shape
    c = np.ones(D) if weights is None else np.asarray(weights, dtype=np.float64)
    Vx = Vs.astype(ft)
    ref, d_ref, min_gap = Vx[reference], 0.0, np.inf
    vnorm = np.sqrt((Vs ** 2).sum(axis=(1, 2)))
    for _ in range(n_refine + 1):
        rc = ref * c.astype(ft)
        M = np.einsum("skd,jd->skj", Vx, rc)
        R, sig = np.empty((S, K, K), dtype=ft), np.empty((S, K))
        for s in range(S):
            if twin:
                R[s], sig[s] = _svd_mp(M[s])
            else:
                U, sig[s], Wt = np.linalg.svd(M[s])
                R[s] = U @ Wt
        Y = np.einsum("sab,sad->sbd", R, Vx)
        mean, std = Y.mean(axis=0), Y.std(axis=0)
        nv, nr = np.einsum("skd,d->s", Vx ** 2, c.astype(ft)), float((ref ** 2 * c).sum())
        den = np.sqrt(nv.astype(np.float64) * nr)
        align = np.where(den > 0, np.minimum(sig.sum(axis=1) / np.where(den > 0, den, 1.0), 1.0), 0.0)
        # ---- the bounds of this round
        absM = np.sqrt((np.einsum("skd,jd->skj", np.abs(Vs), np.abs(np.asarray(ref * c, dtype=np.float64))) ** 2).sum(axis=(1, 2)))
        e_M = gamma(D + 4) * absM + np.sqrt(((Vs * c) ** 2).sum(axis=(1, 2))) * d_ref
        gap = sig[:, -1] + sig[:, -2] if K >= 2 else 2.0 * sig[:, -1]
        min_gap = min(min_gap, float((gap / sig[:, 0]).min()))
        with np.errstate(divide="ignore", invalid="ignore"):  # (a singular case: no bound on R_s, the caller judges what is unique)
            d_R = 2.0 * e_M / gap + jacobi_term(K)
        d_Y = (d_R + gamma(K + 2) * np.sqrt(K)) * vnorm
        d_align = (np.sqrt(K) * e_M + jacobi_term(K) * sig.sum(axis=1)) / den + align * (2 * gamma(D + 4) + d_ref / np.sqrt(nr) + 8 * U_ROUND)
        tol = dict(rotations=d_R, mean=d_Y.mean() + 4 * S * U_ROUND * vnorm.max(), std=d_Y.max() + 4 * S * U_ROUND * vnorm.max(),
                   alignment=d_align, e_M=e_M, Y=d_Y)
        ref, d_ref = mean, tol["mean"]
    f = np.float64
    return dict(mean=np.ascontiguousarray(mean.T).astype(f), std=np.ascontiguousarray(std.T).astype(f), rotations=R.astype(f),
                alignment=align.astype(f), M=M.astype(f), sigma=sig, min_gap=min_gap, tol=tol)


def shares(got, ref):
    """the used share of the tolerance per output, got = (mean, std, rotations, alignment): Frobenius norms of the differences of
    mean and std, per sample of rotations and alignment, each over its bound"""
    tol = ref["tol"]
    return dict(mean=np.linalg.norm(got[0] - ref["mean"]) / tol["mean"], std=np.linalg.norm(got[1] - ref["std"]) / tol["std"],
                rotations=(np.sqrt(((got[2] - ref["rotations"]) ** 2).sum(axis=(1, 2))) / tol["rotations"]).max(),
                alignment=(np.abs(got[3] - ref["alignment"]) / tol["alignment"]).max())
