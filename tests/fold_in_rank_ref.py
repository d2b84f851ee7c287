"""Ranking under a new entity's own posterior (csrc/mfm_foldin_rank.hpp) restated on the host: the reference of
tests/test_gpu_fold_in_rank.py, proved in tests/test_fold_in_rank_cpu.py. Lambda and theta_mean come from tests/fold_in_ref.py; with
f_sc = score_s(X_cand[c]) and z_sc = (1, q_s(X_cand[c])),

    m = f + z^T theta_mean,   v = z^T Lambda^-1 z = |L^-1 z|^2  (Lambda = L L^T),
    mean = mean_s m,  std_within^2 = mean_s v,  std^2 = std_within^2 + mean_s (m - mean)^2,  gain = mean_s 1/2 log1p(alpha_s v).

`summary` does this in np.longdouble with an explicit forward solve, `summary_f64` in float64 with np.linalg (the twin).

Tolerances. Per (sample, entity, candidate) a unit bound e = (M + n_u) 2^-52 cond_2(Lambda_ref) (at least 2^-52: rank 0 without a
linear term estimates nothing), times |z|_1 max(|theta|_inf, |mu|_inf) + |f| for m and times v_ref for v. They carry over:
    mean: mean_s bm;   std_within: mean_s bv / std_within;   gain: mean_s e g_s  (d log1p(x) / log1p(x) <= dx / x);
    std:  mean_s bv / std + 4 max_s bm  (d std^2 <= mean_s bv + 2 mean_s |m - mean| |dm_s - mean dm| <= mean_s bv + 4 sd_between max bm,
          sd_between <= std, and |sqrt a - sqrt b| <= |a - b| / sqrt b).
TWIN_C is the largest error / bound of the float64 twin against the longdouble reference over the grid of the CPU test, as measured
there; the device gets 8 times that.
"""
import numpy as np
import scipy.sparse as sps

from tests import fold_in_ref as fr

LD = np.longdouble
TWIN_C = 1.16  # measured 1.1501 (rank 0 with the linear term, M = 1; 1.10 at rank 1 without it; below 0.16 from rank 3 on)
DEVICE_C = 8.0 * TWIN_C
FIELDS = ("mean", "std", "std_within", "gain")


def candidate_terms(sample, X_cand, fit_linear, dtype=LD):
    """(z (I, M), f (I,)) of the candidate contexts under one sample"""
    z, r = fr.z_and_residual(sample, sps.csr_matrix(X_cand), np.zeros(X_cand.shape[0]), dtype)
    return z[:, 0 if fit_linear else 1:], -r


def per_sample(p, X_cand, fit_linear, dtype=LD):
    """(m (S, U, I), v (S, U, I), ref): the pair's mean and within-sample variance under every sample, and fold_in_ref's posterior"""
    S, U, I = p["S"], p["U"], X_cand.shape[0]
    if dtype is LD:
        ref = fr.posterior(p, fit_linear)
        theta, L = ref["theta"], ref["L"]
    else:
        ref = None
        Lam = fr.systems(p, fit_linear, np.float64)[0]
        theta = fr.posterior_f64(p, fit_linear)
        L = np.linalg.cholesky(Lam) if Lam.shape[-1] else Lam
    m, v = np.zeros((S, U, I), dtype=dtype), np.zeros((S, U, I), dtype=dtype)
    for s in range(S):
        z, f = candidate_terms(p["samples"][s], X_cand, fit_linear, dtype)
        m[s] = f[None, :] + np.dot(theta[s], z.T)
        for u in range(U if z.shape[1] else 0):
            t = fr.solve_lower(L[s, u], z) if dtype is LD else np.linalg.solve(L[s, u], z.T).T
            v[s, u] = (t * t).sum(axis=-1)
    return m, v, ref


def summarise(m, v, alpha):
    """the four (U, I) outputs from the per-sample terms"""
    mean, within2 = m.mean(axis=0), v.mean(axis=0)
    gain = (np.log1p(np.asarray(alpha).astype(m.dtype)[:, None, None] * v) / 2).mean(axis=0)
    return dict(mean=mean, std=np.sqrt(within2 + ((m - mean) ** 2).mean(axis=0)), std_within=np.sqrt(within2), gain=gain)


def summary(p, X_cand, fit_linear=True):
    """the longdouble reference: (dict of the four outputs, dict of their unit bounds (U, I) in float64, cond (S, U))"""
    m, v, ref = per_sample(p, X_cand, fit_linear)
    out = summarise(m, v, p["alpha"])
    M = ref["theta"].shape[-1]
    e = np.maximum(M + ref["counts"][None, :], 1) * 2.0 ** -52 * ref["cond"]  # (S, U)
    big = np.maximum(np.abs(ref["theta"]).max(axis=-1, initial=0), np.abs(ref["mu"]).max(axis=-1, initial=0)[:, None]).astype(np.float64)
    bm, bv = np.zeros(m.shape), e[:, :, None] * v.astype(np.float64)
    for s in range(p["S"]):
        z, f = candidate_terms(p["samples"][s], X_cand, fit_linear)
        bm[s] = e[s][:, None] * (big[s][:, None] * np.abs(z).sum(axis=1).astype(np.float64)[None, :] + np.abs(f).astype(np.float64)[None, :])
    sd, sw = out["std"].astype(np.float64), out["std_within"].astype(np.float64)
    g_s = np.log1p(np.asarray(p["alpha"])[:, None, None] * v.astype(np.float64)) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = dict(mean=bm.mean(axis=0), gain=(e[:, :, None] * g_s).mean(axis=0),
                     std_within=np.where(sw > 0, bv.mean(axis=0) / sw, 0.0),
                     std=np.where(sd > 0, bv.mean(axis=0) / sd, 0.0) + 4 * bm.max(axis=0))
    return out, bound, ref["cond"]


def summary_f64(p, X_cand, fit_linear=True):
    m, v, _ = per_sample(p, X_cand, fit_linear, np.float64)
    return summarise(m, v, p["alpha"])


def worst(got, want, bound):
    """largest |got - want| / bound over the four outputs (a zero bound with a zero error counts as 0)"""
    w = 0.0
    for name in FIELDS:
        err = np.abs(np.asarray(got[name]).astype(LD) - want[name]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = max(w, float(np.where(err == 0, 0.0, err / bound[name]).max(initial=0.0)))
    return w


def ranked(out, by, beta, k, exclude=None):
    """(indices (U, k), value (U, k + 1 candidates' worth)) of the reference: value descending, index ascending; -1 / -inf tail"""
    value = (out["gain"] if by == "gain" else out["mean"] + LD(beta) * out["std"]).copy()
    if exclude is not None:
        value[sps.csr_matrix(exclude).toarray() != 0] = -np.inf
    U, I = value.shape
    idx = np.full((U, k + 1), -1, dtype=np.int64)
    val = np.full((U, k + 1), -np.inf, dtype=LD)
    for u in range(U):
        order = np.lexsort((np.arange(I), -value[u]))
        order = order[np.isfinite(value[u][order])][:k + 1]
        idx[u, :order.size], val[u, :order.size] = order, value[u][order]
    return idx, val
