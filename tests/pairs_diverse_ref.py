"""Reference of the diversified top-k: greedy maximal marginal relevance over a pool, in np.longdouble. The similarity is
tests/pairs_sim_ref.py's (the mean over the samples of the per-sample cosine, candidates x candidates); this file adds the relevance,
the greedy definition, and the REPLAY of a given list: arg-max is discontinuous, so a device list is not compared with the reference's
list but walked step by step, each pick judged given the picks before it.

Tolerance of step t at pool position j (first order):
    tol_sim(j) = max over the chosen c of pairs_sim_ref.bounds' mean bound of the pair (j, c)   (a max moves by at most the largest move),
    tol_rel(j) = 2 b_v / (v_0 - v_min) (1 + rel_j): rel = (v - v_min) / (v_0 - v_min) with every value within b_v of the true one moves by
                 at most (2 b_v + rel 2 b_v) / (v_0 - v_min),
    tol(j)     = lam tol_rel(j) + (1 - lam) tol_sim(j) + ROUND,   ROUND = 8 * 2^-53: the subtraction, the division, the two products and
                 the difference of g, each within half an ulp of a quantity of magnitude <= 1.
A pick p passes when g(p) >= g(j) - tol(j) - tol(p) for every unchosen live j: where the runner-up is further away the pick is forced."""
import numpy as np

from tests import pairs_ref as pr
from tests import pairs_sim_ref as sr

LD = np.longdouble
ROUND = 8.0 * 2.0 ** -53


def default_pool(k):
    return min(128, max(4 * k, 32))


def similarity(samples, Xc):
    """(sim longdouble (I, I), its bound (I, I)); the conditioning of the inputs is asserted here, on the reference alone"""
    assert sr.brackets(samples, Xc, Xc, "cosine").max() < 100.0
    vals = sr.sample_values(samples, Xc, Xc, "cosine")
    return vals.mean(axis=0) if len(samples) else np.zeros(vals.shape[1:], LD), sr.bounds(samples, Xc, Xc, "cosine", vals)[0]


def relevance(v):
    """v: the live pool values, descending"""
    v = np.asarray(v, dtype=np.float64).astype(LD)
    span = v[0] - v[-1]
    return np.ones(v.size, dtype=LD) if span == 0 else (v - v[-1]) / span


def _steps(pool_idx, pool_val, sim, lam, k, picks=None):
    """one query row, step by step: yields (t, n_live, positions c of the pool, j chosen or None, g of every live position with the
    chosen ones at -inf (step 0: position 0 alone is open), the running max-sim). picks None: the definition's own arg-max."""
    n = int((pool_idx >= 0).sum())
    c, rel, lam = pool_idx[:n], relevance(pool_val[:n]) if n else None, LD(lam)
    ms, taken = np.full(n, -np.inf, dtype=LD), np.zeros(n, dtype=bool)
    at = {int(i): j for j, i in enumerate(c)}
    for t in range(k):
        if t >= n:
            yield t, n, c, None, None, None
            continue
        g = lam * rel if t == 0 else lam * rel - (1 - lam) * ms
        g = np.where(taken | ((np.arange(n) > 0) & (t == 0)), -np.inf, g)
        j = int(np.argmax(g)) if picks is None else at.get(int(picks[t]), -1)  # (argmax: the first of equal maxima, the lower position)
        yield t, n, c, j, g, ms.copy()
        if j < 0 or taken[j]:
            return
        taken[j] = True
        ms = np.maximum(ms, sim[c[j], c])


def greedy(pool_idx, pool_val, sim, lam, k):
    """the definition for one query row: (indices (k,), value, objective, redundancy)"""
    idx, val, obj, red = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf), np.full(k, np.nan), np.full(k, np.nan)
    for t, n, c, j, g, ms in _steps(pool_idx, pool_val, sim, lam, k):
        if j is not None:
            idx[t], val[t], obj[t], red[t] = c[j], pool_val[j], g[j], 0.0 if t == 0 else ms[j]
    return idx, val, obj, red


def check_replay(result, pool, sim, b_sim, b_v, lam):
    """The four checks of every (query, step) of a device `result` (indices, value, objective, redundancy) against `pool`, the (indices,
    values) of a separate top-k call of the pool's length. b_sim: the similarity's bound (I, I) or 0; b_v: the value's bound (U, I) or 0.
    Returns the largest used share of tol over all steps (0 where tol is 0 and the figures agree)."""
    idx, val, obj, red = result
    pidx, pval = pool
    used = 0.0
    for u in range(idx.shape[0]):
        for t, n, c, j, g, ms in _steps(pidx[u], pval[u], sim, lam, idx.shape[1], picks=idx[u]):
            if j is None:
                assert idx[u, t] == -1 and val[u, t] == -np.inf and np.isnan(obj[u, t]) and np.isnan(red[u, t]), (u, t)
                continue
            assert j >= 0 and np.isfinite(g[j]), (u, t, "the pick is no unchosen live pool position")
            assert val[u, t] == pval[u, j], (u, t)
            rel = relevance(pval[u, :n])
            bv = float(np.max(np.asarray(b_v)[u, c])) if np.ndim(b_v) else float(b_v)
            span = float(pval[u, 0] - pval[u, n - 1])
            tol_rel = 2.0 * bv / span * (1.0 + rel.astype(np.float64)) if span > 0 else np.zeros(n)
            taken = np.flatnonzero(~np.isfinite(g)) if t else np.zeros(0, dtype=np.int64)
            tol_sim = np.asarray(b_sim)[np.ix_(c, c[taken])].max(axis=1) if np.ndim(b_sim) and taken.size else np.zeros(n)
            tol = lam * tol_rel + (1.0 - lam) * tol_sim + ROUND
            d_obj, d_red = abs(float(obj[u, t] - g[j])), abs(float(red[u, t] - (0.0 if t == 0 else ms[j])))
            assert d_obj <= tol[j] and d_red <= tol_sim[j], (u, t, d_obj, tol[j], d_red, tol_sim[j])
            assert g[j] >= np.max(g - tol) - tol[j], (u, t, "not the arg-max within the tolerance")
            used = max(used, d_obj / tol[j], d_red / tol_sim[j] if tol_sim[j] > 0 else 0.0)
    return used


# ---- inputs shared by the CPU and the GPU tests -------------------------------------------------------------------------------------
def real_case(K, S, U=5, I=300):
    """normal samples and multi-hot sides of tests/pairs_ref.py: (samples, Xq, Xc, exclude)"""
    import scipy.sparse as sps

    rng = np.random.default_rng(500 + K + S)
    Xq, Xc, D = pr.disjoint_sides(rng, U, I, 40, 60, [1.0, -1.0, 2.0, -2.0, 0.5], mean_nnz=3.0)
    ex = sps.random(U, I, density=0.05, random_state=np.random.RandomState(3), format="csr")
    return pr.normal_samples(rng, D, K, S, scale=0.3), Xq, Xc, ex


def value_bound(samples, Xq, Xc):
    """b_v (U, I) of mode 0: test_gpu_pairs.mode_bound's"""
    return 1e-10 * pr.pair_scores_abs(samples, Xq, Xc)


def assert_spread(samples, Xq, Xc, ex, pool):
    """the reference pool's v_0 - v_min stays above 1e3 b_v in every row (or tol_rel would hide a wrong relevance)"""
    ridx, rval = pr.topk(pr.pair_scores(samples, Xq, Xc, 0), pool, ex)
    b_v = value_bound(samples, Xq, Xc)
    for u in range(ridx.shape[0]):
        live = ridx[u] >= 0
        assert rval[u, live][0] - rval[u, live][-1] > 1e3 * b_v[u, ridx[u, live]].max(), u
