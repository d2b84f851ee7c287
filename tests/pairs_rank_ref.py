"""Brute-force references of the rank form of the pair scorer: the rank of a target pair as a count over a dense
(U, I) score array under the total order (value descending, candidate index ascending), and the ranking metrics computed
directly from such an array, pair by pair, without going through ranks."""
import numpy as np
import scipy.sparse as sps


def _rows(M, shape):
    """per row the sorted, unique stored columns of a sparse pattern (None: no columns)"""
    if M is None:
        return [np.empty(0, dtype=np.int64) for _ in range(shape[0])]
    M = sps.csr_matrix(M)
    assert M.shape == shape
    return [np.unique(M.indices[M.indptr[u]:M.indptr[u + 1]]).astype(np.int64) for u in range(shape[0])]


def beats(va, ia, vb, ib):
    return va > vb or (va == vb and ia < ib)


def rank_ref(scores, targets, exclude=None):
    """(rank int64 (nnz,), value (nnz,), n_candidates int64 (U,)): for every stored target (u, i), rows in order and columns
    ascending, the number of candidates j != i of row u that are not excluded and beat it; scores[u, i]; I - |exclude row u|"""
    scores = np.asarray(scores, dtype=np.float64)
    U, I = scores.shape
    T, E = _rows(targets, (U, I)), _rows(exclude, (U, I))
    rank, value = [], []
    for u in range(U):
        allowed = np.ones(I, dtype=bool)
        allowed[E[u]] = False
        for i in T[u]:
            assert allowed[i], "a target is excluded"
            rank.append(sum(1 for j in range(I) if j != i and allowed[j] and beats(scores[u, j], j, scores[u, i], i)))
            value.append(scores[u, i])
    n_cand = np.asarray([I - E[u].size for u in range(U)], dtype=np.int64)
    return np.asarray(rank, dtype=np.int64), np.asarray(value, dtype=np.float64), n_cand


def rank_ref_fast(scores, targets, exclude=None):
    """rank_ref with the inner count vectorised (the GPU tests' larger shapes); same definition, same outputs"""
    scores = np.asarray(scores, dtype=np.float64)
    U, I = scores.shape
    T, E = _rows(targets, (U, I)), _rows(exclude, (U, I))
    cols = np.arange(I)
    rank, value = [], []
    for u in range(U):
        allowed = np.ones(I, dtype=bool)
        allowed[E[u]] = False
        s = scores[u]
        for i in T[u]:
            assert allowed[i], "a target is excluded"
            win = (s > s[i]) | ((s == s[i]) & (cols < i))
            rank.append(int(np.count_nonzero(win & allowed)))
            value.append(s[i])
    n_cand = np.asarray([I - E[u].size for u in range(U)], dtype=np.int64)
    return np.asarray(rank, dtype=np.int64), np.asarray(value, dtype=np.float64), n_cand


def metrics_ref(scores, targets, exclude=None, k=10):
    """the metrics of myfm_amd.utils.ranking.ranking_metrics from the dense scores: every query's admissible candidates are sorted
    into the total order and the list is walked"""
    scores = np.asarray(scores, dtype=np.float64)
    U, I = scores.shape
    T, E = _rows(targets, (U, I)), _rows(exclude, (U, I))
    hit, recall, ndcg, mrr, only, auc = [], [], [], [], [], []
    for u in range(U):
        if T[u].size == 0:
            continue
        allowed = np.ones(I, dtype=bool)
        allowed[E[u]] = False
        cand = np.flatnonzero(allowed)
        order = list(cand[np.lexsort((cand, -scores[u, cand]))])  # best first
        is_t = [j in set(T[u].tolist()) for j in order]
        pos = [p for p, t in enumerate(is_t) if t]
        n_t = len(pos)
        hit.append(1.0 if pos[0] < k else 0.0)
        recall.append(sum(1 for p in pos if p < k) / n_t)
        ndcg.append(sum(1.0 / np.log2(p + 2.0) for p in pos if p < k) / sum(1.0 / np.log2(j + 2.0) for j in range(min(n_t, k))))
        mrr.append(1.0 / (pos[0] + 1.0))
        # a target's rank among the non-targets alone = the non-targets ahead of it
        ahead = [sum(1 for t in is_t[:p] if not t) for p in pos]
        only += ahead
        n_other = len(order) - n_t
        if n_other > 0:
            # the share of (target, non-target) pairs in the right order
            auc.append(sum(n_other - a for a in ahead) / (n_t * n_other))
    mean = lambda x: float(np.mean(x)) if len(x) else float("nan")
    return {"hit_rate@%d" % k: mean(hit), "recall@%d" % k: mean(recall), "ndcg@%d" % k: mean(ndcg), "mrr": mean(mrr),
            "mean_rank": mean(only), "auc": mean(auc), "n_queries": len(hit)}


def draw_targets(rng, U, I, counts, ties_from=None):
    """a (U, I) target pattern: row u gets counts[u % len(counts)] targets (at most I), column 0 in the first row that has any,
    column I - 1 in the last; where `ties_from` (a dense score array) is given, a row with two or more targets gets, if its scores
    allow, two targets of equal value"""
    rows, cols = [], []
    with_t = [u for u in range(U) if min(counts[u % len(counts)], I) > 0]
    for u in with_t:
        n = min(counts[u % len(counts)], I)
        must = []
        if u == with_t[0]:
            must.append(0)
        if u == with_t[-1] and I - 1 not in must:
            must.append(I - 1)
        must = must[:n]
        if ties_from is not None and n - len(must) >= 2:
            vals, inv, cnt = np.unique(ties_from[u], return_inverse=True, return_counts=True)
            for g in np.flatnonzero(cnt >= 2):
                pair = [int(c) for c in np.flatnonzero(inv == g) if c not in must][:2]
                if len(pair) == 2:
                    must += pair
                    break
        rest = np.setdiff1d(np.arange(I), must)
        pick = list(must) + list(rng.choice(rest, size=n - len(must), replace=False))
        rows += [u] * n
        cols += pick
    T = sps.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(U, I))
    T.sort_indices()
    return T


def exclude_without(rng, U, I, density, targets):
    """a random (U, I) exclusion pattern of about `density`, never on a target"""
    E = sps.random(U, I, density=density, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
    E.data[:] = 1.0
    Tp = sps.csr_matrix(targets)
    Tp = sps.csr_matrix((np.ones(Tp.nnz), Tp.indices, Tp.indptr), shape=Tp.shape)
    E = sps.csr_matrix(E - E.multiply(Tp))
    E.eliminate_zeros()
    E.sort_indices()
    return E
