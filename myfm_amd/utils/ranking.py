"""Ranking metrics from the ranks of held-out pairs (predict_rank) and neighbour lists from predict_similar (DESIGN
4.13.4). Pure NumPy."""
import numpy as np
from scipy import sparse as sps


def ranking_metrics(result, targets, k=10):
    """Metrics of a TargetRanks `result` (or any (rank, value, n_candidates) triple) for the (U, I) sparse pattern `targets` it was
    computed for, over the queries with at least one target. With r the ranks of a row's targets (0 is best, other targets of the
    row count), T their number and r' = r minus the number of same-row targets that beat the target (its rank among the
    non-targets alone):

        hit_rate@k  mean[min r < k]
        recall@k    mean(#{r < k} / T)
        ndcg@k      mean(sum_{r < k} 1 / log2(r + 2)  /  sum_{j < min(T, k)} 1 / log2(j + 2))
        mrr         mean 1 / (min r + 1)
        mean_rank   mean of r' over all targets
        auc         mean(1 - sum r' / (T (n_candidates - T))) over the queries with n_candidates > T: the share of
                    (target, non-target) pairs of the query that are ordered correctly
        n_queries   the number of queries with a target

    Returns a dict with the keys "hit_rate@k", "recall@k", "ndcg@k" (k as given), "mrr", "mean_rank", "auc" and "n_queries";
    the means are NaN where no query enters them."""
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError("k must be a positive integer")
    k = int(k)
    rank, _, n_candidates = result
    rank = np.asarray(rank, dtype=np.int64)
    n_candidates = np.asarray(n_candidates, dtype=np.int64)
    T = sps.csr_matrix(targets)
    per_row = np.diff(T.indptr).astype(np.int64)
    if rank.shape != (T.nnz,) or n_candidates.shape != (T.shape[0],):
        raise ValueError("result does not belong to these targets: one rank per stored target and one n_candidates per query")
    row = np.repeat(np.arange(T.shape[0]), per_row)
    # within a row the targets that beat a target are those of smaller rank (ranks of one row are distinct: the order is total)
    order = np.lexsort((rank, row))
    within = np.empty(rank.size, dtype=np.int64)
    within[order] = np.arange(rank.size) - np.repeat(T.indptr[:-1].astype(np.int64), per_row)
    r_only = rank - within
    q = np.flatnonzero(per_row > 0)
    name = lambda m: "%s@%d" % (m, k)
    out = {name("hit_rate"): np.nan, name("recall"): np.nan, name("ndcg"): np.nan, "mrr": np.nan, "mean_rank": np.nan, "auc": np.nan,
           "n_queries": int(q.size)}
    if q.size == 0:
        return out
    starts = T.indptr[q].astype(np.int64)
    Tq = per_row[q].astype(np.float64)
    best = np.minimum.reduceat(rank, starts)
    hit = rank < k
    gain = np.where(hit, 1.0 / np.log2(rank + 2.0), 0.0)
    ideal = np.cumsum(1.0 / np.log2(np.arange(k) + 2.0))[np.minimum(per_row[q], k) - 1]
    out[name("hit_rate")] = float(np.mean(best < k))
    out[name("recall")] = float(np.mean(np.add.reduceat(hit.astype(np.float64), starts) / Tq))
    out[name("ndcg")] = float(np.mean(np.add.reduceat(gain, starts) / ideal))
    out["mrr"] = float(np.mean(1.0 / (best + 1.0)))
    sum_only = np.add.reduceat(r_only.astype(np.float64), starts)
    out["mean_rank"] = float(np.mean(r_only))
    others = n_candidates[q].astype(np.float64) - Tq
    ok = others > 0
    if ok.any():
        out["auc"] = float(np.mean(1.0 - sum_only[ok] / (Tq[ok] * others[ok])))
    return out


def neighbour_table(result, names=None, min_mean=None, max_std=None):
    """Per-query neighbour lists from a RankedSummary `result` of predict_similar (or any (indices, value, mean, std) quadruple of
    (U, k) arrays): a list of U lists of (name or index, mean, std) in the order of the ranking, the padding entries (index -1)
    left out. names: a sequence indexed by candidate index; without it the int index itself. min_mean / max_std: keep only the
    entries with mean >= min_mean and std <= max_std -- neighbours that are similar, and on which the kept samples agree."""
    indices, _, mean, std = result
    indices, mean, std = np.asarray(indices), np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    if indices.ndim != 2 or mean.shape != indices.shape or std.shape != indices.shape:
        raise ValueError("result must hold (U, k) arrays of indices, value, mean and std")
    if names is not None and indices.size and int(indices.max()) >= len(names):
        raise ValueError("names has %d entries but the result holds candidate index %d" % (len(names), int(indices.max())))
    keep = indices >= 0
    if min_mean is not None:
        keep &= mean >= float(min_mean)
    if max_std is not None:
        keep &= std <= float(max_std)
    table = []
    for u in range(indices.shape[0]):
        at = np.flatnonzero(keep[u])
        table.append([(int(indices[u, j]) if names is None else names[int(indices[u, j])], float(mean[u, j]), float(std[u, j])) for j in at])
    return table
