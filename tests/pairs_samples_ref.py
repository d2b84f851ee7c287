"""Reference of the per-sample rankings of the query x candidate scorer: every kept sample's own top k from
pairs_ucb_ref's per-sample values, the vote that turns the S lists into top-k inclusion probabilities, and the draw of the
Thompson list's samples."""
import numpy as np

from tests import pairs_ref as pr


def sample_lists(vals, k, exclude=None):
    """(indices int64 (S, U, k), values float64 (S, U, k)): pairs_ref.topk of every sample's values vals[s] (U, I) -- e.g.
    pairs_ucb_ref.sample_values(...) -- under (value descending, index ascending); tails -1 / -inf"""
    vals = np.asarray(vals, dtype=np.float64)
    S, U = vals.shape[:2]
    idx, val = np.empty((S, U, k), dtype=np.int64), np.empty((S, U, k))
    for s in range(S):
        idx[s], val[s] = pr.topk(vals[s], k, exclude)
    return idx, val


def vote(idx, n_top):
    """(indices int64 (U, n_top), probability float64 (U, n_top)) from the S lists idx (S, U, k): integer counts of the entries
    that are not tails (-1), the n_top candidates of largest count under (count descending, index ascending), probability =
    count / S; missing entries -1 / 0.0"""
    idx = np.asarray(idx)
    S, U = idx.shape[:2]
    out_i = np.full((U, n_top), -1, dtype=np.int64)
    out_p = np.zeros((U, n_top))
    for u in range(U):
        flat = idx[:, u, :].ravel()
        cand, count = np.unique(flat[flat >= 0], return_counts=True)
        order = np.lexsort((cand, -count))[:n_top]
        out_i[u, :order.size] = cand[order]
        out_p[u, :order.size] = count[order].astype(np.float64) / np.float64(S)
    return out_i, out_p


def thompson_samples(seed, S, U):
    """the kept sample of every query row, as predict_topk_thompson draws it"""
    return np.random.default_rng(seed).integers(0, S, size=U)
