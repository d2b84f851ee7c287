"""Reference and inputs of the query x candidate scorer with relation-block sides and of its ordered-probit mode.

A side is a main matrix (R, Dm) plus a list with one entry per block position: (o2b, B) -- side row r additionally holds row
o2b[r] of the sparse B -- or None where the side holds nothing at that position. `expand` makes the flat side of it, so that
pairs_ref.pair_scores / pair_scores_abs / topk stay the direct reference; `decomposed_scores_rel` restates what the device
computes: one table per block (T, lin, vv per block row), gathered through o2b and summed onto the main part."""
import numpy as np
import scipy.sparse as sps
from scipy import special

from tests import pairs_ref as pr

HALVES = [1.0, -1.0, 2.0, -2.0, 0.5]


def expand(X_main, blocks, widths=None):
    """hstack([X_main, B_b[o2b_b] ...]) as CSR; a None entry gives widths[b] zero columns"""
    X_main = sps.csr_matrix(X_main, dtype=np.float64)
    parts = [X_main]
    for b, blk in enumerate(blocks):
        if blk is None:
            parts.append(sps.csr_matrix((X_main.shape[0], int(widths[b])), dtype=np.float64))
        else:
            o2b, B = blk
            parts.append(sps.csr_matrix(B, dtype=np.float64)[np.asarray(o2b, dtype=np.int64)])
    return sps.hstack(parts, format="csr")


def offsets_of(main_width, widths):
    """first column of every block position in the model's feature space"""
    return [int(main_width + sum(widths[:b])) for b in range(len(widths))]


def _side_tables(X_main, blocks, offs, w, V):
    """P (R, K), lin (R), vv (R) of one side: the main part, then every block's table gathered through its o2b, in list order"""
    A = sps.csr_matrix(X_main, dtype=np.float64)
    Dm = A.shape[1]
    P = A @ V[:Dm]
    lin = A @ w[:Dm]
    vv = (A.multiply(A) @ (V[:Dm] ** 2)).sum(axis=1)
    vv = np.asarray(vv).ravel()
    for blk, off in zip(blocks, offs):
        if blk is None:
            continue
        o2b, B = blk
        B = sps.csr_matrix(B, dtype=np.float64)
        Vb, wb = V[off:off + B.shape[1]], w[off:off + B.shape[1]]
        T = B @ Vb                                                    # one row per BLOCK row, whoever points at it
        tl = B @ wb
        tv = np.asarray((B.multiply(B) @ (Vb ** 2)).sum(axis=1)).ravel()
        o2b = np.asarray(o2b, dtype=np.int64)
        P, lin, vv = P + T[o2b], lin + tl[o2b], vv + tv[o2b]
    return P, lin, vv


def expected_class(score, cut):
    """sum_c c p_c with the class probabilities formed as the device predictor forms them: cdf_c = Phi(cut_c - score),
    p_c = cdf_c - cdf_{c-1}, p_last = 1 - cdf_last"""
    score = np.asarray(score, dtype=np.float64)
    prev = np.zeros_like(score)
    acc = np.zeros_like(score)
    for c, cp in enumerate(cut):
        cdf = (1.0 + special.erf((cp - score) * np.sqrt(0.5))) / 2.0
        acc = acc + c * (cdf - prev)
        prev = cdf
    return acc + len(cut) * (1.0 - prev)


def pair_scores_mode(samples, Xq, Xc, mode, cuts=None):
    """pairs_ref.pair_scores for modes 0 and 1; mode 2: the mean over the samples of the expected class index of the direct pair
    rows, cuts[s] the sample's cutpoints"""
    if mode != 2:
        return pr.pair_scores(samples, Xq, Xc, mode)
    X, U, I = pr._pair_rows(Xq, Xc)
    acc = np.zeros(U * I)
    for (w0, w, V), cut in zip(samples, cuts):
        acc = acc + expected_class(pr._sample_scores(X, w0, w, V), cut)
    return (acc / len(samples)).reshape(U, I)


def decomposed_scores_rel(samples, Xq_main, blocks_q, Xc_main, blocks_c, offs, mode, cuts=None):
    """the table decomposition: w0 + A[u] + B[i] + P[u] . Q[i] per sample with the sides' P, lin, vv from _side_tables;
    mode 2 adds sum_j Phi(score - cut_j) per sample, as the device does"""
    acc = None
    for s, (w0, w, V) in enumerate(samples):
        w, V = np.asarray(w, dtype=np.float64), np.asarray(V, dtype=np.float64)
        P, la, va = _side_tables(Xq_main, blocks_q, offs, w, V)
        Q, lb, vb = _side_tables(Xc_main, blocks_c, offs, w, V)
        a = la + 0.5 * ((P ** 2).sum(axis=1) - va)
        b = lb + 0.5 * ((Q ** 2).sum(axis=1) - vb)
        sc = w0 + a[:, None] + b[None, :] + P @ Q.T
        if mode == 1:
            v = (1.0 + special.erf(sc * np.sqrt(0.5))) / 2.0
        elif mode == 2:
            v = sum((1.0 + special.erf((sc - c) * np.sqrt(0.5))) / 2.0 for c in cuts[s])
        else:
            v = sc
        acc = v if acc is None else acc + v
    return acc / len(samples)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_block(rng, R, width, values=HALVES, one_row=False):
    """(o2b, B) for a side of R rows. one_row: a single block row that every side row maps to. Otherwise 7 multi-hot block rows
    with values from `values`, row 2 empty, row 5 never pointed at, and an o2b that is not monotone and repeats (it starts
    4, 0, 4 where the side has that many rows)."""
    M = 1 if one_row else 7
    rows, cols, vals = [], [], []
    for m in range(M):
        if not one_row and m == 2:
            continue
        n = min(width, 2 + int(rng.integers(0, 3)))
        c = rng.choice(width, size=n, replace=False)
        rows += [m] * n
        cols += list(c)
        vals += list(rng.choice(values, size=n))
    B = sps.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(M, width))
    if one_row:
        return np.zeros(R, dtype=np.int64), B
    o2b = rng.choice([0, 1, 2, 3, 4, 6], size=R).astype(np.int64)
    o2b[:3] = np.array([4, 0, 4])[:min(R, 3)]
    return o2b, B


def block_sides(rng, U, I, Dq, Dc, n_q, n_c, values=HALVES, mean_nnz=2.5, empty_every=7, width=6, with_none=True):
    """Main sides from pairs_ref.disjoint_sides (width D0 = Dq + Dc + 3) and n_q + n_c block positions behind them: the first n_q
    belong to the query side, the rest to the candidate side. The first block of a side is multi-hot, its second a one-row block.
    A side with blocks holds None at the other side's positions; a side without any is a list of None (with_none) or empty. Returns a dict:
    Xq, Xc (main), bq, bc (lists per position, or [] for a side without blocks), widths, offs, D."""
    Xq, Xc, D0 = pr.disjoint_sides(rng, U, I, Dq, Dc, values, mean_nnz=mean_nnz, empty_every=empty_every)
    n_pos = n_q + n_c
    widths = [width + b for b in range(n_pos)]
    bq, bc = [None] * n_pos, [None] * n_pos
    for b in range(n_pos):
        if b < n_q:
            bq[b] = make_block(rng, U, widths[b], values, one_row=(b == 1))
        else:
            bc[b] = make_block(rng, I, widths[b], values, one_row=(b - n_q == 1))
    if n_q == 0 and not with_none:
        bq = []
    if n_c == 0 and not with_none:
        bc = []
    return dict(Xq=Xq, Xc=Xc, bq=bq, bc=bc, widths=widths, offs=offsets_of(D0, widths), D=D0 + sum(widths), D0=D0)


def flat_sides(sd):
    """the two sides expanded into the full feature space"""
    n = len(sd["widths"])
    return (expand(sd["Xq"], sd["bq"] or [None] * n, sd["widths"]), expand(sd["Xc"], sd["bc"] or [None] * n, sd["widths"]))


def capi_args(sd):
    """arguments of _capi.Pairs: the main matrices widened to D columns, the blocks as (col_offset, o2b, csr)"""
    pad = sd["D"] - sd["D0"]
    Xq = sps.hstack([sd["Xq"], sps.csr_matrix((sd["Xq"].shape[0], pad))], format="csr")
    Xc = sps.hstack([sd["Xc"], sps.csr_matrix((sd["Xc"].shape[0], pad))], format="csr")
    rq = [(sd["offs"][b], blk[0], blk[1]) for b, blk in enumerate(sd["bq"]) if blk is not None]
    rc = [(sd["offs"][b], blk[0], blk[1]) for b, blk in enumerate(sd["bc"]) if blk is not None]
    return Xq, Xc, rq, rc


def sorted_cuts(rng, S, n_cut):
    """(S, n_cut) cutpoints, ascending per sample"""
    return np.sort(rng.normal(size=(S, n_cut)) * 1.5, axis=1)
