"""NumPy restatement of the per-row Philox latent draws (csrc/mfm_tasks.hpp: philox4x32_10, RowRng, tn_left / tn_right /
tn_twoside, k_tn_classification, k_oprobit_sample_z), vectorised over rows, for holding the device draws against draw for draw.

Every sampler returns (draws, margin): margin[i] is the smallest distance between the two sides of any accept / reject comparison
on row i's path (|r c - mu|, |u - rho|, ...). Device libm (log, exp, sincospi) and glibc differ by a few ulp; such a difference can
flip a decision only where the margin is about 1e-13 or less, so a caller excludes the rows with a small margin (and counts them).

The rejection loops run over the rows still open: every open row is at the same attempt, so the attempt index is the counter word
n of RowRng::next2 for all of them. After TN_MAX_TRIES attempts a row takes the device's fall-back value.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
TN_MAX_TRIES = 1 << 14
_PI_L = np.longdouble("3.14159265358979323846264338327950288")


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64 (products of two words fit; everything else is masked)"""
    c0, c1, c2, c3, k0, k1 = (_u64(v) for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = PHILOX_M0 * c0
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def to_uniform(hi, lo):
    """((hi << 21) | (lo >> 11)) + 0.5) / 2^53, in double as the device computes it"""
    v = ((_u64(hi) << np.uint64(21)) | (_u64(lo) >> np.uint64(11))).astype(np.float64)
    return (v + 0.5) * (1.0 / 9007199254740992.0)


class RowRng:
    """the streams of global rows `grow` (int64 array) for (seed, draw): RowRng(seed ^ (grow >> 32) * GOLDEN, draw, (uint32)grow)"""

    def __init__(self, seed, draw, grow):
        grow = np.asarray(grow, dtype=np.int64)
        s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ ((grow >> 32).astype(np.uint64) * GOLDEN)  # (mod 2^64)
        self.k0, self.k1 = s & M32, s >> np.uint64(32)
        self.row = grow.astype(np.uint64) & M32
        d = int(draw) & 0xFFFFFFFFFFFFFFFF
        self.d0, self.d1 = np.uint64(d & 0xFFFFFFFF), np.uint64(d >> 32)

    def subset(self, idx):
        """the streams of the rows idx of this one"""
        sub = RowRng.__new__(RowRng)
        sub.k0, sub.k1, sub.row, sub.d0, sub.d1 = self.k0[idx], self.k1[idx], self.row[idx], self.d0, self.d1
        return sub

    def next2(self, n, idx=None):
        """the two uniforms of counter word n for the rows idx (all rows: None)"""
        row, k0, k1 = (self.row, self.k0, self.k1) if idx is None else (self.row[idx], self.k0[idx], self.k1[idx])
        r0, r1, r2, r3 = philox4x32_10(row, np.uint64(n), self.d0, self.d1, k0, k1)
        return to_uniform(r0, r1), to_uniform(r2, r3)


def sincospi2(u):
    """(sin, cos)(2 pi u): exact quadrant reduction, the remainder in extended precision, rounded once to double"""
    x = 2.0 * np.asarray(u, dtype=np.float64)
    q = np.rint(2.0 * x)
    r = (x - 0.5 * q).astype(np.longdouble)  # (exact: |r| <= 1/4)
    s0, c0 = np.sin(_PI_L * r), np.cos(_PI_L * r)
    q = q.astype(np.int64) & 3
    s = np.select([q == 0, q == 1, q == 2], [s0, c0, -s0], -c0)
    c = np.select([q == 0, q == 1, q == 2], [c0, -s0, -c0], s0)
    return s.astype(np.float64), c.astype(np.float64)


def tn_left(g, mu, max_tries=TN_MAX_TRIES):
    """z ~ N(0, 1) | z > mu, per row of g (mu: scalar or one value per row)"""
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), g.row.shape).copy()
    n = mu.shape[0]
    out = np.empty(n)
    margin = np.full(n, np.inf)
    neg = mu < 0
    out[~neg] = mu[~neg]  # fall-back values (util.hpp:15-37 never returns them)
    out[neg] = 0.0
    # mu < 0: rejection from N(0, 1), Box-Muller pair r cos first, then r sin
    open_ = np.flatnonzero(neg)
    for it in range(max_tries):
        if open_.size == 0:
            break
        ux, uy = g.next2(it, open_)
        r = np.sqrt(-2.0 * np.log(ux))
        s, c = sincospi2(uy)
        m = mu[open_]
        rc, rs = r * c, r * s
        margin[open_] = np.minimum(margin[open_], np.abs(rc - m))
        take_c = rc > m
        out[open_[take_c]] = rc[take_c]
        rest = ~take_c
        margin[open_[rest]] = np.minimum(margin[open_[rest]], np.abs(rs[rest] - m[rest]))
        take_s = rest & (rs > m)
        out[open_[take_s]] = rs[take_s]
        open_ = open_[~(take_c | take_s)]
    # mu >= 0: exponential proposal (Robert 2009, Prop. 2.3)
    open_ = np.flatnonzero(~neg)
    alpha = (mu + np.sqrt(mu * mu + 4)) / 2
    for it in range(max_tries):
        if open_.size == 0:
            break
        ux, uy = g.next2(it, open_)
        a, m = alpha[open_], mu[open_]
        z = -np.log(ux) / a + m
        rho = np.exp(-(z - a) * (z - a) / 2)
        margin[open_] = np.minimum(margin[open_], np.abs(uy - rho))
        acc = uy < rho
        out[open_[acc]] = z[acc]
        open_ = open_[~acc]
    return out, margin


def tn_right(g, mu, max_tries=TN_MAX_TRIES):
    """z ~ N(0, 1) | z < mu  (= -tn_left(-mu))"""
    z, margin = tn_left(g, -np.asarray(mu, dtype=np.float64), max_tries)
    return -z, margin


def tn_twoside(g, lo, hi, max_tries=TN_MAX_TRIES):
    """z ~ N(0, 1) | lo < z < hi, per row of g"""
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), g.row.shape)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), g.row.shape)
    out = 0.5 * (lo + hi)  # fall-back value
    margin = np.full(lo.shape[0], np.inf)
    open_ = np.arange(lo.shape[0])
    for it in range(max_tries):
        if open_.size == 0:
            break
        ux, uy = g.next2(it, open_)
        a, b = lo[open_], hi[open_]
        z = a + (b - a) * ux
        rho = np.exp(np.where((a <= 0) & (b >= 0), -z * z / 2, np.where(b < 0, (b * b - z * z) / 2, (a * a - z * z) / 2)))
        margin[open_] = np.minimum(margin[open_], np.abs(uy - rho))
        acc = uy < rho
        out[open_[acc]] = z[acc]
        open_ = open_[~acc]
    return out, margin


def tn_hook(kind, lo, hi, n, seed, draw):
    """mfm_test_truncated_normal: draw i on the stream of row i"""
    g = RowRng(seed, draw, np.arange(n, dtype=np.int64))
    if kind == "left":
        return tn_left(g, lo)
    if kind == "right":
        return tn_right(g, hi)
    return tn_twoside(g, lo, hi)


def classification_e(scores, y, seed, draw, row_offset):
    """k_tn_classification: e = score - (score + z), z ~ N(0, 1) truncated to z > -score (y > 0) or z < -score"""
    scores = np.asarray(scores, dtype=np.float64)
    t = np.arange(scores.shape[0], dtype=np.int64)
    g = RowRng(seed, draw, t + int(row_offset))
    pos = np.flatnonzero(np.asarray(y) > 0)
    neg = np.flatnonzero(~(np.asarray(y) > 0))
    z, margin = np.empty(scores.shape[0]), np.empty(scores.shape[0])
    z[pos], margin[pos] = tn_left(g.subset(pos), 0.0 - scores[pos])
    z[neg], margin[neg] = tn_right(g.subset(neg), 0.0 - scores[neg])
    n = scores + z
    return scores - n, margin


def oprobit_sample_z(e, y, rows, n_class, gamma, seed, draw, row_offset):
    """k_oprobit_sample_z on the residual array e (scores on entry): returns (e after the call, margin per entry of rows).
    The stream of table row rows[p] is keyed by that row, not by p."""
    e = np.array(e, dtype=np.float64)
    rows = np.arange(e.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    gamma = np.asarray(gamma, dtype=np.float64)
    cls = np.asarray(y)[rows].astype(np.int64)
    pred = e[rows]
    g = RowRng(seed, draw, rows + int(row_offset))
    z = np.empty(rows.shape[0])
    margin = np.empty(rows.shape[0])
    first, last = cls == 0, cls == n_class - 1
    mid = ~first & ~last
    for sel, fn in ((first, lambda gg, p, c: tn_right(gg, gamma[0] - p)),
                    (last, lambda gg, p, c: tn_left(gg, gamma[n_class - 2] - p)),
                    (mid, lambda gg, p, c: tn_twoside(gg, gamma[c - 1] - p, gamma[c] - p))):
        idx = np.flatnonzero(sel)
        if idx.size == 0:
            continue
        zz, mm = fn(g.subset(idx), pred[idx], cls[idx])
        z[idx] = zz + pred[idx]
        margin[idx] = mm
    e[rows] = pred - z
    return e, margin
