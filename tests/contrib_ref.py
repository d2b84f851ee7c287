"""The score taken apart by field in np.longdouble, a float64 twin that adds in the orders of k_contrib (csrc/mfm_contrib.hpp),
and the error bounds the device and mfm_contrib_row are held to: the reference of tests/test_contributions_cpu.py and
tests/test_gpu_contributions.py. Built on score_ref.flat_rows.

Components of a row under one sample, field_of[j] in [0, F): the F linear terms lin_g, then the P = F (F + 1) / 2 interactions
I_gh at the packed index g F - g (g - 1) / 2 + (h - g), g <= h; C = F + P.

The bound of one (row, sample, component): gamma_n M_c, M_c the sum of the magnitudes of the component's terms and n the kernel's
operation count on the longest path into one result. With L the row's stored entries: an embedding p_g[k] is a sum of at most L
products (L + 1 roundings), a pair's product of two such adds one, the diagonal subtracts q_g (another sum of at most L terms of
three products each: L + 3, and the difference: 1), the butterfly adds at most 6 levels, the factor chunks beyond the first one
addition each. n = 2 L + 8 + 6 + chunks covers every component (the linear terms need L + 1). Derived, not measured.
The mean over S samples inherits the mean of the bounds plus gamma_S mean|c_s|; the standard deviation is 1-Lipschitz in the values:
the largest of the bounds. Both take, for the rounding of the moment recurrence itself, 8 x the largest deviation of the float64
twin from the longdouble reference over the inputs at hand, relative to the component's magnitude scale max_s M_c (measured where
it is used and printed there: no number is fixed beforehand)."""
import numpy as np

from tests.score_ref import LD, U, flat_rows


def pairs(F):
    return [(g, h) for g in range(F) for h in range(g, F)]


def contrib_shape(K, F):
    """(FB fields of the bucket, GS lanes per row) of k_contrib: contrib_bucket / contrib_group of csrc/mfm_contrib.hpp"""
    FB = 2 if F <= 2 else 4 if F <= 4 else 8 if F <= 8 else 16
    GS = 4 if K <= 4 else 16 if K <= 16 else 32 if K <= 32 else 64
    return FB, max(GS, 16) if FB == 16 else GS


def gamma(n):
    n = np.asarray(n, dtype=LD)
    return n * LD(U) / (1 - n * LD(U))


def components(rows, w, V, field_of, F):
    """(c[C, N], M[C, N]) in longdouble: every component of every row under the sample (w[D], V[D, K]), and the sum of the
    magnitudes of its terms"""
    idx, x, cnt = rows
    N, L = x.shape
    live = np.arange(L)[None, :] < cnt[:, None]
    f = np.asarray(field_of)[idx]
    xl, wl, Vl = x.astype(LD), np.asarray(w)[idx].astype(LD), np.asarray(V)[idx].astype(LD)  # (N, L), (N, L), (N, L, K)
    P = F * (F + 1) // 2
    c, M = np.zeros((F + P, N), dtype=LD), np.zeros((F + P, N), dtype=LD)
    p, a, q = [], [], []
    for g in range(F):
        m = (live & (f == g)).astype(LD)
        xg = xl * m
        c[g] = (xg * wl).sum(axis=1)
        M[g] = np.abs(xg * wl).sum(axis=1)
        xv = xg[:, :, None] * Vl
        p.append(xv.sum(axis=1))
        a.append(np.abs(xv).sum(axis=1))
        q.append((xv * xv).sum(axis=(1, 2)))
    for i, (g, h) in enumerate(pairs(F)):
        if g == h:
            c[F + i] = ((p[g] * p[g]).sum(axis=1) - q[g]) / 2
            M[F + i] = ((a[g] * a[g]).sum(axis=1) + q[g]) / 2
        else:
            c[F + i] = (p[g] * p[h]).sum(axis=1)
            M[F + i] = (a[g] * a[h]).sum(axis=1)
    return c, M


def components_f64(rows, w, V, field_of, F):
    """c[C, N] in float64 in k_contrib's orders: lane l of GS owns factor l of each chunk of GS factors and adds the row's entries
    in stored order into the field's p and q; a pair's parts meet in the xor butterfly; the chunks' sums are added in order"""
    idx, x, cnt = rows
    N, L = x.shape
    w, V = np.asarray(w, dtype=np.float64), np.asarray(V, dtype=np.float64)
    K = V.shape[1]
    _, GS = contrib_shape(K, F)
    n_chunk = max(1, -(-K // GS))
    Vp = np.zeros((V.shape[0], n_chunk * GS))
    Vp[:, :K] = V
    f = np.asarray(field_of)[idx]
    live = np.arange(L)[None, :] < cnt[:, None]
    P = F * (F + 1) // 2
    c = np.zeros((F + P, N))
    for l in range(L):
        xw = x[:, l] * w[idx[:, l]]
        for g in range(F):
            m = live[:, l] & (f[:, l] == g)
            c[g, m] = c[g, m] + xw[m]
    lanes = np.arange(GS)
    for ch in range(n_chunk):
        p, q = np.zeros((F, N, GS)), np.zeros((F, N, GS))
        for l in range(L):
            v = Vp[idx[:, l], ch * GS:(ch + 1) * GS]
            xv = x[:, l, None] * v
            x2v2 = (x[:, l] * x[:, l])[:, None] * (v * v)
            for g in range(F):
                m = live[:, l] & (f[:, l] == g)
                p[g, m] = p[g, m] + xv[m]
                q[g, m] = q[g, m] + x2v2[m]
        for i, (g, h) in enumerate(pairs(F)):
            part = 0.5 * (p[g] * p[g] - q[g]) if g == h else p[g] * p[h]
            m = GS // 2
            while m >= 1:
                part = part + part[:, lanes ^ m]
                m //= 2
            c[F + i] = part[:, 0] if ch == 0 else c[F + i] + part[:, 0]
    return c


def moments_f64(values):
    """(mean, std) over axis 0 by the kernel's recurrence in float64: delta = x - mean; mean += delta (1 / n); M2 += delta (x - mean)"""
    values = np.asarray(values, dtype=np.float64)
    mean, m2 = np.zeros(values.shape[1:]), np.zeros(values.shape[1:])
    for n, v in enumerate(values, start=1):
        delta = v - mean
        mean = mean + delta * (1.0 / n)
        m2 = m2 + delta * (v - mean)
    return mean, np.sqrt(m2 / values.shape[0])


def moments(values):
    """(mean, population std) over axis 0 in longdouble, two passes"""
    values = np.asarray(values, dtype=LD)
    mean = values.sum(axis=0) / values.shape[0]
    return mean, np.sqrt(((values - mean) ** 2).sum(axis=0) / values.shape[0])


class Reference:
    """Everything a test compares against, for the rows of (X, blocks) under `samples` = [(w0, w[D], V[D, K]), ...]:
    c[S, C, N] the components per sample (longdouble), mean / std [C, N] and bias / bias_std over the samples, tol_mean / tol_std
    [C, N] the bounds, twin_mean / twin_std the float64 twin, dev the measured relative deviation of the twin that went into them."""

    def __init__(self, X, blocks, samples, field_of, F):
        rows = flat_rows(X, blocks)
        K = np.asarray(samples[0][2]).shape[1]
        S = len(samples)
        _, GS = contrib_shape(K, F)
        both = [components(rows, w, V, field_of, F) for _, w, V in samples]
        self.F, self.S = F, S
        self.c = np.stack([b[0] for b in both])
        M = np.stack([b[1] for b in both])
        n = 2 * rows[2] + 8 + 6 + max(1, -(-K // GS))
        tol = gamma(n)[None, None, :] * M  # (S, C, N)
        self.mean, self.std = moments(self.c)
        self.bias, self.bias_std = moments(np.asarray([s[0] for s in samples], dtype=LD))
        # w0: four roundings per step of the recurrence, every intermediate at most 2 max|w0| in magnitude
        self.tol_bias = gamma(8 * S + 8) * np.abs(np.asarray([s[0] for s in samples], dtype=LD)).max()
        twin = np.stack([components_f64(rows, w, V, field_of, F) for _, w, V in samples])
        self.twin_mean, self.twin_std = moments_f64(twin)
        scale = M.max(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.maximum(np.abs(self.twin_mean - self.mean), np.abs(self.twin_std - self.std)) / scale
        self.dev = float(np.where(scale > 0, rel, 0).max()) if rel.size else 0.0
        rec = 8 * LD(self.dev) * scale
        self.tol_mean = tol.mean(axis=0) + gamma(S) * np.abs(self.c).mean(axis=0) + rec
        self.tol_std = tol.max(axis=0) + rec
        self.tol_score = tol.sum(axis=1)  # (S, N): the bounds of a sample's components summed, without w0

    def split(self, a):
        return a[:self.F], a[self.F:]

    def check(self, got, label=""):
        """got: (bias, bias_std, linear, linear_std, interaction, interaction_std[, pairs]); asserts every value within its bound and
        returns the worst ratio deviation / bound"""
        bias, bias_std, lin, lin_std, inter, inter_std = got[:6]
        assert abs(LD(bias) - self.bias) <= self.tol_bias and abs(LD(bias_std) - self.bias_std) <= self.tol_bias
        mean, std = np.concatenate([lin, inter]), np.concatenate([lin_std, inter_std])
        assert mean.shape == std.shape == self.mean.shape, (mean.shape, self.mean.shape)
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std >= 0)
        worst = 0.0
        for name, a, b, tol in (("mean", mean, self.mean, self.tol_mean), ("std", std, self.std, self.tol_std)):
            d = np.abs(a.astype(LD) - b)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(tol > 0, d / tol, np.where(d > 0, np.inf, 0))
            w = float(ratio.max()) if ratio.size else 0.0
            worst = max(worst, w)
            print("%s %s: worst deviation / bound %.3f (largest deviation %.3e, twin deviation %.3e)"
                  % (label, name, w, float(d.max()) if d.size else 0.0, self.dev))
            assert np.all(d <= tol), (label, name, w)
        return worst


# ---- the shapes both test files run ----------------------------------------------------------------------------------------
D_TEST = 69  # (about 50: sixteen interleaved fields still leave field 0 five columns)
# the ranks at which k_contrib changes shape: 4 | 16 | 32 | 64 lanes per row at ranks <= 4 | 16 | 32 | above, one factor per lane,
# and a second and third walk of the row from ranks 65 and 129
RANKS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 130)
# the buckets of fields end at 2, 4, 8 and 16
FIELDS = (1, 2, 3, 4, 5, 8, 9, 16)


def grouping(F, kind, D=D_TEST):
    """field_of[D]: 'contiguous' as group_shapes [8, then the rest split evenly] gives it, 'interleaved' j % F"""
    if kind == "interleaved":
        return (np.arange(D) % F).astype(np.int32)
    shapes = [D] if F == 1 else [8] + [len(a) for a in np.array_split(np.arange(D - 8), F - 1)]
    return np.repeat(np.arange(F), shapes).astype(np.int32)


def design37(field_of, F, seed=7):
    """37 rows over D_TEST columns as a CSR matrix: row 0 empty; 1 misses every field but the first; 2 two and 3 five entries in
    field 0, non-unit and negative; 4 one unit entry per field (every I_gg exactly 0); 5 every column of the last field; 6 one unit
    entry alone; the rest random rows of 1 to 8 entries, every third of them unit"""
    import scipy.sparse as sps

    rng = np.random.default_rng(seed)
    D = field_of.shape[0]
    cols_of = [np.flatnonzero(field_of == g) for g in range(F)]
    rows = [([], [])]
    rows.append((cols_of[0][:3], rng.normal(size=3)))
    rows.append((cols_of[0][[0, 2]], [-1.5, 0.75]))
    rows.append((cols_of[0][:5], [2.0, -0.5, 1.25, -3.0, 0.125]))
    rows.append(([c[len(c) // 2] for c in cols_of], np.ones(F)))
    rows.append((cols_of[F - 1], rng.normal(size=len(cols_of[F - 1]))))
    rows.append(([D - 1], [1.0]))
    while len(rows) < 37:
        n = int(rng.integers(1, 9))
        c = rng.choice(D, size=n, replace=False)
        rows.append((c, np.ones(n) if len(rows) % 3 == 0 else rng.normal(size=n)))
    indptr, indices, data = [0], [], []
    for c, v in rows:
        order = np.argsort(np.asarray(c, dtype=np.int64), kind="stable")
        indices.extend(np.asarray(c, dtype=np.int64)[order].tolist())
        data.extend(np.asarray(v, dtype=np.float64)[order].tolist())
        indptr.append(len(indices))
    return sps.csr_matrix((np.asarray(data), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)), shape=(37, D))


def random_samples(D, K, S, seed=11):
    rng = np.random.default_rng(seed + 1000 * K + S)
    return [(float(rng.normal()), rng.normal(size=D), rng.normal(size=(D, K)) / np.sqrt(max(K, 1))) for _ in range(S)]


def shape_cases():
    """(K, F, kind, S) of the host-sample cases: every rank edge at three contiguous fields, every field edge at ranks 3 and 33 in
    both groupings, S in {1, 2, 5}"""
    cases = [(K, 3, "contiguous", 2) for K in RANKS]
    cases += [(K, F, kind, 2) for F in FIELDS for K in (3, 33) for kind in ("contiguous", "interleaved")]
    cases += [(9, 3, "interleaved", S) for S in (1, 5)] + [(65, 5, "contiguous", 5)]
    return cases
