"""Designs, the planner's geometry restated, and a reference for the layout-edge tests of the cell path
(tests/test_cell_edges_cpu.py and tests/test_gpu_cell_edges.py; myfm_amd/csrc/mfm_cell.hpp, mfm_cell.hip).

`build_design` makes an index-tuple design -- unit one-hot main fields + relation blocks -- from EXPLICIT index arrays and column
counts, so that a case chooses its cardinalities, run lengths and chunk lengths instead of drawing them.

`plan` restates what the planner does with such a design (cell_plan_streams, cell_plan_groups_fit with CellPlan::lds_bytes, the
group cuts and the chunk cuts) in plain Python: it gives `want`, the Context.cell_info() a case must report. The GPU test asserts
it before it compares a single number; the CPU test asserts that the figures a case names (`expect`) are what `plan` computes.

The reference is np.longdouble and owes nothing to the cell algebra: update_w (FMTrainer.hpp:231-313) and update_V (:315-482)
as the sequential feature-by-feature sweep over the EXPANDED flat design [main | B_b[map_b] ...] in feature order (the flat and
the blocked form are the same conditional), update_e as the closed-form FM score minus y. Plain NumPy / SciPy: no call into the
oracle or the library.

Limits of the layout (mfm_cell.hpp): a pass workgroup has 156 KiB = 19 968 doubles of LDS; with umax the first-field values of
the largest group, a relation block of B rows on an LDS stream (type C) needs, for its statistics-only pass,
    umax + (the cardinalities of all C streams, its own B among them) + 4 B + 2   doubles (+ 1 where a 16-byte alignment pads),
so alone beside one user it is taken up to B = 3993, while a one-hot main field of 4096 columns (2 sums per value) is taken.
"""
import numpy as np
import scipy.sparse as sps

from .resident_ref import TOL_EQ, TOL_STATE, worst  # noqa: F401  (the single-sweep bounds are the project's: shared, not retyped)
from .test_gpu_cell import TOL_SCORE, TOL_W  # noqa: F401  (w after update_w 1e-10 / 1e-12; the scorer's e 1e-10 / 1e-10)

LD = np.longdouble
NW, WROWS = 16, 384          # wave chunks of a group; rows of a wave per step (64 * CELL_R)
SROWS = NW * WROWS           # 6144: rows of a workgroup per step
SMALL_MAX = 4096             # largest cardinality kept as a whole LDS table (type C)
LDS_DOUBLES = 156 * 1024 // 8
TOL_V = TOL_STATE                        # V after update_V: rtol 1e-9 / atol 1e-11


# ---- designs ------------------------------------------------------------------------------------------------------------------
class Design:
    """main (csr), blocks [(map int64, csr)], y, gi (group of every feature: one per main field and per block), idx (the index
    array of every main field), cards, base (first column of every main field), flat (the expanded design, csr), n, D0, D"""


def block_csr(rng, n, n_cols, per_row):
    """multi-hot rows with non-unit values (what utils.synthetic.tuple_design's block() makes)"""
    c = np.sort(rng.integers(0, n_cols, size=(n, per_row)), axis=1)
    keep = np.ones_like(c, dtype=bool)
    keep[:, 1:] = c[:, 1:] != c[:, :-1]
    rows = np.repeat(np.arange(n), per_row).reshape(n, per_row)
    return sps.csr_matrix((rng.uniform(0.3, 1.0, size=int(keep.sum())), (rows[keep], c[keep])), shape=(n, n_cols))


def build_design(u, extra, cards, blocks, seed):
    """u: the first-field index of every row, sorted; extra: the index arrays of the further main fields; cards: the column count
    of every main field (cardinality is the column range, whatever values occur -- index 0 of every further field must occur,
    since the planner finds a field's first column as the smallest column it sees there); blocks: (map, B, n_cols, per_row) with
    map an int p (the index array of main field p) or an array of its own."""
    rng = np.random.default_rng(seed)
    idx = [np.asarray(a, dtype=np.int64) for a in [u] + list(extra)]
    n, W = idx[0].shape[0], len(idx)
    assert len(cards) == W and np.all(np.diff(idx[0]) >= 0), "rows sorted by the first field"
    for p, (a, card) in enumerate(zip(idx, cards)):
        assert a.shape[0] == n and a.min() >= 0 and a.max() < card
        assert p == 0 or a.min() == 0, "index 0 of a further main field must occur"
    d = Design()
    d.n, d.idx, d.cards = n, idx, list(cards)
    d.base = np.concatenate([[0], np.cumsum(cards)]).astype(np.int64)
    d.D0 = int(d.base[-1])
    ind = np.empty(W * n, dtype=np.int32)
    for p in range(W):
        ind[p::W] = d.base[p] + idx[p]
    d.main = sps.csr_matrix((np.ones(W * n), ind, np.arange(0, W * n + 1, W, dtype=np.int64)), shape=(n, d.D0))
    d.blocks, shapes = [], list(cards)
    for mp, B, n_cols, per_row in blocks:
        mp = idx[mp] if isinstance(mp, (int, np.integer)) else np.asarray(mp, dtype=np.int64)
        assert mp.shape[0] == n and mp.min() >= 0 and mp.max() < B
        d.blocks.append((mp.astype(np.int64), block_csr(rng, B, n_cols, per_row)))
        shapes.append(n_cols)
    d.gi = np.repeat(np.arange(len(shapes)), shapes).astype(np.int32)
    d.D = int(d.gi.shape[0])
    d.flat = sps.hstack([d.main] + [Bm[mp] for mp, Bm in d.blocks], format="csr")
    d.flat.sort_indices()
    assert d.flat.shape == (n, d.D)
    a = rng.normal(size=cards[0]) * 0.3
    d.y = rng.normal(size=n) + a[idx[0]] + (0.3 * np.cos(idx[1] * 0.1) if W > 1 else 0.0)
    return d


# ---- the planner's geometry, restated ------------------------------------------------------------------------------------------
def lds_doubles(streams, fields, umax, P, F, sw, linear=False):
    """CellPlan::lds_bytes in doubles. streams: (type, slot, card); fields: (stream, kind, n); P / F: the pending / the statistics
    field of the pass, or -1"""
    sP = fields[P][0] if P >= 0 else -1
    sF = fields[F][0] if F >= 0 else -1
    size = lambda s: umax if streams[s][0] == "U" else streams[s][2]
    o = 0
    for s, st in enumerate(streams):
        if st[0] == "I" or linear:
            continue
        o += size(s)  # one table ...
        if P >= 0 and F >= 0 and (sw or s == sP or s == sF):
            o += size(s)  # ... or the pending side's and the statistics side's
    if sP >= 0 and streams[sP][0] != "I":  # (d1, d2) of the pending field
        o = (o + 1) & ~1
        o += 2 * size(sP)
    if sF >= 0 and streams[sF][0] != "I":  # the accumulators: 1 sum (update_w), 2 (main field) or 4 (block)
        o = (o + 1) & ~1
        o += (1 if linear else (2 if fields[F][1] == 0 else 4)) * size(sF)
    return o + 2


def _is_split(streams, fields, umax, k):
    m = len(fields)
    return lds_doubles(streams, fields, umax, m - 1 if k == 0 else k - 1, k, k == 0) > LDS_DOUBLES


def groups_fit(streams, fields, umax):
    """cell_plan_groups_fit: every pass of a sweep fits, together or as an apply-only and a statistics-only launch"""
    if umax > 65535:
        return False
    m = len(fields)
    for k in range(m):
        P = m - 1 if k == 0 else k - 1
        need = lds_doubles(streams, fields, umax, P, k, k == 0)
        if need > LDS_DOUBLES:
            need = max(lds_doubles(streams, fields, umax, P, -1, False), lds_doubles(streams, fields, umax, -1, k, False))
        if need > LDS_DOUBLES:
            return False
    return True


def score_fb(streams, umax):
    """CellPlan::score_fb: factors per pass of the scorer"""
    def need(tw):
        o = 0
        for ty, _, card in streams:
            if ty != "I":
                o = (o + tw * (umax if ty == "U" else card) + 1) & ~1
        return o + 2

    fb = 4
    while fb > 1 and need(fb) > LDS_DOUBLES:
        fb //= 2
    return fb if need(fb) <= LDS_DOUBLES else 0


REFUSE_LDS = "a group's tables do not fit the LDS"
REFUSE_TWO_I = "more than one large scattered index stream"
REFUSE_STREAMS = "more index streams than a row record holds"
REFUSE_FIELDS = "more than four fields on one index stream"


def plan(d, n_cu):
    """what Context.cell_info() must say of design d planned for n_cu groups (MFM_CELL_GROUPS)"""
    n, W = d.n, len(d.idx)
    src = list(d.idx)                                  # where every stream's indices come from
    cards = [int(c) for c in d.cards]
    fields = [(p, 0, cards[p]) for p in range(W)]
    for mp, Bm in d.blocks:
        found = next((s for s, a in enumerate(src) if np.array_equal(a, mp)), -1)
        if found < 0:
            if len(src) >= 4:
                return dict(ready=False, why=REFUSE_STREAMS)
            src.append(mp)
            cards.append(0)
            found = len(src) - 1
        cards[found] = max(cards[found], Bm.shape[0])
        fields.append((found, 1, Bm.shape[0]))
    if any(sum(1 for f in fields if f[0] == s) > 4 for s in range(len(src))):
        return dict(ready=False, why=REFUSE_FIELDS)
    streams, n_slots, sI = [["U", 0, cards[0]]], 1, -1
    for s in range(1, len(src)):
        if cards[s] <= SMALL_MAX:
            streams.append(["C", n_slots, cards[s]])
            n_slots += 1
        else:
            if sI >= 0:
                return dict(ready=False, why=REFUSE_TWO_I)
            sI = s
            streams.append(["I", -1, cards[s]])
    item32 = False
    if sI >= 0:
        if cards[sI] <= 65536 and n_slots < 4:
            streams[sI][1] = n_slots
        else:
            item32 = True
    streams = [tuple(st) for st in streams]
    # groups of consecutive first-field values, rows balanced; more groups until every pass fits
    u, cardU = d.idx[0], cards[0]
    for mult in (1, 2, 4, 8, 16):
        G0 = max(1, n_cu) * mult
        target = -(-n // G0)
        grow = [0]
        for g in range(1, G0):
            r = min(n, g * target)
            if 0 < r < n and u[r] == u[r - 1]:
                r = int(np.searchsorted(u, u[r], side="right"))
            if grow[-1] < r < n:
                grow.append(r)
        grow.append(n)
        gu0 = [0] + [int(u[r]) for r in grow[1:-1]] + [cardU]
        umax = int(np.max(np.diff(gu0)))
        if groups_fit(streams, fields, umax):
            break
    else:
        return dict(ready=False, why=REFUSE_LDS)
    G = len(grow) - 1
    # wave chunks: the rows of a group in I order, cut at L j / 16 and moved up to the next change of the I index
    clen, steps = [], []
    for g in range(G):
        R0, R1 = grow[g], grow[g + 1]
        L = R1 - R0
        ks = np.sort(src[sI][R0:R1], kind="stable") if sI >= 0 else None
        c = [0]
        for j in range(1, NW + 1):
            r = L if j == NW else L * j // NW
            if ks is not None and j < NW and 0 < r < L and ks[r] == ks[r - 1]:
                r = int(np.searchsorted(ks, ks[r], side="right"))
            c.append(max(r, c[-1]))
        clen += list(np.diff(c))
        steps.append(-(-max(np.diff(c)) // WROWS))
    m = len(fields)
    return dict(ready=True, why="", G=G, umax=umax, item32=item32, n_streams=len(streams), n_fields=m, N=n,
                Npad=int(sum(steps)) * SROWS, max_steps=int(max(steps)), chunk_max=int(max(clen)), chunk_min=int(min(clen)),
                chunks_empty=int(sum(1 for x in clen if x == 0)),
                split_mask=sum(1 << k for k in range(m) if _is_split(streams, fields, umax, k)),
                score_fb=score_fb(streams, umax), streams=streams, fields=fields)


def max_c_block_rows(umax, other_c=0):
    """the most rows B of a relation block that opens a C stream of its own, beside first-field tables of umax values and other C
    tables of other_c values in all: the largest B whose statistics-only pass lds_bytes(-1, block) fits"""
    streams = lambda B: [("U", 0, umax), ("C", 1, B)] + ([("C", 2, other_c)] if other_c else [])
    fields = lambda B: [(0, 0, umax), (1, 1, B)]
    B = 1
    while lds_doubles(streams(B + 1), fields(B + 1), umax, -1, 1, False) <= LDS_DOUBLES:
        B += 1
    return B


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.array(a, dtype=LD)


def _draw(S1, S2, old, z, lam, mu, alpha):
    prec = lam + alpha * S2  # (a column without rows: lam -- the draw is the prior's)
    return (alpha * (S1 + S2 * old) + lam * mu) / prec + z / np.sqrt(prec)


def _sweep(d, coef, e, q, z, lam, mu, alpha):
    """one pass over all features in feature order; coef: w or V[:, f]; q None: update_w (h = x), else update_V of the factor
    whose q-cache q is (h = x (q - x v)). In place on coef, e, q."""
    n = d.n
    for p, cols in enumerate(d.idx):  # a one-hot field: its columns share no row -- one vectorised level
        lo, hi = int(d.base[p]), int(d.base[p + 1])
        cols = lo + cols
        h = np.ones(n, dtype=LD) if q is None else q - coef[cols]
        S1, S2 = np.zeros(d.D0, dtype=LD), np.zeros(d.D0, dtype=LD)
        np.add.at(S2, cols, h * h)
        np.add.at(S1, cols, -e * h)
        j = np.arange(lo, hi)
        new = _draw(S1[j], S2[j], coef[j], z[j], lam[d.gi[j]], mu[d.gi[j]], alpha)
        delta = np.zeros(d.D0, dtype=LD)
        delta[j] = new - coef[j]
        e += h * delta[cols]
        if q is not None:
            q += delta[cols]
        coef[j] = new
    Fc = d.flatc
    for j in range(d.D0, d.D):  # a block's columns overlap (multi-hot rows): one after the other
        rows = Fc.indices[Fc.indptr[j]:Fc.indptr[j + 1]]
        x = _ld(Fc.data[Fc.indptr[j]:Fc.indptr[j + 1]])
        h = x if q is None else x * (q[rows] - x * coef[j])
        er = e[rows]
        S2, S1 = (h * h).sum(), -(er * h).sum()
        g = d.gi[j]
        new = _draw(S1, S2, coef[j], z[j], lam[g], mu[g], alpha)
        e[rows] = er + h * (new - coef[j])
        if q is not None:
            q[rows] += x * (new - coef[j])
        coef[j] = new


def _flatc(d):
    if not hasattr(d, "flatc"):
        d.flatc = d.flat.tocsc()
        d.flatc.sort_indices()


def _row_sums(d, per_entry):
    return np.add.reduceat(per_entry, d.flat.indptr[:-1])  # (every row has entries: a row of one-hot fields)


def sweep_w_ref(d, w, e, alpha, lam, mu, z):
    """one update_w -> (w, e)"""
    _flatc(d)
    w, e = _ld(w), _ld(e)
    _sweep(d, w, e, None, _ld(z), _ld(lam), _ld(mu), LD(alpha))
    return w, e


def sweep_V_ref(d, V, e, alpha, lam_V, mu_V, zv, f_begin, f_end):
    """update_V of factors f_begin .. f_end-1; lam_V, mu_V (G, K), zv (f_end - f_begin, D) -> (V, e, the last factor's q-cache)"""
    _flatc(d)
    V, e, lam_V, mu_V = _ld(V), _ld(e), _ld(lam_V), _ld(mu_V)
    x, q = _ld(d.flat.data), None
    for f in range(f_begin, f_end):
        vf = V[:, f].copy()
        q = _row_sums(d, x * vf[d.flat.indices])
        _sweep(d, vf, e, q, _ld(zv[f - f_begin]), lam_V[:, f], mu_V[:, f], LD(alpha))
        V[:, f] = vf
    return V, e, q


def score_ref(d, w0, w, V, y):
    """update_e of a regression: the closed-form FM score of the flat design (FM.hpp:54-136) minus y"""
    w, V, x, c = _ld(w), _ld(V), _ld(d.flat.data), d.flat.indices
    s = LD(w0) + _row_sums(d, x * w[c])
    for f in range(V.shape[1]):
        xv = x * V[c, f]
        s += (_row_sums(d, xv) ** 2 - _row_sums(d, xv * xv)) / 2
    return s - _ld(y)


# ---- cases --------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, groups, make, K=3, expect=None, why=None):
        self.name, self.groups, self.make, self.K = name, groups, make, K
        self.env = {"MFM_CELL_MIN_ROWS": "0", "MFM_CELL_GROUPS": str(groups)}
        self.expect = expect or {}  # the cell_info() figures the case is about (a subset of want, stated by hand)
        self.why = why              # set: the planner refuses, and its text starts like this
        self._d = self._want = None

    def design(self):  # (built once, shared by every test of the case, never written to)
        if self._d is None:
            self._d = self.make()
        return self._d

    def want(self):
        if self._want is None:
            self._want = plan(self.design(), self.groups)
        return self._want

    def __repr__(self):
        return self.name


def spread(n_rows, n_users):
    return np.full(n_users, n_rows // n_users) + (np.arange(n_users) < n_rows % n_users)


def users(n_rows, n_users, first=0):
    """sorted first-field indices: n_users consecutive values from `first` share n_rows as evenly as they can"""
    return first + np.repeat(np.arange(n_users), spread(n_rows, n_users))


def ends(rng, n, card):
    """n indices below card, with 0 and card - 1 among them (n >= 2)"""
    a = rng.integers(0, card, size=n)
    a[rng.permutation(n)[:2]] = (0, card - 1)
    return a


def _full(n, u, nU, cI, seed, it=None, cT=4, nBu=None, nBi=None, nBc=6):
    """main fields U, I, T (small) + a block mapped by the user, one mapped by the item, one context block with a map of its
    own: streams U, I, C (T), C (context), a main field and a block on each kind"""
    def make():
        rng = np.random.default_rng(seed)
        item = ends(rng, n, cI) if it is None else np.asarray(it)
        third = np.concatenate([[0], rng.integers(0, cT, size=n - 1)])
        ctx = rng.integers(0, nBc, size=n)
        return build_design(u, [item, third], [nU, cI, cT],
                            [(0, nBu or nU, 12, 3), (1, nBi or cI, 10, 3), (ctx, nBc, 8, 2)], seed)

    return make


def _tiny(n, seed):
    nu = min(3, n)
    if n == 1:  # one row: the item index equals the user index on every row, so the item block joins the U stream (three fields
        # on it); its rows are few, since the stream's cardinality -- and with it umax -- is the largest of its fields'
        return _full(1, users(1, 1), 1, 5000, seed, it=np.zeros(1, dtype=np.int64), nBu=2, nBi=3)
    return _full(n, users(n, nu), nu, 5000, seed)


def _user_blocks(n_blocks, seed):
    # n_blocks relation blocks mapped by the user column beside the user field: 1 + n_blocks fields on the U stream
    def make():
        rng = np.random.default_rng(seed)
        return build_design(users(600, 25), [ends(rng, 600, 5000)], [25, 5000], [(0, 25, 6 + b, 3) for b in range(n_blocks)], seed)

    return make


def _all_distinct(n, seed):
    # one group, every row another item: 16 chunks cut at n j / 16, every row a run head
    def make():
        it = np.random.default_rng(seed).permutation(n)
        return build_design(users(n, 12), [it], [12, n], [(0, 12, 12, 3)], seed)

    return make


def _one_item_per_group(seed):
    # two groups of 1000 rows and 10 users; each group has ONE item: chunk 0 holds the group, its run crosses every window and step
    def make():
        it = np.concatenate([np.zeros(1000, dtype=np.int64), np.full(1000, 4999)])
        return build_design(users(2000, 20), [it], [20, 5000], [(0, 20, 12, 3), (1, 5000, 10, 3)], seed)

    return make


def _run_boundaries(seed):
    # one group of 6400 rows: item 0 has 64 rows (its run ends on a window boundary), item 1 has 320 (ends on row 384, the step
    # boundary), item 2 has 64 (the cut at row 400 moves up to 448, a window boundary of step 2); 5952 further items, one row each
    def make():
        it = np.concatenate([np.repeat([0, 1, 2], [64, 320, 64]), 3 + np.arange(5952)])
        np.random.default_rng(seed).shuffle(it)
        return build_design(users(6400, 9), [it], [9, 5955], [(0, 9, 12, 3)], seed)

    return make


def _absent_users(seed):
    # 40 first-field columns; 0-4, 12-17 and 31-39 never occur (leading, middle, trailing)
    u = np.concatenate([users(140, 7, 5), users(260, 13, 18)])
    return _full(400, u, 40, 5000, seed)


def _no_item_g256(seed):
    # 768 users of 8 rows for 256 groups of 3 users; items and context are LDS tables (no scattered stream: its partials would
    # be G x cardI)
    def make():
        rng = np.random.default_rng(seed)
        ctx = rng.integers(0, 7, size=6144)
        return build_design(users(6144, 768), [ends(rng, 6144, 300)], [768, 300], [(0, 768, 12, 3), (1, 300, 10, 3), (ctx, 7, 8, 2)], seed)

    return make


def _flat3(nU, c1, c2, n, seed, n_users=8):
    # three one-hot fields, no block
    def make():
        rng = np.random.default_rng(seed)
        return build_design(users(n, n_users), [ends(rng, n, c1), ends(rng, n, c2)], [nU, c1, c2], [], seed)

    return make


def _flat4(nU, cI, c1, c2, n, seed):
    def make():
        rng = np.random.default_rng(seed)
        return build_design(users(n, 8), [ends(rng, n, cI), ends(rng, n, c1), ends(rng, n, c2)], [nU, cI, c1, c2], [], seed)

    return make


def _ublock_rows(nU, B, seed):
    # a block mapped by the user column with B rows beside nU user columns (the users that occur are below both)
    lo = min(nU, B)
    return _full(500, users(500, lo), nU, 5000, seed, nBu=B)


def _block_opens_I(seed):
    # no item main field: a block with a map of its own and 5000 rows opens the scattered stream
    def make():
        rng = np.random.default_rng(seed)
        return build_design(users(700, 15), [], [15], [(0, 15, 12, 3), (ends(rng, 700, 5000), 5000, 10, 3)], seed)

    return make


def _c_block(B, seed):
    # one user, and a block of B rows with a map of its own: a C stream of B values
    def make():
        rng = np.random.default_rng(seed)
        return build_design(np.zeros(200, dtype=np.int64), [], [1], [(ends(rng, 200, B), B, 8, 2)], seed)

    return make


def _fit_later(seed):
    # 6000 users with a user block: one group (umax 6000) does not fit, two (umax 3000) fit with the block's pass in split form
    return lambda: build_design(users(12000, 6000), [], [6000], [(0, 6000, 12, 3)], seed)


def _five_streams(seed):
    def make():
        rng = np.random.default_rng(seed)
        own = [(rng.integers(0, 5 + b, size=300), 5 + b, 8, 2) for b in range(3)]
        return build_design(users(300, 10), [ends(rng, 300, 5000)], [10, 5000], own, seed)

    return make


C_BLOCK_MAX = max_c_block_rows(1)  # 3993: 1 + B + 4 B + 2 <= 19968
_S = lambda *st: dict(streams=list(st))
CASES = [
    # ---- the planner
    Case("c_main_4096", 1, _flat3(8, 4096, 5, 300, 301), expect=_S(("U", 0, 8), ("C", 1, 4096), ("C", 2, 5))),
    Case("i_main_4097", 1, _flat3(8, 4097, 5, 300, 302), expect=_S(("U", 0, 8), ("I", 2, 4097), ("C", 1, 5))),
    Case("i_65536_slot16", 4, _full(3000, users(3000, 40), 40, 65536, 303), expect=dict(item32=False, G=4)),
    Case("i_65537_item32", 4, _full(3000, users(3000, 40), 40, 65537, 304), expect=dict(item32=True, G=4)),
    Case("fits_at_second_multiple_split", 1, _fit_later(305), K=2, expect=dict(G=2, umax=3000, split_mask=0b10)),
    Case("split_flat_4096x4096", 1, _flat3(2000, 4096, 4096, 600, 306), expect=dict(G=1, umax=2000, split_mask=0b111, score_fb=1)),
    Case("c_block_largest_that_fits", 1, _c_block(C_BLOCK_MAX, 307), expect=dict(G=1, umax=1, split_mask=0b10)),
    Case("c_block_one_more_refused", 1, _c_block(C_BLOCK_MAX + 1, 308), why=REFUSE_LDS),
    Case("two_scattered_refused", 1, _flat3(8, 5000, 5000, 300, 309), why=REFUSE_TWO_I),
    Case("five_streams_refused", 1, _five_streams(310), why=REFUSE_STREAMS),
    Case("three_fields_on_U", 2, _user_blocks(2, 316), expect=_S(("U", 0, 25), ("I", 1, 5000))),
    Case("four_fields_on_U", 2, _user_blocks(3, 317), expect=_S(("U", 0, 25), ("I", 1, 5000))),
    Case("five_fields_on_U_refused", 2, _user_blocks(4, 318), why=REFUSE_FIELDS),
    Case("ublock_fewer_rows_than_columns", 3, _ublock_rows(30, 21, 311), expect=_S(("U", 0, 30), ("I", 3, 5000), ("C", 1, 4), ("C", 2, 6))),
    Case("ublock_more_rows_than_columns", 3, _ublock_rows(21, 30, 312), expect=_S(("U", 0, 30), ("I", 3, 5000), ("C", 1, 4), ("C", 2, 6))),
    Case("block_opens_I_stream", 2, _block_opens_I(313), expect=_S(("U", 0, 15), ("I", 1, 5000))),
    Case("iblock_more_rows_than_columns", 2, _full(800, users(800, 16), 16, 5000, 314, nBi=5200),
         expect=_S(("U", 0, 16), ("I", 3, 5200), ("C", 1, 4), ("C", 2, 6))),
    Case("iblock_fewer_rows_than_columns", 2, _full(800, users(800, 16), 16, 5000, 315, nBi=4500,
                                                     it=np.concatenate([[0, 4499], np.arange(798) * 5 % 4500])),
         expect=_S(("U", 0, 16), ("I", 3, 5000), ("C", 1, 4), ("C", 2, 6))),
    # ---- the pass: chunks, steps, runs
    Case("tiny_1", 2, _tiny(1, 321), expect=dict(G=1, chunks_empty=15, chunk_max=1, streams=[("U", 0, 3), ("I", 3, 5000), ("C", 1, 4), ("C", 2, 6)])),
    Case("tiny_2", 2, _tiny(2, 322), expect=dict(chunk_max=1)),
    Case("tiny_63", 2, _tiny(63, 323)),
    Case("tiny_64", 2, _tiny(64, 324)),
    Case("tiny_65", 2, _tiny(65, 325)),
    Case("rows_6144_all_distinct", 1, _all_distinct(6144, 326),
         expect=dict(G=1, chunk_max=384, chunk_min=384, chunks_empty=0, max_steps=1, Npad=6144)),
    Case("rows_6145_one_row_in_step_2", 1, _all_distinct(6145, 327),
         expect=dict(G=1, chunk_max=385, chunk_min=384, chunks_empty=0, max_steps=2, Npad=12288)),
    Case("one_item_per_group", 2, _one_item_per_group(328), expect=dict(G=2, chunk_max=1000, chunk_min=0, chunks_empty=30, max_steps=3)),
    Case("runs_end_on_window_and_step", 1, _run_boundaries(329), expect=dict(G=1, chunk_max=448, chunk_min=352, max_steps=2)),
    Case("single_user", 7, _full(500, np.zeros(500, dtype=np.int64), 1, 5000, 330), expect=dict(G=1, umax=1)),
    Case("absent_first_field_values", 3, _absent_users(331), expect=dict(G=3)),
    Case("groups_1", 1, _full(900, users(900, 60), 60, 5000, 332), expect=dict(G=1, umax=60)),
    Case("groups_2", 2, _full(900, users(900, 60), 60, 5000, 333), expect=dict(G=2, umax=30)),
    Case("groups_7", 7, _full(900, users(900, 60), 60, 5000, 334), expect=dict(G=7)),
    Case("groups_9", 9, _full(900, users(900, 60), 60, 5000, 335), expect=dict(G=9)),
    Case("groups_256_lds_streams_only", 256, _no_item_g256(336), expect=dict(G=256)),
]
CASE = {c.name: c for c in CASES}

# the scorer: FB = 4, 2, 1 by the LDS its tables need, at both item widths; the rank is the test's parameter
SCORE_RANKS = [1, 4, 5, 33]
SCORE_CASES = [
    Case("score_fb4_item16", 2, _full(700, users(700, 30), 30, 5000, 341), expect=dict(score_fb=4, item32=False)),
    Case("score_fb4_item32", 2, _full(700, users(700, 30), 30, 65537, 342), expect=dict(score_fb=4, item32=True)),
    Case("score_fb2_item16", 1, _flat4(1000, 5000, 4096, 5, 500, 343), expect=dict(score_fb=2, item32=False)),
    Case("score_fb2_item32", 1, _flat4(1000, 65537, 4096, 5, 500, 344), expect=dict(score_fb=2, item32=True)),
    Case("score_fb1_item16", 1, _flat4(2000, 5000, 4096, 4096, 500, 345), expect=dict(score_fb=1, item32=False)),
    Case("score_fb1_item32", 1, _flat4(2000, 65537, 4096, 4096, 500, 346), expect=dict(score_fb=1, item32=True)),
]
ROW_CAP = 82000


def problem(d, K, seed):
    """the state (normal x 0.1, as elsewhere in the suite), a residual, hyper-parameters and variates of one call each"""
    rng = np.random.default_rng(seed)
    G = int(d.gi.max()) + 1
    return dict(w0=0.3, w=rng.normal(size=d.D) * 0.1, V=rng.normal(size=(d.D, K)) * 0.1, e=rng.normal(size=d.n),
                alpha=0.9, lam_w=rng.uniform(0.5, 2.0, size=G), mu_w=rng.normal(size=G) * 0.1,
                lam_V=rng.uniform(0.5, 2.0, size=(G, K)), mu_V=rng.normal(size=(G, K)) * 0.1,
                zw=rng.normal(size=d.D), zv=rng.normal(size=(K, d.D)))


_REF = {}


def reference(case):
    """(problem, dict of the longdouble results of one update_w, one update_V(0, K) and one update_e, each from the problem's
    state) of a case, computed once"""
    if case.name not in _REF:
        d = case.design()
        p = problem(d, case.K, 7)
        w, ew = sweep_w_ref(d, p["w"], p["e"], p["alpha"], p["lam_w"], p["mu_w"], p["zw"])
        V, eV, q = sweep_V_ref(d, p["V"], p["e"], p["alpha"], p["lam_V"], p["mu_V"], p["zv"], 0, case.K)
        _REF[case.name] = (p, dict(w=w, e_w=ew, V=V, e_V=eV, q=q, score=score_ref(d, p["w0"], p["w"], p["V"], d.y)))
    return _REF[case.name]


QUANTITIES = dict(w=TOL_W, e_w=TOL_EQ, V=TOL_V, e_V=TOL_EQ, q=TOL_EQ, score=TOL_SCORE)
