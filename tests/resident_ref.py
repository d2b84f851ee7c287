"""Reference and designs for the layout-edge tests of the persistent sweep (tests/test_resident_edges_cpu.py and
tests/test_gpu_resident_edges.py).

`sweep_ref` is one fused sweep (mfm_sweep_wV: update_w0's shift, update_w, update_V of factors f_begin..f_end;
FMTrainer.hpp:226, :231-254, :316-376) of a two-field unit one-hot table in np.longdouble, written from the kernel header of
myfm_amd/csrc/mfm_res.hpp: plain NumPy, no call into the oracle or the library.

`build_table` makes a user-sorted two-field table from EXPLICIT per-workgroup user and item assignments, and says what layout the
planner (ResPlan::choose_layout: workgroup g ends at the user boundary nearest to g N / G) must then report: a case states its
geometry, and the GPU test asserts it through Context.res_info() before it compares a single number.

Capacities (mfm_res.hpp): 512 threads per workgroup; 16, 32 or 64 + 16 slots per thread on chip, then 16 .. 80 more per thread
streamed from global memory; a workgroup of s slots per thread holds at most 512 s - 1 rows (one pad slot closes the last run);
at most 512 users per workgroup and 512 items per slice (a thread draws each).
"""
import numpy as np
import scipy.sparse as sps

LD = np.longdouble
NT = 512


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _level(cols, lo, hi, h, e, v, z, lam, mu, gi, alpha):
    """columns lo..hi-1 of one level (no two of them share a row): statistics, draw, residual update. In place on e and v."""
    D = v.shape[0]
    S1, S2 = np.zeros(D, dtype=LD), np.zeros(D, dtype=LD)
    np.add.at(S2, cols, h * h)
    np.add.at(S1, cols, -e * h)
    j = np.arange(lo, hi)
    lam_j, mu_j = lam[gi[j]], mu[gi[j]]
    prec = lam_j + alpha * S2[j]  # (a column without rows: lam -- the draw is the prior's)
    new = (alpha * (S1[j] + S2[j] * v[j]) + lam_j * mu_j) / prec + z[j] / np.sqrt(prec)
    d = np.zeros(D, dtype=LD)
    d[j] = new - v[j]
    e += h * d[cols]
    v[j] = new


def sweep_ref(u, i, n_user_cols, gi, w, V, e, alpha, e_shift, lam_w, mu_w, zw, f_begin, f_end, lam_V, mu_V, zv):
    """u, i: the two columns of every row (u < n_user_cols <= i); gi: group of every column; w (D), V (D, K), e (N): the state;
    lam_w, mu_w (G); lam_V, mu_V (G, K); zw (D); zv (f_end - f_begin, D). zw None: no linear sweep.
    Returns (w, V, e, q) in longdouble; q is the q-cache of the last factor swept (FMTrainer.hpp:320, :373), None without one."""
    ld = lambda a: np.array(a, dtype=LD)
    w, V, e = ld(w), ld(V), ld(e)
    lam_w, mu_w, lam_V, mu_V = ld(lam_w), ld(mu_w), ld(lam_V), ld(mu_V)
    alpha = LD(alpha)
    D = w.shape[0]
    e += LD(e_shift)
    one = np.ones(u.shape[0], dtype=LD)
    if zw is not None:
        zw = ld(zw)
        _level(u, 0, n_user_cols, one, e, w, zw, lam_w, mu_w, gi, alpha)
        _level(i, n_user_cols, D, one, e, w, zw, lam_w, mu_w, gi, alpha)
    q = None
    for f in range(f_begin, f_end):
        vf, z = V[:, f].copy(), ld(zv[f - f_begin])
        _level(u, 0, n_user_cols, vf[i], e, vf, z, lam_V[:, f], mu_V[:, f], gi, alpha)
        _level(i, n_user_cols, D, vf[u], e, vf, z, lam_V[:, f], mu_V[:, f], gi, alpha)
        V[:, f] = vf
        q = vf[u] + vf[i]
    return w, V, e, q


def score_ref(u, i, w0, w, V, y):
    """update_e of a regression (FMTrainer.hpp:493-497 -> FM.hpp:54-136) in longdouble"""
    ld = lambda a: np.array(a, dtype=LD)
    w, V = ld(w), ld(V)
    return LD(w0) + w[u] + w[i] + (V[u] * V[i]).sum(axis=1) - ld(y)


# ---- designs ------------------------------------------------------------------------------------------------------------------
class Table:
    """X (csr), y, gi (group of every column: 0 users, 1 items), u, i (columns of every row), n_user_cols, and `want`: the
    res_info() fields the planner must report for the assignment the table was built from"""


def build_table(wgs, seed, n_items=None):
    """wgs: per workgroup (user_rows, items) -- user_rows: rows of each of its users, in order; items: the item (0-based id) of
    each of its rows, in row order. Every user and every item 0 .. n_items-1 must occur (no never-drawn column changes the
    counts the case states)."""
    rng = np.random.default_rng(seed)
    u_parts, i_parts, n_users, runs, maxu = [], [], 0, 0, 0
    for user_rows, items in wgs:
        user_rows, items = np.asarray(user_rows, dtype=np.int64), np.asarray(items, dtype=np.int64)
        assert user_rows.min() >= 1 and user_rows.sum() == items.shape[0]
        u_parts.append(n_users + np.repeat(np.arange(user_rows.shape[0]), user_rows))
        i_parts.append(items)
        n_users += user_rows.shape[0]
        runs += np.unique(items).shape[0]
        maxu = max(maxu, user_rows.shape[0])
    u, it = np.concatenate(u_parts), np.concatenate(i_parts)
    if n_items is None:
        n_items = int(it.max()) + 1
    assert np.unique(it).shape[0] == n_items and it.max() == n_items - 1, "every item must occur"
    n = u.shape[0]
    t = Table()
    t.n, t.n_user_cols, t.D = n, n_users, n_users + n_items
    t.u, t.i = u.astype(np.int32), (n_users + it).astype(np.int32)
    ind = np.empty(2 * n, dtype=np.int32)
    ind[0::2], ind[1::2] = t.u, t.i
    t.X = sps.csr_matrix((np.ones(2 * n), ind, np.arange(0, 2 * n + 1, 2)), shape=(n, t.D))
    t.gi = np.concatenate([np.zeros(n_users, dtype=np.int32), np.ones(n_items, dtype=np.int32)])
    a, b = rng.normal(size=n_users) * 0.3, rng.normal(size=n_items) * 0.3
    t.y = rng.normal(size=n) + a[u] + b[it]
    t.want = dict(G=len(wgs), n_items=n_items, n_runs=runs, max_wg_users=maxu, n_rows=n)
    return t


def spread(n_rows, n_users):
    """rows of n_users users that share n_rows as evenly as they can"""
    return np.full(n_users, n_rows // n_users) + (np.arange(n_users) < n_rows % n_users)


def draw_items(rng, n_rows, n_items):
    """uniform items, every one at least once (n_rows >= n_items), shuffled"""
    it = np.concatenate([np.arange(n_items), rng.integers(0, n_items, size=n_rows - n_items)])
    rng.shuffle(it)
    return it


def planner_cuts(user_rows, G):
    """ResPlan::choose_layout's cuts where no capacity binds: workgroup g ends at the user boundary nearest to g N / G (a tie goes
    to the earlier one), every workgroup gets a user. Returns the users per workgroup."""
    ustart = np.concatenate([[0], np.cumsum(user_rows)])
    n_users, N = len(user_rows), int(ustart[-1])
    cuts = [0]
    for g in range(1, G):
        want = (N * g) // G
        hi = int(np.searchsorted(ustart, want, side="right")) - 1
        if hi + 1 <= n_users and ustart[hi + 1] - want < want - ustart[hi]:
            hi += 1
        hi = min(max(hi, cuts[-1] + 1), n_users - (G - g))
        cuts.append(hi)
    cuts.append(n_users)
    return np.diff(cuts)


class Case:
    def __init__(self, name, env, make, K=3, expect=None, why=None, overflow=False):
        self.name, self.env, self.make, self.K = name, env, make, K
        self.expect = expect or {}  # res_info() fields beyond Table.want
        self.why = why              # set: the planner refuses, and its text starts like this
        self.overflow = overflow
        self._t = None

    def table(self):  # (built once, shared by every test of the case, never written to)
        if self._t is None:
            self._t = self.make()
        return self._t

    def __repr__(self):
        return self.name


ONE_CU = {"MFM_RES_CUS": "1"}


def _wgs_env(g):
    return {"MFM_RES_CUS": str(g), "MFM_RES_WGS": str(g)}


def _one_wg(n, n_users, n_items, seed):
    def make():
        rng = np.random.default_rng(seed)
        return build_table([(spread(n, n_users), draw_items(rng, n, n_items))], seed)

    return make


def _many_users(n_wg, users_per_wg, rows_per_user, n_items, seed):
    def make():
        rng = np.random.default_rng(seed)
        rows = users_per_wg * rows_per_user
        it = draw_items(rng, n_wg * rows, n_items)
        return build_table([(np.full(users_per_wg, rows_per_user), it[g * rows:(g + 1) * rows]) for g in range(n_wg)], seed)

    return make


def _all_heads(seed):
    # 4 workgroups of 1500 rows, 2000 items, an item at most once per workgroup: every slot starts a run, every partial is one slot
    def make():
        rng = np.random.default_rng(seed)
        wgs = []
        for g in range(4):
            it = (500 * g + np.arange(1500)) % 2000
            rng.shuffle(it)
            wgs.append((spread(1500, 50), it))
        return build_table(wgs, seed)

    return make


def _one_item(rows_per_wg, users_per_wg, seed):
    def make():
        return build_table([(spread(rows_per_wg, users_per_wg), np.zeros(rows_per_wg, dtype=np.int64)) for g in range(3)], seed)

    return make


def _config3_mix(seed):
    # 4 workgroups of 8000 rows and 275 users, about 2000 items with Zipf-like popularity: mean (workgroup, item) run near 5 slots
    def make():
        rng = np.random.default_rng(seed)
        p = 1.0 / (np.arange(2000) + 12.0) ** 0.85
        it = rng.choice(2000, size=32000, p=p / p.sum())
        it = np.unique(it, return_inverse=True)[1]  # (items that were never drawn leave no empty column)
        return build_table([(spread(8000, 275), it[8000 * g:8000 * (g + 1)]) for g in range(4)], seed)

    return make


def _tiny(n, n_users, n_items, seed):
    def make():
        rng = np.random.default_rng(seed)
        return build_table([(spread(n, n_users), draw_items(rng, n, n_items))], seed)

    return make


def _lopsided(seed):
    # one user of 8000 rows, then 600 users of one row: the row-balanced cut would leave 600 users to the second workgroup; the
    # planner moves 88 of them into the first (8088 of its 8191 rows) so that the second draws 512
    def make():
        rng = np.random.default_rng(seed)
        it = draw_items(rng, 8600, 100)
        return build_table([(np.concatenate([[8000], np.ones(88, dtype=np.int64)]), it[:8088]), (np.ones(512, dtype=np.int64), it[8088:])],
                           seed)

    return make


N_CU = 256  # MI355X


def _all_cus(seed):
    # 600 users of 50 rows on 256 workgroups: 2 or 3 users, about 117 rows each
    def make():
        rng = np.random.default_rng(seed)
        rows = np.full(600, 50)
        it = draw_items(rng, 30000, 150)
        ends = np.cumsum(planner_cuts(rows, N_CU)) * 50
        return build_table([(np.full((e - b) // 50, 50), it[b:e]) for b, e in zip(np.concatenate([[0], ends[:-1]]), ends)], seed)

    return make


def _v(rv, rl=0, rx=0):
    return dict(RV=rv, RL=rl, RX=rx)


NO_FIT = "no variant fits"
CASES = [
    # capacity boundaries of one workgroup: cap = 512 slots - 1
    Case("cap_8191_rv16", ONE_CU, _one_wg(8191, 60, 100, 101), expect=_v(16)),
    Case("cap_8192_rv32", ONE_CU, _one_wg(8192, 60, 100, 102), expect=_v(32)),
    Case("cap_16383_rv32", ONE_CU, _one_wg(16383, 60, 100, 103), expect=_v(32)),
    Case("cap_16384_rv64_rl16", ONE_CU, _one_wg(16384, 60, 100, 104), expect=_v(64, 16)),
    Case("cap_40959_last_on_chip", ONE_CU, _one_wg(40959, 60, 100, 105), expect=_v(64, 16)),
    Case("cap_40960_rx16", ONE_CU, _one_wg(40960, 60, 100, 106), expect=_v(64, 16, 16), overflow=True),
    Case("cap_81919_rx80", ONE_CU, _one_wg(81919, 60, 100, 107), expect=_v(64, 16, 80), overflow=True),
    Case("cap_81920_refused", ONE_CU, _one_wg(81920, 60, 100, 108), why=NO_FIT),
    # users per workgroup: 10-bit fields, the fourth user of a batch split over two words
    Case("users_512_one_wg", ONE_CU, _one_wg(8000, 512, 100, 111), expect=dict(_v(16), umax=513)),
    Case("users_513_refused", ONE_CU, _one_wg(8000, 513, 100, 112), why="more first-level columns in a workgroup than threads"),
    Case("users_273_per_wg_x4", _wgs_env(4), _many_users(4, 273, 7, 120, 113), expect=_v(16)),
    # a single user: G = 1 whatever the device offers; every lane of every LDS add hits one address
    Case("single_user_30011", {}, _one_wg(30011, 1, 100, 121), expect=dict(_v(64, 16), umax=101)),
    Case("single_user_50000_overflow", {}, _one_wg(50000, 1, 100, 122), expect=dict(_v(64, 16, 32), umax=101), overflow=True),
    # items per slice
    Case("items_512_one_wg", ONE_CU, _one_wg(3000, 40, 512, 131), expect=dict(_v(16), max_slice_items=512, umax=513)),
    Case("items_513_refused", ONE_CU, _one_wg(3000, 40, 513, 132), why="more second-level columns than the workgroups can draw"),
    Case("all_heads_x4", _wgs_env(4), _all_heads(141), expect=dict(_v(16), n_runs=6000)),
    # one item: a workgroup is ONE run over its threads (segmented scan + wave carry), one slice draws it from G partials
    Case("one_item_x3_19998", _wgs_env(3), _one_item(6666, 6, 151), expect=dict(_v(16), n_runs=3, max_slice_items=1)),
    Case("one_item_x3_all_512_threads", _wgs_env(3), _one_item(8184, 6, 152), expect=dict(_v(16), n_runs=3, max_slice_items=1)),
    Case("config3_mix_x4", _wgs_env(4), _config3_mix(161), expect=_v(16)),
    # tiny tables: almost every slot a pad
    Case("tiny_1", {}, _tiny(1, 1, 1, 171), expect=_v(16)),
    Case("tiny_7", {}, _tiny(7, 3, 2, 172), expect=_v(16)),
    Case("tiny_63", {}, _tiny(63, 5, 4, 173), expect=_v(16)),
    Case("tiny_64", {}, _tiny(64, 5, 4, 174), expect=_v(16)),
    Case("tiny_65", {}, _tiny(65, 5, 4, 175), expect=_v(16)),
    Case("lopsided_cuts", {}, _lopsided(181), expect=_v(16)),
    # the production workgroup count: every XCD, full census, hierarchical barrier
    Case("all_cus_at_the_barrier", _wgs_env(N_CU), _all_cus(191), expect=_v(16)),
    # rank
    Case("config3_mix_x4_rank33", _wgs_env(4), _config3_mix(161), K=33, expect=_v(16)),
    Case("tiny_7_rank1", {}, _tiny(7, 3, 2, 172), K=1, expect=_v(16)),
]
CASE = {c.name: c for c in CASES}

# the slot-order scorer's instantiations: one workgroup of R / 16 = 1, 2, 5 .. 10 groups of 16 slots per thread
SCORE_NG = {8000: 1, 16000: 2, 40000: 5, 41000: 6, 49200: 7, 57400: 8, 65600: 9, 73800: 10}
SCORE_CASES = [Case("score_ng%d_%d" % (ng, n), ONE_CU, _one_wg(n, 60, 100, 200 + ng), K=6, expect=dict(ng=ng)) for n, ng in SCORE_NG.items()]


def problem(t, K, seed):
    """the state (normal x 0.1, as elsewhere in the suite), a residual, hyper-parameters and variates of one fused sweep"""
    rng = np.random.default_rng(seed)
    G = 2
    return dict(w0=0.3, w=rng.normal(size=t.D) * 0.1, V=rng.normal(size=(t.D, K)) * 0.1, e=rng.normal(size=t.n),
                alpha=0.9, e_shift=0.05, lam_w=rng.uniform(0.5, 2.0, size=G), mu_w=rng.normal(size=G) * 0.1,
                lam_V=rng.uniform(0.5, 2.0, size=(G, K)), mu_V=rng.normal(size=(G, K)) * 0.1,
                zw=rng.normal(size=t.D), zv=rng.normal(size=(K, t.D)))


_REF = {}


def reference(case):
    """(problem, sweep_ref's result) of a case, computed once"""
    if case.name not in _REF:
        t = case.table()
        p = problem(t, case.K, 7)
        _REF[case.name] = (p, sweep_ref(t.u, t.i, t.n_user_cols, t.gi, p["w"], p["V"], p["e"], p["alpha"], p["e_shift"], p["lam_w"],
                                        p["mu_w"], p["zw"], 0, case.K, p["lam_V"], p["mu_V"], p["zv"]))
    return _REF[case.name]


# the project's single-sweep bound (test_resident_factor_subranges_and_empty_columns), against the longdouble reference
TOL_STATE = dict(rtol=1e-9, atol=1e-11)
TOL_EQ = dict(rtol=1e-8, atol=1e-9)


def worst(got, want, rtol, atol):
    """largest |got - want| / (atol + rtol |want|): <= 1 is what assert_allclose(got, want, rtol, atol) accepts"""
    want = np.asarray(want, dtype=LD)
    d = np.abs(np.asarray(got, dtype=LD) - want) / (LD(atol) + LD(rtol) * np.abs(want))
    return float(d.max()) if d.size else 0.0
