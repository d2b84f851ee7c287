"""The persistent sweep's phase edges (k_mf_resident, myfm_amd/csrc/mfm_res.hpp): the first sweep's sum of h^2 loaded from the
plan's table (ResPlan::s2_lin) when the launch starts with the linear sweep, and the item draw's list entries packed into 4 bytes
(mfm_res_entry.hpp).

The tables are those of tests/resident_ref.py, one per layout edge. Every test first proves through Context.res_info() the
geometry the case names, the kernel form (field 13, `s2_in_sweep_b`: only <512, 4, 1> and its overflow form have it, where the
third accumulator array fits the LDS -- only there is the table read) and the width of the list entries (field 15,
`entry_bytes`: 4 on every unsharded plan of these sizes, 8 row-sharded). Then:
  (a) one mfm_sweep_wV against the np.longdouble reference (resident_ref.sweep_ref) at the bounds of
      tests/test_gpu_resident_edges.py (w, V: rtol 1e-9 / atol 1e-11; e, q: rtol 1e-8 / atol 1e-9), with MFM_PLAN_CHECK (the host
      planner's arrays, the packed list and the table among them, against the device planner's) and without it;
  (b) three iterations against the oracle draw for draw and a second context bit for bit (the Zipf mix and the 4 x 273 table);
  (c) split launches against the fused one bit for bit; (d) one row-sharded case: the exchange form keeps the 8-byte list.
A user's count in the table is the linear sweep's S2 of that user: one slot more or less moves w by far more than (a)'s bound.
"""
import threading

import numpy as np
import pytest

from . import datasets as ds
from . import resident_ref as R
from .gibbs_driver import CapiGibbs

pytestmark = pytest.mark.gpu

NT, NW = 512, 8
LDS_LIMIT = 160 * 1024 - 512


def _s2_form(info):
    """ResPlan::plan_lds: the form with the third accumulator array exists for 64 + 16 slots per thread (with or without overflow
    slots) and is taken where the array fits the LDS"""
    two = info["RL"] * NT * 8 + 2 * NW * info["umax"] * 8 + info["umax"] * 16 + NW * 16 + NW * 4 + 64
    return 1 if (info["RV"], info["RL"]) == (64, 16) and two + NW * info["umax"] * 8 <= LDS_LIMIT else 0


# the tables of (a), by the edge they stand for
TABLES = [
    "tiny_1", "tiny_7", "tiny_63", "tiny_64", "tiny_65",   # pads: almost every slot, around a wave's width
    "single_user_30011",            # one user: a count of thousands on one address of the table; G = 1; the table is read
    "single_user_50000_overflow",   # ... and the overflow slots are counted too
    "users_273_per_wg_x4",          # 4 workgroups x 273 users
    "all_heads_x4",                 # every slot a run head: as many list entries as rows
    "one_item_x3_19998",            # one item: one slice draws it from G partials
    "items_512_one_wg",             # local item 511 fills the entry's 9 bits
    "all_cus_at_the_barrier",       # 256 workgroups: every XCD, every slice's list across all sources
    "config3_mix_x4_rank33",        # the Zipf mix at K = 33
    "tiny_7_rank1",                 # K = 1
]
S2_FORM = {"single_user_30011": 1, "single_user_50000_overflow": 1}  # (every other table: 16 slots per thread, two arrays)
# one workgroup of 20 000 rows, 60 users, 100 items: the form that reads the table, with users of several hundred rows
ONE_WG_S2 = R.Case("one_wg_20000", R.ONE_CU, R._one_wg(20000, 60, 100, 301), expect=dict(RV=64, RL=16, RX=0))


@pytest.fixture(autouse=True)
def _small_tables_take_the_persistent_sweep(monkeypatch):
    monkeypatch.setenv("MFM_RES_MIN_ROWS", "0")
    monkeypatch.setenv("MFM_SCATTER_MIN_NNZ", "1000")


@pytest.fixture(scope="module")
def capi():
    from myfm_amd import _capi

    if _capi.lib().mfm_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _capi


def _env(monkeypatch, case, checked=None):
    for k in ("MFM_RES_CUS", "MFM_RES_WGS", "MFM_NO_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if checked is True:
        monkeypatch.setenv("MFM_PLAN_CHECK", "1")
    elif checked is False:
        monkeypatch.delenv("MFM_PLAN_CHECK", raising=False)


def _assert_geometry(c, case, s2_form):
    """the variant, the kernel form and the list width the case names -- before any number is compared"""
    info, flags, t = c.res_info(), c.plan_flags(), case.table()
    assert info["ready"], info["why"]
    for k, v in dict(t.want, **case.expect).items():
        assert info[k] == v, (k, info)
    assert flags["resident"] and flags["resident_overflow"] == case.overflow == (info["RX"] > 0)
    assert info["s2_in_sweep_b"] == s2_form == _s2_form(info), info
    assert info["n_runs"] + info["G"] < 2 ** 23 and info["entry_bytes"] == 4, info  # (run indices: the pad runs and the zero run too)
    assert info["max_slice_items"] <= 512
    return info


def _check(got, ref, what):
    w, V, e, q = ref
    pairs = dict(w=(got[1], w, R.TOL_STATE), V=(got[2], V, R.TOL_STATE), e=(got[3], e, R.TOL_EQ))
    if q is not None:
        pairs["q"] = (got[4], q, R.TOL_EQ)
    print("%s: %s" % (what, {k: (float(np.abs(g - r).max()), R.worst(g, r, **tol)) for k, (g, r, tol) in pairs.items()}))
    for k, (g, r, tol) in pairs.items():
        np.testing.assert_allclose(g, r.astype(np.float64), err_msg="%s, %s" % (k, what), **tol)


@pytest.mark.parametrize("checked", [True, False], ids=["checked", "device_planner_alone"])
@pytest.mark.parametrize("name", TABLES)
def test_one_sweep_against_the_longdouble_reference(capi, monkeypatch, name, checked):
    case = R.CASE[name]
    _env(monkeypatch, case, checked)
    t = case.table()
    p, ref = R.reference(case)
    c = capi.Context(t.X, t.y, rank=case.K, group_index=t.gi)
    try:
        _assert_geometry(c, case, S2_FORM.get(name, 0))
        c.set_state(p["w0"], p["w"], p["V"])
        c.set_e(p["e"])
        c.sweep_wV(p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"], p["zw"], 0, case.K, p["lam_V"], p["mu_V"], p["zv"])
        assert c.res_info()["e_where"] == "slots"  # (the persistent launch ran and left its residual in slot order)
        got = c.get_state() + (c.get_e(), c.get_q())
    finally:
        c.close()
    assert got[0] == p["w0"]
    _check(got, ref, "%s %s" % (name, "checked" if checked else "device planner alone"))


@pytest.mark.parametrize("name", ["config3_mix_x4", "users_273_per_wg_x4"])
def test_three_iterations_against_the_oracle_and_a_rerun(oracle, capi, monkeypatch, name):
    case = R.CASE[name]
    _env(monkeypatch, case)
    t = case.table()
    n, K = t.n, case.K
    chains = []
    for rep in range(2):
        o = oracle.OracleTrainer(t.X, t.y, rank=K, group_index=t.gi)
        c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
        try:
            _assert_geometry(c, case, 0)
            c.set_state(*o.fm())
            c.set_e(o.e(n))
            drv = CapiGibbs(c, o.clone(), n, t.gi, fused=True)
            for it in range(3):
                drv.step()
                if rep == 0:  # (the second context is held against the first, bit for bit)
                    o.step()
                    w0, w, V = o.fm()
                    gw0, gw, gV = c.get_state()
                    np.testing.assert_allclose(gV, V, rtol=1e-7, atol=1e-8, err_msg="V, iteration %d" % it)
                    np.testing.assert_allclose(gw, w, rtol=1e-7, atol=1e-8, err_msg="w, iteration %d" % it)
                    np.testing.assert_allclose(gw0, w0, rtol=1e-7, atol=1e-8)
            if rep == 0:
                np.testing.assert_allclose(c.get_e(), o.e(n), rtol=1e-7, atol=1e-7)
            chains.append(c.get_state() + (c.get_e(),))
        finally:
            c.close()
    assert chains[0][0] == chains[1][0]
    for a, b in zip(chains[0][1:], chains[1][1:]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("case,s2_form", [(ONE_WG_S2, 1), (R.CASE["single_user_50000_overflow"], 1), (R.CASE["config3_mix_x4"], 0)],
                         ids=lambda v: repr(v))
def test_split_launches_bit_for_bit(capi, monkeypatch, case, s2_form):
    """mfm_sweep_wV(0, 1) then mfm_sweep_V(1, K) == mfm_sweep_wV(0, K), bit for bit, and both against the longdouble reference.
    The first launch of either side starts with the linear sweep and takes its first sum of h^2 from the plan's table; the split
    side's second launch takes the walking prologue, which must rebuild what sweep B of factor 0 leaves for factor 1 inside the
    fused launch.

    The C API cannot split at the linear / latent boundary itself: mfm_sweep_w alone runs the per-level passes (it is no
    persistent launch), and mfm_sweep_wV with an empty factor range falls back to them as well, so a persistent launch that
    starts with the linear sweep through the WALKING prologue cannot be made from outside. The table's counts are held to account
    by the longdouble reference instead (a user's S2 of the linear sweep is its row count), here and in
    test_one_sweep_against_the_longdouble_reference."""
    _env(monkeypatch, case)
    t = case.table()
    K = 3
    p = R.problem(t, K, 7)
    args_w = (p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"], p["zw"])
    res = []
    for split in (False, True):
        c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
        try:
            _assert_geometry(c, case, s2_form)
            c.set_state(p["w0"], p["w"], p["V"])
            c.set_e(p["e"])
            if split:
                c.sweep_wV(*args_w, 0, 1, p["lam_V"], p["mu_V"], p["zv"][:1])
                c.sweep_V(1, K, p["alpha"], p["lam_V"], p["mu_V"], p["zv"][1:K])
            else:
                c.sweep_wV(*args_w, 0, K, p["lam_V"], p["mu_V"], p["zv"][:K])
            res.append(c.get_state() + (c.get_e(),))
        finally:
            c.close()
    assert res[0][0] == res[1][0]
    for x, y in zip(res[0][1:], res[1][1:]):
        np.testing.assert_array_equal(x, y)
    ref = R.sweep_ref(t.u, t.i, t.n_user_cols, t.gi, p["w"], p["V"], p["e"], p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"], p["zw"],
                      0, K, p["lam_V"], p["mu_V"], p["zv"][:K])
    _check(res[0] + (None,), ref[:3] + (None,), "%s sweep_wV(0, %d)" % (case, K))


def test_row_sharded_sweep_keeps_the_8_byte_list(oracle, capi, monkeypatch):
    """Two ranks as two sessions of one process on one GPU, set up as tests/test_gpu_sharded.py's in-launch exchange test: the
    exchange form of the kernel (XCH) reads the 8-byte list, whatever the run indices are -- the same rows unsharded take 4
    bytes. Three iterations against the unsharded oracle chain, replicas identical."""
    from myfm_amd import _myfm
    from myfm_amd.distributed import shard_cuts

    from .test_gpu_sharded import Lockstep, _config

    world, n, K = 2, 60001, 3
    for k in ("MFM_RES_WGS", "MFM_NO_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MFM_RES_CUS", str(240 // world))
    X, y, shapes = ds.onehot_mf(n, 300, 170, seed=13, sort_by_user=True)
    gi = ds.group_index_from_shapes(shapes)
    c = capi.Context(X, y, rank=K, group_index=gi)
    try:
        info = c.res_info()
    finally:
        c.close()
    assert info["ready"] and info["entry_bytes"] == 4, info
    cuts = shard_cuts(X.indices[X.indptr[:-1]], world)
    ls = Lockstep(world)
    levels = capi.column_levels(X)[0]
    errs, peers, out = [], {}, {}
    meet = threading.Barrier(world)

    def run(rank):
        try:
            lo, hi = cuts[rank], cuts[rank + 1]
            s = _myfm.GibbsSession(K, 0.1, X[lo:hi], [], y[lo:hi], 42, _config(gi), allreduce=ls.callback(rank), n_total_rows=n,
                                   row_offset=lo, main_levels=levels, shard_rank=rank, shard_world=world)
            pending, sum_p, flag_p = s.peer_info()[:3]
            assert pending and sum_p and flag_p
            peers[rank] = (sum_p, flag_p)
            meet.wait()
            s.peer_set(world, rank, [peers[r][0] for r in range(world)], [peers[r][1] for r in range(world)])
            flags, rinfo = s.plan_flags(), dict(zip(capi.Context.RES_INFO, s.res_info()))
            for it in range(3):
                s.step()
            out[rank] = (s.fm.w0, np.asarray(s.fm.w), np.asarray(s.fm.V), flags, rinfo)
        except BaseException as ex:  # noqa
            errs.append(ex)
            ls.bar.abort()
            meet.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join(timeout=300)
    assert not errs, errs
    o = oracle.OracleTrainer(X, y, rank=K, group_index=gi)
    for it in range(3):
        o.step()
    w0, w, V = o.fm()
    for rank in range(world):
        gw0, gw, gV, flags, rinfo = out[rank]
        assert flags & 256 and flags & 8, flags  # persistent sweep, row-sharded
        assert rinfo["ready"] and rinfo["entry_bytes"] == 8 and rinfo["s2_in_sweep_b"] == 0, rinfo
        assert rinfo["n_runs"] + rinfo["G"] < 2 ** 23  # (the width is the form's, not the run indices')
        assert abs(gw0 - w0) < 1e-7
        np.testing.assert_allclose(gw, w, rtol=1e-7, atol=1e-8)
        np.testing.assert_allclose(gV, V, rtol=1e-7, atol=1e-8)
        assert np.array_equal(gV, out[0][2]) and np.array_equal(gw, out[0][1])
