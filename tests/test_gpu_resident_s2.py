"""The persistent sweep's form that takes the user level's sum of h^2 one phase early (k_mf_resident<.., S2B>,
myfm_amd/csrc/mfm_res.hpp): sweep B of a sweep accumulates, into a third wave-private LDS array, the squares of the item
coefficients the NEXT sweep's user draw needs; sweep A no longer does. dv carries the square as a third value per item; the first
sweep of a launch gets its sum from a prologue that walks the slots once.

Only k_mf_resident<512, 4, 1> and its overflow form have the form (more than 16 383 rows in a workgroup), and only where the
third array fits the LDS: every test first asserts through Context.res_info() the variant and the form (`s2_in_sweep_b`) the
case names, then compares numbers -- against resident_ref.sweep_ref (np.longdouble) at the bounds of
tests/test_gpu_resident_edges.py, bit for bit between launches that must rebuild the same sums, against the oracle draw for draw,
and against the per-factor passes at test_resident_latent_sweep's tolerance.
"""
import numpy as np
import pytest

from . import resident_ref as R
from .gibbs_driver import CapiGibbs

pytestmark = pytest.mark.gpu

NT, NW = 512, 8
LDS_LIMIT = 160 * 1024 - 512


def lds_bytes(umax, rl=16, third=False):
    """ResPlan::plan_lds: residual slots in LDS, the per-wave accumulator arrays, utab, the waves' carries and flags"""
    return rl * NT * 8 + (3 if third else 2) * NW * umax * 8 + umax * 16 + NW * 16 + NW * 4 + 64


# the largest accumulator stride at which <512, 4, 1> still takes the form
UMAX_NEW = max(u for u in range(2, 1025) if lds_bytes(u, third=True) <= LDS_LIMIT)
V41 = dict(RV=64, RL=16)


def _case(name, env, make, form, rx=0, **expect):
    return R.Case(name, env, make, expect=dict(V41, RX=rx, s2_in_sweep_b=form, **expect), overflow=rx > 0)


# one workgroup of 20 000 rows: 100 items in its slice, 60 users (the item draw's accumulators reach further than the users');
# the other way round: 300 users, 40 items
ONE_WG = _case("one_wg_20000", R.ONE_CU, R._one_wg(20000, 60, 100, 301), 1)
MORE_USERS = _case("one_wg_20000_users_300_items_40", R.ONE_CU, R._one_wg(20000, 300, 40, 302), 1, umax=301, max_slice_items=40)
# four workgroups of 16 500 rows (150 users of 110 rows each), 400 items: slices of about 100 items, 150 users per workgroup
FOUR_WG = _case("four_wg_16500", R._wgs_env(4), R._many_users(4, 150, 110, 400, 303), 1)
OVERFLOW = _case("one_wg_50000_overflow", R.ONE_CU, R._one_wg(50000, 60, 100, 304), 1, rx=32)
# the LDS boundary: the last stride that takes the form, and the first that does not (users + the pad user = umax)
LDS_LAST = _case("umax_%d_last_with_third_array" % UMAX_NEW, R.ONE_CU, R._one_wg(20000, UMAX_NEW - 1, 100, 305), 1, umax=UMAX_NEW)
LDS_FIRST_OLD = _case("umax_%d_first_without" % (UMAX_NEW + 1), R.ONE_CU, R._one_wg(20000, UMAX_NEW, 100, 306), 0, umax=UMAX_NEW + 1)


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


def _env(monkeypatch, case):
    for k in ("MFM_RES_CUS", "MFM_RES_WGS", "MFM_NO_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _assert_geometry(c, case):
    """the variant and the form the case names -- before any number is compared"""
    info, flags, t = c.res_info(), c.plan_flags(), case.table()
    assert info["ready"], info["why"]
    for k, v in dict(t.want, **case.expect).items():
        assert info[k] == v, (k, info)
    assert info["lds_bytes"] == lds_bytes(info["umax"], info["RL"], third=bool(info["s2_in_sweep_b"])) <= LDS_LIMIT, info
    assert flags["resident"] and flags["resident_overflow"] == case.overflow == (info["RX"] > 0)
    return info


_PROBLEM = {}


def _problem(case, K):
    key = (case.name, K)
    if key not in _PROBLEM:
        _PROBLEM[key] = R.problem(case.table(), K, 7)
    return _PROBLEM[key]


def _context(capi, case, K, p):
    t = case.table()
    c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
    try:
        _assert_geometry(c, case)
        c.set_state(p["w0"], p["w"], p["V"])
        c.set_e(p["e"])
    except BaseException:
        c.close()
        raise
    return c


def _state(c):
    w0, w, V = c.get_state()
    return w0, w, V, c.get_e()


def _check(got, ref, case, what):
    gw0, gw, gV, ge, gq = got
    w, V, e, q = ref
    pairs = dict(w=(gw, w, R.TOL_STATE), V=(gV, V, R.TOL_STATE), e=(ge, e, R.TOL_EQ))
    if q is not None:
        pairs["q"] = (gq, q, R.TOL_EQ)
    print("%s %s: %s" % (case, what, {k: (float(np.abs(g - r).max()), R.worst(g, r, **tol)) for k, (g, r, tol) in pairs.items()}))
    for k, (g, r, tol) in pairs.items():
        np.testing.assert_allclose(g, r.astype(np.float64), err_msg="%s, %s" % (k, what), **tol)


def _sweep_ref(case, p, f_begin, f_end, linear):
    t = case.table()
    return R.sweep_ref(t.u, t.i, t.n_user_cols, t.gi, p["w"], p["V"], p["e"], p["alpha"], p["e_shift"] if linear else 0.0,
                       p["lam_w"], p["mu_w"], p["zw"] if linear else None, f_begin, f_end, p["lam_V"], p["mu_V"],
                       p["zv"][:f_end - f_begin])


def _one_fused_sweep(capi, monkeypatch, case, K, f_begin=0):
    """mfm_sweep_wV(f_begin, K): the linear sweep and the factors in one launch, against the longdouble reference"""
    _env(monkeypatch, case)
    p = _problem(case, K)
    ref = _sweep_ref(case, p, f_begin, K, True)
    c = _context(capi, case, K, p)
    try:
        c.sweep_wV(p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"], p["zw"], f_begin, K, p["lam_V"], p["mu_V"], p["zv"][:K - f_begin])
        assert c.res_info()["e_where"] == "slots"  # (the persistent launch ran and left its residual in slot order)
        got = _state(c) + (c.get_q(),)
    finally:
        c.close()
    assert got[0] == p["w0"]
    _check(got, ref, case, "sweep_wV(%d, %d)" % (f_begin, K))


# K = 1: the third dv value is 0 from the start (no sweep after the next); K = 2: the init kernel's square is the only one ever
# read; K = 3: the item draw's first square is the last; K = 33: more factors than the benchmark's
@pytest.mark.parametrize("K", [1, 2, 3, 33])
def test_one_fused_sweep_against_the_longdouble_reference(capi, monkeypatch, K):
    _one_fused_sweep(capi, monkeypatch, ONE_WG, K)


@pytest.mark.parametrize("case", [MORE_USERS, FOUR_WG, OVERFLOW, LDS_LAST, LDS_FIRST_OLD], ids=repr)
def test_one_fused_sweep_every_table(capi, monkeypatch, case):
    # item slices with more items than users and the other way round (a third array that aliases acc1 / acc2, or is zeroed over
    # the wrong range, fails here), several workgroups, overflow groups, both sides of the LDS boundary
    _one_fused_sweep(capi, monkeypatch, case, 3)


def test_linear_sweep_in_front_of_a_later_factor(capi, monkeypatch):
    # the linear sweep's "next" and "after next" coefficients are V[f_begin] and V[f_begin + 1], not V[0] and V[1]
    _one_fused_sweep(capi, monkeypatch, ONE_WG, 3, f_begin=1)


@pytest.mark.parametrize("case,f0,f1", [(ONE_WG, 1, 3), (ONE_WG, 2, 3), (FOUR_WG, 1, 3), (OVERFLOW, 1, 3)],
                         ids=lambda v: repr(v))
def test_sweep_V_alone_from_a_later_factor(capi, monkeypatch, case, f0, f1):
    # no linear sweep, f_begin > 0: the prologue's first coefficient is V[f0], not 1
    _env(monkeypatch, case)
    K = 3
    p = _problem(case, K)
    ref = _sweep_ref(case, p, f0, f1, False)
    c = _context(capi, case, K, p)
    try:
        c.sweep_V(f0, f1, p["alpha"], p["lam_V"], p["mu_V"], p["zv"][:f1 - f0])
        got = _state(c) + (c.get_q(),)
    finally:
        c.close()
    _check(got, ref, case, "sweep_V(%d, %d)" % (f0, f1))


@pytest.mark.parametrize("case", [ONE_WG, FOUR_WG, OVERFLOW, LDS_FIRST_OLD], ids=repr)
def test_split_launches_bit_for_bit(capi, monkeypatch, case):
    # mfm_sweep_V(0, 1) then mfm_sweep_V(1, K) == mfm_sweep_V(0, K): the second launch's prologue rebuilds exactly the sum that
    # sweep B of factor 0 leaves for factor 1 inside the single launch
    _env(monkeypatch, case)
    K = 4
    p = _problem(case, K)
    res = []
    for cuts in ([0, K], [0, 1, K], [0, 2, 3, K]):
        c = _context(capi, case, K, p)
        try:
            for f0, f1 in zip(cuts[:-1], cuts[1:]):
                c.sweep_V(f0, f1, p["alpha"], p["lam_V"], p["mu_V"], p["zv"][f0:f1])
            res.append(_state(c))
        finally:
            c.close()
    for other in res[1:]:
        assert res[0][0] == other[0]
        for x, y in zip(res[0][1:], other[1:]):
            np.testing.assert_array_equal(x, y)
    _check(res[0] + (None,), _sweep_ref(case, p, 0, K, False)[:3] + (None,), case, "sweep_V(0, %d)" % K)


@pytest.mark.parametrize("case", [ONE_WG, MORE_USERS, FOUR_WG, OVERFLOW, LDS_LAST], ids=repr)
def test_three_iterations_against_the_oracle_and_a_rerun(oracle, capi, monkeypatch, case):
    _env(monkeypatch, case)
    t = case.table()
    n, K = t.n, 3
    chains = []
    for rep in range(2):
        o = oracle.OracleTrainer(t.X, t.y, rank=K, group_index=t.gi)
        c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
        try:
            _assert_geometry(c, case)
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


def test_an_existing_512_user_table_keeps_the_two_array_form(capi, monkeypatch):
    case = R.CASE["users_512_one_wg"]
    _env(monkeypatch, case)
    t = case.table()
    c = capi.Context(t.X, t.y, rank=case.K, group_index=t.gi)
    try:
        info = c.res_info()
    finally:
        c.close()
    assert info["ready"] and info["umax"] == 513 and info["s2_in_sweep_b"] == 0, info
    assert info["lds_bytes"] == lds_bytes(513, info["RL"]) and lds_bytes(513, 16, third=True) > LDS_LIMIT


def test_resident_chain_equals_the_per_factor_passes(oracle, capi, monkeypatch):
    case = FOUR_WG
    t = case.table()
    n, K = t.n, 3
    out = []
    for resident in (True, False):
        _env(monkeypatch, case)
        if not resident:
            monkeypatch.setenv("MFM_NO_RESIDENT", "1")
        o = oracle.OracleTrainer(t.X, t.y, rank=K, group_index=t.gi)
        c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
        try:
            if resident:
                _assert_geometry(c, case)
            else:
                assert not c.plan_flags()["resident"] and c.plan_flags()["mf"]
            c.set_state(*o.fm())
            c.set_e(o.e(n))
            drv = CapiGibbs(c, o.clone(), n, t.gi)
            for it in range(3):
                drv.step()
            out.append(c.get_state()[2])
        finally:
            c.close()
    np.testing.assert_allclose(out[1], out[0], rtol=1e-9, atol=1e-10)
