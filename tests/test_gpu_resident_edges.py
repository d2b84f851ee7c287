"""The persistent sweep (k_mf_resident, myfm_amd/csrc/mfm_res.hpp) and the slot-order scorer (k_res_score) on every structural edge
of the slot layout, at tables of at most 82 k rows.

The chain tests of tests/test_gpu_capi.py run the kernel on one kind of table (about 8 users per workgroup, item runs dozens of
slots long, 20 to 40 workgroups, never on a capacity boundary); config 3's geometry -- uid >= 256, a 4.9-slot mean run, 256
workgroups on 8 XCDs, K = 32 -- is reached only by the full-size tests. Here every edge has a small table built for it
(tests/resident_ref.py: explicit per-workgroup user and item assignments), and every test first PROVES through
Context.res_info() that the planner produced the geometry the case names. Then:
  (a) one mfm_sweep_wV from a set state with given variates against the np.longdouble reference (resident_ref.sweep_ref): w, V,
      the residual and q, at the project's single-sweep bound (rtol 1e-9 / atol 1e-11 on w, V; rtol 1e-8 / atol 1e-9 on e, q),
      both with the host planner holding the device planner to account (MFM_PLAN_CHECK) and without it (what users run);
      tests/test_resident_edges_cpu.py shows that the float64 oracle uses at most a tenth of that bound on the same cases;
  (b) three iterations of mfm_sweep_wV + update_e against the oracle draw for draw, (c) a second context bit for bit,
  (d) the sweep ran as the persistent launch exactly when the planner took the table.
Refused tables (planner refusals, decided on the host before any launch) must say why and walk the same chain on the
per-factor passes.

MYFM_RESIDENT_EDGES_REPORT=<path>: the largest device error of every case of (a) is written there (profiles/resident_edges_errors.txt).
"""
import os

import numpy as np
import pytest

from . import resident_ref as R
from .gibbs_driver import CapiGibbs

pytestmark = pytest.mark.gpu


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


ERRORS = []  # (case, mode, {quantity: (largest |error|, largest error as a fraction of the bound)})


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("MYFM_RESIDENT_EDGES_REPORT")
    if not path or not ERRORS:
        return
    with open(path, "w") as fp:
        fp.write("# one mfm_sweep_wV against the np.longdouble reference (tests/test_gpu_resident_edges.py, check (a)), MI355X.\n"
                 "# per quantity: largest |device - reference|, and the largest error as a fraction of the bound\n"
                 "# (w, V: atol 1e-11 + rtol 1e-9 |x|; e, q: atol 1e-9 + rtol 1e-8 |x|; the test requires <= 1)\n")
        fp.write("%-34s %-9s %s\n" % ("case", "planner", "".join("%-22s" % k for k in ("w", "V", "e", "q"))))
        for name, mode, err in ERRORS:
            fp.write("%-34s %-9s %s\n" % (name, mode, "".join("%.2e (%.1e)     " % err[k] for k in ("w", "V", "e", "q"))))


def _env(monkeypatch, case, checked=None):
    for k in ("MFM_RES_CUS", "MFM_RES_WGS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if checked is True:
        monkeypatch.setenv("MFM_PLAN_CHECK", "1")
    elif checked is False:
        monkeypatch.delenv("MFM_PLAN_CHECK", raising=False)


def _assert_geometry(c, case):
    """the case reached the edge it names -- before any number is compared"""
    info, flags, t = c.res_info(), c.plan_flags(), case.table()
    if case.why is not None:
        assert not info["ready"] and info["why"].startswith(case.why), info
        assert not flags["resident"]
        return info
    assert info["ready"], info["why"]
    for k, v in dict(t.want, **case.expect).items():
        assert info[k] == v, (k, info)
    assert flags["resident"] and flags["resident_overflow"] == case.overflow == (info["RX"] > 0)
    return info


def _timing_classes(c, drv):
    c.timing_enable(True)
    c.timing_reset()
    c.sweep_V(0, 1, drv.alpha, drv.lam_V, drv.mu_V, np.zeros(c.D))
    names = set(c.timing())
    c.timing_enable(False)
    return names


@pytest.mark.parametrize("checked", [True, False], ids=["checked", "device_planner_alone"])
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_one_sweep_against_the_longdouble_reference(capi, monkeypatch, case, checked):
    _env(monkeypatch, case, checked)
    t = case.table()
    p, (w, V, e, q) = R.reference(case)
    c = capi.Context(t.X, t.y, rank=case.K, group_index=t.gi)
    try:
        info = _assert_geometry(c, case)
        c.set_state(p["w0"], p["w"], p["V"])
        c.set_e(p["e"])
        assert c.res_info()["e_where"] == "rows"
        c.sweep_wV(p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"], p["zw"], 0, case.K, p["lam_V"], p["mu_V"], p["zv"])
        if info["ready"]:
            assert c.res_info()["e_where"] == "slots"  # (the launch left its residual in slot order)
        gw0, gw, gV = c.get_state()
        ge, gq = c.get_e(), c.get_q()
    finally:
        c.close()
    assert gw0 == p["w0"]
    got = dict(w=(gw, w, R.TOL_STATE), V=(gV, V, R.TOL_STATE), e=(ge, e, R.TOL_EQ), q=(gq, q, R.TOL_EQ))
    err = {k: (float(np.abs(g - r).max()), R.worst(g, r, **tol)) for k, (g, r, tol) in got.items()}
    print("%s %s: %s" % (case, "checked" if checked else "device planner alone", err))
    ERRORS.append((case.name, "checked" if checked else "device", err))
    for k, (g, r, tol) in got.items():
        np.testing.assert_allclose(g, r.astype(np.float64), err_msg=k, **tol)


CHAINS = [(c, False) for c in R.CASES] + [(c, True) for c in R.CASES if c.overflow]


@pytest.mark.parametrize("case,recomputable", CHAINS, ids=["%s%s" % (c, "-residual_not_stored" if r else "") for c, r in CHAINS])
def test_three_iterations_against_the_oracle_and_a_rerun(oracle, capi, monkeypatch, case, recomputable):
    _env(monkeypatch, case)
    t = case.table()
    n, K = t.n, case.K
    chains = []
    for rep in range(2):
        o = oracle.OracleTrainer(t.X, t.y, rank=K, group_index=t.gi)
        c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
        try:
            _assert_geometry(c, case)
            c.set_state(*o.fm())
            c.set_e(o.e(n))
            if recomputable:
                c.set_residual_policy(True)
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
            assert ("sweep_V_resident" in _timing_classes(c, drv)) == (case.why is None)
        finally:
            c.close()
    assert chains[0][0] == chains[1][0]
    for a, b in zip(chains[0][1:], chains[1][1:]):
        np.testing.assert_array_equal(a, b)


def test_all_cus_case_uses_every_cu_of_the_device(capi, monkeypatch):
    # the production workgroup count: the case is built for 256 workgroups, which must be the CUs of the device under test
    import torch

    case = R.CASE["all_cus_at_the_barrier"]
    _env(monkeypatch, case)
    t = case.table()
    c = capi.Context(t.X, t.y, rank=case.K, group_index=t.gi)
    try:
        info = _assert_geometry(c, case)
    finally:
        c.close()
    assert info["G"] == min(torch.cuda.get_device_properties(0).multi_processor_count, t.n_user_cols) == R.N_CU
    assert info["max_wg_users"] == 3 and t.n // info["G"] == 117


# ---- the slot-order scorer ---------------------------------------------------------------------------------------------------
def _score_and_sweep(capi, t, K, in_slots, seed):
    """update_e_regression against the longdouble sum, its reductions, which scorer ran; then one fused sweep from the residual
    as the scorer left it against the same sweep from the row-ordered one, bit for bit. Returns res_info() after finalize."""
    c = capi.Context(t.X, t.y, rank=K, group_index=t.gi)
    try:
        info = c.res_info()
        p = R.problem(t, K, seed)
        c.set_state(p["w0"], p["w"], p["V"])
        c.update_e_regression()
        assert c.res_info()["e_where"] == ("slots_with_sums" if in_slots else "rows")
        want = R.score_ref(t.u, t.i, p["w0"], p["w"], p["V"], t.y)
        s, s2 = c.reduce_e()
        np.testing.assert_allclose(c.get_e(), want.astype(np.float64), rtol=1e-12, atol=1e-12)
        assert abs(s - float(want.sum())) < 1e-8 * t.n and abs(s2 - float((want * want).sum())) < 1e-8 * t.n
        args = (p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"], p["zw"], 0, K, p["lam_V"], p["mu_V"], p["zv"])
        c.update_e_regression()  # the residual where the scorer leaves it
        c.sweep_wV(*args)
        a = c.get_state() + (c.get_e(),)
        c.set_state(p["w0"], p["w"], p["V"])
        c.update_e_regression()
        c.get_e()  # row order
        assert c.res_info()["e_where"] == "rows"
        c.sweep_wV(*args)
        b = c.get_state() + (c.get_e(),)
    finally:
        c.close()
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)
    return info


@pytest.mark.parametrize("case", R.SCORE_CASES, ids=repr)
def test_slot_order_scorer_every_instantiation(capi, monkeypatch, case):
    # k_res_score<512, NG, 16> for NG = R / 16 = 1, 2, 5 (on chip) and 6 .. 10 (with overflow slots), one workgroup each
    _env(monkeypatch, case)
    t = case.table()
    info = _score_and_sweep(capi, t, case.K, True, 11)
    assert info["ready"] and info["G"] == 1, info
    assert (info["RV"] + info["RL"] + info["RX"]) // 16 == case.expect["ng"]
    assert info["n_runs"] == t.want["n_runs"] and info["max_wg_users"] == t.want["max_wg_users"]


@pytest.mark.parametrize("K", [0, 1, 15, 16, 17, 31, 32, 33])
@pytest.mark.parametrize("name", ["users_512_one_wg", "all_heads_x4"])
def test_slot_order_scorer_ranks(capi, monkeypatch, name, K):
    # KS = (K + 1) & ~1 <= 32 is the scorer's limit: K = 32 is the last rank it takes; K = 33 and K = 0 are scored in row order
    case = R.CASE[name]
    _env(monkeypatch, case)
    t = case.table()
    info = _score_and_sweep(capi, t, K, 1 <= K <= 32, 13)
    assert info["ready"], info["why"]  # (the layout does not depend on the rank: K = 0 has it too, and no sweep to run on it)
    for k, v in dict(t.want, **case.expect).items():
        assert info[k] == v, (k, info)
