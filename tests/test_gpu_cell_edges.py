"""The cell path (k_cell_pass, k_cell_score and the planners of myfm_amd/csrc/mfm_cell.hip) on every structural edge of its layout,
at tables of at most 82 k rows -- most of them a few hundred.

tests/test_gpu_cell.py runs the path on tuple_design shapes of 30 k - 150 k rows with users and items drawn uniformly: no chunk
length, run length or stream cardinality is chosen there. Here every edge has a small design built for it (tests/cell_ref.py:
explicit index arrays and column counts), and every test first PROVES through Context.cell_info() that the planner produced the
geometry the case names (cell_ref.plan restates the planner). Then:
  (a) one mfm_sweep_w, one mfm_sweep_V(0, K) and one mfm_update_e_regression, each from a set state with given variates, against
      the np.longdouble reference (the sequential sweep over the expanded flat design) at the project's single-call bounds
      (V 1e-9 / 1e-11, w 1e-10 / 1e-12, e and q after a sweep 1e-8 / 1e-9, the scorer's e 1e-10 / 1e-10), both with the host
      planner holding the device planner to account (MFM_PLAN_CHECK) and without it (what users run);
      tests/test_cell_edges_cpu.py shows that the float64 oracle uses at most a tenth of those bounds on the same cases;
  (b) three Gibbs iterations against the oracle and against a MFM_NO_CELL context of the same library at 1e-7, and a second
      context from the same state bit for bit;
  (c) the scorer at every tile width FB and the ranks that give every tail K mod FB, at both item index widths.
Refused designs (decided on the host before any launch) must say why and walk the same checks on the generic path.

MYFM_CELL_EDGES_REPORT=<path>: the largest device error of every case of (a) and (c) is written there
(profiles/cell_edges_errors.txt).
"""
import os
import time

import numpy as np
import pytest

from . import cell_ref as R
from .gibbs_driver import CapiGibbs

pytestmark = pytest.mark.gpu

GEOMETRY = ("G", "umax", "item32", "n_streams", "n_fields", "N", "Npad", "max_steps", "chunk_max", "chunk_min", "chunks_empty",
            "split_mask", "score_fb", "streams", "fields")


@pytest.fixture(scope="module")
def capi():
    from myfm_amd import _capi

    if _capi.lib().mfm_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _capi


ERRORS = []  # (case, mode, {quantity: (largest |error|, largest error as a fraction of the bound)})
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("MYFM_CELL_EDGES_REPORT")
    if not path or not ERRORS:
        return
    keys = list(R.QUANTITIES)
    with open(path, "w") as fp:
        fp.write("# one mfm_sweep_w, one mfm_sweep_V(0, K), one mfm_update_e_regression against the np.longdouble reference\n"
                 "# (tests/test_gpu_cell_edges.py), MI355X. Per quantity: largest |device - reference| and, in brackets, the largest\n"
                 "# error as a fraction of the bound (w 1e-10 / 1e-12; V 1e-9 / 1e-11; e_w, e_V, q 1e-8 / 1e-9; score 1e-10 / 1e-10;\n"
                 "# the test requires <= 1). planner: checked = MFM_PLAN_CHECK, device = the device planner alone, generic = the design\n"
                 "# was refused and ran on the generic path.\n")
        fp.write("%-36s %-5s %-8s %s\n" % ("case", "K", "planner", "".join("%-21s" % k for k in keys)))
        top = 0.0
        for name, K, mode, err in ERRORS:
            fp.write("%-36s %-5d %-8s %s\n" % (name, K, mode, "".join(("%.2e (%.1e)    " % err[k]) if k in err else "%-21s" % "-" for k in keys)))
            top = max([top] + [v[1] for v in err.values()])
        fp.write("# largest fraction of a bound: %.3g; wall time of the module up to here: %.1f s\n" % (top, time.time() - T0))


def _env(monkeypatch, case, checked=None):
    for k in ("MFM_NO_CELL", "MFM_NO_CELL_W", "MFM_CELL_GROUPS", "MFM_CELL_MIN_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if checked is True:
        monkeypatch.setenv("MFM_PLAN_CHECK", "1")
    elif checked is False:
        monkeypatch.delenv("MFM_PLAN_CHECK", raising=False)


def _context(capi, case, K=None):
    d = case.design()
    return capi.Context(d.main, d.y, d.blocks, rank=case.K if K is None else K, group_index=d.gi)


def _assert_geometry(c, case):
    """the case reached the edge it names -- before any number is compared"""
    info, flags, want = c.cell_info(), c.plan_flags(), case.want()
    if case.why is not None:
        assert not info["ready"] and info["why"].startswith(case.why), info
        assert not flags["cell"]
        return info
    assert info["ready"] and info["why"] == "", info["why"]
    for k in GEOMETRY:
        assert info[k] == want[k], (k, info[k], want[k])
    for k, v in case.expect.items():
        assert info[k] == v, (k, info[k], v)
    assert flags["cell"]
    return info


def _record_and_assert(case, K, mode, got):
    err = {k: (float(np.abs(g - r).max()), R.worst(g, r, **R.QUANTITIES[k])) for k, (g, r) in got.items()}
    print("%s %s: %s" % (case, mode, err))
    ERRORS.append((case.name, K, mode, err))
    for k, (g, r) in got.items():
        np.testing.assert_allclose(g, r.astype(np.float64), err_msg=k, **R.QUANTITIES[k])


@pytest.mark.parametrize("checked", [True, False], ids=["checked", "device_planner_alone"])
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_one_call_each_against_the_longdouble_reference(capi, monkeypatch, case, checked):
    _env(monkeypatch, case, checked)
    p, ref = R.reference(case)
    c = _context(capi, case)
    try:
        _assert_geometry(c, case)
        c.set_state(p["w0"], p["w"], p["V"])
        c.set_e(p["e"])
        c.sweep_w(p["alpha"], p["lam_w"], p["mu_w"], p["zw"])
        gw0, gw, gV = c.get_state()
        assert gw0 == p["w0"] and np.array_equal(gV, p["V"])
        got = dict(w=(gw, ref["w"]), e_w=(c.get_e(), ref["e_w"]))
        c.set_state(p["w0"], p["w"], p["V"])
        c.set_e(p["e"])
        c.sweep_V(0, case.K, p["alpha"], p["lam_V"], p["mu_V"], p["zv"])
        _, gw, gV = c.get_state()
        assert np.array_equal(gw, p["w"])
        got.update(V=(gV, ref["V"]), e_V=(c.get_e(), ref["e_V"]), q=(c.get_q(), ref["q"]))
        c.set_state(p["w0"], p["w"], p["V"])
        c.update_e_regression()
        got.update(score=(c.get_e(), ref["score"]))
    finally:
        c.close()
    _record_and_assert(case, case.K, "generic" if case.why else ("checked" if checked else "device"), got)


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_three_iterations_against_the_oracle_the_generic_path_and_a_rerun(oracle, capi, monkeypatch, case):
    _env(monkeypatch, case)
    d = case.design()
    n, K = d.n, case.K
    o = oracle.OracleTrainer(d.main, d.y, d.blocks, rank=K, group_index=d.gi)
    o0 = o.clone()
    ctxs = []
    try:
        for rep in range(3):  # the cell path, the cell path again from the same state, the generic path of the same library
            if rep == 2:
                monkeypatch.setenv("MFM_NO_CELL", "1")
            c = _context(capi, case)
            ctxs.append(c)
            if rep < 2:
                _assert_geometry(c, case)
            else:
                assert not c.plan_flags()["cell"]
            c.set_state(*o0.fm())
            c.set_e(o0.e(n))
        drv = [CapiGibbs(c, o0.clone(), n, d.gi) for c in ctxs]
        for it in range(3):
            o.step()
            for x in drv:
                x.step()
            w0, w, V = o.fm()
            gw0, gw, gV = ctxs[0].get_state()
            np.testing.assert_allclose(gV, V, rtol=1e-7, atol=1e-7, err_msg="V, iteration %d" % it)
            np.testing.assert_allclose(gw, w, rtol=1e-7, atol=1e-7, err_msg="w, iteration %d" % it)
            np.testing.assert_allclose(gw0, w0, rtol=1e-7, atol=1e-7)
            hw0, hw, hV = ctxs[2].get_state()
            np.testing.assert_allclose(gV, hV, rtol=1e-7, atol=1e-7, err_msg="V against the generic path, iteration %d" % it)
            np.testing.assert_allclose(gw, hw, rtol=1e-7, atol=1e-7, err_msg="w against the generic path, iteration %d" % it)
        np.testing.assert_allclose(ctxs[0].get_e(), o.e(n), rtol=1e-7, atol=1e-7)
        np.testing.assert_allclose(ctxs[0].get_e(), ctxs[2].get_e(), rtol=1e-7, atol=1e-7)
        # every sum has a fixed order: the second context is bit-identical
        a, b = ctxs[0].get_state() + (ctxs[0].get_e(),), ctxs[1].get_state() + (ctxs[1].get_e(),)
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            np.testing.assert_array_equal(x, y)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("K", R.SCORE_RANKS)
@pytest.mark.parametrize("case", R.SCORE_CASES, ids=repr)
def test_scorer_every_tile_width_and_tail(capi, monkeypatch, case, K):
    # FB factors per pass with the last pass nf = K mod FB wide (K = 5: FB 4 -> 1, FB 2 -> 1; K = 33: KS = 34 > K)
    _env(monkeypatch, case)
    d = case.design()
    p = R.problem(d, K, 11)
    c = _context(capi, case, K)
    try:
        info = _assert_geometry(c, case)
        assert info["score_fb"] == case.expect["score_fb"] and info["item32"] == case.expect["item32"]
        c.set_state(p["w0"], p["w"], p["V"])
        c.update_e_regression()
        e = c.get_e()
        c.update_e_regression()  # (a second call finds its tables allocated: the same numbers)
        assert np.array_equal(e, c.get_e())
    finally:
        c.close()
    _record_and_assert(case, K, "device", dict(score=(e, R.score_ref(d, p["w0"], p["w"], p["V"], d.y))))
