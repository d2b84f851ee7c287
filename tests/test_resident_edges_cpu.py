"""The longdouble reference of the persistent sweep's layout-edge tests (tests/resident_ref.py) against the float64 oracle, on every
case of tests/test_gpu_resident_edges.py -- no GPU.

Two things are established here before any device number is looked at: the reference function computes what the oracle's
update_w0 shift + update_w + update_V_factor compute (it is written from the kernel header, the oracle from FMTrainer.hpp), and
the float64 oracle, with its sequential sums, sits within ONE TENTH of the project's single-sweep bound of the extended-precision
result on these shapes. The other nine tenths are what the device's different summation order may use.
"""
import numpy as np
import pytest

from . import resident_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_oracle_within_a_tenth_of_the_bound_of_the_longdouble_reference(oracle, case):
    t = case.table()
    p = R.problem(t, case.K, 7)
    o = oracle.OracleTrainer(t.X, t.y, rank=case.K, group_index=t.gi)
    assert o.D == t.D and o.G == 2
    o.set_fm(p["w0"], p["w"], p["V"])
    o.set_e(p["e"] + p["e_shift"])  # (update_w0's e += w0' - w0, FMTrainer.hpp:226)
    o.set_hyper(p["alpha"], p["mu_w"], p["lam_w"], p["mu_V"], p["lam_V"])
    # the variates: the oracle draws them itself, so the reference is run on what its generator is about to hand out
    z = o.clone().rng_sample_normals(t.D * (1 + case.K)).reshape(1 + case.K, t.D)
    w, V, e, q = R.sweep_ref(t.u, t.i, t.n_user_cols, t.gi, p["w"], p["V"], p["e"], p["alpha"], p["e_shift"], p["lam_w"], p["mu_w"],
                             z[0], 0, case.K, p["lam_V"], p["mu_V"], z[1:])
    o.substep(4)  # update_w
    for f in range(case.K):
        o.update_V_factor(f)
    ow0, ow, oV = o.fm()
    tenth = lambda tol: dict(rtol=tol["rtol"] / 10, atol=tol["atol"] / 10)
    np.testing.assert_allclose(ow, w.astype(np.float64), **tenth(R.TOL_STATE))
    np.testing.assert_allclose(oV, V.astype(np.float64), **tenth(R.TOL_STATE))
    np.testing.assert_allclose(o.e(t.n), e.astype(np.float64), **tenth(R.TOL_EQ))
    np.testing.assert_allclose(o.q(t.n), q.astype(np.float64), **tenth(R.TOL_EQ))


@pytest.mark.parametrize("case", R.CASES + R.SCORE_CASES, ids=repr)
def test_tables_state_their_geometry(case):
    # the designs are what the cases say: user-sorted, unit-valued, two entries per row, every column occurs, and no workgroup of
    # an accepted case is beyond a capacity the planner enforces
    t = case.table()
    assert np.all(np.diff(t.u) >= 0) and t.u.max() < t.n_user_cols <= t.i.min()
    assert np.unique(t.u).shape[0] == t.n_user_cols and np.unique(t.i).shape[0] == t.D - t.n_user_cols
    assert t.X.shape == (t.n, t.D) and t.X.nnz == 2 * t.n and np.all(t.X.data == 1.0)
    assert t.n <= 82000
    if case.why is None and "ng" not in case.expect:
        slots = case.expect["RV"] + case.expect["RL"] + case.expect["RX"]
        assert t.want["max_wg_users"] <= R.NT and -(-t.n // t.want["G"]) <= R.NT * slots - 1


def test_score_reference_is_the_plain_sum():
    t = R.CASE["tiny_7"].table()
    p = R.problem(t, 3, 7)
    e = R.score_ref(t.u, t.i, p["w0"], p["w"], p["V"], t.y)
    want = [p["w0"] + p["w"][a] + p["w"][b] + float(np.dot(p["V"][a], p["V"][b])) - yy for a, b, yy in zip(t.u, t.i, t.y)]
    np.testing.assert_allclose(e.astype(np.float64), want, rtol=1e-14, atol=1e-15)


def test_all_cus_case_follows_the_planners_cut_rule():
    # 600 users of 50 rows on 256 workgroups: the boundary nearest to g N / 256 gives 2 or 3 users per workgroup
    per = R.planner_cuts(np.full(600, 50), R.N_CU)
    assert per.shape[0] == R.N_CU and per.sum() == 600 and set(per) == {2, 3}
    assert R.CASE["all_cus_at_the_barrier"].table().want["max_wg_users"] == 3


def test_config3_mix_has_short_runs():
    # config 3's mean (workgroup, item) run is 4.9 slots; the GPU tests hold res_info()'s n_runs to this table's count
    t = R.CASE["config3_mix_x4"].table()
    assert 4.0 < t.n / t.want["n_runs"] < 6.0 and 1900 < t.want["n_items"] <= 2000
