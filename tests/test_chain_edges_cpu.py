"""Every overflow path and step edge of the streamed block chain (csrc/mfm_chain_stream.hpp, k_cs_stream), without a GPU: for the designs
of tests/chain_designs.py `mfm_cs_plan_probe` builds the plan as the launch takes it, and the test asserts on the plan record that each of
the kernel's paths is reached by one of the listed (Cg, Lw, NB) -- and which of them the complement configuration stays off --, then that
the host emulation of the launch's data flow (cs_emulate, csrc/mfm_chain_plan.hpp) gives the sequential sweep's numbers.

The emulation's values are 0.01-0.024: with the kernel tests' 0.2-1.0 the toy map expands round-off on the heavy columns, and the two
summation orders alone differ by 1 to 2 (measured at (4, 2, 2): test_emulation_goes_blind_with_large_values). With the small values
the difference is 1e-15; a record routed to the wrong slot, ring position or step moves a coefficient by about 1e-2. The bound 1e-10
stands between them."""
import numpy as np
import pytest

from . import chain_designs as cd

EMU_TOL = 1e-10


@pytest.fixture(scope="module")
def edges_small():
    return cd.edges(small=True)


@pytest.fixture(scope="module")
def edges_plans(edges_small):
    return {cfg: cd.probe(edges_small, *cfg) for cfg in cd.EDGES_CONFIGS}


def test_every_column_of_the_designs_is_its_own_level():
    from myfm_amd import _capi

    level, n = _capi.column_levels(cd.edges())
    assert n == 41 and list(level) == [0, 0, 0, 0] + list(range(1, 41))
    for k in cd.SHORT_NS:
        level, n = _capi.column_levels(cd.short(k))
        assert n == k and list(level) == list(range(k))
    level, n = _capi.column_levels(cd.tiny())
    assert n == 5 and list(level) == list(range(5))


@pytest.mark.parametrize("cfg", cd.EDGES_CONFIGS)
def test_edges_emulation_matches_the_sequential_sweep(edges_plans, cfg):
    rec, hot, built, diff = edges_plans[cfg]
    print(cfg, rec, "emulation difference %.3g" % diff)
    assert built and (rec["Cg"], rec["Lw"], rec["NB"], rec["RD"]) == cfg + (cd.RD,)
    assert rec["n_cols"] == 44 and rec["n_steps"] == -(-44 // cfg[0])
    assert rec["n_cold"] + rec["n_hot"] == 8290 and sum(rec["hot_rounds"]) == 44 and int(hot.sum()) == rec["n_hot"]
    assert rec["lds_bytes"] <= cd.LDS_MAX
    assert diff < EMU_TOL, diff


def test_edges_plan_records(edges_plans):
    # the planner's numbers for this design (RD = 2): a change of the plan that moves them moves what the kernel tests reach
    rec = edges_plans[(4, 2, 2)][0]
    want = dict(n_steps=11, n_slots=1581, max_enter=908, max_exit=1017, max_cold_sr=500, max_enter_sr=602, max_exit_sr=1017, lds_bytes=144948,
                n_cols_no_hot=3, max_hot_col=564)
    assert {k: rec[k] for k in want} == want, rec
    assert rec["hot_rounds"] == [3, 23, 2, 2, 2, 2, 2, 2, 2, 4], rec["hot_rounds"]
    assert edges_plans[(4, 3, 1)][0]["max_cold_sr"] == 580
    rec = edges_plans[(2, 4, 2)][0]
    assert (rec["n_steps"], rec["n_slots"], rec["max_enter"], rec["max_exit"], rec["lds_bytes"]) == (22, 1073, 560, 560, 88852), rec
    rec = edges_plans[(3, 3, 2)][0]
    assert (rec["n_steps"], rec["lds_bytes"]) == (15, 102676), rec
    rec = edges_plans[(1, 7, 2)][0]
    assert (rec["n_steps"], rec["n_slots"], rec["lds_bytes"]) == (44, 564, 46524), rec


def test_every_walker_path_is_reached(edges_plans):
    rec, hot, _, _ = edges_plans[(4, 2, 2)]
    hot = list(hot)
    # no hot entry: the three columns of private rows; column 0 has the spine only
    assert hot[:4] == [4, 0, 0, 0] and rec["n_cols_no_hot"] == 3 and rec["hot_rounds"][0] == 3
    # the group columns: exactly 64, 65 and 512 hot entries among them (a full last round, one entry in the last round, all eight
    # register rounds full), every round count 1..8, and two pairs of columns beyond the registers
    for g, h in enumerate(cd.EDGES_HOT):
        assert hot[6 + 3 * g] == h and hot[7 + 3 * g] == h, (g, hot)
    assert {64, 65, 512, 513} <= set(hot)
    assert all(rec["hot_rounds"][nr] > 0 for nr in range(1, 9)), rec["hot_rounds"]
    assert rec["hot_rounds"][9] == 4 and rec["max_hot_col"] == 564 and rec["max_hot_col"] <= 1024


def test_every_helper_and_range_path_is_reached_and_the_complement_stays_off_them(edges_plans):
    for path, (field, thr) in cd.PATHS.items():
        reached = [cfg for cfg in cd.EDGES_CONFIGS if edges_plans[cfg][0][field] > thr]
        print(path, field, ">", thr, "at", reached, {cfg: edges_plans[cfg][0][field] for cfg in cd.EDGES_CONFIGS})
        assert (4, 2, 2) in reached, (path, edges_plans[(4, 2, 2)][0])
    # one range: the most cold entries of a (step, range) there are
    assert edges_plans[(4, 3, 1)][0]["max_cold_sr"] > 384
    # The complement: 32 ranges keep the cold entries of every (step, range) inside the first tiles (130 <= 384), so the S tile loop and
    # the U tail loop do not run. What a step moves as a whole (walker, X, Y) does not depend on the ranges. The entering / leaving rows
    # of a (step, range) are 130 there as well -- two rows past the first 128, not below it: the complement of those two paths is
    # short(4) and short(5) at (1, 2, 32), at most 8 rows (test_short_runs_emulate_exactly).
    rec = edges_plans[(4, 3, 32)][0]
    assert (rec["max_cold_sr"], rec["max_enter_sr"], rec["max_exit_sr"]) == (130, 130, 130), rec
    assert rec["max_cold_sr"] <= 384


def test_window_beyond_the_lds_is_not_built(edges_small):
    rec, hot, built, diff = cd.probe(edges_small, *cd.EDGES_REFUSED)
    assert not built and rec["lds_bytes"] == 169012 and rec["lds_bytes"] > cd.LDS_MAX, rec


@pytest.mark.parametrize("n", cd.SHORT_NS)
@pytest.mark.parametrize("cfg", cd.SHORT_CONFIGS)
def test_short_runs_emulate_exactly(n, cfg):
    cg, lw, nb = cfg
    B = cd.short(n, small=True)
    rec, hot, built, diff = cd.probe(B, cg, lw, nb)
    print(n, cfg, rec, "emulation difference %.3g" % diff)
    assert built and rec["n_cols"] == n and rec["n_steps"] == -(-n // cg) and rec["n_cold"] + rec["n_hot"] == B.nnz
    assert diff < EMU_TOL, diff
    if n == 2:
        assert list(hot) == [702, 702] and rec["hot_rounds"][9] == 2  # both columns beyond the registers
    if cfg == (1, 2, 32):  # every per-range path stays inside its first tiles / rows; with n = 4, 5 and 9 the per-step ones as well
        assert rec["max_cold_sr"] <= 384 and rec["max_enter_sr"] <= 128 and rec["max_exit_sr"] <= 128, rec
        assert n < 4 or (rec["max_enter"] <= 384 and rec["max_exit"] <= 512 and rec["max_hot_col"] <= 512), rec


def test_short_runs_reach_the_step_edges():
    steps = {(n, cfg): -(-n // cfg[0]) for n in cd.SHORT_NS for cfg in cd.SHORT_CONFIGS}
    assert any(s == 1 for s in steps.values())                                        # one step
    assert any(1 < s < cfg[1] for (n, cfg), s in steps.items())                       # fewer steps than the window
    assert any(s <= cd.RD for s in steps.values())                                    # no slot comes back
    assert any(n % 2 == 1 and cfg[0] == 1 for (n, cfg) in steps)                      # an odd column count, column by column
    assert any(n % cfg[0] != 0 and n > cfg[0] for (n, cfg) in steps)                  # a partial last step after full ones
    assert any(n < cfg[0] for (n, cfg) in steps)                                      # a partial ONLY step


@pytest.mark.parametrize("n_rows", cd.TINY_ROWS)
def test_tiny_block_has_empty_ranges(n_rows):
    # 40 rows: one or two rows a range, most (step, range) lists empty; 24 rows: fewer rows than ranges, eight ranges own no row at all
    B = cd.tiny(n_rows, small=True)
    rec, hot, built, diff = cd.probe(B, 4, 2, 32)
    assert built and rec["NB"] == 32 and rec["n_steps"] == 2 and diff < EMU_TOL, (rec, diff)
    owned = len(set((np.arange(n_rows) * 32) // n_rows))
    assert owned == min(n_rows, 32) and rec["n_cold"] < rec["n_steps"] * 32


def test_emulation_goes_blind_with_large_values():
    # the reason for the small values: with the kernel tests' values the two orders of summation alone differ by O(1) on this design, so
    # that a bound on the difference would say nothing about the plan (the plan is the same: the structure decides it)
    rec_s, hot_s, _, _ = cd.probe(cd.edges(small=True), 4, 2, 2)
    rec_l, hot_l, built, diff = cd.probe(cd.edges(small=False), 4, 2, 2)
    assert built and {k: rec_l[k] for k in cd.PLAN_FIELDS} == {k: rec_s[k] for k in cd.PLAN_FIELDS} and list(hot_l) == list(hot_s)
    print("emulation difference with values 0.2-1.0: %.3g" % diff)
    assert diff > 1e-3, diff
