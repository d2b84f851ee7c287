"""The longdouble reference and the restated planner geometry of the cell path's layout-edge tests (tests/cell_ref.py) -- no GPU.

Established here before any device number is looked at: the reference (the sequential sweep over the expanded flat design)
computes what the float64 oracle's update_w, update_V_factor and update_e compute on the blocked design, from the same state and
variates, and the oracle sits within ONE TENTH of the single-call bounds on every accepted case -- the other nine tenths are what
the device's different summation order may use. And every case states its geometry: the figures it names are what the restated
planner (cell_ref.plan) computes for its arrays.
"""
import numpy as np
import pytest

from . import cell_ref as R

ACCEPTED = [c for c in R.CASES if c.why is None]


def _tenth(tol):
    return dict(rtol=tol["rtol"] / 10, atol=tol["atol"] / 10)


@pytest.mark.parametrize("case", ACCEPTED, ids=repr)
def test_oracle_within_a_tenth_of_the_bound_of_the_longdouble_reference(oracle, case):
    d = case.design()
    p, ref = R.reference(case)
    K = case.K
    o = oracle.OracleTrainer(d.main, d.y, d.blocks, rank=K, group_index=d.gi)
    assert o.D == d.D and o.G == int(d.gi.max()) + 1

    def reset():
        o.set_fm(p["w0"], p["w"], p["V"])
        o.set_e(p["e"])
        o.set_hyper(p["alpha"], p["mu_w"], p["lam_w"], p["mu_V"], p["lam_V"])

    # the oracle draws its variates itself: the reference is run on what its generator is about to hand out
    reset()
    z = o.clone().rng_sample_normals(d.D)
    w, e = R.sweep_w_ref(d, p["w"], p["e"], p["alpha"], p["lam_w"], p["mu_w"], z)
    o.substep(4)  # update_w
    got = dict(w=(o.fm()[1], w, R.TOL_W), e_w=(o.e(d.n), e, R.TOL_EQ))
    reset()
    z = o.clone().rng_sample_normals(K * d.D).reshape(K, d.D)
    V, e, q = R.sweep_V_ref(d, p["V"], p["e"], p["alpha"], p["lam_V"], p["mu_V"], z, 0, K)
    for f in range(K):
        o.update_V_factor(f)
    got.update(V=(o.fm()[2], V, R.TOL_V), e_V=(o.e(d.n), e, R.TOL_EQ), q=(o.q(d.n), q, R.TOL_EQ))
    reset()
    o.substep(8)  # update_e
    got.update(score=(o.e(d.n), ref["score"], R.TOL_SCORE))
    for k, (g, r, tol) in got.items():
        print("%s %s: %.2e of the bound" % (case, k, R.worst(g, r, **tol)))
        np.testing.assert_allclose(g, r.astype(np.float64), err_msg=k, **_tenth(tol))


@pytest.mark.parametrize("case", R.SCORE_CASES, ids=repr)
@pytest.mark.parametrize("K", R.SCORE_RANKS)
def test_oracle_score_within_a_tenth_of_the_bound(oracle, case, K):
    d = case.design()
    p = R.problem(d, K, 11)
    o = oracle.OracleTrainer(d.main, d.y, d.blocks, rank=K, group_index=d.gi)
    o.set_fm(p["w0"], p["w"], p["V"])
    o.substep(8)
    np.testing.assert_allclose(o.e(d.n), R.score_ref(d, p["w0"], p["w"], p["V"], d.y).astype(np.float64), **_tenth(R.TOL_SCORE))


@pytest.mark.parametrize("case", R.CASES + R.SCORE_CASES, ids=repr)
def test_cases_state_their_geometry(case):
    d, want = case.design(), case.want()
    assert d.n <= R.ROW_CAP
    assert d.main.nnz == len(d.idx) * d.n and np.all(d.main.data == 1.0) and np.all(np.diff(d.idx[0]) >= 0)
    if case.why is not None:
        assert not want["ready"] and want["why"] == case.why and not case.expect
        return
    assert want["ready"], want["why"]
    for k, v in case.expect.items():
        assert want[k] == v, (k, want[k], v)
    # self-consistency of the restated layout
    assert want["N"] == d.n and want["Npad"] % R.SROWS == 0 and want["Npad"] >= want["G"] * R.SROWS
    assert 0 <= want["chunk_min"] <= want["chunk_max"] <= want["max_steps"] * R.WROWS < want["chunk_max"] + R.WROWS
    assert (want["chunks_empty"] > 0) == (want["chunk_min"] == 0)
    assert want["G"] * R.NW * want["chunk_max"] >= d.n >= want["G"] * R.NW * want["chunk_min"]
    assert sum(1 for st in want["streams"] if st[0] == "I") <= 1 and want["streams"][0][0] == "U"
    assert want["item32"] == any(st[0] == "I" and st[1] < 0 for st in want["streams"])
    if want["G"] > 9:  # the (group, item) partials are G x cardI: many groups only without a scattered stream
        assert all(st[0] != "I" or st[2] <= R.SMALL_MAX for st in want["streams"])


def test_the_cases_cover_every_kind_of_field_at_both_item_widths():
    seen = set()
    for case in R.CASES:
        want = case.want()
        if want["ready"]:
            for s, kind, _ in want["fields"]:
                ty = want["streams"][s][0]
                seen.add((ty, kind, want["item32"] if ty == "I" else None))
    assert seen >= {("U", 0, None), ("U", 1, None), ("C", 0, None), ("C", 1, None), ("I", 0, False), ("I", 1, False),
                    ("I", 0, True), ("I", 1, True)}
    assert {R.CASE[n].want()["G"] for n in ("groups_1", "groups_2", "groups_7", "groups_9", "groups_256_lds_streams_only")} == {1, 2, 7, 9, 256}
    assert {c.want()["score_fb"] for c in R.SCORE_CASES} == {4, 2, 1}


def test_6144_rows_are_sixteen_chunks_of_384_and_6145_put_one_row_in_step_two():
    a, b = R.CASE["rows_6144_all_distinct"].want(), R.CASE["rows_6145_one_row_in_step_2"].want()
    assert (a["chunk_min"], a["chunk_max"], a["max_steps"], a["chunks_empty"]) == (384, 384, 1, 0)
    assert (b["chunk_min"], b["chunk_max"], b["max_steps"]) == (384, 385, 2) and b["N"] == 16 * 384 + 1


def test_lds_limit_of_a_block_on_a_c_stream_comes_from_lds_bytes():
    # beside one user: 1 + B (tables) + 4 B (accumulators) + 2 (turn word) <= 19968 -> B <= 3993; a main field of 4096 is taken
    B = R.C_BLOCK_MAX
    assert B == (R.LDS_DOUBLES - 2 - 1) // 5 == 3993 < R.SMALL_MAX
    st, fd = [("U", 0, 1), ("C", 1, B)], [(0, 0, 1), (1, 1, B)]
    assert R.lds_doubles(st, fd, 1, -1, 1, False) == 1 + B + 4 * B + 2 == R.LDS_DOUBLES
    assert R.groups_fit(st, fd, 1) and not R.groups_fit([("U", 0, 1), ("C", 1, B + 1)], [(0, 0, 1), (1, 1, B + 1)], 1)
    assert R.CASE["c_main_4096"].want()["ready"]


def test_reference_is_the_plain_conditional_on_a_tiny_design():
    # one update_w of the flat design written out with dense float arithmetic, feature after feature
    d = R.CASE["tiny_63"].design()
    p = R.problem(d, 2, 3)
    X = d.flat.toarray()
    w, e = p["w"].copy(), p["e"].copy()
    for j in range(d.D):
        x, g = X[:, j], d.gi[j]
        prec = p["lam_w"][g] + p["alpha"] * (x * x).sum()
        new = (-p["alpha"] * (x * (e - x * w[j])).sum() + p["lam_w"][g] * p["mu_w"][g]) / prec + p["zw"][j] / np.sqrt(prec)
        e += x * (new - w[j])
        w[j] = new
    rw, re = R.sweep_w_ref(d, p["w"], p["e"], p["alpha"], p["lam_w"], p["mu_w"], p["zw"])
    np.testing.assert_allclose(rw.astype(np.float64), w, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(re.astype(np.float64), e, rtol=1e-11, atol=1e-12)
    s = p["w0"] + X @ p["w"] + 0.5 * (((X @ p["V"]) ** 2).sum(axis=1) - ((X * X) @ (p["V"] ** 2)).sum(axis=1)) - d.y
    np.testing.assert_allclose(R.score_ref(d, p["w0"], p["w"], p["V"], d.y).astype(np.float64), s, rtol=1e-12, atol=1e-13)
