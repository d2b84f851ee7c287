"""The streamed block chain (csrc/mfm_chain_stream.hpp, k_cs_stream) on every overflow path and step edge: the designs of
tests/chain_designs.py, with (Cg, Lw, NB) forced, two Gibbs iterations against the CPU oracle (same seed, 1e-7). Which paths a case
reaches is asserted on the plan record in tests/test_chain_edges_cpu.py; here every case proves through `chain_stream_info()` that the
forced plan is the one that was built (the record equals the host probe's, field by field) and that k_cs_stream was launched for
update_w and for update_V -- the launcher prefers the one-workgroup LDS chain for blocks of up to 1996 rows, which is why the blocks of
the oracle cases have more."""
import numpy as np
import pytest

from . import chain_designs as cd
from .gibbs_driver import CapiGibbs

pytestmark = pytest.mark.gpu

ITERS = 2


@pytest.fixture(scope="module")
def capi():
    from myfm_amd import _capi

    if _capi.lib().mfm_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _capi


_BLOCKS = {"edges": cd.edges, "tiny40": lambda: cd.tiny(40), "tiny24": lambda: cd.tiny(24)}
_BLOCKS.update({"short%d" % n: (lambda n=n: cd.short(n)) for n in cd.SHORT_NS})
_refs = {}


def _ref(oracle, name, rank):
    """the design, the oracle's start and its state after ITERS iterations: computed once per (design, rank), never changed"""
    if (name, rank) not in _refs:
        B = _BLOCKS[name]()
        design = cd.with_main_table(B, n_min=2000)
        main, y, blocks, gi = design
        t0 = oracle.OracleTrainer(main, y, blocks, rank=rank, group_index=gi)
        t = t0.clone()
        for _ in range(ITERS):
            t.step()
        n = main.shape[0]
        _refs[(name, rank)] = dict(B=B, design=design, t0=t0, fm0=t0.fm(), e0=t0.e(n), fm=t.fm(), e=t.e(n))
    return _refs[(name, rank)]


def _force(monkeypatch, cg, lw, nb):
    monkeypatch.setenv("MFM_CHAIN_GRID_MIN", "0")  # (small blocks: their cold parts would not go to the grid otherwise)
    monkeypatch.setenv("MFM_NO_CELL", "1")         # the generic relation-block path
    monkeypatch.setenv("MFM_CS_CG", str(cg))
    monkeypatch.setenv("MFM_CS_NB", str(nb))
    monkeypatch.setenv("MFM_CS_LW", str(lw))
    monkeypatch.setenv("MFM_CS_LW_MIN", str(lw))


def _run(capi, ref, rank):
    main, y, blocks, gi = ref["design"]
    c = capi.Context(main, y, blocks, rank=rank, group_index=gi)
    c.set_state(*ref["fm0"])
    c.set_e(ref["e0"])
    drv = CapiGibbs(c, ref["t0"].clone(), main.shape[0], gi)
    for _ in range(ITERS):
        drv.step()
    return c


def _assert_oracle(c, ref):
    w0, w, V = ref["fm"]
    _, gw, gV = c.get_state()
    np.testing.assert_allclose(gV, V, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(gw, w, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(c.get_e(), ref["e"], rtol=1e-7, atol=1e-7)


def _assert_streamed(c, ref, cfg, rank):
    """one streamed run over the whole block with the forced plan -- the host probe's record -- launched once per sweep"""
    info = c.chain_stream_info()
    print(cfg, info)
    assert len(info) == 1 and c.plan_flags()["streamed_chain"], info
    rec = info[0]
    assert rec["block"] == 0 and (rec["Cg"], rec["Lw"], rec["NB"]) == tuple(cfg), rec
    want, _, built, _ = cd.probe(ref["B"], *cfg)
    assert built and {k: rec[k] for k in cd.PLAN_FIELDS} == {k: want[k] for k in cd.PLAN_FIELDS}, (rec, want)
    assert rec["launches_w"] > 0 and rec["launches_V"] > 0, rec
    assert (rec["launches_w"], rec["launches_V"]) == (ITERS, ITERS * rank), rec  # update_w once, update_V once per factor
    return rec


def _case(oracle, capi, monkeypatch, name, cfg, rank=3):
    _force(monkeypatch, *cfg)
    ref = _ref(oracle, name, rank)
    c = _run(capi, ref, rank)
    rec = _assert_streamed(c, ref, cfg, rank)
    _assert_oracle(c, ref)
    return c, rec


@pytest.mark.parametrize("cfg", cd.EDGES_CONFIGS)
def test_edges_match_the_oracle(oracle, capi, monkeypatch, cfg):
    c, rec = _case(oracle, capi, monkeypatch, "edges", cfg)
    assert rec["n_cols"] == 44 and rec["hot_rounds"] == [3, 23, 2, 2, 2, 2, 2, 2, 2, 4], rec


@pytest.mark.parametrize("rank", [1, 8])
def test_edges_at_rank_1_and_8(oracle, capi, monkeypatch, rank):
    _case(oracle, capi, monkeypatch, "edges", (4, 2, 2), rank=rank)


def test_edges_are_reproducible_and_equal_the_batched_form(oracle, capi, monkeypatch):
    ref = _ref(oracle, "edges", 3)
    _force(monkeypatch, 4, 2, 2)
    c1, c2 = _run(capi, ref, 3), _run(capi, ref, 3)
    _assert_streamed(c1, ref, (4, 2, 2), 3)
    _assert_streamed(c2, ref, (4, 2, 2), 3)
    for a, b in zip(c1.get_state()[1:], c2.get_state()[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(c1.get_e(), c2.get_e())
    monkeypatch.setenv("MFM_NO_CB_STREAM", "1")
    c3 = _run(capi, ref, 3)
    assert c3.chain_stream_info() == [] and not c3.plan_flags()["streamed_chain"]
    np.testing.assert_allclose(c3.get_state()[2], c1.get_state()[2], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(c3.get_state()[1], c1.get_state()[1], rtol=1e-8, atol=1e-8)


def test_a_window_beyond_the_lds_is_not_streamed(oracle, capi, monkeypatch):
    # (4, 7, 2) needs 169012 bytes: the planner keeps the conflict batches, and the chain is the oracle's all the same
    ref = _ref(oracle, "edges", 3)
    _force(monkeypatch, *cd.EDGES_REFUSED)
    c = _run(capi, ref, 3)
    assert c.chain_stream_info() == [] and not c.plan_flags()["streamed_chain"]
    _assert_oracle(c, ref)


@pytest.mark.parametrize("n", cd.SHORT_NS)
@pytest.mark.parametrize("cfg", cd.SHORT_CONFIGS)
def test_short_runs_match_the_oracle(oracle, capi, monkeypatch, n, cfg):
    c, rec = _case(oracle, capi, monkeypatch, "short%d" % n, cfg)
    assert rec["n_cols"] == n and rec["n_steps"] == -(-n // cfg[0]), rec


@pytest.mark.parametrize("name", ["tiny40", "tiny24"])
def test_tiny_block_with_empty_ranges(oracle, capi, monkeypatch, name):
    # 40 (24) block rows in 32 ranges. A block this small goes to the LDS chain unless batching is forced; with it forced the planner
    # streams it (asserted through the info: the record and the launches)
    monkeypatch.setenv("MFM_CHAIN_FORCE_BATCHED", "1")
    c, rec = _case(oracle, capi, monkeypatch, name, (4, 2, 32))
    assert rec["NB"] == 32 and rec["n_steps"] == 2, rec
