"""The scorer family -- k_score, its one-pass twin k_score_store, k_block_score_cache and the transposes k_build_vt /
k_build_vt_batch -- at every lane-group shape of score_shape (csrc/mfm_hip.hip) and of launch_block_score_cache, on every row
layout (unit ELL, unit ragged CSR, valued ragged CSR, valued fixed-width, empty rows, an empty table), across sample chunks
(the continuation of k_score_store), with up to 33 ordered-probit classes, over row tiles of the summaries, and up to the
refusal of rank > 512.

Held against tests/score_ref.py: the score in np.longdouble, tolerance tol = gamma_n M per row, the running-error bound of a
float64 evaluation in any fixed order (derived, not tuned; tests/test_score_ref_cpu.py shows that float64 in three orders
uses about a tenth of it and that every factor and entry moves a row by 100 tol). Mean Phi and the class probabilities get
PHI_SLOPE tol (Phi' <= 0.3990) and ERF_ALLOW for the device's erf. The designs are tests/score_designs.py's: the smallest at
which the respective code can go wrong.
"""
import numpy as np
import pytest

from . import score_designs as sd
from . import score_ref as sr

pytestmark = pytest.mark.gpu

LD = np.longdouble
# What a probability may be off beyond PHI_SLOPE times the score's own error: the device's erf and scipy's, the rounding of
# their arguments and of (1 + erf) / 2, and the sums over the samples. The one constant here that is not derived: four units
# of roundoff, a chosen allowance. It has not had to be measured up: on the MI355X the largest error of a mean Phi in this
# file is 0.20 of PHI_SLOPE tol + ERF_ALLOW, of a class probability 0.07 of twice that.
ERF_ALLOW = 4 * 2.0 ** -53


@pytest.fixture(scope="module")
def capi():
    from myfm_amd import _capi

    if _capi.lib().mfm_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _capi


class Ref:
    """mean score, mean Phi(score), mean class probabilities of a design over samples, with their per-row tolerances"""

    def __init__(self, X, blocks, samples, cuts=None):
        rows = sr.flat_rows(X, blocks)
        self.scores = [sr.fm_score(X, blocks, *s, rows) for s in samples]
        self.tols = [sr.fm_score_bound(X, blocks, *s, rows)[1] for s in samples]
        S = len(samples)
        self.tol = sum(self.tols) / S
        self.prob_tol = sr.PHI_SLOPE * self.tol + ERF_ALLOW
        self.mean = {0: sum(self.scores) / S, 1: sum(sr.phi(sc) for sc in self.scores) / S}
        if cuts is not None:
            self.mean[2] = sum(sr.class_probs(sc, cp) for sc, cp in zip(self.scores, cuts)) / S

    def check(self, mode, got, what):
        ref = self.mean[mode]
        assert got.shape == ref.shape, what
        tol = {0: self.tol, 1: self.prob_tol, 2: (2 * self.prob_tol)[:, None]}[mode]
        err = np.abs(got.astype(LD) - ref)
        print("%s mode %d: largest error / tolerance %.3f" % (what, mode, float((err / tol).max())))
        assert np.all(err <= tol), (what, mode, float((err / tol).max()))


def _store(capi, D, K, samples):
    st = capi.Store(D, K)
    for s in samples:
        st.push(*s)
    return st


def _cut(cuts, mode, lo=None, hi=None):
    return None if mode != 2 else cuts[lo:hi]


def _predict_everywhere(capi, monkeypatch, dev, st, samples, cuts, first, count, modes=(0, 1, 2)):
    """{mode: result} of samples [first, first + count): the store as it runs by default, the same under
    MFM_PREDICT_PER_SAMPLE=1 and the host samples through the ring must agree bit for bit"""
    sub, subcuts = samples[first:first + count], cuts[first:first + count]
    out = {}
    for mode in modes:
        out[mode] = st.predict(dev, mode, _cut(subcuts, mode), first=first, count=count)
    monkeypatch.setenv("MFM_PREDICT_PER_SAMPLE", "1")
    for mode in modes:
        assert np.array_equal(out[mode], st.predict(dev, mode, _cut(subcuts, mode), first=first, count=count)), ("per-sample", mode)
        assert np.array_equal(out[mode], dev.predict(sub, mode, _cut(subcuts, mode))), ("host samples", mode)
    monkeypatch.delenv("MFM_PREDICT_PER_SAMPLE")
    return out


# ---- the rank table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sd.RANKS)
def test_every_rank_shape_on_every_row_layout(capi, monkeypatch, K):
    cuts = sd.cutpoints(5, 4, 200)
    samples = sd.samples(sd.D0, K, 5, 100)
    for lay in sd.LAYOUTS:
        X = sd.layout(lay)
        dev, st = capi.Design(X, []), _store(capi, sd.D0, K, samples)
        for first, count in ((0, 5), (1, 3)):
            got = _predict_everywhere(capi, monkeypatch, dev, st, samples, cuts, first, count)
            ref = Ref(X, [], samples[first:first + count], cuts[first:first + count])
            for mode in (0, 1, 2):
                ref.check(mode, got[mode], "rank %d layout %s samples %d+%d" % (K, lay, first, count))
            assert got[2].shape == (sd.N_ROWS, 5)


@pytest.mark.parametrize("K", sd.TINY_RANKS)
def test_tables_of_one_and_three_rows_and_without_entries(capi, monkeypatch, K):
    cuts = sd.cutpoints(5, 4, 201)
    for N in (1, 3):
        X, samples = sd.layout("b", N=N), sd.samples(sd.D0, K, 5, 101)
        dev, st = capi.Design(X, []), _store(capi, sd.D0, K, samples)
        got = _predict_everywhere(capi, monkeypatch, dev, st, samples, cuts, 0, 5)
        ref = Ref(X, [], samples, cuts)
        for mode in (0, 1, 2):
            ref.check(mode, got[mode], "rank %d, %d rows" % (K, N))
    # no stored entry at all: the score is w0, exactly
    X, samples = sd.empty_table(), sd.samples(sd.D0, K, 5, 102)
    dev, st = capi.Design(X, []), _store(capi, sd.D0, K, samples)
    got = _predict_everywhere(capi, monkeypatch, dev, st, samples, cuts, 0, 5)
    ref = Ref(X, [], samples, cuts)
    for mode in (0, 1, 2):
        ref.check(mode, got[mode], "rank %d, empty table" % K)
    for k, s in enumerate(samples):
        one = _predict_everywhere(capi, monkeypatch, dev, st, samples, cuts, k, 1, modes=(0,))
        assert np.array_equal(one[0], np.full(5, s[0]))


# ---- one design, many ranks ----------------------------------------------------------------------------------------------
def test_one_design_at_many_ranks_in_turn(capi):
    # design_use_rank re-sizes the caches at every change of rank: the pad columns of Vt / bq must come back zero
    X, blocks = sd.layout("c"), sd.two_blocks()
    D = sd.dim_all(X, blocks)
    dev = capi.Design(X, blocks)
    for K in sd.REUSE_RANKS:
        samples = sd.samples(D, K, 3, 103)
        ref = Ref(X, blocks, samples)
        ref.check(0, dev.predict(samples, 0), "one design, now rank %d" % K)


# ---- relation blocks: the boundaries of both tables ----------------------------------------------------------------------
def _check_blocks(capi, X, blocks, K, seed, what):
    D = sd.dim_all(X, blocks)
    samples, cuts = sd.samples(D, K, 3, seed), sd.cutpoints(3, 4, 202)
    dev, st = capi.Design(X, blocks), _store(capi, D, K, samples)
    ref = Ref(X, blocks, samples, cuts)
    for mode in (0, 2):
        got = dev.predict(samples, mode, _cut(cuts, mode))
        assert np.array_equal(got, st.predict(dev, mode, _cut(cuts, mode))), (what, mode)
        ref.check(mode, got, what)


@pytest.mark.parametrize("K", sd.BLOCK_RANKS)
def test_relation_blocks_at_the_boundaries_of_both_tables(capi, K):
    _check_blocks(capi, sd.layout("c"), sd.two_blocks(), K, 104, "two blocks, rank %d" % K)


@pytest.mark.parametrize("K", sd.MANY_BLOCK_RANKS)
def test_seventeen_blocks_under_wide_shapes(capi, K):
    # one block more than travels in the kernel arguments (MAX_BLOCKS = 16): its pointers come through device arrays
    _check_blocks(capi, sd.layout("c"), sd.many_blocks(), K, 105, "17 blocks, rank %d" % K)


# ---- the training context's scorer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sd.TRAIN_RANKS)
def test_training_context_scores_on_the_generic_path(capi, K):
    # k_score mode 0 with y (update_e) and score_design on the context's own Vt / bq (score_ctx). No sweep is run.
    X, y, blocks = sd.train_design()
    c = capi.Context(X, y, blocks, rank=K, group_index=np.zeros(sd.dim_all(X, blocks), dtype=np.int32))
    flags = c.plan_flags()
    assert not flags["mf"] and not flags["cell"] and not flags["resident"], flags  # else k_mf_score / k_cell_score / k_res_score
    (w0, w, V), = sd.samples(c.D, K, 1, 106)
    c.set_state(w0, w, V)
    c.set_w0(w0)
    c.update_e_regression()
    ref = Ref(X, blocks, [(w0, w, V)])
    err = np.abs(c.get_e().astype(LD) - (ref.mean[0] - y.astype(LD)))
    print("rank %d update_e: largest error / tolerance %.3f" % (K, float((err / ref.tol).max())))
    assert np.all(err <= ref.tol)
    Xt, tblocks = sd.train_test_design()
    Ref(Xt, tblocks, [(w0, w, V)]).check(0, capi.Design(Xt, tblocks).score_ctx(c), "rank %d score_ctx" % K)


# ---- classes in mode 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sd.CLASS_RANKS)
@pytest.mark.parametrize("n_class", sd.CLASS_COUNTS)
def test_class_counts_up_to_and_past_the_one_pass_limit(capi, n_class, K):
    # CPL = ceil(32 / GS) classes per lane: rank 4 has eight, rank 65 one with lanes beyond n_class idle; 33 classes take
    # the per-sample passes
    X, samples, cuts = sd.layout("b"), sd.samples(sd.D0, K, 4, 107), sd.cutpoints(4, n_class - 1, 203)
    dev, st = capi.Design(X, []), _store(capi, sd.D0, K, samples)
    got = st.predict(dev, 2, cuts)
    assert got.shape == (sd.N_ROWS, n_class)
    assert np.array_equal(got, dev.predict(samples, 2, cuts))
    Ref(X, [], samples, cuts).check(2, got, "rank %d, %d classes" % (K, n_class))


# ---- sample chunks: the continuation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sd.CHUNK_CASES))
def test_sample_chunks_continue_the_sums(capi, monkeypatch, name):
    # k_score_store with sa.first == 0: the sums of the earlier chunks are read back from `out`, the last chunk scales
    case = sd.CHUNK_CASES[name]
    # (design_stage_samples, csrc/mfm_predict.hpp: a chunk is the samples whose row-major V copies fit 512 MB)
    chunk = (512 * 2 ** 20) // (8 * case.D * ((case.K + 1) & ~1))
    assert chunk == sd.chunk_size(case.D, case.K) and 1 < chunk < case.S
    X, samples = sd.chunk_samples(name)
    cuts = sd.cutpoints(case.S, case.n_class - 1, 204)
    dev, st = capi.Design(X, []), _store(capi, case.D, case.K, samples)
    for first, count in ((0, case.S), (2, case.S - 3)):
        if name == "B":
            assert count > chunk  # 3 + 3 + 1, then 3 + 1
        sub, subcuts = samples[first:first + count], cuts[first:first + count]
        got = {mode: st.predict(dev, mode, _cut(subcuts, mode), first=first, count=count) for mode in (0, 1, 2)}
        monkeypatch.setenv("MFM_PREDICT_PER_SAMPLE", "1")
        for mode in (0, 1, 2):
            assert np.array_equal(got[mode], st.predict(dev, mode, _cut(subcuts, mode), first=first, count=count)), (mode, first)
        monkeypatch.delenv("MFM_PREDICT_PER_SAMPLE")
        ref = Ref(X, [], sub, subcuts)
        for mode in (0, 1, 2):
            ref.check(mode, got[mode], "chunks %s samples %d+%d" % (name, first, count))
        assert got[2].shape == (sd.CHUNK_ROWS, case.n_class)


# ---- row tiles of the summaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sd.TILE_RANKS)
def test_row_tiles_of_the_summaries(capi, K):
    # score_rows: the pointer arithmetic of modes 3 / 4. 63 rows per tile is no multiple of SCORE_RU; 203 = 3 * 63 + 14
    for lay in ("a", "b"):
        X, samples = sd.layout(lay), sd.samples(sd.D0, K, 5, 108)
        dev, st = capi.Design(X, []), _store(capi, sd.D0, K, samples)
        ref = Ref(X, [], samples)
        for mode in (0, 1):
            mean, _, q = st.summary(dev, mode, quantiles=(0.5,), tile_rows=63, chunk_samples=2)
            assert np.array_equal(mean, st.predict(dev, mode)), (lay, mode)
            # the median of five is the third smallest; an order statistic moves by no more than the largest move of a value
            values = np.stack(ref.scores if mode == 0 else [sr.phi(sc) for sc in ref.scores])
            tol = np.max(np.stack(ref.tols), axis=0)
            tol = tol if mode == 0 else sr.PHI_SLOPE * tol + ERF_ALLOW
            err = np.abs(q[0].astype(LD) - np.sort(values, axis=0)[2])
            print("rank %d layout %s mode %d median: largest error / tolerance %.3f" % (K, lay, mode, float((err / tol).max())))
            assert np.all(err <= tol), (lay, mode)


# ---- the refusal (last: it leaves a design at a rank no kernel takes) ------------------------------------------------------
@pytest.mark.parametrize("with_blocks", [False, True])
def test_rank_above_512_is_refused_and_the_design_lives_on(capi, with_blocks):
    X, blocks = sd.layout("c"), (sd.two_blocks() if with_blocks else [])
    D = sd.dim_all(X, blocks)
    dev = capi.Design(X, blocks)
    with pytest.raises(ValueError, match="rank > 512 is not supported"):
        dev.predict(sd.samples(D, 513, 2, 109), 0)
    samples = sd.samples(D, 4, 2, 109)
    Ref(X, blocks, samples).check(0, dev.predict(samples, 0), "rank 4 after the refusal")
