"""The three device predictors read the kept samples through one view: a range of a device store in place, or host
samples uploaded for the call. Whatever the samples' origin the same kernels run over the same numbers, so every comparison here
is bit for bit, at the C-API level: host samples against a store, a sub-range of a store against the host call on that slice, the
tiled and chunked summaries against the untiled ones, and the streaming per-sample predictor against the store's."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import pairs_ref as pr
from tests import pairs_rel_ref as rr
from tests.test_gpu_predict_dist import design

pytestmark = pytest.mark.gpu

QUANTILES = (0.05, 0.5, 0.95)


def store_of(samples):
    from myfm_amd import _capi

    st = _capi.Store(samples[0][1].shape[0], samples[0][2].shape[1])
    for w0, w, V in samples:
        st.push(w0, w, V)
    return st


def same(a, b):
    """a and b (arrays or tuples of arrays) are equal bit for bit"""
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---- pairs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("blocks", [0, 1])
def test_pairs_host_samples_equal_the_store(blocks, K, mode):
    """U = 17, I = 250 (one query tile, candidates short of a stripe step), without blocks and with one relation block per side"""
    from myfm_amd import _capi

    rng = np.random.default_rng(100 * blocks + 10 * K + mode)
    sd = rr.block_sides(rng, 17, 250, 9, 11, blocks, blocks, mean_nnz=2.0)
    Xq, Xc, rq, rc = rr.capi_args(sd)
    samples = pr.normal_samples(rng, sd["D"], K, 4)
    cuts = rr.sorted_cuts(rng, 4, 2) if mode == 2 else None

    def pairs(lo, hi):
        return _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, cutpoints=None if cuts is None else cuts[lo:hi])

    P, st3 = pairs(0, 3), store_of(samples[:3])
    assert same(P.scores(samples[:3], mode), P.scores_store(st3, mode))
    assert same(P.topk(samples[:3], 10, mode), P.topk_store(st3, 10, mode))
    P.close()
    st3.close()
    P, st4 = pairs(1, 3), store_of(samples)
    assert same(P.scores(samples[1:3], mode), P.scores_store(st4, mode, first=1, count=2))
    assert same(P.topk(samples[1:3], 10, mode), P.topk_store(st4, 10, mode, first=1, count=2))
    P.close()
    st4.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("blocks", [0, 1])
def test_pair_moments_host_samples_equal_the_store(blocks, K, mode):
    """The moments form (mean and std of every pair, the top 10 by mean + 0.7 std) on the shapes of the test above. k = 10 < I
    and nothing is excluded, so no NaN tail enters the comparison."""
    from myfm_amd import _capi

    rng = np.random.default_rng(1000 + 100 * blocks + 10 * K + mode)
    sd = rr.block_sides(rng, 17, 250, 9, 11, blocks, blocks, mean_nnz=2.0)
    Xq, Xc, rq, rc = rr.capi_args(sd)
    samples = pr.normal_samples(rng, sd["D"], K, 4)
    cuts = rr.sorted_cuts(rng, 4, 2) if mode == 2 else None

    def pairs(lo, hi):
        return _capi.Pairs(Xq, Xc, rel_query=rq, rel_cand=rc, cutpoints=None if cuts is None else cuts[lo:hi])

    P, st3 = pairs(0, 3), store_of(samples[:3])
    assert same(P.moments(samples[:3], mode), P.moments_store(st3, mode))
    assert same(P.topk_ucb(samples[:3], 10, beta=0.7, mode=mode), P.topk_ucb_store(st3, 10, beta=0.7, mode=mode))
    P.close()
    st3.close()
    P, st4 = pairs(1, 3), store_of(samples)
    assert same(P.moments(samples[1:3], mode), P.moments_store(st4, mode, first=1, count=2))
    assert same(P.topk_ucb(samples[1:3], 10, beta=0.7, mode=mode), P.topk_ucb_store(st4, 10, beta=0.7, mode=mode, first=1, count=2))
    P.close()
    st4.close()


# ---- summaries and predictions -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["flat", "block"])
def rows257(request):
    """257 rows (more than one 128-row tile, and one row over), 5 samples of rank 3 on the host and in a store; "block": the
    design carries one relation block, so it takes the per-sample passes"""
    from myfm_amd import _capi

    rng = np.random.default_rng(7)
    X = design("values", 257, rng)
    blocks, n_features = [], X.shape[1]
    if request.param == "block":
        B = sps.csr_matrix(rng.choice([0.0, 1.0, -0.5], size=(7, 5), p=[0.5, 0.25, 0.25]))
        blocks = [(rng.integers(0, 7, size=257), B)]
        n_features += 5
    samples = pr.normal_samples(rng, n_features, 3, 5)
    d, st = _capi.Design(X, blocks), store_of(samples)
    yield d, st, samples, rng.uniform(0.5, 2.0, size=5), rr.sorted_cuts(rng, 5, 2)
    st.close()
    d.close()


@pytest.mark.parametrize("mode,noise", [(0, False), (1, False), (0, True)])
def test_summary_host_samples_equal_the_store(rows257, mode, noise):
    d, st, samples, prec, _ = rows257
    kw = dict(mode=mode, quantiles=QUANTILES)
    host = d.summary(samples, precisions=prec if noise else None, **kw)
    assert same(host, st.summary(d, precisions=prec if noise else None, **kw))
    # two-sample chunks (5 = 2 + 2 + 1) and 128-row tiles (257 = 128 + 128 + 1)
    assert same(host, st.summary(d, precisions=prec if noise else None, tile_rows=128, chunk_samples=2, **kw))
    part = st.summary(d, precisions=prec[1:4] if noise else None, first=1, count=3, **kw)
    assert same(part, d.summary(samples[1:4], precisions=prec[1:4] if noise else None, **kw))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_predict_store_range_equals_streamed_host_samples(rows257, mode):
    """mfm_design_predict streams one sample at a time through the per-sample pass; the store's predictor takes one pass over all
    samples on the flat design"""
    d, st, samples, _, cuts = rows257
    got = st.predict(d, mode, cutpoints=cuts[1:4] if mode == 2 else None, first=1, count=3)
    assert got.shape == ((257, 3) if mode == 2 else (257,))
    assert same(got, d.predict(samples[1:4], mode, cutpoints=cuts[1:4] if mode == 2 else None))
