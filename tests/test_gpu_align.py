"""aligned_factors on the device: k_align_gram, k_align_polar and k_align_apply behind mfm_align against the float64
reference of tests/align_ref.py, whose tolerance is derived there and checked against a 40-digit twin in test_align_cpu.py.

Largest used share of the tolerance over the real-valued cases, as printed by test_real_valued: see DESIGN 4.15."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import align_ref as ar
from tests.test_gpu_pairs_sim import _fit, tiny_table, N_ITEMS, N_USERS  # noqa: F401

pytestmark = pytest.mark.gpu
CHUNK = 2048  # (align_chunk_cols of csrc/mfm_align.hpp)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _orth_err(R):
    return np.sqrt(((np.einsum("sab,sac->sbc", R, R) - np.eye(R.shape[1])) ** 2).sum(axis=(1, 2)))


@pytest.mark.parametrize("n_refine", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 33, 64])
def test_exact_layout(K, S, n_refine):
    """ref's factor a lives on the columns d = a mod K with entries +-2^e, e one of three per factor; sample s is a signed
    permutation of ref's factors. Every sum has one non-zero term or is a small integer times a power of two, so the rotations are
    the signed permutations, mean is ref and alignment is 1 BIT FOR BIT and std is 0: R against its transpose, the permutation's
    direction, tile and chunk edges (D = K, 63 + K, 64 + K, one column past a chunk), the bye of an odd K."""
    from myfm_amd import _capi

    for D in (K, 63 + K, 64 + K, CHUNK + 1):
        rng = np.random.default_rng([K, S, D])
        ref = np.zeros((K, D))
        d = np.arange(D)
        ref[d % K, d] = rng.choice([-1.0, 1.0], D) * 2.0 ** rng.integers(-1, 2, K)[d % K]
        Vs, Rs = np.empty((S, K, D)), np.zeros((S, K, K))
        for s in range(S):
            perm, sign = rng.permutation(K), rng.choice([-1.0, 1.0], K)
            Rs[s, np.arange(K), perm] = sign  # V_s[a] = sign_a ref[perm_a]  =>  M_s[a][perm_a] = sign_a |ref[perm_a]|^2
            Vs[s] = sign[:, None] * ref[perm]
        Vs[S - 1], Rs[S - 1] = ref, np.eye(K)  # (the reference sample itself)
        got = _capi.align(ar.samples_of(Vs), -1, n_refine)
        assert _same(got, (ref.T, np.zeros((D, K)), Rs, np.ones(S))), (D, got[3])


@pytest.mark.parametrize("K,S,D,n_refine,weighted", ar.REAL_CASES)
def test_real_valued(K, S, D, n_refine, weighted):
    from myfm_amd import _capi

    Vs, w = ar.real_case(K, S, D, weighted)
    ref = ar.align_ref(Vs, -1, n_refine, w)
    got = _capi.align(ar.samples_of(Vs), -1, n_refine, w)
    used = ar.shares(got, ref)
    print("K %d S %d D %d rounds %d weighted %d: used shares %s, orthogonality %.3g of %.3g" % (
        K, S, D, n_refine + 1, weighted, used, _orth_err(got[2]).max(), ar.jacobi_term(K)))
    assert max(used.values()) <= 1.0
    assert _orth_err(got[2]).max() <= ar.jacobi_term(K)
    assert _same(got, _capi.align(ar.samples_of(Vs), -1, n_refine, w, scratch_bound=1))  # (one sample per group: the same sums)


@pytest.mark.parametrize("K,D,zero", [(5, 100, True), (8, 5, False), (33, 20, True)])
def test_singular(K, D, zero):
    """a sample with a zero factor, and D < K: R_s is not unique, so what is unique is judged. R_s orthogonal; tr(R_s^T M_s) =
    sum sigma_i of the reference within sqrt(K) e_M + e_J sum sigma (Mirsky, and |tr((R - R*)^T M)| <= ||R^T R - I|| sum sigma);
    Y_s = R_s^T V_s, which IS unique here because every left null vector of M_s annihilates V_s, within (4 e_M / sigma_r + e_J) ||V_s||,
    sigma_r the least non-zero singular value (the polar bound on the range of M_s, the gap sigma_r + 0 in place of the two least)"""
    from myfm_amd import _capi

    S = 3
    Vs, _ = ar.real_case(K, S, D, False, seed=7)
    if zero:
        Vs[1, K // 2] = 0.0
    ref = ar.align_ref(Vs, -1, 0)
    _, _, R, al = _capi.align(ar.samples_of(Vs), -1, 0)
    assert _orth_err(R).max() <= ar.jacobi_term(K)
    for s in range(S):
        sig, e_M, eJ = ref["sigma"][s], ref["tol"]["e_M"][s], ar.jacobi_term(K)
        assert abs(np.trace(R[s].T @ ref["M"][s]) - sig.sum()) <= np.sqrt(K) * e_M + eJ * sig.sum()
        sig_r = sig[sig > 1e-9 * sig[0]].min()
        tol_Y = (4 * e_M / sig_r + eJ) * np.linalg.norm(Vs[s])
        assert np.linalg.norm(R[s].T @ Vs[s] - ref["rotations"][s].T @ Vs[s]) <= tol_Y
    assert np.all(np.abs(al - ref["alignment"]) <= ref["tol"]["alignment"] + 1e-300)
    zeros = _capi.align(ar.samples_of(np.zeros((2, 3, 7))), 0, 1)  # M = 0: the completion alone
    assert _same(zeros, (np.zeros((7, 3)), np.zeros((7, 3)), np.stack([np.eye(3)] * 2), np.zeros(2)))


def test_sources():
    """a device store and its host copy, and two calls, give the same bits; a range of the store is that range of the samples"""
    from myfm_amd import _capi

    Vs, w = ar.real_case(17, 5, 300, True)
    samples = ar.samples_of(Vs)
    store = _capi.Store(300, 17)
    for smp in samples:
        store.push(*smp)
    host = _capi.align(samples, 2, 1, w)
    assert _same(host, _capi.align_store(store, 2, 1, w)) and _same(host, _capi.align(samples, 2, 1, w))
    assert _same(_capi.align(samples[1:4], -1, 1, w), _capi.align_store(store, -1, 1, w, first=1, count=3))
    store.close()


@pytest.mark.parametrize("kind", ["regressor", "classifier", "ordered"])
def test_estimator_surface(kind, tiny_table):
    """aligned_factors on a fresh fit (device store) equals the _capi call on V_samples; embed; a pickle round trip, a combine_chains
    result, a fold_in result; the host checks; rank 0 and rank 65 through _capi"""
    import myfm_amd
    from myfm_amd import _capi

    X, y, shapes = tiny_table
    est = _fit(kind, X, y, shapes)
    D, w = N_USERS + N_ITEMS, np.r_[np.zeros(N_USERS), np.ones(N_ITEMS)]
    for e in (est, pickle.loads(pickle.dumps(est)), myfm_amd.combine_chains([est, _fit(kind, X, y, shapes, seed=11)])):
        for kw in (dict(), dict(reference=0, n_refine=0, weights=w)):
            got = e.aligned_factors(**kw)
            assert isinstance(got, myfm_amd.AlignedFactors) and got.mean.shape == (D, est.rank)
            assert _same(got, _capi.align([(0.0, np.zeros(D), V) for V in e.V_samples], kw.get("reference", -1), kw.get("n_refine", 1),
                                          kw.get("weights")))
    assert np.array_equal(got.embed(X[:9]), X[:9] @ got.mean)
    if kind == "regressor":
        new = est.fold_in(sps.csr_matrix(([1.0, 1.0], ([0, 1], [N_USERS, N_USERS + 1])), shape=(2, D)), np.ones(2), np.zeros(2, np.int64), 0)
        assert new.aligned_factors().mean.shape == (D + 1, est.rank)
    for bad in (dict(reference=6), dict(reference=-7), dict(n_refine=9), dict(weights=-w), dict(weights=np.full(D, np.inf))):
        with pytest.raises(ValueError):
            est.aligned_factors(**bad)
    with pytest.raises(ValueError):
        _capi.align(ar.samples_of(np.zeros((1, 65, 4))))
    got = _capi.align(ar.samples_of(np.zeros((2, 0, 7))))  # rank 0: empty arrays, no launch
    assert got[0].shape == (7, 0) and got[2].shape == (2, 0, 0) and np.array_equal(got[3], np.zeros(2))
    assert not hasattr(myfm_amd.VariationalFMRegressor, "aligned_factors")
