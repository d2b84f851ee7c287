"""Variational FM surface that needs no GPU: the truncated-normal moments binding against scipy, the exported names and C ABI
symbols, the pickle states of the reference (cpp_source/declare_module.hpp:194-404), the initial weights and the estimators
before fit."""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps
from scipy import special

import myfm_amd
from myfm_amd import _myfm

from . import vb_ref


def _scipy_moments(mu):
    r = np.exp(-mu * mu / 2 - special.log_ndtr(mu)) / np.sqrt(2 * np.pi)  # phi / Phi
    return mu + r, 1 - mu * r - r * r, np.log(2.0) + special.log_ndtr(mu)


@pytest.mark.parametrize("side", ["left", "right"])
def test_truncated_normal_moments_match_scipy(side):
    fn = getattr(_myfm, "mean_var_truncated_normal_" + side)
    for mu in np.linspace(-40, 40, 801):
        m, v, lz = fn(float(mu))
        em, ev, elz = _scipy_moments(mu if side == "left" else -mu)
        if side == "right":
            em = -em
        # mean = mu + phi / Phi cancels for mu << 0 (on both sides): absolute, relative to the terms' size
        np.testing.assert_allclose(m, em, rtol=1e-12, atol=1e-12 * (1 + abs(mu)))
        np.testing.assert_allclose(lz, elz, rtol=1e-12, atol=1e-15)
        # var = 1 - mu r - r^2 cancels for mu << 0 (both sides lose the same digits): relative to the terms' size
        np.testing.assert_allclose(v, ev, rtol=0, atol=1e-12 * (1 + mu * mu))


def test_exports():
    for name in ("VariationalFMRegressor", "VariationalFMClassifier"):
        assert name in myfm_amd.__all__ and hasattr(myfm_amd, name)
    for name in ("VariationalFM", "VariationalFMHyperParameters", "VariationalPredictor", "VariationalFMTrainer",
                 "VariationalLearningHistory", "create_train_vfm", "mean_var_truncated_normal_left",
                 "mean_var_truncated_normal_right"):
        assert hasattr(_myfm, name), name
    from myfm_amd import _capi

    L = _capi.lib()
    for s in _capi.SYMBOLS:
        if s.startswith("mfm_vb_"):
            assert hasattr(L, s), s


def _vfm(D=5, K=3, seed=0):
    rs = np.random.RandomState(seed)
    return (0.3, 0.7, rs.randn(D), rs.rand(D), rs.randn(D, K), rs.rand(D, K))


def test_variational_fm_pickle_states():
    st = _vfm()
    fm = _myfm.VariationalFM.__new__(_myfm.VariationalFM)
    fm.__setstate__(st)  # the 6-tuple of earlier versions
    for got, want in zip((fm.w0, fm.w0_var, fm.w, fm.w_var, fm.V, fm.V_var), st):
        np.testing.assert_array_equal(got, want)
    assert list(fm.cutpoints) == []
    state = fm.__getstate__()
    assert len(state) == 7
    fm2 = pickle.loads(pickle.dumps(fm))
    for a in ("w0", "w0_var", "w", "w_var", "V", "V_var"):
        np.testing.assert_array_equal(getattr(fm2, a), getattr(fm, a))
    assert repr(fm2) == "<Factorization Machine sample with feature size = 5, rank = 3>"
    with pytest.raises(RuntimeError):
        _myfm.VariationalFM.__new__(_myfm.VariationalFM).__setstate__((1.0, 2.0))


def test_hyper_predictor_history_pickle_states():
    rs = np.random.RandomState(1)
    G, K = 2, 3
    st = (1.5, 2.5, rs.randn(G), rs.rand(G), rs.rand(G), rs.rand(G), rs.randn(G, K), rs.rand(G, K), rs.rand(G, K),
          rs.rand(G, K))
    h = _myfm.VariationalFMHyperParameters.__new__(_myfm.VariationalFMHyperParameters)
    h.__setstate__(st)
    h2 = pickle.loads(pickle.dumps(h))
    names = ("alpha", "alpha_rate", "mu_w", "mu_w_var", "lambda_w", "lambda_w_rate", "mu_V", "mu_V_var", "lambda_V",
             "lambda_V_rate")
    assert len(h.__getstate__()) == 10
    for n, want in zip(names, st):
        np.testing.assert_array_equal(getattr(h2, n), want)

    fm = _myfm.VariationalFM.__new__(_myfm.VariationalFM)
    fm.__setstate__(_vfm())
    p = _myfm.VariationalPredictor.__new__(_myfm.VariationalPredictor)
    p.__setstate__((3, 5, 0, [fm]))
    p2 = pickle.loads(pickle.dumps(p))
    assert len(p2.__getstate__()) == 4
    np.testing.assert_array_equal(p2.weights().V, fm.V)

    gh = _myfm.FMHyperParameters.__new__(_myfm.FMHyperParameters)
    gh.__setstate__((1.0, np.zeros(G), np.ones(G), np.zeros((G, K)), np.ones((G, K))))
    hist = _myfm.VariationalLearningHistory.__new__(_myfm.VariationalLearningHistory)
    hist.__setstate__((gh, [1.0, 2.0]))
    hist2 = pickle.loads(pickle.dumps(hist))
    assert list(hist2.elbos) == [1.0, 2.0]
    assert hist2.hypers.alpha == 1.0


def _config(D, task=_myfm.TaskType.REGRESSION):
    b = _myfm.ConfigBuilder()
    b.set_identical_groups(D).set_n_iter(3).set_n_kept_samples(3).set_task_type(task)
    return b.build()


def test_initial_weights_reassign_the_gibbs_stream():
    X = sps.random(30, 7, density=0.3, format="csr", random_state=3)
    y = np.arange(30.0)
    cfg = _config(7)
    fm = _myfm.VariationalFMTrainer(X, [], y, 11, cfg).create_FM(4, 0.2)
    w0, w, V = vb_ref.initial_weights(X, y, 4, 0.2, 11)  # (the CPU oracle's Gibbs start)
    assert fm.w0 == w0 and fm.w0_var == 1
    np.testing.assert_array_equal(fm.w, w)
    np.testing.assert_array_equal(fm.V, V)
    np.testing.assert_array_equal(fm.w_var, np.full(7, 0.2 * 0.2))
    np.testing.assert_array_equal(fm.V_var, np.full((7, 4), 0.2 * 0.2))
    h = _myfm.VariationalFMTrainer(X, [], y, 11, cfg).create_Hyper(4)
    assert h.mu_V.shape == (1, 4)


@pytest.mark.parametrize("cls", ["VariationalFMRegressor", "VariationalFMClassifier"])
def test_estimator_properties_none_before_fit(cls):
    est = getattr(myfm_amd, cls)(3)
    for a in ("w0_mean", "w0_var", "w_mean", "w_var", "V_mean", "V_var"):
        assert getattr(est, a) is None
    with pytest.raises(RuntimeError):
        est.predict(sps.csr_matrix(np.ones((2, 3))))


def test_vb_ref_truncated_normal_matches_binding():
    mus = np.linspace(-30, 30, 121)
    for side in ("left", "right"):
        m, v, lz = getattr(vb_ref, "truncated_normal_" + side)(mus)
        fn = getattr(_myfm, "mean_var_truncated_normal_" + side)
        got = np.array([fn(float(u)) for u in mus])
        np.testing.assert_allclose(got[:, 0], m, rtol=1e-12, atol=1e-12 * (1 + np.abs(mus)).max())
        np.testing.assert_allclose(got[:, 2], lz, rtol=1e-12, atol=1e-15)


def _block_design(N=1000, seed=1):
    # tests/regression/test_block.py:10-77 of the reference
    rns = np.random.RandomState(seed)
    ub = sps.csr_matrix([[1, 0, 1], [0, 1, 1], [1, 1, 0]], dtype=np.float64)
    ui = rns.randint(0, 3, size=N)
    ib = sps.csr_matrix([[1, 0, 0, 1], [0, 1, 1, 0]], dtype=np.float64)
    ii = rns.randint(0, 2, size=N)
    tm = sps.csr_matrix(rns.randn(N, 1))
    y = rns.randn(N) + 3.0
    return tm, [(ui, ub), (ii, ib)], sps.hstack([tm, ub[ui], ib[ii]]).tocsr(), y


@pytest.mark.parametrize("task", ["regression", "classification"])
def test_vb_ref_flat_equals_blocked(task):
    tm, blocks, Xf, y = _block_design()
    if task == "classification":
        y = np.where(y > np.median(y), 1.0, -1.0)
    rs = np.random.RandomState(0)
    w, V = rs.randn(8) * 0.1, rs.randn(8, 3) * 0.1
    gi = np.r_[0, 1, 1, 1, 2, 2, 2, 2]
    flat = vb_ref.VBRef(Xf, y, 3, gi, task, vb_ref.Config(), 0.05, w, V, 0.1)
    blk = vb_ref.VBRef(tm, y, 3, gi, task, vb_ref.Config(), 0.05, w, V, 0.1, blocks=blocks)
    for _ in range(20):
        flat.iterate()
        blk.iterate()
    for a in ("w", "w_var", "V", "V_var", "e"):
        np.testing.assert_allclose(getattr(blk, a), getattr(flat, a), rtol=1e-9, atol=1e-9 * np.abs(getattr(flat, a)).max())
    hf, hb = flat.hyper(), blk.hyper()
    for k in hf:
        np.testing.assert_allclose(hb[k], hf[k], rtol=1e-9)
    np.testing.assert_allclose(blk.elbos, flat.elbos, rtol=1e-9)


def test_initial_weights_with_blocks_follow_the_flat_stream():
    tm, blocks, Xf, y = _block_design(200)
    a = vb_ref.initial_weights(tm, y, 3, 0.1, 5, blocks)
    b = vb_ref.initial_weights(Xf, y, 3, 0.1, 5)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    rels = [myfm_amd.RelationBlock(mp, B) for mp, B in blocks]
    fm = _myfm.VariationalFMTrainer(tm, rels, y, 5, _config(8)).create_FM(3, 0.1)
    np.testing.assert_array_equal(fm.V, a[2])


def test_variational_estimators_are_not_gibbs_estimators():
    for cls, gibbs in ((myfm_amd.VariationalFMRegressor, myfm_amd.MyFMGibbsRegressor),
                       (myfm_amd.VariationalFMClassifier, myfm_amd.MyFMGibbsClassifier)):
        est = cls(3)
        assert not isinstance(est, gibbs)
        for name in ("w0_samples", "w_samples", "V_samples", "get_hyper_trace", "exact_latent_draws"):
            assert not hasattr(est, name), name
