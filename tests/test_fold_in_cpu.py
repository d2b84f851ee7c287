"""Fold-in of new one-hot entities, the parts that need no GPU: the algebra the device kernel rests on (tests/fold_in_ref.py), the
float64 restatement against the longdouble reference within the tolerance the GPU test uses, the argument checks of
MyFMGibbsRegressor.fold_in, which run on the host before the device is looked for, and the exported symbols."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import fold_in_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NEW_SYMBOLS = ("mfm_foldin_create", "mfm_foldin_destroy", "mfm_foldin_last_error", "mfm_foldin_set_scratch_bound", "mfm_foldin_max_rank",
               "mfm_foldin_solve_store", "mfm_foldin_solve")


def _direct_score(w0, w, V, idx, x):
    """the FM formula on one row given as (columns, values), longdouble"""
    x, wl, Vl = np.asarray(x, dtype=LD), np.asarray(w)[idx].astype(LD), np.asarray(V)[idx].astype(LD)
    q = (x[:, None] * Vl).sum(axis=0)
    return LD(w0) + (x * wl).sum() + ((q * q - ((x * x)[:, None] * Vl * Vl).sum(axis=0)) / 2).sum()


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 3, 8])
def test_algebra_identity(K):
    """score(x + e_u) of the extended sample = f(x) + theta . z, against the direct FM formula on the D + 1 wide row"""
    rng = np.random.default_rng(10 + K)
    D = 12
    p = fr.problem(rng, D, K, 2, 1, counts=[9])
    theta = rng.normal(size=K + 1)
    for sample in p["samples"]:
        z, r = fr.z_and_residual(sample, p["X"], p["y"])
        f = p["y"].astype(LD) - r
        w0, w2, V2 = fr.extend_sample(sample, theta[:1], theta[None, 1:])
        for i in range(p["X"].shape[0]):
            row = p["X"][i]
            idx, x = np.append(row.indices, D), np.append(row.data, 1.0)
            direct = _direct_score(w0, w2, V2, idx, x)
            lin = f[i] + (z[i] * theta.astype(LD)).sum()
            assert abs(direct - lin) <= 1e-16 * (1 + abs(direct)), (i, direct, lin)


@pytest.mark.parametrize("K,fit_linear", [(0, True), (2, True), (5, False), (17, True)])
def test_posterior_mean_maximises_the_log_posterior(K, fit_linear):
    """the gradient of -1/2 alpha sum (r - theta . z)^2 - 1/2 sum lambda (theta - mu)^2 at theta_mean is ~0 in longdouble"""
    rng = np.random.default_rng(20 + K)
    p = fr.problem(rng, 15, K, 2, 4, counts=[0, 3, 40, 65])
    ref = fr.posterior(p, fit_linear)
    o = 0 if fit_linear else 1
    Xg, yg, off = fr.grouped(p["X"], p["y"], p["entity"], 4)
    for s in range(2):
        z, r = fr.z_and_residual(p["samples"][s], Xg, yg)
        z = z[:, o:]
        for u in range(4):
            zu, ru, th = z[off[u]:off[u + 1]], r[off[u]:off[u + 1]], ref["theta"][s, u]
            grad = LD(p["alpha"][s]) * np.dot(zu.T, ru - np.dot(zu, th)) - ref["lam"][s] * (th - ref["mu"][s])
            scale = LD(p["alpha"][s]) * (np.abs(zu) * np.abs(ru)[:, None]).sum(axis=0) + np.abs(ref["lam"][s] * ref["mu"][s]) + 1
            assert np.all(np.abs(grad) <= 1e-15 * scale), (s, u, np.abs(grad / scale).max())
            if off[u + 1] == off[u]:
                assert np.array_equal(th, ref["mu"][s])


def test_rank_zero_closed_form():
    rng = np.random.default_rng(3)
    p = fr.problem(rng, 9, 0, 3, 5, counts=[0, 1, 7, 64, 0])
    ref = fr.posterior(p, True)
    Xg, yg, off = fr.grouped(p["X"], p["y"], p["entity"], 5)
    for s in range(3):
        _, r = fr.z_and_residual(p["samples"][s], Xg, yg)
        for u in range(5):
            n = off[u + 1] - off[u]
            lam, mu, a = LD(p["lam"][s, 0]), LD(p["mu"][s, 0]), LD(p["alpha"][s])
            want = (lam * mu + a * r[off[u]:off[u + 1]].sum()) / (lam + a * n)
            assert abs(ref["theta"][s, u, 0] - want) <= 4e-19 * (abs(want) + 1)
    # without the linear term and without factors there is nothing to estimate
    none = fr.posterior(p, False)
    assert none["theta"].shape == (3, 5, 0)


@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("K", [0, 1, 3, 4, 15, 16, 17, 31, 33, 63, 64])
def test_float64_restatement_stays_within_the_tolerance(K, fit_linear):
    """what the GPU test asks of the kernel is attainable in float64: np.linalg.cholesky and two solves stay inside
    16 (K + 1 + n) 2^-52 cond max(|theta|, |mu|) of the longdouble reference, means and draws, rows {0 .. 257}"""
    rng = np.random.default_rng(500 + 2 * K + fit_linear)
    p = fr.problem(rng, 40, K, 2, 7)
    assert 0 in p["counts"] and p["counts"].max() >= 64
    ref = fr.posterior(p, fit_linear)
    M = ref["theta"].shape[-1]
    if M == 0:
        return
    assert ref["cond"].max() <= 1e5
    got = fr.posterior_f64(p, fit_linear)
    tol = fr.tolerance(ref, K)
    err = np.abs(got - ref["theta"]).max(axis=-1).astype(np.float64)
    assert np.all(err <= tol), (err / tol).max()
    empty = p["counts"] == 0
    assert empty.any() and np.array_equal(got[:, empty], np.broadcast_to(ref["mu"][:, None, :].astype(np.float64), got[:, empty].shape))
    eps = fr.normals(7, 2, 7, M)
    want = fr.drawn(ref, eps)
    got = fr.posterior_f64(p, fit_linear, eps)
    tol = fr.tolerance(ref, K, want)
    err = np.abs(got - want).max(axis=-1).astype(np.float64)
    assert np.all(err <= tol), (err / tol).max()


def test_normals_are_standard_and_keyed_by_row():
    eps = fr.normals(11, 40, 50, 33)
    assert abs(eps.mean()) < 0.01 and abs(eps.std() - 1.0) < 0.01
    # the stream of (s, u) is row s U + u: U = 50 row 120 is (2, 20); U = 60 row 120 is (2, 0)
    other = fr.normals(11, 40, 60, 33)
    assert np.array_equal(eps[2, 20], other[2, 0]) and not np.array_equal(eps[2, 20], other[2, 20])
    assert np.array_equal(fr.normals(11, 3, 4, 6)[..., :5], fr.normals(11, 3, 4, 5))  # component j does not depend on M
    assert not np.array_equal(fr.normals(12, 3, 4, 5), fr.normals(11, 3, 4, 5))
    with open(os.path.join(ROOT, "myfm_amd", "csrc", "mfm_foldin.hpp")) as f:
        assert "FOLDIN_DRAW_TAG = 0x%Xull" % fr.FOLDIN_DRAW_TAG in f.read()


# ---- argument validation: an estimator restored by __setstate__, no fit, no device ---------------------------------------------
def _restored(D=6, K=3, S=2, G=2, with_history=True, fit_linear=True):
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    fms = []
    for _ in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(_myfm.TaskType.REGRESSION), fms))
    est = myfm_amd.MyFMRegressor(K, fit_linear=fit_linear)
    est.predictor_ = p
    est.n_groups_ = G
    if with_history:
        hypers = []
        for _ in range(S + 1):
            h = _myfm.FMHyperParameters.__new__(_myfm.FMHyperParameters)
            h.__setstate__((1.5, rng.normal(size=G), rng.uniform(1, 2, size=G), rng.normal(size=(G, K)), rng.uniform(1, 2, size=(G, K))))
            hypers.append(h)
        hist = _myfm.LearningHistory.__new__(_myfm.LearningHistory)
        hist.__setstate__((hypers, [], []))
        est.history_ = hist
    return est


def test_argument_checks_need_no_gpu():
    import myfm_amd
    from myfm_amd import _myfm

    est = _restored()
    X = sps.csr_matrix(np.eye(4, 6))
    y, ent = np.arange(4.0), np.array([1, 0, 1, 2])
    with pytest.raises(ValueError, match="X has 5 columns but the fitted feature size is 6"):
        est.fold_in(sps.csr_matrix((4, 5)), y, ent, 0)
    with pytest.raises(ValueError, match="X has 7 columns"):  # the new entity's own column does not belong in X
        est.fold_in(sps.csr_matrix((4, 7)), y, ent, 0)
    with pytest.raises(ValueError, match="scipy sparse"):
        est.fold_in(np.eye(4, 6), y, ent, 0)
    with pytest.raises(ValueError, match="X has 4 rows but y has 3"):
        est.fold_in(X, y[:3], ent, 0)
    with pytest.raises(ValueError, match="X has 4 rows but entity has shape"):
        est.fold_in(X, y, ent[:3], 0)
    with pytest.raises(ValueError, match="negative index"):
        est.fold_in(X, y, np.array([1, -1, 0, 0]), 0)
    with pytest.raises(ValueError, match="entity holds index 2 but n_entities is 2"):
        est.fold_in(X, y, ent, 0, n_entities=2)
    with pytest.raises(ValueError, match="must hold integers"):
        est.fold_in(X, y, ent * 0.5, 0)
    with pytest.raises(ValueError, match="an empty entity array needs n_entities"):
        est.fold_in(sps.csr_matrix((0, 6)), np.zeros(0), np.zeros(0, dtype=np.int64), 0)
    with pytest.raises(ValueError, match="n_entities must be"):
        est.fold_in(X, y, ent, 0, n_entities=-1)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="y holds a value that is not finite"):
            est.fold_in(X, np.array([0.0, bad, 1.0, 2.0]), ent, 0)
    for g in (-1, 2, 1.0, True, None):
        with pytest.raises(ValueError, match=r"group must be an integer in \[0, 2\)"):
            est.fold_in(X, y, ent, g)
    # the rank limit: an exported constant, at least 64, the library's own
    assert myfm_amd.FOLD_IN_MAX_RANK >= 64
    from myfm_amd import _capi

    assert _capi.lib().mfm_foldin_max_rank() == myfm_amd.FOLD_IN_MAX_RANK
    big = _restored(D=6, K=myfm_amd.FOLD_IN_MAX_RANK + 1, S=1)
    with pytest.raises(ValueError, match="fold_in serves ranks up to 64, this model has rank 65"):
        big.fold_in(X, y, ent, 0)
    # a missing history is predict_dist(noise=True)'s RuntimeError; before fit, the usual one
    with pytest.raises(RuntimeError, match="history_"):
        _restored(with_history=False).fold_in(X, y, ent, 0)
    with pytest.raises(RuntimeError, match="before fit"):
        myfm_amd.MyFMRegressor(2).fold_in(X, y, ent, 0)
    # only the Gibbs regressor folds in
    for cls in ("MyFMClassifier", "MyFMOrderedProbit", "VariationalFMRegressor", "VariationalFMClassifier"):
        assert not hasattr(getattr(myfm_amd, cls), "fold_in")
    # valid arguments: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fold_in(X, y, ent, 1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fold_in(X, y, ent, np.int64(0), n_entities=9, draw=True, random_seed=3)


def test_capi_argument_checks_need_no_gpu():
    """mfm_foldin_create checks its arrays before it looks for a device"""
    from myfm_amd import _capi

    L = _capi.lib()
    import ctypes as C

    def create(ip, ix, dv, y, off, D=4):
        h = C.c_void_p()
        ip, off = np.asarray(ip, dtype=np.int64), np.asarray(off, dtype=np.int64)
        ix, dv, y = np.asarray(ix, dtype=np.int32), np.asarray(dv, dtype=np.float64), np.asarray(y, dtype=np.float64)
        rc = L.mfm_foldin_create(0, D, ip.shape[0] - 1, _capi._p(ip), _capi._p(ix), _capi._p(dv), _capi._p(y), off.shape[0] - 1,
                                 _capi._p(off), 1, C.byref(h))
        msg = L.mfm_foldin_last_error(None).decode()
        if rc == 0:
            L.mfm_foldin_destroy(h)
        return rc, msg

    assert create([0, 1, 2], [0, 4], [1, 1], [0, 0], [0, 2]) == (_capi.MFM_ERR_INVALID, "fold-in X: column index out of range")
    assert create([0, 2, 1], [0, 1], [1, 1], [0, 0], [0, 2])[0] == _capi.MFM_ERR_INVALID
    assert create([0, 1, 2], [0, 1], [1, 1], [0, 0], [0, 1])[1].startswith("fold-in: the entity offsets must run from 0")
    assert create([0, 1, 2], [0, 1], [1, 1], [0, 0], [0, 2, 1, 2])[1].endswith("must be non-decreasing")
    assert create([0, 1, 2], [0, 1], [1, 1], [0, np.nan], [0, 2])[1] == "fold-in: y holds a value that is not finite"
    assert create([0, 1, 2], [0, 1], [1, np.inf], [0, 0], [0, 2])[0] == _capi.MFM_ERR_INVALID
    if L.mfm_device_count() == 0:
        rc, msg = create([0, 1, 2], [0, 1], [1, 1], [0, 0], [0, 0, 2])
        assert rc == _capi.MFM_ERR_DEVICE and "no CPU fallback" in msg


def test_group_by_entity_is_stable():
    from myfm_amd import _capi

    X = sps.csr_matrix(np.arange(12.0).reshape(6, 2))
    Xg, yg, off = _capi.group_by_entity(X, np.arange(6.0), [2, 0, 2, 3, 0, 2], 5)
    assert list(yg) == [1, 4, 0, 2, 5, 3] and list(off) == [0, 2, 2, 5, 6, 6]
    assert np.array_equal(Xg.toarray()[:, 0], 2 * yg)
    X2, y2, off2 = fr.grouped(X, np.arange(6.0), [2, 0, 2, 3, 0, 2], 5)
    assert np.array_equal(y2, yg) and np.array_equal(off2, off) and np.array_equal(X2.toarray(), Xg.toarray())


# ---- the exports ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi, _myfm

    with open(os.path.join(ROOT, "include", "myfm_hip.h")) as f:
        declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", f.read()))
    L = _capi.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.FoldIn.solve) and callable(_capi.FoldIn.solve_store)
    assert callable(myfm_amd.MyFMGibbsRegressor.fold_in)
    assert hasattr(_myfm.Predictor, "fold_in_solve") and hasattr(_myfm.Predictor, "extended")
