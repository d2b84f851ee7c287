"""Variational FM on the device (csrc/mfm_vb.hip behind create_train_vfm) against the NumPy restatement of the reference's
VariationalFMTrainer (tests/vb_ref.py): every model field, all ten hyper-parameter fields and the ELBOs after 1 and 10
iterations, over regression and classification, several group layouts, ranks 0 / 1 / 4, fit_w0 / fit_linear off; the
estimators' predictions against the closed-form score of the mean model; bit-identical reruns."""
import numpy as np
import pytest
import scipy.sparse as sps
from scipy import special

import myfm_amd
from myfm_amd import _myfm
from myfm_amd.utils import synthetic

from . import vb_ref

pytestmark = pytest.mark.gpu

HYPER = ("alpha", "alpha_rate", "mu_w", "mu_w_var", "lambda_w", "lambda_w_rate", "mu_V", "mu_V_var", "lambda_V", "lambda_V_rate")


def _onehot(N, sizes, seed, values=False):
    rs = np.random.RandomState(seed)
    cols, off = [], 0
    for s in sizes:
        cols.append(rs.randint(0, s, N) + off)
        off += s
    idx = np.stack(cols, 1).ravel()
    data = rs.choice([1.0, -1.0, 2.0, -2.0, 0.5], size=idx.size) if values else np.ones(idx.size)
    X = sps.csr_matrix((data, idx, np.arange(0, idx.size + 1, len(sizes))), shape=(N, off))
    X.sort_indices()
    return X


def _toy():
    # BASELINE configs[0] (examples/toy.py)
    X, _ = synthetic.toy()
    return X, np.array([5.0, 3.0, 2.0, 1.0])


def _config(gi, task, n_iter, fit_w0=True, fit_linear=True, alpha_0=1.0, beta_0=1.0, gamma_0=1.0, mu_0=0.0, reg_0=1.0):
    b = _myfm.ConfigBuilder()
    b.set_alpha_0(alpha_0).set_beta_0(beta_0).set_gamma_0(gamma_0).set_mu_0(mu_0).set_reg_0(reg_0)
    b.set_fit_w0(fit_w0).set_fit_linear(fit_linear)
    b.set_group_index([int(g) for g in gi]).set_n_iter(n_iter).set_n_kept_samples(n_iter).set_task_type(task)
    return b.build()


def _run(X, y, rank, gi, task, n_iter, seed=7, init_std=0.1, blocks=(), **kw):
    cfg = _config(gi, task, n_iter, **kw)
    hyp = {}

    def cb(i, fm, hyper, hist):
        for n in HYPER:
            hyp[n] = np.array(getattr(hyper, n))
        return False

    rels = [myfm_amd.RelationBlock(mp, B) for mp, B in blocks]
    pred, hist = _myfm.create_train_vfm(rank, init_std, X, rels, y, seed, cfg, cb)
    w0, w, V = vb_ref.initial_weights(X, y, rank, init_std, seed, blocks)
    ref = vb_ref.VBRef(X, y, rank, gi, "classification" if task == _myfm.TaskType.CLASSIFICATION else "regression",
                       vb_ref.Config(fit_w0=kw.get("fit_w0", True), fit_linear=kw.get("fit_linear", True)), w0, w, V, init_std,
                       blocks=blocks)
    for _ in range(n_iter):
        ref.iterate()
    return pred, hist, hyp, ref


def _close(got, want, rtol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if got.size == 0:
        return
    scale = np.max(np.abs(want[np.isfinite(want)])) if np.isfinite(want).any() else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale)


def _check(pred, hist, hyp, ref, rtol):
    fm = pred.weights()
    _close(fm.w0, ref.w0, rtol)
    _close(fm.w0_var, ref.w0_var, rtol)
    _close(fm.w, ref.w, rtol)
    _close(fm.w_var, ref.w_var, rtol)
    _close(fm.V, ref.V, rtol)
    _close(fm.V_var, ref.V_var, rtol)
    want = ref.hyper()
    for n in HYPER:
        _close(hyp[n], want[n], rtol)
    elbos = np.asarray(hist.elbos)
    assert elbos.shape == (len(ref.elbos),)
    fin = np.isfinite(ref.elbos)
    assert np.array_equal(np.isfinite(elbos), fin) and np.array_equal(elbos[~fin], np.asarray(ref.elbos)[~fin])
    if fin.any():
        np.testing.assert_allclose(elbos[fin], np.asarray(ref.elbos)[fin], rtol=rtol * 10)
    _close(hist.hypers.alpha, want["alpha"], rtol)
    _close(hist.hypers.mu_V, want["mu_V"], rtol)


def _cases():
    X2 = _onehot(3000, [40, 60], 1)
    X2v = _onehot(3000, [40, 60], 2, values=True)
    X3 = _onehot(2000, [20, 30, 25], 3, values=True)
    X3 = sps.hstack([X3, sps.csr_matrix((2000, 4))]).tocsr()  # four unused features
    rs = np.random.RandomState(5)
    y2 = rs.randn(3000) + 1.0
    y3 = rs.choice([-2.0, -1.0, 1.0, 2.0], 2000)
    gi3 = np.r_[np.zeros(20), np.ones(30), np.full(25, 2), np.full(4, 2)]
    Xt, yt = _toy()
    return {
        "toy": (Xt, yt, 4, np.zeros(9), {}),
        "onehot_unit": (X2, y2, 4, np.r_[np.zeros(40), np.ones(60)], {}),
        "onehot_values": (X2v, y2, 4, np.r_[np.zeros(40), np.ones(60)], {}),
        "three_groups_unused": (X3, y3, 4, gi3, {}),
        "rank0": (X2v, y2, 0, np.r_[np.zeros(40), np.ones(60)], {}),
        "rank1": (X3, y3, 1, gi3, {}),
        "no_w0": (X2v, y2, 3, np.r_[np.zeros(40), np.ones(60)], {"fit_w0": False}),
        "no_linear": (X2v, y2, 3, np.r_[np.zeros(40), np.ones(60)], {"fit_linear": False}),
        "blocks_test_block": _test_block_design(),
        "blocks_multihot": _multihot_design(),
    }


def _test_block_design(N=1000):
    # tests/regression/test_block.py:10-77 of the reference
    rns = np.random.RandomState(1)
    ub = sps.csr_matrix([[1, 0, 1], [0, 1, 1], [1, 1, 0]], dtype=np.float64)
    ui = rns.randint(0, 3, size=N)
    ib = sps.csr_matrix([[1, 0, 0, 1], [0, 1, 1, 0]], dtype=np.float64)
    ii = rns.randint(0, 2, size=N)
    tm = sps.csr_matrix(rns.randn(N, 1))
    y = rns.randn(N) + 3.0
    return tm, y, 3, np.r_[0, 1, 1, 1, 2, 2, 2, 2], {"blocks": [(ui, ub), (ii, ib)]}


def _multihot_design(N=4000, U=60, I=45, seed=6):
    # shaped like ML-100k-extended: user and item one-hot in the main table, a user block holding a normalised multi-hot
    # row of rated items (implicit feedback), an item block holding multi-hot side information
    rs = np.random.RandomState(seed)
    u, i = rs.randint(0, U, N), rs.randint(0, I, N)
    X = sps.csr_matrix((np.ones(2 * N), np.stack([u, U + i], 1).ravel(), np.arange(0, 2 * N + 1, 2)), shape=(N, U + I))

    def multihot(rows, cols, lo, hi):
        m = sps.lil_matrix((rows, cols))
        for r in range(rows):
            c = rs.choice(cols, rs.randint(lo, hi + 1), replace=False)
            m[r, c] = 1.0 / np.sqrt(max(1, len(c)))
        return m.tocsr()

    ub, ib = multihot(U, I, 0, 8), multihot(I, 12, 1, 3)
    y = rs.randn(N) + 2.0
    gi = np.r_[np.zeros(U), np.ones(I), np.full(I, 2), np.full(12, 3)]
    return X, y, 4, gi, {"blocks": [(u, ub), (i, ib)]}


@pytest.mark.parametrize("task", ["regression", "classification"])
@pytest.mark.parametrize("name", list(_cases()))
@pytest.mark.parametrize("n_iter,rtol", [(1, 1e-9), (10, 1e-7)])
def test_chain_matches_reference(name, task, n_iter, rtol):
    X, y, rank, gi, kw = _cases()[name]
    tt = _myfm.TaskType.REGRESSION
    if task == "classification":
        tt = _myfm.TaskType.CLASSIFICATION
        y = np.where(y > np.median(y), 1.0, -1.0)
    pred, hist, hyp, ref = _run(X, y, rank, gi, tt, n_iter, **kw)
    _check(pred, hist, hyp, ref, rtol)
    if not kw.get("fit_w0", True):
        assert np.all(np.isneginf(hist.elbos))


def test_ordered_raises_the_reference_error():
    X, y = _toy()
    cfg = _config(np.zeros(9), _myfm.TaskType.ORDERED, 2)
    with pytest.raises(RuntimeError, match="Ordered Probit Regression  for Variational FM not implemented"):
        _myfm.create_train_vfm(2, 0.1, X, [], np.array([0.0, 1.0, 2.0, 1.0]), 1, cfg, lambda *a: False)


def test_duplicate_entries_are_refused():
    X = sps.csr_matrix((np.ones(3), np.array([0, 0, 1]), np.array([0, 2, 3])), shape=(2, 2))  # row 0 holds column 0 twice
    with pytest.raises(ValueError, match="same column twice"):
        _myfm.create_train_vfm(1, 0.1, X, [], np.ones(2), 1, _config(np.zeros(2), _myfm.TaskType.REGRESSION, 1),
                               lambda *a: False)


def test_block_estimator_flat_equals_blocked_after_pickling():
    # tests/regression/test_block.py:10-77 of the reference (n_iter 100)
    import pickle

    tm, y, _, _, kw = _test_block_design()
    (ui, ub), (ii, ib) = kw["blocks"]
    Xf = sps.hstack([tm, ub[ui], ib[ii]]).tocsr()
    blocks = pickle.loads(pickle.dumps([myfm_amd.RelationBlock(ui, ub), myfm_amd.RelationBlock(ii, ib)]))
    flat = myfm_amd.VariationalFMRegressor(3).fit(Xf, y, n_iter=100)
    blk = pickle.loads(pickle.dumps(myfm_amd.VariationalFMRegressor(3).fit(tm, y, blocks, n_iter=100)))
    np.testing.assert_allclose(blk.w_mean, flat.w_mean, rtol=1e-7)
    np.testing.assert_allclose(blk.V_mean, flat.V_mean, rtol=1e-7, atol=1e-7 * np.abs(flat.V_mean).max())
    np.testing.assert_allclose(flat.predict(tm, blocks), blk.predict(Xf), rtol=1e-7)


@pytest.mark.parametrize("alpha_inv", [0.3, 1.0, 3])
def test_middle_reg(alpha_inv):
    # the VB half of tests/regression/test_fit.py:19-72 of the reference
    X, score = synthetic.middle_data()
    rns = np.random.RandomState(0)
    y = score + alpha_inv * rns.normal(0, 1, size=score.shape)
    vfm = myfm_amd.VariationalFMRegressor(3).fit(X, y, X_test=X, y_test=y, n_iter=50)
    V = vfm.predictor_.weights().V
    F = synthetic.STUB_V
    for i in range(3):
        for j in range(i + 1, 3):
            cross = F[:, i].dot(F[:, j])
            if abs(cross) < 0.1:
                continue
            sign = cross / abs(cross)
            assert sign * cross * 0.8 < V[i].dot(V[j]) < sign * cross * 1.25


def test_middle_clf():
    # the VB half of tests/classification/test_classification.py:13-70 of the reference
    X, score = synthetic.middle_data()
    rns = np.random.RandomState(0)
    s = score + rns.normal(0, 1, size=score.shape)
    s -= s.mean()
    y = s > 0
    vfm = myfm_amd.VariationalFMClassifier(3).fit(X, y, X_test=X, y_test=y, n_iter=200)
    for a in ("w0_mean", "w0_var", "w_mean", "w_var", "V_mean", "V_var"):
        assert getattr(vfm, a) is not None
    F = synthetic.STUB_V
    for i in range(3):
        for j in range(i + 1, 3):
            cross = F[:, i].dot(F[:, j])
            if abs(cross) < 0.5:
                continue
            sign = cross / abs(cross)
            assert sign * cross * 0.8 < vfm.V_mean[i].dot(vfm.V_mean[j]) < sign * cross * 1.2


def test_middle_size_parity():
    X = _onehot(200_000, [1000, 2000], 9, values=True)
    rs = np.random.RandomState(4)
    y = rs.randn(200_000)
    gi = np.r_[np.zeros(1000), np.ones(2000)]
    pred, hist, hyp, ref = _run(X, y, 8, gi, _myfm.TaskType.REGRESSION, 3)
    _check(pred, hist, hyp, ref, 1e-8)


def _score(fm, X):
    w0, w, V = fm.w0, np.asarray(fm.w), np.asarray(fm.V)
    XV = X @ V
    return w0 + X @ w + 0.5 * ((XV**2).sum(1) - (X.multiply(X) @ (V**2)).sum(1))


def test_estimators_predict_the_mean_model_and_rerun_bit_identical():
    X = _onehot(5000, [50, 80], 11, values=True)
    rs = np.random.RandomState(2)
    y = rs.randn(5000)
    Xte = _onehot(700, [50, 80], 12, values=True)
    est = myfm_amd.VariationalFMRegressor(4, random_seed=3).fit(X, y, n_iter=8, group_shapes=[50, 80])
    fm = est.predictor_.weights()
    np.testing.assert_allclose(est.predict(Xte), _score(fm, Xte), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(fm.predict_score(Xte, []), _score(fm, Xte), rtol=1e-10, atol=1e-10)
    assert est.w_mean.shape == (130,) and est.V_var.shape == (130, 4) and est.w0_var > 0
    est2 = myfm_amd.VariationalFMRegressor(4, random_seed=3).fit(X, y, n_iter=8, group_shapes=[50, 80])
    for a in ("w0_mean", "w0_var", "w_mean", "w_var", "V_mean", "V_var"):
        assert np.array_equal(getattr(est, a), getattr(est2, a)), a
    assert np.array_equal(est.history_.elbos, est2.history_.elbos)

    yc = (y > 0).astype(int)
    clf = myfm_amd.VariationalFMClassifier(4, random_seed=3).fit(X, yc, n_iter=8, X_test=Xte, y_test=(Xte.sum(1).A1 > 0))
    fmc = clf.predictor_.weights()
    p = clf.predict_proba(Xte)
    np.testing.assert_allclose(p, special.ndtr(_score(fmc, Xte)), rtol=1e-10, atol=1e-12)
    assert np.array_equal(clf.predict(Xte), p > 0.5)
    import pickle

    clf2 = pickle.loads(pickle.dumps(clf))
    np.testing.assert_array_equal(clf2.predict_proba(Xte), p)


def test_callback_sees_live_model():
    X = _onehot(1000, [20, 30], 13)
    y = np.random.RandomState(0).randn(1000)
    seen = []

    def cb(i, fm, hyper, hist):
        seen.append((i, fm.w0, np.array(fm.V), len(hist.elbos)))
        return i == 2

    pred, hist = _myfm.create_train_vfm(3, 0.1, X, [], y, 5, _config(np.zeros(50), _myfm.TaskType.REGRESSION, 10), cb)
    assert [s[0] for s in seen] == [0, 1, 2] and [s[3] for s in seen] == [1, 2, 3]
    assert len(hist.elbos) == 3
    np.testing.assert_array_equal(seen[-1][2], pred.weights().V)
    assert not np.array_equal(seen[0][2], seen[-1][2])


# ---- single steps through the C ABI (include/myfm_hip.h mfm_vb_*) -----------------------------------------------------------
class _VB:
    def __init__(self, X, y, gi, K, blocks=()):
        import ctypes as C

        from myfm_amd import _capi

        self.C, self.L = C, _capi.lib()
        P, I64, I32, D = C.c_void_p, C.c_int64, C.c_int32, C.c_double
        sig = {
            "mfm_vb_create": [C.c_int, I64, I64, P, P, P, P, P], "mfm_vb_add_block": [P, I64, I64, P, P, P, P],
            "mfm_vb_finalize": [P, P, I32, I32], "mfm_vb_set_state": [P, D, D, P, P, P, P],
            "mfm_vb_get_state": [P, P, P, P, P, P, P], "mfm_vb_update_e": [P, I32, P], "mfm_vb_get_e": [P, P],
            "mfm_vb_get_cache": [P, P, P, P], "mfm_vb_sweep_w": [P, D, P, P], "mfm_vb_sweep_V": [P, I32, I32, D, P, P],
            "mfm_vb_plan_info": [P, P, P], "mfm_vb_synchronize": [P], "mfm_vb_destroy": [P],
        }
        for name, a in sig.items():
            getattr(self.L, name).argtypes = a
        self.L.mfm_vb_last_error.restype = C.c_char_p
        X = sps.csr_matrix(X, dtype=np.float64)
        self.keep = []
        self.h = C.c_void_p()
        self._ok(self.L.mfm_vb_create(0, X.shape[0], X.shape[1], self._p(X.indptr, np.int64), self._p(X.indices, np.int32),
                                      self._p(X.data), self._p(y), C.byref(self.h)))
        for mp, B in blocks:
            B = sps.csr_matrix(B, dtype=np.float64)
            self._ok(self.L.mfm_vb_add_block(self.h, B.shape[0], B.shape[1], self._p(B.indptr, np.int64),
                                             self._p(B.indices, np.int32), self._p(B.data), self._p(mp, np.int64)))
        self.N, self.D, self.K, self.G = X.shape[0], len(gi), K, int(max(gi)) + 1
        self._ok(self.L.mfm_vb_finalize(self.h, self._p(gi, np.int32), self.G, K))

    def _p(self, a, dt=np.float64):
        a = np.ascontiguousarray(a, dtype=dt)
        self.keep.append(a)
        return a.ctypes.data

    def _ok(self, code):
        assert code == 0, self.L.mfm_vb_last_error(self.h if self.h.value else None)

    def set_state(self, w0, w0_var, w, w_var, V, V_var):
        f = lambda a: self._p(np.asarray(a).ravel("F"))  # noqa: E731
        self._ok(self.L.mfm_vb_set_state(self.h, w0, w0_var, f(w), f(w_var), f(V), f(V_var)))

    def state(self):
        w, wv, V, Vv = np.empty(self.D), np.empty(self.D), np.empty(self.D * self.K), np.empty(self.D * self.K)
        self._ok(self.L.mfm_vb_get_state(self.h, None, None, w.ctypes.data, wv.ctypes.data, V.ctypes.data, Vv.ctypes.data))
        return w, wv, V.reshape((self.D, self.K), order="F"), Vv.reshape((self.D, self.K), order="F")

    def update_e(self, mode):
        out = np.empty(4)
        self._ok(self.L.mfm_vb_update_e(self.h, mode, out.ctypes.data))
        return out

    def e(self):
        e = np.empty(self.N)
        self._ok(self.L.mfm_vb_get_e(self.h, e.ctypes.data))
        return e

    def cache(self):
        q, a, b = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        self._ok(self.L.mfm_vb_get_cache(self.h, q.ctypes.data, a.ctypes.data, b.ctypes.data))
        return q, a, b

    def __del__(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.mfm_vb_destroy(self.h)


def _random_state(D, K, seed):
    rs = np.random.RandomState(seed)
    return 0.3, 0.2, rs.randn(D) * 0.3, rs.rand(D) * 0.1, rs.randn(D, K) * 0.3, rs.rand(D, K) * 0.1


@pytest.mark.parametrize("design", ["onehot_values", "blocks_multihot"])
def test_single_steps_match_reference(design):
    X, y, K, gi, kw = _cases()[design]
    blocks = kw.get("blocks", ())
    vb = _VB(X, y, gi, K, blocks)
    D = len(gi)
    n_levels, launches = np.zeros(1, np.int64), np.zeros(1, np.int64)
    vb._ok(vb.L.mfm_vb_plan_info(vb.h, n_levels.ctypes.data, launches.ctypes.data))
    assert n_levels[0] >= 2 and launches[0] > 0
    st = _random_state(D, K, 3)
    vb.set_state(*st)
    ref = vb_ref.VBRef(X, y, K, gi, "regression", vb_ref.Config(), st[0], st[2], st[4], 0.1, blocks=blocks)
    ref.w0_var, ref.w_var[:], ref.V_var[:] = st[1], st[3], st[5]
    score, var = vb_ref.update_e_and_var(ref.Xf, *st)
    ref.e, ref.e_var_sum = score - y, var
    # update_e_and_var
    sums = vb.update_e(0)
    _close(vb.e(), ref.e, 1e-11)
    _close(sums[2], ref.e_var_sum, 1e-11)
    _close(sums[0], ref.e.sum(), 1e-10)
    # update_w
    ref.alpha = 1.7
    ref.lambda_w[:] = np.linspace(0.5, 2.0, ref.G)
    ref.mu_w[:] = np.linspace(-0.1, 0.2, ref.G)
    vb._ok(vb.L.mfm_vb_sweep_w(vb.h, ref.alpha, vb._p(ref.lambda_w), vb._p(ref.mu_w)))
    ref.sweep_w()
    w, wv, V, Vv = vb.state()
    _close(w, ref.w, 1e-10)
    _close(wv, ref.w_var, 1e-10)
    _close(vb.e(), ref.e, 1e-10)
    # one factor of update_V
    ref.lambda_V[:] = np.linspace(0.5, 2.0, ref.G * K).reshape(ref.G, K)
    ref.mu_V[:] = np.linspace(-0.2, 0.1, ref.G * K).reshape(ref.G, K)
    f = 1
    vb._ok(vb.L.mfm_vb_sweep_V(vb.h, f, f + 1, ref.alpha, vb._p(ref.lambda_V.ravel("F")), vb._p(ref.mu_V.ravel("F"))))
    vb._ok(vb.L.mfm_vb_synchronize(vb.h))
    ref.sweep_factor(f)
    w, wv, V, Vv = vb.state()
    _close(V, ref.V, 1e-10)
    _close(Vv, ref.V_var, 1e-10)
    _close(vb.e(), ref.e, 1e-10)
    for got, want in zip(vb.cache(), (ref.q, ref.x2s, ref.x3sv)):
        _close(got, want, 1e-10)


def test_config3_scale():
    # BASELINE configs[2]'s shape at full size: N = 10 M, two one-hot fields, rank 32
    X, y, shapes = synthetic.movielens_like(10_000_000, 69878, 10677, rank_true=32, seed=1)
    gi = synthetic.group_index_from_shapes(shapes)
    D, K = X.shape[1], 32
    vb = _VB(X, y, gi, K)
    st = _random_state(D, K, 8)
    vb.set_state(*st)
    sums = vb.update_e(0)
    e = vb.e()
    # e against the closed-form score - y on 200 k sampled rows
    rows = np.random.RandomState(2).choice(X.shape[0], 200_000, replace=False)
    Xs = X[rows]
    _close(e[rows], synthetic.fm_score(Xs, st[0], st[2], st[4]) - y[rows], 1e-10)
    # e_var_sum against the closed form, factor by factor
    X2 = X.multiply(X).tocsr()
    X3, X4 = X2.multiply(X).tocsr(), X2.multiply(X2).tocsr()
    var = st[1] * X.shape[0] + (X2 @ st[3]).sum()
    for r in range(K):
        v, s = st[4][:, r], st[5][:, r]
        q, x2s = X @ v, X2 @ s
        var += (q * q * x2s + 0.5 * x2s * x2s - 2 * (X3 @ (s * v)) * q - 0.5 * (X4 @ (s * s)) + X4 @ (s * v * v)).sum()
    _close(sums[2], var, 1e-9)
    del vb
    # two iterations, twice: bit-identical
    cfg = _config(gi, _myfm.TaskType.REGRESSION, 2)
    a = _myfm.create_train_vfm(K, 0.1, X, [], y, 42, cfg, lambda *x: False)
    b = _myfm.create_train_vfm(K, 0.1, X, [], y, 42, cfg, lambda *x: False)
    fa, fb = a[0].weights(), b[0].weights()
    for n in ("w0", "w", "w_var", "V", "V_var"):
        assert np.array_equal(getattr(fa, n), getattr(fb, n)), n
    assert np.array_equal(a[1].elbos, b[1].elbos) and np.all(np.isfinite(a[1].elbos))
