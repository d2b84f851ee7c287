"""Row-sharded variational FM on the device (csrc/mfm_vb.hip, the split path behind create_train_vfm_sharded): ranks as
lock-stepped threads on one GPU, every rank held to the NumPy restatement of the reference on the UNSHARDED data
(tests/vb_ref.py) at the tolerances of tests/test_gpu_variational.py; bit-identical replicas and reruns; each rank's residual
through the C ABI; the collective budget; the check of a schedule handed in; the native RCCL provider with a world of 1; and
VariationalFM*.fit() under torch.distributed (tests/mp_vb_fit_worker.py)."""
import ctypes as C
import os
import subprocess
import sys
import threading
import types

import numpy as np
import pytest
import scipy.sparse as sps

import myfm_amd
from myfm_amd import _capi, _myfm

from . import test_gpu_variational as tgv
from . import vb_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ("w0", "w0_var", "w", "w_var", "V", "V_var")


class Lockstep:
    """sums the buffers of `world` contexts living in threads of one process, in rank order on every rank (stand-in for RCCL
    on one GPU)"""

    def __init__(self, world):
        import torch

        self.torch = torch
        self.world = world
        self.bar = threading.Barrier(world)
        self.bufs = [None] * world

    def callback(self, rank):
        from myfm_amd.distributed import _DevView

        def cb(ptr, count):
            torch = self.torch
            torch.cuda.synchronize()
            self.bufs[rank] = torch.as_tensor(_DevView(ptr, count), device="cuda")
            self.bar.wait()
            total = self.bufs[0].clone()
            for b in self.bufs[1:]:
                assert b.shape == total.shape
                total += b
            torch.cuda.synchronize()
            self.bar.wait()
            self.bufs[rank].copy_(total)
            torch.cuda.synchronize()
            self.bar.wait()

        return cb

    def run(self, fn):
        """fn(rank) on one thread per rank; the first failure breaks the barrier, so no rank waits for a dead one"""
        out, errs = [None] * self.world, []

        def body(rank):
            try:
                out[rank] = fn(rank)
            except BaseException as ex:  # noqa: BLE001
                errs.append((rank, ex))
                self.bar.abort()

        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        real = [e for e in errs if not isinstance(e[1], threading.BrokenBarrierError)] or errs
        if real:
            raise real[0][1]
        return out


def _cuts(kind, N):
    return {"world1": [0, N], "balanced2": [0, N // 2, N], "uneven2": [0, (9 * N) // 10, N],
            "empty3": [0, N // 3, N // 3, N]}[kind]


def _run_sharded(X, y, rank, gi, task, n_iter, cuts, blocks=(), seed=7, init_std=0.1, comm_id=None, **kw):
    """one context per shard; per rank (predictor, history, hyper-parameters of the last iteration, snapshot after the first
    iteration, all-reduce calls counted at every iteration)"""
    X = sps.csr_matrix(X, dtype=np.float64)
    world, N = len(cuts) - 1, X.shape[0]
    rels_all = [myfm_amd.RelationBlock(mp, B) for mp, B in blocks]
    levels = _myfm.vb_column_levels(X, rels_all)
    ls = Lockstep(world)

    def one(r):
        lo, hi = cuts[r], cuts[r + 1]
        cfg = tgv._config(gi, task, n_iter, **kw)
        hyp, first, calls = {}, {}, []

        def cb(i, fm, hyper, hist):
            for n in tgv.HYPER:
                hyp[n] = np.array(getattr(hyper, n))
            calls.append(fm.comm_stats()[0])
            if i == 0:
                first.update({a: np.array(getattr(fm, a)) for a in MODEL})
                first["hyper"] = dict(hyp)
                first["elbos"] = list(hist.elbos)
            return False

        rels = [myfm_amd.RelationBlock(np.asarray(mp)[lo:hi], B) for mp, B in blocks]
        prov = dict(comm_id=comm_id) if comm_id is not None else dict(allreduce=ls.callback(r))
        pred, hist = _myfm.create_train_vfm_sharded(rank, init_std, X[lo:hi], rels, np.ascontiguousarray(y[lo:hi]), seed, cfg, cb,
                                                    r, world, N, lo, levels, **prov)
        return pred, hist, hyp, first, calls

    return ls.run(one), levels


class _Snap:
    """the reference's state at one point, in the shape tgv._check reads"""

    def __init__(self, ref):
        for a in MODEL:
            setattr(self, a, np.array(getattr(ref, a)))
        self._hyper = {k: np.array(v) for k, v in ref.hyper().items()}
        self.elbos = list(ref.elbos)
        self.e = np.array(ref.e)

    def hyper(self):
        return self._hyper


_REF = {}


def _reference(name, task, n_iter=10):
    """data and the unsharded reference after 1 and after n_iter iterations: computed once, shared, left unchanged"""
    key = (name, task, n_iter)
    if key not in _REF:
        X, y, rank, gi, kw = tgv._cases()[name] if name != "mid" else _mid()
        if task == "classification":
            y = np.where(y > np.median(y), 1.0, -1.0)
        blocks = kw.get("blocks", ())
        w0, w, V = vb_ref.initial_weights(X, y, rank, 0.1, 7, blocks)
        ref = vb_ref.VBRef(X, y, rank, gi, task, vb_ref.Config(fit_w0=kw.get("fit_w0", True), fit_linear=kw.get("fit_linear", True)),
                           w0, w, V, 0.1, blocks=blocks)
        ref.iterate()
        snaps = {1: _Snap(ref)}
        for _ in range(n_iter - 1):
            ref.iterate()
        snaps[n_iter] = _Snap(ref)
        _REF[key] = (X, y, rank, gi, kw, snaps)
    return _REF[key]


def _mid():
    X = tgv._onehot(200_000, [1000, 2000], 9, values=True)
    return X, np.random.RandomState(4).randn(200_000), 8, np.r_[np.zeros(1000), np.ones(2000)], {}


def _task(task):
    return _myfm.TaskType.CLASSIFICATION if task == "classification" else _myfm.TaskType.REGRESSION


def _check_first(first, snap, rtol):
    """tgv._check on the snapshot a rank's callback took after the first iteration"""
    pred = types.SimpleNamespace(weights=lambda: types.SimpleNamespace(**{a: first[a] for a in MODEL}))
    hist = types.SimpleNamespace(elbos=first["elbos"], hypers=types.SimpleNamespace(alpha=first["hyper"]["alpha"],
                                                                                  mu_V=first["hyper"]["mu_V"]))
    tgv._check(pred, hist, first["hyper"], snap, rtol)


def _check_replicas(outs):
    a = outs[0][0].weights()
    for pred, hist, _, _, calls in outs[1:]:
        b = pred.weights()
        for n in ("w", "V", "V_var"):
            assert np.array_equal(getattr(a, n), getattr(b, n)), n
        assert np.array_equal(outs[0][1].elbos, hist.elbos)
        assert calls == outs[0][4]


def _budget(levels, K):
    return (K + 1) * len(np.unique(levels)) + 1


NAMES = ["onehot_unit", "onehot_values", "three_groups_unused", "rank0", "no_w0", "no_linear", "blocks_test_block", "blocks_multihot"]


@pytest.mark.parametrize("task", ["regression", "classification"])
@pytest.mark.parametrize("cut", ["world1", "balanced2", "uneven2", "empty3"])
@pytest.mark.parametrize("name", NAMES)
def test_chain_matches_unsharded_reference(name, cut, task):
    X, y, rank, gi, kw, snaps = _reference(name, task)
    outs, levels = _run_sharded(X, y, rank, gi, _task(task), 10, _cuts(cut, X.shape[0]), **kw)
    for pred, hist, hyp, first, calls in outs:
        _check_first(first, snaps[1], 1e-9)
        tgv._check(pred, hist, hyp, snaps[10], 1e-7)
        if not kw.get("fit_w0", True):
            assert np.all(np.isneginf(hist.elbos))
        # one score pass at the start, then (K + 1) * (non-empty levels) + 1 collectives per iteration, exactly
        assert calls == [1 + (i + 1) * _budget(levels, rank) for i in range(10)]
    _check_replicas(outs)


def test_middle_size_two_shards():
    X, y, rank, gi, kw, snaps = _reference("mid", "regression", 3)
    outs, _ = _run_sharded(X, y, rank, gi, _task("regression"), 3, _cuts("balanced2", X.shape[0]))
    for pred, hist, hyp, first, calls in outs:
        tgv._check(pred, hist, hyp, snaps[3], 1e-8)
    _check_replicas(outs)


def test_rerun_is_bit_identical():
    X, y, rank, gi, kw, _ = _reference("onehot_values", "regression")
    a, _ = _run_sharded(X, y, rank, gi, _task("regression"), 10, _cuts("uneven2", X.shape[0]))
    b, _ = _run_sharded(X, y, rank, gi, _task("regression"), 10, _cuts("uneven2", X.shape[0]))
    for (pa, ha, *_), (pb, hb, *_) in zip(a, b):
        for n in MODEL:
            assert np.array_equal(getattr(pa.weights(), n), getattr(pb.weights(), n)), n
        assert np.array_equal(ha.elbos, hb.elbos)


def test_budget_two_fields_rank_32():
    X = tgv._onehot(2000, [30, 50], 21)
    y = np.random.RandomState(1).randn(2000)
    outs, levels = _run_sharded(X, y, 32, np.r_[np.zeros(30), np.ones(50)], _task("regression"), 2, _cuts("balanced2", 2000))
    assert _budget(levels, 32) == 67
    for *_, calls in outs:
        assert calls == [1 + 67, 1 + 2 * 67]


def test_native_provider_world_1():
    X, y, rank, gi, kw, snaps = _reference("onehot_values", "regression")
    outs, levels = _run_sharded(X, y, rank, gi, _task("regression"), 10, _cuts("world1", X.shape[0]),
                                comm_id=_myfm.comm_unique_id())
    pred, hist, hyp, first, calls = outs[0]
    _check_first(first, snaps[1], 1e-9)
    tgv._check(pred, hist, hyp, snaps[10], 1e-7)
    assert calls[0] > 0 and calls[-1] == 1 + 10 * _budget(levels, rank)


# ---- single steps of every shard through the C ABI ---------------------------------------------------------------------------
_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


class _ShardVB(tgv._VB):
    """tgv._VB over rows [lo, hi) of a design, with the sharded calls between create and finalize"""

    def __init__(self, X, y, gi, K, blocks, lo, hi, rank, world, levels, allreduce, finalize=True):
        self.C, self.L = C, _capi.lib()
        P, I64, I32, D = C.c_void_p, C.c_int64, C.c_int32, C.c_double
        sig = {
            "mfm_vb_create": [C.c_int, I64, I64, P, P, P, P, P], "mfm_vb_add_block": [P, I64, I64, P, P, P, P],
            "mfm_vb_finalize": [P, P, I32, I32], "mfm_vb_set_state": [P, D, D, P, P, P, P],
            "mfm_vb_get_state": [P, P, P, P, P, P, P], "mfm_vb_update_e": [P, I32, P], "mfm_vb_get_e": [P, P],
            "mfm_vb_get_cache": [P, P, P, P], "mfm_vb_sweep_w": [P, D, P, P], "mfm_vb_sweep_V": [P, I32, I32, D, P, P],
            "mfm_vb_plan_info": [P, P, P], "mfm_vb_synchronize": [P], "mfm_vb_destroy": [P],
            "mfm_vb_set_allreduce": [P, P, P], "mfm_vb_set_shard": [P, I32, I32, I64, I64], "mfm_vb_set_levels": [P, P, I64],
            "mfm_vb_comm_stats": [P, P, P],
        }
        for name, a in sig.items():
            getattr(self.L, name).argtypes = a
        self.L.mfm_vb_last_error.restype = C.c_char_p
        X = sps.csr_matrix(X, dtype=np.float64)
        Xl = X[lo:hi]
        self.keep = []
        self.h = C.c_void_p()
        self._ok(self.L.mfm_vb_create(0, Xl.shape[0], Xl.shape[1], self._p(Xl.indptr, np.int64), self._p(Xl.indices, np.int32),
                                      self._p(Xl.data), self._p(y[lo:hi]), C.byref(self.h)))
        for mp, B in blocks:
            B = sps.csr_matrix(B, dtype=np.float64)
            self._ok(self.L.mfm_vb_add_block(self.h, B.shape[0], B.shape[1], self._p(B.indptr, np.int64),
                                             self._p(B.indices, np.int32), self._p(B.data), self._p(np.asarray(mp)[lo:hi], np.int64)))
        self.fn = _ALLREDUCE(lambda user, buf, count: allreduce(buf, count) or 0)
        self._ok(self.L.mfm_vb_set_allreduce(self.h, C.cast(self.fn, C.c_void_p), None))
        self._ok(self.L.mfm_vb_set_shard(self.h, rank, world, X.shape[0], lo))
        self._ok(self.L.mfm_vb_set_levels(self.h, self._p(levels, np.int32), len(levels)))
        self.N, self.D, self.K, self.G = hi - lo, len(gi), K, int(max(gi)) + 1
        self.gi = self._p(gi, np.int32)
        if finalize:
            self._ok(self.finalize())

    def finalize(self):
        return self.L.mfm_vb_finalize(self.h, self.gi, self.G, self.K)

    def calls(self):
        c, d = C.c_int64(), C.c_int64()
        self._ok(self.L.mfm_vb_comm_stats(self.h, C.byref(c), C.byref(d)))
        return c.value, d.value


@pytest.mark.parametrize("design,cut", [("onehot_values", "uneven2"), ("blocks_multihot", "empty3")])
def test_local_residual_of_every_shard(design, cut):
    X, y, K, gi, kw = tgv._cases()[design]
    blocks = kw.get("blocks", ())
    D = len(gi)
    cuts = _cuts(cut, X.shape[0])
    world = len(cuts) - 1
    levels = _myfm.vb_column_levels(X, [myfm_amd.RelationBlock(mp, B) for mp, B in blocks])
    n_lv = len(np.unique(levels))
    st = tgv._random_state(D, K, 3)
    ref = vb_ref.VBRef(X, y, K, gi, "regression", vb_ref.Config(), st[0], st[2], st[4], 0.1, blocks=blocks)
    ref.w0_var, ref.w_var[:], ref.V_var[:] = st[1], st[3], st[5]
    score, var = vb_ref.update_e_and_var(ref.Xf, *st)
    ref.e, ref.e_var_sum = score - y, var
    want = {"e0": ref.e.copy(), "var": var}
    ref.alpha = 1.7
    ref.lambda_w[:] = np.linspace(0.5, 2.0, ref.G)
    ref.mu_w[:] = np.linspace(-0.1, 0.2, ref.G)
    ref.sweep_w()
    want.update(w=ref.w.copy(), w_var=ref.w_var.copy(), e1=ref.e.copy())
    ref.lambda_V[:] = np.linspace(0.5, 2.0, ref.G * K).reshape(ref.G, K)
    ref.mu_V[:] = np.linspace(-0.2, 0.1, ref.G * K).reshape(ref.G, K)
    f = 1
    ref.sweep_factor(f)
    ls = Lockstep(world)

    def one(r):
        lo, hi = cuts[r], cuts[r + 1]
        vb = _ShardVB(X, y, gi, K, blocks, lo, hi, r, world, levels, ls.callback(r))
        launches = np.zeros(1, np.int64)
        vb._ok(vb.L.mfm_vb_plan_info(vb.h, None, launches.ctypes.data))
        assert launches[0] == 2 + 2 * n_lv + K * (1 + 2 * n_lv) + 2  # statistics and apply per level
        vb.set_state(*st)
        sums = vb.update_e(0)
        tgv._close(vb.e(), want["e0"][lo:hi], 1e-11)
        tgv._close(sums[2], want["var"], 1e-11)
        tgv._close(sums[0], want["e0"].sum(), 1e-10)
        assert vb.calls() == (1, 4)
        vb._ok(vb.L.mfm_vb_sweep_w(vb.h, ref.alpha, vb._p(ref.lambda_w), vb._p(ref.mu_w)))
        w, wv, V, Vv = vb.state()
        tgv._close(w, want["w"], 1e-10)
        tgv._close(wv, want["w_var"], 1e-10)
        tgv._close(vb.e(), want["e1"][lo:hi], 1e-10)
        assert vb.calls() == (1 + n_lv, 4 + 2 * D)
        vb._ok(vb.L.mfm_vb_sweep_V(vb.h, f, f + 1, ref.alpha, vb._p(ref.lambda_V.ravel("F")), vb._p(ref.mu_V.ravel("F"))))
        vb._ok(vb.L.mfm_vb_synchronize(vb.h))
        w, wv, V, Vv = vb.state()
        tgv._close(V, ref.V, 1e-10)
        tgv._close(Vv, ref.V_var, 1e-10)
        tgv._close(vb.e(), ref.e[lo:hi], 1e-10)
        for got, full in zip(vb.cache(), (ref.q, ref.x2s, ref.x3sv)):
            tgv._close(got, full[lo:hi], 1e-10)
        assert vb.calls() == (1 + 2 * n_lv, 4 + 6 * D)
        return sums, w, V

    outs = ls.run(one)
    for sums, w, V in outs[1:]:
        assert np.array_equal(sums, outs[0][0]) and np.array_equal(w, outs[0][1]) and np.array_equal(V, outs[0][2])


def test_a_schedule_that_shares_a_local_row_is_refused():
    X = tgv._onehot(400, [6, 9], 31)
    y = np.zeros(400)
    gi = np.r_[np.zeros(6), np.ones(9)]
    good = _myfm.vb_column_levels(X, [])
    called = []
    bad = good.copy()
    bad[6:] = 0  # the second field's columns in the first field's level: every row has two columns of level 0
    vb = _ShardVB(X, y, gi, 2, (), 100, 300, 1, 2, bad, lambda buf, count: called.append(count), finalize=False)
    assert vb.finalize() == 1  # MFM_ERR_INVALID
    assert b"share a row" in vb.L.mfm_vb_last_error(vb.h)
    out = np.empty(4)
    assert vb.L.mfm_vb_update_e(vb.h, 0, out.ctypes.data) == 1 and b"mfm_vb_finalize first" in vb.L.mfm_vb_last_error(vb.h)
    assert vb.calls() == (0, 0) and not called
    # levels that do not grow with the column index along a row are no schedule of this design either
    worse = good.copy()
    worse[:6], worse[6:] = 1, 0
    vb2 = _ShardVB(X, y, gi, 2, (), 100, 300, 1, 2, worse, lambda buf, count: called.append(count), finalize=False)
    assert vb2.finalize() == 1
    # unsharded, no row stays an error with its message
    h = C.c_void_p()
    z = np.zeros(1, np.int64)
    assert vb.L.mfm_vb_create(0, 0, 3, z.ctypes.data, None, None, None, C.byref(h)) == 0
    g3 = np.zeros(3, np.int32)
    assert vb.L.mfm_vb_finalize(h, g3.ctypes.data, 1, 2) == 1
    assert b"needs at least one row" in vb.L.mfm_vb_last_error(h)
    vb.L.mfm_vb_destroy(h)


# ---- fit() under torch.distributed ----------------------------------------------------------------------------------------
def _launch(world, port, env):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mp_vb_fit_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "mp_vb_fit_worker ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_two_processes_one_gpu_sharded_vb_fit():
    # two ranks under torch.distributed.run, both on device 0, process group over gloo, the library's all-reduces through the
    # torch.distributed callback (distributed.enable(native=False))
    _launch(2, 29651, {"MP_FIT_ONE_GPU": "1"})


def test_multi_gpu_sharded_vb_fit():
    # one process per GPU, the library's own RCCL communicator: needs >= 2 visible GPUs, skipped otherwise
    n = _myfm.device_count()
    if n < 2:
        pytest.skip("needs >= 2 GPUs (this box has %d)" % n)
    _launch(2 if n < 4 else 4, 29653, {})
