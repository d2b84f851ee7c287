"""Worker of tests/test_gpu_variational_sharded.py (one process per rank, launched by torch.distributed.run):
VariationalFMRegressor.fit() on a one-hot table and VariationalFMClassifier.fit() with relation blocks, row-sharded over the
ranks, must reproduce the NumPy restatement of the reference on the unsharded data on every rank, with bit-identical replicas
and the predictions of the unsharded estimator."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _close(got, want, rtol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * np.max(np.abs(want)))


def main():
    import torch
    import torch.distributed as dist

    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    # MP_FIT_ONE_GPU=1: every rank on device 0, process group over gloo, the library's all-reduces through the
    # torch.distributed callback (RCCL refuses two ranks on one device)
    one_gpu = bool(os.environ.get("MP_FIT_ONE_GPU"))
    if one_gpu:
        local = 0
        os.environ["MYFM_AMD_DEVICE"] = "0"
    torch.cuda.set_device(local)
    if one_gpu:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    import myfm_amd
    from myfm_amd import distributed as D
    from tests import test_gpu_variational as tgv
    from tests import vb_ref

    def fit_both(make, *args, **kw):
        D.enable(native=not one_gpu)
        assert D.active()
        sharded = make().fit(*args, **kw)
        D.disable()
        return sharded, make().fit(*args, **kw)

    def check(est, ref):
        for a, b in (("w0_mean", "w0"), ("w0_var", "w0_var"), ("w_mean", "w"), ("w_var", "w_var"), ("V_mean", "V"), ("V_var", "V_var")):
            _close(getattr(est, a), getattr(ref, b), 1e-7)
        h = ref.hyper()
        _close(est.history_.hypers.alpha, h["alpha"], 1e-7)
        _close(est.history_.hypers.mu_V, h["mu_V"], 1e-7)
        np.testing.assert_allclose(est.history_.elbos, ref.elbos, rtol=1e-6)
        # replicas agree bit for bit
        mine = (est.w_mean.tobytes(), est.V_mean.tobytes(), est.V_var.tobytes(), np.asarray(est.history_.elbos).tobytes())
        every = [None] * world
        dist.all_gather_object(every, mine)
        assert all(o == every[0] for o in every)

    # regression on a one-hot table
    X, y, K, gi, _ = tgv._cases()["onehot_values"]
    Xte = tgv._onehot(300, [40, 60], 12, values=True)
    est, single = fit_both(lambda: myfm_amd.VariationalFMRegressor(K, random_seed=7), X, y, n_iter=10, group_shapes=[40, 60])
    w0, w, V = vb_ref.initial_weights(X, y, K, 0.1, 7)
    ref = vb_ref.VBRef(X, y, K, gi, "regression", vb_ref.Config(), w0, w, V, 0.1)
    for _ in range(10):
        ref.iterate()
    check(est, ref)
    _close(est.predict(Xte), single.predict(Xte), 1e-7)

    # classification with relation blocks
    tm, yb, Kb, gib, kw = tgv._test_block_design()
    blocks = kw["blocks"]
    rels = [myfm_amd.RelationBlock(mp, B) for mp, B in blocks]
    yc = yb > np.median(yb)
    clf, single = fit_both(lambda: myfm_amd.VariationalFMClassifier(Kb, random_seed=7), tm, yc, rels, n_iter=10,
                           grouping=[int(g) for g in gib])
    ypm = np.where(yc, 1.0, -1.0)
    w0, w, V = vb_ref.initial_weights(tm, ypm, Kb, 0.1, 7, blocks)
    ref = vb_ref.VBRef(tm, ypm, Kb, gib, "classification", vb_ref.Config(), w0, w, V, 0.1, blocks=blocks)
    for _ in range(10):
        ref.iterate()
    check(clf, ref)
    _close(clf.predict_proba(tm[:200], [myfm_amd.RelationBlock(mp[:200], B) for mp, B in blocks]),
           single.predict_proba(tm[:200], [myfm_amd.RelationBlock(mp[:200], B) for mp, B in blocks]), 1e-7)
    dist.barrier()
    if rank == 0:
        print("mp_vb_fit_worker ok: world", world)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
