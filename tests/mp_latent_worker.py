"""Worker of tests/test_gpu_sharded.py::test_two_processes_one_gpu_sharded_latent_fit (two ranks on device 0 under
torch.distributed.run, process group over gloo, the library's all-reduces through the torch.distributed callback):
MyFMClassifier and MyFMOrderedProbit fitted row-sharded on rows that arrive UNSORTED (fit() re-sorts them) must give, on every
rank, the chain of the unsharded fit with exact_latent_draws=False at the same seed -- the per-row Philox latent draws are keyed by
the global row, whatever the sharding -- and the ranks' copies of the model must agree bit for bit."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _digest(fm, ordered):
    h = hashlib.sha256()
    for s in fm.predictor_.samples:
        h.update(np.float64(s.w0).tobytes())
        h.update(np.ascontiguousarray(s.w, dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(s.V, dtype=np.float64).tobytes())
        if ordered:
            for c in s.cutpoints:
                h.update(np.ascontiguousarray(c, dtype=np.float64).tobytes())
    return h.hexdigest()


def main():
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ["MYFM_AMD_DEVICE"] = "0"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import myfm_amd
    from myfm_amd import distributed as D
    from tests import datasets as ds

    n_iter = 6
    X, yr, shapes = ds.onehot_mf(20000, 200, 60, seed=8, sort_by_user=False)
    first = X.indices[X.indptr[:-1]]
    assert np.any(first[1:] < first[:-1])  # (fit() re-sorts these rows: the path that used to set a row order of ALL rows)
    for name, make, y in (
        ("classifier", myfm_amd.MyFMClassifier, (yr > np.median(yr)).astype(np.int64)),
        ("ordered", myfm_amd.MyFMOrderedProbit, np.searchsorted(np.quantile(yr, [0.2, 0.5, 0.7]), yr).astype(np.int64)),
    ):
        ordered = name == "ordered"
        D.disable()
        ref = make(4, random_seed=7, exact_latent_draws=False).fit(X, y, group_shapes=shapes, n_iter=n_iter, n_kept_samples=n_iter)
        D.enable(native=False)
        got = make(4, random_seed=7).fit(X, y, group_shapes=shapes, n_iter=n_iter, n_kept_samples=n_iter)
        assert len(got.predictor_.samples) == len(ref.predictor_.samples) == n_iter
        for s, r in zip(got.predictor_.samples, ref.predictor_.samples):
            assert abs(s.w0 - r.w0) < 1e-7, (name, s.w0, r.w0)
            np.testing.assert_allclose(s.w, r.w, rtol=1e-7, atol=1e-7, err_msg=name)
            np.testing.assert_allclose(s.V, r.V, rtol=1e-7, atol=1e-7, err_msg=name)
            if ordered:
                np.testing.assert_allclose(s.cutpoints[0], r.cutpoints[0], rtol=1e-7, atol=1e-7, err_msg=name)
        if ordered:
            assert list(got.history_.n_mh_accept) == list(ref.history_.n_mh_accept)
        np.testing.assert_allclose(got.predict_proba(X[:3000]), ref.predict_proba(X[:3000]), rtol=1e-7, atol=1e-7, err_msg=name)
        # the ranks' copies of the model: bit for bit
        digests = [None] * world
        dist.all_gather_object(digests, _digest(got, ordered))
        assert len(set(digests)) == 1, (name, digests)
    dist.barrier()
    if rank == 0:
        print("mp_latent_worker ok: world", world)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
