"""Variational FM iterations per second on the device (create_train_vfm), regression and classification, at the shapes of
BASELINE configs 2 (ML-100k one-hot, rank 8) and 3 (ML-10M-shaped, rank 32), with the seeded data bench.py uses. One JSON
line per case: setup seconds (trainer construction, uploads, initial pass), iterations per second over --steps iterations
after --warmup, the algorithmic bytes of one iteration by the model below and the share of the 8 TB/s HBM roofline.

Bytes model of one iteration (every array touched once per pass, 8-byte values, 4-byte indices, N rows, Z entries, D
features, K factors): the score pass reads the CSR (12 Z + 8 N) and y, gathers w, w_var and per factor V, V_var (16 Z (K + 1))
and writes e; the w sweep streams the CSC (12 Z) and reads and writes e per entry (16 Z); per factor the cache build reads
the CSR and gathers V, V_var (28 Z) and writes q, x2s, x3sv (24 N), and the V sweep streams the CSC and reads e, q, x2s,
x3sv in its statistics pass and reads and writes them in its update pass (12 Z + 32 Z + 12 Z + 64 Z); the group statistics
read w, w_var, V, V_var twice (32 D (K + 1)). Timing synchronises with the device (the callback of the last iteration
fetches the model).

--split adds, after every case, the same fit on the row-sharded path with a world of 1 (create_train_vfm_sharded with the
library's own RCCL communicator): the statistics / all-reduce / apply kernels on one GPU, (K + 1) * levels + 1 collectives of
one rank per iteration. Its line carries "path": "split" and the ratio of its rate to the unsharded rate of the same run.
    python scripts/bench_variational.py [--configs 2,3] [--steps 5] [--warmup 1] [--split]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from myfm_amd import _myfm  # noqa: E402
from myfm_amd.utils import synthetic as ds  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def bytes_per_iteration(N, Z, D, K):
    score = 12 * Z + 8 * N + 8 * N + 16 * Z * (K + 1) + 8 * N
    sweep_w = 12 * Z + 16 * Z
    per_factor = (12 * Z + 8 * N + 16 * Z) + 24 * N + (12 * Z + 32 * Z + 12 * Z + 64 * Z)
    stats = 2 * 32 * D * (K + 1)
    return score + sweep_w + K * per_factor + stats


def data(config):
    if config == 2:
        X, y, shapes = ds.movielens_like(80000, 943, 1682, rank_true=8, seed=0, user_offset=30.0, item_offset=20.0)
        return X, y, shapes, 8
    X, y, shapes = ds.movielens_like(10_000_000, 69878, 10677, rank_true=32, seed=1)
    return X, y, shapes, 32


def run(X, y, shapes, rank, task, n_iter, split=False):
    b = _myfm.ConfigBuilder()
    b.set_group_index([int(g) for g in ds.group_index_from_shapes(shapes)]).set_n_iter(n_iter).set_n_kept_samples(n_iter)
    b.set_task_type(task)
    stamps = []

    def cb(i, fm, hyper, hist):
        if i == n_iter - 1:
            np.asarray(fm.w)  # (fetches the model: waits for the device)
        stamps.append(time.perf_counter())
        return False

    if split:
        levels = _myfm.vb_column_levels(X, [])  # (not part of the fit's setup time: fit() computes it on the full data)
        t0 = time.perf_counter()
        _myfm.create_train_vfm_sharded(rank, 0.1, X, [], y, 42, b.build(), cb, 0, 1, X.shape[0], 0, levels,
                                       comm_id=_myfm.comm_unique_id())
        return t0, stamps
    t0 = time.perf_counter()
    _myfm.create_train_vfm(rank, 0.1, X, [], y, 42, b.build(), cb)
    return t0, stamps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--split", action="store_true", help="also time the row-sharded path with a world of 1")
    a = ap.parse_args()
    for config in [int(c) for c in a.configs.split(",")]:
        X, y, shapes, rank = data(config)
        for name, task in (("regression", _myfm.TaskType.REGRESSION), ("classification", _myfm.TaskType.CLASSIFICATION)):
            yy = y if name == "regression" else np.where(y > np.median(y), 1.0, -1.0)
            n_iter = a.warmup + a.steps
            base = None
            for split in ((False, True) if a.split else (False,)):
                t0, st = run(X, yy, shapes, rank, task, n_iter, split)
                # setup: up to the end of the first iteration minus that iteration's time at the steady rate
                per_it = (st[-1] - st[a.warmup - 1]) / a.steps if a.warmup else (st[-1] - st[0]) / max(1, a.steps - 1)
                setup = st[0] - t0 - per_it
                B = bytes_per_iteration(X.shape[0], X.nnz, X.shape[1], rank)
                out = {"config": config, "task": name, "rows": X.shape[0], "nnz": int(X.nnz), "features": X.shape[1],
                       "rank": rank, "steps": a.steps, "warmup": a.warmup, "it_per_s": round(1.0 / per_it, 3),
                       "setup_s": round(setup, 3), "alg_bytes_per_it": int(B),
                       "hbm_roofline_share": round(B / per_it / HBM_BYTES_PER_S, 4)}
                if split:
                    out.update(path="split", world=1, ratio_to_unsharded=round(base / per_it, 4))
                base = per_it
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
