"""fold_in_topk at the config-3 shape (D = 80 555, rank 32, 95 samples in a device store), DESIGN 4.14.2: `--new-users` new users with
100 observations each, all 10 677 items as candidates (the item's one-hot), k = 10, by = "ucb".
  (r) the device: mfm_foldin_rank_topk_store end to end (candidate table, kept operands, tile kernel, selection, moments of the
      listed pairs, copy back), and its fp64 rate: the MFMA k-steps the tile kernel walks, padded tiles included, against the MFMA
      peak scripts/bench_topk.py uses; the useful count U S I (M + 1) M is given beside it.
  (f) mfm_foldin_solve_store on the same handle -- the kernel the kept form shares with fold_in -- to be held against the range
      profiles/fold_in_bench.txt records for the commit before.
  (h) the same computation in float64 NumPy on `--host-entities` entities and `--host-samples` samples, scaled to all, stated as such.
(r) and (f) are interleaved run by run; a run reports its median call. Writes the report to stdout and, with --out FILE, to it."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--new-users", type=int, nargs="+", default=[256, 4096])
ap.add_argument("--obs", type=int, default=100)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--host-entities", type=int, default=4)
ap.add_argument("--host-samples", type=int, default=2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myfm_amd import _capi  # noqa: E402

FP64_MFMA_PEAK = 78.6e12  # MI355X data sheet: FP64 matrix, dense (scripts/bench_topk.py)
NU, NI, K, S, R = args.users, args.items, args.rank, args.samples, args.obs
D, M = NU + NI, K + 1
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def timed(fn):
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


rng = np.random.default_rng(0)
alpha = rng.uniform(1.0, 2.0, size=S)
mu, lam = rng.normal(size=(S, K + 1)) * 0.1, rng.uniform(0.5, 5.0, size=(S, K + 1))
store, kept = _capi.Store(D, K), []
for _ in range(S):
    smp = (float(rng.normal()), rng.normal(size=D) * 0.1, rng.normal(size=(D, K)) * 0.1)
    store.push(*smp)
    if len(kept) < args.host_samples:
        kept.append(smp)
Xc = sps.csr_matrix((np.ones(NI), (NU + np.arange(NI)).astype(np.int32), np.arange(NI + 1, dtype=np.int64)), shape=(NI, D))
ksteps = sum(min((M + 3) // 4, 4 * t + 4) for t in range((M + 16) // 16))  # per 16-candidate tile of one (entity, sample)

for U in args.new_users:
    n = U * R
    items = rng.integers(0, NI, size=n)
    X = sps.csr_matrix((np.ones(n), (NU + items).astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, D))
    y, entity = rng.normal(size=n) + 3.5, np.repeat(np.arange(U, dtype=np.int64), R)
    say("fold_in_topk: %d new users x %d observations, %d candidates, k = %d, D = %d, rank %d, %d samples" % (U, R, NI, args.k, D, K, S))
    h = _capi.FoldIn(X, y, entity, U, True)
    h.set_candidates(Xc)
    top = h.rank_topk_store(store, alpha, mu, lam, args.k)  # warm-up
    h.solve_store(store, alpha, mu, lam)
    med_r, med_f = [], []
    for _ in range(args.runs):
        med_r.append(timed(lambda: h.rank_topk_store(store, alpha, mu, lam, args.k)))
        med_f.append(timed(lambda: h.solve_store(store, alpha, mu, lam)))
    t = float(np.median(med_r))
    walked = float(U) * S * ((NI + 15) // 16) * ksteps * 16 * 16 * 4 * 2
    useful = float(U) * S * NI * (M + 1) * M
    say("(r) mfm_foldin_rank_topk_store: median call of each run %s s" % ", ".join("%.4f" % m for m in med_r))
    say("    walked MFMA work %.3f TFLOP (useful (M + 1) M count %.3f TFLOP): %.2f TFLOP/s fp64 over the whole call, %.1f %% of the "
        "%.1f TFLOP/s MFMA peak" % (walked / 1e12, useful / 1e12, walked / t / 1e12, 100 * walked / t / FP64_MFMA_PEAK, FP64_MFMA_PEAK / 1e12))
    say("(f) mfm_foldin_solve_store on the same handle: median call of each run %s s" % ", ".join("%.4f" % m for m in med_f))
    # ---- the host, on a few entities and samples
    ne, t0, worst = min(args.host_entities, U), time.perf_counter(), 0.0
    for s, (w0, w, V) in enumerate(kept):
        qc = Xc @ V
        fc = w0 + Xc @ w + 0.5 * ((qc * qc).sum(axis=1) - (Xc.multiply(Xc) @ (V * V)).sum(axis=1))
        zc = np.concatenate([np.ones((NI, 1)), qc], axis=1)
        Xe = X[:ne * R]
        q = Xe @ V
        f = w0 + Xe @ w + 0.5 * ((q * q).sum(axis=1) - (Xe.multiply(Xe) @ (V * V)).sum(axis=1))
        z = np.concatenate([np.ones((ne * R, 1)), q], axis=1).reshape(ne, R, M)
        Lam = alpha[s] * (np.swapaxes(z, 1, 2) @ z) + np.diag(lam[s])[None]
        b = alpha[s] * (np.swapaxes(z, 1, 2) @ (y[:ne * R] - f).reshape(ne, R, 1)) + (lam[s] * mu[s])[None, :, None]
        L = np.linalg.cholesky(Lam)
        theta = np.linalg.solve(np.swapaxes(L, 1, 2), np.linalg.solve(L, b))[..., 0]
        m = fc[None, :] + theta @ zc.T
        v = (np.linalg.solve(L, np.broadcast_to(zc.T, (ne, M, NI))) ** 2).sum(axis=1)
    host = time.perf_counter() - t0
    scaled = host / (ne * len(kept)) * U * S
    say("(h) host float64 NumPy: %.3f s for %d entities x %d samples; scaled to %d x %d: %.1f s (%.0f x the device call); not "
        "computed in full" % (host, ne, len(kept), U, S, scaled, scaled / t))
    say("    first list of the device call: %s" % top[0][0].tolist())
    h.close()
say("not measured: fold_in + predict_topk_ucb on the folded model (the route without the within-sample term), predict_topk_ucb "
    "itself, by = 'gain', the dense form, other ranks, rocprofv3 kernel statistics")
store.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
