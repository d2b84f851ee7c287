"""Ranking at the config-3 shape (69 878 users x 10 677 items, rank 32, 95 samples, k = 10), DESIGN 4.13:
  (a) what the library offered before predict_topk: materialise the U x I pair rows, predict(), np.argpartition per row;
  (b) predict_topk's device path (mfm_pairs_topk_store) on the same samples;
for U = 4096 queries, then (b) alone for all users. The samples are random draws pushed into a device store (what a fit keeps);
the model's quality plays no role in the timing. Every timing: one warm-up, `reps` repetitions, median and min .. max.
Writes the report to stdout and, with --out FILE, to that file."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myfm_amd import _capi  # noqa: E402

FP64_MFMA_PEAK = 78.6e12  # MI355X data sheet: FP64 matrix, dense

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reps-materialised", type=int, default=3)
ap.add_argument("--skip-materialised", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
NU, NI, K, S, U, k = args.users, args.items, args.rank, args.samples, args.queries, args.k
D = NU + NI
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, float(np.median(ts)), min(ts), max(ts)


rng = np.random.default_rng(0)
store = _capi.Store(D, K)
for _ in range(S):
    store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
users = np.sort(rng.choice(NU, size=U, replace=False))
Xc = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))


def onehot_users(u):
    return sps.csr_matrix((np.ones(u.size), (np.arange(u.size), u)), shape=(u.size, D))


say("ranking at the config-3 shape: %d users x %d items, rank %d, %d samples, k = %d" % (NU, NI, K, S, k))
Xq = onehot_users(users)
pairs = _capi.Pairs(Xq, Xc)
(idx_b, val_b), med_b, lo_b, hi_b = timed(lambda: pairs.topk_store(store, k), args.reps)
flop = 2.0 * U * NI * S * K
say("(b) predict_topk, %d queries x %d items: median %.4f s (min %.4f, max %.4f, %d reps) -- %.1f TFLOP/s fp64 over the whole "
    "call (embedding, contraction + selection, merge, copy back), %.0f %% of the %.1f TFLOP/s MFMA peak"
    % (U, NI, med_b, lo_b, hi_b, args.reps, flop / med_b / 1e12, 100 * flop / med_b / FP64_MFMA_PEAK, FP64_MFMA_PEAK / 1e12))

if not args.skip_materialised:
    def materialised():
        n = U * NI
        indices = np.empty((n, 2), dtype=np.int32)
        indices[:, 0] = np.repeat(users, NI)
        indices[:, 1] = np.tile(NU + np.arange(NI, dtype=np.int32), U)
        X = sps.csr_matrix((np.ones(2 * n), indices.ravel(), np.arange(0, 2 * n + 1, 2, dtype=np.int64)), shape=(n, D))
        design = _capi.Design(X)
        score = store.predict(design).reshape(U, NI)
        design.close()
        part = np.argpartition(-score, k - 1, axis=1)[:, :k]
        order = np.argsort(-np.take_along_axis(score, part, 1), axis=1, kind="stable")
        top = np.take_along_axis(part, order, 1)
        return top, np.take_along_axis(score, top, 1)

    (idx_a, val_a), med_a, lo_a, hi_a = timed(materialised, args.reps_materialised)
    say("(a) materialise %.1e pair rows + predict() + argpartition: median %.3f s (min %.3f, max %.3f, %d reps)"
        % (U * NI, med_a, lo_a, hi_a, args.reps_materialised))
    say("    (b) is %.0fx faster than (a); max |top-k value difference| = %.2e, rows whose index lists agree: %d of %d"
        % (med_a / med_b, np.abs(val_a - val_b).max(), int(np.all(idx_a == idx_b, axis=1).sum()), U))
    # (a) is predict() itself: its k best values must be (b)'s. The scale of a score's rounding error is the sum of the absolute
    # terms, at most S-averaged |w0| + 2 max|w| + (2 max|V|)^2 K here; 1e-10 of it is the bound of tests/test_gpu_pairs.py
    scale = 1.0 + 2 * 0.3 * 6 + K * (2 * 0.2 * 6) ** 2
    if not np.all(np.abs(val_a - val_b) <= 1e-10 * scale):
        raise SystemExit("predict_topk's values differ from predict()'s on the materialised pairs")
pairs.close()

if NU > U:
    pairs = _capi.Pairs(onehot_users(np.arange(NU)), Xc)
    _, med, lo, hi = timed(lambda: pairs.topk_store(store, k), max(2, args.reps // 2))
    flop = 2.0 * NU * NI * S * K
    say("(b) predict_topk, all %d users x %d items: median %.3f s (min %.3f, max %.3f) -- %.1f TFLOP/s fp64 over the whole call, "
        "%.0f %% of the MFMA peak" % (NU, NI, med, lo, hi, flop / med / 1e12, 100 * flop / med / FP64_MFMA_PEAK))
    pairs.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
