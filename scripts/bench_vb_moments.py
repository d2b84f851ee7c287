"""Analytic score moments of a variational model at the config-3 shape (69 878 users x 10 677 items, rank 32), DESIGN 10.1:
  rows   mfm_design_moments_vb (predict_moments) next to mfm_design_predict of the mean model (predict()), on one resident design
         of --rows one-hot rows; both calls upload the model and copy their outputs back, as the estimators' calls do;
  pairs  mfm_pairs_topk_bound_vb (predict_topk_bound) next to mfm_pairs_topk of the mean model (predict_topk) for --queries queries
         x all items, k = --k; and mfm_pairs_moments_vb on --dense-queries queries followed by a host argpartition, the thing the
         fused top-k replaces.
The posterior is random (the model's quality plays no role in the timing). Every timing: one warm-up, `reps` repetitions, median
and min .. max of a host clock around calls that end in a device synchronise. Writes the report to stdout and, with --out FILE, to
that file."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myfm_amd import _capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--dense-queries", type=int, default=1024)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--beta", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
NU, NI, K, N, U, k = args.users, args.items, args.rank, args.rows, args.queries, args.k
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
model = (float(rng.normal()), 0.05, rng.normal(size=D) * 0.3, rng.uniform(0.01, 0.1, size=D), rng.normal(size=(D, K)) * 0.2,
         rng.uniform(0.005, 0.05, size=(D, K)))
mean_model = [(model[0], model[2], model[4])]

# ---- rows
say("score moments at the config-3 shape: %d rows of one user and one item out of %d + %d, rank %d" % (N, NU, NI, K))
cols = np.stack([rng.integers(0, NU, size=N), NU + rng.integers(0, NI, size=N)], 1).astype(np.int32)
X = sps.csr_matrix((np.ones(2 * N), cols.ravel(), np.arange(0, 2 * N + 1, 2, dtype=np.int64)), shape=(N, D))
design = _capi.Design(X)
score, med_p, lo_p, hi_p = timed(lambda: design.predict(mean_model), args.reps)
(mean, std), med_m, lo_m, hi_m = timed(lambda: design.moments_vb(model), args.reps)
design.close()
say("predict() of the mean model:  median %.4f s (min %.4f, max %.4f, %d reps)" % (med_p, lo_p, hi_p, args.reps))
say("predict_moments:              median %.4f s (min %.4f, max %.4f, %d reps) -- %.2fx predict()" % (med_m, lo_m, hi_m, args.reps, med_m / med_p))
say("    mean == predict() bit for bit: %s; std in [%.3g, %.3g]" % (bool(np.array_equal(mean, score)), std.min(), std.max()))
if not np.array_equal(mean, score):
    raise SystemExit("predict_moments' mean differs from predict()")

# ---- pairs
users = np.sort(rng.choice(NU, size=U, replace=False))
Xq = sps.csr_matrix((np.ones(U), (np.arange(U), users)), shape=(U, D))
Xc = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))
pairs = _capi.Pairs(Xq, Xc)
say("ranking by mean + beta * std of the score: %d queries x %d items, rank %d, k = %d, beta = %g" % (U, NI, K, k, args.beta))
(idx_t, val_t), med_t, lo_t, hi_t = timed(lambda: pairs.topk(mean_model, k), args.reps)
(idx_b, val_b, m_b, s_b), med_b, lo_b, hi_b = timed(lambda: pairs.topk_bound_vb(model, k, args.beta), args.reps)
say("predict_topk of the mean model: median %.4f s (min %.4f, max %.4f, %d reps)" % (med_t, lo_t, hi_t, args.reps))
say("predict_topk_bound:             median %.4f s (min %.4f, max %.4f, %d reps) -- %.2fx predict_topk" % (med_b, lo_b, hi_b, args.reps, med_b / med_t))
say("    max |value - (mean + beta std)| = %.2e, std in [%.3g, %.3g]" % (np.abs(val_b - (m_b + args.beta * s_b)).max(), s_b.min(), s_b.max()))
(idx_0, val_0, _, _) = pairs.topk_bound_vb(model, k, 0.0)
say("    beta = 0 returns predict_topk's lists: indices %s, values %s" % (bool(np.array_equal(idx_0, idx_t)), bool(np.array_equal(val_0, val_t))))
pairs.close()

Ud = min(args.dense_queries, U)
dense = _capi.Pairs(Xq[:Ud], Xc)


def host_topk():
    mean_d, std_d = dense.moments_vb(model)
    v = mean_d + args.beta * std_d
    part = np.argpartition(-v, k - 1, axis=1)[:, :k]
    order = np.argsort(-np.take_along_axis(v, part, 1), axis=1, kind="stable")
    top = np.take_along_axis(part, order, 1)
    return top, np.take_along_axis(v, top, 1)


(idx_h, val_h), med_h, lo_h, hi_h = timed(host_topk, max(2, args.reps // 2))
dense.close()
say("predict_pairs_moments on %d queries + host argpartition: median %.4f s (min %.4f, max %.4f) -- %.1fx predict_topk_bound per query"
    % (Ud, med_h, lo_h, hi_h, (med_h / Ud) / (med_b / U)))
say("    its values equal the fused lists' bit for bit: %s" % bool(np.array_equal(val_h, val_b[:Ud])))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
