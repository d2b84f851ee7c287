"""Fold-in at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples), DESIGN 4.14: 10 000 new users with
100 observations each (the context of an observation is the item's one-hot), folded into every kept sample.
  (d) the device: mfm_foldin_solve_store on samples resident in a device store, timed end to end (kernels, copy back of the
      (S, U, K + 1) result, synchronisation) in `--runs` runs of `--reps` calls after one warm-up; a run reports its median call.
      Creating the handle (the upload of the observations) is timed apart.
  (h) the host: the same computation in float64 NumPy -- per sample one sparse product for z and the residual, a batched
      (U, K + 1, 100) x (U, 100, K + 1) product for the Gram matrices, np.linalg.cholesky and two batched solves -- on
      `--host-samples` of the samples; the time for all samples is that time scaled by their number, and is reported as such.
The samples are random draws (what a fit keeps); the model's quality plays no role in the timing. The device result is compared
with the host's on the samples the host computed. Writes the report to stdout and, with --out FILE, to that file."""
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
ap.add_argument("--new-users", type=int, default=10000)
ap.add_argument("--obs", type=int, default=100)
ap.add_argument("--host-samples", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, U, R = args.users, args.items, args.rank, args.samples, args.new_users, args.obs
D, n = NU + NI, args.new_users * args.obs
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


rng = np.random.default_rng(0)
items = rng.integers(0, NI, size=n)
X = sps.csr_matrix((np.ones(n), (NU + items).astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, D))
y = rng.normal(size=n) + 3.5
entity = np.repeat(np.arange(U, dtype=np.int64), R)
alpha = rng.uniform(1.0, 2.0, size=S)
mu, lam = rng.normal(size=(S, K + 1)) * 0.1, rng.uniform(0.5, 5.0, size=(S, K + 1))
samples = []
store = _capi.Store(D, K)
for _ in range(S):
    smp = (float(rng.normal()), rng.normal(size=D) * 0.1, rng.normal(size=(D, K)) * 0.1)
    store.push(*smp)
    if len(samples) < args.host_samples:
        samples.append(smp)

say("fold-in: %d new users x %d observations, D = %d, rank %d, %d samples" % (U, R, D, K, S))
t0 = time.perf_counter()
h = _capi.FoldIn(X, y, entity, U, True)
say("(d) handle: grouping and upload of the observations %.3f s" % (time.perf_counter() - t0))
w_dev, V_dev = h.solve_store(store, alpha, mu, lam)  # warm-up
meds = []
for _ in range(args.runs):
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        h.solve_store(store, alpha, mu, lam)
        ts.append(time.perf_counter() - t0)
    meds.append(float(np.median(ts)))
say("(d) device, all %d samples, end to end: median call of each run %s s" % (S, ", ".join("%.4f" % m for m in meds)))
ts = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    h.solve_store(store, alpha, mu, lam, draw=True, seed=1)
    ts.append(time.perf_counter() - t0)
say("(d) device, posterior draws instead of means: median call %.4f s" % float(np.median(ts)))

# ---- the host
t0 = time.perf_counter()
worst = 0.0
for s, (w0, w, V) in enumerate(samples):
    q = X @ V
    f = w0 + X @ w + 0.5 * ((q * q).sum(axis=1) - (X.multiply(X) @ (V * V)).sum(axis=1))
    z = np.concatenate([np.ones((n, 1)), q], axis=1).reshape(U, R, K + 1)
    r = (y - f).reshape(U, R, 1)
    Lam = alpha[s] * (np.swapaxes(z, 1, 2) @ z) + np.diag(lam[s])[None]
    b = alpha[s] * (np.swapaxes(z, 1, 2) @ r) + (lam[s] * mu[s])[None, :, None]
    L = np.linalg.cholesky(Lam)
    theta = np.linalg.solve(np.swapaxes(L, 1, 2), np.linalg.solve(L, b))[..., 0]
    got = np.concatenate([w_dev[s][:, None], V_dev[s]], axis=1)
    worst = max(worst, float(np.abs(got - theta).max()))
host = time.perf_counter() - t0
say("(h) host float64 NumPy: %.3f s for %d samples = %.3f s per sample; scaled to all %d samples: %.1f s" %
    (host, len(samples), host / len(samples), S, host / len(samples) * S))
say("    largest |device - host| over those samples: %.3e" % worst)
say("    host (scaled) / device: %.1f x" % (host / len(samples) * S / float(np.median(meds))))
h.close()
store.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
