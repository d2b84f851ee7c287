"""Fold-in of a probit classifier at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples), DESIGN 4.14.1:
10 000 new users with 100 labelled observations each (the context of an observation is the item's one-hot), folded into every kept
sample by the inner chain with the default n_burn = 10 and n_inner = 40.
  (d) the device: mfm_foldin_gibbs_solve_store on samples resident in a device store, timed end to end (kernels, copy back of the
      (S, U, K + 1) result, synchronisation) in `--runs` runs of `--reps` calls after one warm-up; a run reports its median call.
      Creating the handle (the upload of the observations) is timed apart.
  (h) the host: the same chain in float64 NumPy with the draws of tests/philox_ref.py (the twin of tests/fold_in_gibbs_ref.py,
      batched over the entities, which all have the same number of rows here) on `--host-samples` of the samples; the time for
      all samples is that time scaled by their number, and is reported as such.
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
ap.add_argument("--n-burn", type=int, default=10)
ap.add_argument("--n-inner", type=int, default=40)
ap.add_argument("--host-samples", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--host-only", action="store_true", help="run the host chain alone (no device): a check of this script")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fold_in_gibbs_ref as gr  # noqa: E402
from tests import philox_ref as ph  # noqa: E402

NU, NI, K, S, U, R = args.users, args.items, args.rank, args.samples, args.new_users, args.obs
D, n, M, T = NU + NI, args.new_users * args.obs, args.rank + 1, args.n_burn + args.n_inner
SEED = 1
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


rng = np.random.default_rng(0)
items = rng.integers(0, NI, size=n)
X = sps.csr_matrix((np.ones(n), (NU + items).astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, D))
y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
entity = np.repeat(np.arange(U, dtype=np.int64), R)
mu, lam = rng.normal(size=(S, K + 1)) * 0.1, rng.uniform(0.5, 5.0, size=(S, K + 1))
all_samples = [(float(rng.normal() * 0.3), rng.normal(size=D) * 0.1, rng.normal(size=(D, K)) * 0.1) for _ in range(S)]


def host_chain(s):
    """the Rao-Blackwellised mean (U, M) of sample s: float64 linear algebra, the draws of the per-row streams"""
    w0, w, V = all_samples[s]
    q = X @ V
    f = (w0 + X @ w + 0.5 * ((q * q).sum(axis=1) - (X.multiply(X) @ (V * V)).sum(axis=1))).reshape(U, R)
    z = np.concatenate([np.ones((n, 1)), q], axis=1).reshape(U, R, M)
    L = np.linalg.cholesky(np.swapaxes(z, 1, 2) @ z + np.diag(lam[s])[None])
    Lt = np.swapaxes(L, 1, 2)
    rows = s * n + np.arange(n, dtype=np.int64)
    pos, neg = np.flatnonzero(y > 0), np.flatnonzero(~(y > 0))
    theta = np.broadcast_to(mu[s], (U, M)).copy()
    mean = np.zeros((U, M))
    for t in range(T):
        zt = (z * theta[:, None, :]).sum(axis=-1)
        bound = (0.0 - (f + zt)).ravel()
        g = ph.RowRng(SEED, gr.FOLDIN_LATENT_TAG + t, rows)
        d = np.empty(n)
        d[pos] = ph.tn_left(g.subset(pos), bound[pos])[0]
        d[neg] = ph.tn_right(g.subset(neg), bound[neg])[0]
        r = zt + d.reshape(U, R)
        b = (lam[s] * mu[s])[None, :] + (z * r[:, :, None]).sum(axis=1)
        yv = np.linalg.solve(L, b[:, :, None])
        eps = gr.normals_of_rows(SEED, gr.FOLDIN_DRAW_TAG + 1 + t, s * U + np.arange(U, dtype=np.int64), M)
        theta = np.linalg.solve(Lt, yv + eps[:, :, None])[..., 0]
        if t >= args.n_burn:
            mean += np.linalg.solve(Lt, yv)[..., 0]
    return mean / args.n_inner


say("fold-in of a classifier: %d new users x %d observations, D = %d, rank %d, %d samples, n_burn = %d, n_inner = %d"
    % (U, R, D, K, S, args.n_burn, args.n_inner))
w_dev = V_dev = None
if not args.host_only:
    from myfm_amd import _capi  # noqa: E402

    store = _capi.Store(D, K)
    for smp in all_samples:
        store.push(*smp)
    t0 = time.perf_counter()
    h = _capi.FoldIn(X, y, entity, U, True)
    say("(d) handle: grouping and upload of the observations %.3f s" % (time.perf_counter() - t0))
    kw = dict(n_burn=args.n_burn, n_inner=args.n_inner, seed=SEED)
    t0 = time.perf_counter()
    w_dev, V_dev = h.solve_gibbs_store(store, mu, lam, "classifier", **kw)  # warm-up
    say("(d) device, first call: %.4f s" % (time.perf_counter() - t0))
    meds = []
    for _ in range(args.runs):
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            h.solve_gibbs_store(store, mu, lam, "classifier", **kw)
            ts.append(time.perf_counter() - t0)
        meds.append(float(np.median(ts)))
    say("(d) device, all %d samples, end to end: median call of each run %s s" % (S, ", ".join("%.4f" % m for m in meds)))
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        h.solve_gibbs_store(store, mu, lam, "classifier", draw=True, **kw)
        ts.append(time.perf_counter() - t0)
    say("(d) device, posterior draws instead of means: median call %.4f s" % float(np.median(ts)))
    say("    per (entity, sample) and sweep: %.3f us" % (float(np.median(meds)) / (U * S * T) * 1e6))
    h.close()
    store.close()

t0 = time.perf_counter()
diffs = []
for s in range(min(args.host_samples, S)):
    theta = host_chain(s)
    print("(h) host sample %d done after %.0f s" % (s, time.perf_counter() - t0), flush=True)
    if w_dev is not None:
        diffs.append(np.abs(np.concatenate([w_dev[s][:, None], V_dev[s]], axis=1) - theta).max(axis=1))
host = time.perf_counter() - t0
ns = min(args.host_samples, S)
say("(h) host float64 NumPy: %.1f s for %d samples = %.1f s per sample; scaled to all %d samples: %.0f s" % (host, ns, host / ns, S, host / ns * S))
if diffs:
    diffs = np.concatenate(diffs)
    say("    |device - host| over the %d cells of those samples: median %.3e, largest %.3e, above 1e-9: %d (a draw within rounding of "
        "a sampler's decision takes another path)" % (diffs.shape[0], float(np.median(diffs)), float(diffs.max()), int((diffs > 1e-9).sum())))
    say("    host (scaled) / device: %.0f x" % (host / ns * S / float(np.median(meds))))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
