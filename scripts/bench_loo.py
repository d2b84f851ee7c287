"""Pareto-smoothed leave-one-out at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples, 1 M rows), DESIGN
4.9.3:
  (r) (c) (o)  predict_loo of a regression / classification / ordered-probit (5 classes) target (mfm_design_loo_store);
  (R) (C) (O)  the same with log_weights=True: the (S, N) log weights are copied to the host as well;
  (h)          what a user had to do before: the log density with pointwise=True (mfm_design_logdens_store, the (S, N) matrix to the
               host), then the vectorised NumPy PSIS of tests/psis_ref.py on the host. The host part is timed on the first
               `--host-rows` rows and scaled to all rows (it is linear in the rows); the report says so;
  (d)          the log density without the matrix (regression), in this tree and, with --parent-root, in the parent: the existing
               call is unchanged.
The samples are random draws around one model pushed into a device store (what a fit keeps), the targets random; the model's
quality plays no role in the timing. Every device variant is timed end to end (the call on an uploaded design: kernels, copy back,
synchronisation) in `--runs` runs of `--reps` calls each after one warm-up, the runs of the variants interleaved; a run reports its
median call.

--parent-root DIR: a built checkout of the parent commit. Its log density is timed in child processes interleaved with this
tree's, `--runs` runs each, and the report says whether this tree's lies within the spread of the parent's runs.
Writes the report to stdout and, with --out FILE, to that file."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sps

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--host-rows", type=int, default=20_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help=argparse.SUPPRESS)
ap.add_argument("--child", choices=["d"], default=None, help=argparse.SUPPRESS)  # one variant: a JSON line of its run
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, N = args.users, args.items, args.rank, args.samples, args.rows
D = NU + NI
N_CUT = 4
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def setup():
    rng = np.random.default_rng(0)
    store = _capi.Store(D, K)
    w0, w, V = float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2
    for _ in range(S):  # a posterior around one model
        store.push(w0 + 0.05 * float(rng.normal()), w + 0.05 * rng.normal(size=D), V + 0.02 * rng.normal(size=(D, K)))
    indices = np.empty((N, 2), dtype=np.int32)
    indices[:, 0] = np.sort(rng.integers(0, NU, size=N))
    indices[:, 1] = NU + rng.integers(0, NI, size=N)
    X = sps.csr_matrix((np.ones(2 * N), indices.ravel(), np.arange(0, 2 * N + 1, 2, dtype=np.int64)), shape=(N, D))
    alphas = np.exp(rng.normal(size=S) * 0.1) * 1.5
    cuts = np.sort(rng.normal(size=(S, N_CUT)) * 0.1 + np.array([-1.5, -0.5, 0.5, 1.5]), axis=1)
    y = {0: rng.normal(size=N), 1: (rng.random(N) < 0.5).astype(np.float64), 2: rng.integers(0, N_CUT + 1, size=N).astype(np.float64)}
    design = _capi.Design(X)
    calls = {"d": lambda: store.log_density(design, 0, y[0], precisions=alphas),
             "D": lambda: store.log_density(design, 0, y[0], precisions=alphas, pointwise=True)}
    if hasattr(store, "loo"):
        for name, task, kw in (("r", 0, dict(precisions=alphas)), ("c", 1, {}), ("o", 2, dict(cutpoints=cuts))):
            calls[name] = lambda task=task, kw=kw: store.loo(design, task, y[task], **kw)
            calls[name.upper()] = lambda task=task, kw=kw: store.loo(design, task, y[task], log_weights=True, **kw)
    return calls


def one_run(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


if args.child:
    fn = setup()[args.child]
    fn()  # warm-up
    print(json.dumps({"variant": args.child, "median_s": one_run(fn, args.reps)}), flush=True)
    sys.exit(0)


def child_cmd(variant, root):
    return [sys.executable, os.path.abspath(__file__), "--child", variant, "--root", root, "--users", str(NU), "--items", str(NI), "--rank",
            str(K), "--samples", str(S), "--rows", str(N), "--reps", str(args.reps)]


def spread(ts):
    return "%s ms (min %.3f, max %.3f)" % (", ".join("%.3f" % (1e3 * t) for t in ts), 1e3 * min(ts), 1e3 * max(ts))


say("PSIS leave-one-out at the config-3 shape: %d + %d one-hot columns, rank %d, %d samples, %d rows; ordered probit with %d classes"
    % (NU, NI, K, S, N, N_CUT + 1))
calls = setup()
for fn in calls.values():
    fn()  # warm-up
runs = {v: [] for v in calls}
for _ in range(args.runs):  # interleaved
    for v, fn in calls.items():
        runs[v].append(one_run(fn, args.reps))
names = {"d": "(d) log density, regression            ", "D": "(D) log density, regression, pointwise ",
         "r": "(r) predict_loo, regression            ", "R": "(R) predict_loo, regression, weights   ",
         "c": "(c) predict_loo, classification        ", "C": "(C) predict_loo, classification, weights",
         "o": "(o) predict_loo, ordered probit        ", "O": "(O) predict_loo, ordered probit, weights"}
say("end to end, median call of each of %d runs of %d calls:" % (args.runs, args.reps))
for v in calls:
    say("  %s %s" % (names[v], spread(runs[v])))
med = {v: float(np.median(t)) for v, t in runs.items()}
say("  log_weights=True and pointwise=True copy %.2f GB to the host" % (8.0 * N * S / 1e9))

# (h) the host path: the matrix of (D), then the NumPy reference on a row subset, scaled
from tests import psis_ref  # noqa: E402

ll = calls["D"]()[4]
H = min(args.host_rows, N)
sub = np.ascontiguousarray(ll[:, :H])
psis_ref.psis(sub[:, : min(H, 1000)])  # warm-up
host = []
for _ in range(args.runs):
    t0 = time.perf_counter()
    elpd, k, _ = psis_ref.psis(sub)
    host.append(time.perf_counter() - t0)
scaled = float(np.median(host)) * N / H
say("(h) the host path: (D) %.1f ms + NumPy PSIS of tests/psis_ref.py on the first %d rows %s, scaled by %d / %d to %.0f ms: %.0f ms"
    % (1e3 * med["D"], H, spread(host), N, H, 1e3 * scaled, 1e3 * (med["D"] + scaled)))
got = calls["r"]()
say("    (the device's elpd_loo of those rows deviates from the host's by at most %.2e, k by %.2e; %d of %d rows with k above 0.7)"
    % (psis_ref.deviation(got[0][:H], elpd).max(), psis_ref.deviation(got[1][:H], k).max(), int((got[1] > 0.7).sum()), N))
say("    the host path takes %.0f x the time of (r)" % ((med["D"] + scaled) / med["r"]))

if args.parent_root:
    here, parent = [], []
    for _ in range(args.runs):  # interleaved child processes, each with its own upload and warm-up
        for root, dst in ((args.parent_root, parent), (args.root, here)):
            out = subprocess.run(child_cmd("d", root), check=True, capture_output=True, text=True, timeout=600).stdout
            dst.append(json.loads(out.strip().splitlines()[-1])["median_s"])
    say("%s against the parent commit, one process per run, interleaved:" % names["d"].strip())
    say("  parent   %s" % spread(parent))
    say("  this one %s" % spread(here))
    m = float(np.median(here))
    say("  this tree's median run %.3f ms %s the parent's runs [%.3f, %.3f] ms"
        % (1e3 * m, "lies within" if min(parent) <= m <= max(parent) else "lies BELOW" if m < min(parent) else "lies ABOVE",
           1e3 * min(parent), 1e3 * max(parent)))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
