"""Continuous ranked probability score at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples, 1 M test
rows), DESIGN 4.9.5:
  (q) predict_dist() without quantiles: mean and standard deviation (mfm_design_summary_store) -- the same stage 1, an O(S) stage 2;
  (r) (c) (o) the log density of a regression / classification / ordered-probit (5 classes) target (mfm_design_logdens_store);
  (R) (C) (O) the CRPS of the same targets (mfm_design_crps_store);
  (b) what a user had to do before, regression: S single-sample predict() calls for the scores, then the vectorised float64 form of
      tests/crps_ref.py on the first `--ref-rows` rows, scaled linearly to all rows (the report says that it is scaled).
The samples are random draws pushed into a device store (what a fit keeps), the targets random; the model's quality plays no role
in the timing. Every variant is timed end to end (the call on an uploaded design: kernels, copy back, synchronisation) in `--runs`
runs of `--reps` calls each after one warm-up, the runs of the variants interleaved; a run reports its median call. The pair-term
rate of k_row_crps_mix is S (S + 1) / 2 terms a row over the time of (R), and over (R) - (q), which takes the shared stage 1 out.

--parent-root DIR: a built checkout of the parent commit. Its regression log density (r) is timed in child processes interleaved with
this tree's, `--runs` runs each, and the report says whether this tree's lies within the spread of the parent's runs.
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
ap.add_argument("--ref-rows", type=int, default=2000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help=argparse.SUPPRESS)
ap.add_argument("--child", choices=["r"], default=None, help=argparse.SUPPRESS)  # one variant: a JSON line of its run
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
    for _ in range(S):
        store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
    indices = np.empty((N, 2), dtype=np.int32)
    indices[:, 0] = np.sort(rng.integers(0, NU, size=N))
    indices[:, 1] = NU + rng.integers(0, NI, size=N)
    X = sps.csr_matrix((np.ones(2 * N), indices.ravel(), np.arange(0, 2 * N + 1, 2, dtype=np.int64)), shape=(N, D))
    alphas = np.exp(rng.normal(size=S) * 0.1) * 1.5
    cuts = np.sort(rng.normal(size=(S, N_CUT)) + np.array([-1.5, -0.5, 0.5, 1.5]), axis=1)
    y = {0: rng.normal(size=N), 1: (rng.random(N) < 0.5).astype(np.float64), 2: rng.integers(0, N_CUT + 1, size=N).astype(np.float64)}
    design = _capi.Design(X)
    calls = {"q": lambda: store.summary(design, 0, ())}
    for name, task, kw in (("r", 0, dict(precisions=alphas)), ("c", 1, {}), ("o", 2, dict(cutpoints=cuts))):
        calls[name] = lambda task=task, kw=kw: store.log_density(design, task, y[task], **kw)
        if hasattr(store, "crps"):
            calls[name.upper()] = lambda task=task, kw=kw: store.crps(design, task, y[task], **kw)
    return calls, store, design, y[0], alphas


def one_run(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


if args.child:
    fn = setup()[0][args.child]
    fn()  # warm-up
    print(json.dumps({"variant": args.child, "median_s": one_run(fn, args.reps)}), flush=True)
    sys.exit(0)


def child_cmd(variant, root):
    return [sys.executable, os.path.abspath(__file__), "--child", variant, "--root", root, "--users", str(NU), "--items", str(NI), "--rank",
            str(K), "--samples", str(S), "--rows", str(N), "--reps", str(args.reps)]


def spread(ts):
    return "%s ms (min %.3f, max %.3f)" % (", ".join("%.3f" % (1e3 * t) for t in ts), 1e3 * min(ts), 1e3 * max(ts))


say("CRPS at the config-3 shape: %d + %d one-hot columns, rank %d, %d samples, %d rows; ordered probit with %d classes"
    % (NU, NI, K, S, N, N_CUT + 1))
calls, store, design, y0, alphas = setup()
for fn in calls.values():
    fn()  # warm-up
runs = {v: [] for v in calls}
for _ in range(args.runs):  # interleaved
    for v, fn in calls.items():
        runs[v].append(one_run(fn, args.reps))
names = {"q": "(q) predict_dist, no quantiles    ", "r": "(r) log density, regression       ", "R": "(R) CRPS, regression              ",
         "c": "(c) log density, classification   ", "C": "(C) CRPS, classification          ", "o": "(o) log density, ordered probit   ",
         "O": "(O) CRPS, ordered probit          "}
say("end to end, median call of each of %d runs of %d calls:" % (args.runs, args.reps))
for v in calls:
    say("  %s %s" % (names[v], spread(runs[v])))
med = {v: float(np.median(t)) for v, t in runs.items()}
say("  medians of the runs, CRPS over log density: " + ", ".join("(%s)/(%s) %.2f" % (v.upper(), v, med[v.upper()] / med[v]) for v in "rco"))
terms = 0.5 * S * (S + 1) * N
say("  k_row_crps_mix: %.3e pair terms (one erf, one exp each); %.3e terms/s over (R), %.3e terms/s over (R) - (q)"
    % (terms, terms / med["R"], terms / max(med["R"] - med["q"], 1e-9)))

# (b) the host path: the scores sample by sample, then NumPy on a slice of the rows
from tests import crps_ref  # noqa: E402

t0 = time.perf_counter()
scores = np.stack([store.predict(design, first=k, count=1) for k in range(S)])
t_scores = time.perf_counter() - t0
n_ref = min(args.ref_rows, N)
t0 = time.perf_counter()
ref = crps_ref.crps_mixture(scores[:, :n_ref], y0[:n_ref], alphas)
t_ref = time.perf_counter() - t0
got = calls["R"]()
dev = float(crps_ref.deviation(np.stack(got)[:, :n_ref], np.stack(ref)).max())
say("(b) before, regression: %d predict() calls %.3f s; NumPy float64 on %d rows %.3f s, scaled linearly to %d rows: %.1f s (SCALED, not run);"
    % (S, t_scores, n_ref, t_ref, N, t_ref * N / n_ref))
say("    together %.1f s against %.3f s of (R): %.0f x. Largest deviation of (R) from that reference on the %d rows: %.2e"
    % (t_scores + t_ref * N / n_ref, med["R"], (t_scores + t_ref * N / n_ref) / med["R"], n_ref, dev))

if args.parent_root:
    here, parent = [], []
    for _ in range(args.runs):  # interleaved child processes, each with its own upload and warm-up
        for root, dst in ((args.parent_root, parent), (args.root, here)):
            out = subprocess.run(child_cmd("r", root), check=True, capture_output=True, text=True, timeout=600).stdout
            dst.append(json.loads(out.strip().splitlines()[-1])["median_s"])
    say("%s against the parent commit, one process per run, interleaved:" % names["r"].strip())
    say("  parent   %s" % spread(parent))
    say("  this one %s" % spread(here))
    m = float(np.median(here))
    say("  this tree's median run %.3f ms %s the parent's runs [%.3f, %.3f] ms"
        % (1e3 * m, "lies within" if min(parent) <= m <= max(parent) else "lies BELOW" if m < min(parent) else "lies ABOVE",
           1e3 * min(parent), 1e3 * max(parent)))
say("not measured: kernel times from a trace, other S, relation-block designs, the effect of the default tile size on the scratch re-reads")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
