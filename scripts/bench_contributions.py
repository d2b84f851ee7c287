"""The score's decomposition by field at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples, 1 M test
rows), DESIGN 4.9.7:
  (p) predict(): the mean score (mfm_design_predict_store);
  (q) predict_dist() without quantiles: mean and standard deviation (mfm_design_summary_store);
  (k) predict_contributions, two fields (users, items): F = 2, P = 3 (mfm_design_contrib_store);
  (p6) (q6) (k6) the same three on a six-field design of the same size: four more one-hot fields of 365, 20, 10 and 21 columns, F = 6, P = 21;
  (b) what a user had to do before: every kept sample to the host (Store.get), then the float64 reference of tests/contrib_ref.py on
      the first `--ref-rows` rows of the two-field design, scaled linearly to all rows (the report says that it is scaled).
The samples are random draws pushed into a device store (what a fit keeps); the model's quality plays no role in the timing. Every
variant is timed end to end (the call on an uploaded design: kernels, copy back, synchronisation) in `--runs` runs of `--reps` calls
each after one warm-up, the runs of the variants interleaved; a run reports its median call.

--parent-root DIR: a built checkout of the parent commit. Its (q) is timed in child processes interleaved with this tree's, `--runs`
runs each, and the report says whether this tree's lies within the spread of the parent's runs.
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
ap.add_argument("--child", choices=["q"], default=None, help=argparse.SUPPRESS)  # one variant: a JSON line of its run
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, N = args.users, args.items, args.rank, args.samples, args.rows
EXTRA = (365, 20, 10, 21)
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def make(widths, seed):
    """a store of S random samples and an uploaded one-hot design of one entry per field"""
    rng = np.random.default_rng(seed)
    D, m = int(sum(widths)), len(widths)
    store = _capi.Store(D, K)
    for _ in range(S):
        store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
    off = np.concatenate([[0], np.cumsum(widths)[:-1]])
    indices = np.empty((N, m), dtype=np.int32)
    indices[:, 0] = np.sort(rng.integers(0, widths[0], size=N))
    for f in range(1, m):
        indices[:, f] = off[f] + rng.integers(0, widths[f], size=N)
    X = sps.csr_matrix((np.ones(m * N), indices.ravel(), np.arange(0, m * N + 1, m, dtype=np.int64)), shape=(N, D))
    field_of = np.repeat(np.arange(m), widths).astype(np.int32)
    return store, _capi.Design(X), X, field_of


def setup(six=True):
    calls, keep = {}, []
    for tag, widths, seed in (("", (NU, NI), 0),) + ((("6", (NU, NI) + EXTRA, 1),) if six else ()):
        store, design, X, fo = make(widths, seed)
        keep.append((store, design, X, fo))
        calls["p" + tag] = lambda store=store, design=design: store.predict(design)
        calls["q" + tag] = lambda store=store, design=design: store.summary(design, 0, ())
        if hasattr(store, "contributions"):
            calls["k" + tag] = lambda store=store, design=design, fo=fo, m=len(widths): store.contributions(design, m, fo)
    return calls, keep


def one_run(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


if args.child:
    fn = setup(six=False)[0][args.child]
    fn()  # warm-up
    print(json.dumps({"variant": args.child, "median_s": one_run(fn, args.reps)}), flush=True)
    sys.exit(0)


def child_cmd(variant, root):
    return [sys.executable, os.path.abspath(__file__), "--child", variant, "--root", root, "--users", str(NU), "--items", str(NI), "--rank",
            str(K), "--samples", str(S), "--rows", str(N), "--reps", str(args.reps)]


def spread(ts):
    return "%s ms (min %.3f, max %.3f)" % (", ".join("%.3f" % (1e3 * t) for t in ts), 1e3 * min(ts), 1e3 * max(ts))


say("score contributions at the config-3 shape: %d + %d one-hot columns, rank %d, %d samples, %d rows; six fields: %s more columns"
    % (NU, NI, K, S, N, " + ".join(str(v) for v in EXTRA)))
calls, keep = setup()
for fn in calls.values():
    fn()  # warm-up
runs = {v: [] for v in calls}
for _ in range(args.runs):  # interleaved
    for v, fn in calls.items():
        runs[v].append(one_run(fn, args.reps))
names = {"p": "(p)  predict, two fields               ", "q": "(q)  predict_dist, no quantiles, two   ", "k": "(k)  predict_contributions, F = 2      ",
         "p6": "(p6) predict, six fields               ", "q6": "(q6) predict_dist, no quantiles, six   ", "k6": "(k6) predict_contributions, F = 6      "}
say("end to end, median call of each of %d runs of %d calls:" % (args.runs, args.reps))
for v in calls:
    say("  %s %s" % (names[v], spread(runs[v])))
med = {v: float(np.median(t)) for v, t in runs.items()}
say("  medians of the runs: (k)/(q) %.2f, (k6)/(q6) %.2f" % (med["k"] / med["q"], med["k6"] / med["q6"]))
for tag, m in (("", 2), ("6", 6)):
    gather = S * N * m * (K + 1) * 8.0  # every entry's factor row and weight under every sample
    out = 2.0 * (m + m * (m + 1) // 2) * N * 8.0
    say("  (k%s): %.1f GB gathered from the staged samples (%.2f TB/s over the call), %.0f MB of results written and copied back"
        % (tag, gather / 1e9, gather / med["k" + tag] / 1e12, out / 1e6))

# (b) the host route: the samples to the host, then NumPy on a slice of the rows
from tests import contrib_ref as cr  # noqa: E402
from tests.score_ref import flat_rows  # noqa: E402

store, design, X, fo = keep[0]
t0 = time.perf_counter()
samples = [store.get(k) for k in range(S)]
t_get = time.perf_counter() - t0
n_ref = min(args.ref_rows, N)
rows = flat_rows(X[:n_ref])
t0 = time.perf_counter()
per_sample = np.stack([cr.components_f64(rows, w, V, fo, 2) for _, w, V in samples])
ref_mean, ref_std = cr.moments_f64(per_sample)
t_ref = time.perf_counter() - t0
got = calls["k"]()
mean = np.concatenate([got[2], got[4]])[:, :n_ref]
std = np.concatenate([got[3], got[5]])[:, :n_ref]
dev = max(float(np.abs(mean - ref_mean).max()), float(np.abs(std - ref_std).max()))
say("(b) before, two fields: %d samples to the host %.3f s; NumPy float64 on %d rows %.3f s, scaled linearly to %d rows: %.1f s (SCALED, not run);"
    % (S, t_get, n_ref, t_ref, N, t_ref * N / n_ref))
say("    together %.1f s against %.3f s of (k): %.0f x. Largest deviation of (k) from that reference on the %d rows: %.2e"
    % (t_get + t_ref * N / n_ref, med["k"], (t_get + t_ref * N / n_ref) / med["k"], n_ref, dev))

if args.parent_root:
    here, parent = [], []
    for _ in range(args.runs):  # interleaved child processes, each with its own upload and warm-up
        for root, dst in ((args.parent_root, parent), (args.root, here)):
            out = subprocess.run(child_cmd("q", root), check=True, capture_output=True, text=True, timeout=600).stdout
            dst.append(json.loads(out.strip().splitlines()[-1])["median_s"])
    say("%s against the parent commit, one process per run, interleaved:" % names["q"].strip())
    say("  parent   %s" % spread(parent))
    say("  this one %s" % spread(here))
    m = float(np.median(here))
    say("  this tree's median run %.3f ms %s the parent's runs [%.3f, %.3f] ms"
        % (1e3 * m, "lies within" if min(parent) <= m <= max(parent) else "lies BELOW" if m < min(parent) else "lies ABOVE",
           1e3 * min(parent), 1e3 * max(parent)))
say("not measured: kernel times from a trace, other S, other ranks, relation-block designs, more than six fields")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
