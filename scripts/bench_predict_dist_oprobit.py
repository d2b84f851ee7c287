"""Ordered-probit posterior summaries at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples, 1 M test
rows, 5 classes), DESIGN 4.9.1:
  (p) predict_proba(): the mean class probabilities alone (mfm_design_predict_store, mode 2);
  (c) predict_proba_dist() with three quantiles (mfm_design_summary_oprobit_store, expected = 0);
  (e) predict_expected_dist() with three quantiles (expected = 1).
The samples are random draws pushed into a device store (what a fit keeps), the cutpoints random and ascending; the model's
quality plays no role in the timing. Every variant is timed end to end (the call on an uploaded design: kernels, copy back,
synchronisation) in `--runs` runs of `--reps` calls each after one warm-up, the runs of the variants interleaved; a run reports
its median call. The kernel time of each variant is taken from a kernel trace: one call in a child process under
`rocprofv3 --kernel-trace --stats` (skipped, and said so, where rocprofv3 is not installed).

--parent-root DIR: a built checkout of the parent commit. The calls that existed there -- predict_proba() (o) and, for a
regressor over the same samples, predict() (r) and predict_dist() with three quantiles (q) -- are timed in child processes, one
per run, this tree's interleaved with the parent's, and the report compares the difference of the two trees' median runs with
the spread of the parent's runs among themselves.
Writes the report to stdout and, with --out FILE, to that file."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sps

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help=argparse.SUPPRESS)
ap.add_argument("--child", choices=["o", "r", "q", "c", "e"], default=None, help=argparse.SUPPRESS)  # one variant: a JSON line of its run
ap.add_argument("--once", action="store_true", help=argparse.SUPPRESS)  # (the traced child: warm-up and one call, nothing reported)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, N, NC = args.users, args.items, args.rank, args.samples, args.rows, args.classes
D = NU + NI
QUANTILES = (0.05, 0.5, 0.95)
PREDICTION_KERNELS = ("k_build_vt_batch", "k_score_store", "k_row_summary")
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
    cuts = np.sort(rng.normal(size=(S, NC - 1)), axis=1) * 1.5
    design = _capi.Design(X)
    calls = {"o": lambda: store.predict(design, 2, cuts), "r": lambda: store.predict(design),
             "q": lambda: store.summary(design, 0, QUANTILES)}
    if hasattr(store, "summary_oprobit"):
        calls["c"] = lambda: store.summary_oprobit(design, cuts, False, QUANTILES)
        calls["e"] = lambda: store.summary_oprobit(design, cuts, True, QUANTILES)
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
    if args.once:
        fn()
    else:
        print(json.dumps({"variant": args.child, "median_s": one_run(fn, args.reps)}), flush=True)
    sys.exit(0)


def child_cmd(variant, root, extra=()):
    return [sys.executable, os.path.abspath(__file__), "--child", variant, "--root", root, "--users", str(NU), "--items", str(NI), "--rank",
            str(K), "--samples", str(S), "--rows", str(N), "--classes", str(NC), "--reps", str(args.reps)] + list(extra)


def kernel_times(variant):
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    tmp = tempfile.mkdtemp(prefix="predict_dist_oprobit_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"] + child_cmd(variant, args.root, ["--once"])
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        parts = {}
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    short = next((k for k in PREDICTION_KERNELS if k in row["Name"]), None)
                    if short is None:  # (the store's and the design's setup runs once, not per call)
                        continue
                    parts[short] = parts.get(short, 0.0) + float(row["TotalDurationNs"]) / 2.0  # (the child calls twice: warm-up and one more)
        return parts or None
    except (subprocess.SubprocessError, OSError, KeyError, ValueError):
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def spread(ts):
    return "%s ms (min %.3f, max %.3f)" % (", ".join("%.3f" % (1e3 * t) for t in ts), 1e3 * min(ts), 1e3 * max(ts))


say("ordered-probit posterior summaries at the config-3 shape: %d + %d one-hot columns, rank %d, %d samples, %d rows, %d classes; "
    "quantiles %s" % (NU, NI, K, S, N, NC, QUANTILES))
calls = setup()
timed = ("o", "c", "e")
for v in timed:
    calls[v]()  # warm-up
runs = {v: [] for v in timed}
for _ in range(args.runs):  # interleaved
    for v in timed:
        runs[v].append(one_run(calls[v], args.reps))
names = {"o": "(p) predict_proba()                     ", "c": "(c) predict_proba_dist, 3 quantiles     ",
         "e": "(e) predict_expected_dist, 3 quantiles  "}
say("end to end, median call of each of %d runs of %d calls:" % (args.runs, args.reps))
for v in timed:
    say("  %s %s" % (names[v], spread(runs[v])))
med = {v: float(np.median(t)) for v, t in runs.items()}
say("  (c) / (p) = %.2f, (e) / (p) = %.2f (medians of the runs); (c) sorts %d values for each of %d x %d (row, class) pairs and "
    "copies back %.0f MB, (e) %d x as little" % (med["c"] / med["o"], med["e"] / med["o"], S, N, NC, 8e-6 * N * NC * (2 + len(QUANTILES)), NC))
del calls
for v in timed:
    parts = kernel_times(v)
    if parts is None:
        say("  %s kernel time: not measured (rocprofv3 not found, or its trace held no kernel statistics)" % names[v].strip())
    else:
        say("  %s kernel time %.2f ms: %s" % (names[v].strip(), sum(parts.values()) / 1e6,
                                             ", ".join("%s %.2f ms" % (n, t / 1e6) for n, t in sorted(parts.items(), key=lambda x: -x[1]))))

if args.parent_root:
    existing = {"o": "predict_proba() (ordered probit)", "r": "predict() (regressor)", "q": "predict_dist(), 3 quantiles (regressor)"}
    here, parent = {v: [] for v in existing}, {v: [] for v in existing}
    for _ in range(args.runs):  # interleaved child processes, each with its own upload and warm-up
        for v in existing:
            for root, dst in ((args.parent_root, parent), (args.root, here)):
                out = subprocess.run(child_cmd(v, root), check=True, capture_output=True, text=True, timeout=600).stdout
                dst[v].append(json.loads(out.strip().splitlines()[-1])["median_s"])
    say("the calls that existed before, against the parent commit, one process per run, interleaved:")
    for v, name in existing.items():
        m, mp, width = float(np.median(here[v])), float(np.median(parent[v])), max(parent[v]) - min(parent[v])
        say("  %s" % name)
        say("    parent   %s" % spread(parent[v]))
        say("    this one %s" % spread(here[v]))
        say("    median run %.3f ms against the parent's %.3f ms: %+.3f ms, %s the %.3f ms that the parent's %d runs spread among themselves"
            % (1e3 * m, 1e3 * mp, 1e3 * (m - mp), "within" if m - mp <= width else "BEYOND", 1e3 * width, args.runs))
else:
    say("the calls that existed before were not timed against the parent commit (no --parent-root given)")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
