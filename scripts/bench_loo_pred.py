"""Leave-one-out predictions at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples, 1 M rows), DESIGN
4.9.6:
  (s) (S)      predict_loo_dist of a regression target with the quantiles (0.05, 0.5, 0.95) / with quantiles=() (mfm_design_loo_summary_store);
  (x)          predict_loo_crps of the regression target (mfm_design_loo_crps_store);
  (sc) (xc) (so) (xo)  both for a classification and an ordered-probit (5 classes) target;
  (l) (L) (k)  beside them on the same visit: predict_loo(), predict_loo(log_weights=True) and predict_crps() of the regression target;
  (h)          the host route to the same numbers: predict_loo(log_weights=True) (the (S, N) log weights to the host), the per-sample
               scores by one single-sample predict call per sample, then the NumPy reference of tests/loo_pred_ref.py. The NumPy
               parts are timed on the first `--host-rows` (summary) and `--host-crps-rows` (CRPS) rows and scaled to all rows (they
               are linear in the rows); the report says so;
  (l) against the parent commit with --parent-root: the existing call is unchanged.
The samples are random draws around one model pushed into a device store (what a fit keeps), the targets random; the model's
quality plays no role in the timing. Every device variant is timed end to end (the call on an uploaded design: kernels, copy back,
synchronisation) in `--runs` runs of `--reps` calls each after one warm-up, the runs of the variants interleaved; a run reports its
median call.

--parent-root DIR: a built checkout of the parent commit. Its predict_loo() is timed in child processes interleaved with this
tree's, `--parent-runs` (default `--runs`) runs each, and the report says whether this tree's lies within the spread of the parent's runs.
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
ap.add_argument("--host-crps-rows", type=int, default=2_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--parent-runs", type=int, default=None, help="runs of the comparison with the parent (default: --runs)")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help=argparse.SUPPRESS)
ap.add_argument("--child", choices=["l"], default=None, help=argparse.SUPPRESS)  # one variant: a JSON line of its run
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, N = args.users, args.items, args.rank, args.samples, args.rows
D = NU + NI
N_CUT = 4
QUANTILES = (0.05, 0.5, 0.95)
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
    kws = {0: dict(precisions=alphas), 1: {}, 2: dict(cutpoints=cuts)}
    calls = {"l": lambda: store.loo(design, 0, y[0], **kws[0]),
             "L": lambda: store.loo(design, 0, y[0], log_weights=True, **kws[0])}
    if hasattr(store, "loo_summary"):
        calls["k"] = lambda: store.crps(design, 0, y[0], **kws[0])
        for tag, task in (("", 0), ("c", 1), ("o", 2)):
            calls["s" + tag] = lambda task=task: store.loo_summary(design, task, y[task], quantiles=QUANTILES, **kws[task])
            calls["x" + tag] = lambda task=task: store.loo_crps(design, task, y[task], **kws[task])
        calls["S"] = lambda: store.loo_summary(design, 0, y[0], **kws[0])
    return calls, dict(store=store, design=design, y=y, alphas=alphas)


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


say("leave-one-out predictions at the config-3 shape: %d + %d one-hot columns, rank %d, %d samples, %d rows; ordered probit with %d classes"
    % (NU, NI, K, S, N, N_CUT + 1))
calls, ctx = setup()
for fn in calls.values():
    fn()  # warm-up
runs = {v: [] for v in calls}
for _ in range(args.runs):  # interleaved
    for v, fn in calls.items():
        runs[v].append(one_run(fn, args.reps))
names = {"l": "(l)  predict_loo, regression                      ", "L": "(L)  predict_loo, regression, log weights         ",
         "k": "(k)  predict_crps, regression                     ", "s": "(s)  predict_loo_dist, regression, 3 quantiles    ",
         "S": "(S)  predict_loo_dist, regression, no quantiles   ", "x": "(x)  predict_loo_crps, regression                 ",
         "sc": "(sc) predict_loo_dist, classification, 3 quantiles", "xc": "(xc) predict_loo_crps, classification             ",
         "so": "(so) predict_loo_dist, ordered probit, 3 quantiles", "xo": "(xo) predict_loo_crps, ordered probit             "}
say("end to end, median call of each of %d runs of %d calls:" % (args.runs, args.reps))
for v in calls:
    say("  %s %s" % (names[v], spread(runs[v])))
med = {v: float(np.median(t)) for v, t in runs.items()}
say("  log_weights=True copies %.2f GB to the host; the new calls copy %d and 4 columns of %d doubles" % (8.0 * N * S / 1e9, 5 + len(QUANTILES), N))

# (h) the host route: the weights of (L), the scores sample by sample, then the NumPy reference on a row subset, scaled
from tests import loo_pred_ref as lr  # noqa: E402

store, design, y, alphas = ctx["store"], ctx["design"], ctx["y"][0], ctx["alphas"]
lw = calls["L"]()[4]
t0 = time.perf_counter()
f = np.stack([store.predict(design, 0, first=s, count=1) for s in range(S)])
t_scores = time.perf_counter() - t0
H, HC = min(args.host_rows, N), min(args.host_crps_rows, N)
host_s, host_c = [], []
for _ in range(args.runs):
    t0 = time.perf_counter()
    ref_s = lr.summary(f[:, :H], lw[:, :H], QUANTILES, 1.0 / alphas)
    host_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref_c = lr.crps(0, f[:, :HC], lw[:, :HC], y[:HC], alphas)
    host_c.append(time.perf_counter() - t0)
sc_s, sc_c = float(np.median(host_s)) * N / H, float(np.median(host_c)) * N / HC
say("(h) the host route, regression: (L) %.1f ms + the scores by %d single-sample predict calls %.1f ms, then tests/loo_pred_ref.py:"
    % (1e3 * med["L"], S, 1e3 * t_scores))
say("    summary on the first %d rows %s, scaled by %d / %d to %.0f ms: %.0f ms in all, %.0f x (s)"
    % (H, spread(host_s), N, H, 1e3 * sc_s, 1e3 * (med["L"] + t_scores + sc_s), (med["L"] + t_scores + sc_s) / med["s"]))
say("    CRPS on the first %d rows %s, scaled by %d / %d to %.0f ms: %.0f ms in all, %.0f x (x)"
    % (HC, spread(host_c), N, HC, 1e3 * sc_c, 1e3 * (med["L"] + t_scores + sc_c), (med["L"] + t_scores + sc_c) / med["x"]))
got_s, got_c = calls["s"](), calls["x"]()
keep = ~ref_s[5]
say("    (the device deviates from the host's numbers on those rows by at most: mean %.2e, std %.2e, std_y %.2e, ess %.2e, quantiles %.2e "
    "with %d of %d cells left out, crps %.2e, accuracy %.2e, spread %.2e; %d of %d rows with k above 0.7)"
    % (lr.deviation(got_s[0][:H], ref_s[0]).max(), lr.deviation(got_s[1][:H], ref_s[1]).max(), lr.deviation(got_s[3][:H], ref_s[3]).max(),
       lr.deviation(got_s[4][:H], ref_s[4]).max(), lr.deviation(got_s[2][:, :H], ref_s[2])[keep].max(), int((~keep).sum()), keep.size,
       lr.deviation(got_c[0][:HC], ref_c[0]).max(), lr.deviation(got_c[1][:HC], ref_c[1]).max(), lr.deviation(got_c[2][:HC], ref_c[2]).max(),
       int((got_s[5] > 0.7).sum()), N))
say("    (pareto_k of (s) and (x) equals predict_loo's bit for bit: %s)"
    % (np.array_equal(got_s[5], calls["l"]()[1]) and np.array_equal(got_c[3], got_s[5])))

if args.parent_root:
    here, parent = [], []
    for _ in range(args.parent_runs or args.runs):  # interleaved child processes, each with its own upload and warm-up
        for root, dst in ((args.parent_root, parent), (args.root, here)):
            out = subprocess.run(child_cmd("l", root), check=True, capture_output=True, text=True, timeout=600).stdout
            dst.append(json.loads(out.strip().splitlines()[-1])["median_s"])
    say("%s against the parent commit, one process per run, interleaved:" % names["l"].strip())
    say("  parent   %s" % spread(parent))
    say("  this one %s" % spread(here))
    m = float(np.median(here))
    say("  this tree's median run %.3f ms %s the parent's runs [%.3f, %.3f] ms"
        % (1e3 * m, "lies within" if min(parent) <= m <= max(parent) else "lies BELOW" if m < min(parent) else "lies ABOVE",
           1e3 * min(parent), 1e3 * max(parent)))
say("not measured: kernel times from a trace (every figure is an end-to-end call); other sample counts; designs with relation blocks")
if args.out:
    with open(args.out, "w") as f_out:
        f_out.write("\n".join(lines) + "\n")
