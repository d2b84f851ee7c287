"""Chain diagnostics at the config-3 shape (69 878 users + 10 677 items one-hot, rank 32, 95 samples, 1 M rows), DESIGN 4.9.4:
  (pr) (pc) (po)  predict_diagnostics of a regressor / classifier / ordered probit (5 classes): mfm_design_ess_store, kind 0;
  (lr) (lc) (lo)  likelihood_diagnostics of the same three: kind 1;
  (s)             predict_dist(quantiles=()) of the regressor (mfm_design_summary_store): the cheapest pass over the same scores;
  (d) (D)         predict_log_density of the regressor, and with pointwise=True (the (S, N) matrix to the host);
  (l)             predict_loo(r_eff=1.0) of the regressor (mfm_design_loo_store), in this tree and, with --parent-root, in the
                  parent: the existing call is unchanged;
  --chains M      the six diagnostics calls once more with the samples read as M chains of samples / M draws each (n_chains = M:
                  the AR(1) sequence starts afresh at every chain), next to the single-chain calls of the same run;
  (h)             what a user had to do before for the likelihood's diagnostics: (D), then the vectorised NumPy reference of
                  tests/ess_ref.py on the host. The host part is timed on the first `--host-rows` rows and scaled to all rows (it
                  is linear in the rows); the report says so.
The samples are an AR(1) sequence in the sample index (phi = `--phi`) around one model pushed into a device store (what a fit
keeps), the targets random; the model's quality plays no role in the timing, the autocorrelation sets how many lag batches a row
needs (at 95 samples: one, whatever phi is). Every device variant is timed end to end (the call on an uploaded design: kernels,
copy back, synchronisation) in `--runs` runs of `--reps` calls each after one warm-up, the runs of the variants interleaved; a run
reports its median call.

--parent-root DIR: a built checkout of the parent commit. Its predict_loo and its six single-chain diagnostics calls are timed in
child processes alternating with this tree's, `--runs` runs each (a child uploads once and times every variant), and the report
says per variant whether this tree's median run lies within the spread of the parent's runs.
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
ap.add_argument("--phi", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help=argparse.SUPPRESS)
ap.add_argument("--chains", type=int, default=1)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # variants, comma-separated: a JSON line of their runs
args = ap.parse_args()
if args.chains < 1 or args.samples % args.chains:
    ap.error("--samples must be a multiple of --chains")
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
    a0, aw, aV = 0.0, np.zeros(D), np.zeros((D, K))
    innov = np.sqrt(1.0 - args.phi ** 2)
    for k in range(S):  # an autocorrelated chain around one model (--chains: one per chain)
        if k % (S // args.chains) == 0:
            a0, aw, aV = 0.0, np.zeros(D), np.zeros((D, K))
        a0 = args.phi * a0 + innov * float(rng.normal())
        aw = args.phi * aw + innov * rng.normal(size=D)
        aV = args.phi * aV + innov * rng.normal(size=(D, K))
        store.push(w0 + 0.05 * a0, w + 0.05 * aw, V + 0.02 * aV)
    indices = np.empty((N, 2), dtype=np.int32)
    indices[:, 0] = np.sort(rng.integers(0, NU, size=N))
    indices[:, 1] = NU + rng.integers(0, NI, size=N)
    X = sps.csr_matrix((np.ones(2 * N), indices.ravel(), np.arange(0, 2 * N + 1, 2, dtype=np.int64)), shape=(N, D))
    alphas = np.exp(rng.normal(size=S) * 0.1) * 1.5
    cuts = np.sort(rng.normal(size=(S, N_CUT)) * 0.1 + np.array([-1.5, -0.5, 0.5, 1.5]), axis=1)
    y = {0: rng.normal(size=N), 1: (rng.random(N) < 0.5).astype(np.float64), 2: rng.integers(0, N_CUT + 1, size=N).astype(np.float64)}
    design = _capi.Design(X)
    calls = {"s": lambda: store.summary(design, 0, ()),
             "d": lambda: store.log_density(design, 0, y[0], precisions=alphas),
             "D": lambda: store.log_density(design, 0, y[0], precisions=alphas, pointwise=True),
             "l": lambda: store.loo(design, 0, y[0], precisions=alphas)}
    if hasattr(store, "ess"):
        for name, task, kw in (("r", 0, dict(precisions=alphas)), ("c", 1, {}), ("o", 2, dict(cutpoints=cuts))):
            calls["p" + name] = lambda task=task, kw=kw: store.ess(design, 0, task, cutpoints=kw.get("cutpoints"))
            calls["l" + name] = lambda task=task, kw=kw: store.ess(design, 1, task, y[task], **kw)
        if args.chains > 1 and not args.child:
            for name, task, kw in (("r", 0, dict(precisions=alphas)), ("c", 1, {}), ("o", 2, dict(cutpoints=cuts))):
                calls["p" + name + "M"] = lambda task=task, kw=kw: store.ess(design, 0, task, cutpoints=kw.get("cutpoints"), n_chains=args.chains)
                calls["l" + name + "M"] = lambda task=task, kw=kw: store.ess(design, 1, task, y[task], n_chains=args.chains, **kw)
    return calls


def one_run(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


if args.child:
    calls = setup()
    out = {}
    for v in args.child.split(","):
        calls[v]()  # warm-up
        out[v] = one_run(calls[v], args.reps)
    print(json.dumps({"median_s": out}), flush=True)
    sys.exit(0)


def child_cmd(variant, root):
    return [sys.executable, os.path.abspath(__file__), "--child", variant, "--root", root, "--users", str(NU), "--items", str(NI), "--rank",
            str(K), "--samples", str(S), "--rows", str(N), "--reps", str(args.reps), "--phi", str(args.phi), "--chains", str(args.chains)]


def spread(ts):
    return "%s ms (min %.3f, max %.3f)" % (", ".join("%.3f" % (1e3 * t) for t in ts), 1e3 * min(ts), 1e3 * max(ts))


say("chain diagnostics at the config-3 shape: %d + %d one-hot columns, rank %d, %d samples (%sAR(1) in the sample index, phi = %.2f), "
    "%d rows; ordered probit with %d classes"
    % (NU, NI, K, S, "%d chains of %d, each " % (args.chains, S // args.chains) if args.chains > 1 else "", args.phi, N, N_CUT + 1))
calls = setup()
for fn in calls.values():
    fn()  # warm-up
runs = {v: [] for v in calls}
for _ in range(args.runs):  # interleaved
    for v, fn in calls.items():
        runs[v].append(one_run(fn, args.reps))
names = {"s": "(s)  predict_dist(quantiles=()), regression   ", "d": "(d)  log density, regression                 ",
         "D": "(D)  log density, regression, pointwise      ", "l": "(l)  predict_loo(r_eff=1.0), regression      ",
         "pr": "(pr) predict_diagnostics, regression         ", "pc": "(pc) predict_diagnostics, classification     ",
         "po": "(po) predict_diagnostics, ordered probit     ", "lr": "(lr) likelihood_diagnostics, regression      ",
         "lc": "(lc) likelihood_diagnostics, classification  ", "lo": "(lo) likelihood_diagnostics, ordered probit  "}
for v in list(names):
    if v[0] in "pl" and len(v) == 2:
        names[v + "M"] = names[v].rstrip().replace(")", "M)", 1) + ", %d chains " % args.chains
say("end to end, median call of each of %d runs of %d calls:" % (args.runs, args.reps))
for v in calls:
    say("  %s %s" % (names[v], spread(runs[v])))
med = {v: float(np.median(t)) for v, t in runs.items()}
say("  predict_diagnostics takes %.1f x predict_dist(quantiles=()), likelihood_diagnostics %.1f x predict_log_density, %.1f x predict_loo (regression)"
    % (med["pr"] / med["s"], med["lr"] / med["d"], med["lr"] / med["l"]))

# (h) the host path: the matrix of (D), then the NumPy reference on a row subset, scaled
from tests import ess_ref  # noqa: E402

ll = calls["D"]()[4]
H = min(args.host_rows, N)
sub = np.ascontiguousarray(ll[:, :H])
table = _capi.rank_z_table(S)
ess_ref.likelihood_diagnostics(sub[:, : min(H, 1000)], table)  # warm-up
host = []
for _ in range(args.runs):
    t0 = time.perf_counter()
    want = ess_ref.likelihood_diagnostics(sub, table)
    host.append(time.perf_counter() - t0)
scaled = float(np.median(host)) * N / H
say("(h) the host path: (D) %.1f ms + the NumPy reference of tests/ess_ref.py on the first %d rows %s, SCALED by %d / %d to %.0f ms: %.0f ms"
    % (1e3 * med["D"], H, spread(host), N, H, 1e3 * scaled, 1e3 * (med["D"] + scaled)))
got = calls["lr"]()
use = ~want.near
say("    (the device's r_eff of those rows deviates from the host's by at most %.2e, rhat by %.2e; %d rows near a Geyer decision left out;"
    % (ess_ref.deviation(got[2][:H][use], want.r_eff[use]).max(), ess_ref.deviation(got[0][:H][use], want.rhat[use]).max(), int(want.near.sum())))
say("     over all %d rows: mean r_eff %.3f, %d rows with rhat above 1.01, median truncation lag of the first %d rows %d)"
    % (N, float(np.nanmean(got[2])), int((got[0] > 1.01).sum()), H, int(np.median(want.T))))
say("    the host path takes %.0f x the time of (lr)" % ((med["D"] + scaled) / med["lr"]))

if args.parent_root:
    variants = ["l", "pr", "lr", "pc", "lc", "po", "lo"]
    here, parent = {v: [] for v in variants}, {v: [] for v in variants}
    for _ in range(args.runs):  # alternating child processes, each with its own upload and warm-up
        for root, dst in ((args.parent_root, parent), (args.root, here)):
            out = subprocess.run(child_cmd(",".join(variants), root), check=True, capture_output=True, text=True, timeout=600).stdout
            for v, t in json.loads(out.strip().splitlines()[-1])["median_s"].items():
                dst[v].append(t)
    say("the single-chain calls against the parent commit, one process per run, alternating:")
    for v in variants:
        say("  %s" % names[v].strip())
        say("    parent   %s" % spread(parent[v]))
        say("    this one %s" % spread(here[v]))
        m = float(np.median(here[v]))
        say("    this tree's median run %.3f ms %s the parent's runs [%.3f, %.3f] ms"
            % (1e3 * m, "lies within" if min(parent[v]) <= m <= max(parent[v]) else "lies BELOW" if m < min(parent[v]) else "lies ABOVE",
               1e3 * min(parent[v]), 1e3 * max(parent[v])))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
