"""Ranking under each kept sample at bench_topk.py's shape (4096 queries x 10 677 items, rank 32, 95 samples, k = 10), DESIGN
4.13.3, every timing a whole call (upload of nothing but the arguments, kernels, copy back), one warm-up and the median of
`reps` repetitions:
  (a) what the library offered before: a loop of S single-sample Pairs.topk_store(first=s, count=1) calls for the lists, and a
      NumPy vote (per query np.unique of its S * k entries, then a lexsort by (-count, index)) for the probabilities;
  (b) Pairs.topk_samples_store: every sample's list in one call;
  (c) Pairs.topk_prob_store: the top-k inclusion probabilities, the lists counted on the device;
  (d) Pairs.topk_samples_store(row_sample=...), the Thompson list, next to Pairs.topk_store (predict_topk) of the same inputs.
The samples are random draws pushed into a device store (what a fit keeps); the model's quality plays no role in the timing.
The results of (b), (c), (d) are compared with (a)'s bit for bit. The kernel split of (b), (d) and predict_topk comes from a child
process each under `rocprofv3 --kernel-trace --stats` (skipped, and said so, where rocprofv3 is not installed).
Writes the report to stdout and, with --out FILE, to that file."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myfm_amd import _capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=0, help="of the Thompson draw")
ap.add_argument("--out", default=None)
ap.add_argument("--variant", choices=["samples", "thompson", "topk", "prob"], default=None, help=argparse.SUPPRESS)  # (the traced child)
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


def numpy_vote(idx, n_top):
    n_s, n_u = idx.shape[:2]
    flat = idx.transpose(1, 0, 2).reshape(n_u, -1)
    out_i, out_p = np.full((n_u, n_top), -1, dtype=np.int64), np.zeros((n_u, n_top))
    for u in range(n_u):
        cand, count = np.unique(flat[u][flat[u] >= 0], return_counts=True)
        order = np.lexsort((cand, -count))[:n_top]
        out_i[u, :order.size], out_p[u, :order.size] = cand[order], count[order] / np.float64(n_s)
    return out_i, out_p


def kernel_split(variant):
    """{kernel name: total ms} of one child run under rocprofv3 --kernel-trace --stats, or a string saying why there is none"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="topk_samples_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--variant", variant, "--users", str(NU), "--items", str(NI), "--rank", str(K), "--samples",
               str(S), "--queries", str(U), "--k", str(k), "--seed", str(args.seed)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        parts = {}
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    short = row["Name"].split("(")[0].split("::")[-1].split("<")[0]
                    parts[short] = parts.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6
        return parts or "the trace held no kernel statistics"
    except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
        return type(e).__name__
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


rng = np.random.default_rng(0)
store = _capi.Store(D, K)
for _ in range(S):
    store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
users = np.sort(rng.choice(NU, size=U, replace=False))
Xq = sps.csr_matrix((np.ones(U), (np.arange(U), users)), shape=(U, D))
Xc = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))
pairs = _capi.Pairs(Xq, Xc)
row_sample = np.random.default_rng(args.seed).integers(0, S, size=U)
calls = {"samples": lambda: pairs.topk_samples_store(store, k), "prob": lambda: pairs.topk_prob_store(store, k),
         "thompson": lambda: pairs.topk_samples_store(store, k, row_sample=row_sample), "topk": lambda: pairs.topk_store(store, k)}
if args.variant:  # the traced child: one call, nothing reported
    calls[args.variant]()
    pairs.close()
    sys.exit(0)


def loop():
    idx, val = np.empty((S, U, k), dtype=np.int64), np.empty((S, U, k))
    for s in range(S):
        idx[s], val[s] = pairs.topk_store(store, k, first=s, count=1)
    return idx, val


say("ranking under each kept sample: %d queries x %d items, rank %d, %d samples, k = %d, regressor's value (mode 0)" % (U, NI, K, S, k))
fmt = "median %.4f s (min %.4f, max %.4f, %d reps)"
(idx_a, val_a), a_loop, lo, hi = timed(loop, args.reps)
say("(a) loop of %d single-sample topk_store calls:   " % S + fmt % (a_loop, lo, hi, args.reps))
(vi_a, vp_a), a_vote, lo, hi = timed(lambda: numpy_vote(idx_a, k), args.reps)
say("(a) NumPy vote of the %d x %d x %d lists:        " % (S, U, k) + fmt % (a_vote, lo, hi, args.reps))
(idx_b, val_b), b, lo, hi = timed(calls["samples"], args.reps)
say("(b) topk_samples_store:                           " + fmt % (b, lo, hi, args.reps))
(vi_c, vp_c), c, lo, hi = timed(calls["prob"], args.reps)
say("(c) topk_prob_store (n_top = k):                  " + fmt % (c, lo, hi, args.reps))
(idx_d, val_d), d, lo, hi = timed(calls["thompson"], args.reps)
say("(d) topk_samples_store(row_sample), Thompson:     " + fmt % (d, lo, hi, args.reps))
_, t, lo, hi = timed(calls["topk"], args.reps)
say("    topk_store of the same inputs (predict_topk): " + fmt % (t, lo, hi, args.reps))
same = (np.array_equal(idx_a, idx_b) and np.array_equal(val_a, val_b), np.array_equal(vi_a, vi_c) and np.array_equal(vp_a, vp_c),
        np.array_equal(idx_d, idx_a[row_sample, np.arange(U)]) and np.array_equal(val_d, val_a[row_sample, np.arange(U)]))
say("    (b) equals (a)'s lists bit for bit: %s; (c) equals (a)'s vote bit for bit: %s; (d) equals (a)'s lists at the drawn samples: %s" % same)
say("(b) / (a) = %.3f against the loop alone (%.3f against loop + vote); (c) / (a) = %.3f against loop + vote; "
    "(d) / predict_topk = %.3f" % (b / a_loop, b / (a_loop + a_vote), c / (a_loop + a_vote), d / t))
for name in ("samples", "thompson", "topk", "prob"):
    parts = kernel_split(name)
    if isinstance(parts, str):
        say("    %s kernel split: not measured (%s)" % (name, parts))
    else:
        say("    %s kernel time %.3f ms: %s" % (name, sum(parts.values()), ", ".join("%s %.3f" % (n, v) for n, v in sorted(parts.items(), key=lambda t: -t[1]))))
pairs.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
if not all(same):
    raise SystemExit("the per-sample calls differ from the loop of single-sample calls")
