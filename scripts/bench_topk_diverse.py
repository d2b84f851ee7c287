"""The diversified top-k at README's shape (4096 queries x 10 677 items, rank 32, 95 samples, k = 10, pool 64 and 128), DESIGN 4.13.6:
  (a) mfm_pairs_topk_diverse_store, the whole call on an open handle;
  (b) mfm_pairs_topk_store with k = pool alone on the same handle -- (a) - (b) is the price of diversification;
  (c) the host alternative: the pool from (b), the items' V of every sample on the host, per-sample normalisation, the pool's Gram
      matrix and a NumPy greedy loop per query -- timed on --host-queries queries and scaled to all of them (the pool call is not
      part of it);
the three in turns, one warm-up each, `reps` repetitions, medians and ranges. --trace: instead, one call of (a) per pool under
`rocprofv3 --kernel-trace --stats` in a child process of its own, for the split between the pool, k_div_pack and k_div_select.
The samples are random draws pushed into a device store; the model's quality plays no role in the timing. Writes the report to stdout
and, with --out FILE, appends it to that file."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--lam", type=float, default=0.7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-queries", type=int, default=64)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--child-pool", type=int, default=None, help=argparse.SUPPRESS)  # (the traced child runs one call once)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, k, lam = args.users, args.items, args.rank, args.samples, args.k, args.lam
D = NU + NI
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def fmt(ts):
    return "median %.2f ms (min %.2f, max %.2f, %d reps)" % (1e3 * np.median(ts), 1e3 * min(ts), 1e3 * max(ts), len(ts))


if args.trace:
    say("kernel split of one topk_diverse call per pool (rocprofv3 --kernel-trace --stats, a child process each)")
    for pool in (64, 128):
        tmp = tempfile.mkdtemp()
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--child-pool", str(pool)] + [a for a in sys.argv[1:] if a not in ("--trace",)], check=True, stdout=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
        say("  pool %d:" % pool)
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]:
            say("    %-60s calls %4s  total %9.3f ms" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6))
        shutil.rmtree(tmp, ignore_errors=True)
else:
    rng = np.random.default_rng(0)
    store = _capi.Store(D, K)
    Vs = []
    for _ in range(S):
        V = rng.normal(size=(D, K)) * 0.2
        store.push(float(rng.normal()), rng.normal(size=D) * 0.3, V)
        Vs.append(V[NU:])
    users = np.sort(np.random.default_rng(1).choice(NU, size=args.queries, replace=False))
    Xq = sps.csr_matrix((np.ones(users.size), (np.arange(users.size), users)), shape=(users.size, D))
    Xi = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))
    pairs = _capi.Pairs(Xq, Xi)
    if args.child_pool:
        pairs.topk_diverse_store(store, k, lam, args.child_pool)
        sys.exit(0)
    Qn = np.concatenate([V / np.linalg.norm(V, axis=1, keepdims=True) for V in Vs], axis=1)  # (items, S K): done once, not timed

    def host(pool_idx, pool_val):
        out = np.empty((args.host_queries, k), dtype=np.int64)
        for u in range(args.host_queries):
            c, v = pool_idx[u], pool_val[u]
            G = (Qn[c] @ Qn[c].T) / S
            rel = (v - v[-1]) / (v[0] - v[-1])
            ms, taken, j = np.full(c.size, -np.inf), np.zeros(c.size, dtype=bool), 0
            for t in range(k):
                if t:
                    j = int(np.argmax(np.where(taken, -np.inf, lam * rel - (1 - lam) * ms)))
                out[u, t], taken[j] = c[j], True
                ms = np.maximum(ms, G[j])
        return out

    say("predict_topk_diverse, %d queries x %d items, rank %d, %d samples, k = %d, lam = %.1f" % (args.queries, NI, K, S, k, lam))
    for pool in (64, 128):
        calls = {"diverse": lambda: pairs.topk_diverse_store(store, k, lam, pool), "topk(pool)": lambda: pairs.topk_store(store, pool)}
        pidx, pval = calls["topk(pool)"]()
        calls["host greedy"] = lambda: host(pidx, pval)
        ts = {name: [] for name in calls}
        got = calls["diverse"]()
        for fn in calls.values():
            fn()  # warm-up
        for _ in range(args.reps):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - t0)
        agree = float(np.mean(got[0][:args.host_queries] == calls["host greedy"]()))
        say("  pool %3d  the host loop's picks equal the device's in %.1f %% of the entries (fp64 against fp64: near-ties may differ)" % (pool, 100 * agree))
        say("  pool %3d  (a) topk_diverse:      %s" % (pool, fmt(ts["diverse"])))
        say("            (b) topk(k = pool):    %s" % fmt(ts["topk(pool)"]))
        say("            (a) - (b), medians:    %.2f ms" % (1e3 * (np.median(ts["diverse"]) - np.median(ts["topk(pool)"]))))
        say("            (c) host greedy on %d queries: %s; scaled by %d / %d to all: %.0f ms" % (
            args.host_queries, fmt(ts["host greedy"]), args.queries, args.host_queries,
            1e3 * np.median(ts["host greedy"]) * args.queries / args.host_queries))
    pairs.close()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
