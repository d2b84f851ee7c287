"""The screened top-k against predict_topk's path at bench_topk.py's shape and on the same random store: 4096 queries
of 69 878 users x 10 677 items, rank 32, 95 samples, k = 10. In one process and interleaved, one call of each per repetition after
a warm-up of both: (a) mfm_pairs_topk_store, (b) mfm_pairs_topk_screened_store alone, (c) the whole screened answer -- (b) and the
uncertified rows sent through (a)'s path, as predict_topk_screened does it. Reports median and min .. max of each, the certified
share, whether (c) equals (a) bit for bit, and the kernel split of one screened call from a child process under
`rocprofv3 --kernel-trace --stats` (skipped, and said so, where rocprofv3 is not installed). --out FILE also writes the report there."""
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
ap.add_argument("--out", default=None)
ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)  # (one screened call, nothing reported)
args = ap.parse_args()
NU, NI, K, S, U, k = args.users, args.items, args.rank, args.samples, args.queries, args.k
D = NU + NI
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


rng = np.random.default_rng(0)
store = _capi.Store(D, K)
for _ in range(S):
    store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
users = np.sort(rng.choice(NU, size=U, replace=False))
Xq = sps.csr_matrix((np.ones(U), (np.arange(U), users)), shape=(U, D))
Xc = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))
pairs = _capi.Pairs(Xq, Xc)


def plain():
    return pairs.topk_store(store, k)


def screened():
    return pairs.topk_screened_store(store, k)


def whole():
    idx, val, cert = screened()
    rows = np.flatnonzero(~cert)
    if rows.size:
        sub = _capi.Pairs(Xq[rows], Xc)
        idx[rows], val[rows] = sub.topk_store(store, k)
        sub.close()
    return idx, val, cert


if args.traced_child:
    screened()
    sys.exit(0)

calls = {"a": plain, "b": screened, "c": whole}
for fn in calls.values():
    fn()  # warm-up
times = {name: [] for name in calls}
for _ in range(args.reps):
    for name, fn in calls.items():
        t0 = time.perf_counter()
        res = fn()
        times[name].append(time.perf_counter() - t0)
        if name == "a":
            ref = res
        if name == "c":
            got = res
say("screened top-k at the config-3 shape: %d queries x %d items, rank %d, %d samples, k = %d; %d interleaved repetitions"
    % (U, NI, K, S, k, args.reps))
for name, what in (("a", "(a) predict_topk's path (fp64 MFMA)              "), ("b", "(b) screened call alone (uncertified rows open) "),
                   ("c", "(c) screened call + fallback of the open rows   ")):
    t = times[name]
    say("%s: median %.4f s (min %.4f, max %.4f)" % (what, float(np.median(t)), min(t), max(t)))
cert = got[2]
say("certified rows: %d of %d (%.1f %%); (c) equals (a) bit for bit: %s"
    % (int(cert.sum()), U, 100.0 * cert.mean(), bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))))
say("(b) takes %.2fx and (c) %.2fx the time of (a)" % (np.median(times["b"]) / np.median(times["a"]), np.median(times["c"]) / np.median(times["a"])))
if not (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])):
    raise SystemExit("the screened answer differs from predict_topk's")

prof = shutil.which("rocprofv3")
if not prof:
    say("kernel split of one screened call: not measured (rocprofv3 not found)")
else:
    tmp = tempfile.mkdtemp(prefix="topk_screen_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--traced-child", "--users", str(NU), "--items", str(NI), "--rank", str(K), "--samples", str(S), "--queries", str(U), "--k", str(k)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        parts = {}
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    short = row["Name"].split("(")[0].split("::")[-1].split("<")[0]
                    parts[short] = parts.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6
        if parts:
            say("kernel time of one screened call %.3f ms: %s"
                % (sum(parts.values()), ", ".join("%s %.3f" % (n, v) for n, v in sorted(parts.items(), key=lambda t: -t[1]))))
        else:
            say("kernel split of one screened call: not measured (the trace held no kernel statistics)")
    except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
        say("kernel split of one screened call: not measured (%s)" % type(e).__name__)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
pairs.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
