"""Ranks of held-out pairs at the config-3 shape: 4096 queries x 10 677 items, rank 32, 95 samples, one target per
query, about 100 excluded candidates per query. On the same store and the same sides, in one process:
  (a) predict_topk's device path (mfm_pairs_topk_store, k = 10) with the same exclusions -- one contraction with the selection;
  (b) predict_rank's device path (mfm_pairs_rank_store) -- the values at the targets, then the contraction with the count;
and for 1024 of the queries
  (c) what the library offered before: predict_pairs' path (mfm_pairs_scores_store), the (U, I) matrix copied to the host and
      sorted there (np.argsort per row), the target's place looked up.
The samples are random draws pushed into a device store (what a fit keeps); the model's quality plays no role in the timing.
Every timing: one warm-up, `reps` repetitions, median and min .. max. The kernel split of (b) comes from a child process under
`rocprofv3 --kernel-trace --stats` (skipped, and said so, where rocprofv3 is not installed). Writes the report to stdout and,
with --out FILE, to that file."""
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
ap.add_argument("--queries-host", type=int, default=1024, help="queries of the host-sort comparison (c)")
ap.add_argument("--excluded", type=int, default=100, help="excluded candidates per query")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--mode", type=int, default=0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)  # (one rank call, nothing reported)
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


def kernel_split(child_args):
    """{kernel name: total ms} of one child run under rocprofv3 --kernel-trace --stats, or a string saying why there is none"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="rank_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__)] + child_args
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        parts = {}
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    short = row["Name"].split("(")[0].split("::")[-1]
                    parts[short] = parts.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6
        return parts or "the trace held no kernel statistics"
    except (subprocess.CalledProcessError, OSError, KeyError, ValueError) as e:
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
# per query one target and `excluded` other candidates
n_ex = min(args.excluded, NI - 1)
picks = np.stack([rng.choice(NI, size=n_ex + 1, replace=False) for _ in range(U)]).astype(np.int32)
targets = sps.csr_matrix((np.ones(U), (np.arange(U), picks[:, 0])), shape=(U, NI))
exclude = sps.csr_matrix((np.ones(U * n_ex), (np.repeat(np.arange(U), n_ex), picks[:, 1:].ravel())), shape=(U, NI))
pairs = _capi.Pairs(Xq, Xc, exclude=exclude, targets=targets)

if args.traced_child:
    pairs.rank_store(store, mode=args.mode)
    pairs.close()
    sys.exit(0)

say("ranks of held-out pairs at the config-3 shape: %d queries x %d items, rank %d, %d samples, mode %d, one target and %d excluded "
    "candidates per query" % (U, NI, K, S, args.mode, n_ex))
flop = 2.0 * U * NI * S * K
(_, _), med_a, lo_a, hi_a = timed(lambda: pairs.topk_store(store, k, mode=args.mode), args.reps)
say("(a) predict_topk's path, k = %d:  median %.4f s (min %.4f, max %.4f, %d reps) -- %.1f TFLOP/s fp64 over the whole call"
    % (k, med_a, lo_a, hi_a, args.reps, flop / med_a / 1e12))
(rank, value), med_b, lo_b, hi_b = timed(lambda: pairs.rank_store(store, mode=args.mode), args.reps)
say("(b) predict_rank's path:          median %.4f s (min %.4f, max %.4f, %d reps) -- %.2fx (a)"
    % (med_b, lo_b, hi_b, args.reps, med_b / med_a))
say("    ranks in [%d, %d], mean %.1f of %d candidates" % (rank.min(), rank.max(), rank.mean(), NI - n_ex))
parts = kernel_split(["--traced-child", "--users", str(NU), "--items", str(NI), "--rank", str(K), "--samples", str(S), "--queries", str(U),
                      "--excluded", str(args.excluded), "--mode", str(args.mode)])
if isinstance(parts, str):
    say("    (b) kernel split: not measured (%s)" % parts)
else:
    say("    (b) kernel time %.3f ms: %s" % (sum(parts.values()), ", ".join("%s %.3f" % (n, v) for n, v in sorted(parts.items(), key=lambda t: -t[1]))))
pairs.close()

Uh = min(args.queries_host, U)
if Uh > 0 and Uh * NI <= 1 << 24:
    sub = _capi.Pairs(Xq[:Uh], Xc, exclude=exclude[:Uh], targets=targets[:Uh])
    ex_h, t_h = exclude[:Uh], picks[:Uh, 0]

    def host_sort():
        score = sub.scores_store(store, mode=args.mode)
        score[np.repeat(np.arange(Uh), n_ex), ex_h.indices] = -np.inf  # (excluded candidates go last; none of them ties a target)
        order = np.argsort(-score, axis=1, kind="stable")  # value descending, index ascending
        return np.argmax(order == t_h[:, None], axis=1), score[np.arange(Uh), t_h]

    (rank_c, value_c), med_c, lo_c, hi_c = timed(host_sort, max(2, args.reps // 2))
    (rank_d, value_d), med_d, lo_d, hi_d = timed(lambda: sub.rank_store(store, mode=args.mode), args.reps)
    say("(c) %d queries: predict_pairs' path + host argsort: median %.4f s (min %.4f, max %.4f); predict_rank's path on the same "
        "queries: median %.4f s (min %.4f, max %.4f) -- %.1fx faster" % (Uh, med_c, lo_c, hi_c, med_d, lo_d, hi_d, med_c / med_d))
    same = int(np.count_nonzero(rank_c == rank_d))
    say("    ranks that agree with the host sort: %d of %d; values bit for bit equal: %s" % (same, Uh, bool(np.array_equal(value_c, value_d))))
    if same != Uh or not np.array_equal(value_c, value_d) or not np.array_equal(rank_d, rank[:Uh]):
        raise SystemExit("predict_rank's ranks or values differ from the host sort's")
    sub.close()
else:
    say("(c) predict_pairs' path + host argsort: not measured (%d x %d pairs exceed 2^24)" % (Uh, NI))

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
