"""Similar items at the config-3 shape (10 677 items x 10 677 items, rank 32, 95 samples, k = 10, cosine), DESIGN 4.13.4:
  (a) predict_similar's device path: a similarity handle over the items on both sides with the diagonal excluded, then
      mfm_pairs_topk_sim_store -- the whole call, handle included;
  (b) the yardstick, predict_topk_ucb's path for 10 677 user queries against the same items on the same store (the same
      contraction with the additive finish), the whole call likewise;
  (c) the host alternative: the samples' V on the host, per-sample normalisation, matmul, moments, np.argpartition -- timed on
      --host-queries query items and scaled to all of them;
then the kernel split of (a) and (b), each from a child process under `rocprofv3 --kernel-trace --stats`.
--check-topk: predict_topk's and predict_topk_ucb's paths at README's shape (4096 queries x 10 677 items) and nothing else; with
--tree DIR the library of another checkout is timed and named by --label, so that two commits can be run in turns.
The samples are random draws pushed into a device store; the model's quality plays no role in the timing. Every timing: one
warm-up, `reps` repetitions, median and min .. max. Writes the report to stdout and, with --out FILE, to that file."""
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
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-queries", type=int, default=256)
ap.add_argument("--check-topk", action="store_true")
ap.add_argument("--queries", type=int, default=4096, help="--check-topk: the number of user queries")
ap.add_argument("--label", default="this commit", help="--check-topk: what the report calls the timed library")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose myfm_amd is timed")
ap.add_argument("--variant", choices=["sim", "ucb"], default=None, help=argparse.SUPPRESS)  # (the traced child runs one call once)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from myfm_amd import _capi  # noqa: E402

NU, NI, K, S, k = args.users, args.items, args.rank, args.samples, args.k
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


def fmt(med, lo, hi, reps):
    return "median %.2f ms (min %.2f, max %.2f, %d reps)" % (1e3 * med, 1e3 * lo, 1e3 * hi, reps)


rng = np.random.default_rng(0)
store = _capi.Store(D, K)
Vs = []
for _ in range(S):
    V = rng.normal(size=(D, K)) * 0.2
    store.push(float(rng.normal()), rng.normal(size=D) * 0.3, V)
    Vs.append(V[NU:])  # (the items' rows: what the host alternative pulls)
Xi = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))


def onehot_users(n):
    users = np.sort(np.random.default_rng(1).choice(NU, size=n, replace=False))
    return sps.csr_matrix((np.ones(n), (np.arange(n), users)), shape=(n, D))


if args.check_topk:
    pairs = _capi.Pairs(onehot_users(args.queries), Xi)
    say("predict_topk / predict_topk_ucb at README's shape, %d queries x %d items, rank %d, %d samples, k = %d (%s)"
        % (args.queries, NI, K, S, k, args.label))
    for name, call in (("predict_topk     (mode 0)", lambda: pairs.topk_store(store, k, mode=0)),
                       ("predict_topk_ucb (mode 0)", lambda: pairs.topk_ucb_store(store, k, 1.0, mode=0)),
                       ("predict_topk     (mode 1)", lambda: pairs.topk_store(store, k, mode=1)),
                       ("predict_topk_ucb (mode 1)", lambda: pairs.topk_ucb_store(store, k, 1.0, mode=1))):
        _, med, lo, hi = timed(call, args.reps)
        say("  %s: %s" % (name, fmt(med, lo, hi, args.reps)))
    pairs.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

diag = sps.identity(NI, format="csr")
Xu = onehot_users(NI)


def similar():
    P = _capi.Pairs(Xi, Xi, exclude=diag, similarity=True)
    r = P.topk_sim_store(store, k, "cosine", 0.0)
    P.close()
    return r


def ucb():
    P = _capi.Pairs(Xu, Xi)
    r = P.topk_ucb_store(store, k, 1.0, mode=0)
    P.close()
    return r


if args.variant:  # the traced child: one call, nothing reported
    (similar if args.variant == "sim" else ucb)()
    sys.exit(0)


def host(q):
    """the q first items against all items on the host: per sample normalise, matmul, Welford's moments; then argpartition"""
    mean, m2 = np.zeros((q, NI)), np.zeros((q, NI))
    for s, V in enumerate(Vs):
        n = np.sqrt((V * V).sum(axis=1))
        E = V * np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)[:, None]
        c = E[:q] @ E.T
        d = c - mean
        mean += d / (s + 1)
        m2 += d * (c - mean)
    std = np.sqrt(m2 / S)
    mean[np.arange(q), np.arange(q)] = -np.inf
    part = np.argpartition(-mean, k - 1, axis=1)[:, :k]
    order = np.argsort(-np.take_along_axis(mean, part, 1), axis=1, kind="stable")
    top = np.take_along_axis(part, order, 1)
    return top, np.take_along_axis(mean, top, 1), np.take_along_axis(std, top, 1)


def kernel_split(variant):
    """{kernel name: total ms} of one child run under rocprofv3 --kernel-trace --stats, or a string saying why there is none"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="similar_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--variant", variant, "--users", str(NU), "--items", str(NI), "--rank", str(K), "--samples", str(S), "--k", str(k)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=300)
        parts = {}
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    short = row["Name"].split("(")[0].split("<")[0].split("::")[-1]
                    parts[short] = parts.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6
        return parts or "the trace held no kernel statistics"
    except subprocess.CalledProcessError as e:  # (the child's own last words say what went wrong)
        return "the traced child ended with status %d: %s" % (e.returncode, " | ".join((e.stderr or "").strip().splitlines()[-3:]))
    except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
        return "%s: %s" % (type(e).__name__, e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


say("similar items at the config-3 shape: %d items x %d items, rank %d, %d samples, k = %d, cosine, beta = 0" % (NI, NI, K, S, k))
flop = 2.0 * NI * NI * S * K
(idx, val, mean, std), med_a, lo, hi = timed(similar, args.reps)
say("(a) predict_similar's path (similarity handle, diagonal excluded, mfm_pairs_topk_sim_store): %s -- %.1f TFLOP/s fp64 over the "
    "whole call" % (fmt(med_a, lo, hi, args.reps), flop / med_a / 1e12))
say("    no item lists itself: %s; mean in [%.3f, %.3f], std in [%.3g, %.3g], max |value - mean| = %.2e"
    % (not np.any(idx == np.arange(NI)[:, None]), mean.min(), mean.max(), std.min(), std.max(), np.abs(val - mean).max()))
_, med_b, lo, hi = timed(ucb, args.reps)
say("(b) predict_topk_ucb's path, %d user queries x %d items, mode 0 (the yardstick):             %s" % (NI, NI, fmt(med_b, lo, hi, args.reps)))
say("    (a) takes %.2fx the time of (b)" % (med_a / med_b))
q = min(args.host_queries, NI)
(h_idx, h_mean, h_std), med_c, lo, hi = timed(lambda: host(q), max(1, args.reps // 2))
say("(c) host: V_samples, per-sample normalisation, matmul, moments, argpartition, %d of the %d query items: %s; scaled by %d / %d "
    "to all of them: %.1f s, %.0fx the time of (a). (Measured on the subset only; the samples are already on the host, the "
    "download of V_samples is not in it.)" % (q, NI, fmt(med_c, lo, hi, max(1, args.reps // 2)), NI, q, med_c * NI / q, med_c * NI / q / med_a))
say("    rows of the subset whose index lists agree with (a): %d of %d; max |mean difference| on those = %.2e"
    % (int(np.all(h_idx == idx[:q], axis=1).sum()), q,
       float(np.abs(h_mean - mean[:q])[np.all(h_idx == idx[:q], axis=1)].max()) if np.any(np.all(h_idx == idx[:q], axis=1)) else float("nan")))
for name, variant in (("(a)", "sim"), ("(b)", "ucb")):
    parts = kernel_split(variant)
    if isinstance(parts, str):
        say("    %s kernel split: not measured (%s)" % (name, parts))
        if parts != "rocprofv3 not found":
            say("    no further traced run is started after a failed one")
        break
    else:
        say("    %s kernel time %.3f ms: %s" % (name, sum(parts.values()), ", ".join("%s %.3f" % (n, v) for n, v in sorted(parts.items(), key=lambda t: -t[1]))))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
