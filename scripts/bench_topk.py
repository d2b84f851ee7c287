"""Ranking at the config-3 shape (69 878 users x 10 677 items, rank 32, 95 samples, k = 10), DESIGN 4.13:
  (a) what the library offered before predict_topk: materialise the U x I pair rows, predict(), np.argpartition per row;
  (b) predict_topk's device path (mfm_pairs_topk_store) on the same samples;
for U = 4096 queries, then (b) alone for all users. The samples are random draws pushed into a device store (what a fit keeps);
the model's quality plays no role in the timing. Every timing: one warm-up, `reps` repetitions, median and min .. max.
Writes the report to stdout and, with --out FILE, to that file.

--rel-blocks: both sides carry multi-hot relation blocks (config 5's block shapes, scaled by --rel-scale: the query side a
user-side block of 10 entries per row and a context block of 5, the candidate side an item-side block of 10), and the script
times (a) the sides expanded on the host into flat matrices, run through the path without blocks, against (b) the block
arguments of mfm_pairs_add_block. The embedding kernels' share of the call is taken from a kernel trace: each variant is run once
more in a child process under `rocprofv3 --kernel-trace --stats` (skipped, and said so, where rocprofv3 is not installed).

--ucb: the cost of keeping the spread. At the same shape and on the same store, in one process: predict_topk's
path (mfm_pairs_topk_store, the mean) against predict_topk_ucb's (mfm_pairs_topk_ucb_store, mean + beta * std with --beta), for
the regressor's value (mode 0) and the classifier's (mode 1); then the kernel split of each of the four calls from a child process
under `rocprofv3 --kernel-trace --stats`."""
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

FP64_MFMA_PEAK = 78.6e12  # MI355X data sheet: FP64 matrix, dense

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=69878)
ap.add_argument("--items", type=int, default=10677)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--samples", type=int, default=95)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reps-materialised", type=int, default=3)
ap.add_argument("--skip-materialised", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--rel-blocks", action="store_true", help="relation-block sides: expanded flat matrices against block arguments")
ap.add_argument("--rel-scale", type=float, default=0.02, help="scale of config 5's block shapes (1.0: 500 000 users, 50 000 items)")
ap.add_argument("--rel-variant", choices=["flat", "blocks"], default=None, help=argparse.SUPPRESS)  # (the traced child runs one variant once)
ap.add_argument("--ucb", action="store_true", help="predict_topk_ucb's path against predict_topk's on the same store")
ap.add_argument("--beta", type=float, default=1.0)
ap.add_argument("--ucb-variant", choices=["mean0", "ucb0", "mean1", "ucb1"], default=None, help=argparse.SUPPRESS)  # (the traced child)
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


def write_out():
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def rel_blocks():
    """config 5's blocks, scaled: feature space [user one-hot | item one-hot | user-side block | context block | item-side block]"""
    rng = np.random.default_rng(0)
    nu, ni = max(1000, int(500_000 * args.rel_scale)), max(200, int(50_000 * args.rel_scale))
    U = args.queries

    def block(n_rows, n_cols, per_row):
        cols = np.sort(rng.integers(0, n_cols, size=(n_rows, per_row)), axis=1)
        keep = np.ones_like(cols, dtype=bool)
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
        rows = np.repeat(np.arange(n_rows), per_row).reshape(n_rows, per_row)
        return sps.csr_matrix((np.full(keep.sum(), 1.0 / np.sqrt(per_row)), (rows[keep], cols[keep])), shape=(n_rows, n_cols))

    ub, cb, ib = block(nu, 2000, 10), block(1000, 200, 5), block(ni, 1000, 10)
    D0 = nu + ni
    offs = [D0, D0 + 2000, D0 + 2200]
    Dr = D0 + 3200
    users = rng.integers(0, nu, size=U)  # (a user may be asked for more than once, in several contexts)
    ctx = rng.integers(0, 1000, size=U)
    Xq = sps.csr_matrix((np.ones(U), (np.arange(U), users)), shape=(U, Dr))
    Xc = sps.csr_matrix((np.ones(ni), (np.arange(ni), nu + np.arange(ni))), shape=(ni, Dr))
    rel_q = [(offs[0], users, ub), (offs[1], ctx, cb)]
    rel_c = [(offs[2], np.arange(ni), ib)]

    def widen(B, off):
        B = sps.coo_matrix(B)
        return sps.csr_matrix((B.data, (B.row, B.col + off)), shape=(B.shape[0], Dr))

    store = _capi.Store(Dr, K)
    for _ in range(S):
        store.push(float(rng.normal()), rng.normal(size=Dr) * 0.3, rng.normal(size=(Dr, K)) * 0.2)

    def flat():
        Fq = Xq + widen(ub[users], offs[0]) + widen(cb[ctx], offs[1])
        Fc = Xc + widen(ib, offs[2])
        P = _capi.Pairs(Fq, Fc)
        r = P.topk_store(store, k)
        P.close()
        return r

    def blocks():
        P = _capi.Pairs(Xq, Xc, rel_query=rel_q, rel_cand=rel_c)
        r = P.topk_store(store, k)
        P.close()
        return r

    if args.rel_variant:  # the traced child: one call, nothing reported
        (flat if args.rel_variant == "flat" else blocks)()
        return
    say("ranking with relation-block sides (config 5's blocks at scale %g): %d queries of %d users x %d items, rank %d, %d samples, "
        "k = %d; side rows hold 1 + 10 + 5 (query) and 1 + 10 (candidate) entries" % (args.rel_scale, U, nu, ni, K, S, k))
    (idx_a, val_a), med_a, lo_a, hi_a = timed(flat, args.reps)
    (idx_b, val_b), med_b, lo_b, hi_b = timed(blocks, args.reps)
    say("(a) sides expanded on the host, path without blocks (expansion, upload and call): median %.4f s (min %.4f, max %.4f, %d reps)"
        % (med_a, lo_a, hi_a, args.reps))
    say("(b) block arguments (upload and call):                                            median %.4f s (min %.4f, max %.4f, %d reps)"
        % (med_b, lo_b, hi_b, args.reps))
    say("    max |top-k value difference| = %.2e, rows whose index lists agree: %d of %d"
        % (np.abs(val_a - val_b).max(), int(np.all(idx_a == idx_b, axis=1).sum()), U))
    scale = 1.0 + 2 * 0.3 * 6 * 4 + K * (2 * 0.2 * 6 * 4) ** 2
    if not np.all(np.abs(val_a - val_b) <= 1e-10 * scale):
        raise SystemExit("the block path's values differ from the expanded path's")
    prof = shutil.which("rocprofv3")
    if not prof:
        say("    embedding kernels' share of the call: not measured (rocprofv3 not found)")
        return
    for name, variant in (("(a)", "flat"), ("(b)", "blocks")):
        tmp = tempfile.mkdtemp(prefix="topk_rel_")
        try:
            cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--", sys.executable,
                   os.path.abspath(__file__), "--rel-blocks", "--rel-variant", variant, "--rel-scale", str(args.rel_scale), "--rank", str(K),
                   "--samples", str(S), "--queries", str(args.queries), "--k", str(k)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            tot, emb, parts = 0.0, 0.0, {}
            for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                with open(fn) as f:
                    for row in csv.DictReader(f):
                        ns = float(row["TotalDurationNs"])
                        tot += ns
                        if "k_pairs_embed" in row["Name"]:
                            emb += ns
                            short = row["Name"].split("(")[0].split("::")[-1]
                            parts[short] = parts.get(short, 0.0) + ns
            if tot > 0:
                say("    %s kernel time %.3f ms, of it embedding %.3f ms = %.1f %% (%s)"
                    % (name, tot / 1e6, emb / 1e6, 100 * emb / tot, ", ".join("%s %.3f ms" % (n, v / 1e6) for n, v in sorted(parts.items()))))
            else:
                say("    %s embedding kernels' share: not measured (the trace held no kernel statistics)" % name)
        except (subprocess.CalledProcessError, OSError, KeyError, ValueError) as e:
            say("    %s embedding kernels' share: not measured (%s)" % (name, type(e).__name__))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


def kernel_split(child_args):
    """{kernel name: total ms} of one child run under rocprofv3 --kernel-trace --stats, or a string saying why there is none"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="topk_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__)] + child_args
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        parts = {}
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    short = row["Name"].split("(")[0].split("::")[-1].split("<")[0]
                    parts[short] = parts.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6
        return parts or "the trace held no kernel statistics"
    except (subprocess.CalledProcessError, OSError, KeyError, ValueError) as e:
        return type(e).__name__
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def ucb():
    rng = np.random.default_rng(0)
    store = _capi.Store(D, K)
    for _ in range(S):
        store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
    users = np.sort(rng.choice(NU, size=U, replace=False))
    Xq = sps.csr_matrix((np.ones(U), (np.arange(U), users)), shape=(U, D))
    Xc = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))
    pairs = _capi.Pairs(Xq, Xc)
    calls = {"mean0": lambda: pairs.topk_store(store, k, mode=0), "ucb0": lambda: pairs.topk_ucb_store(store, k, args.beta, mode=0),
             "mean1": lambda: pairs.topk_store(store, k, mode=1), "ucb1": lambda: pairs.topk_ucb_store(store, k, args.beta, mode=1)}
    if args.ucb_variant:  # the traced child: one call, nothing reported
        calls[args.ucb_variant]()
        return
    say("ranking by mean + beta * std at the config-3 shape: %d queries x %d items, rank %d, %d samples, k = %d, beta = %g"
        % (U, NI, K, S, k, args.beta))
    flop = 2.0 * U * NI * S * K
    med = {}
    for name, what in (("mean0", "predict_topk, regressor's value (mode 0)      "), ("ucb0", "predict_topk_ucb, regressor's value (mode 0)  "),
                       ("mean1", "predict_topk, classifier's value (mode 1)     "), ("ucb1", "predict_topk_ucb, classifier's value (mode 1) ")):
        r, med[name], lo, hi = timed(calls[name], args.reps)
        say("%s: median %.4f s (min %.4f, max %.4f, %d reps) -- %.1f TFLOP/s fp64 over the whole call"
            % (what, med[name], lo, hi, args.reps, flop / med[name] / 1e12))
        if name.startswith("ucb"):
            idx, val, mean, std = r
            say("    max |value - (mean + beta std)| = %.2e, std in [%.3g, %.3g]" % (np.abs(val - (mean + args.beta * std)).max(), std.min(), std.max()))
    say("keeping the spread costs %.2fx the mean path's time for the regressor's value and %.2fx for the classifier's; the regressor's "
        "moments call takes %.2fx the classifier's mean call" % (med["ucb0"] / med["mean0"], med["ucb1"] / med["mean1"], med["ucb0"] / med["mean1"]))
    for name in ("mean0", "ucb0", "mean1", "ucb1"):
        parts = kernel_split(["--ucb", "--ucb-variant", name, "--users", str(NU), "--items", str(NI), "--rank", str(K), "--samples", str(S),
                              "--queries", str(U), "--k", str(k), "--beta", str(args.beta)])
        if isinstance(parts, str):
            say("    %s kernel split: not measured (%s)" % (name, parts))
        else:
            say("    %s kernel time %.3f ms: %s" % (name, sum(parts.values()), ", ".join("%s %.3f" % (n, v) for n, v in sorted(parts.items(), key=lambda t: -t[1]))))
    pairs.close()


if args.rel_blocks:
    rel_blocks()
    write_out()
    sys.exit(0)
if args.ucb:
    ucb()
    write_out()
    sys.exit(0)

rng = np.random.default_rng(0)
store = _capi.Store(D, K)
for _ in range(S):
    store.push(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.2)
users = np.sort(rng.choice(NU, size=U, replace=False))
Xc = sps.csr_matrix((np.ones(NI), (np.arange(NI), NU + np.arange(NI))), shape=(NI, D))


def onehot_users(u):
    return sps.csr_matrix((np.ones(u.size), (np.arange(u.size), u)), shape=(u.size, D))


say("ranking at the config-3 shape: %d users x %d items, rank %d, %d samples, k = %d" % (NU, NI, K, S, k))
Xq = onehot_users(users)
pairs = _capi.Pairs(Xq, Xc)
(idx_b, val_b), med_b, lo_b, hi_b = timed(lambda: pairs.topk_store(store, k), args.reps)
flop = 2.0 * U * NI * S * K
say("(b) predict_topk, %d queries x %d items: median %.4f s (min %.4f, max %.4f, %d reps) -- %.1f TFLOP/s fp64 over the whole "
    "call (embedding, contraction + selection, merge, copy back), %.0f %% of the %.1f TFLOP/s MFMA peak"
    % (U, NI, med_b, lo_b, hi_b, args.reps, flop / med_b / 1e12, 100 * flop / med_b / FP64_MFMA_PEAK, FP64_MFMA_PEAK / 1e12))

if not args.skip_materialised:
    def materialised():
        n = U * NI
        indices = np.empty((n, 2), dtype=np.int32)
        indices[:, 0] = np.repeat(users, NI)
        indices[:, 1] = np.tile(NU + np.arange(NI, dtype=np.int32), U)
        X = sps.csr_matrix((np.ones(2 * n), indices.ravel(), np.arange(0, 2 * n + 1, 2, dtype=np.int64)), shape=(n, D))
        design = _capi.Design(X)
        score = store.predict(design).reshape(U, NI)
        design.close()
        part = np.argpartition(-score, k - 1, axis=1)[:, :k]
        order = np.argsort(-np.take_along_axis(score, part, 1), axis=1, kind="stable")
        top = np.take_along_axis(part, order, 1)
        return top, np.take_along_axis(score, top, 1)

    (idx_a, val_a), med_a, lo_a, hi_a = timed(materialised, args.reps_materialised)
    say("(a) materialise %.1e pair rows + predict() + argpartition: median %.3f s (min %.3f, max %.3f, %d reps)"
        % (U * NI, med_a, lo_a, hi_a, args.reps_materialised))
    say("    (b) is %.0fx faster than (a); max |top-k value difference| = %.2e, rows whose index lists agree: %d of %d"
        % (med_a / med_b, np.abs(val_a - val_b).max(), int(np.all(idx_a == idx_b, axis=1).sum()), U))
    # (a) is predict() itself: its k best values must be (b)'s. The scale of a score's rounding error is the sum of the absolute
    # terms, at most S-averaged |w0| + 2 max|w| + (2 max|V|)^2 K here; 1e-10 of it is the bound of tests/test_gpu_pairs.py
    scale = 1.0 + 2 * 0.3 * 6 + K * (2 * 0.2 * 6) ** 2
    if not np.all(np.abs(val_a - val_b) <= 1e-10 * scale):
        raise SystemExit("predict_topk's values differ from predict()'s on the materialised pairs")
pairs.close()

if NU > U:
    pairs = _capi.Pairs(onehot_users(np.arange(NU)), Xc)
    _, med, lo, hi = timed(lambda: pairs.topk_store(store, k), max(2, args.reps // 2))
    flop = 2.0 * NU * NI * S * K
    say("(b) predict_topk, all %d users x %d items: median %.3f s (min %.3f, max %.3f) -- %.1f TFLOP/s fp64 over the whole call, "
        "%.0f %% of the MFMA peak" % (NU, NI, med, lo, hi, flop / med / 1e12, 100 * flop / med / FP64_MFMA_PEAK))
    pairs.close()
write_out()
