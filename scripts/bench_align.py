"""Times the alignment behind aligned_factors() at config 3's shape (D = 80 555, rank 32, 95 kept samples, n_refine = 1) on samples
resident in a device store -- mfm_align_store, the entry point a freshly fitted model's aligned_factors() calls, with the handle's
creation and the copies of the results -- against the same rounds in NumPy on the host (BLAS matmul, LAPACK SVD), which first has
to copy the 95 x 20 MB of samples out of the store. Runs are interleaved; a run's figure is the median call.

    python scripts/bench_align.py [--runs 5] [--calls 5] [--D 80555] [--rank 32] [--samples 95] [--refine 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_rounds(Vs, n_refine):
    """the rounds of aligned_factors on (S, K, D) host samples, reference -1, no weights"""
    ref = Vs[-1]
    for _ in range(n_refine + 1):
        M = Vs @ ref.T
        U, sig, Wt = np.linalg.svd(M)
        R = U @ Wt
        Y = np.swapaxes(R, 1, 2) @ Vs
        mean, std = Y.mean(axis=0), Y.std(axis=0)
        align = sig.sum(axis=1) / np.sqrt((Vs ** 2).sum(axis=(1, 2)) * (ref ** 2).sum())
        ref = mean
    return mean.T, std.T, R, align


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--D", type=int, default=80555)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--samples", type=int, default=95)
    ap.add_argument("--refine", type=int, default=1)
    a = ap.parse_args()
    from myfm_amd import _capi

    rng = np.random.default_rng(0)
    V0 = rng.standard_normal((a.D, a.rank))
    store = _capi.Store(a.D, a.rank)
    for s in range(a.samples):
        Q, _ = np.linalg.qr(rng.standard_normal((a.rank, a.rank)))
        store.push(0.0, np.zeros(a.D), V0 @ Q + 0.1 * rng.standard_normal((a.D, a.rank)))
    _capi.align_store(store, -1, a.refine)  # (warm-up: the kernels' code objects, the LDS attributes)
    dev, host, copy = [], [], []
    for _ in range(a.runs):
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            got = _capi.align_store(store, -1, a.refine)
            t.append(time.perf_counter() - t0)
        dev.append(float(np.median(t)))
        t0 = time.perf_counter()
        Vs = np.stack([store.get(s)[2].T for s in range(a.samples)])
        t1 = time.perf_counter()
        ref = host_rounds(Vs, a.refine)
        host.append(time.perf_counter() - t0)
        copy.append(t1 - t0)
    err = max(float(np.abs(g - r).max()) for g, r in zip(got, ref))
    print(json.dumps(dict(D=a.D, rank=a.rank, samples=a.samples, n_refine=a.refine, device_ms=[round(1e3 * x, 2) for x in dev],
                          host_s=[round(x, 2) for x in host], host_copy_s=[round(x, 2) for x in copy],
                          device_ms_median=round(1e3 * float(np.median(dev)), 2), host_s_median=round(float(np.median(host)), 2),
                          max_abs_difference=err, min_alignment=float(got[3].min()))))


if __name__ == "__main__":
    main()
