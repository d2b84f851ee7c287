"""Designs that take the streamed block chain (csrc/mfm_chain_stream.hpp, k_cs_stream) down every path it has, shared by
tests/test_chain_edges_cpu.py (the plan and its emulation on the host) and tests/test_gpu_chain_stream_edges.py (the kernel against the
oracle). The structure is deterministic (no RNG): which path a (step, range) or a column takes is a matter of counts, and the tests
assert those counts on the plan record. In every design all columns share a few dense rows, so that after level 0 every column is a
level of its own and the whole block is ONE chain run in index order.

With 64 lanes a wavefront, the kernel's paths and what takes a plan there (record fields of mfm_chain_stream_info):

  walker  no hot entry                              hot_rounds[0] > 0
  walker  NR = 1..8 rounds, last one predicated     hot_rounds[NR] > 0 (edges: 64, 65 and 512 hot entries)
  walker  from the staged lists, twice              hot_rounds[9] > 0             (> 512 hot entries of a column)
  Y       entering rows beyond the first batch      max_enter > 384
  Y       hot lists beyond the registers            max_hot_col > 512
  X       exits slot by slot                        max_exit > 512
  S       tiles beyond the first tiles              max_cold_sr > 384
  S       entering rows beyond the first            max_enter_sr > 128
  U       upd() tail loop                           max_cold_sr > 384
  U       leaving rows beyond the first             max_exit_sr > 128
"""
import ctypes

import numpy as np
import scipy.sparse as sps

RD = 2  # the launch's slot reuse delay (CsParams, csrc/mfm_chain_plan.hpp)
LDS_MAX = 156 * 1024  # CS_LDS_MAX

# path -> (record field, threshold): reached when field > threshold
PATHS = {
    "Y enter beyond the first batch": ("max_enter", 384),
    "Y hot lists beyond the registers": ("max_hot_col", 512),
    "X exits slot by slot": ("max_exit", 512),
    "S tiles beyond the first / U upd tail": ("max_cold_sr", 384),
    "S entering rows beyond the first": ("max_enter_sr", 128),
    "U leaving rows beyond the first": ("max_exit_sr", 128),
}

EDGES_GROUPS = (60, 61, 150, 220, 280, 340, 400, 508, 509, 560)
EDGES_CONFIGS = [(4, 2, 2), (4, 3, 1), (4, 3, 32), (2, 4, 2), (3, 3, 2), (1, 7, 2)]  # (Cg, Lw, NB)
EDGES_REFUSED = (4, 7, 2)  # needs 169012 bytes of LDS
SHORT_NS = (2, 3, 4, 5, 9)
SHORT_CONFIGS = [(4, 2, 2), (1, 2, 32), (2, 3, 5)]


def _values(rows, cols, lo, hi, digits):
    # a fixed value per (row, column) in [lo, hi): the fractional part of an irrational combination
    f = np.mod(rows * 0.6180339887498949 + cols * 0.3819660112501051 + 0.123, 1.0)
    return np.round(lo + (hi - lo) * f, digits)


def _block(row_cols, n_cols, small):
    rows = np.concatenate([np.full(len(c), r, dtype=np.int64) for r, c in enumerate(row_cols)])
    cols = np.concatenate([np.asarray(c, dtype=np.int64) for c in row_cols])
    # the kernel tests: 0.2-1.0 as the other chain tests; the host emulation: 0.01-0.024 (cs_emulate's toy map expands round-off on
    # heavy columns with larger values, csrc/mfm_chain_plan.hpp)
    vals = _values(rows, cols, 0.01, 0.024, 6) if small else _values(rows, cols, 0.2, 1.0, 3)
    B = sps.csr_matrix((vals, (rows, cols)), shape=(len(row_cols), n_cols))
    B.sort_indices()
    return B


def edges(small=False):
    """4142 rows x 44 columns; row order fixes the ranges"""
    rc = [[4, 43] for _ in range(500)]                                   # cold at both ends
    rc += [[0] + list(range(4, 44)) for _ in range(4)]                   # the spine: hot from column 0 to the end
    for j in (1, 2, 3):
        rc += [[j] for _ in range(50)]                                   # private rows: level 0, all cold, no hot entry
    for g, size in enumerate(EDGES_GROUPS):
        rc += [[6 + 3 * g, 7 + 3 * g] for _ in range(size)]              # with the spine: 64, 65, .., 512, 513, 564 hot entries
    rc += [[4 + i % 20, 24 + i % 20] for i in range(400)]
    B = _block(rc, 44, small)
    assert B.shape == (4142, 44)
    return B


EDGES_HOT = [s + 4 for s in EDGES_GROUPS]  # hot entries of columns 6 + 3 g and 7 + 3 g at (4, 2, 2)


def short(n, small=False):
    """2100 rows x n columns: one step, fewer steps than the window, steps <= RD, an odd column count, a partial last step"""
    rc = [list(range(n)) for _ in range(3)]
    rc += [sorted({i % n, (i + 1) % n}) if i % 3 == 0 else [i % n] for i in range(3, 2100)]
    return _block(rc, n, small)


TINY_ROWS = (40, 24)


def tiny(n_rows=40, small=False):
    """n_rows x 5 columns, short()'s pattern: at NB = 32 a range owns one or two rows (40 rows) or some ranges own none (24 rows)"""
    rc = [list(range(5)) for _ in range(3)]
    rc += [sorted({i % 5, (i + 1) % 5}) if i % 3 == 0 else [i % 5] for i in range(3, n_rows)]
    return _block(rc, 5, small)


def with_main_table(B, seed=1, per_row=3, n_min=0):
    """(main, y, blocks, group_index): 20 one-hot main columns, per_row observations per block row, every block row mapped"""
    rng = np.random.default_rng(seed)
    n = max(per_row * B.shape[0], n_min)
    m = (np.arange(n) % B.shape[0]).astype(np.int64)
    main = sps.csr_matrix((np.ones(n), (np.arange(n), rng.integers(0, 20, size=n))), shape=(n, 20))
    gi = np.concatenate([[0] * 20, [1] * B.shape[1]]).astype(np.int32)
    y = rng.normal(size=n) + 0.3 * (m % 7) - 0.2 * (m % 5)
    return main, y, [(m, B)], gi


def probe(B, cg, lw, nb, rd=RD):
    """mfm_cs_plan_probe on the block: (record dict, hot entries per column, built, emulation difference)"""
    from myfm_amd import _capi

    L = _capi.lib()
    csc = sps.csc_matrix(B)
    csc.sort_indices()
    ptr = np.ascontiguousarray(csc.indptr, dtype=np.int64)
    idx = np.ascontiguousarray(csc.indices, dtype=np.int32)
    val = np.ascontiguousarray(csc.data, dtype=np.float64)
    rec = np.zeros(_capi.CHAIN_STREAM_INFO_FIELDS, dtype=np.int64)
    hot = np.zeros(B.shape[1], dtype=np.int32)
    built, diff = ctypes.c_int32(-1), ctypes.c_double(-1.0)
    rc = L.mfm_cs_plan_probe(B.shape[0], B.shape[1], ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, cg, lw, nb, rd, rec.ctypes.data,
                             hot.ctypes.data, ctypes.byref(built), ctypes.byref(diff))
    assert rc == 0, rc
    return _capi.chain_stream_record(rec), hot, bool(built.value), diff.value


PLAN_FIELDS = ("n_cols", "n_steps", "Cg", "Lw", "NB", "RD", "n_slots", "max_hot_col", "max_enter", "max_exit", "max_cold_sr", "max_enter_sr",
               "max_exit_sr", "n_cols_no_hot", "hot_rounds", "lds_bytes", "n_cold", "n_hot")  # a record without block and launches
