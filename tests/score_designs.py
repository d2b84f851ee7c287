"""The seeded designs, samples and cases of tests/test_gpu_score_shapes.py, built here so that tests/test_score_ref_cpu.py
proves the reference and its tolerance on exactly what the device is held to.

Four layouts of the main table over the same D0 = 67 columns (not a multiple of the transposes' 32-wide tile; column 0 and
column D0 - 1 are used by every layout), N = 203 rows (50 groups of SCORE_RU = 4 rows and 3 more):

  a  unit ELL          two one-hot fields                               -> <UNIT, ELL>
  b  unit ragged CSR   row lengths 0 .. 9, different inside every group of four rows, row 0 and the last row empty
  c  valued ragged CSR the pattern of b, values from {0.5, -1, 1.5, 2}
  d  valued fixed-width
"""
import collections

import numpy as np
import scipy.sparse as sps

D0 = 67
N_ROWS = 203
VALUES = np.array([0.5, -1.0, 1.5, 2.0])
LAYOUTS = ("a", "b", "c", "d")

# the boundaries of score_shape (8|9, 16|17, 32|33, 64|65, 128|129, 256|257, 512), odd ranks in every shape, the smallest ranks
RANKS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
# ... and those of launch_block_score_cache as well (4|5, 8|9, ..., 256|257)
BLOCK_RANKS = (3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512)
MANY_BLOCK_RANKS = (65, 129)  # 17 blocks: one more than travels in the kernel arguments
REUSE_RANKS = (9, 8, 7, 129, 2, 64)  # one Design, in this order
TRAIN_RANKS = (7, 8, 9, 17, 33, 65, 129)
CLASS_RANKS = (4, 65)
CLASS_COUNTS = (2, 3, 5, 31, 32, 33)
TILE_RANKS = (9, 33, 130)
TINY_RANKS = (7, 65)

Case = collections.namedtuple("Case", "name X blocks K samples")


def _csr(lens, cols, vals, D):
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return sps.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(cols, dtype=np.int32), indptr), shape=(len(lens), D))


def ragged_lengths(N):
    """0 .. 9, four different lengths in every group of four rows (steps of 3 modulo 10); row 0 is empty, and so is the last row of
    a table of more than three rows. A one-row table keeps its three entries."""
    lens = (3 * np.arange(N)) % 10
    if N == 1:
        lens[0] = 3
    elif N > 3:
        lens[-1] = 0
    return lens


def ragged(N, D, seed, valued):
    """Ragged rows over D columns; the first row of three entries holds column 0 and column D - 1."""
    rng = np.random.default_rng([seed, N, D])
    lens = ragged_lengths(N)
    cols = [np.sort(rng.choice(D, size=n, replace=False)) for n in lens]
    first3 = int(np.flatnonzero(lens == 3)[0])
    cols[first3] = np.array([0, int(cols[first3][1]) if 0 < cols[first3][1] < D - 1 else D // 2, D - 1])
    assert all(len(c) == n for c, n in zip(cols, lens))
    nnz = int(lens.sum())
    vals = VALUES[rng.integers(0, 4, size=nnz)] if valued else np.ones(nnz)
    return _csr(lens, np.concatenate(cols) if nnz else [], vals, D)


def layout(name, N=N_ROWS, seed=1):
    if name == "a":
        rng = np.random.default_rng([seed, 10])
        u, i = rng.integers(0, 33, size=N), rng.integers(33, D0, size=N)
        u[0], i[0] = 0, D0 - 1
        return _csr(np.full(N, 2), np.stack([u, i], axis=1).ravel(), np.ones(2 * N), D0)
    if name == "b":
        return ragged(N, D0, seed, valued=False)
    if name == "c":
        return ragged(N, D0, seed, valued=True)
    if name == "d":
        rng = np.random.default_rng([seed, 13])
        cols = np.stack([np.sort(rng.choice(D0, size=5, replace=False)) for _ in range(N)])
        cols[0, 0], cols[0, -1] = 0, D0 - 1
        return _csr(np.full(N, 5), cols.ravel(), VALUES[rng.integers(0, 4, size=5 * N)], D0)
    raise ValueError(name)


def empty_table(N=5):
    return sps.csr_matrix((N, D0), dtype=np.float64)


def _map_hitting_every_row(rng, N, B):
    return rng.permutation(np.arange(N) % B).astype(np.int64)


def two_blocks(N=N_ROWS, seed=2):
    """Block 0: 11 rows x 9 columns, multi-hot and valued, block row 4 empty. Block 1: 6 rows x 5 columns, valued. The maps hit
    every block row."""
    rng = np.random.default_rng([seed, N])
    lens0 = np.array([2, 3, 1, 4, 0, 2, 5, 3, 1, 2, 9])
    cols0 = np.concatenate([np.sort(rng.choice(9, size=n, replace=False)) for n in lens0])
    B0 = _csr(lens0, cols0, VALUES[rng.integers(0, 4, size=int(lens0.sum()))], 9)
    lens1 = np.array([1, 2, 3, 1, 5, 2])
    cols1 = np.concatenate([np.sort(rng.choice(5, size=n, replace=False)) for n in lens1])
    B1 = _csr(lens1, cols1, VALUES[rng.integers(0, 4, size=int(lens1.sum()))], 5)
    n0, n1 = min(N, 11), min(N, 6)  # (a table shorter than a block cannot hit all of its rows)
    m0 = _map_hitting_every_row(rng, N, 11) if n0 == 11 else rng.integers(0, 11, size=N).astype(np.int64)
    m1 = _map_hitting_every_row(rng, N, 6) if n1 == 6 else rng.integers(0, 6, size=N).astype(np.int64)
    return [(m0, B0), (m1, B1)]


def many_blocks(N=N_ROWS, seed=3):
    """17 blocks: the two above and 15 of (3 + b) rows x 2 columns"""
    rng = np.random.default_rng([seed, N])
    blocks = two_blocks(N, seed)
    for b in range(15):
        rows = 3 + b
        B = _csr(np.full(rows, 2), np.tile([0, 1], rows), VALUES[rng.integers(0, 4, size=2 * rows)], 2)
        blocks.append((_map_hitting_every_row(rng, N, rows), B))
    return blocks


def dim_all(X, blocks=()):
    return X.shape[1] + sum(B.shape[1] for _, B in blocks)


def samples(D, K, S, seed):
    """S samples (w0, w[D], V[D, K]): w0 ~ N(0, 1), w and V ~ 0.3 N(0, 1)"""
    rng = np.random.default_rng([seed, D, K, S])
    return [(float(rng.normal()), rng.normal(size=D) * 0.3, rng.normal(size=(D, K)) * 0.3) for _ in range(S)]


def cutpoints(S, n_cut, seed):
    """sorted normals, one set per sample"""
    rng = np.random.default_rng([seed, S, n_cut])
    return [np.sort(rng.normal(size=n_cut)) for _ in range(S)]


def train_design():
    """What decide_main_paths sends down the generic path: a multi-hot valued main table (layout c) and the two blocks"""
    X = layout("c", seed=4)
    y = np.random.default_rng(40).normal(size=X.shape[0])
    return X, y, two_blocks(seed=4)


def train_test_design():
    """another design over the same columns and block tables, for Design.score_ctx"""
    X = layout("c", N=57, seed=5)
    rng = np.random.default_rng(50)
    blocks = [(_map_hitting_every_row(rng, 57, B.shape[0]), B) for _, B in two_blocks(seed=4)]
    return X, blocks


# sample chunks: design_stage_samples (csrc/mfm_predict.hpp) gives the row-major V copies of a chunk of samples 512 MB
CHUNK_BYTES = 512 << 20
ChunkCase = collections.namedtuple("ChunkCase", "K D S n_class")
CHUNK_CASES = {
    "A": ChunkCase(K=257, D=16387, S=17, n_class=5),     # <64, 4>; 33.8 MB per sample: 15 + 2
    "B": ChunkCase(K=7, D=2097157, S=7, n_class=32),     # <4, 1>; 134.2 MB per sample: 3 + 3 + 1, a middle chunk
}
CHUNK_ROWS = 37


def chunk_size(D, K):
    """design_stage_samples' formula: floor(512 * 2^20 / (8 D KS)) samples, KS the rank rounded up to even"""
    KS = (K + 1) & ~1
    return max(1, CHUNK_BYTES // (8 * D * KS))


def chunk_design(name):
    """(X, the three distinct samples that are pushed cyclically)"""
    c = CHUNK_CASES[name]
    return ragged(CHUNK_ROWS, c.D, 6, valued=True), samples(c.D, c.K, 3, 60)


def chunk_samples(name):
    c = CHUNK_CASES[name]
    X, three = chunk_design(name)
    return X, [three[k % 3] for k in range(c.S)]


# ---- every (design, rank, samples) the device file scores, by group -----------------------------------------------------
def _rank_table():
    for K in RANKS:
        for lay in LAYOUTS:
            yield Case("rank%d-%s" % (K, lay), layout(lay), [], K, samples(D0, K, 5, 100))


def _tiny():
    for K in TINY_RANKS:
        for N in (1, 3):
            yield Case("tiny%d-b-N%d" % (K, N), layout("b", N=N), [], K, samples(D0, K, 5, 101))
        yield Case("tiny%d-empty" % K, empty_table(), [], K, samples(D0, K, 5, 102))


def _reuse():
    X, blocks = layout("c"), two_blocks()
    for K in REUSE_RANKS:
        yield Case("reuse%d" % K, X, blocks, K, samples(dim_all(X, blocks), K, 3, 103))


def _blocks():
    X, blocks = layout("c"), two_blocks()
    for K in BLOCK_RANKS:
        yield Case("blocks%d" % K, X, blocks, K, samples(dim_all(X, blocks), K, 3, 104))
    blocks = many_blocks()
    for K in MANY_BLOCK_RANKS:
        yield Case("blocks17-%d" % K, X, blocks, K, samples(dim_all(X, blocks), K, 3, 105))


def _train():
    X, _, blocks = train_design()
    Xt, tblocks = train_test_design()
    for K in TRAIN_RANKS:
        smp = samples(dim_all(X, blocks), K, 1, 106)
        yield Case("train%d" % K, X, blocks, K, smp)
        yield Case("train%d-test" % K, Xt, tblocks, K, smp)


def _classes():
    for K in CLASS_RANKS:
        yield Case("classes%d" % K, layout("b"), [], K, samples(D0, K, 4, 107))


def _chunks():
    for name, c in CHUNK_CASES.items():
        X, three = chunk_design(name)
        yield Case("chunk" + name, X, [], c.K, three)


def _tiles():
    for K in TILE_RANKS:
        for lay in ("a", "b"):
            yield Case("tiles%d-%s" % (K, lay), layout(lay), [], K, samples(D0, K, 5, 108))


def _refusal():
    X = layout("c")
    for blocks in ([], two_blocks()):
        yield Case("refusal-%d" % len(blocks), X, blocks, 4, samples(dim_all(X, blocks), 4, 2, 109))


GROUPS = {"rank_table": _rank_table, "tiny": _tiny, "reuse": _reuse, "blocks": _blocks, "train": _train, "classes": _classes,
          "chunks": _chunks, "tiles": _tiles, "refusal": _refusal}


def cases(group):
    return GROUPS[group]()
