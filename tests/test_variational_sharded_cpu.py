"""Row-sharded variational FM, the part that needs no GPU: the new C ABI symbols and bindings, the level schedule of the expanded
design (vb_column_levels), and the NumPy model of the sharded protocol (tests/vb_shard_ref.py) against the unsharded restatement
of the reference (tests/vb_ref.py): what is summed over the shards and what happens after the sum."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import myfm_amd
from myfm_amd import _capi, _myfm

from . import test_gpu_variational as tgv
from . import vb_ref, vb_shard_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfm_vb_set_stream", "mfm_vb_set_allreduce", "mfm_vb_set_shard", "mfm_vb_comm_init", "mfm_vb_comm_stats",
       "mfm_vb_set_levels", "mfm_vb_design_levels")


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "myfm_hip.h")).read()
    declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", header))
    L = _capi.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for s in NEW:
        assert s in _capi.SYMBOLS and s in declared and s in exported and hasattr(L, s), s
    assert hasattr(_myfm, "create_train_vfm_sharded") and hasattr(_myfm, "vb_column_levels")
    assert hasattr(_myfm.VariationalFM, "comm_stats")


def _onehot3():
    return tgv._onehot(500, [7, 11, 5], 4, values=True), []


def _design(name):
    if name == "onehot":
        return _onehot3()
    X, _, _, _, kw = tgv._test_block_design() if name == "test_block" else tgv._multihot_design()
    return X, kw["blocks"]


@pytest.mark.parametrize("name", ["onehot", "test_block", "multihot"])
def test_vb_column_levels_are_those_of_the_expanded_table(name):
    X, blocks = _design(name)
    rels = [myfm_amd.RelationBlock(mp, B) for mp, B in blocks]
    got = _myfm.vb_column_levels(X, rels)
    flat = sps.hstack([sps.csr_matrix(X)] + [sps.csr_matrix(B)[np.asarray(mp)] for mp, B in blocks]).tocsr()
    want, n = _capi.column_levels(flat)
    assert got.dtype == np.int32 and np.array_equal(got, want) and got.max() + 1 == n
    assert np.array_equal(vb_shard_ref.column_levels(flat), want)  # (the protocol model's own restatement)
    if name == "onehot":
        assert np.array_equal(got, np.r_[np.zeros(7), np.ones(11), np.full(5, 2)])
    if name == "multihot":  # four fields, but multi-hot block columns chain: far more levels than fields
        assert n > 4 * 4


def test_vb_column_levels_refuses_a_duplicate_entry():
    X = sps.csr_matrix((np.ones(3), np.array([0, 0, 1]), np.array([0, 2, 3])), shape=(2, 2))  # row 0 holds column 0 twice
    with pytest.raises(ValueError, match="same column twice"):
        _myfm.vb_column_levels(X, [])


def _close(got, want, rtol):
    # the scaling of tests/test_gpu_variational.py::_close
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    scale = np.max(np.abs(want[fin])) if fin.any() else 1.0
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=rtol * scale)


def _protocol_case(name):
    if name == "onehot":
        X, blocks = _onehot3()
        y = np.random.RandomState(8).randn(500) + 0.5
        return X, y, 3, np.r_[np.zeros(7), np.ones(11), np.full(5, 2)], blocks
    X, y, rank, gi, kw = tgv._test_block_design(300) if name == "test_block" else tgv._multihot_design(N=600, U=20, I=15)
    return X, y, rank, gi, kw["blocks"]


_REF = {}


def _reference(name, task):
    """the unsharded restatement after 10 iterations, computed once per (design, task) and left unchanged"""
    if (name, task) not in _REF:
        X, y, rank, gi, blocks = _protocol_case(name)
        if task == "classification":
            y = np.where(y > np.median(y), 1.0, -1.0)
        rs = np.random.RandomState(3)
        D = len(gi)
        w0, w, V = 0.05, rs.randn(D) * 0.1, rs.randn(D, rank) * 0.1
        ref = vb_ref.VBRef(X, y, rank, gi, task, vb_ref.Config(), w0, w, V, 0.1, blocks=blocks)
        for _ in range(10):
            ref.iterate()
        _REF[name, task] = (X, y, rank, gi, blocks, (w0, w, V), ref)
    return _REF[name, task]


@pytest.mark.parametrize("task", ["regression", "classification"])
@pytest.mark.parametrize("name", ["onehot", "test_block", "multihot"])
@pytest.mark.parametrize("cut", ["one", "two_uneven", "three_one_empty"])
def test_protocol_model_matches_unsharded_reference(name, task, cut):
    X, y, rank, gi, blocks, (w0, w, V), ref = _reference(name, task)
    N = X.shape[0]
    cuts = {"one": [0, N], "two_uneven": [0, (9 * N) // 10, N], "three_one_empty": [0, N // 3, N // 3, N]}[cut]
    sh = vb_shard_ref.ShardedVBRef(X, y, rank, gi, task, vb_ref.Config(), w0, w, V, 0.1, blocks=blocks, cuts=cuts)
    assert sh.collectives == 1  # initialize_e's score pass
    for _ in range(10):
        sh.iterate()
    # (K + 1) * (non-empty levels) + 1 sums over the shards per iteration
    assert sh.collectives == 1 + 10 * ((rank + 1) * len(sh.levels) + 1)
    for a in ("w0", "w0_var", "w", "w_var", "V", "V_var"):
        _close(getattr(sh, a), getattr(ref, a), 1e-9)
    _close(sh.e_all, ref.e, 1e-9)
    want = ref.hyper()
    for k, v in sh.hyper().items():
        _close(v, want[k], 1e-9)
    _close(sh.elbos, ref.elbos, 1e-9)
