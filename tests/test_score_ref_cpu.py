"""The reference of tests/test_gpu_score_shapes.py (tests/score_ref.py) proved on the CPU, on every design, rank and sample
set that file uses (tests/score_designs.py):

  * fm_score == the oracle's FM::predict_score == the dense closed form on the flat design, at 1e-12 relative to the rows'
    magnitude M;
  * a float64 evaluation in three orders (factors ascending, descending, and the kernel's lane tree) stays inside
    tol = gamma_n M on every row: the bound leaves room for a correct float64 kernel;
  * every factor and every stored entry moves at least one row by 100 tol: a dropped factor pair or entry cannot hide.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from . import score_designs as sd
from . import score_ref as sr

GROUPS = sorted(sd.GROUPS)


def _flat(X, blocks):
    return sps.hstack([sps.csr_matrix(X)] + [sps.csr_matrix(B)[np.asarray(mp)] for mp, B in blocks], format="csr")


def test_longdouble_is_finer_than_float64():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_the_shape_table_restated():
    assert [sr.score_shape(K) for K in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512)] == [
        (4, 1), (4, 1), (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 2), (64, 4), (64, 4)]
    with pytest.raises(ValueError):
        sr.score_shape(513)


def test_layouts_are_what_they_claim():
    a, b, c, d = (sd.layout(n) for n in sd.LAYOUTS)
    for X in (a, b, c, d):
        assert X.shape == (203, 67) and X.has_sorted_indices
        assert 0 in X.indices and 66 in X.indices
    assert np.all(np.diff(a.indptr) == 2) and np.all(a.data == 1.0)
    assert np.all(np.diff(d.indptr) == 5) and set(d.data) == set(sd.VALUES)
    for X in (b, c):
        lens = np.diff(X.indptr)
        assert lens[0] == 0 and lens[-1] == 0 and lens.min() == 0 and lens.max() == 9
        for g in range(0, 203, 4):
            assert len(set(lens[g:g + 4])) > 1  # maxlen against len[u] inside every group of SCORE_RU rows
    assert np.all(b.data == 1.0) and set(c.data) == set(sd.VALUES)
    assert np.array_equal(b.indices, c.indices)
    assert sd.layout("b", N=1).nnz == 3 and list(np.diff(sd.layout("b", N=3).indptr)) == [0, 3, 6]
    assert sd.empty_table().nnz == 0 and sd.empty_table().shape == (5, 67)
    (m0, B0), (m1, B1) = sd.two_blocks()
    assert B0.shape == (11, 9) and B1.shape == (6, 5) and 0 in np.diff(B0.indptr) and np.diff(B0.indptr).max() > 1
    assert set(m0) == set(range(11)) and set(m1) == set(range(6))
    assert len(sd.many_blocks()) == 17 and all(set(mp) == set(range(B.shape[0])) for mp, B in sd.many_blocks())
    for name, c in sd.CHUNK_CASES.items():
        X, three = sd.chunk_design(name)
        assert X.shape == (37, c.D) and 0 in X.indices and c.D - 1 in X.indices
        assert 1 < sd.chunk_size(c.D, c.K) < c.S
    assert sd.chunk_size(16387, 257) == 15 and sd.chunk_size(2097157, 7) == 3


@pytest.mark.parametrize("group", GROUPS)
def test_reference_agrees_with_the_oracle_and_the_dense_form(oracle, group):
    for case in sd.cases(group):
        od = oracle.OracleDesign(case.X, case.blocks)
        F = _flat(case.X, case.blocks)
        F2 = F.multiply(F).tocsr()
        rows = sr.flat_rows(case.X, case.blocks)
        for w0, w, V in case.samples:
            ref = sr.fm_score(case.X, case.blocks, w0, w, V, rows)
            M, _ = sr.fm_score_bound(case.X, case.blocks, w0, w, V, rows)
            dense = w0 + F @ w + 0.5 * (np.square(F @ V) - F2 @ np.square(V)).sum(axis=1)
            for other in (od.predict_score(w0, w, V), np.asarray(dense).ravel()):
                assert np.all(np.abs(other - ref) <= 1e-12 * M), case.name
            if F.nnz == 0:
                assert np.all(ref == w0)


@pytest.mark.parametrize("group", GROUPS)
def test_float64_in_any_order_stays_inside_the_bound(group):
    worst = 0.0
    for case in sd.cases(group):
        rows = sr.flat_rows(case.X, case.blocks)
        for w0, w, V in case.samples:
            ref = sr.fm_score(case.X, case.blocks, w0, w, V, rows)
            _, tol = sr.fm_score_bound(case.X, case.blocks, w0, w, V, rows)
            for order in ("ascending", "descending", "tree"):
                err = np.abs(sr.fm_score_f64(case.X, case.blocks, w0, w, V, order, rows) - ref)
                assert np.all(err <= tol), (case.name, order, float((err / tol).max()))
                worst = max(worst, float((err / tol).max()))
    print("largest float64 error / tol in group %s: %.3f" % (group, worst))


@pytest.mark.parametrize("group", GROUPS)
def test_every_factor_and_entry_is_visible(group):
    for case in sd.cases(group):
        idx, x, cnt = sr.flat_rows(case.X, case.blocks)
        if cnt.sum() == 0:
            continue
        S = len(case.samples)
        tol = sum(sr.fm_score_bound(case.X, case.blocks, *s, (idx, x, cnt))[1] for s in case.samples) / S
        # a factor zeroed: its column of the pair terms leaves the score
        pair = sum(sr.fm_score_terms(case.X, case.blocks, *s, (idx, x, cnt))[1] for s in case.samples) / S
        assert np.all((np.abs(pair) >= 100 * tol[:, None]).any(axis=0)), case.name
        # a stored entry zeroed (slot l of every flat row that has one, all rows at once): its products leave the row's sums.
        # (Taken out of the longdouble sums instead of summing the row again without it: the same to 2^-63 of M, against a
        #  threshold of at least 1600 * 2^-53 of M, at 1 / L of the cost.)
        moved = np.zeros(x.shape, dtype=sr.LD)
        for w0, w, V in case.samples:
            xl, wl, Vl = x.astype(sr.LD), np.asarray(w)[idx].astype(sr.LD), np.asarray(V)[idx].astype(sr.LD)
            xv = xl[:, :, None] * Vl
            s, q = xv.sum(axis=1), (xv * xv).sum(axis=1)
            full = (s * s - q).sum(axis=1) / 2
            for l in range(x.shape[1]):
                sl, ql = s - xv[:, l], q - xv[:, l] * xv[:, l]
                moved[:, l] += xl[:, l] * wl[:, l] + full - (sl * sl - ql).sum(axis=1) / 2
        has = np.arange(x.shape[1])[None, :] < cnt[:, None]
        assert np.all((np.abs(moved / S) >= 100 * tol[:, None])[has]), case.name
