"""Fold-in for the probit estimators, the parts that need no GPU: the chain of tests/fold_in_gibbs_ref.py in float64 against
longdouble within the tolerance the GPU test uses, the chain's mean against the posterior mean by quadrature, the keys of the random
streams, the argument checks of fold_in_gibbs (which run on the host before the device is looked for), the chunk plan and the
refusals of the native host code under a host sanitizer, and the exported symbols."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from tests import fold_in_gibbs_ref as gr
from tests import fold_in_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mfm_foldin_gibbs_solve_store", "mfm_foldin_gibbs_solve")
CHAINS = ((0, 1), (1, 1), (2, 3))


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("K", [0, 1, 3, 16, 33])
def test_float64_twin_stays_within_the_tolerance(K, fit_linear):
    """what the GPU test asks of the kernel is attainable in float64: the same chain with float64 linear algebra and identical
    draws stays inside 16 T (M + n_u) 2^-52 cond max(|theta|, |mu|) of the longdouble chain (largest ratio seen: 0.045), and no
    cell is left out by the margin rule. D = 40, U = 8, S = 2, rows per entity over ROW_CHOICES."""
    worst, left = 0.0, 0
    for n_class in (0, 3, 5):
        for n_burn, n_inner in CHAINS:
            rng = np.random.default_rng(1000 * K + 10 * n_class + fit_linear + 100 * n_burn + 7 * n_inner)
            p = gr.problem(rng, 40, K, 2, 8, n_class)
            assert 0 in p["counts"] and p["counts"].max() >= 64
            ref = gr.chain(p, fit_linear, n_burn, n_inner, 5)
            twin = gr.chain(p, fit_linear, n_burn, n_inner, 5, np.float64)
            if ref["last"].shape[-1] == 0:
                continue
            assert ref["cond"].max() <= 1e5
            keep = ref["margin"] >= 1e-9
            left += int((~keep).sum())
            empty = p["counts"] == 0
            for key in ("last", "mean"):
                tol = gr.tolerance(ref, ref[key], n_burn + n_inner)
                err = np.abs(twin[key] - ref[key]).max(axis=-1).astype(np.float64)
                assert np.all(err[keep] <= tol[keep]), (n_class, n_burn, n_inner, key, (err / tol)[keep].max())
                worst = max(worst, float((err / tol)[keep].max()))
            assert np.array_equal(twin["mean"][:, empty], np.broadcast_to(p["mu"][:, None, (0 if fit_linear else 1):], twin["mean"][:, empty].shape))
    assert left == 0
    print("fold-in chain, float64 against longdouble, K=%d fit_linear=%d: largest error / bound = %.4f" % (K, fit_linear, worst))


@pytest.mark.parametrize("n_class", [0, 3])
def test_chain_mean_matches_quadrature(n_class):
    """rank 0 with the linear term, one entity of 6 rows: the mean over 12 seeds of the Rao-Blackwellised mean (20 sweeps of burn-in,
    600 kept) lies within 4 of its own standard errors of the 1-D posterior mean on a grid"""
    p = gr.problem(np.random.default_rng(40 + n_class), 12, 0, 1, 1, n_class, counts=[6])
    want = gr.quadrature_mean(p)
    vals = np.array([float(gr.chain(p, True, 20, 600, seed, np.float64)["mean"][0, 0, 0]) for seed in range(12)])
    mean, se = vals.mean(), vals.std(ddof=1) / np.sqrt(12)
    print("n_class=%d: chain %.4f +- %.4f, quadrature %.4f" % (n_class, mean, se, want))
    assert abs(mean - want) <= 4 * se
    # the chain moved: the posterior mean is not the prior's
    assert abs(want - p["mu"][0, 0]) > 10 * se


def _placed(base, U, u, lead=0, rng=None):
    """the 6 rows of `base` as entity u of U, behind `lead` rows of entity 0 (u > 0) that shift their grouped position"""
    n = base["X"].shape[0]
    q = dict(base)
    X, y, ent = base["X"], base["y"], np.full(n, u, dtype=np.int64)
    if lead:
        X = sps.vstack([fr.context_rows(rng, lead, base["D"]), X]).tocsr()
        y = np.concatenate([base["y"][:1].repeat(lead), y])
        ent = np.concatenate([np.zeros(lead, dtype=np.int64), ent])
    q.update(U=U, X=X, y=y, entity=ent, counts=np.bincount(ent, minlength=U))
    return q


@pytest.mark.parametrize("n_class", [0, 4])
def test_streams_are_keyed_as_documented(n_class):
    """latent stream row = s n + i (i the grouped row, n the row count), eps stream row = s U + u. The same rows as entity 3 of 5 and
    as entity 1 of 7 (alone, so i and n agree): sample 1 reads eps row 8 in both and gives the same bits, sample 0 reads rows 3 and 1
    and differs. Behind 6 other rows (n = 12, i shifted by 6) as entity 1 of 2, sample 0 reads latent rows 6 .. 11 and eps row 1:
    what sample 1 of the problem alone (n = 6, U = 1) reads -- the same bits when both samples are the same model."""
    rng = np.random.default_rng(77 + n_class)
    base = gr.problem(rng, 20, 3, 2, 1, n_class, counts=[6])
    a, b = gr.chain(_placed(base, 5, 3), True, 1, 2, 9), gr.chain(_placed(base, 7, 1), True, 1, 2, 9)
    for key in ("last", "mean"):
        assert np.array_equal(a[key][1, 3], b[key][1, 1]) and not np.array_equal(a[key][0, 3], b[key][0, 1])
    same = dict(base)
    same.update(samples=[base["samples"][1]] * 2, mu=base["mu"][[1, 1]], lam=base["lam"][[1, 1]],
                cut=None if n_class == 0 else base["cut"][[1, 1]])
    alone = gr.chain(same, True, 1, 2, 9)
    moved = gr.chain(_placed(same, 2, 1, lead=6, rng=rng), True, 1, 2, 9)
    for key in ("last", "mean"):
        assert np.array_equal(moved[key][0, 1], alone[key][1, 0]) and not np.array_equal(moved[key][1, 1], alone[key][1, 0])
        assert not np.array_equal(alone[key][0, 0], alone[key][1, 0])
    assert not np.array_equal(gr.chain(base, True, 1, 2, 10)["mean"], gr.chain(base, True, 1, 2, 9)["mean"])


def test_normals_and_tags():
    # component j of eps does not depend on M; the word moves the draw; the regressor's own word is fold_in_ref's
    w = gr.FOLDIN_DRAW_TAG + 1
    assert np.array_equal(gr.normals(11, w, 3, 4, 6)[..., :5], gr.normals(11, w, 3, 4, 5))
    assert not np.array_equal(gr.normals(11, w + 1, 3, 4, 5), gr.normals(11, w, 3, 4, 5))
    assert np.array_equal(gr.normals(11, gr.FOLDIN_DRAW_TAG, 3, 4, 5), fr.normals(11, 3, 4, 5))
    assert gr.FOLDIN_LATENT_TAG == int.from_bytes(b"FOLDLT", "big") << 16 and gr.FOLDIN_LATENT_TAG & 0xFFFF == 0
    with open(os.path.join(ROOT, "myfm_amd", "csrc", "mfm_foldin_gibbs.hpp")) as f:
        assert "FOLDIN_LATENT_TAG = 0x%Xull" % gr.FOLDIN_LATENT_TAG in f.read()
    with open(os.path.join(ROOT, "myfm_amd", "csrc", "mfm_foldin.hpp")) as f:
        assert "FOLDIN_DRAW_TAG = 0x%Xull" % gr.FOLDIN_DRAW_TAG in f.read()
    with open(os.path.join(ROOT, "myfm_amd", "csrc", "mfm_foldin_gibbs_plan.hpp")) as f:
        assert "FOLDIN_GIBBS_MAX_SWEEPS = %d" % gr.MAX_SWEEPS in f.read()


# ---- argument validation: estimators restored by __setstate__, no fit, no device -------------------------------------------------
def _restored(task, D=6, K=3, S=2, G=2, with_history=True, fit_linear=True, cutpoints=None, lam_w=None, mu_V=None):
    import myfm_amd
    from myfm_amd import _myfm

    rng = np.random.default_rng(5)
    ordered = task == "ordered"
    cuts = [np.array([-0.5, 0.4, 1.0])] if cutpoints is None else cutpoints
    fms = []
    for _ in range(S):
        fm = _myfm.FM.__new__(_myfm.FM)
        fm.__setstate__((0.5, rng.normal(size=D), rng.normal(size=(D, K)), [np.asarray(c, dtype=np.float64) for c in cuts] if ordered else []))
        fms.append(fm)
    p = _myfm.Predictor.__new__(_myfm.Predictor)
    p.__setstate__((K, D, int(_myfm.TaskType.ORDERED if ordered else _myfm.TaskType.CLASSIFICATION), fms))
    est = (myfm_amd.MyFMOrderedProbit if ordered else myfm_amd.MyFMGibbsClassifier)(K, fit_linear=fit_linear)
    est.predictor_ = p
    est.n_groups_ = G
    if with_history:
        hypers = []
        for _ in range(S + 1):
            h = _myfm.FMHyperParameters.__new__(_myfm.FMHyperParameters)
            h.__setstate__((1.0, rng.normal(size=G), rng.uniform(1, 2, size=G) if lam_w is None else np.full(G, lam_w),
                            rng.normal(size=(G, K)) if mu_V is None else np.full((G, K), mu_V), rng.uniform(1, 2, size=(G, K))))
            hypers.append(h)
        hist = _myfm.LearningHistory.__new__(_myfm.LearningHistory)
        hist.__setstate__((hypers, [], []))
        est.history_ = hist
    return est


@pytest.mark.parametrize("task", ["classifier", "ordered"])
def test_argument_checks_need_no_gpu(task):
    import myfm_amd
    from myfm_amd import _myfm

    est = _restored(task)
    X = sps.csr_matrix(np.eye(4, 6))
    y, ent = np.array([1, 0, 1, 0]), np.array([1, 0, 1, 2])
    # the checks fold_in makes, with its messages
    with pytest.raises(ValueError, match="X has 5 columns but the fitted feature size is 6"):
        est.fold_in_gibbs(sps.csr_matrix((4, 5)), y, ent, 0)
    with pytest.raises(ValueError, match="scipy sparse"):
        est.fold_in_gibbs(np.eye(4, 6), y, ent, 0)
    with pytest.raises(ValueError, match="X has 4 rows but y has 3"):
        est.fold_in_gibbs(X, y[:3], ent, 0)
    with pytest.raises(ValueError, match="X has 4 rows but entity has shape"):
        est.fold_in_gibbs(X, y, ent[:3], 0)
    with pytest.raises(ValueError, match="negative index"):
        est.fold_in_gibbs(X, y, np.array([1, -1, 0, 0]), 0)
    with pytest.raises(ValueError, match="entity holds index 2 but n_entities is 2"):
        est.fold_in_gibbs(X, y, ent, 0, n_entities=2)
    with pytest.raises(ValueError, match="must hold integers"):
        est.fold_in_gibbs(X, y, ent * 0.5, 0)
    with pytest.raises(ValueError, match="an empty entity array needs n_entities"):
        est.fold_in_gibbs(sps.csr_matrix((0, 6)), np.zeros(0), np.zeros(0, dtype=np.int64), 0)
    with pytest.raises(ValueError, match="n_entities must be"):
        est.fold_in_gibbs(X, y, ent, 0, n_entities=-1)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="y holds a value that is not finite"):
            est.fold_in_gibbs(X, np.array([0.0, bad, 1.0, 0.0]), ent, 0)
    for g in (-1, 2, 1.0, True, None):
        with pytest.raises(ValueError, match=r"group must be an integer in \[0, 2\)"):
            est.fold_in_gibbs(X, y, ent, g)
    # the chain's length
    for kw in (dict(n_inner=0), dict(n_inner=-3), dict(n_inner=2.0), dict(n_inner=True)):
        with pytest.raises(ValueError, match="n_inner must be an integer of at least 1"):
            est.fold_in_gibbs(X, y, ent, 0, **kw)
    for kw in (dict(n_burn=-1), dict(n_burn=None)):
        with pytest.raises(ValueError, match="n_burn must be an integer of at least 0"):
            est.fold_in_gibbs(X, y, ent, 0, **kw)
    with pytest.raises(ValueError, match="n_burn \\+ n_inner must not exceed 65535"):
        est.fold_in_gibbs(X, y, ent, 0, n_burn=65535, n_inner=1)
    with pytest.raises(ValueError, match="n_burn \\+ n_inner must not exceed 65535"):
        est.fold_in_gibbs(X, y, ent, 0, n_burn=0, n_inner=65536)
    # the prior of the kept samples
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="prior precision that is not positive and finite"):
            _restored(task, lam_w=bad).fold_in_gibbs(X, y, ent, 0)
    with pytest.raises(ValueError, match="prior mean that is not finite"):
        _restored(task, mu_V=np.inf).fold_in_gibbs(X, y, ent, 0)
    # (component 0 is not read without the linear term: see the end)
    # the rank limit, a missing history, before fit
    big = _restored(task, K=myfm_amd.FOLD_IN_MAX_RANK + 1, S=1)
    with pytest.raises(ValueError, match="fold_in_gibbs serves ranks up to 64, this model has rank 65"):
        big.fold_in_gibbs(X, y, ent, 0)
    with pytest.raises(RuntimeError, match="history_"):
        _restored(task, with_history=False).fold_in_gibbs(X, y, ent, 0)
    with pytest.raises(RuntimeError, match="before fit"):
        type(est)(2).fold_in_gibbs(X, y, ent, 0)
    # valid arguments: the usual refusal of a machine without a GPU comes only now
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fold_in_gibbs(X, y, ent, 1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fold_in_gibbs(X, y, ent, np.int64(0), n_entities=9, draw=True, random_seed=3, n_burn=0, n_inner=1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _restored(task, lam_w=-1.0, fit_linear=False).fold_in_gibbs(X, y, ent, 0)


def test_ordered_probit_argument_checks_need_no_gpu():
    from myfm_amd import _myfm

    est = _restored("ordered")  # 3 cutpoints: classes 0 .. 3
    X = sps.csr_matrix(np.eye(4, 6))
    ent = np.array([1, 0, 1, 2])
    for bad in ([0, 1, 2, 4], [0, -1, 2, 3], [0, 1.5, 2, 3]):
        with pytest.raises(ValueError, match=r"y must hold integer class labels in \[0, 4\)"):
            est.fold_in_gibbs(X, np.array(bad), ent, 0)
    for ci in (1, -1):
        with pytest.raises(ValueError, match="cutpoint_index %d out of range" % ci):
            est.fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0, cutpoint_index=ci)
    for ci in (0.0, True, None):
        with pytest.raises(ValueError, match="cutpoint_index must be an integer"):
            est.fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0, cutpoint_index=ci)
    # the second group has 2 cutpoints: labels in [0, 3)
    two = _restored("ordered", cutpoints=[[-0.5, 0.4, 1.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match=r"labels in \[0, 3\)"):
        two.fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0, cutpoint_index=1)
    with pytest.raises(ValueError, match="cutpoint that is not finite"):
        _restored("ordered", cutpoints=[[-0.5, np.nan, 1.0]]).fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0)
    with pytest.raises(ValueError, match="cutpoint that is not finite"):
        _restored("ordered", cutpoints=[[-0.5, 0.0, np.inf]]).fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0)
    with pytest.raises(ValueError, match="not non-decreasing"):
        _restored("ordered", cutpoints=[[-0.5, 1.0, 0.4]]).fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0)
    if _myfm.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            two.fold_in_gibbs(X, np.array([0, 1, 2, 2]), ent, 0, cutpoint_index=1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # equal cutpoints are non-decreasing
            _restored("ordered", cutpoints=[[-0.5, 0.4, 0.4]]).fold_in_gibbs(X, np.array([0, 1, 2, 3]), ent, 0)


def test_classifier_takes_labels_as_fit_does():
    from myfm_amd import _myfm

    est = _restored("classifier")
    X, ent = sps.csr_matrix(np.eye(4, 6)), np.array([1, 0, 1, 2])
    if _myfm.device_count() == 0:
        for y in (np.array([True, False, True, False]), [0, 1, 1, 0], np.array([0.0, 1.0, 1.0, 0.0])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                est.fold_in_gibbs(X, y, ent, 0)


# ---- the native host code under a host sanitizer ---------------------------------------------------------------------------------
PLAN_MAIN = os.path.join(ROOT, "tests", "native", "foldin_gibbs_plan_main.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_chunk_plan_and_refusals_under_a_host_sanitizer(tmp_path):
    """tests/native/foldin_gibbs_plan_main.cpp: a stand-alone program around csrc/mfm_foldin_gibbs_plan.hpp (no HIP, no device),
    compiled with -fsanitize=address,undefined. It checks that the chunks of random entity offsets cover every (entity, sample)
    exactly once, that a chunk of more than one cell stays under the bound, and every refusal of the argument check."""
    exe = str(tmp_path / "plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "myfm_amd", "csrc"), PLAN_MAIN, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0, out.stdout.decode()
    assert b"plan: ok" in out.stdout and b"check: ok" in out.stdout


# ---- the exports -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_and_exported():
    import myfm_amd
    from myfm_amd import _capi, _myfm

    with open(os.path.join(ROOT, "include", "myfm_hip.h")) as f:
        declared = set(re.findall(r"\b(mfm_[A-Za-z0-9_]+)\s*\(", f.read()))
    L = _capi.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mfm_[A-Za-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert callable(_capi.FoldIn.solve_gibbs) and callable(_capi.FoldIn.solve_gibbs_store)
    assert hasattr(_myfm.Predictor, "fold_in_gibbs_solve")
    assert callable(myfm_amd.MyFMGibbsClassifier.fold_in_gibbs) and callable(myfm_amd.MyFMOrderedProbit.fold_in_gibbs)
    assert myfm_amd.MyFMClassifier is myfm_amd.MyFMGibbsClassifier
    # closed form there, inner chain here: the regressor has no fold_in_gibbs, the variational estimators have neither
    assert not hasattr(myfm_amd.MyFMGibbsRegressor, "fold_in_gibbs")
    for cls in ("VariationalFMRegressor", "VariationalFMClassifier"):
        assert not hasattr(getattr(myfm_amd, cls), "fold_in") and not hasattr(getattr(myfm_amd, cls), "fold_in_gibbs")
    for cls in ("MyFMGibbsClassifier", "MyFMOrderedProbit"):
        assert not hasattr(getattr(myfm_amd, cls), "fold_in")
    # the shared argument helper left the regressor's method where it was
    assert callable(myfm_amd.MyFMGibbsRegressor.fold_in)
