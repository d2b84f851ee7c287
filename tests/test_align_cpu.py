"""The reference of aligned_factors against its own twin (tests/align_ref.py): nothing here touches the device."""
import numpy as np
import pytest

from tests import align_ref as ar


@pytest.mark.parametrize("K,S,D,n_refine,weighted", ar.REAL_CASES)
def test_reference_inside_tolerance_of_twin(K, S, D, n_refine, weighted):
    """the float64 rounds stay inside the derived tolerance of the longdouble / 40-digit twin on every real-valued case of the
    GPU test, and each case is as well conditioned as the bound's denominator needs: sigma_K + sigma_{K-1} >= 0.05 sigma_1 in
    every round"""
    Vs, w = ar.real_case(K, S, D, weighted)
    ref = ar.align_ref(Vs, -1, n_refine, w)
    assert ref["min_gap"] >= 0.05
    twin = ar.align_ref(Vs, -1, n_refine, w, twin=True)
    used = ar.shares((ref["mean"], ref["std"], ref["rotations"], ref["alignment"]), twin)
    print("K %d S %d D %d rounds %d weighted %d: used shares %s, min gap %.3f" % (K, S, D, n_refine + 1, weighted, used, ref["min_gap"]))
    assert max(used.values()) <= 1.0
    R = ref["rotations"]
    assert np.sqrt(((np.einsum("sab,sac->sbc", R, R) - np.eye(K)) ** 2).sum(axis=(1, 2))).max() <= ar.jacobi_term(K)


def test_host_checks_raise_without_a_device():
    from myfm_amd import _capi

    for bad in (dict(reference=4), dict(reference=-5), dict(n_refine=9), dict(n_refine=-1), dict(weights=-np.ones(6)),
                dict(weights=np.full(6, np.nan)), dict(weights=np.ones(5)), dict(K=65), dict(reference=1.5)):
        kw = dict(S=4, K=3, D=6, reference=-1, n_refine=1, weights=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            _capi.align_args(**kw)
    assert _capi.align_args(4, 3, 6, -1, 0, None) == (3, 0, None)
