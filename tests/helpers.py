"""Shared helpers of the test-suite: plain-data tensors <-> device tensors, invariant checks."""
import numpy as np

from cyten_amd import abelian as ab
from cyten_amd import workloads as wl


def to_device_tensor(bb, spec: wl.TensorSpec) -> ab.AbelianTensor:
    return ab.AbelianTensor.from_spec(bb, spec)


def check_svd_invariants(a, U, S, Vh, tol=1e-10, sref=None):
    """The reference's SVD acceptance criteria (tests/python_tests/test_tensors.py:3405-3500):
    S >= 0 and descending, |S| = |A|, U S Vh = A, U^T U = 1, Vh Vh^T = 1 -- plus, with `sref`
    (LAPACK singular values), |S - sref| <= tol * |A|."""
    k = min(a.shape)
    assert U.shape == (a.shape[0], k) and S.shape == (k,) and Vh.shape == (k, a.shape[1])
    nrm = max(np.linalg.norm(a), 1e-300)
    assert np.all(S >= 0)
    assert np.all(S[:-1] >= S[1:] - tol * nrm)
    assert abs(np.linalg.norm(S) - np.linalg.norm(a)) <= tol * nrm
    assert np.abs((U * S) @ Vh - a).max() <= tol * nrm
    assert np.abs(U.T @ U - np.eye(k)).max() <= tol
    assert np.abs(Vh @ Vh.T - np.eye(k)).max() <= tol
    if sref is not None:
        assert np.abs(S - sref).max() <= tol * nrm


def check_svd_accuracy(a, U, S, Vh, sref=None, cap=1e-13, name='block'):
    """The strict sibling of `check_svd_invariants`: the same facts held to the rounding level.  S >= 0 and descending with no
    slack, shapes and dtypes exactly; |U^H U - 1|, |Vh Vh^H - 1|, |U S Vh - A| / sigma_1 and -- with `sref`, reference values
    whose own error is negligible (long double) -- |S - sref| / sigma_1, each formed in long double, each <= `cap`.
    Returns the measures in units of 2^-52 (tests/decomp_accuracy_cases.py)."""
    import decomp_accuracy_cases as dac
    ref = None if sref is None else np.asarray(sref, dtype=np.longdouble)
    return dac.check_svd(dac.Case(name, np.asarray(a), ref), U, S, Vh, cap_eps=cap / dac.EPS)
