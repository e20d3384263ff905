"""The vector operations of the Krylov solvers on tensors (krylov_vectors._TensorOps, _TreeTensorOps, _DirectSumOps) method
by method against numpy, on a numpy stand-in: the checks of tests/pool_ops_cases.py that tests/test_gpu_pool_ops.py runs on
pools.  Validates the reference and the case builders without a device and pins ``_mgs``, ``_TensorOps.combine`` and
``_TensorOps.rotate``; what only a pool has (gaps, support, ``_promote``, ``orthonormalize``) is left to the device file."""
import numpy as np
import pytest

import direct_sum_cases as dc
import pool_ops_cases as pc
from cyten_amd import krylov_vectors as kv

LAYOUTS = list(pc.LAYOUTS)
CLASSES = {'abelian': kv._TensorOps, 'tree': kv._TreeTensorOps, 'abelian+abelian': kv._DirectSumOps,
           'abelian+tree': kv._DirectSumOps, 'three': kv._DirectSumOps}
_cases = {}


@pytest.fixture
def nbb():
    return dc.NumpyDirectSumBackend()


def _rig(nbb, layout):
    if layout not in _cases:
        _cases[layout] = pc.OpsCase(nbb, layout)
    case = _cases[layout]
    V = kv._vector_ops(case.bb, case.H, case.template, None)
    assert type(V) is CLASSES[layout]
    return pc.Rig(case, V)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_case_coordinates_and_dense_operator(nbb, rng, layout):
    """the case builders: coordinates round-trip bit for bit, a subset holds fewer blocks, y is the scaled form in which the
    container's inner product is the plain one and the operator the dense matrix"""
    rig = _rig(nbb, layout)
    case = rig.case
    x, u = case.rand(rng, True)
    assert case.u(x).tobytes() == u.tobytes()
    xs, us = case.rand(rng, False, subset=True)
    comps = xs.components if case.is_sum else [xs]
    assert sum(len(t.blocks) for t in comps) == len(case.subset) and case.u(xs).tobytes() == us.tobytes()
    y = case.s * u
    assert abs(rig.V.norm(x) - np.linalg.norm(y)) <= 1e-13 * np.linalg.norm(y)
    My = case.s * case.u(case.H.matvec(x))
    assert np.linalg.norm(My - case.M @ y) <= 1e-12 * np.linalg.norm(case.M, 2) * np.linalg.norm(y)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_enter_leave(nbb, rng, layout, cplx):
    pc.check_enter_leave(_rig(nbb, layout), rng, cplx)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_scale_lincomb(nbb, rng, layout):
    pc.check_scale_lincomb(_rig(nbb, layout), rng)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_combine(nbb, rng, layout):
    pc.check_combine(_rig(nbb, layout), rng)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_inner_norm(nbb, rng, layout):
    pc.check_inner_norm(_rig(nbb, layout), rng)


def test_three_four_five(nbb):
    pc.check_three_four(nbb, kv._vector_ops(nbb, None, dc.three_four(nbb), None))


@pytest.mark.parametrize('kind', ['general', 'ortho', 'mixed'])
@pytest.mark.parametrize('passes', [1, 2])
@pytest.mark.parametrize('m', [0, 1, 5, 64, 65])
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_project_out(nbb, rng, layout, cplx, m, passes, kind):
    """(``passes`` is not read on tensors: one pass of modified Gram-Schmidt)"""
    pc.check_project_out(_rig(nbb, layout), rng, cplx, passes, m, kind)


@pytest.mark.parametrize('m,k', pc.ROTATIONS)
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_rotate(nbb, rng, layout, cplx, m, k):
    pc.check_rotate(_rig(nbb, layout), rng, cplx, m, k)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_operator_wrappers(nbb, rng, layout, cplx):
    pc.check_apply(_rig(nbb, layout), rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_orthonormalize_list_is_decided_by_the_reference(nbb, rng, layout, cplx):
    """the builder of the list that the device file hands to ``orthonormalize`` (its assertions run inside)"""
    us, norms, flags = pc.orthonormalize_list(_rig(nbb, layout).case, rng, cplx)
    assert len(us) == 6 and flags.sum() == 4
