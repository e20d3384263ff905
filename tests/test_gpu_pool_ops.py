"""The pool layer between the Krylov solvers and the pool kernels (krylov_vectors._FlatOps on the layouts of an abelian
tensor, a fusion-tree tensor and direct sums) method by method against numpy: which entry runs (float64 or complex128,
weighted or not), over which length, with which pointers, and what happens when the pools of one call differ in dtype.
The cases, the reference, the bounds and the checks are those of tests/pool_ops_cases.py, which tests/test_pool_ops.py runs
on the tensor classes without a device; here they run on pools of both dtypes and on the tensor classes on the device.
Every pool a check looks at is downloaded whole and must be +0.0 byte for byte outside its blocks."""
import pytest

import direct_sum_cases as dc
import pool_ops_cases as pc
from cyten_amd import krylov_vectors as kv

pytestmark = pytest.mark.gpu

LAYOUTS = list(pc.LAYOUTS)
POOLS = {'abelian': kv._FlatOps, 'tree': kv._FlatTreeOps, 'abelian+abelian': kv._FlatDirectSumOps,
         'abelian+tree': kv._FlatDirectSumOps, 'three': kv._FlatDirectSumOps}
TENSORS = {'abelian': kv._TensorOps, 'tree': kv._TreeTensorOps, 'abelian+abelian': kv._DirectSumOps,
           'abelian+tree': kv._DirectSumOps, 'three': kv._DirectSumOps}
both_dtypes = pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
all_layouts = pytest.mark.parametrize('layout', LAYOUTS)


@pytest.fixture(scope='module')
def cases(bb):
    made = {}

    def get(layout, cplx_op=False):
        if (layout, cplx_op) not in made:
            made[layout, cplx_op] = pc.OpsCase(bb, layout, cplx_op)
        return made[layout, cplx_op]
    return get


def _pools(cases, layout, cplx):
    """a rig on fresh pool ops objects of both dtypes; the one under test has the dtype `cplx`"""
    case = cases(layout)
    Vr, Vc = (kv._vector_ops(case.bb, case.H, case.template, mode) for mode in (False, True))
    for V, mode in ((Vr, False), (Vc, True)):
        assert type(V) is POOLS[layout] and V.cplx is mode and V.total <= 3072
        assert V.weighted == (layout in pc.WEIGHTED)
    return pc.Rig(case, Vc if cplx else Vr, Vr, Vc)


def _tensors(cases, layout):
    case = cases(layout)
    V = kv._vector_ops(case.bb, case.H, case.template, None)
    assert type(V) is TENSORS[layout]
    return pc.Rig(case, V)


# ---------------------------------------------------------------------------------------------------------------------------
# pools

@both_dtypes
@all_layouts
def test_pool_enter_leave(cases, rng, layout, cplx):
    pc.check_enter_pool(_pools(cases, layout, cplx), rng)
    pc.check_enter_leave(_pools(cases, layout, cplx), rng, cplx)


@both_dtypes
@all_layouts
def test_pool_promote(cases, rng, layout, cplx):
    pc.check_promote(_pools(cases, layout, cplx), rng)


@both_dtypes
@all_layouts
def test_pool_scale_lincomb(cases, rng, layout, cplx):
    pc.check_scale_lincomb(_pools(cases, layout, cplx), rng)


@both_dtypes
@all_layouts
def test_pool_combine(cases, rng, layout, cplx):
    pc.check_combine(_pools(cases, layout, cplx), rng)


@both_dtypes
@all_layouts
def test_pool_inner_norm(cases, rng, layout, cplx):
    pc.check_inner_norm(_pools(cases, layout, cplx), rng)


@both_dtypes
def test_pool_three_four_five(bb, cplx):
    pc.check_three_four(bb, kv._vector_ops(bb, None, dc.three_four(bb), cplx))


# (kind, m, passes): m = 65 is beyond MAX_BASIS and a basis of mixed dtypes never reaches the fused kernel -- both run _mgs
PROJECTIONS = ([('general', m, p) for m in (0, 1, 5) for p in (1, 2)] + [('general', 64, 2), ('general', 65, 2)]
               + [('ortho', m, p) for m in (1, 5) for p in (1, 2)] + [('ortho', 64, 2), ('ortho', 65, 2)])


@pytest.mark.parametrize('kind,m,passes', PROJECTIONS)
@both_dtypes
@all_layouts
def test_pool_project_out(cases, rng, layout, cplx, kind, m, passes):
    pc.check_project_out(_pools(cases, layout, cplx), rng, cplx, passes, m, kind)


@pytest.mark.parametrize('passes', [1, 2])
@both_dtypes
@all_layouts
def test_pool_project_out_mixed_dtypes(cases, rng, layout, cplx, passes):
    pc.check_project_out(_pools(cases, layout, cplx), rng, cplx, passes, 5, 'mixed')


@pytest.mark.parametrize('m,k', pc.ROTATIONS)
@both_dtypes
@all_layouts
def test_pool_rotate(cases, rng, layout, cplx, m, k):
    pc.check_rotate(_pools(cases, layout, cplx), rng, cplx, m, k)


@both_dtypes
@all_layouts
def test_pool_rotate_errors(cases, rng, layout, cplx):
    pc.check_rotate_errors(_pools(cases, layout, cplx), rng)


@both_dtypes
@all_layouts
def test_pool_orthonormalize(cases, rng, layout, cplx):
    pc.check_orthonormalize(_pools(cases, layout, cplx), rng, cplx)


@both_dtypes
@all_layouts
def test_pool_operator_wrappers(cases, rng, layout, cplx):
    pc.check_apply(_pools(cases, layout, cplx), rng, cplx)


@all_layouts
def test_pool_operator_wrappers_need_complex(cases, rng, layout):
    pc.check_apply_needs_complex(_pools(cases, layout, False), rng, cases(layout, True))


# ---------------------------------------------------------------------------------------------------------------------------
# the tensor classes on the device: the same checks as on the numpy stand-in

@both_dtypes
@all_layouts
def test_tensor_enter_leave(cases, rng, layout, cplx):
    pc.check_enter_leave(_tensors(cases, layout), rng, cplx)


@all_layouts
def test_tensor_blas1_all_dtype_pairs(cases, rng, layout):
    rig = _tensors(cases, layout)
    pc.check_scale_lincomb(rig, rng)
    pc.check_combine(rig, rng)
    pc.check_inner_norm(rig, rng)


@pytest.mark.parametrize('kind,m', [('general', 0), ('general', 5), ('ortho', 5), ('mixed', 5), ('ortho', 65)])
@both_dtypes
@all_layouts
def test_tensor_project_out(cases, rng, layout, cplx, kind, m):
    pc.check_project_out(_tensors(cases, layout), rng, cplx, 2, m, kind)


@pytest.mark.parametrize('m,k', [(5, 5), (3, 5), (3, 0)])
@both_dtypes
@all_layouts
def test_tensor_rotate(cases, rng, layout, cplx, m, k):
    pc.check_rotate(_tensors(cases, layout), rng, cplx, m, k)


@both_dtypes
@all_layouts
def test_tensor_operator_wrappers(cases, rng, layout, cplx):
    pc.check_apply(_tensors(cases, layout), rng, cplx)
