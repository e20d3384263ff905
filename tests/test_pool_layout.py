"""Where the blocks of a Krylov vector lie in its pool (cyten_amd.krylov_vectors.PoolLayout), on the CPU: the layout is host
arithmetic, so the numpy stand-in and the vectors of tests/direct_sum_cases.py show all of it.  The pinned numbers follow
from the rules: abelian blocks (5, 9, 140 elements for 'ab2', 23 for 'ab1') at multiples of 32 elements, tree blocks
(tests/tree_krylov_cases.py) at multiples of 256, and with a tree component every segment padded to a multiple of 256 with the
weight 1.0 on the granules of abelian segments.  The first two are what tests/test_gpu_direct_sum.py finds on the device."""
import numpy as np
import pytest

import direct_sum_cases as dc
import tree_krylov_cases as tcases
from cyten_amd import direct_sum as ds
from cyten_amd import krylov
from cyten_amd.krylov_vectors import PoolLayout

PHI = tcases.PHI
THREE = (('ab2', 2.0), ('tree', 2.5), ('ab1', -5.5))


@pytest.fixture
def nbb():
    return dc.NumpyDirectSumBackend()


def _same(a, b):
    return (a.offs == b.offs and a.total == b.total and a.shapes == b.shapes and a.strides == b.strides and a.weighted == b.weighted
            and np.array_equal(a.weights, b.weights) and all(np.array_equal(x, y) for x, y in zip(a.tables, b.tables)))


def _check_bounds(L):
    """every block inside its segment, every segment at a multiple of the alignment"""
    align = 256 if L.weighted else 32
    ends = L.first[1:] + [len(L.offs)]
    seg_end = [L.offs[e] if e < len(L.offs) else L.total for e in ends]
    for first, last, end in zip(L.first, ends, seg_end):
        assert L.offs[first] % align == 0 and end % align == 0
        for p in range(first, last):
            nxt = L.offs[p + 1] if p + 1 < last else end
            assert L.offs[p] + int(np.prod(L.shapes[p])) <= nxt
    assert L.total % align == 0 and len(L.weights) == (L.total // 256 if L.weighted else 0)


def test_three_components_with_a_tree(nbb):
    L = PoolLayout(dc.SumCase(nbb, THREE, 0).psi0)
    assert L.offs == [0, 32, 64, 256, 512, 768, 1024, 2816] and L.total == 3072
    assert L.weights.tolist() == [1.0, 1.0, 2.0, 3.0] + [PHI] * 7 + [1.0]
    assert L.weighted and L.first == [0, 3, 7]
    _check_bounds(L)


def test_without_a_tree_component(nbb):
    L = PoolLayout(dc.SumCase(nbb, 'abelian+abelian').psi0)
    assert L.offs == [0, 32, 64, 224] and L.total == 256
    assert L.weights.tolist() == [] and not L.weighted
    _check_bounds(L)


def test_one_abelian_component_is_the_bare_tensor(nbb):
    case = dc.SumCase(nbb, (('ab2', 2.0),))
    L = PoolLayout(case.psi0)
    assert L.offs == [0, 32, 64] and L.total == 224 and not L.weighted and L.shapes == [(1, 5), (9, 1), (20, 7)]
    assert L.strides == [(5, 1), (1, 1), (7, 1)]
    bare = PoolLayout(case.parts[0].psi0)
    assert _same(L, bare) and L.is_sum and not bare.is_sum
    _check_bounds(L)


def test_one_tree_component_is_tree_pool_layout(nbb):
    case = dc.SumCase(nbb, (('tree', 2.5),))
    L = PoolLayout(case.psi0)
    assert L.offs == [0, 256, 512, 768] and L.total == 2560 and L.weighted
    assert L.weights.tolist() == [1.0, 2.0, 3.0] + [PHI] * 7
    t = case.parts[0].psi0
    inds, shapes, offs, total, weights = krylov.tree_pool_layout(t.codomain, t.domain)
    assert np.array_equal(L.tables[0], inds) and L.shapes == list(shapes) and L.offs == list(offs) and L.total == total
    assert np.array_equal(L.weights, weights)
    assert _same(L, PoolLayout(t))
    _check_bounds(L)


def test_positions(nbb):
    case = dc.SumCase(nbb, THREE, 0)
    L = PoolLayout(case.psi0)
    assert L.positions(case.psi0) == list(range(8))                                    # the full block tables
    ab2, tree, ab1 = case.parts
    assert L.positions(ab2.psi0, 0) == [0, 1, 2] and L.positions(tree.psi0, 1) == [3, 4, 5, 6] and L.positions(ab1.psi0, 2) == [7]
    some = ds.DirectSum([ab2.tensor(ab2.y0, keep=[0, 2]), tree.tensor(tree.y0, keep=[1, 3]), ab1.psi0])
    assert L.positions(some) == [0, 2, 4, 6, 7]
    swapped = ab2.tensor(ab2.y0, keep=[0, 2])                                          # rows in the tensor's order
    swapped.block_inds = ab2.inds[[2, 0]]
    assert L.positions(swapped, 0) == [2, 0]
    foreign = ab2.tensor(ab2.y0, keep=[0])
    foreign.block_inds = np.array([[0, 3]])
    with pytest.raises(krylov._NotFlat):
        L.positions(foreign, 0)
    for wrong in (ds.DirectSum([ab2.psi0, tree.psi0]), ab2.psi0):
        with pytest.raises(krylov._NotFlat):
            L.positions(wrong)
    bare = PoolLayout(ab2.psi0)
    assert bare.positions(ab2.psi0) == [0, 1, 2] and bare.positions(ab2.tensor(ab2.y0, keep=[1])) == [1]
    with pytest.raises(krylov._NotFlat):
        bare.positions(case.psi0)
