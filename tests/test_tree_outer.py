"""``cyten_amd.fusion_tree.outer`` on the numpy stand-in: the loops, tables and records without a device.  The cases and their
tolerance are in tests/tree_outer_cases.py; tests/test_gpu_tree_outer.py runs the same ones through HipBlockBackend."""
import dataclasses

import numpy as np
import pytest

import tree_outer_cases as cases
import tree_outer_ref as ref
from cyten_amd import fusion_tree as ft


@pytest.fixture
def nb():
    return cases.NumpyOuterBackend()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees against the dense tensor

@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=lambda c: 'x'.join(map(str, c)))
def test_outer_of_abelian_trees_is_the_dense_tensor_product(nb, rng, config, kind):
    c, disagree = cases.check_abelian(nb, rng, config, kind)
    assert len(nb.outer_calls) == 1                                    # ONE tree_outer_many call for the tensor
    if config in [(1, 1, 1, 1), (2, 1, 1, 2)]:
        assert disagree > 0                                            # tiles whose a-side charges disagree exist, and are zeros
        assert any(n == 0 and np.prod(shape) > 0 for shape, n in nb.outer_calls[0])
    assert max(n for _, n in nb.outer_calls[0]) == 1                   # concatenation: one pair per new tree pair


# ---------------------------------------------------------------------------------------------------------------------------
# (b) random tables against the restatement of the reference's loop

@pytest.mark.parametrize('cplx_a,cplx_b', [(False, False), (True, True), (False, True)])
def test_random_tables_with_complex_amplitudes_match_the_restatement(nb, rng, cplx_a, cplx_b):
    """the conditions the case is meant to meet, checked for the seed in use: several pairs feed one tile, one pair feeds
    several coupled sectors, lists are empty, tiles stay without a term"""
    c = cases.check_table(nb, rng, cplx_a, cplx_b)
    records = nb.outer_calls[0]
    assert len(nb.outer_calls) == 1
    assert any(n >= 2 for _, n in records) and any(n == 0 and np.prod(shape) > 0 for shape, n in records)
    for tb in (c['ct'], c['dt']):
        assert any(len(lst) == 0 for lst in tb.table.values())
        sectors = [{k[2] for k, _ in lst} for lst in tb.table.values()]
        assert any(len(s) >= 2 for s in sectors)
        targets = [k for lst in tb.table.values() for k, _ in lst]
        assert len(set(targets)) < len(targets)                        # several (alpha, beta) go to the same gamma


def test_real_data_under_real_amplitudes_stays_float64(nb, rng):
    cases.check_table(nb, rng, False, False, cplx_amps=False)


def test_blocks_without_a_term_are_absent_and_all_tiles_of_the_others_are_emitted(nb, rng):
    c = cases.table_case(rng, False, False)
    got = cases.run_outer(nb, c, discard=False)
    fed = set()
    for (ca, cb), lst in c['ct'].table.items():
        for (da, db), lst2 in c['dt'].table.items():
            if ca[2] == da[2] and cb[2] == db[2]:                      # (the data holds the diagonal sectors of a and of b)
                fed |= {k[2] for k, _ in lst} & {k[2] for k, _ in lst2}
    assert got.block_inds.tolist() == [[s, s] for s in sorted(fed)]
    n_tiles = sum(len(c['n_cod'].tree_blocks[s]) * len(c['n_dom'].tree_blocks[s]) for s in fed)
    assert len(nb.outer_calls[0]) == n_tiles
    assert not any(np.isnan(blk).any() for blk in got.blocks)          # (empty_many hands out NaN)


def test_coefficient_conjugates_the_codomain_amplitude(nb):
    """u = i, v = 1: conj(u) v (A (x) B) = -i (A (x) B), the opposite placement to partial_trace's f_cod conj(f_dom); exact
    integer data, compared with =="""
    mk = ft.TreeSpace.from_multiplicities
    a_cod, a_dom = mk([[0]], [[(2,)]], None, 1, [['xa']]), mk([[0]], [[(3,)]], None, 1, [['ya']])
    b_cod, b_dom = mk([[0]], [[(2,)]], None, 1, [['xb']]), mk([[0]], [[(2,)]], None, 1, [['yb']])
    n_cod, n_dom = mk([[0]], [[(2, 2)]], None, 2, [['x']]), mk([[0]], [[(3, 2)]], None, 2, [['y']])
    A, B = np.arange(-3.0, 3.0).reshape(2, 3), np.array([[1.0, -2.0], [3.0, 5.0]])
    got = ft.outer(nb, ft.FusionTreeData([(0, 0)], [A]), a_cod, a_dom, ft.FusionTreeData([(0, 0)], [B]), b_cod, b_dom, n_cod, n_dom,
                   ft.TreeOuter({('xa', 'xb'): [('x', 1j)]}), ft.TreeOuter({('ya', 'yb'): [('y', 1.0)]}))
    assert got.block_inds.tolist() == [[0, 0]]
    assert np.array_equal(got.blocks[0], -1j * np.kron(A, B))
    # and the other way round: u = 1, v = i gives +i
    got = ft.outer(nb, ft.FusionTreeData([(0, 0)], [A]), a_cod, a_dom, ft.FusionTreeData([(0, 0)], [B]), b_cod, b_dom, n_cod, n_dom,
                   ft.TreeOuter({('xa', 'xb'): [('x', 1.0)]}), ft.TreeOuter({('ya', 'yb'): [('y', 1j)]}))
    assert np.array_equal(got.blocks[0], 1j * np.kron(A, B))


def test_terms_come_in_the_documented_order(rng):
    """one tile fed by 2 x 2 tree pairs of a times 1 x 1 of b: a's codomain trees, then a's domain trees"""
    mk = ft.TreeSpace.from_multiplicities
    a_cod, a_dom = mk([[0]], [[(1,), (1,)]], None, 1, [['x0', 'x1']]), mk([[0]], [[(1,), (1,)]], None, 1, [['y0', 'y1']])
    b_sp = mk([[0]], [[(2,)]], None, 1, [['z']])
    n_sp = mk([[0]], [[(1, 2)]], None, 2, [['n']])
    ct = ft.TreeOuter({('x0', 'z'): [('n', 2.0)], ('x1', 'z'): [('n', 3.0)]})
    dt = ft.TreeOuter({('y0', 'z'): [('n', 5.0)], ('y1', 'z'): [('n', 7.0)]})
    seen = []

    class Spy(cases.NumpyOuterBackend):
        def tree_outer_many(self, outputs):
            seen.extend(outputs)
            super().tree_outer_many(outputs)

    A, B = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    ft.outer(Spy(), ft.FusionTreeData([(0, 0)], [A]), a_cod, a_dom, ft.FusionTreeData([(0, 0)], [B]), b_sp, b_sp, n_sp, n_sp, ct, dt)
    (dst, terms), = seen
    assert [t[2] for t in terms] == [10.0, 14.0, 15.0, 21.0]
    assert [float(t[0][0, 0]) for t in terms] == [A[0, 0], A[0, 1], A[1, 0], A[1, 1]]
    assert all(isinstance(t[2], float) for t in terms)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) SU(2)

@pytest.mark.parametrize('cplx', [False, True])
def test_su2_interchange_law_with_tables_from_fusion_rules(nb, rng, cplx):
    cases.check_su2_interchange(nb, rng, cplx)


@pytest.mark.parametrize('m', [(1, 1, 1, 1), (2, 1, 3, 2), (3, 2, 1, 3)])
def test_su2_identity_times_identity_is_the_identity_by_F_unitarity(nb, m):
    c = cases.check_su2_identity(nb, m)
    amps = [x for lst in c['ct'].table.values() for _, x in lst]
    assert any(abs(abs(x) - 1.0) > 1e-3 and abs(x) > 1e-3 for x in amps)           # genuine F symbols, not signs
    assert any(n >= 2 for _, n in nb.outer_calls[0])


# ---------------------------------------------------------------------------------------------------------------------------
# (d) a zero-leg operand

@pytest.mark.parametrize('cplx', [False, True])
def test_zero_leg_operand_scales_the_other(nb, rng, cplx):
    cases.check_zero_leg(nb, rng, cplx)


def test_two_zero_leg_operands_give_the_product_of_the_scalars(nb):
    one = ft.TreeSpace.from_multiplicities([[0]], [[()]], None, 0, [['e']], [[()]])
    tb = ft.TreeOuter({('e', 'e'): [('e', 1.0)]})
    got = ft.outer(nb, ft.FusionTreeData([(0, 0)], [np.array([[3.0]])]), one, one, ft.FusionTreeData([(0, 0)], [np.array([[-0.5]])]), one, one,
                   one, one, tb, tb)
    assert got.block_inds.tolist() == [[0, 0]] and got.blocks[0].tolist() == [[-1.5]]


# ---------------------------------------------------------------------------------------------------------------------------
# error paths

def _replace_tree(space: ft.TreeSpace, tree, **changes) -> ft.TreeSpace:
    blocks = [[dataclasses.replace(tb, **changes) if tb.tree == tree else tb for tb in tbs] for tbs in space.tree_blocks]
    return ft.TreeSpace(space.sectors, space.qdims, blocks, space.num_legs)


def test_error_a_tree_pair_of_the_data_is_absent_from_the_table(nb, rng):
    c = cases.table_case(rng, False, False)
    table = dict(c['ct'].table)
    del table[next(iter(table))]
    c['ct'] = ft.TreeOuter(table)
    with pytest.raises(ValueError, match='no entry'):
        cases.run_outer(nb, c)
    assert not nb.outer_calls


def test_error_a_new_tree_the_new_space_does_not_hold(nb, rng):
    c = cases.table_case(rng, False, False)
    table = dict(c['dt'].table)
    key = next(k for k, lst in table.items() if lst)
    table[key] = [(('d', 'nowhere'), 1.0)]
    c['dt'] = ft.TreeOuter(table)
    with pytest.raises(ValueError, match='no tree'):
        cases.run_outer(nb, c)
    assert not nb.outer_calls


def test_error_a_new_tree_whose_multiplicities_are_not_those_of_its_factors(nb, rng):
    c = cases.table_case(rng, False, False)
    target = next(k for lst in c['ct'].table.values() for k, _ in lst)
    m = c['n_cod'].tree_block_slice(target)[1].multiplicities
    c['n_cod'] = _replace_tree(c['n_cod'], target, multiplicities=(m[1] + 1, m[0]))
    with pytest.raises(ValueError, match='multiplicities'):
        cases.run_outer(nb, c)
    assert not nb.outer_calls


def test_restatement_of_one_pair_is_the_kronecker_product(rng):
    mk = ft.TreeSpace.from_multiplicities
    sp = lambda n, name: mk([[0]], [[(n,)]], None, 1, [[name]])                       # noqa: E731
    A, B = rng.standard_normal((2, 3)), rng.standard_normal((4, 5))
    got = ref.outer_ref(ft.FusionTreeData([(0, 0)], [A]), sp(2, 'a'), sp(3, 'b'), ft.FusionTreeData([(0, 0)], [B]), sp(4, 'c'), sp(5, 'd'),
                        mk([[0]], [[(2, 4)]], None, 2, [['x']]), mk([[0]], [[(3, 5)]], None, 2, [['y']]),
                        ft.TreeOuter({('a', 'c'): [('x', 1.0)]}), ft.TreeOuter({('b', 'd'): [('y', 1.0)]}))
    assert np.array_equal(got[(0, 0)], np.einsum('ij,kl->ikjl', A, B).reshape(8, 15))
