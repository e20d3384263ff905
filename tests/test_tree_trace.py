"""``cyten_amd.fusion_tree.partial_trace`` on the numpy stand-in: the loops, tables and records without a device.  The cases
and their tolerance are in tests/tree_trace_cases.py; tests/test_gpu_tree_trace.py runs the same ones through HipBlockBackend."""
import numpy as np
import pytest

import tree_trace_cases as cases
import tree_trace_ref as ref
from cyten_amd import fusion_tree as ft
from fusion_tree_cases import AbelianTrees


@pytest.fixture
def nb():
    return cases.NumpyTraceBackend()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees against the dense tensor

@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('name', ['codomain', 'domain', 'both', 'two_pairs', 'between'])
def test_partial_trace_of_abelian_trees_is_the_index_paired_sum_of_the_dense_tensor(nb, rng, name, cplx):
    c, _ = cases.check_abelian(nb, rng, name, cplx)
    assert len(nb.trace_calls) == 1                                    # ONE tree_trace_many call for the tensor
    assert max(n for _, n in nb.trace_calls[0]) >= 2                   # several old trees (traced charges) feed one tile


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('name', ['codomain', 'between'])
def test_tiles_without_a_term_are_zeros_and_sectors_outside_the_new_spaces_are_skipped(nb, rng, name, cplx):
    """the conditions the zero-tile and the skip path need, checked for the seed in use"""
    c, got = cases.check_abelian(nb, rng, name, cplx, starve=True)
    records = nb.trace_calls[0]
    assert any(n == 0 and np.prod(shape) > 0 for shape, n in records)  # a tile of at least one element receives no term ...
    assert any(n >= 2 for _, n in records)                             # ... next to tiles several old trees feed
    new_sectors = {tuple(s) for s in c['n_cod'].sectors.tolist()} & {tuple(s) for s in c['n_dom'].sectors.tolist()}
    data_sectors = {tuple(c['dom'].sectors[j].tolist()) for j in c['data'].block_inds[:, 1]}
    assert data_sectors - new_sectors                                  # a coupled sector of the data is absent from the new spaces
    assert data_sectors & new_sectors


@pytest.mark.parametrize('cplx', [False, True])
def test_full_trace_is_the_one_by_one_block_and_equals_trace_full(nb, rng, cplx):
    cases.check_full_trace(nb, rng, cplx)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) random tables against the restatement of the reference's loop

@pytest.mark.parametrize('cplx_data', [False, True])
def test_random_tables_with_complex_factors_match_the_restatement(nb, rng, cplx_data):
    c = cases.check_forest(nb, rng, cplx_data)
    records = nb.trace_calls[0]
    assert any(n == 0 for _, n in records) and any(n >= 2 for _, n in records)
    n_cod, n_dom = c['n_cod'], c['n_dom']
    assert len(records) == sum(len(n_cod.tree_blocks[i]) * len(n_dom.tree_blocks[j]) for i, j in ft.common_sectors(n_cod, n_dom)
                               if tuple(n_cod.sectors[i]) in {(1,), (2,)})


def test_real_data_under_real_factors_stays_real(nb, rng):
    cases.check_forest(nb, rng, False, cplx_factors=False)


def test_coefficient_conjugates_the_domain_factor_and_terms_come_in_tree_order(nb, rng):
    """one tile, two old codomain trees x two old domain trees: the four terms arrive codomain-major with f_cod conj(f_dom)"""
    mk = ft.TreeSpace.from_multiplicities
    cod = mk([[0]], [[(2, 2), (3, 3)]], None, 2, [['x0', 'x1']], [[('a', 'A'), ('b', 'B')]])
    dom = mk([[0]], [[(1, 1), (2, 2)]], None, 2, [['y0', 'y1']], [[('c', 'C'), ('d', 'D')]])
    one = mk([[0]], [[()]], None, 0, [['e']], [[()]])
    ct = ft.TreeTrace((0,), {'x0': ('e', 2.0 + 1.0j), 'x1': ('e', -1.0j)})
    dt = ft.TreeTrace((0,), {'y0': ('e', 0.5 + 0.5j), 'y1': ('e', 3.0j)})
    blk = rng.standard_normal((13, 5))
    seen = []

    class Spy(cases.NumpyTraceBackend):
        def tree_trace_many(self, outputs):
            seen.extend(outputs)
            super().tree_trace_many(outputs)

    got = ft.partial_trace(Spy(), ft.FusionTreeData([(0, 0)], [blk]), cod, dom, one, one, ct, dt)
    (dst, terms), = seen
    want_c = [(2 + 1j) * np.conj(0.5 + 0.5j), (2 + 1j) * np.conj(3j), -1j * np.conj(0.5 + 0.5j), -1j * np.conj(3j)]
    assert [t[4] for t in terms] == want_c
    assert [t[0].shape for t in terms] == [(2, 2, 1, 1), (2, 2, 2, 2), (3, 3, 1, 1), (3, 3, 2, 2)]
    assert all(t[1:4] == ([0, 2], [1, 3], []) for t in terms)
    want = (want_c[0] * np.einsum('aacc', blk[0:4, 0:1].reshape(2, 2, 1, 1)) + want_c[1] * np.einsum('aacc', blk[0:4, 1:5].reshape(2, 2, 2, 2))
            + want_c[2] * np.einsum('aacc', blk[4:13, 0:1].reshape(3, 3, 1, 1)) + want_c[3] * np.einsum('aacc', blk[4:13, 1:5].reshape(3, 3, 2, 2)))
    assert abs(complex(got.blocks[0][0, 0]) - want) <= 1e-13 * max(1.0, abs(want))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) move

@pytest.mark.parametrize('cplx', [False, True])
def test_move_braids_first_and_equals_the_dense_permute_then_trace(nb, rng, cplx):
    cases.check_move(nb, rng, cplx)
    assert len(nb.trace_calls) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# (d) error paths

def _forest(rng):
    c = cases.forest_case(rng, False)
    return c, [c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt']]


def test_error_a_tree_without_uncoupled_keys(nb, rng):
    at = AbelianTrees(rng, J=3, K=2)                                   # plain AbelianTrees spaces carry no ``uncoupled`` keys
    keyed = cases.DualAbelianTrees(np.random.default_rng(12345), 3, 2, [(0, 1)])
    ct, ncf = keyed.trace_table([0, 1, 2], (0,))
    at.legs = keyed.legs
    cod, dom, data = at.to_blocks(at.dense(rng), [0, 1, 2], [3, 4])
    with pytest.raises(ValueError, match='uncoupled'):
        ft.partial_trace(nb, data, cod, dom, at.space(ncf), dom, ct, None)
    assert not nb.trace_calls


def test_error_the_multiplicities_of_a_traced_pair_differ(nb, rng):
    c, args = _forest(rng)
    tree = ('c', 'old', 1, 0)
    m = c['cod'].tree_block_slice(tree)[1].multiplicities
    args[0] = cases.replace_tree(c['cod'], tree, multiplicities=(m[0], m[1], m[2] + 1))
    with pytest.raises(ValueError, match='multiplicities'):
        ft.partial_trace(nb, c['data'], *args)
    assert not nb.trace_calls


def test_error_a_new_tree_has_other_multiplicities_than_the_remaining_legs(nb, rng):
    c, args = _forest(rng)
    args[3] = cases.replace_tree(c['n_dom'], ('d', 'new', 2, 0), multiplicities=(3,))
    with pytest.raises(ValueError, match='without the traced legs'):
        ft.partial_trace(nb, c['data'], *args)


def test_error_a_new_tree_lies_in_another_coupled_sector(nb, rng):
    c, args = _forest(rng)
    table = dict(c['ct'].table)
    table[('c', 'old', 1, 0)] = (('c', 'new', 2, 0), table[('c', 'old', 1, 0)][1])     # both new trees have the multiplicity 2
    args[4] = ft.TreeTrace(c['ct'].positions, table)
    with pytest.raises(ValueError, match='another coupled sector'):
        ft.partial_trace(nb, c['data'], *args)


def test_error_a_new_tree_the_new_space_does_not_hold_and_overlapping_positions(nb, rng):
    c, args = _forest(rng)
    table = dict(c['ct'].table)
    table[('c', 'old', 1, 0)] = (('c', 'nowhere'), 1.0)
    args[4] = ft.TreeTrace(c['ct'].positions, table)
    with pytest.raises(ValueError, match='no tree'):
        ft.partial_trace(nb, c['data'], *args)
    args[4] = ft.TreeTrace((0, 1), c['ct'].table)
    with pytest.raises(ValueError, match='do not overlap'):
        ft.partial_trace(nb, c['data'], *args)
    assert not nb.trace_calls


def test_restated_trace_partial_is_the_pairwise_diagonal_sum(rng):
    a = rng.standard_normal((3, 2, 4, 2, 3))
    assert np.allclose(ref.trace_partial(a, [0, 1], [4, 3], [2]), np.einsum('abcba->c', a))
