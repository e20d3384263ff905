"""``cyten_amd.fusion_tree.partial_compose`` on the numpy stand-in: the loops, tables and records without a device.  The cases
and their tolerance are in tests/tree_compose_cases.py; tests/test_gpu_tree_compose.py runs the same ones through
HipBlockBackend."""
import dataclasses

import numpy as np
import pytest

import tree_compose_cases as cases
import tree_compose_ref as ref
from cyten_amd import fusion_tree as ft
from cyten_amd import krylov

CONFIG_IDS = ['-'.join(map(str, c)) for c in cases.ABELIAN_CONFIGS]


@pytest.fixture
def nb():
    return cases.NumpyComposeBackend()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees against the dense contraction

@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=CONFIG_IDS)
def test_partial_compose_of_abelian_trees_is_the_dense_contraction(nb, rng, config, kind):
    c = cases.check_abelian(nb, rng, config, kind)
    assert len(nb.compose_calls) == 1                                  # ONE tree_compose_many call for the tensor
    records = nb.compose_calls[0]
    side, n_before, n_after, n_contr, n_surv = config
    assert all(r[1] == side for r in records)
    fed = [r for r in records if r[4]]
    assert fed
    if n_contr == 1:
        assert all(len(r[4]) == 1 for r in fed)                        # splicing one leg: one old tree per new tree
    if n_before == 0:
        assert all(r[2] == 1 for r in fed)                             # inserted leg first: m0 = 1
    if n_after == 0:
        assert all(r[3] == 1 for r in fed)                             # inserted leg last: m2 = 1
    if n_surv == 0:                                                    # b's surviving side has no legs: N = 1
        assert all(r[0][1 if side == 'domain' else 0] == r[2] * r[3] for r in fed)
    assert c['insert'].leg == n_before


# ---------------------------------------------------------------------------------------------------------------------------
# (b) random tables against the restatement of the reference's loop

@pytest.mark.parametrize('cplx_a,cplx_b', [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize('side', cases.SIDES)
def test_random_tables_with_complex_amplitudes_match_the_restatement(nb, rng, side, cplx_a, cplx_b):
    """the conditions the case is meant to meet, checked for the seed in use: several old and several new trees per lookup,
    terms of different K in one strip, empty lists, a strip without a term"""
    c = cases.check_table(nb, rng, side, cplx_a, cplx_b)
    assert len(nb.compose_calls) == 1
    records = nb.compose_calls[0]
    assert any(len(set(r[4])) >= 2 for r in records)                   # terms of different K in one strip
    assert any(not r[4] and np.prod(r[0]) > 0 for r in records)        # a strip without a term
    lens = [len(lst) for lst in c['insert'].table.values()]
    assert 0 in lens and 2 in lens
    n_strips = sum(len((c['n_dom'] if side == 'domain' else c['n_cod']).tree_blocks[s]) for s in (0, 1))
    assert len(records) == n_strips                                    # every strip of every result block is a record


def test_real_data_under_real_amplitudes_stays_float64(nb, rng):
    for side in cases.SIDES:
        cases.check_table(nb, rng, side, False, False, cplx_amps=False)


def test_terms_come_in_the_loop_order_of_the_reference(rng):
    """outer tree, xb, yb, old tree, new tree: one strip fed by 2 outer trees x 2 xb x 1 yb x 2 old trees"""
    mk = ft.TreeSpace.from_multiplicities
    kept = mk([[0]], [[(2,)]], None, 1, [['kept']])
    olds = [('old', o, x, v) for o in 'pq' for x in (0, 1) for v in (0, 1)]
    old = mk([[0]], [[(1, 1, 1)] * 8], None, 3, [olds])
    new = mk([[0]], [[(1, 1, 1)]], None, 3, [['new']])
    bk, bn = mk([[0]], [[(1,), (1,)]], None, 1, [[('bk', 0), ('bk', 1)]]), mk([[0]], [[(1,)]], None, 1, [['bn']])
    table = {(o, ('bk', x)): [(('old', o, x, v), float(2 + olds.index(('old', o, x, v)))) for v in (0, 1)] for o in 'pq' for x in (0, 1)}
    table.update({(o, 'bn'): [('new', 1.0)] for o in 'pq'})
    insert = ft.TreeInsert('domain', 0, {(0,): [('p', (0,), 1, 1), ('q', (0,), 1, 1)]}, table)
    seen = []

    class Spy(cases.NumpyComposeBackend):
        def tree_compose_many(self, outputs):
            seen.extend(outputs)
            super().tree_compose_many(outputs)

    A, B = rng.standard_normal((2, 8)), rng.standard_normal((2, 1))
    ft.partial_compose(Spy(), ft.FusionTreeData([(0, 0)], [A]), kept, old, ft.FusionTreeData([(0, 0)], [B]), bk, bn, kept, new, insert)
    (dst, side, m0, m2, terms), = seen
    assert (side, m0, m2) == ('domain', 1, 1)
    assert [t[2] for t in terms] == [float(2 + n) for n in range(8)] and all(isinstance(t[2], float) for t in terms)
    assert [float(t[0][0, 0]) for t in terms] == A[0].tolist()
    assert [float(t[1][0, 0]) for t in terms] == [B[0, 0], B[0, 0], B[1, 0], B[1, 0]] * 2


# ---------------------------------------------------------------------------------------------------------------------------
# (c) SU(2)

@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('side', cases.SIDES)
def test_su2_one_leg_operator_at_the_last_leg_equals_compose_with_the_outer_of_the_identity(nb, rng, side, cplx):
    cases.check_su2_last_leg(nb, rng, side, cplx)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('side', cases.SIDES)
def test_su2_identity_on_two_spins_at_leg_one_gives_a_again_by_F_unitarity(nb, rng, side, cplx):
    c = cases.check_su2_identity(nb, rng, side, cplx)
    amps = [x for lst in c['insert'].table.values() for _, x in lst]
    assert any(abs(abs(x) - 1.0) > 1e-3 and abs(x) > 1e-3 for x in amps)           # genuine F symbols, not signs
    assert any(len(r[4]) >= 4 for r in nb.compose_calls[0])                        # 2 outer trees x 2 old trees feed one strip


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the placement of the conjugate

def test_conjugate_sits_on_the_new_amplitude_in_the_domain_and_on_the_old_one_in_the_codomain(nb):
    cases.check_conjugate_placement(nb)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) discard, empty operands, the chain step

@pytest.mark.parametrize('side', cases.SIDES)
def test_discard_false_keeps_the_zero_blocks(nb, rng, side):
    cases.check_discard_false_keeps_zero_blocks(nb, rng, side)


@pytest.mark.parametrize('side', cases.SIDES)
def test_an_empty_operand_gives_empty_data(nb, rng, side):
    cases.check_empty_operand(nb, rng, side)
    assert not nb.compose_calls


@pytest.mark.parametrize('side', cases.SIDES)
def test_chain_operator_step_equals_the_direct_call(nb, rng, side):
    cases.check_chain_step(nb, rng, side)


def test_chain_operator_refuses_a_wrong_step_tuple(nb, rng):
    c = cases.table_case(rng, 'domain', False, False)
    good = ('partial_compose', c['b'], c['b_cod'], c['b_dom'], c['n_cod'], c['n_dom'], c['insert'])
    krylov.TreeChainOperator(nb, [good], c['a_cod'], c['a_dom'])
    for bad in (good[:6], good + (1,), good[:1] + (c['b'].blocks,) + good[2:], good[:6] + (c['insert'].table,)):
        with pytest.raises(ValueError, match='partial_compose'):
            krylov.TreeChainOperator(nb, [bad], c['a_cod'], c['a_dom'])


def test_a_block_whose_sector_a_new_space_lacks_gives_no_result_block(nb, rng):
    """:2756-2768: the coupled sector must be in both new spaces"""
    c = cases.table_case(rng, 'domain', False, False)
    sp = c['n_cod']
    c['n_cod'] = ft.TreeSpace(sp.sectors[1:], sp.qdims[1:], sp.tree_blocks[1:], sp.num_legs)
    got = cases.run_compose(nb, c, discard=False)
    assert got.block_inds.tolist() == [[0, 1]]
    want = cases.run_ref(c)
    assert sorted(want) == [(0, 1)] and np.abs(got.blocks[0] - want[(0, 1)]).max() <= 1e-13 * np.abs(want[(0, 1)]).max()


# ---------------------------------------------------------------------------------------------------------------------------
# error paths

def _replace_tree(space: ft.TreeSpace, tree, **changes) -> ft.TreeSpace:
    blocks = [[dataclasses.replace(tb, **changes) if tb.tree == tree else tb for tb in tbs] for tbs in space.tree_blocks]
    return ft.TreeSpace(space.sectors, space.qdims, blocks, space.num_legs)


def _move_tree(space: ft.TreeSpace, tree) -> ft.TreeSpace:
    """the same space with `tree` taken out of its coupled sector and appended to the other one"""
    i, tb = space.tree_block_slice(tree)
    lists = [[t for t in tbs if t.tree != tree] for tbs in space.tree_blocks]
    lists[1 - i].append(tb)
    mk = ft.TreeSpace.from_multiplicities
    return mk(space.sectors, [[t.multiplicities for t in tbs] for tbs in lists], None, space.num_legs, [[t.tree for t in tbs] for tbs in lists])


@pytest.mark.parametrize('side', cases.SIDES)
def test_errors_of_the_tables_and_spaces(nb, rng, side):
    dom = side == 'domain'
    old_key, new_key = ('a_dom', 'n_dom') if dom else ('a_cod', 'n_cod')
    kept_new = 'n_cod' if dom else 'n_dom'

    def fresh():
        return cases.table_case(np.random.default_rng(7), side, False, False)

    def expect(c, match):
        with pytest.raises(ValueError, match=match):
            cases.run_compose(nb, c)
        assert not nb.compose_calls                                    # refused before anything is computed

    # a missing table entry
    c = fresh()
    table = dict(c['insert'].table)
    del table[(('o', 0, 0), ('bk', 0, 0))]
    expect(dict(c, insert=c['insert']._replace(table=table)), 'no entry')
    # a tree the old / the new space does not hold
    for tag, word in (('bk', 'of a has no tree'), ('bn', 'new .* has no tree')):
        c = fresh()
        table = dict(c['insert'].table)
        table[(('o', 0, 0), (tag, 0, 0))] = [(('nowhere',), 1.0)]
        expect(dict(c, insert=c['insert']._replace(table=table)), word)
    # an old tree block whose size is not m_before K m_after, a new one whose size is not m_before N m_after
    c = fresh()
    expect(dict(c, **{old_key: _replace_tree(c[old_key], ('old', ('o', 0, 0), 0, 0), stop=c[old_key].tree_block_slice(('old', ('o', 0, 0), 0, 0))[1].stop - 1)}),
           'old tree .* has the size')
    c = fresh()
    expect(dict(c, **{new_key: _replace_tree(c[new_key], ('new', ('o', 0, 0), 0, 0), stop=c[new_key].tree_block_slice(('new', ('o', 0, 0), 0, 0))[1].stop - 1)}),
           'new tree .* has the size')
    # an outer tree whose b-sector has no block in b (:2775)
    c = fresh()
    expect(dict(c, b=ft.FusionTreeData(c['b'].block_inds[:1], c['b'].blocks[:1])), 'b has no block')
    # a new tree in a coupled sector other than the block's
    c = fresh()
    expect(dict(c, **{new_key: _move_tree(c[new_key], ('new', ('o', 0, 0), 0, 0))}), 'new tree .* lies in the coupled sector')
    # a result block whose untouched side differs in size from a's block
    c = fresh()
    sp = c[kept_new]
    grown = ft.TreeSpace.from_multiplicities(sp.sectors, [[(4,)], [(2,)]], None, 1, [[('kept', 0)], [('kept', 1)]])
    expect(dict(c, **{kept_new: grown}), 'keeps its space')
    # an unknown side
    c = fresh()
    expect(dict(c, insert=c['insert']._replace(side='both')), "'codomain' or 'domain'")


def test_restatement_of_one_tree_is_the_matrix_product(rng):
    mk = ft.TreeSpace.from_multiplicities
    kept, old, new = mk([[0]], [[(2,)]], None, 1, [['kept']]), mk([[0]], [[(2, 3, 2)]], None, 3, [['old']]), mk([[0]], [[(2, 4, 2)]], None, 3, [['new']])
    bk, bn = mk([[0]], [[(3,)]], None, 1, [['bk']]), mk([[0]], [[(4,)]], None, 1, [['bn']])
    A, B = rng.standard_normal((2, 12)), rng.standard_normal((3, 4))
    insert = ft.TreeInsert('domain', 1, {(0,): [('o', (0,), 2, 2)]}, {('o', 'bk'): [('old', 1.0)], ('o', 'bn'): [('new', 1.0)]})
    got = ref.partial_compose_ref(ft.FusionTreeData([(0, 0)], [A]), kept, old, ft.FusionTreeData([(0, 0)], [B]), bk, bn, kept, new, insert)
    assert np.allclose(got[(0, 0)], np.einsum('rikj,kn->rinj', A.reshape(2, 2, 3, 2), B).reshape(2, 16), rtol=0, atol=1e-14)
    count = ref.partial_compose_ref(ft.FusionTreeData([(0, 0)], [A]), kept, old, ft.FusionTreeData([(0, 0)], [B]), bk, bn, kept, new, insert, count=True)
    assert np.all(count[(0, 0)] == 3)
