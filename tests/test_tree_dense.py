"""Host side of to_dense_block / from_dense_block on fusion-tree tensors: the shared cases of tests/tree_dense_cases.py on a
numpy stand-in of the block backend (the record building, without a device)."""
import pytest

import tree_dense_cases as cases

CONFIG_IDS = ['-'.join(map(str, c)) for c in cases.ABELIAN_CONFIGS]


@pytest.fixture
def nb():
    return cases.NumpyDenseBackend()


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=CONFIG_IDS)
def test_abelian_trees_give_the_dense_tensor_and_come_back_exactly(nb, rng, config, cplx):
    cases.check_abelian(nb, rng, config, cplx)


@pytest.mark.parametrize('cplx_data,cplx_tables', [(False, False), (True, True), (False, True), (True, False)])
def test_random_isometric_tables_match_the_restatement_in_both_directions(nb, rng, cplx_data, cplx_tables):
    cases.check_table(nb, rng, cplx_data, cplx_tables)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_su2_to_dense_is_a_homomorphism_keeps_the_norm_and_commutes_with_dagger(nb, rng, cplx):
    cases.check_su2_homomorphism(nb, rng, cplx)


def test_su2_heisenberg_coupling_has_the_blocks_minus_three_quarters_and_one_quarter(nb):
    cases.check_su2_heisenberg(nb)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_su2_three_spins_one_half_with_a_two_tree_forest(nb, rng, cplx):
    cases.check_su2_three_spins(nb, rng, cplx)


def test_a_block_that_is_not_symmetric_raises_and_is_projected_with_tol_zero(nb):
    cases.check_projection(nb)


def test_an_absent_block_gives_written_zeros_and_discard_false_keeps_zero_blocks(nb, rng):
    cases.check_absent_block_and_discard(nb, rng)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_an_empty_domain(nb, rng, cplx):
    cases.check_empty_domain(nb, rng, cplx)


def test_seven_legs_raise(nb, rng):
    cases.check_seven_legs_raise(nb, rng)


def test_errors(nb, rng):
    cases.check_errors(nb, rng)
