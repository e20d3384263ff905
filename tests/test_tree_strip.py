"""Host side of the factorized tree moves: ``fusion_tree.transform_tensor_factorized`` and the 'transform_factorized' step of
``krylov.TreeChainOperator`` on the numpy stand-in -- the record building without a device.  The cases, their inputs and their
criteria are those of tests/tree_strip_cases.py; tests/test_gpu_tree_strip.py runs the same through HipBlockBackend."""
import pytest

import tree_strip_cases as cases


@pytest.fixture
def nb():
    return cases.NumpyStripBackend()


@pytest.mark.parametrize('real', [False, True], ids=['complex', 'real'])
@pytest.mark.parametrize('case', cases.STRIP_CASES, ids=[c['name'] for c in cases.STRIP_CASES])
def test_golden_strips_reproduce_the_reference_expectation(nb, rng, case, real):
    cases.check_golden(nb, rng, case, real)


def test_the_golden_file_holds_the_eight_strip_cases():
    assert len(cases.STRIP_CASES) == 8 and sorted({c['axis'] for c in cases.STRIP_CASES}) == [0, 1]


@pytest.mark.parametrize('kind', cases.KINDS, ids=lambda k: ('c' if k[0] else 'r') + 'data-' + ('c' if k[1] else 'r') + 'map')
@pytest.mark.parametrize('cod_perm', cases.COD_PERMS, ids=lambda p: ''.join(map(str, p)))
@pytest.mark.parametrize('sides', cases.SIDES)
def test_exact_data_equals_the_pair_route_and_the_restatement(nb, rng, sides, cod_perm, kind):
    cases.check_exact(nb, rng, sides, cod_perm, *kind)


@pytest.mark.parametrize('kind', cases.KINDS, ids=lambda k: ('c' if k[0] else 'r') + 'data-' + ('c' if k[1] else 'r') + 'map')
@pytest.mark.parametrize('sides', cases.SIDES)
def test_rounded_data_is_within_the_derived_bound_of_the_wide_evaluation(nb, rng, sides, kind):
    cases.check_rounded(nb, rng, sides, cases.COD_PERMS[2], *kind)


def test_real_data_stays_float64_and_is_read_in_place_under_a_complex_map(nb, rng):
    cases.check_dtypes(nb, rng)


def test_an_identity_side_is_no_launch(nb, rng):
    cases.check_identities(nb, rng)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_a_braid_and_its_inverse_give_the_input_back(nb, rng, cplx):
    cases.check_round_trip(nb, rng, cplx)


def test_every_error_path(nb, rng):
    cases.check_errors(nb, rng)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_chain_operator_step_is_the_direct_call(nb, rng, cplx):
    cases.check_chain_step(nb, rng, cplx)
