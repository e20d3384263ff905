"""Host logic of the functions of a square tensor in cyten_amd.abelian -- act_block_diagonal_square_matrix, exp, eye,
hermitian_function -- on the numpy stand-in (tests/tensor_function_ref.py), against the dense matrix of the tensor; and the
error of the device's exponential algorithm itself, restated in numpy, against scipy.linalg.expm."""
import numpy as np
import pytest
import scipy.linalg

import tensor_function_ref as ref
from cyten_amd import abelian as ab
from tensor_function_cases import CASE_IDS, cases

CASES = cases()
ALL_CASES = pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
NP = ref.NumpyExpmBackend()


def _tensor(case, bb=NP):
    t = ab.AbelianTensor.from_spec(bb, case['tensor'])
    t.labels = [f'l{i}' for i in range(t.nlegs)]
    return t


def _close(got, want, tol=1e-12):
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= tol * max(np.abs(want).max(), 1e-300)


def _hermitian(bb, t):
    return ab.linear_combination(bb, 0.5, t, 0.5, ab.dagger(bb, t))


@pytest.mark.parametrize('factor', [1.0, -0.7, 0.3 - 0.4j], ids=['one', 'real', 'complex'])
@ALL_CASES
def test_exp_dense(case, factor):
    """exp(factor t) is scipy's expm of the d x d matrix of the dense tensor"""
    c = CASES[case]
    t = _tensor(c)
    got = ab.exp(NP, t, factor)
    want = ref.dense_exp(t.to_dense(NP), factor)
    _close(got.to_dense(NP), want)
    assert got.labels == t.labels and got.num_codomain == t.num_codomain
    assert all(x is y for x, y in zip(got.legs, t.legs))
    if isinstance(factor, complex):
        assert all(np.iscomplexobj(b) for b in got.blocks)
    got.check_charges()


@ALL_CASES
def test_exp_without_matrix_exp_many(case):
    """a backend without matrix_exp_many: the loop over matrix_exp gives the same tensor"""
    c = CASES[case]
    loop = ref.NumpyLoopBackend()
    t = _tensor(c, loop)
    _close(ab.exp(loop, t, -0.7).to_dense(loop), ref.dense_exp(t.to_dense(loop), -0.7))


def test_act_block_diagonal_structure():
    c = CASES[CASE_IDS.index('u1u1-r2-missing')]
    t = _tensor(c)
    leg = t.legs[0]
    assert len(t.blocks) < leg.nsec
    seen = []

    def method(entries):
        seen.append(list(entries))
        return NP.matrix_exp_many(entries)
    got = ab.act_block_diagonal_square_matrix(NP, t, method)
    assert len(seen) == 1 and len(seen[0]) == leg.nsec          # the whole list, once
    assert got.block_inds.tolist() == [[j, j] for j in range(leg.nsec)]
    have = set(t.block_inds[:, 0].tolist())
    for j, (e, b) in enumerate(zip(seen[0], got.blocks)):
        if j in have:
            assert isinstance(e, np.ndarray)
        else:
            assert e == (int(leg.mults[j]), None)
            assert np.array_equal(b, np.eye(int(leg.mults[j])))   # a missing sector is an identity block
    with pytest.raises(ValueError):
        ab.act_block_diagonal_square_matrix(NP, _tensor(CASES[CASE_IDS.index('u1-r4')]), method)
    with pytest.raises(ValueError):
        ab.act_block_diagonal_square_matrix(NP, t, lambda entries: [])


@ALL_CASES
def test_eye(case):
    c = CASES[case]
    t = _tensor(c)
    k = c['k']
    e = ab.eye(NP, t.symmetry, t.legs[:k])
    assert e.num_codomain == k and e.nlegs == 2 * k
    for x, y in zip(e.legs, t.legs):
        assert x.sign == y.sign and np.array_equal(x.sectors, y.sectors) and np.array_equal(x.mults, y.mults)
    d = int(np.prod([l.dim for l in t.legs[:k]]))
    want = ref.from_matrix(np.eye(d), *ref.as_matrix(t.to_dense(NP), k)[1:])
    assert np.array_equal(e.to_dense(NP), want)
    e.check_charges()
    assert ab.eye(NP, t.symmetry, t.legs[:k], dtype='complex128').blocks[0].dtype == np.complex128


def test_exp_of_the_empty_tensor_is_eye():
    c = CASES[CASE_IDS.index('u1-r4-empty')]
    t = _tensor(c)
    assert len(t.blocks) == 0
    got = ab.exp(NP, t, 2.5)
    assert np.array_equal(got.to_dense(NP), ab.eye(NP, t.symmetry, t.legs[:c['k']]).to_dense(NP))


def test_leg_requirements():
    t = _tensor(CASES[CASE_IDS.index('u1-r4')])
    odd = ab.AbelianTensor(t.symmetry, t.legs[:3], [], np.zeros((0, 3), np.int64), 2)
    swapped = ab.permute_legs(NP, t, [0, 1, 3, 2])          # pairs (0, 2) and (1, 3): not the pairing of compose
    same_sign = ab.AbelianTensor(t.symmetry, [t.legs[0], t.legs[0]], [], np.zeros((0, 2), np.int64), 1)
    for fn in (lambda x: ab.exp(NP, x), lambda x: ab.hermitian_function(NP, x, 'exp')):
        with pytest.raises(ValueError):
            fn(odd)
        with pytest.raises(ValueError):
            fn(same_sign)
        if not all(swapped.legs[3 - i].can_contract_with(swapped.legs[i]) for i in range(2)):
            with pytest.raises(ValueError):
                fn(swapped)
    with pytest.raises(ValueError):
        ab.hermitian_function(NP, t, 'cosh')
    with pytest.raises(ValueError):
        ab.eye(NP, t.symmetry, [])


@pytest.mark.parametrize('func,param', [('exp', None), ('square', None), ('abs', None), ('pow', 3.0), ('cutoff_inverse', 0.05)])
@ALL_CASES
def test_hermitian_function_dense(case, func, param):
    """V f(w) V^dagger of the dense matrix; f(0) != 0 fills the missing sectors, the others leave them out"""
    c = CASES[case]
    h = _hermitian(NP, _tensor(c))
    h.labels = [f'l{i}' for i in range(h.nlegs)]
    f = {'exp': np.exp, 'square': np.square, 'abs': np.abs, 'pow': lambda w: w ** 3.0,
         'cutoff_inverse': lambda w: np.where(np.abs(w) < 0.05, 0.0, 1.0 / np.where(w == 0, 1.0, w))}[func]
    got = ab.hermitian_function(NP, h, func, param)
    want = ref.dense_hermitian_function(h.to_dense(NP), f)
    _close(got.to_dense(NP), want, 1e-10)
    assert got.labels == h.labels and got.num_codomain == h.num_codomain
    if c['missing'] and c['k'] == 1:
        assert len(got.blocks) == (h.legs[0].nsec if func == 'exp' else len(h.blocks))


@ALL_CASES
def test_sqrt_of_a_positive_tensor(case):
    c = CASES[case]
    h = _hermitian(NP, _tensor(c))
    pos = ab.exp(NP, h)                       # positive definite on every sector, missing ones included
    r = ab.hermitian_function(NP, pos, 'sqrt')
    _close(ab.compose(NP, r, r, c['k']).to_dense(NP), pos.to_dense(NP), 1e-11)
    _close(ab.hermitian_function(NP, pos, 'log').to_dense(NP), h.to_dense(NP) if len(h.blocks) else 0 * pos.to_dense(NP), 1e-10)


# ------------------------------------------------------------------------------------------- the algorithm's own error

@pytest.mark.parametrize('n', [1, 2, 7, 33, 64, 97, 150])
def test_taylor18_against_scipy(n):
    """Scaling by 2^-s, the degree-18 Taylor polynomial (truncation < 2e-23 for ||M||_1 <= 1/2) and s squarings, in numpy
    float64, against scipy.linalg.expm for the families of the device tolerance, ||A||_1 <= 64.  The bound is the project's
    line for this operation (tests/test_gpu_api_surface.py::test_matrix_exp): max|got - want| <= 1e-10 max|want|; the
    figures are printed (observed: four orders below it)."""
    rng = np.random.default_rng(100 + n)
    for name, a in ref.families(rng, n):
        want = scipy.linalg.expm(a)
        got = ref.expm_taylor18(a)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f'n={n} {name}: ||A||_1={np.abs(a).sum(axis=0).max():.3g} rel err {err:.2e}')
        assert err <= 1e-10, (name, err)


def test_squarings():
    assert [ref.squarings(x) for x in (0.0, 0.5, 0.500001, 1.0, 1.5, 2.0, 64.0, 64.1)] == [0, 0, 1, 1, 2, 2, 7, 8]
