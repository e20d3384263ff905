"""The cases and the cap of tests/decomp_accuracy_cases.py, without a GPU: LAPACK meets the cap on every case with a factor 8 to
spare, the measures see the defects they are meant to see (each mutant of a LAPACK result fails the cap), and the builders of
the exact family refuse what would not be exact."""
import numpy as np
import pytest
import scipy.linalg

import decomp_accuracy_cases as dac
from decomp_accuracy_cases import CAP_EPS, AccuracyError


def _lapack_svd(a):
    return np.linalg.svd(a, full_matrices=False)


@pytest.fixture(scope='module')
def cases():
    return dac.all_cases()


def test_long_double_is_the_x87_format():
    assert np.finfo(np.longdouble).eps <= 1.1e-19


def test_lapack_stays_within_an_eighth_of_the_cap(cases):
    """Every case of the module through np.linalg.svd / scipy.linalg.qr (economic and full) / np.linalg.eigh: every measure
    <= CAP / 8.  Prints the worst of each measure per kind: the LAPACK column of the table in DESIGN.md."""
    worst = {}
    for kind, c in cases:
        if kind == 'svd':
            runs = [dac.check_svd(c, *_lapack_svd(c.a), cap_eps=CAP_EPS / 8)]
        elif kind == 'eigh':
            runs = [dac.check_eigh(c, *np.linalg.eigh(c.a), cap_eps=CAP_EPS / 8)]
        else:
            runs = [dac.check_qr(c, *scipy.linalg.qr(c.a, mode=mode), full=mode == 'full', cap_eps=CAP_EPS / 8)
                    for mode in ('economic', 'full')]
        for ms in runs:
            print(dac.table_line('LAPACK ' + kind, c, ms))
            key = (kind, 'complex' if np.iscomplexobj(c.a) else 'real', c.origin)
            for k, v in ms.items():
                worst.setdefault(key, {})[k] = max(worst.get(key, {}).get(k, 0.0), v)
    for key, ms in sorted(worst.items()):
        print('[accuracy] worst of LAPACK', *key, dac.format_measures(ms))
    kinds = {k for k, _ in cases}
    assert kinds == {'svd', 'eigh', 'qr'}
    assert {c.origin for _, c in cases} == {'exact', 'mpmath', 'dense'}


def test_every_reference_value_set_is_sorted_and_complete(cases):
    for kind, c in cases:
        if c.ref is None:
            assert c.origin == 'dense'
            continue
        assert c.ref.dtype == np.longdouble and c.ref.shape == (min(c.shape),)
        assert np.all(np.diff(c.ref) <= 0) if kind != 'eigh' else np.all(np.diff(c.ref) >= 0)
        if c.origin == 'exact':
            assert np.count_nonzero(c.ref) == c.rank


# ---- mutants: each starts from a LAPACK result that passes and must fail the cap
@pytest.fixture(scope='module')
def full_case():
    c = dac.mp_svd_case(33, 33)
    return c, _lapack_svd(c.a)


@pytest.fixture(scope='module')
def deficient_case():
    c = dac.exact_svd_case('exact rank 32 128x64', 128, 64, dac.d_graded(64, 32))
    return c, _lapack_svd(c.a)


def test_mutant_column_of_u_leaning_on_another(full_case):
    c, (U, S, Vh) = full_case
    dac.check_svd(c, U, S, Vh)
    U = U.copy()
    U[:, 5] += 1e-12 * U[:, 2]
    ms = dac.svd_measures(c, U, S, Vh)
    assert 0.9e-12 <= ms['orth_u'] * dac.EPS <= 1.1e-12
    with pytest.raises(AccuracyError, match='orth_u'):
        dac.check_svd(c, U, S, Vh)


def test_mutant_one_singular_value_moved(full_case):
    c, (U, S, Vh) = full_case
    S = S.copy()
    S[0] += 1e-12 * S[0]
    ms = dac.svd_measures(c, U, S, Vh)
    assert 4400 < ms['values'] < 4600 and ms['orth_u'] < CAP_EPS / 8 and ms['orth_v'] < CAP_EPS / 8
    with pytest.raises(AccuracyError, match='values'):
        dac.check_svd(c, U, S, Vh)


def test_mutant_two_adjacent_values_swapped(full_case):
    c, (U, S, Vh) = full_case
    S = S.copy()
    assert S[10] != S[11]
    S[[10, 11]] = S[[11, 10]]
    with pytest.raises(AccuracyError, match='not descending'):
        dac.check_svd(c, U, S, Vh)
    W, V = np.linalg.eigh(dac.mp_eigh_case(9).a)
    dac.check_eigh(dac.mp_eigh_case(9), W, V)
    W[[3, 4]] = W[[4, 3]]
    with pytest.raises(AccuracyError, match='not ascending'):
        dac.check_eigh(dac.mp_eigh_case(9), W, V)


def test_mutant_entry_below_the_diagonal_of_r():
    c = dac.gaussian(20, 20, 61)
    Q, R = scipy.linalg.qr(c.a, mode='economic')
    dac.check_qr(c, Q, R)
    R[7, 3] = 1e-300
    with pytest.raises(AccuracyError, match='below its diagonal'):
        dac.check_qr(c, Q, R)
    sgn = np.where(np.diagonal(R) < 0, -1.0, 1.0)
    Q, R = Q * sgn, sgn[:, None] * np.triu(R)
    dac.check_qr(c, Q, R, positive_diagonal=True)
    R[4] *= -1
    Q[:, 4] *= -1
    with pytest.raises(AccuracyError, match='non-negative'):
        dac.check_qr(c, Q, R, positive_diagonal=True)


def test_mutant_null_vector_tilted_towards_the_range(deficient_case):
    """A null vector of a rank-deficient block that leans 1e-12 on a range vector: the reconstruction does not see it (its
    singular value is zero), the values do not see it, orthogonality does."""
    c, (U, S, Vh) = deficient_case
    dac.check_svd(c, U, S, Vh)
    assert c.rank == 32 and S[c.rank] <= 1e-13 * S[0]
    U = U.copy()
    U[:, c.rank + 3] += 1e-12 * U[:, 0]
    ms = dac.svd_measures(c, U, S, Vh)
    assert ms['resid'] <= CAP_EPS / 8 and ms['values'] <= CAP_EPS / 8 and ms['orth_u'] > 2 * CAP_EPS
    with pytest.raises(AccuracyError, match='orth_u'):
        dac.check_svd(c, U, S, Vh)


def test_nan_fails_the_cap(full_case):
    c, (U, S, Vh) = full_case
    U = U.copy()
    U[3, 3] = np.nan
    with pytest.raises(AccuracyError):
        dac.check_svd(c, U, S, Vh)


# ---- builders
@pytest.mark.parametrize('d', [[3.0], [2.0 ** -31], [0.75], [2.0], [-1.0], [1.0] * 9])
def test_exact_builder_refuses_what_is_not_exact(d):
    with pytest.raises(ValueError):
        dac.exact_svd_case('bad', 16, 8, d)


def test_exact_builder_refuses_large_extents_and_accepts_the_edges():
    with pytest.raises(ValueError):
        dac.exact_svd_case('bad', 4096, 8, [1.0])
    with pytest.raises(ValueError):
        dac.exact_eigh_case('bad', 16, [0.3])
    c = dac.exact_svd_case('edge', 2048, 2048, np.r_[2.0 ** -np.arange(31.0), 0.0])
    assert c.rank == 31 and c.ref[0] == 2048 and c.ref[30] == 2048 * 2.0 ** -30 and c.ref[31] == 0
    assert dac.exact_eigh_case('signed', 16, [-1.0, 0.5]).ref.tolist() == [-16.0] + [0.0] * 14 + [8.0]


def test_exact_vectors_are_singular_vectors():
    """The Hadamard columns the builder hands out are singular vectors of the block it built: A v_i = sigma_i u_i in long
    double, permuted, bordered and complex forms included."""
    for c in (dac.exact_svd_case('a', 64, 32, dac.d_graded(32, 20)),
              dac.exact_svd_case('b', 64, 64, dac.d_cluster(64, 40), shape=(90, 70), cplx=True, seed=4)):
        a, u, v = dac._ld(c.a), c.u, c.v
        assert u.shape == (c.shape[0], c.rank) and v.shape == (c.shape[1], c.rank)
        assert np.abs(a @ v - u * c.ref[:c.rank]).max() <= 1e-18 * c.ref[0]
        assert np.abs(u.conj().T @ u - np.eye(c.rank)).max() <= 1e-18 and np.abs(v.conj().T @ v - np.eye(c.rank)).max() <= 1e-18


def test_mpmath_and_exact_references_agree():
    import mpmath
    d = 2.0 ** -np.arange(8.0)
    for cplx in (False, True):
        c = dac.exact_svd_case('both', 16, 8, d, cplx=cplx, seed=9)
        got = dac.mp_singular_values(c.a)
        want = [mpmath.sqrt(128) * mpmath.mpf(float(x)) for x in d]
        assert max(abs(g - w) for g, w in zip(got, want)) <= mpmath.mpf('1e-25') * want[0]
        assert np.abs(dac._to_ld(got) - c.ref).max() <= 2e-19 * c.ref[0]
    h = dac.exact_eigh_case('both', 16, [1.0, -1.0, 0.5, -0.25], cplx=True, seed=9)
    got = dac.mp_eigenvalues(h.a)
    want = sorted([16, -16, 8, -4] + [0] * 12)
    assert max(abs(g - w) for g, w in zip(got, want)) <= mpmath.mpf('1e-25') * 16


def test_split_product_agrees_with_the_long_double_loop():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((150, 300)), rng.standard_normal((300, 90)) * 1e-3
    ref = dac._ld(x) @ dac._ld(y)
    assert np.abs(dac._matmul_ld_split(x, y) - ref).max() <= 1e-18 * np.abs(ref).max()
    q, _ = np.linalg.qr(rng.standard_normal((200, 200)))
    g = dac._matmul_ld_split(np.ascontiguousarray(q.T), q)
    assert np.abs(g - dac._ld(q.T) @ dac._ld(q)).max() <= 2e-18      # (the loop's own error: 200 terms at 5e-20; 0.01 eps)
