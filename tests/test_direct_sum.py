"""Direct sums as Krylov vectors on the CPU (cyten_amd.direct_sum, the wrappers and gram_schmidt of cyten_amd.sparse, the
solvers of cyten_amd.krylov on ``_DirectSumOps``): the host logic on a numpy stand-in against the block-diagonal dense
matrix of tests/direct_sum_cases.py.  The expectations of the reference's tests/python_tests/test_direct_sum.py and, for the
solvers, the criteria of tests/test_tree_krylov.py with their tolerances."""
import numpy as np
import pytest

import direct_sum_cases as dc
from cyten_amd import abelian as ab
from cyten_amd import direct_sum as ds
from cyten_amd import krylov, sparse
from cyten_amd.direct_sum import DirectSum

ALL = list(dc.COMBOS)


@pytest.fixture
def nbb():
    return dc.NumpyDirectSumBackend()


# ---------------------------------------------------------------------------------------------------------------------------
# construction and algebra

def test_construction_errors_and_indexing(nbb):
    case = dc.SumCase(nbb, 'abelian+tree')
    x1, x2 = case.psi0.components
    with pytest.raises(ValueError):
        DirectSum([])
    with pytest.raises(ValueError):
        DirectSum([x1, None])
    with pytest.raises(ValueError):
        DirectSum([x1, DirectSum([x2])])
    x = DirectSum([x1, x2])
    assert len(x) == 2 and isinstance(x.components, tuple)
    assert x[0] is x1 and x[1] is x2 and x[-1] is x2 and x[-2] is x1
    for i in (2, -3):
        with pytest.raises(IndexError):
            x[i]
    assert not x.is_complex()
    assert dc.SumCase(nbb, 'abelian+tree', cplx_vec=[False, True]).psi0.is_complex()


@pytest.mark.parametrize('combo', ALL)
def test_compatible_both_ways(nbb, combo):
    case = dc.SumCase(nbb, combo)
    x = case.psi0
    t = x[0]
    assert ds.compatible(x, ds.scale(nbb, 1.0, x))
    assert not ds.compatible(t, x) and not ds.compatible(x, t)
    assert not ds.compatible(x, DirectSum([t]))
    # (the two tree parts live on the same spaces: swapping them changes nothing)
    assert ds.compatible(x, DirectSum([x[1], x[0]])) == (combo == 'tree+tree')
    # the solvers' and the wrappers' notion is the same one
    assert krylov.compatible(x, x) and not krylov.compatible(t, x) and not krylov.compatible(x, t) and krylov.compatible(t, t)
    assert sparse._compatible(x, x) and not sparse._compatible(t, x) and not sparse._compatible(x, t)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('combo', ALL)
def test_algebra_against_the_componentwise_formulas(nbb, combo, cplx, tol=1e-12):
    cx, cy = dc.SumCase(nbb, combo, 1, cplx_vec=cplx), dc.SumCase(nbb, combo, 2, cplx_vec=cplx)
    x, y = cx.psi0, cy.psi0
    y1x, y1y = cx.y0, cx.y(y)
    inner_expect = sum(ds._inner1(nbb, a, b) for a, b in zip(x.components, y.components))
    assert abs(ds.inner(nbb, x, y) - inner_expect) < tol * (abs(inner_expect) + 1.0)
    assert abs(ds.inner(nbb, x, y) - np.vdot(y1x, y1y)) < tol * (abs(inner_expect) + 1.0)
    n2_expect = sum(ds._norm1(nbb, c) ** 2 for c in x.components)
    assert abs(ds.norm(nbb, x) ** 2 - n2_expect) < tol * (n2_expect + 1.0)
    assert abs(ds.norm(nbb, x) - np.linalg.norm(y1x)) < tol * (np.linalg.norm(y1x) + 1.0)
    a = 2.5 - 0.3j
    scaled = ds.scale(nbb, a, x)
    assert isinstance(scaled, DirectSum) and np.allclose(cx.y(scaled), a * y1x, rtol=0, atol=tol * np.abs(y1x).max() * 3)
    axpy = ds.axpy(nbb, a, x, y)
    assert isinstance(axpy, DirectSum) and np.allclose(cx.y(axpy), a * y1x + y1y, rtol=0, atol=tol * 10)
    lc = ds.linear_combination(nbb, 1.0, x, a, y)
    assert isinstance(lc, DirectSum) and np.allclose(cx.y(lc), y1x + a * y1y, rtol=0, atol=tol * 10)
    assert ds.almost_equal(nbb, lc, ds.axpy(nbb, a, y, x), 1e-12, 1e-12)
    assert not ds.almost_equal(nbb, lc, axpy, 1e-5, 1e-8)
    for i in range(2):
        assert ds.almost_equal(nbb, DirectSum([scaled[i]]), DirectSum([ds._scale1(nbb, a, x[i])]), 0.0, 0.0)


def test_size_mismatches_name_the_operation(nbb):
    x = dc.SumCase(nbb, 'abelian+tree').psi0
    short = DirectSum([x[0]])
    for name, call in (('inner', lambda: ds.inner(nbb, x, short)), ('axpy', lambda: ds.axpy(nbb, 1.0, x, short)),
                       ('linear_combination', lambda: ds.linear_combination(nbb, 1.0, short, 1.0, x)),
                       ('almost_equal', lambda: ds.almost_equal(nbb, x, short)), ('inner', lambda: ds.inner(nbb, x, x[0]))):
        with pytest.raises(ValueError, match=name):
            call()


# ---------------------------------------------------------------------------------------------------------------------------
# wrappers

@pytest.mark.parametrize('combo', ALL)
def test_wrappers(nbb, combo):
    case = dc.SumCase(nbb, combo, 3)
    H, psi = case.H, case.psi0
    got = H.matvec(psi)
    assert isinstance(got, DirectSum)
    for i, p in enumerate(case.parts):
        assert np.array_equal(p.y(got[i]), p.y(p.H.matvec(psi[i])))
    scale = np.linalg.norm(case.M @ case.y0)
    assert np.linalg.norm(case.y(got) - case.M @ case.y0) <= 1e-12 * scale
    got_s = sparse.ShiftedLinearOperator(H, 1.5).matvec(psi)
    assert isinstance(got_s, DirectSum) and np.linalg.norm(case.y(got_s) - (case.M @ case.y0 + 1.5 * case.y0)) <= 1e-12 * scale
    got_sum = sparse.SumLinearOperator(H, [H]).matvec(psi)
    assert np.linalg.norm(case.y(got_sum) - 2 * case.M @ case.y0) <= 2e-12 * scale
    q0 = sparse.gram_schmidt(nbb, [psi])[0]
    res = sparse.ProjectedLinearOperator(H, [q0], project_operator=True, penalty=None).matvec(q0)
    assert ds.norm(nbb, res) < 1e-8 * (ds.norm(nbb, q0) + 1.0)
    with pytest.raises(NotImplementedError):
        H.to_tensor()
    assert H.is_complex is False and dc.SumCase(nbb, combo, 3, cplx_op=True).H.is_complex is True
    with pytest.raises(ValueError):
        H.matvec(psi[0])
    with pytest.raises(ValueError):
        H.matvec(DirectSum([psi[0]]))
    with pytest.raises(ValueError):
        sparse.DirectSumLinearOperator([])
    with pytest.raises(ValueError):
        sparse.ProjectedLinearOperator(H, [psi, psi[0]])


def test_adjoints_are_componentwise(nbb):
    case = dc.SumCase(nbb, (('ab2', 2.0), ('ab1', -5.5)), 4, cplx_op=True, cplx_vec=True)
    adj = case.H.adjoint()
    assert isinstance(adj, sparse.DirectSumLinearOperator) and len(adj.operators) == 2
    got = case.y(adj.matvec(case.psi0))
    want = case.M.conj().T @ case.y0
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)


def test_tensor_linear_operator(nbb, rng):
    part = dc.Ab1Part(nbb, rng, True, True, -5.5)
    op = part.H
    T = op.tensor
    assert op.which_leg == 1 and op.other_leg == 0 and op.is_complex
    assert np.linalg.norm(part.y(op.matvec(part.psi0)) - part.M @ part.y0) <= 1e-13 * np.linalg.norm(part.M @ part.y0)
    assert op.to_tensor() is T
    # leg 0 as the contracted one: the transposed matrix, and to_tensor puts the contracted leg last
    op0 = sparse.TensorLinearOperator(nbb, T, 0)
    v = ab.AbelianTensor.from_numpy_blocks(nbb, dc.U1, [dc.LEG_C.dual()], [part.x0[0]], [[0]], 1)
    got = np.asarray(op0.matvec(v).blocks[0])
    assert np.linalg.norm(got - part.M.T @ part.y0) <= 1e-13 * np.linalg.norm(part.M @ part.y0)
    assert [l.sign for l in op0.to_tensor().legs] == [-1, +1]
    adj = op.adjoint()
    assert np.linalg.norm(part.y(adj.matvec(part.psi0)) - part.M.conj().T @ part.y0) <= 1e-13 * np.linalg.norm(part.y0) * 6
    with pytest.raises(ValueError, match='two-leg'):
        sparse.TensorLinearOperator(nbb, part.psi0)
    two = dc.Ab2Part(nbb, rng, False, False, 2.0)
    with pytest.raises(ValueError, match='contractible'):
        sparse.TensorLinearOperator(nbb, two.psi0)
    with pytest.raises(ValueError):
        op.matvec(two.psi0)
    with pytest.raises(ValueError):
        op.matvec(DirectSum([part.psi0]))


# ---------------------------------------------------------------------------------------------------------------------------
# gram_schmidt

def _gram(bb, vecs):
    return np.array([[ds.inner(bb, v, w) for w in vecs] for v in vecs])


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('combo', ALL)
def test_gram_schmidt_orthonormalises_and_drops_a_duplicate(nbb, combo, cplx):
    vecs = [dc.SumCase(nbb, combo, 10 + k, cplx_vec=cplx).psi0 for k in range(4)]
    out = sparse.gram_schmidt(nbb, vecs)
    assert len(out) == 4 and all(isinstance(v, DirectSum) for v in out)
    assert np.abs(_gram(nbb, out) - np.eye(4)).max() < 1e-12
    dup = [vecs[0], vecs[1], vecs[0], vecs[2]]
    out = sparse.gram_schmidt(nbb, dup, rcond=1e-10)
    assert len(out) == 3
    assert np.abs(_gram(nbb, out) - np.eye(3)).max() < 1e-12
    # the span: the input vectors lie in it
    case = dc.SumCase(nbb, combo, 10)
    Q = np.array([case.y(v) for v in out])
    for v in dup:
        y = case.y(v)
        assert np.linalg.norm(y - Q.T @ (Q.conj() @ y)) <= 1e-12 * np.linalg.norm(y)
    with pytest.raises(ValueError):
        sparse.gram_schmidt(nbb, [vecs[0], vecs[0][0]])
    assert sparse.gram_schmidt(nbb, []) == []


def test_gram_schmidt_threshold_is_strict_and_absolute(nbb):
    v = dc.three_four(nbb)
    assert ds.norm(nbb, v) == 5.0
    assert sparse.gram_schmidt(nbb, [v], rcond=5.0) == []
    kept = sparse.gram_schmidt(nbb, [v], rcond=np.nextafter(5.0, 0.0))
    assert len(kept) == 1 and abs(ds.norm(nbb, kept[0]) - 1.0) < 1e-15
    # single tensors and tree tensors go the same way
    t = dc.SumCase(nbb, 'abelian+tree').psi0
    for single in t.components:
        q = sparse.gram_schmidt(nbb, [single, single], rcond=1e-10)
        assert len(q) == 1 and abs(ds.norm(nbb, DirectSum(q)) - 1.0) < 1e-14
    bad = ds.scale(nbb, np.nan, v)
    assert sparse.gram_schmidt(nbb, [bad]) == []


# ---------------------------------------------------------------------------------------------------------------------------
# solvers (the test functions of tests/test_tree_krylov.py, test_krylov_evolution.py and test_krylov_gmres.py)

@pytest.mark.parametrize('cplx_op,cplx_vec', [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize('combo', ALL)
def test_lanczos_ground_state_and_tridiagonal_matrix(nbb, combo, cplx_op, cplx_vec):
    case = dc.SumCase(nbb, combo, 0, cplx_op, cplx_vec)
    solver, E0, psi, N = dc.check_ground_state(case, dict(N_max=40))
    assert type(solver.V) is krylov._DirectSumOps and 2 < N <= 40 and isinstance(psi, DirectSum)
    # the minimum pin: a generic start finds the lower of the two ground energies
    assert abs(E0 - min(p.E0 for p in case.parts)) < 1e-9 * abs(E0)
    for p in case.parts:
        assert abs(np.linalg.eigvalsh(p.M)[0] - p.E0) < 1e-12 * abs(p.E0)


@pytest.mark.parametrize('combo', ALL)
def test_lanczos_leaves_a_zero_component_zero(nbb, combo):
    """the invariance pin: H1 (+) H2 never couples the components, so a start vector without a first component finds the
    ground state of H2 alone and its first component stays exactly zero"""
    case = dc.SumCase(nbb, combo, 1)
    # the part with the LOWER ground energy is the one that is switched off
    order = [0, 1] if case.parts[0].E0 < case.parts[1].E0 else [1, 0]
    off, on = order
    comps = list(case.psi0.components)
    comps[off] = ds._scale1(nbb, 0.0, comps[off])
    E0, psi, N = krylov.lanczos(nbb, case.H, DirectSum(comps), dict(N_max=40, reortho=True))
    assert abs(E0 - case.parts[on].E0) < 1e-9 * abs(E0)
    assert dc.component_is_zero(nbb, psi[off]) and not dc.component_is_zero(nbb, psi[on])
    E_alone, _, _ = krylov.lanczos(nbb, case.parts[on].H, case.parts[on].psi0, dict(N_max=40, reortho=True))
    assert abs(E0 - E_alone) < 1e-9 * abs(E0)


@pytest.mark.parametrize('combo', ALL)
def test_lanczos_small_cache_rebuilds_the_dropped_vectors(nbb, combo):
    case = dc.SumCase(nbb, combo, 1)
    E_full, psi_full, N_full = krylov.lanczos(nbb, case.H, case.psi0, dict(N_max=40))
    E_small, psi_small, N_small = krylov.lanczos(nbb, case.H, case.psi0, dict(N_max=40, N_cache=3))
    assert N_full == N_small and abs(E_full - E_small) < 1e-10 * abs(E_full)
    assert abs(abs(ds.inner(nbb, psi_full, psi_small)) - 1.0) < 1e-8


@pytest.mark.parametrize('combo', ALL)
def test_projected_lanczos_finds_the_second_ground_energy(nbb, combo):
    case = dc.SumCase(nbb, combo, 2)
    E, U = case.spectrum()
    g = case.tensor(U[:, 0])
    op = sparse.ProjectedLinearOperator(case.H, [g], project_operator=True)
    E1, psi, N = krylov.LanczosGroundState(nbb, op, case.psi0, dict(N_max=60, reortho=True)).run()
    assert abs(E1 - E[1]) < 1e-8
    assert abs(np.vdot(U[:, 0], case.y(psi))) < 1e-6


@pytest.mark.parametrize('z', [-8.0, -7.0 + 0.5j])
@pytest.mark.parametrize('combo', ALL)
def test_gmres_solves_the_shifted_system(nbb, combo, z):
    case = dc.SumCase(nbb, combo, 3)
    A = sparse.ShiftedLinearOperator(case.H, -z)
    b = case.psi0
    g = krylov.GMRES(nbb, A, case.zero_like(), b, {'N_max': 40, 'restart': 10, 'res': 1e-10, 'N_min': 0})
    assert type(g.V) is krylov._DirectSumOps
    x, rel, errs, iters = g.run()
    assert isinstance(x, DirectSum)
    Am = case.M - z * np.eye(len(case.y0))
    xd = case.y(x)
    assert rel < 1e-8
    assert np.linalg.norm(Am @ xd - case.y0) / np.linalg.norm(case.y0) < 1e-8
    want = np.linalg.solve(Am, case.y0)
    assert np.linalg.norm(xd - want) / np.linalg.norm(want) < 1e-7


def test_gmres_refuses_a_tensor_beside_a_direct_sum(nbb):
    case = dc.SumCase(nbb, 'abelian+tree')
    with pytest.raises(ValueError):
        krylov.GMRES(nbb, case.H, case.psi0[0], case.psi0)
    with pytest.raises(ValueError):
        krylov.GMRES(nbb, case.H, case.psi0, DirectSum([case.psi0[0]]))


@pytest.mark.parametrize('N_cache', [10, 40])
@pytest.mark.parametrize('combo', ALL)
def test_lanczos_evolution_against_expm(nbb, combo, N_cache):
    case = dc.SumCase(nbb, combo, 4)
    solver = krylov.LanczosEvolution(nbb, case.H, case.psi0, dict(N_max=40, N_cache=N_cache))
    for delta in (-0.1j, 1j, 0.1, 1.0):
        out, _ = solver.run(delta, normalize=False)
        out_n, _ = solver.run(delta, normalize=True)
        got, got_n = case.y(out), case.y(out_n)
        n = np.linalg.norm(got)
        assert n > 0 and np.linalg.norm(got / n - got_n) < 1e-8
        want = case.expm_apply(delta, case.y0)
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-8, delta


@pytest.mark.parametrize('combo', ALL)
def test_arnoldi_finds_the_dominant_eigenvalue(nbb, combo):
    case = dc.SumCase(nbb, combo, 5)
    Es, psis, N = krylov.Arnoldi(nbb, case.H, case.psi0, dict(N_max=40, which='LM')).run()
    E, _ = case.spectrum()
    want = E[np.argmax(np.abs(E))]
    assert abs(Es[0] - want) < 1e-8 * abs(want)
    v = case.y(psis[0])
    assert abs(np.linalg.norm(v) - 1.0) < 1e-8 and np.linalg.norm(case.M @ v - Es[0] * v) < 1e-6 * (abs(want) + 1.0)


def test_arnoldi_evolution_runs_on_a_direct_sum(nbb):
    case = dc.SumCase(nbb, 'abelian+tree', 6)
    out, _ = krylov.ArnoldiEvolution(nbb, case.H, case.psi0, dict(N_max=40)).run(0.1)
    want = case.expm_apply(0.1, case.y0)
    assert np.linalg.norm(case.y(out) - want) / np.linalg.norm(want) <= 1e-8
