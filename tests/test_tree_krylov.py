"""Krylov solvers on fusion-tree vectors (cyten_amd.krylov on fusion_tree.TreeTensor, cyten_amd.sparse) on the CPU: the host
logic -- the dispatch on the vector type, the weighted inner product in every recurrence, the operator wrappers, the chain
operator and the pool layout -- on a numpy stand-in, against dense linear algebra in scaled coordinates
(tests/tree_krylov_ref.py)."""
import numpy as np
import pytest
import scipy.linalg as sla

import tree_krylov_cases as cases
import tree_krylov_ref as ref
from cyten_amd import fusion_tree as ft
from cyten_amd import krylov, sparse


@pytest.fixture
def nbb():
    return cases.NumpyKrylovBackend()


@pytest.mark.parametrize('cplx_op,cplx_vec', [(False, False), (True, True), (False, True)])
def test_lanczos_ground_state_and_tridiagonal_matrix(nbb, cplx_op, cplx_vec):
    case = cases.Case(nbb, 0, cplx_op, cplx_vec)
    solver, N = cases.check_ground_state(case, dict(N_max=40))
    assert isinstance(solver.V, krylov._TreeTensorOps) and 2 < N < 40
    # every symmetric operator is block diagonal in the coupled sector, so eigenvalues do not see the weights; the Krylov
    # coefficients do: the same blocks with all quantum dimensions 1 give another tridiagonal matrix
    plain = cases.Case(nbb, 0, cplx_op, cplx_vec, qdims=(1.0, 1.0, 1.0, 1.0))
    other = krylov.LanczosGroundState(nbb, plain.H, plain.psi0, dict(N_max=40, reortho=True))
    other.run()
    assert np.abs(other._h[:3, :3] - solver._h[:3, :3]).max() > 1e-3 * np.abs(solver._h[:3, :3]).max()


def test_lanczos_small_cache_rebuilds_the_dropped_vectors(nbb):
    case = cases.Case(nbb, 1)
    E_full, psi_full, N_full = krylov.lanczos(nbb, case.H, case.psi0, dict(N_max=40))
    E_small, psi_small, N_small = krylov.lanczos(nbb, case.H, case.psi0, dict(N_max=40, N_cache=3))
    assert N_full == N_small and abs(E_full - E_small) < 1e-10 * abs(E_full)
    assert abs(abs(ft.inner(nbb, psi_full.data, psi_small.data, case.cod, do_dagger=True)) - 1.0) < 1e-8


def _ortho_vector(case, rng):
    """a vector spread over all four sectors with a large component along the ground vector"""
    E, U = np.linalg.eigh(case.M)
    y = rng.standard_normal(len(case.y0))
    y = y / np.linalg.norm(y) + 0.8 * U[:, 0]
    return y / np.linalg.norm(y)


def test_projected_operator_projects_in_the_weighted_inner_product(nbb, rng):
    case = cases.Case(nbb, 2)
    yo = _ortho_vector(case, rng)
    o = case.tensor(yo)
    assert all(np.abs(b).max() > 0 for b in cases.host_blocks(nbb, o))
    op = sparse.ProjectedLinearOperator(case.H, [o], project_operator=True)
    E0, psi, N = krylov.LanczosGroundState(nbb, op, case.psi0, dict(N_max=60, reortho=True)).run()
    n = len(yo)
    P = np.eye(n) - np.outer(yo, yo.conj())
    want = np.linalg.eigvalsh(P @ case.M @ P)[0]
    # the projector of the same blocks in the unweighted inner product is another operator with another lowest eigenvalue
    # (in block coordinates x it is 1 - xh xh^H with xh = x / |x|; in scaled coordinates y = S x that is 1 - (S xh)(S^-1 xh)^H)
    S = np.sqrt(np.repeat(case.qdims, [r * c for r, c in cases.SHAPES]))
    xh = np.concatenate([b.ravel() for b in cases.host_blocks(nbb, o)])
    xh = xh / np.linalg.norm(xh)
    Q = np.eye(n) - np.outer(S * xh, (xh / S).conj())
    wrong = np.linalg.eigvals(Q @ case.M @ Q).real.min()
    assert abs(wrong - want) > 1e-4
    assert abs(E0 - want) < 1e-8
    assert abs(np.vdot(yo, case.y(psi))) < 1e-6


@pytest.mark.parametrize('z', [-8.0, -7.0 + 0.5j])
def test_gmres_solves_the_shifted_system(nbb, rng, z):
    case = cases.Case(nbb, 3)
    A = sparse.ShiftedLinearOperator(case.H, -z)
    b = case.psi0
    x0 = ft.TreeTensor(ft.mul(nbb, 0.0, b.data), case.cod, case.dom)
    g = krylov.GMRES(nbb, A, x0, b, {'N_max': 40, 'restart': 10, 'res': 1e-10, 'N_min': 0})
    x, rel, errs, iters = g.run()
    Am = case.M - z * np.eye(len(case.y0))
    xd = case.y(x)
    assert rel < 1e-8
    assert np.linalg.norm(Am @ xd - case.y0) / np.linalg.norm(case.y0) < 1e-8      # the weighted residual norm
    want = np.linalg.solve(Am, case.y0)
    assert np.linalg.norm(xd - want) / np.linalg.norm(want) < 1e-7


@pytest.mark.parametrize('N_cache', [10, 40])
def test_lanczos_evolution_against_expm(nbb, N_cache):
    case = cases.Case(nbb, 4)
    solver = krylov.LanczosEvolution(nbb, case.H, case.psi0, dict(N_max=40, N_cache=N_cache))
    for delta in (-0.1j, 1j, 0.1, 1.0):
        out, _ = solver.run(delta, normalize=False)
        out_n, _ = solver.run(delta, normalize=True)
        got, got_n = case.y(out), case.y(out_n)
        n = np.linalg.norm(got)
        assert n > 0 and np.linalg.norm(got / n - got_n) < 1e-8
        want = ref.expm_apply(case.A, case.B, delta, case.y0)
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-8, delta


def test_arnoldi_finds_the_dominant_eigenvalue(nbb):
    case = cases.Case(nbb, 5)
    Es, psis, N = krylov.Arnoldi(nbb, case.H, case.psi0, dict(N_max=40, which='LM')).run()
    E = np.linalg.eigvalsh(case.M)
    want = E[np.argmax(np.abs(E))]
    assert abs(Es[0] - want) < 1e-8 * abs(want)
    v = case.y(psis[0])
    assert abs(np.linalg.norm(v) - 1.0) < 1e-8 and np.linalg.norm(case.M @ v - Es[0] * v) < 1e-6 * (abs(want) + 1.0)


def test_sum_and_shift_wrappers_act_on_tree_tensors(nbb):
    case = cases.Case(nbb, 6, True, True)
    op = sparse.SumLinearOperator(case.H, [sparse.ShiftedLinearOperator(case.H, 0.5 - 0.25j)])
    got = case.y(op.matvec(case.psi0))
    want = 2 * case.M @ case.y0 + (0.5 - 0.25j) * case.y0
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    assert op.is_complex and not sparse.ShiftedLinearOperator(cases.Case(nbb, 6).H, 1.0).is_complex
    other = ft.TreeTensor(case.psi0.data, case.dom, case.dom)
    with pytest.raises(ValueError):
        sparse.ProjectedLinearOperator(case.H, [case.psi0, other])


@pytest.mark.parametrize('cplx', [False, True])
def test_chain_operator_with_a_leg_move_between_two_contractions(nbb, rng, cplx):
    op, x, want, (ncod, ndom) = cases.braid_chain(nbb, rng, cplx)
    out = op.matvec(x)
    assert out.codomain is ncod and ft.same_space(out.domain, ndom) and op.out_codomain is ncod and op.is_complex == cplx
    got = {tuple(r): np.asarray(b) for r, b in zip(out.block_inds.tolist(), out.blocks)}
    scale = max(np.abs(b).max() for b in want.values())
    assert len(want) > 1 and set(want) <= set(got)
    for key, g in got.items():
        w = want.get(key)
        assert np.abs(g - (w if w is not None else 0.0)).max() <= 1e-10 * scale


def test_chain_operator_refuses_steps_that_do_not_fit(nbb):
    case = cases.Case(nbb, 0)
    a = cases.tree_tensor(nbb, case.A, case.cod, case.cod)
    with pytest.raises(ValueError):
        krylov.TreeChainOperator(nbb, [('compose_right', a)], case.cod, case.dom)       # A is on the codomain
    with pytest.raises(ValueError):
        krylov.TreeChainOperator(nbb, [('permute', a)], case.cod, case.dom)
    assert krylov.TreeChainOperator(nbb, [('compose_left', a)], case.cod, case.dom).is_complex is False
    c = cases.Case(nbb, 0, True)
    assert c.H.is_complex is True


def test_pool_layout_starts_blocks_on_granules_and_weights_every_granule():
    cod, dom = cases.spaces()
    inds, shapes, offs, total, weights = krylov.tree_pool_layout(cod, dom)
    assert inds.tolist() == [[k, k] for k in range(4)] and shapes == cases.SHAPES
    assert offs == [0, 256, 512, 768] and total == 768 + 7 * 256           # 1600 elements: seven granules
    assert all(o % 256 == 0 for o in offs) and len(weights) == total // 256
    for (i, _), sh, o in zip(inds.tolist(), shapes, offs):
        g0, g1 = o // 256, (o + sh[0] * sh[1] + 255) // 256
        assert g1 > g0 and np.all(weights[g0:g1] == cod.qdims[i])
    # a domain with fewer sectors, in another order of indices: pairs follow common_sectors, weights the codomain index
    dom2 = ft.TreeSpace.from_multiplicities([[1], [3]], [[(300,)], [(2,)]], np.array([2.0, cases.PHI]), 1)
    inds, shapes, offs, total, weights = krylov.tree_pool_layout(cod, dom2)
    assert inds.tolist() == [[1, 0], [3, 1]] and shapes == [(1, 300), (40, 2)] and offs == [0, 512] and total == 768
    assert weights.tolist() == [2.0, 2.0, cases.PHI]
