"""Thick-restart Lanczos on the device (krylov.LanczosEigenpairs on pools and on tensors, krylov._FlatOps.rotate): the inputs
and the criteria of tests/test_eigenpairs.py (tests/eigenpairs_cases.py), and what only the device has -- the pool fallback,
the library calls of a step and of a restart, the weighted entries of fusion-tree pools."""
import numpy as np
import pytest

import direct_sum_cases as dc
import eigenpairs_cases as ec
from cyten_amd import direct_sum as ds
from cyten_amd import krylov, sparse
from cyten_amd.direct_sum import DirectSum

pytestmark = pytest.mark.gpu

ALL = list(dc.COMBOS)
GS_ENTRIES = ['cyb_gram_schmidt_f64', 'cyb_gram_schmidt_c128', 'cyb_gram_schmidt_weighted_f64', 'cyb_gram_schmidt_weighted_c128']


class _Spy:
    """counts the calls of attributes of an object and puts the ORIGINAL objects back (a ctypes function keeps its prototype)"""

    def __init__(self, obj, *names):
        self.obj, self.names = obj, names
        self.orig = {n: getattr(obj, n) for n in names}
        self.n = {n: 0 for n in names}

    def __enter__(self):
        for name in self.names:
            def counted(*a, _name=name, **k):
                self.n[_name] += 1
                return self.orig[_name](*a, **k)
            setattr(self.obj, name, counted)
        return self

    def __exit__(self, *exc):
        for name in self.names:
            setattr(self.obj, name, self.orig[name])


def _ops_class(flat):
    return krylov._FlatDirectSumOps if flat else krylov._DirectSumOps


@pytest.mark.parametrize('which,num_ev,N_max', ec.SETTINGS[:2], ids=lambda v: str(v))
@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('combo', ALL)
def test_device_spectrum_and_vectors_on_pools_and_on_tensors(bb, combo, cplx, which, num_ev, N_max):
    case = ec.shared_case(bb, combo, 0, cplx)
    Es = {}
    for flat in (True, False):
        solver, Es[flat], vecs, N, Y = ec.run_and_check(case, which, num_ev, N_max, flat=flat)
        assert type(solver.V) is _ops_class(flat) and all(isinstance(v, DirectSum) for v in vecs)
        assert not flat or solver.V.cplx == cplx
        assert solver.restarts >= 2
        print(f'{combo} cplx {cplx} {which} flat {flat}: {N} matvecs, {solver.restarts} restarts')
    assert np.all(np.abs(Es[True] - Es[False]) <= 1e-12 * np.abs(Es[False]))


class Undeclared:
    """an operator that does not say whether it is complex"""

    def __init__(self, op):
        self.op = op

    def matvec(self, x):
        return self.op.matvec(x)


def test_device_real_pools_restart_on_complex_pools(bb):
    case = dc.SumCase(bb, 'abelian+tree', 0, True, False)
    seen = []
    orig = krylov._FlatDirectSumOps.__init__

    def spy(self, bb_, H, template, cplx=False):
        seen.append(bool(cplx))
        orig(self, bb_, H, template, cplx)

    krylov._FlatDirectSumOps.__init__ = spy
    try:
        solver, Es, vecs, N, Y = ec.run_and_check(case, 'SA', 4, 12, flat=True, H=Undeclared(case.H))
    finally:
        krylov._FlatDirectSumOps.__init__ = orig
    assert seen == [False, True] and type(solver.V) is krylov._FlatDirectSumOps and solver.V.cplx


def _pools(bb, combo, count, cplx=False):
    case = dc.SumCase(bb, combo, 0, cplx, cplx)
    V = krylov._FlatDirectSumOps(bb, case.H, case.psi0, cplx)
    return case, V, [V.enter(dc.SumCase(bb, combo, 30 + s, cplx, cplx).psi0) for s in range(count)]


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('combo', ['abelian+abelian', 'abelian+tree'])
def test_rotate_on_pools_is_one_call_in_place_and_no_download(bb, rng, combo, cplx):
    m, k = 7, 3
    case, V, pools = _pools(bb, combo, m, cplx)
    X = np.array([case.y(V.leave(p)) for p in pools]).T
    before = [p.cpu().numpy().copy() for p in pools]
    Q = rng.standard_normal((m, k))
    with _Spy(bb.lib, 'cyb_basis_rotate_f64', 'cyb_lincomb_strided_batched_f64', 'cyb_lincomb_strided_batched_c128') as calls, \
            _Spy(bb.ctx, 'd2h', 'empty') as ctx:
        out = V.rotate(pools, Q)
    assert calls.n == {'cyb_basis_rotate_f64': 1, 'cyb_lincomb_strided_batched_f64': 0, 'cyb_lincomb_strided_batched_c128': 0}
    assert ctx.n == {'d2h': 0, 'empty': 0}
    assert len(out) == k and all(o is p for o, p in zip(out, pools))                 # in place on the first k pools
    want = X @ Q
    bound = 2 * m * 2.0 ** -53 * (np.abs(X) @ np.abs(Q)) * 2                          # (the scaled coordinates: one more rounding)
    got = np.array([case.y(V.leave(o)) for o in out]).T
    assert np.all(np.abs(got - want) <= bound + 1e-300)
    for p, b in zip(pools[k:], before[k:]):
        assert p.cpu().numpy().tobytes() == b.tobytes()
    # the gaps of the pool are zero and stay zero
    used = np.zeros(V.total, dtype=bool)
    for off, sh in zip(V.offs, V.shapes):
        used[off:off + int(np.prod(sh))] = True
    for o in out:
        gaps = o.cpu().numpy()[~used]
        assert gaps.tobytes() == np.zeros(len(gaps), dtype=gaps.dtype).tobytes()


def test_rotate_with_more_than_32_columns_writes_fresh_pools_in_chunks(bb, rng):
    m = k = 40
    case, V, pools = _pools(bb, 'abelian+abelian', m)
    X = np.array([case.y(V.leave(p)) for p in pools]).T
    before = [p.cpu().numpy().copy() for p in pools]
    Q = np.linalg.qr(rng.standard_normal((m, k)))[0]
    with _Spy(bb.lib, 'cyb_basis_rotate_f64') as calls, _Spy(bb.ctx, 'd2h') as ctx:
        out = V.rotate(pools, Q)
    assert calls.n['cyb_basis_rotate_f64'] == 2 and ctx.n['d2h'] == 0
    assert len(out) == k and not any(o is p for o in out for p in pools)
    got = np.array([case.y(V.leave(o)) for o in out]).T
    assert np.all(np.abs(got - X @ Q) <= 2 * m * 2.0 ** -53 * (np.abs(X) @ np.abs(Q)) + 1e-300)
    for p, b in zip(pools, before):
        assert p.cpu().numpy().tobytes() == b.tobytes()


def test_rotate_refuses_pools_of_mixed_dtypes(bb, rng):
    case, V, pools = _pools(bb, 'abelian+abelian', 3)
    pools[1] = V.combine([1j], [pools[1]])
    assert pools[1].is_complex() and not pools[0].is_complex()
    with pytest.raises(krylov._NeedComplex):
        V.rotate(pools, rng.standard_normal((3, 2)))
    with pytest.raises(ValueError):
        V.rotate(pools[:1], rng.standard_normal((3, 2)))


@pytest.mark.parametrize('combo', ['abelian+abelian', 'abelian+tree'])
def test_a_step_is_one_gram_schmidt_call_and_a_restart_one_rotation_without_a_download(bb, combo):
    """'abelian+tree' runs the weighted entry, 'abelian+abelian' the unweighted one"""
    case = dc.SumCase(bb, combo, 0)
    solver = krylov.LanczosEigenpairs(bb, case.H, case.psi0, dict(num_ev=4, N_max=12, max_restarts=ec.MAX_RESTARTS))
    rotations, orig = [], krylov._FlatOps.rotate

    def rotate(self, basis, Q):
        with _Spy(bb.lib, 'cyb_basis_rotate_f64') as inner, _Spy(bb.ctx, 'd2h') as reads:
            out = orig(self, basis, Q)
        rotations.append((inner.n['cyb_basis_rotate_f64'], reads.n['d2h'], all(o is b for o, b in zip(out, basis))))
        return out

    krylov._FlatOps.rotate = rotate
    try:
        with _Spy(bb.lib, 'cyb_basis_rotate_f64', *GS_ENTRIES) as calls:
            Es, vecs, N = solver.run()
    finally:
        krylov._FlatOps.rotate = orig
    assert type(solver.V) is krylov._FlatDirectSumOps and solver.restarts >= 2
    entry = 'cyb_gram_schmidt_weighted_f64' if combo == 'abelian+tree' else 'cyb_gram_schmidt_f64'
    assert calls.n[entry] == N and sum(calls.n[e] for e in GS_ENTRIES) == N
    # every restart, and the result: ONE library call, in place, nothing downloaded
    assert rotations == [(1, 0, True)] * (solver.restarts + 1) and calls.n['cyb_basis_rotate_f64'] == solver.restarts + 1
    ec.check_pairs(case, solver, Es, vecs, 'SA', 4)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_a_tree_tensor_runs_on_the_weighted_entries(bb, cplx):
    """a plain TreeTensor as the vector; the yardstick is the dense operator in the scaled coordinates of the weighted metric"""
    case = ec.PartCase(dc.SumCase(bb, (('tree', 2.5),), 0, cplx, cplx).parts[0])
    sfx = 'c128' if cplx else 'f64'
    with _Spy(bb.lib, 'cyb_basis_rotate_f64', *GS_ENTRIES) as calls:
        solver, Es, vecs, N, Y = ec.run_and_check(case, 'SA', 4, 12, flat=True)
    assert type(solver.V) is krylov._FlatTreeOps and solver.V.cplx == cplx and solver.restarts >= 1
    assert calls.n['cyb_gram_schmidt_weighted_' + sfx] == N and sum(calls.n[e] for e in GS_ENTRIES) == N
    assert calls.n['cyb_basis_rotate_f64'] == solver.restarts + 1
    tensors = ec.run_and_check(case, 'SA', 4, 12, flat=False)
    assert type(tensors[0].V) is krylov._TreeTensorOps
    assert np.all(np.abs(Es - tensors[1]) <= 1e-12 * np.abs(Es))


@pytest.mark.parametrize('flat', [True, False])
def test_device_a_zero_component_stays_exactly_zero(bb, flat):
    case = dc.SumCase(bb, 'abelian+tree', 1)
    comps = list(case.psi0.components)
    comps[1] = ds._scale1(bb, 0.0, comps[1])
    solver = krylov.LanczosEigenpairs(bb, case.H, DirectSum(comps), dict(num_ev=4, N_max=12, max_restarts=ec.MAX_RESTARTS, flat=flat))
    Es, vecs, N = solver.run()
    assert type(solver.V) is _ops_class(flat) and solver.restarts >= 1 and len(vecs) == 4
    for v in vecs:
        assert dc.component_is_zero(bb, v[1]) and not dc.component_is_zero(bb, v[0])
    want = np.linalg.eigvalsh(case.parts[0].M)[:4]
    assert np.all(np.abs(Es - want) <= 1e-9 * np.abs(want))


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_device_breakdown_returns_the_exact_pairs(bb, cplx, flat):
    """the bound of tests/test_eigenpairs.py: |dE| <= 1e-12 |M|"""
    case = dc.SumCase(bb, (('ab1', -5.5),), 0, cplx, cplx)
    solver = krylov.LanczosEigenpairs(bb, case.H, case.psi0, dict(num_ev=4, N_max=32, tol=0.0, flat=flat))
    Es, vecs, N = solver.run()
    E = np.linalg.eigvalsh(case.M)
    assert type(solver.V) is _ops_class(flat) and N <= 23 and solver.restarts == 0
    assert len(Es) == 4 and np.abs(Es - E[:4]).max() <= 1e-12 * np.abs(E).max()
    Y = np.array([case.y(v) for v in vecs]).T
    assert np.linalg.norm(case.M @ Y - Y * Es, axis=0).max() <= 1e-12 * np.abs(E).max()


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('combo', ALL)
def test_device_projected_operator_gives_the_next_states(bb, combo, flat):
    """the exact ground state projected out and parked at a penalty above the spectrum: 'SA' finds states 2 and 3 of M"""
    case = dc.SumCase(bb, combo, 2)
    E, U = case.spectrum()
    u = U[:, 0]
    penalty = 50.0
    op = sparse.ProjectedLinearOperator(case.H, [case.tensor(u)], project_operator=True, penalty=penalty)
    P = np.eye(len(u)) - np.outer(u, u.conj())
    Mp = P @ case.M @ P + penalty * np.outer(u, u.conj())
    solver, Es, vecs, N, Y = ec.run_and_check(case, 'SA', 2, 12, flat=flat, H=op, M=Mp)
    assert type(solver.V) is _ops_class(flat)
    assert np.all(np.abs(Es - E[1:3]) <= 1e-9 * np.abs(E[1:3]))
    assert np.abs(u.conj() @ Y).max() <= 1e-7
