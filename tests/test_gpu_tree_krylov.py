"""Device side of the Krylov solvers on fusion-tree vectors: the weighted pool reductions of krylov_vec.hip at the C-ABI
(cyb_multi_dot_weighted_*, cyb_gram_schmidt_weighted_*) -- bit for bit against the unweighted entries on scaled data, and
against numpy with general weights -- and the solvers of cyten_amd.krylov on pools (_FlatTreeOps) and on tensors
(_TreeTensorOps) with the inputs and criteria of tests/test_tree_krylov.py."""
import ctypes as C

import numpy as np
import pytest

import su2_fixture
import tree_krylov_cases as cases
import tree_krylov_ref as ref
from cyten_amd import _lib
from cyten_amd import fusion_tree as ft
from cyten_amd import krylov, sparse

pytestmark = pytest.mark.gpu

GRANULE = 256
SMALL_N = [0, 1, 255, 256, 257, 4097]
# two tiles per workgroup (more than 2048 tiles of 256 doubles / 128 complex numbers): a workgroup crosses a weight change
LARGE_N = {False: 2100 * 256, True: 1100 * 256}
ALL_M = [1, 4, 5, 17, 64]              # J = 1, 1, 2, 8, 16 basis vectors per wave


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels at the C-ABI

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _ptrs(basis):
    return (C.c_void_p * max(len(basis), 1))(*[v.data_ptr() for v in basis])


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dot(bb, sfx, basis, w, n, h, weights=None, weighted=False):
    bb.ctx.sync_stream()
    if weighted:
        return getattr(bb.lib, f'cyb_multi_dot_weighted_{sfx}')(bb.ctx.handle, _ptrs(basis), len(basis), _vp(w), n, _vp(weights), _vp(h))
    return getattr(bb.lib, f'cyb_multi_dot_{sfx}')(bb.ctx.handle, _ptrs(basis), len(basis), _vp(w), n, _vp(h))


def _gs(bb, sfx, basis, w, n, passes, out, weights=None, weighted=False):
    bb.ctx.sync_stream()
    if weighted:
        return getattr(bb.lib, f'cyb_gram_schmidt_weighted_{sfx}')(bb.ctx.handle, _ptrs(basis), len(basis), _vp(w), n, passes, _vp(weights), _vp(out))
    return getattr(bb.lib, f'cyb_gram_schmidt_{sfx}')(bb.ctx.handle, _ptrs(basis), len(basis), _vp(w), n, passes, _vp(out))


def _random(rng, shape, cplx):
    return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)


def _granules(n):
    return (n + GRANULE - 1) // GRANULE


def _per_element(table, n):
    return np.repeat(table, GRANULE)[:n]


def _power_of_two_scales(rng, n):
    """s per granule from {1, 2, 4}, adjacent granules different"""
    s = np.empty(_granules(n))
    prev = 0.0
    for g in range(len(s)):
        prev = s[g] = rng.choice([x for x in (1.0, 2.0, 4.0) if x != prev])
    return s


def _run_both(bb, cplx, V, w0, table, m_list, unweighted_on):
    """(weighted results on (V, w0), unweighted results on `unweighted_on` = (V', w0')) per (m, passes): h of the multi-dot,
    out and the updated vector of the Gram-Schmidt step, as host arrays"""
    sfx, k, n = ('c128' if cplx else 'f64'), (2 if cplx else 1), V.shape[1]
    Vu, wu = unweighted_on
    tv, tvu = [_dev(v) for v in V], [_dev(v) for v in Vu]
    tab = _dev(table if len(table) else np.zeros(1))
    res = {}
    for m in m_list:
        h, hu = bb.ctx.empty(k * m), bb.ctx.empty(k * m)
        tw, twu = _dev(w0), _dev(wu)
        _lib.check(_dot(bb, sfx, tv[:m], tw, n, h, tab, True))
        _lib.check(_dot(bb, sfx, tvu[:m], twu, n, hu))
        res[(m, 0)] = ((bb.ctx.d2h(h, k * m, np.float64),), (bb.ctx.d2h(hu, k * m, np.float64),))
        for passes in (1, 2):
            out, outu = bb.ctx.empty(k * m + 1), bb.ctx.empty(k * m + 1)
            tw, twu = _dev(w0), _dev(wu)
            _lib.check(_gs(bb, sfx, tv[:m], tw, n, passes, out, tab, True))
            _lib.check(_gs(bb, sfx, tvu[:m], twu, n, passes, outu))
            res[(m, passes)] = ((bb.ctx.d2h(out, k * m + 1, np.float64), tw.cpu().numpy()),
                                (bb.ctx.d2h(outu, k * m + 1, np.float64), twu.cpu().numpy()))
    return res


def _sizes():
    out = []
    for cplx in (False, True):
        out += [(cplx, n, ALL_M) for n in SMALL_N] + [(cplx, LARGE_N[cplx], [1, 4, 64])]
    return out


@pytest.mark.parametrize('cplx,n,m_list', _sizes(), ids=lambda v: str(v) if not isinstance(v, list) else '')
def test_weights_that_are_squares_of_powers_of_two_give_the_bits_of_the_unweighted_entries_on_scaled_data(bb, rng, cplx, n, m_list):
    """d = s^2 with s in {1, 2, 4} per granule: scaling by a power of two commutes with rounding, so the weighted entry on
    (V, w) and the unweighted entry on (s V, s w) go through the same roundings -- the same h, the same norm, and s times the
    updated w, byte for byte.  Fails for a wrong granule index (a c128 tile is half a granule), a weight hoisted per
    workgroup, a norm without the weight, or another order of summation."""
    V, w0 = _random(rng, (max(m_list), n), cplx), _random(rng, n, cplx)
    s = _power_of_two_scales(rng, n)
    assert n <= GRANULE or np.all(s[1:] != s[:-1])
    se = _per_element(s, n)
    res = _run_both(bb, cplx, V, w0, s * s, m_list, (V * se, w0 * se))
    for (m, passes), (wt, un) in res.items():
        assert wt[0].tobytes() == un[0].tobytes(), (m, passes)
        if passes:
            assert (wt[1] * se).tobytes() == un[1].tobytes(), (m, passes)
            assert n == 0 or wt[0][-1] > 0.0


@pytest.mark.parametrize('cplx', [False, True])
def test_unit_weights_give_the_bits_of_the_unweighted_entries(bb, rng, cplx):
    for n in (257, 4097, LARGE_N[cplx]):
        m_list = [1, 5, 64] if n < 5000 else [4]
        V, w0 = _random(rng, (max(m_list), n), cplx), _random(rng, n, cplx)
        res = _run_both(bb, cplx, V, w0, np.ones(_granules(n)), m_list, (V, w0))
        for key, (wt, un) in res.items():
            assert all(a.tobytes() == b.tobytes() for a, b in zip(wt, un)), (n, key)


@pytest.mark.parametrize('cplx', [False, True])
def test_general_weights_against_numpy(bb, rng, cplx):
    """quantum dimensions 2j + 1 = 1, 2, 3, ... and the golden ratio, one per granule in turn; the bounds of
    test_gpu_projection_kernels with the norms taken in the weighted inner product"""
    sfx, k = ('c128' if cplx else 'f64'), (2 if cplx else 1)
    dims = np.array([1.0, 2.0, 3.0, cases.PHI, 4.0, 5.0, 6.0])
    for n in (1, 255, 256, 257, 4097):
        table = dims[np.arange(_granules(n)) % len(dims)]
        d = _per_element(table, n)
        wnorm = lambda x: np.sqrt(np.sum(d * np.abs(x) ** 2, axis=-1))
        tab = _dev(table)
        for m in ALL_M:
            V, w0 = _random(rng, (m, n), cplx), _random(rng, n, cplx)
            tv = [_dev(v) for v in V]
            scale = wnorm(V) * wnorm(w0)
            h = bb.ctx.empty(k * m)
            _lib.check(_dot(bb, sfx, tv, _dev(w0), n, h, tab, True))
            r = bb.ctx.d2h(h, k * m, np.float64)
            got = r[0::2] + 1j * r[1::2] if cplx else r
            assert np.all(np.abs(got - (V.conj() * d) @ w0) <= 1e-13 * scale + 1e-300)
            if n > m:       # a basis orthonormal in the weighted inner product, so that two passes leave w orthogonal to it
                V = ref.weighted_qr(V, d)
                tv = [_dev(v) for v in V]
                scale = wnorm(V) * wnorm(w0)
            for passes in (1, 2):
                outs, ws = [], []
                for _ in range(2):
                    tw = _dev(w0)
                    out = bb.ctx.empty(k * m + 1)
                    _lib.check(_gs(bb, sfx, tv, tw, n, passes, out, tab, True))
                    outs.append(bb.ctx.d2h(out, k * m + 1, np.float64))
                    ws.append(tw.cpu().numpy())
                assert outs[0].tobytes() == outs[1].tobytes() and ws[0].tobytes() == ws[1].tobytes()       # run to run
                r, wg = outs[0], ws[0]
                hg = r[0:2 * m:2] + 1j * r[1:2 * m:2] if cplx else r[:m]
                h1 = (V.conj() * d) @ w0
                nw = wnorm(wg)
                assert abs(r[k * m] - nw) <= 1e-13 * max(nw, 1e-300) + 1e-300
                if passes == 1:
                    assert np.all(np.abs(hg - h1) <= 1e-13 * scale + 1e-300)
                    assert np.abs(wg - (w0 - h1 @ V)).max(initial=0) <= 1e-12 * np.linalg.norm(w0)
                else:
                    size = np.linalg.norm(w0) + np.abs(hg) @ np.linalg.norm(V, axis=1) + np.linalg.norm(wg)
                    assert np.abs(w0 - hg @ V - wg).max(initial=0) <= 1e-12 * size
                    if n > m:
                        assert np.abs((V.conj() * d) @ wg).max() <= 1e-13 * nw


@pytest.mark.parametrize('cplx', [False, True])
def test_argument_checks_follow_the_unweighted_entries(bb, rng, cplx):
    import torch
    sfx, k = ('c128' if cplx else 'f64'), (2 if cplx else 1)
    dt = torch.complex128 if cplx else torch.float64
    tv = [torch.zeros(8, dtype=dt, device='cuda:0') for _ in range(65)]
    tw = torch.zeros(8, dtype=dt, device='cuda:0')
    tab = _dev(np.ones(1))
    out = bb.ctx.empty(k * 65 + 1)
    for weighted in (False, True):
        assert _gs(bb, sfx, tv, tw, 8, 2, out, tab, weighted) == _lib.CYB_ERR_UNSUPPORTED
        assert _dot(bb, sfx, tv, tw, 8, out, tab, weighted) == _lib.CYB_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        _lib.check(_gs(bb, sfx, tv, tw, 8, 2, out, tab, True))
    # a NULL table: refused where there is data, accepted for an empty vector
    assert _gs(bb, sfx, tv[:2], tw, 8, 2, out, None, True) == _lib.CYB_ERR_INVALID
    assert _dot(bb, sfx, tv[:2], tw, 8, out, None, True) == _lib.CYB_ERR_INVALID
    assert 'weight table' in bb.lib.cyb_last_error().decode()
    assert _dot(bb, sfx, tv[:2], tw, 0, out, None, True) == _lib.CYB_OK
    # m = 0: the Gram-Schmidt step leaves w alone and returns its weighted norm
    n = 700
    w0 = _random(rng, n, cplx)
    table = np.array([2.0, cases.PHI, 3.0])
    tw = _dev(w0)
    _lib.check(_gs(bb, sfx, [], tw, n, 2, out, _dev(table), True))
    want = np.sqrt(np.sum(_per_element(table, n) * np.abs(w0) ** 2))
    assert abs(bb.ctx.d2h(out, 1, np.float64)[0] - want) <= 1e-13 * want
    assert np.array_equal(tw.cpu().numpy(), w0)


# ---------------------------------------------------------------------------------------------------------------------------
# the solvers on the device

class Undeclared:
    """an operator that does not say whether it is complex: the solver finds out when a complex vector comes back"""

    def __init__(self, op):
        self.op = op

    def matvec(self, x):
        return self.op.matvec(x)


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('cplx_op,cplx_vec', [(False, False), (True, True), (False, True)])
def test_device_lanczos_ground_state_and_tridiagonal_matrix(bb, flat, cplx_op, cplx_vec):
    case = cases.Case(bb, 0, cplx_op, cplx_vec)
    solver, N = cases.check_ground_state(case, dict(N_max=40), flat=flat)
    if flat:
        assert isinstance(solver.V, krylov._FlatTreeOps) and solver.V.cplx == (cplx_op or cplx_vec)
    else:
        assert type(solver.V) is krylov._TreeTensorOps


def test_device_real_pools_restart_on_complex_pools_when_the_operator_returns_a_complex_vector(bb):
    case = cases.Case(bb, 0, True, False)
    seen = []
    orig = krylov._FlatTreeOps.__init__

    def spy(self, bb_, H, template, cplx=False):
        seen.append(bool(cplx))
        orig(self, bb_, H, template, cplx)

    krylov._FlatTreeOps.__init__ = spy
    try:
        case.H = Undeclared(case.H)
        solver, N = cases.check_ground_state(case, dict(N_max=40), flat=True)
    finally:
        krylov._FlatTreeOps.__init__ = orig
    assert seen == [False, True] and isinstance(solver.V, krylov._FlatTreeOps) and solver.V.cplx


class _Count:
    """counts the calls of one method of an object"""

    def __init__(self, obj, name):
        self.obj, self.name, self.n, self.orig = obj, name, 0, getattr(obj, name)

    def __enter__(self):
        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        setattr(self.obj, self.name, counted)
        return self

    def __exit__(self, *exc):
        delattr(self.obj, self.name)


def test_device_leave_returns_views_into_the_pool(bb):
    case = cases.Case(bb, 1)
    V = krylov._FlatTreeOps(bb, case.H, case.psi0, False)
    assert V.total == 768 + 7 * 256 and V.offs == [0, 256, 512, 768]
    buf = V.enter(case.psi0)
    with _Count(bb, 'copy_many') as copies, _Count(bb.ctx, 'empty') as allocs:
        t = V.leave(buf)
    assert copies.n == 0 and allocs.n == 0
    assert t.block_inds.tolist() == [[k, k] for k in range(4)] and t.codomain is case.cod and t.domain is case.dom
    for blk, off, sh in zip(t.blocks, V.offs, cases.SHAPES):
        assert blk.buf is buf and blk.ptr == buf.data_ptr() + 8 * off and tuple(blk.shape) == sh
    for got, want in zip(cases.host_blocks(bb, t), case.x0):
        assert np.array_equal(got, want)
    # the gaps are zero, so the weighted reduction over the flat range is the weighted norm of the tensor
    assert abs(V.norm(buf) - np.linalg.norm(case.y0)) <= 1e-13 * np.linalg.norm(case.y0)
    assert abs(V.inner(buf, V.scale(2.0, buf)) - 2 * np.vdot(case.y0, case.y0)) <= 1e-13 * 2 * np.vdot(case.y0, case.y0)


def _ortho(case, rng):
    E, U = np.linalg.eigh(case.M)
    y = rng.standard_normal(len(case.y0))
    y = y / np.linalg.norm(y) + 0.8 * U[:, 0]
    return y / np.linalg.norm(y)


@pytest.mark.parametrize('flat', [True, False])
def test_device_projected_lanczos(bb, rng, flat):
    case = cases.Case(bb, 2)
    yo = _ortho(case, rng)
    op = sparse.ProjectedLinearOperator(case.H, [case.tensor(yo)], project_operator=True)
    solver = krylov.LanczosGroundState(bb, op, case.psi0, dict(N_max=60, reortho=True, flat=flat))
    E0, psi, N = solver.run()
    assert isinstance(solver.V, krylov._FlatTreeOps if flat else krylov._TreeTensorOps)
    P = np.eye(len(yo)) - np.outer(yo, yo.conj())
    assert abs(E0 - np.linalg.eigvalsh(P @ case.M @ P)[0]) < 1e-8
    assert abs(np.vdot(yo, case.y(psi))) < 1e-6


def test_device_projected_matvec_on_pools_does_not_wait_for_the_host(bb, rng):
    case = cases.Case(bb, 2)
    ys = np.linalg.qr(rng.standard_normal((len(case.y0), 3)))[0].T
    for project, pen in ((True, 2.0), (False, 2.0)):
        op = sparse.ProjectedLinearOperator(case.H, [case.tensor(y) for y in ys], project_operator=project, penalty=pen)
        V = krylov._FlatTreeOps(bb, op, case.psi0, False)
        buf = V.enter(case.psi0)
        V.matvec(buf)
        with _Count(bb.ctx, 'd2h') as c:
            out = V.matvec(buf)
        assert c.n == 0
        got = case.y(V.leave(out))
        # the sequential projection of sparse.cpp:294-327 in scaled coordinates
        y, coef = case.y0.copy(), []
        if project:
            for o in ys:
                coef.append(np.vdot(o, y))
                y = y - coef[-1] * o
        else:
            coef = [np.vdot(o, y) for o in ys]
        y = case.M @ y
        if project:
            for o in ys:
                y = y - np.vdot(o, y) * o
        for o, c_ in zip(ys, coef):
            y = y + pen * c_ * o
        assert np.linalg.norm(got - y) <= 1e-12 * np.linalg.norm(y)
        # ... and it is what the wrapper computes on tensors
        assert np.linalg.norm(case.y(op.matvec(case.psi0)) - y) <= 1e-12 * np.linalg.norm(y)


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('z', [-8.0, -7.0 + 0.5j])
def test_device_gmres_solves_the_shifted_system(bb, flat, z):
    case = cases.Case(bb, 3)
    A = sparse.ShiftedLinearOperator(case.H, -z)
    b = case.psi0
    x0 = b.like(ft.mul(bb, 0.0, b.data))
    g = krylov.GMRES(bb, A, x0, b, {'N_max': 40, 'restart': 10, 'res': 1e-10, 'N_min': 0, 'flat': flat})
    assert isinstance(g.V, krylov._FlatTreeOps if flat else krylov._TreeTensorOps)
    assert not flat or g.V.cplx == isinstance(z, complex)
    x, rel, errs, iters = g.run()
    Am = case.M - z * np.eye(len(case.y0))
    xd = case.y(x)
    assert rel < 1e-8
    assert np.linalg.norm(Am @ xd - case.y0) / np.linalg.norm(case.y0) < 1e-8
    want = np.linalg.solve(Am, case.y0)
    assert np.linalg.norm(xd - want) / np.linalg.norm(want) < 1e-7


def test_device_lanczos_evolution_on_pools(bb):
    case = cases.Case(bb, 4)
    solver = krylov.LanczosEvolution(bb, case.H, case.psi0, dict(N_max=40))
    for delta in (1j, 0.1):
        out, _ = solver.run(delta, normalize=False)
        assert isinstance(solver.V, krylov._FlatTreeOps) and not solver.V.cplx        # real Krylov vectors whatever delta
        want = ref.expm_apply(case.A, case.B, delta, case.y0)
        assert np.linalg.norm(case.y(out) - want) / np.linalg.norm(want) <= 1e-8, delta


def test_device_lanczos_on_the_su2xu1_structure(bb, rng):
    """the SU(2) x U(1) structure of tests/golden/su2_chi512.npz scaled down to chi = 32: 28 coupled sectors with quantum
    dimensions 2j + 1, block sizes that are no multiples of anything; pools against tensors"""
    cod, dom = cases.su2xu1_spaces(su2_fixture.load(), 32)
    assert cod.num_sectors == 28 and len(set(cod.qdims.tolist())) > 3
    n = cod.num_sectors
    big = int(np.argmax(cod.multiplicities))
    A = [cases._hermitian(rng, cod.block_size(k), False, 2.5 if k == big else None) for k in range(n)]
    B = [cases._hermitian(rng, dom.block_size(k), False, -2.5 if k == big else None) for k in range(n)]
    H = cases.chain(bb, A, B, cod, dom)
    psi0 = cases.tree_tensor(bb, [rng.standard_normal((cod.block_size(k), dom.block_size(k))) for k in range(n)], cod, dom)
    opts = dict(N_max=40, reortho=True)
    s_flat = krylov.LanczosGroundState(bb, H, psi0, dict(opts, flat=True))
    E_flat, psi_flat, N_flat = s_flat.run()
    s_tens = krylov.LanczosGroundState(bb, H, psi0, dict(opts, flat=False))
    E_tens, psi_tens, N_tens = s_tens.run()
    assert isinstance(s_flat.V, krylov._FlatTreeOps) and type(s_tens.V) is krylov._TreeTensorOps
    assert N_flat == N_tens and abs(E_flat - E_tens) < 1e-9 * abs(E_tens)
    assert abs(E_flat + 6.25) < 1e-9 * 6.25
    assert abs(abs(ft.inner(bb, psi_flat.data, psi_tens.data, cod, do_dagger=True)) - 1.0) < 1e-7
    assert abs(ft.norm(bb, psi_flat.data, cod) - 1.0) < 1e-12
