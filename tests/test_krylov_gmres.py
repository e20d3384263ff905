"""GMRES (krylov_based.cpp:358-530), the operator wrappers of cyten_amd.sparse (sparse.cpp:188-344) and the projection
kernels of krylov_vec.hip.

CPU part: the solver's and the wrappers' host logic on the numpy stand-in backend, against dense matrices and the numpy
restatement in gmres_ref.py.  GPU part: the kernels against numpy, GMRES and projected Lanczos on flat pools against the
dense answers and against tensor operations, and the host synchronisations of a step."""
import ctypes as C

import numpy as np
import pytest

from cyten_amd import abelian as ab
from cyten_amd import krylov, sparse
from cyten_amd import workloads as wl
from oracle import abelian_ref as ref
from oracle import krylov_ref

from gmres_ref import gmres_dense, projected_dense
from helpers import to_device_tensor
from numpy_backend import NumpyGroupedBackend


class ComplexNumpyBackend(NumpyGroupedBackend):
    """The numpy stand-in with the complex inner product and norm (conj(x) y, |x|^2)."""

    def as_block(self, a, dtype=None, device=None):
        return np.array(a, dtype=complex if np.iscomplexobj(a) else float)

    def norm_many(self, blocks):
        return float(np.sqrt(sum(np.vdot(b, b).real for b in blocks)))

    def inner_many(self, xs, ys):
        s = np.sum([np.vdot(x, y) for x, y in zip(xs, ys)])
        return complex(s) if np.iscomplexobj(s) else float(s)


def _setup(bbk, chi=16, D=2, hermitian=True, seed=7):
    cfg = wl.config_heff(chi, D, seed=seed, hermitian=hermitian)
    dev = {k: to_device_tensor(bbk, v) for k, v in cfg.items()}
    dense = {k: ref.to_dense(v) for k, v in cfg.items()}
    H = krylov.HEffective(bbk, dev['LP'], dev['W1'], dev['W2'], dev['RP'])
    Hm = krylov_ref.heff_matrix(dense['LP'], dense['W1'], dense['W2'], dense['RP'])
    return dev, dense, H, Hm


def _dense_of(bbk, t):
    return np.asarray(t.to_dense(bbk)).ravel()


def _from_dense(bbk, t, vec):
    """A tensor on t's legs holding every charge-allowed block of the dense vector `vec`."""
    inds = ab.AbelianTensor.allowed_block_inds(t.symmetry, t.legs)
    arr = np.asarray(vec).reshape([l.dim for l in t.legs])
    blocks = []
    for row in inds:
        sl = tuple(slice(int(l.slices[i]), int(l.slices[i + 1])) for l, i in zip(t.legs, row))
        blocks.append(np.ascontiguousarray(arr[sl]))
    return ab.AbelianTensor.from_numpy_blocks(bbk, t.symmetry, t.legs, blocks, inds, t.num_codomain)


def _sector(bbk, t):
    """Mask of the dense entries that the charge rule allows on t's legs (the space the operator acts on)."""
    ones = _from_dense(bbk, t, np.ones([l.dim for l in t.legs]).ravel())
    return _dense_of(bbk, ones) != 0


def _rel(got, want):
    return np.linalg.norm(got - want) / np.linalg.norm(want)


def _restricted(Hm, mask):
    return Hm[np.ix_(mask, mask)]


# ------------------------------------------------------------------------------------------ GMRES host logic (CPU)

def test_gmres_shifted_real_matches_dense_and_restatement():
    """The reference's test (test_krylov_based.py:191-203): a non-Hermitian H_eff shifted by 1.5, real data.  Its spectrum
    surrounds 0 (indefinite): restarted GMRES(20) stagnates near |r| / |b| = 0.8 on this 200-dimensional sector, so the
    Krylov space is allowed to span it (N_max=200; full GMRES converges in about 150 steps)."""
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk, hermitian=False)
    A = sparse.ShiftedLinearOperator(H, 1.5)
    b = dev['theta']
    bd = _dense_of(nbk, b)
    mask = _sector(nbk, b)
    Am = _restricted(Hm, mask) + 1.5 * np.eye(mask.sum())
    x0 = ab.scale(nbk, 0.0, b)
    opts = {'N_max': 200, 'restart': 2, 'res': 1e-10, 'N_min': 0}
    x, rel, errs, iters = krylov.GMRES(nbk, A, x0, b, opts).run()
    xd = _dense_of(nbk, x)
    want = np.zeros_like(bd)
    want[mask] = np.linalg.solve(Am, bd[mask])
    assert _rel(xd, want) < 1e-8
    assert rel < 1e-6
    _, rel_r, errs_r, iters_r = gmres_dense(lambda v: Am @ v, np.zeros(mask.sum()), bd[mask], **opts)
    assert iters == iters_r
    assert len(errs) == len(errs_r)
    for a, r in zip(errs, errs_r):
        assert len(a) == len(r)
        np.testing.assert_allclose(a, r, rtol=1e-8)


def test_gmres_restarts():
    """GMRES(5) on a definite operator (H_eff + 20): several cycles, each list of total_error starting with the true residual
    that reset() computed."""
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk)
    A = sparse.ShiftedLinearOperator(H, 20.0)
    b = dev['theta']
    bd = _dense_of(nbk, b)
    bn = np.linalg.norm(bd)
    mask = _sector(nbk, b)
    Am = _restricted(Hm, mask) + 20.0 * np.eye(mask.sum())
    opts = {'N_max': 5, 'restart': 50, 'res': 1e-9, 'N_min': 0}
    g = krylov.GMRES(nbk, A, ab.scale(nbk, 0.0, b), b, opts)
    x, rel, errs, iters = g.run()
    assert len(iters) >= 2 and len(errs) == len(iters)
    assert all(len(e) == n + 1 for e, n in zip(errs, iters))
    assert all(n == 5 for n in iters[:-1])
    assert errs[0][0] == pytest.approx(1.0)
    xs = np.zeros(mask.sum())
    for k in range(len(errs)):     # (the x after k cycles, by one dense cycle at a time)
        assert errs[k][0] == pytest.approx(np.linalg.norm(Am @ xs - bd[mask]) / bn, rel=1e-8)
        xs = gmres_dense(lambda v: Am @ v, xs, bd[mask], N_min=0, N_max=5, restart=1, res=1e-9)[0]
    assert rel < 1e-8
    assert g.H_numpy().shape == (6, 5) and g.H_numpy().dtype == np.complex128
    xd = _dense_of(nbk, x)
    assert np.linalg.norm(Am @ xd[mask] - bd[mask]) / bn < 1e-8
    _, _, errs_r, iters_r = gmres_dense(lambda v: Am @ v, np.zeros(mask.sum()), bd[mask], **opts)
    assert iters == iters_r
    for a, r in zip(errs, errs_r):
        np.testing.assert_allclose(a, r, rtol=1e-8)


def test_gmres_early_exit():
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk, hermitian=False)
    A = sparse.ShiftedLinearOperator(H, 1.5)
    b = dev['theta']
    bd = _dense_of(nbk, b)
    mask = _sector(nbk, b)
    Am = _restricted(Hm, mask) + 1.5 * np.eye(mask.sum())
    xs = np.zeros_like(bd)
    xs[mask] = np.linalg.solve(Am, bd[mask])
    x, rel, errs, iters = krylov.GMRES(nbk, A, _from_dense(nbk, b, xs), b, {'res': 1e-8}).run()
    assert iters == []
    assert len(errs) == 1 and errs[0][0] < 1e-8
    assert rel == errs[0][0]


class Dense:
    """A dense matrix acting on the tensors of one template (dense <-> tensor round trip)."""

    def __init__(self, bbk, M, template, is_complex=None):
        self.bb, self.M, self.t = bbk, M, template
        self.is_complex = np.iscomplexobj(M) if is_complex is None else is_complex

    def matvec(self, v):
        return _from_dense(self.bb, self.t, self.M @ _dense_of(self.bb, v))

    def adjoint(self):
        return Dense(self.bb, self.M.conj().T, self.t)


def test_gmres_breakdown():
    """b in a 3-dimensional invariant subspace of A: the third Krylov vector is exactly zero -- no NaN, the exact x."""
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk)
    t = dev['theta']
    n = int(np.prod([l.dim for l in t.legs]))
    mask = _sector(nbk, t)
    idx = np.flatnonzero(mask)
    M = np.zeros((n, n))
    rng = np.random.default_rng(3)
    M[np.ix_(idx, idx)] = np.diag(rng.uniform(1.0, 2.0, len(idx)))
    M[np.ix_(idx[:3], idx[:3])] = [[2.0, 1.0, 0.0], [0.0, 3.0, 1.0], [0.0, 0.0, 4.0]]   # upper triangular: exact in floats
    bd = np.zeros(n)
    bd[idx[0]] = 1.0
    b = _from_dense(nbk, t, bd)
    x, rel, errs, iters = krylov.GMRES(nbk, Dense(nbk, M, t), ab.scale(nbk, 0.0, b), b, {'N_min': 10, 'res': 1e-14}).run()
    xd = _dense_of(nbk, x)
    assert np.all(np.isfinite(xd))
    assert iters == [3] or iters[0] <= 3
    want = np.zeros(n)
    want[idx[:3]] = np.linalg.solve(M[np.ix_(idx[:3], idx[:3])], bd[idx[:3]])
    assert np.linalg.norm(xd - want) < 1e-12
    assert rel < 1e-12


def _complex_shift_case(nbk):
    dev, dense, H, Hm = _setup(nbk)
    t = dev['theta']
    mask = _sector(nbk, t)
    Hs = _restricted(Hm, mask)
    E0 = np.linalg.eigvalsh(Hs)[0]
    z = E0 + 0.3 + 0.2j   # H - (E0 + omega + i eta)
    rng = np.random.default_rng(11)
    bd = np.zeros(mask.size, dtype=np.complex128)
    bd[mask] = rng.standard_normal(mask.sum()) + 1j * rng.standard_normal(mask.sum())
    b = _from_dense(nbk, t, bd)
    A = sparse.ShiftedLinearOperator(H, -z)
    Am = Hs - z * np.eye(mask.sum())
    return A, Am, b, bd, mask


def test_gmres_complex_shift():
    nbk = ComplexNumpyBackend()
    A, Am, b, bd, mask = _complex_shift_case(nbk)
    assert A.is_complex
    opts = {'N_max': 20, 'restart': 50, 'res': 1e-10, 'N_min': 0}
    g = krylov.GMRES(nbk, A, ab.scale(nbk, 0.0, b), b, opts)
    x, rel, errs, iters = g.run()
    xd = _dense_of(nbk, x)
    assert rel < 1e-8
    assert _rel(xd[mask], np.linalg.solve(Am, bd[mask])) < 1e-7
    bn = np.linalg.norm(bd)
    xk = np.zeros(mask.sum(), dtype=np.complex128)
    # replay the cycles densely: the last error of each cycle is the true relative residual after it
    _, _, errs_r, iters_r = gmres_dense(lambda v: Am @ v, xk, bd[mask], N_min=0, N_max=20, restart=50, res=1e-10)
    assert iters == iters_r
    for e in errs:
        assert all(e[i + 1] <= e[i] * (1 + 1e-12) for i in range(len(e) - 1))
    for k in range(1, len(errs)):
        assert errs[k - 1][-1] == pytest.approx(errs[k][0], rel=1e-6)
    assert errs[-1][-1] == pytest.approx(np.linalg.norm(Am @ xd[mask] - bd[mask]) / bn, rel=1e-6)


def test_gmres_legs_must_match():
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk)
    with pytest.raises(ValueError):
        krylov.GMRES(nbk, H, dev['LP'], dev['theta'])


# ------------------------------------------------------------------------------------------ wrappers (CPU)

def _ortho_dense(nbk, t, mask, k, orthonormal, seed=5, cplx=False):
    rng = np.random.default_rng(seed)
    vs = rng.standard_normal((mask.sum(), k)) + (1j * rng.standard_normal((mask.sum(), k)) if cplx else 0)
    if orthonormal:
        vs = np.linalg.qr(vs)[0]
    out = []
    for i in range(k):
        v = np.zeros(mask.size, dtype=vs.dtype)
        v[mask] = vs[:, i]
        out.append(v)
    return out


def test_wrappers_against_dense():
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk)
    dev2, _, H2, Hm2 = _setup(nbk, seed=9)
    t = dev['theta']
    v = _dense_of(nbk, t)
    mask = _sector(nbk, t)
    P = np.diag(mask.astype(float))
    z = 0.7 - 0.25j
    sh = sparse.ShiftedLinearOperator(H, z)
    assert sh.is_complex and not sparse.ShiftedLinearOperator(H, 2.0).is_complex
    assert sh.unwrapped() is H
    np.testing.assert_allclose(_dense_of(nbk, sh.matvec(t)), (Hm + z * P) @ v, rtol=0, atol=1e-12 * np.abs(Hm @ v).max())
    sm = sparse.SumLinearOperator(H, [H2])
    np.testing.assert_allclose(_dense_of(nbk, sm.matvec(t)), (Hm + Hm2) @ v, rtol=0, atol=1e-12 * np.abs(Hm @ v).max())
    assert sparse.SumLinearOperator(sh, [H2]).unwrapped() is H
    # projections: orthonormal -> P H P + penalty (1 - P); otherwise the reference's sequential order
    for orthonormal in (True, False):
        os_ = _ortho_dense(nbk, t, mask, 3, orthonormal)
        ot = [_from_dense(nbk, t, o) for o in os_]
        for project, pen in ((True, None), (True, 2.5), (False, 2.5), (False, None)):
            op = sparse.ProjectedLinearOperator(H, ot, project_operator=project, penalty=pen)
            got = _dense_of(nbk, op.matvec(t))
            want = projected_dense(Hm, os_, v, project, pen)
            assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
            if orthonormal:
                Q = np.stack(os_, axis=1)
                Pr = np.eye(len(v)) - Q @ Q.T
                M = (Pr @ Hm @ Pr if project else Hm) + (pen or 0.0) * (np.eye(len(v)) - Pr)
                assert np.linalg.norm(got - M @ v) <= 1e-12 * np.linalg.norm(want)
    # adjoint where the wrapped operator has one
    D = Dense(nbk, Hm + 0.1j * Hm2, t)
    adj = sparse.ProjectedLinearOperator(sparse.ShiftedLinearOperator(D, 1j), ot, penalty=1 + 1j).adjoint()
    assert adj.penalty == 1 - 1j and adj.original_operator.shift == -1j
    assert np.allclose(adj.unwrapped().M, (Hm + 0.1j * Hm2).conj().T)


def test_projected_lanczos_excited_state():
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk)
    t = dev['theta']
    mask = _sector(nbk, t)
    Hs = _restricted(Hm, mask)
    E, U = np.linalg.eigh(Hs)
    g = np.zeros(mask.size)
    g[mask] = U[:, 0]
    gt = _from_dense(nbk, t, g)
    op = sparse.ProjectedLinearOperator(H, [gt])
    E1, psi, N = krylov.LanczosGroundState(nbk, op, t, dict(N_max=60, N_min=2, P_tol=1e-24)).run()
    assert abs(E1 - E[1]) < 1e-9 * max(1.0, abs(E[1]))
    assert abs(np.vdot(g, _dense_of(nbk, psi))) < 1e-6


def test_projected_e_shift_rule():
    """E_shift shifts the operator INSIDE a projected operator: the ortho vectors keep eigenvalue `penalty`."""
    nbk = ComplexNumpyBackend()
    dev, dense, H, Hm = _setup(nbk)
    t = dev['theta']
    mask = _sector(nbk, t)
    Hs = _restricted(Hm, mask)
    E, U = np.linalg.eigh(Hs)
    g = np.zeros(mask.size)
    g[mask] = U[:, 0]
    gt = _from_dense(nbk, t, g)
    shift, pen = 3.0, -100.0
    op = sparse.ProjectedLinearOperator(H, [gt], penalty=pen)
    E0, psi, N = krylov.LanczosGroundState(nbk, op, t, dict(N_max=80, E_shift=shift, P_tol=1e-24)).run()
    # dense equivalent: P (H + shift) P + pen |g><g|, lowest eigenvalue is pen; E0 reported with the shift taken off
    Pr = np.eye(mask.sum()) - np.outer(U[:, 0], U[:, 0])
    Md = Pr @ (Hs + shift * np.eye(mask.sum())) @ Pr + pen * np.outer(U[:, 0], U[:, 0])
    assert abs(E0 - (np.linalg.eigvalsh(Md)[0] - shift)) < 1e-8
    assert op.original_operator is H      # the caller's operator is not changed


# ------------------------------------------------------------------------------------------ kernels (GPU)

def _gs_call(bb, name, basis, w, *args):
    from cyten_amd import _lib
    ptrs = (C.c_void_p * max(len(basis), 1))(*[v.data_ptr() for v in basis])
    n = w.numel()
    bb.ctx.sync_stream()
    fn = getattr(bb.lib, name)
    if name.startswith('cyb_multi_axpy'):
        h, alpha = args
        al = [complex(alpha).real, complex(alpha).imag] if name.endswith('c128') else [float(alpha)]
        _lib.check(fn(bb.ctx.handle, ptrs, len(basis), C.c_void_p(h.data_ptr()), *al, C.c_void_p(w.data_ptr()), n))
    elif name.startswith('cyb_multi_dot'):
        (h,) = args
        _lib.check(fn(bb.ctx.handle, ptrs, len(basis), C.c_void_p(w.data_ptr()), n, C.c_void_p(h.data_ptr())))
    else:
        passes, out = args
        _lib.check(fn(bb.ctx.handle, ptrs, len(basis), C.c_void_p(w.data_ptr()), n, passes, C.c_void_p(out.data_ptr())))


@pytest.mark.gpu
@pytest.mark.parametrize('cplx', [False, True])
def test_gpu_projection_kernels(bb, cplx):
    import torch
    sfx = 'c128' if cplx else 'f64'
    rng = np.random.default_rng(21)
    k = 2 if cplx else 1
    two_tiles = 2048 * 256 + 257   # float64 sweeps: gs_grid gives a workgroup two tiles above 2048 * 256 elements
    for n in (0, 1, 31, 4097, 300001, two_tiles):
        for m in (1, 5) if n == two_tiles else (1, 2, 7, 21, 64):
            if (n > 5000 and m in (2, 7)) or (n == two_tiles and cplx):
                continue
            V = rng.standard_normal((m, n)) + (1j * rng.standard_normal((m, n)) if cplx else 0)
            w0 = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
            tv = [torch.from_numpy(np.ascontiguousarray(v)).to('cuda:0') for v in V]
            scale = np.linalg.norm(V, axis=1) * np.linalg.norm(w0)
            # multi-dot
            h = bb.ctx.empty(k * m)
            tw = torch.from_numpy(w0.copy()).to('cuda:0')
            _gs_call(bb, f'cyb_multi_dot_{sfx}', tv, tw, h)
            r = bb.ctx.d2h(h, k * m, np.float64)
            got = r[0::2] + 1j * r[1::2] if cplx else r
            assert np.all(np.abs(got - V.conj() @ w0) <= 1e-13 * scale + 1e-300)
            # multi-axpy with device coefficients: w + alpha V^T c
            c = rng.standard_normal(m) + (1j * rng.standard_normal(m) if cplx else 0)
            tc = torch.from_numpy(np.ascontiguousarray(c)).to('cuda:0')
            alpha = (0.5 - 2j) if cplx else -0.75
            _gs_call(bb, f'cyb_multi_axpy_{sfx}', tv, tw, tc, alpha)
            want = w0 + alpha * (c @ V)
            assert np.abs(tw.cpu().numpy() - want).max(initial=0) <= 1e-13 * (np.abs(want).max(initial=0) + 1) * m
            # Gram-Schmidt, one and two passes: coefficients, orthogonality, norm, determinism (an orthonormal basis where
            # n > m, so that two passes leave w orthogonal to it)
            if n > m:
                V = np.linalg.qr(V.T)[0].T.copy()
                tv = [torch.from_numpy(np.ascontiguousarray(v)).to('cuda:0') for v in V]
                scale = np.linalg.norm(V, axis=1) * np.linalg.norm(w0)
            for passes in (1, 2):
                outs, ws = [], []
                for _ in range(2):
                    tw = torch.from_numpy(w0.copy()).to('cuda:0')
                    out = bb.ctx.empty(k * m + 1)
                    _gs_call(bb, f'cyb_gram_schmidt_{sfx}', tv, tw, passes, out)
                    outs.append(bb.ctx.d2h(out, k * m + 1, np.float64))
                    ws.append(tw.cpu().numpy())
                assert outs[0].tobytes() == outs[1].tobytes() and ws[0].tobytes() == ws[1].tobytes()
                r = outs[0]
                hg = r[0:2 * m:2] + 1j * r[1:2 * m:2] if cplx else r[:m]
                h1 = V.conj() @ w0
                wg = ws[0]
                nw = np.linalg.norm(wg)
                assert abs(r[k * m] - nw) <= 1e-13 * max(nw, 1e-300) + 1e-300
                if passes == 1:
                    assert np.all(np.abs(hg - h1) <= 1e-13 * scale + 1e-300)
                    assert np.abs(wg - (w0 - h1 @ V)).max(initial=0) <= 1e-12 * np.linalg.norm(w0)
                else:
                    # h = h1 + h2 reproduces w0 = V^T h + w, w orthogonal to V
                    size = np.linalg.norm(w0) + np.abs(hg) @ np.linalg.norm(V, axis=1) + nw   # (n < m: terms grow)
                    assert np.abs(w0 - hg @ V - wg).max(initial=0) <= 1e-12 * size
                    if n > m:
                        assert np.abs(V.conj() @ wg).max() <= 1e-13 * nw
    # m = 65: rejected with an error, not a crash
    tv = [torch.zeros(8, dtype=torch.complex128 if cplx else torch.float64, device='cuda:0') for _ in range(65)]
    tw = torch.zeros(8, dtype=tv[0].dtype, device='cuda:0')
    out = bb.ctx.empty(k * 65 + 1)
    with pytest.raises(NotImplementedError):
        _gs_call(bb, f'cyb_gram_schmidt_{sfx}', tv, tw, 2, out)
    with pytest.raises(NotImplementedError):
        _gs_call(bb, f'cyb_multi_dot_{sfx}', tv, tw, out)


# ------------------------------------------------------------------------------------------ solvers on the device (GPU)

@pytest.mark.gpu
def test_gpu_gmres_real(bb):
    """A 56-dimensional sector: one cycle of at most 60 steps, every step a fused CGS2 call (m <= 56)."""
    dev, dense, H, Hm = _setup(bb, 7, hermitian=False)
    A = sparse.ShiftedLinearOperator(H, 1.5)
    b = dev['theta']
    bd = _dense_of(bb, b)
    mask = _sector(bb, b)
    Am = _restricted(Hm, mask) + 1.5 * np.eye(mask.sum())
    opts = {'N_max': 60, 'restart': 2, 'res': 1e-10, 'N_min': 0}
    g = krylov.GMRES(bb, A, ab.scale(bb, 0.0, b), b, opts)
    assert isinstance(g.V, krylov._FlatOps) and not g.V.cplx
    x, rel, errs, iters = g.run()
    xt, relt, errst, iterst = krylov.GMRES(bb, A, ab.scale(bb, 0.0, b), b, dict(opts, flat=False)).run()
    xd, xtd = _dense_of(bb, x), _dense_of(bb, xt)
    assert rel < 1e-6 and iters == iterst
    assert _rel(xd[mask], np.linalg.solve(Am, bd[mask])) < 1e-8
    assert _rel(xd, xtd) < 1e-10


@pytest.mark.gpu
def test_gpu_gmres_complex(bb):
    A, Am, b, bd, mask = _complex_shift_case(bb)
    opts = {'N_max': 20, 'restart': 50, 'res': 1e-10, 'N_min': 0}
    g = krylov.GMRES(bb, A, ab.scale(bb, 0.0, b), b, opts)
    assert isinstance(g.V, krylov._FlatOps) and g.V.cplx
    x, rel, errs, iters = g.run()
    xt, relt, errst, iterst = krylov.GMRES(bb, A, ab.scale(bb, 0.0, b), b, dict(opts, flat=False)).run()
    xd, xtd = _dense_of(bb, x), _dense_of(bb, xt)
    assert rel < 1e-8 and iters == iterst
    assert _rel(xd[mask], np.linalg.solve(Am, bd[mask])) < 1e-7
    assert _rel(xd, xtd) < 1e-10


class _CountD2H:
    def __init__(self, ctx):
        self.ctx, self.n, self.orig = ctx, 0, ctx.d2h

    def __enter__(self):
        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        self.ctx.d2h = counted
        return self

    def __exit__(self, *exc):
        del self.ctx.d2h


@pytest.mark.gpu
def test_gpu_host_syncs(bb):
    dev, dense, H, Hm = _setup(bb, hermitian=False)
    A = sparse.ShiftedLinearOperator(H, 1.5)
    b = dev['theta']
    g = krylov.GMRES(bb, A, ab.scale(bb, 0.0, b), b, {})
    g.arnoldi(0)
    g.arnoldi(1)            # (warm: operator plans and recordings exist)
    with _CountD2H(bb.ctx) as c:
        g.arnoldi(2)
    assert c.n == 1
    mask = _sector(bb, b)
    os_ = _ortho_dense(bb, b, mask, 3, False)
    for project, pen in ((True, 2.0), (False, 2.0)):
        op = sparse.ProjectedLinearOperator(H, [_from_dense(bb, b, o) for o in os_], project_operator=project, penalty=pen)
        V = krylov._FlatOps(bb, op, b, ab.AbelianTensor.allowed_block_inds(b.symmetry, b.legs), False)
        buf = V.enter(b)
        V.matvec(buf)
        with _CountD2H(bb.ctx) as c:
            out = V.matvec(buf)
        assert c.n == 0
        got = _dense_of(bb, V.leave(out))
        want = projected_dense(Hm, os_, _dense_of(bb, b), project, pen)
        assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)


@pytest.mark.gpu
@pytest.mark.parametrize('flat', [True, False])
def test_gpu_projected_lanczos(bb, flat):
    dev, dense, H, Hm = _setup(bb)
    t = dev['theta']
    mask = _sector(bb, t)
    E, U = np.linalg.eigh(_restricted(Hm, mask))
    g = np.zeros(mask.size)
    g[mask] = U[:, 0]
    op = sparse.ProjectedLinearOperator(H, [_from_dense(bb, t, g)])
    E1, psi, N = krylov.LanczosGroundState(bb, op, t, dict(N_max=60, P_tol=1e-24, flat=flat)).run()
    assert abs(E1 - E[1]) < 1e-9 * max(1.0, abs(E[1]))
