"""Device side of direct sums as Krylov vectors: the list orthonormalisation of krylov_vec.hip at the C-ABI
(cyb_orthonormalize_*, all four entries) -- bit for bit against its step-by-step composition from the host --, the pool of a
direct sum (krylov._FlatDirectSumOps), and the solvers and sparse.gram_schmidt on pools and on tensors with the inputs and
criteria of tests/test_direct_sum.py."""
import ctypes as C

import numpy as np
import pytest

import direct_sum_cases as dc
import tree_krylov_cases as tcases
from cyten_amd import _lib
from cyten_amd import direct_sum as ds
from cyten_amd import krylov, sparse
from cyten_amd.direct_sum import DirectSum

pytestmark = pytest.mark.gpu

GRANULE = 256
SMALL_N = [0, 1, 3, 255, 256, 257, 4097]
# two tiles per workgroup of the sweeps (more than 2048 tiles of 256 doubles / 128 complex numbers)
LARGE_N = {False: 2100 * 256, True: 1100 * 256}
ALL_M = [1, 2, 5, 17]
ENTRIES = [(False, False), (False, True), (True, False), (True, True)]        # (cplx, weighted)
ENTRY_IDS = ['f64', 'weighted_f64', 'c128', 'weighted_c128']
DIMS = np.array([1.0, 2.0, 3.0, tcases.PHI, 4.0, 5.0, 6.0])                   # quantum dimensions, one per granule in turn


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptrs(addresses):
    return (C.c_void_p * max(len(addresses), 1))(*addresses)


def _sfx(cplx):
    return 'c128' if cplx else 'f64'


def _random(rng, shape, cplx):
    return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)


def _granules(n):
    return (n + GRANULE - 1) // GRANULE


def _table(n, weighted):
    """the weight table of a weighted case (general quantum dimensions), None for an unweighted one"""
    return DIMS[np.arange(max(_granules(n), 1)) % len(DIMS)] if weighted else None


def _per_element(table, n):
    return np.ones(n) if table is None else np.repeat(table, GRANULE)[:n]


def _ortho_raw(bb, cplx, addresses, m, n, rcond, out, wt=None):
    """the status of cyb_orthonormalize[_weighted]_{f64,c128} on raw device addresses"""
    bb.ctx.sync_stream()
    if wt is not None:
        return getattr(bb.lib, f'cyb_orthonormalize_weighted_{_sfx(cplx)}')(bb.ctx.handle, _ptrs(addresses), m, n, rcond, _vp(wt), _vp(out))
    return getattr(bb.lib, f'cyb_orthonormalize_{_sfx(cplx)}')(bb.ctx.handle, _ptrs(addresses), m, n, rcond, _vp(out))


def _ortho(bb, cplx, V, rcond, table=None):
    """one call on the rows of V: (vectors, norms, flags) as host arrays"""
    m, n = V.shape
    tv = [_dev(v) for v in V]
    out = _dev(np.full(2 * m, -7.0))
    _lib.check(_ortho_raw(bb, cplx, [t.data_ptr() for t in tv], m, n, rcond, out, None if table is None else _dev(table)))
    r = out.cpu().numpy()
    return np.array([t.cpu().numpy() for t in tv]).reshape(m, n), r[:m], r[m:]


def _gs(bb, cplx, basis, w, n, out, wt=None):
    bb.ctx.sync_stream()
    ptrs = _ptrs([v.data_ptr() for v in basis])
    if wt is not None:
        return getattr(bb.lib, f'cyb_gram_schmidt_weighted_{_sfx(cplx)}')(bb.ctx.handle, ptrs, len(basis), _vp(w), n, 2, _vp(wt), _vp(out))
    return getattr(bb.lib, f'cyb_gram_schmidt_{_sfx(cplx)}')(bb.ctx.handle, ptrs, len(basis), _vp(w), n, 2, _vp(out))


def _scaled_by(x, f):
    """every double of x times the double f (both parts of a complex number), as numpy rounds one multiplication"""
    return (np.ascontiguousarray(x).view(np.float64) * f).view(x.dtype)


def _composed(bb, cplx, V, rcond, table=None):
    """the same list step by step from the host: the CGS2 entry against the finished vectors, the norm downloaded, the vector
    multiplied in numpy by the double 1.0 / norm (or replaced by zeros) and uploaded again"""
    m, n = V.shape
    kk = 2 if cplx else 1
    wt = None if table is None else _dev(table)
    done, norms, flags = [], [], []
    for k in range(m):
        tw = _dev(V[k])
        out = bb.ctx.empty(kk * k + 1)
        _lib.check(_gs(bb, cplx, done, tw, n, out, wt))
        norm = float(bb.ctx.d2h(out, kk * k + 1, np.float64)[kk * k])
        x = tw.cpu().numpy()
        keep = norm > rcond
        done.append(_dev(_scaled_by(x, 1.0 / norm) if keep else np.zeros_like(x)))
        norms.append(norm)
        flags.append(1.0 if keep else 0.0)
    return np.array([t.cpu().numpy() for t in done]).reshape(m, n), np.array(norms), np.array(flags)


def _sizes():
    return [(c, w, n) for c, w in ENTRIES for n in SMALL_N + [LARGE_N[c]]]


def _size_id(v):
    return ('T' if v else 'F') if isinstance(v, bool) else str(v)


@pytest.mark.parametrize('cplx,weighted,n', _sizes(), ids=_size_id)
def test_one_call_is_the_composition_of_its_steps_bit_for_bit(bb, rng, cplx, weighted, n):
    """The yardstick: the list entry adds nothing to the existing CGS2 entry but one IEEE multiplication per double.  Fails
    for a step that reads the norm of another step, a scale kernel that misses or repeats an element (an odd count, an item
    boundary), a reciprocal that is not the correctly rounded 1.0 / norm, or workspace shared between the steps."""
    table = _table(n, weighted)
    for m in ALL_M:
        if 0 < n < m:
            continue                                     # (no independent list of m vectors of n elements)
        V = _random(rng, (m, n), cplx)
        if n == 0:
            out = _dev(np.full(2 * m, -7.0))
            tv = [_dev(np.zeros(1, dtype=V.dtype)) for _ in range(m)]
            _lib.check(_ortho_raw(bb, cplx, [t.data_ptr() for t in tv], m, 0, 0.0, out, None if table is None else _dev(table)))
            assert np.all(out.cpu().numpy() == -7.0)        # nothing is launched, nothing is written
            continue
        got, want = _ortho(bb, cplx, V, 0.0, table), _composed(bb, cplx, V, 0.0, table)
        for g, w, what in zip(got, want, ('vectors', 'norms', 'flags')):
            assert g.tobytes() == w.tobytes(), (m, what)
        assert np.all(got[2] == 1.0)


def _gram(Q, d):
    """the Gram matrix of the rows of Q in the inner product with the weights d, in extended precision"""
    Ql = Q.astype(np.clongdouble if np.iscomplexobj(Q) else np.longdouble)
    return (Ql.conj() * d.astype(np.longdouble)) @ Ql.T


def _reference_loop(V, d, rcond):
    """sparse.cpp:420-436 in numpy: one pass of modified Gram-Schmidt, kept iff the norm is > rcond"""
    res = []
    for v in V:
        v = v.copy()
        for o in res:
            v = v - np.sum(d * o.conj() * v) * o
        nrm = np.sqrt(np.sum(d * np.abs(v) ** 2))
        if nrm > rcond:
            res.append(v / nrm)
    return np.array(res)


@pytest.mark.parametrize('m', [5, 17])
@pytest.mark.parametrize('cplx,weighted,n', [s for s in _sizes() if s[2] >= 255], ids=_size_id)
def test_an_exact_copy_is_dropped_and_zeroed_and_the_rest_is_orthonormal(bb, rng, cplx, weighted, n, m):
    table = _table(n, weighted)
    d = _per_element(table, n)
    V = _random(rng, (m, n), cplx)
    V[2] = V[0]
    independent = np.delete(V, 2, axis=0)
    G0 = np.asarray(_gram(independent, d), dtype=np.complex128 if cplx else np.float64)
    assert np.linalg.cond(G0) <= 10.0
    Q, norms, flags = _ortho(bb, cplx, V, 1e-10, table)
    assert flags.tolist() == [1.0, 1.0, 0.0] + [1.0] * (m - 3)
    assert norms[2] <= 1e-10 and np.all(norms[flags == 1.0] > 1e-10)
    assert Q[2].tobytes() == np.zeros(n, dtype=V.dtype).tobytes()                   # +0.0 everywhere
    kept = Q[flags == 1.0]
    G = _gram(kept, d)
    assert float(np.abs(G - np.eye(m - 1)).max()) <= 1e-13
    want = _reference_loop(V, d, 1e-10)
    assert len(want) == m - 1
    # the same span: what the kept vectors leave of each vector of the reference loop (and the other way round)
    for A, B in ((want, kept), (kept, want)):
        coef = (A.conj() * d) @ B.T                                                  # <a_i, b_j>, conjugated below
        rest = A - coef.conj() @ B
        assert np.sqrt(np.sum(d * np.abs(rest) ** 2, axis=1)).max() <= 1e-12


@pytest.mark.parametrize('cplx,weighted', ENTRIES, ids=ENTRY_IDS)
def test_a_vector_with_a_nan_is_dropped_and_leaves_no_trace(bb, rng, cplx, weighted):
    for n in (257, 4097):
        table = _table(n, weighted)
        V = _random(rng, (5, n), cplx)
        bad, zero = V.copy(), V.copy()
        bad[1, n // 2] = np.nan
        bad[1, 3] = np.inf
        zero[1] = 0.0
        Q, norms, flags = _ortho(bb, cplx, bad, 1e-10, table)
        Qz, norms_z, flags_z = _ortho(bb, cplx, zero, 1e-10, table)
        assert flags.tolist() == [1.0, 0.0, 1.0, 1.0, 1.0] and np.isnan(norms[1])
        assert Q[1].tobytes() == np.zeros(n, dtype=V.dtype).tobytes()
        assert np.all(np.isfinite(Q)) and np.all(np.isfinite(np.delete(norms, 1)))
        assert Q.tobytes() == Qz.tobytes() and flags.tobytes() == flags_z.tobytes()
        assert np.delete(norms, 1).tobytes() == np.delete(norms_z, 1).tobytes() and norms_z[1] == 0.0


@pytest.mark.parametrize('cplx,weighted', ENTRIES, ids=ENTRY_IDS)
def test_the_threshold_is_strict_and_absolute(bb, cplx, weighted):
    """[3, 4] has the norm 5 exactly: dropped at rcond = 5, kept at the double below 5"""
    V = np.array([[3.0 + 4.0j]]) if cplx else np.array([[3.0, 4.0]])
    table = np.ones(1) if weighted else None
    Q, norms, flags = _ortho(bb, cplx, V, 5.0, table)
    assert norms.tolist() == [5.0] and flags.tolist() == [0.0] and Q.tobytes() == np.zeros_like(V).tobytes()
    Q, norms, flags = _ortho(bb, cplx, V, float(np.nextafter(5.0, 0.0)), table)
    assert norms.tolist() == [5.0] and flags.tolist() == [1.0]
    assert Q.tobytes() == _scaled_by(V, 1.0 / 5.0).tobytes()


@pytest.mark.parametrize('cplx,weighted,n', [s for s in _sizes() if s[2] > 0], ids=_size_id)
def test_nothing_is_written_outside_the_vectors(bb, rng, cplx, weighted, n):
    """every vector inside a larger allocation filled with a sentinel; an f64 vector starts at an odd element (8-byte
    aligned only: the scale kernel's leading scalar word)"""
    import torch
    m, guard, first = 3, 64, 65 if not cplx else 64
    table = _table(n, weighted)
    V = _random(rng, (m, n), cplx)
    V[1] = V[0]                                          # one dropped vector: the zeroing stays inside as well
    sentinel = 1234.5 + (0.25j if cplx else 0.0)
    bufs = []
    for v in V:
        host = np.full(first + n + guard, sentinel, dtype=V.dtype)
        host[first:first + n] = v
        bufs.append(_dev(host))
    esz = 16 if cplx else 8
    out = _dev(np.full(2 * m + 2 * guard, -7.0))
    out_view = out[guard:guard + 2 * m]
    _lib.check(_ortho_raw(bb, cplx, [b.data_ptr() + esz * first for b in bufs], m, n, 1e-10, out_view,
                          None if table is None else _dev(table)))
    torch.cuda.synchronize()
    Q, norms, flags = _ortho(bb, cplx, V, 1e-10, table)
    for b, q in zip(bufs, Q):
        host = b.cpu().numpy()
        assert np.all(host[:first] == sentinel) and np.all(host[first + n:] == sentinel)
        assert host[first:first + n].tobytes() == q.tobytes()          # and the alignment does not change a bit
    r = out.cpu().numpy()
    assert np.all(r[:guard] == -7.0) and np.all(r[guard + 2 * m:] == -7.0)
    assert r[guard:guard + m].tobytes() == norms.tobytes() and r[guard + m:guard + 2 * m].tobytes() == flags.tobytes()
    assert flags.tolist() == ([1.0, 0.0, 1.0] if n > 1 else [1.0, 0.0, 0.0])


def _power_of_two_scales(rng, n):
    """s per granule from {1, 2, 4}, adjacent granules different"""
    s = np.empty(_granules(n))
    prev = 0.0
    for g in range(len(s)):
        prev = s[g] = rng.choice([x for x in (1.0, 2.0, 4.0) if x != prev])
    return s


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 4097, 'large'])
def test_weights_that_are_squares_of_powers_of_two_give_the_bits_of_the_unweighted_entry_on_scaled_data(bb, rng, cplx, n):
    """the argument of the weighted-entry test of tests/test_gpu_tree_krylov.py: scaling by a power of two commutes with
    rounding, so the weighted entry on V and the unweighted entry on s V see the same norms and flags and leave s times the
    same vectors"""
    n = LARGE_N[cplx] if n == 'large' else n
    s = _power_of_two_scales(rng, n)
    se = np.repeat(s, GRANULE)[:n]
    for m in ALL_M:
        V = _random(rng, (m, n), cplx)
        if m >= 3:
            V[2] = V[0]
        Qw, norms_w, flags_w = _ortho(bb, cplx, V, 1e-10, s * s)
        Qu, norms_u, flags_u = _ortho(bb, cplx, V * se, 1e-10, None)
        assert norms_w.tobytes() == norms_u.tobytes() and flags_w.tobytes() == flags_u.tobytes(), m
        assert (Qw * se).tobytes() == Qu.tobytes(), m


@pytest.mark.parametrize('cplx,weighted', ENTRIES, ids=ENTRY_IDS)
def test_argument_checks(bb, cplx, weighted):
    import torch
    dt = torch.complex128 if cplx else torch.float64
    tv = [torch.ones(8, dtype=dt, device='cuda:0') for _ in range(65)]
    addr = [t.data_ptr() for t in tv]
    wt = _dev(np.ones(1)) if weighted else None
    out = _dev(np.full(2 * 65, -7.0))
    assert _ortho_raw(bb, cplx, addr, 65, 8, 0.0, out, wt) == _lib.CYB_ERR_UNSUPPORTED
    assert '65' in bb.lib.cyb_last_error().decode()
    with pytest.raises(NotImplementedError):
        _lib.check(_ortho_raw(bb, cplx, addr, 65, 8, 0.0, out, wt))
    assert _ortho_raw(bb, cplx, addr, 0, 8, 0.0, out, wt) == _lib.CYB_OK
    assert _ortho_raw(bb, cplx, addr[:3], 3, 0, 0.0, out, wt) == _lib.CYB_OK
    if cplx:        # 16-byte alignment of complex vectors, as for cyb_gram_schmidt_c128
        assert _ortho_raw(bb, cplx, [addr[0], addr[1] + 8], 2, 4, 0.0, out, wt) == _lib.CYB_ERR_INVALID
        assert 'misaligned' in bb.lib.cyb_last_error().decode()
    if weighted:
        assert getattr(bb.lib, f'cyb_orthonormalize_weighted_{_sfx(cplx)}')(bb.ctx.handle, _ptrs(addr[:2]), 2, 8, 0.0, None,
                                                                          _vp(out)) == _lib.CYB_ERR_INVALID
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7.0) and all(bool((t == 1).all()) for t in tv[:3])


# ---------------------------------------------------------------------------------------------------------------------------
# pools

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


THREE = (('ab2', 2.0), ('tree', 2.5), ('ab1', -5.5))


def test_pool_layout_round_trip_gaps_and_weights(bb):
    case = dc.SumCase(bb, THREE, 0, cplx_vec=[False, True, False])
    V = krylov._FlatDirectSumOps(bb, case.H, case.psi0, True)
    # ab2: blocks of 5, 9 and 140 elements at multiples of 32, the segment padded to a granule; the tree pool; ab1
    assert V.weighted and V.offs == [0, 32, 64, 256, 512, 768, 1024, 2816] and V.total == 3072
    assert V.weights.tolist() == [1.0] + [1.0, 2.0, 3.0] + [tcases.PHI] * 7 + [1.0]
    assert np.array_equal(bb.ctx.d2h(V._wdev, 12, np.float64), V.weights)
    with _Count(bb, 'copy_many') as copies:
        buf = V.enter(case.psi0)
    assert copies.n == 1
    with _Count(bb, 'copy_many') as copies, _Count(bb.ctx, 'empty') as allocs:
        back = V.leave(buf)
    assert copies.n == 0 and allocs.n == 0 and isinstance(back, DirectSum) and len(back) == 3
    for p, got, want in zip(case.parts, back.components, case.psi0.components):
        assert np.array_equal(got.block_inds, want.block_inds)
        for g, w in zip(got.blocks, want.blocks):
            assert g.buf is buf
            g, w = bb.to_numpy(g), bb.to_numpy(w)
            assert g.real.tobytes() == w.real.tobytes() and np.array_equal(g.imag, np.zeros_like(g.imag) + w.imag)
    host = buf.cpu().numpy()
    used = np.zeros(V.total, dtype=bool)
    for off, sh in zip(V.offs, V.shapes):
        used[off:off + int(np.prod(sh))] = True
    assert used.sum() == len(case.y0) and host[~used].tobytes() == np.zeros((~used).sum(), dtype=host.dtype).tobytes()
    # norm and inner over the flat range against the functions of the container
    other = dc.SumCase(bb, THREE, 1, cplx_vec=[True, False, False]).psi0
    obuf = V.enter(other)
    want_n, want_i = ds.norm(bb, case.psi0), ds.inner(bb, case.psi0, other)
    assert abs(V.norm(buf) - want_n) <= 1e-13 * want_n
    assert abs(V.inner(buf, obuf) - want_i) <= 1e-13 * ds.norm(bb, case.psi0) * ds.norm(bb, other)
    assert abs(V.inner(buf, obuf) - np.vdot(case.y0, case.y(other))) <= 1e-13 * ds.norm(bb, case.psi0) * ds.norm(bb, other)


def test_pool_without_a_tree_component_is_unweighted_and_packed_at_32(bb):
    case = dc.SumCase(bb, 'abelian+abelian')
    V = krylov._FlatDirectSumOps(bb, case.H, case.psi0, False)
    assert not V.weighted and V.offs == [0, 32, 64, 224] and V.total == 256 and V._weights_ptr() is None
    buf = V.enter(case.psi0)
    assert abs(V.norm(buf) - np.linalg.norm(case.y0)) <= 1e-13 * np.linalg.norm(case.y0)
    assert np.array_equal(case.y(V.leave(buf)), case.y0)


def _bytes_of(bb, t):
    return [t.block_inds.tobytes()] + [bb.to_numpy(b).tobytes() for b in t.blocks]


@pytest.mark.parametrize('kind,special', [('ab2', 2.0), ('tree', 2.5)])
def test_one_component_gives_the_bits_of_the_plain_tensor(bb, kind, special):
    """DirectSum([t]) has the pool of t byte for byte, so every launch of a run sees the same data"""
    case = dc.SumCase(bb, ((kind, special),), 7)
    part = case.parts[0]
    plain_ops = krylov._vector_ops(bb, part.H, part.psi0, False)
    sum_ops = krylov._vector_ops(bb, case.H, case.psi0, False)
    assert type(sum_ops) is krylov._FlatDirectSumOps and type(plain_ops) in (krylov._FlatOps, krylov._FlatTreeOps)
    assert sum_ops.offs == list(plain_ops.offs) and sum_ops.total == plain_ops.total
    assert sum_ops.enter(case.psi0).cpu().numpy().tobytes() == plain_ops.enter(part.psi0).cpu().numpy().tobytes()
    opts = dict(N_max=40, reortho=True)
    s_sum, s_plain = krylov.LanczosGroundState(bb, case.H, case.psi0, opts), krylov.LanczosGroundState(bb, part.H, part.psi0, opts)
    (E_s, psi_s, N_s), (E_p, psi_p, N_p) = s_sum.run(), s_plain.run()
    assert type(s_sum.V) is krylov._FlatDirectSumOps and isinstance(s_plain.V, krylov._FlatOps)
    assert N_s == N_p and E_s == E_p and _bytes_of(bb, psi_s[0]) == _bytes_of(bb, psi_p)
    g_opts = {'N_max': 40, 'restart': 10, 'res': 1e-10, 'N_min': 0}
    x_s, rel_s, errs_s, _ = krylov.GMRES(bb, sparse.ShiftedLinearOperator(case.H, 8.0), case.zero_like(), case.psi0, g_opts).run()
    x0 = ds._scale1(bb, 0.0, part.psi0)
    x_p, rel_p, errs_p, _ = krylov.GMRES(bb, sparse.ShiftedLinearOperator(part.H, 8.0), x0, part.psi0, g_opts).run()
    assert rel_s == rel_p and errs_s == errs_p and _bytes_of(bb, x_s[0]) == _bytes_of(bb, x_p)


# ---------------------------------------------------------------------------------------------------------------------------
# the solvers on the device: the cases and criteria of tests/test_direct_sum.py

ALL = list(dc.COMBOS)


def _ops_class(flat):
    return krylov._FlatDirectSumOps if flat else krylov._DirectSumOps


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('cplx_op,cplx_vec', [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize('combo', ALL)
def test_device_lanczos_ground_state_and_tridiagonal_matrix(bb, combo, cplx_op, cplx_vec, flat):
    """with (False, True): a real operator on a complex start vector -- complex pools from the first step"""
    case = dc.SumCase(bb, combo, 0, cplx_op, cplx_vec)
    solver, E0, psi, N = dc.check_ground_state(case, dict(N_max=40), flat=flat)
    assert type(solver.V) is _ops_class(flat) and isinstance(psi, DirectSum)
    assert not flat or solver.V.cplx == (cplx_op or cplx_vec)
    assert abs(E0 - min(p.E0 for p in case.parts)) < 1e-9 * abs(E0)                 # the minimum pin


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('combo', ALL)
def test_device_lanczos_leaves_a_zero_component_zero(bb, combo, flat):
    """the invariance pin of tests/test_direct_sum.py"""
    case = dc.SumCase(bb, combo, 1)
    off, on = (0, 1) if case.parts[0].E0 < case.parts[1].E0 else (1, 0)
    comps = list(case.psi0.components)
    comps[off] = ds._scale1(bb, 0.0, comps[off])
    solver = krylov.LanczosGroundState(bb, case.H, DirectSum(comps), dict(N_max=40, reortho=True, flat=flat))
    E0, psi, N = solver.run()
    assert type(solver.V) is _ops_class(flat)
    assert abs(E0 - case.parts[on].E0) < 1e-9 * abs(E0)
    assert dc.component_is_zero(bb, psi[off]) and not dc.component_is_zero(bb, psi[on])


class Undeclared:
    """an operator that does not say whether it is complex: the solver finds out when a complex vector comes back"""

    def __init__(self, op):
        self.op = op

    def matvec(self, x):
        return self.op.matvec(x)


def test_device_real_pools_restart_on_complex_pools(bb):
    """a real start vector under a complex operator that does not declare itself: the float64 pools meet a complex vector
    (_NeedComplex) and the run starts again on complex128 pools"""
    case = dc.SumCase(bb, 'abelian+tree', 0, True, False)
    seen = []
    orig = krylov._FlatDirectSumOps.__init__

    def spy(self, bb_, H, template, cplx=False):
        seen.append(bool(cplx))
        orig(self, bb_, H, template, cplx)

    krylov._FlatDirectSumOps.__init__ = spy
    try:
        case.H = Undeclared(case.H)
        solver, E0, psi, N = dc.check_ground_state(case, dict(N_max=40), flat=True)
    finally:
        krylov._FlatDirectSumOps.__init__ = orig
    assert seen == [False, True] and type(solver.V) is krylov._FlatDirectSumOps and solver.V.cplx


def test_device_a_component_operator_creates_blocks_outside_the_support_of_the_start_vector(bb, rng):
    """the start vector holds two of the three blocks of its abelian component; the component's operator couples all three.
    The pool is laid out over every charge-allowed block, so the run stays on pools and the result holds the new block."""
    case = dc.SumCase(bb, 'abelian+tree', 2)
    part = case.parts[0]
    n = len(part.y0)
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    ev = rng.uniform(0.5, 1.5, n)
    ev[0] = -9.0
    M = (q * ev) @ q.T
    M = 0.5 * (M + M.T)
    y0 = part.y0.copy()
    y0[5:14] = 0.0                                       # (the 9 x 1 block)
    case.H = sparse.DirectSumLinearOperator([dc.DenseOp(part, M), case.parts[1].H], bb)
    case.psi0 = DirectSum([part.tensor(y0, keep=[0, 2]), case.psi0[1]])
    assert len(case.psi0[0].blocks) == 2
    solver = krylov.LanczosGroundState(bb, case.H, case.psi0, dict(N_max=60, reortho=True))
    E0, psi, N = solver.run()
    assert type(solver.V) is krylov._FlatDirectSumOps
    assert abs(E0 + 9.0) < 1e-9 * 9.0
    assert len(psi[0].blocks) == 3 and np.abs(part.y(psi[0])[5:14]).max() > 1e-3
    assert abs(abs(np.vdot(q[:, 0], part.y(psi[0]))) - 1.0) < 1e-7 and ds.norm(bb, DirectSum([psi[1]])) < 1e-7


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('combo', ALL)
def test_device_projected_lanczos(bb, combo, flat):
    case = dc.SumCase(bb, combo, 2)
    E, U = case.spectrum()
    op = sparse.ProjectedLinearOperator(case.H, [case.tensor(U[:, 0])], project_operator=True)
    solver = krylov.LanczosGroundState(bb, op, case.psi0, dict(N_max=60, reortho=True, flat=flat))
    E1, psi, N = solver.run()
    assert type(solver.V) is _ops_class(flat)
    assert abs(E1 - E[1]) < 1e-8
    assert abs(np.vdot(U[:, 0], case.y(psi))) < 1e-6


def test_device_projected_matvec_on_pools_does_not_wait_for_the_host(bb, rng):
    case = dc.SumCase(bb, 'abelian+tree', 2)
    ys = np.linalg.qr(rng.standard_normal((len(case.y0), 3)))[0].T
    op = sparse.ProjectedLinearOperator(sparse.ShiftedLinearOperator(case.H, 0.5), [case.tensor(y) for y in ys], penalty=2.0)
    V = krylov._FlatDirectSumOps(bb, op, case.psi0, False)
    buf = V.enter(case.psi0)
    V.matvec(buf)
    with _Count(bb.ctx, 'd2h') as c, _Count(V, 'enter') as enters:
        out = V.matvec(buf)
    assert c.n == 0 and enters.n == 1            # one memset and one batched copy write the results of all components back
    y = case.y0.copy()
    coef = []
    for o in ys:
        coef.append(np.vdot(o, y))
        y = y - coef[-1] * o
    y = case.M @ y + 0.5 * y
    for o in ys:
        y = y - np.vdot(o, y) * o
    for o, c_ in zip(ys, coef):
        y = y + 2.0 * c_ * o
    assert np.linalg.norm(case.y(V.leave(out)) - y) <= 1e-12 * np.linalg.norm(y)
    assert np.linalg.norm(case.y(op.matvec(case.psi0)) - y) <= 1e-12 * np.linalg.norm(y)


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('z', [-8.0, -7.0 + 0.5j])
@pytest.mark.parametrize('combo', ALL)
def test_device_gmres_solves_the_shifted_system(bb, combo, z, flat):
    case = dc.SumCase(bb, combo, 3)
    A = sparse.ShiftedLinearOperator(case.H, -z)
    g = krylov.GMRES(bb, A, case.zero_like(), case.psi0, {'N_max': 40, 'restart': 10, 'res': 1e-10, 'N_min': 0, 'flat': flat})
    assert type(g.V) is _ops_class(flat)
    assert not flat or g.V.cplx == isinstance(z, complex)
    x, rel, errs, iters = g.run()
    Am = case.M - z * np.eye(len(case.y0))
    xd = case.y(x)
    assert rel < 1e-8
    assert np.linalg.norm(Am @ xd - case.y0) / np.linalg.norm(case.y0) < 1e-8
    want = np.linalg.solve(Am, case.y0)
    assert np.linalg.norm(xd - want) / np.linalg.norm(want) < 1e-7


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('combo', ALL)
def test_device_lanczos_evolution_against_expm(bb, combo, flat):
    case = dc.SumCase(bb, combo, 4)
    solver = krylov.LanczosEvolution(bb, case.H, case.psi0, dict(N_max=40, flat=flat))
    for delta in (1j, 0.1):
        out, _ = solver.run(delta, normalize=False)
        assert type(solver.V) is _ops_class(flat) and (not flat or not solver.V.cplx)    # real Krylov vectors whatever delta
        want = case.expm_apply(delta, case.y0)
        assert np.linalg.norm(case.y(out) - want) / np.linalg.norm(want) <= 1e-8, delta


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('combo', ALL)
def test_device_arnoldi_finds_the_dominant_eigenvalue(bb, combo, flat):
    case = dc.SumCase(bb, combo, 5)
    solver = krylov.Arnoldi(bb, case.H, case.psi0, dict(N_max=40, which='LM', flat=flat))
    Es, psis, N = solver.run()
    assert type(solver.V) is _ops_class(flat)
    E, _ = case.spectrum()
    want = E[np.argmax(np.abs(E))]
    assert abs(Es[0] - want) < 1e-8 * abs(want)
    v = case.y(psis[0])
    assert abs(np.linalg.norm(v) - 1.0) < 1e-8 and np.linalg.norm(case.M @ v - Es[0] * v) < 1e-6 * (abs(want) + 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# sparse.gram_schmidt

@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('combo', ALL)
def test_device_gram_schmidt_of_direct_sums_is_one_call_and_one_download(bb, combo, cplx):
    vecs = [dc.SumCase(bb, combo, 10 + k, cplx_vec=cplx).psi0 for k in range(4)]
    vecs.insert(2, ds.linear_combination(bb, 0.5, vecs[0], -2.0, vecs[1]))          # the dependent one
    calls = []
    orig = krylov._FlatOps.orthonormalize

    def spy(self, pools, rcond):
        calls.append(len(pools))
        return orig(self, pools, rcond)

    krylov._FlatOps.orthonormalize = spy
    try:
        with _Count(bb.ctx, 'd2h') as reads, _Count(bb, 'copy_many') as copies:
            out = sparse.gram_schmidt(bb, vecs, rcond=1e-10)
    finally:
        krylov._FlatOps.orthonormalize = orig
    assert calls == [5] and reads.n == 1 and copies.n == 5       # each vector enters its pool once; the flags are read once
    assert len(out) == 4 and all(isinstance(v, DirectSum) for v in out)
    G = np.array([[ds.inner(bb, v, w) for w in out] for v in out])
    assert np.abs(G - np.eye(4)).max() <= 1e-13
    case = dc.SumCase(bb, combo, 10)
    Q = np.array([case.y(v) for v in out])
    for v in vecs:
        y = case.y(v)
        assert np.linalg.norm(y - Q.T @ (Q.conj() @ y)) <= 1e-12 * np.linalg.norm(y)
    # the host-synchronous loop on tensors (what a backend without pools runs) spans the same space
    loop = [v for v in _host_loop(bb, vecs, 1e-10)]
    assert len(loop) == 4
    for v in loop:
        y = case.y(v)
        assert np.linalg.norm(y - Q.T @ (Q.conj() @ y)) <= 1e-12 * np.linalg.norm(y)


def _host_loop(bb, vecs, rcond):
    orig = krylov._flat_usable
    krylov._flat_usable = lambda *_: False
    try:
        return sparse.gram_schmidt(bb, vecs, rcond)
    finally:
        krylov._flat_usable = orig


def test_device_gram_schmidt_threshold_and_single_tensors(bb):
    v = dc.three_four(bb)
    assert sparse.gram_schmidt(bb, [v], rcond=5.0) == []
    kept = sparse.gram_schmidt(bb, [v], rcond=float(np.nextafter(5.0, 0.0)))
    assert len(kept) == 1 and abs(ds.norm(bb, kept[0]) - 1.0) < 1e-15
    t = dc.SumCase(bb, 'abelian+tree').psi0
    for single in t.components:
        q = sparse.gram_schmidt(bb, [single, single], rcond=1e-10)
        assert len(q) == 1 and abs(ds.norm(bb, DirectSum(q)) - 1.0) < 1e-14
