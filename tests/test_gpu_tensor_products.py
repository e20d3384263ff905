"""tensor_outer_many of the HIP block backend (csrc/outer_grouped.hip) and outer / tensor_from_grid / trivial legs of
cyten_amd.abelian on the device, through the C-ABI.

Tolerances.  float64: every element of a tensor product is ONE correctly rounded multiplication on the device and in numpy,
so the results are compared with ``np.array_equal``.  complex128 (and lists mixing real and complex operands): each side
rounds a two-term sum of products per component, error at most 2u (|a_r b_r| + |a_i b_i|) <= 2u |a| |b|, u = 2^-53, and the
device may contract it to an FMA, so the bound is |got - want| <= 4 * 2^-52 * |a| |b| per element.  tensor_from_grid only
moves data: bit-identical.  The exponential of the end-to-end gate keeps the project's line for exp, 1e-10
(tests/test_gpu_tensor_functions.py).  The error cases are argument checks on the host: nothing here hands the device
anything that could fault it."""
import collections
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import tensor_product_ref as ref
from cyten_amd import _lib
from cyten_amd import abelian as ab
from tensor_product_cases import GRID_IDS, OUTER_IDS, dense_of, grid_cases, outer_cases, to_tensor
from test_tensor_products import _dense_grid, as_matrix, bond_hamiltonian, check_heisenberg, check_tfi

pytestmark = pytest.mark.gpu

NP = ref.NumpyOuterBackend()
OUTER = outer_cases()
GRID = grid_cases()
ALL_OUTER = pytest.mark.parametrize('case', range(len(OUTER)), ids=OUTER_IDS)
ALL_GRID = pytest.mark.parametrize('case', range(len(GRID)), ids=GRID_IDS)


class _CountingLib:
    """proxy of the loaded library that counts the C-ABI calls by name"""

    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


@pytest.fixture
def counted(bb, monkeypatch):
    """(C-ABI call counter of bb.lib, list of the sizes of the downloads through bb.ctx.d2h)"""
    lib = _CountingLib(bb.lib)
    monkeypatch.setattr(bb, 'lib', lib)
    downloads, real = [], bb.ctx.d2h

    def d2h(src, n, *args, **kw):
        downloads.append(int(n))
        return real(src, n, *args, **kw)
    monkeypatch.setattr(bb.ctx, 'd2h', d2h)
    return lib, downloads


def _calls(lib):
    return {k: v for k, v in lib.calls.items() if k != 'cyb_last_error'}


def _rand(rng, shape, cplx=False):
    a = np.asarray(rng.standard_normal(shape))
    return a + 1j * np.asarray(rng.standard_normal(shape)) if cplx else a


def _check_list(bb, pairs_np, pairs_dev, K):
    """one tensor_outer_many call against numpy, pair by pair; returns the largest error relative to its bound"""
    got = bb.tensor_outer_many(pairs_dev, K)
    assert len(got) == len(pairs_np)
    cplx = any(np.iscomplexobj(x) for p in pairs_np for x in p)
    worst = 0.0
    for (a, b), g in zip(pairs_np, got):
        assert g.is_contiguous() and g.shape == a.shape[:K] + b.shape + a.shape[K:]
        assert g.is_complex == cplx
        if g.size == 0:
            continue
        g = bb.to_numpy(g)
        want = np.asarray(ref.dense_outer(a, b, K))         # (np.ascontiguousarray would turn a 0-d result into 1-d)
        assert g.shape == want.shape
        assert g.dtype == (np.complex128 if cplx else np.float64)
        if cplx:
            bound = 4 * 2.0 ** -52 * ref.dense_outer(np.abs(a), np.abs(b), K)
            err = np.abs(g - want)
            assert np.all(err <= bound), (a.shape, b.shape, K)
            if err.size and bound.max() > 0:
                worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
        else:
            assert np.array_equal(g, want), (a.shape, b.shape, K)
    return worst


# shapes of (a, b): extents of 1, zero extents, 1-element blocks, odd innermost extents, rank 0, N + M = CYB_MAX_NDIM
SHAPES = [((3, 5), (4,)), ((1, 1), (1,)), ((2, 1, 3), (1, 7)), ((4, 0, 3), (2,)), ((5,), (0, 2)), ((7, 3), (5, 3)),
          ((), (3, 3)), ((6, 5), ()), ((), ()), ((33, 17), (9, 11)), ((2, 3, 2, 3), (3, 2, 3, 2)), ((2, 2, 2, 2, 2, 2, 2), (3,)),
          ((3,), (2, 2, 2, 2, 2, 2, 2)), ((129, 65), (31,)), ((1, 300, 1), (1, 7, 1)), ((2, 2, 2, 2, 2, 2, 2, 2), ())]


@pytest.mark.parametrize('kind', ['f64', 'c128', 'mixed'])
def test_block_level_every_k(bb, kind):
    """every K from 0 to N for every shape pair; one call per (N, K) with all pairs of that N"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for N in sorted({len(sa) for sa, _ in SHAPES}):
        shapes = [(sa, sb) for sa, sb in SHAPES if len(sa) == N]
        for K in range(N + 1):
            pairs = []
            for i, (sa, sb) in enumerate(shapes):
                ca = kind == 'c128' or (kind == 'mixed' and (i + K) % 3 == 0)
                cb = kind == 'c128' or (kind == 'mixed' and (i + K) % 3 == 1)
                pairs.append((_rand(rng, sa, ca), _rand(rng, sb, cb)))
            if kind == 'mixed' and not any(np.iscomplexobj(x) for p in pairs for x in p):
                pairs[0] = (pairs[0][0] + 0j, pairs[0][1])
            worst = max(worst, _check_list(bb, pairs, [(bb.as_block(a), bb.as_block(b)) for a, b in pairs], K))
    print(f'tensor_outer_many {kind}: largest error / bound = {worst:.3f}')


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'mixed'])
def test_large_block_beside_one_element_blocks(bb, cplx):
    """a block of more than 32 MB of output (odd innermost extent) in one list with 1-element blocks"""
    rng = np.random.default_rng(12)
    big = (_rand(rng, (2048, 33)), _rand(rng, (64,)))                   # 2048 x 64 x 33 doubles = 34.6 MB
    assert big[0].size * big[1].size * 8 >= 32 * 2 ** 20
    tiny = [(_rand(rng, (1, 1)), _rand(rng, (1,), cplx and i == 0)) for i in range(5)]
    pairs = tiny[:3] + [big] + tiny[3:] + [(_rand(rng, (3, 1)), _rand(rng, (2,)))]
    worst = _check_list(bb, pairs, [(bb.as_block(a), bb.as_block(b)) for a, b in pairs], 1)
    print(f'large + tiny list: largest error / bound = {worst:.3f}')


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_views_as_operands(bb, cplx):
    """permuted and sliced views (more levels than the contiguous case: the general kernel variant) next to contiguous blocks"""
    rng = np.random.default_rng(13)
    pairs_np, pairs_dev = [], []
    base = _rand(rng, (6, 9, 5, 4), cplx)
    d = bb.as_block(base)
    for perm in ([3, 1, 0, 2], [1, 0, 3, 2], [0, 2, 1, 3]):
        b = _rand(rng, (3, 2))
        pairs_np.append((np.transpose(base, perm), b))
        pairs_dev.append((bb.permute_axes(d, perm), bb.as_block(b)))
    key = (slice(1, 5), slice(2, 9, 2), slice(None), slice(0, 3))
    bsrc = _rand(rng, (8, 7), cplx)
    pairs_np.append((base[key], bsrc[1:6, ::3].T))
    pairs_dev.append((bb.get_item(d, key), bb.permute_axes(bb.get_item(bb.as_block(bsrc), (slice(1, 6), slice(0, 7, 3))), [1, 0])))
    pairs_np.append((_rand(rng, (2, 3, 4, 5)), _rand(rng, (7,))))
    pairs_dev.append(tuple(bb.as_block(x) for x in pairs_np[-1]))
    assert not pairs_dev[0][0].is_contiguous() and not pairs_dev[3][1].is_contiguous()
    for K in range(5):
        _check_list(bb, pairs_np, pairs_dev, K)


def test_empty_list_and_dtype_policy(bb):
    assert bb.tensor_outer_many([], 0) == []
    rng = np.random.default_rng(14)
    a, b = rng.standard_normal((3, 4)), rng.standard_normal((5,))
    with pytest.raises(TypeError, match='boolean'):
        bb.tensor_outer_many([(bb.as_block(a), bb.as_block(b > 0))], 1)
    a32, b32 = bb.to_dtype(bb.as_block(a), 'float32'), bb.to_dtype(bb.as_block(b), 'float32')
    out = bb.tensor_outer_many([(a32, b32)], 1)[0]
    assert out.dtype == np.dtype('float32')
    want = ref.dense_outer(a.astype(np.float32).astype(float), b.astype(np.float32).astype(float), 1)
    assert np.array_equal(bb.to_numpy(out), want.astype(np.float32))   # one product in double precision, rounded once more
    ai, bi = bb.to_dtype(bb.as_block(np.round(4 * a)), 'int64'), bb.to_dtype(bb.as_block(np.round(4 * b)), 'int64')
    out = bb.tensor_outer_many([(ai, bi)], 2)[0]
    assert out.dtype == np.dtype('int64') and np.array_equal(bb.to_numpy(out), ref.dense_outer(np.round(4 * a), np.round(4 * b), 2).astype(np.int64))
    with pytest.raises(ValueError, match='more than 8 axes'):
        bb.tensor_outer_many([(bb.as_block(np.zeros((1,) * 5)), bb.as_block(np.zeros((1,) * 4)))], 0)
    with pytest.raises(ValueError, match='outside'):
        bb.tensor_outer_many([(bb.as_block(a), bb.as_block(b))], 3)


# ------------------------------------------------------------------------------------------- the C-ABI directly

def _record(dst, a, b, K, a_real=1, b_real=1):
    arr = np.zeros(1, dtype=_lib.OUTER_DTYPE)
    arr['dst'], arr['a'], arr['b'] = dst, a.ptr, b.ptr
    arr['n_a'], arr['n_b'], arr['k'] = a.ndim, b.ndim, K
    arr['a_is_real'], arr['b_is_real'] = a_real, b_real
    arr['a_shape'][0, :a.ndim], arr['a_strides'][0, :a.ndim] = a.shape, a.strides
    arr['b_shape'][0, :b.ndim], arr['b_strides'][0, :b.ndim] = b.shape, b.strides
    return arr


def _run(bb, arr, cplx=False):
    fn = bb.lib.cyb_outer_grouped_c128 if cplx else bb.lib.cyb_outer_grouped_f64
    bb.ctx.sync_stream()
    return fn(bb.ctx.handle, arr.ctypes.data_as(C.POINTER(_lib.OuterRec)), len(arr))


@pytest.mark.parametrize('shape_a,shape_b', [((37, 5), (3,)), ((1,), (1,)), ((2,), (1,)), ((301, 7), (11, 3))])
def test_destination_on_an_odd_double(bb, shape_a, shape_b):
    """a float64 destination that is 8 but not 16 bytes aligned: every work item stores its first (and, for an even count,
    its last) element alone and the 16-byte pairs between them; the words around the destination stay untouched"""
    rng = np.random.default_rng(15)
    a, b = rng.standard_normal(shape_a), rng.standard_normal(shape_b)
    n = a.size * b.size
    for lead in (1, 2, 3):
        buf = bb.as_block(np.full(n + lead + 2, -7.0))
        da, db = bb.as_block(a), bb.as_block(b)
        _lib.check(_run(bb, _record(buf.ptr + 8 * lead, da, db, 1)))
        got = bb.to_numpy(buf)
        assert np.all(got[:lead] == -7.0) and np.all(got[lead + n:] == -7.0)
        assert np.array_equal(got[lead:lead + n], ref.dense_outer(a, b, 1).reshape(-1))


def test_argument_checks(bb):
    """host checks only: every bad record is refused before anything is launched"""
    a, b = bb.as_block(np.ones((2, 3))), bb.as_block(np.ones((4,)))
    out = bb.as_block(np.zeros(24))
    good = _record(out.ptr, a, b, 1)
    _lib.check(_run(bb, good))
    assert np.array_equal(bb.to_numpy(out), np.ones(24))
    assert _run(bb, good[:0]) == _lib.CYB_OK                                  # empty list
    for field, value, match in (('n_a', 8, 'axes'), ('n_b', 7, 'axes'), ('n_a', -1, 'axes'), ('k', 3, 'outside'), ('k', -1, 'outside'),
                                ('dst', 0, 'dst is NULL'), ('a', 0, 'a is NULL'), ('b', 0, 'b is NULL'), ('dst', out.ptr + 4, 'misaligned')):
        bad = good.copy()
        bad[field] = value
        status = _run(bb, bad)
        assert status == _lib.CYB_ERR_INVALID, field
        with pytest.raises(ValueError, match=match):
            _lib.check(status)
    bad = good.copy()
    bad['a_shape'][0, 1] = -3
    with pytest.raises(ValueError, match='negative extent'):
        _lib.check(_run(bb, bad))
    zero = good.copy()
    zero['b_shape'][0, 0] = 0
    zero['dst'] = zero['a'] = zero['b'] = 0                                   # a zero extent: nothing is addressed
    assert _run(bb, zero) == _lib.CYB_OK
    cz = _record(out.ptr + 8, a, b, 1, 1, 1)
    with pytest.raises(ValueError, match='misaligned'):                       # a complex destination needs 16 bytes
        _lib.check(_run(bb, cz, cplx=True))
    with pytest.raises(ValueError, match='ctx is NULL'):
        _lib.check(bb.lib.cyb_outer_grouped_f64(None, good.ctypes.data_as(C.POINTER(_lib.OuterRec)), 1))


# ------------------------------------------------------------------------------------------- tensor level

@ALL_OUTER
def test_outer_against_the_stand_in(bb, case):
    c = OUTER[case]
    pair = []
    for backend in (bb, NP):
        a, b = to_tensor(backend, c['a'], c['views']), to_tensor(backend, c['b'], c['views'])
        a.labels, b.labels = list('abcdefg')[:a.nlegs], list('hijklmn')[:b.nlegs]
        pair.append(ab.outer(backend, a, b, {'a': 'x'}, {'h': 'y'}))
    got, want = pair
    assert np.array_equal(got.block_inds, want.block_inds) and got.labels == want.labels and got.num_codomain == want.num_codomain
    got.check_charges()
    assert all(blk.is_contiguous() and blk.shape == got.block_shape(row) for blk, row in zip(got.blocks, got.block_inds))
    A, B = dense_of(c['a']), dense_of(c['b'])
    K = c['a'].num_codomain
    dense = ref.dense_outer(A, B, K)
    if np.iscomplexobj(dense) and not len(got.blocks):
        dense = dense.real
    ref.assert_products_equal(got.to_dense(bb), dense, A, B, K)
    if len(got.blocks):
        assert all(blk.is_complex for blk in got.blocks) == np.iscomplexobj(dense)


@ALL_GRID
def test_grid_against_the_stand_in_and_the_concatenation(bb, case):
    c = GRID[case]
    grids = [[[None if s is None else to_tensor(backend, s, c['views']) for s in row] for row in c['grid']] for backend in (bb, NP)]
    labels = [f'l{k}' for k in range(grids[0][0][0].nlegs)]
    got, want = ab.tensor_from_grid(bb, grids[0], labels=labels), ab.tensor_from_grid(NP, grids[1], labels=labels)
    assert np.array_equal(got.block_inds, want.block_inds) and got.labels == want.labels and got.num_codomain == want.num_codomain
    got.check_charges()
    assert all(blk.is_contiguous() and blk.shape == got.block_shape(row) for blk, row in zip(got.blocks, got.block_inds))
    dense = got.to_dense(bb)
    concat = _dense_grid(c)
    assert dense.dtype == concat.dtype and np.array_equal(dense, concat)
    assert np.array_equal(ab.tensor_from_grid(bb, grids[0]).to_dense(bb), concat)      # (the cached plan)


def test_trivial_legs_are_metadata(bb, counted):
    lib, downloads = counted
    t = to_tensor(bb, OUTER[0]['a'])
    lib.calls.clear()
    u = ab.add_trivial_leg(bb, t, 0, label='w')
    back = ab.squeeze_legs(bb, u)
    assert _calls(lib) == {} and downloads == []
    assert all(x.ptr == y.ptr and x.shape == y.shape for x, y in zip(back.blocks, t.blocks))
    assert np.array_equal(u.to_dense(bb), t.to_dense(bb)[None])


# ------------------------------------------------------------------------------------------- launch structure

def _many_block_pair(bb, rng, nsec):
    sym = ab.Symmetry([0])
    leg = ab.Leg(sym, [[q] for q in range(nsec)], rng.integers(1, 4, nsec), +1)
    inds = np.array([[i, i] for i in range(nsec)])
    return tuple(ab.AbelianTensor.from_numpy_blocks(bb, sym, [leg, leg.dual()], [rng.standard_normal((int(m), int(m))) for m in leg.mults], inds, 1)
                 for _ in range(2))


def test_outer_is_one_launch(bb, counted):
    """one cyb_outer_grouped call whatever the number of block pairs; no GEMM, no copy, no download"""
    lib, downloads = counted
    rng = np.random.default_rng(16)
    counts = []
    for nsec in (6, 12):                                     # 36 and 144 block pairs
        a, b = _many_block_pair(bb, rng, nsec)
        lib.calls.clear()
        del downloads[:]
        res = ab.outer(bb, a, b)
        assert len(res.blocks) == nsec * nsec
        counts.append(_calls(lib))
        assert counts[-1] == {'cyb_outer_grouped_f64': 1} and downloads == []
        assert not any(k.startswith(('cyb_gemm', 'cyb_copy')) for k in counts[-1])
    assert counts[0] == counts[1]
    a, b = _many_block_pair(bb, rng, 5)
    b.blocks = [bb.as_complex(x) for x in b.blocks]
    lib.calls.clear()
    ab.outer(bb, a, b)                                       # real next to complex: no promotion pass
    assert _calls(lib) == {'cyb_outer_grouped_c128': 1}


def test_repeated_grid_reuses_its_plan(bb, counted):
    lib, downloads = counted
    c = GRID[GRID_IDS.index('u1-11-3x3')]
    grid = [[None if s is None else to_tensor(bb, s) for s in row] for row in c['grid']]
    ab.tensor_from_grid(bb, grid)                            # (builds the plan of the structure)
    lib.calls.clear()
    del downloads[:]
    ab.tensor_from_grid(bb, grid)
    calls = _calls(lib)
    assert calls.get('cyb_place_plan_enqueue') == 1 and 'cyb_place_plan_create' not in calls and downloads == []
    assert set(calls) <= {'cyb_place_plan_enqueue', 'cyb_memset'}, calls
    full = GRID[GRID_IDS.index('z2-21-2x3-full')]
    grid = [[to_tensor(bb, s) for s in row] for row in full['grid']]
    ab.tensor_from_grid(bb, grid)
    lib.calls.clear()
    ab.tensor_from_grid(bb, grid)
    print('full grid calls:', _calls(lib))
    assert _calls(lib).get('cyb_place_plan_enqueue') == 1 and 'cyb_place_plan_create' not in _calls(lib)


# ------------------------------------------------------------------------------------------- end to end

def test_tfi_mpo_on_the_device(bb):
    check_tfi(bb)


def test_heisenberg_mpo_on_the_device(bb):
    check_heisenberg(bb)


def test_bond_hamiltonian_on_the_device(bb):
    h, want = bond_hamiltonian(bb)
    assert np.array_equal(as_matrix(h.to_dense(bb)), want)


def test_tebd_gate_from_the_outer_built_bond_term(bb):
    """u = exp(-i dt h) of the Heisenberg bond term built with outer: unitary, and equal to scipy's expm of the np.kron form, both
    to the project's line for exp (1e-10)"""
    J, dt = 0.9, 0.05
    h, dense = ref.heisenberg_bond(bb, J)
    assert np.array_equal(as_matrix(h.to_dense(bb)), dense)
    u = ab.exp(bb, h, -1j * dt)
    uu = ab.compose(bb, ab.dagger(bb, u), u, 2)
    err_unitary = np.abs(as_matrix(uu.to_dense(bb)) - np.eye(4)).max()
    want = scipy.linalg.expm(-1j * dt * dense)
    err = np.abs(as_matrix(u.to_dense(bb)) - want).max() / np.abs(want).max()
    print(f'TEBD gate: |u^dagger u - 1| = {err_unitary:.2e}, |u - expm| / |expm| = {err:.2e}')
    assert err_unitary <= 1e-10 and err <= 1e-10
