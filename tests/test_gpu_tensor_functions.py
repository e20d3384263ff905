"""matrix_exp_many of the HIP block backend (csrc/expm_small.hip and the grouped route for large blocks) and exp / eye /
hermitian_function of cyten_amd.abelian on the device, through the C-ABI.

Tolerance of the exponential: the project's own line for this operation, tests/test_gpu_api_surface.py::test_matrix_exp --
max|got - want| <= 1e-10 max|want| against scipy.linalg.expm, the routine the reference calls (numpy.cpp:1227-1234) -- for the
matrix families of tests/tensor_function_ref.py::families RESTRICTED TO ||A||_1 <= 64 (at most 7 squarings), for which the
numpy restatement of the algorithm stays four orders below that line (tests/test_tensor_functions.py); measured on an MI355X:
at most 9.9e-14 over every case of this file.  The error cases are
argument checks on the host: nothing here hands the device anything that could fault it."""
import collections
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import tensor_function_ref as ref
from cyten_amd import _lib
from cyten_amd import abelian as ab
from tensor_function_cases import CASE_IDS, cases

pytestmark = pytest.mark.gpu

CASES = cases()
ALL_CASES = pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
NP = ref.NumpyExpmBackend()
LIMIT_F64, LIMIT_C128 = _lib.CYB_EXPM_SMALL_MAX_N_F64, _lib.CYB_EXPM_SMALL_MAX_N_C128
TOL = 1e-10


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


def _rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _gauss(rng, n, cplx=False):
    a = rng.standard_normal((n, n)) / np.sqrt(max(n, 1))
    return a + 1j * rng.standard_normal((n, n)) / np.sqrt(max(n, 1)) if cplx else a


# ------------------------------------------------------------------------------------------- accuracy

@pytest.mark.parametrize('n', [1, 2, 7, 16, 33, LIMIT_C128, LIMIT_C128 + 1, LIMIT_F64, LIMIT_F64 + 1, 130])
def test_families_against_scipy(bb, n):
    """every family (||A||_1 <= 64) within 1e-10 max|want| of scipy: the real ones through the float64 entry, all of them
    through the complex entry; the difference to the per-block bb.matrix_exp (same polynomial, other summation order) is
    printed next to the error"""
    rng = np.random.default_rng(500 + n)
    fam = ref.families(rng, n)
    real = [(name, a) for name, a in fam if not np.iscomplexobj(a)]
    for label, sel in (('f64', real), ('c128', fam)):
        got = bb.matrix_exp_many([bb.as_block(a) for _, a in sel])
        for (name, a), g in zip(sel, got):
            g = bb.to_numpy(g)
            assert g.dtype == (np.float64 if label == 'f64' else np.complex128)
            want = scipy.linalg.expm(a)
            err = _rel(g, want)
            one = _rel(bb.to_numpy(bb.matrix_exp(bb.as_block(a))), want) if n in (33, LIMIT_F64, 130) else float('nan')
            print(f'expm n={n} {label} {name}: ||A||_1={np.abs(a).sum(axis=0).max():.3g} err {err:.2e} per-block matrix_exp err {one:.2e}')
            assert err <= TOL, (name, label, err)


def test_reference_case(bb):
    """tests/python_tests/backends/test_torch_block_backend.py::test_matrix_exp of the reference, its own tolerance"""
    a = np.array([[0.3, -1.0], [1.0, 0.5]])
    got = bb.to_numpy(bb.matrix_exp_many([bb.as_block(a)])[0])
    np.testing.assert_allclose(got, scipy.linalg.expm(a), rtol=1e-12, atol=1e-12)


SIZES = [1, 2, 7, 16, 33, LIMIT_C128, LIMIT_C128 + 1, LIMIT_F64, LIMIT_F64 + 1, 97, 212]


def _mixed(bb, rng, kinds):
    """one list over SIZES: per size a block of the next kind of `kinds` ('r' real, 'c' complex, 'v' real permuted view,
    'w' complex permuted view, 'n' None entry); returns (entries, numpy matrices)"""
    entries, mats = [], []
    for i, n in enumerate(SIZES):
        kind = kinds[i % len(kinds)]
        if kind == 'n':
            entries.append((n, None))
            mats.append(np.zeros((n, n)))
            continue
        a = _gauss(rng, n, kind in 'cw')
        if kind in 'vw':
            blk = bb.permute_axes(bb.as_block(np.ascontiguousarray(a.T)), [1, 0])
            assert n < 2 or not blk.is_contiguous()
        else:
            blk = bb.as_block(a)
        entries.append(blk)
        mats.append(a)
    return entries, mats


@pytest.mark.parametrize('kinds,alpha', [('rvn', 1.0), ('rvn', -2.5), ('crwvn', 1.0), ('wcn', 0.7), ('rvn', 0.3 - 1.1j), ('crn', -0.05j)],
                         ids=['real', 'real-alpha', 'mixed', 'complex', 'complex-alpha-on-real', 'gate'])
def test_mixed_list(bb, kinds, alpha):
    """sizes 1 .. 212 in one list (both sides of both limits), real and complex blocks, permuted views, None entries"""
    rng = np.random.default_rng(77)
    entries, mats = _mixed(bb, rng, kinds)
    cplx = isinstance(alpha, complex) or any(np.iscomplexobj(m) for m in mats)
    got = bb.matrix_exp_many(entries, alpha)
    assert len(got) == len(entries)
    for n, m, g in zip(SIZES, mats, got):
        g = bb.to_numpy(g)
        assert g.shape == (n, n) and g.dtype == (np.complex128 if cplx else np.float64)
        want = scipy.linalg.expm(alpha * m)
        err = _rel(g, want)
        print(f'mixed {kinds} alpha={alpha} n={n}: err {err:.2e}')
        assert err <= TOL
    for e, g in zip(entries, got):
        if isinstance(e, tuple):
            assert np.array_equal(bb.to_numpy(g), np.eye(e[0]))


def test_alpha_zero_gives_exact_identities(bb):
    entries, _ = _mixed(bb, np.random.default_rng(5), 'rvn')
    for g, n in zip(bb.matrix_exp_many(entries, 0.0), SIZES):
        g = bb.to_numpy(g)
        assert g.dtype == np.float64 and np.array_equal(g, np.eye(n))
    assert bb.matrix_exp_many([]) == []
    assert bb.to_numpy(bb.matrix_exp_many([(0, None)])[0]).shape == (0, 0)


# ------------------------------------------------------------------------------------------- launch structure

@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_small_list_is_one_launch(bb, counted, cplx):
    lib, downloads = counted
    rng = np.random.default_rng(9)
    limit = LIMIT_C128 if cplx else LIMIT_F64
    blocks = [bb.as_block(_gauss(rng, n, cplx and n % 2 == 0)) for n in (1, 3, 8, 20, 41, limit)] + [(5, None)]
    lib.calls.clear()
    del downloads[:]
    bb.matrix_exp_many(blocks, -0.3j if cplx else 0.9)
    assert _calls(lib) == {'cyb_expm_small_batched_c128' if cplx else 'cyb_expm_small_batched_f64': 1}
    assert downloads == []


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_large_route_calls_do_not_depend_on_the_number_of_blocks(bb, counted, cplx):
    lib, downloads = counted
    rng = np.random.default_rng(10)
    mats = [2.0 * _gauss(rng, n, cplx) for n in (100, 117, 140)]
    counts = []
    for rep in (1, 2):
        blocks = [bb.as_block(m) for m in mats * rep] + [bb.as_block(_gauss(rng, 12, cplx))]
        lib.calls.clear()
        del downloads[:]
        got = bb.matrix_exp_many(blocks)
        counts.append(_calls(lib))
        assert downloads == [3 * rep]                  # the norm table, once
        assert counts[-1]['cyb_norm1_batched_c128' if cplx else 'cyb_norm1_batched_f64'] == 1
        assert counts[-1]['cyb_expm_small_batched_c128' if cplx else 'cyb_expm_small_batched_f64'] == 1
        for m, g in zip(mats * rep, got):
            assert _rel(bb.to_numpy(g), scipy.linalg.expm(m)) <= TOL
    assert counts[0] == counts[1]
    print('large route calls:', counts[0])


def test_norm1_table(bb):
    rng = np.random.default_rng(3)
    mats = [_gauss(rng, 70), _gauss(rng, 131, True), np.zeros((9, 9)), _gauss(rng, 1)]
    blocks = [bb.as_block(m) for m in mats]
    arr = np.zeros(len(mats) + 1, dtype=_lib.EXPM_DTYPE)
    arr['A'][:4] = [b.ptr for b in blocks]
    arr['n'][:4] = arr['lda'][:4] = [m.shape[0] for m in mats]
    arr['a_is_real'][:4] = [0 if np.iscomplexobj(m) else 1 for m in mats]
    arr['n'][4] = 6                                      # A == NULL: the zero matrix
    table = bb.ctx.empty(5)
    bb.ctx.sync_stream()
    _lib.check(bb.lib.cyb_norm1_batched_c128(bb.ctx.handle, arr.ctypes.data_as(C.POINTER(_lib.ExpmDesc)), 5, C.c_void_p(table.data_ptr())))
    got = bb.ctx.d2h(table, 5, np.float64)
    want = [np.abs(m).sum(axis=0).max() for m in mats] + [0.0]
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------- error cases (host checks only)

def test_argument_checks(bb):
    big = bb.as_block(np.zeros((LIMIT_F64 + 1, LIMIT_F64 + 1)))
    out = bb.as_block(np.zeros((LIMIT_F64 + 1, LIMIT_F64 + 1), dtype=complex))
    arr = np.zeros(1, dtype=_lib.EXPM_DTYPE)
    arr['A'], arr['E'], arr['a_is_real'] = big.ptr, out.ptr, 1
    descs = arr.ctypes.data_as(C.POINTER(_lib.ExpmDesc))
    bb.ctx.sync_stream()
    for n, fn, args in ((LIMIT_F64 + 1, bb.lib.cyb_expm_small_batched_f64, (1.0,)),
                        (LIMIT_C128 + 1, bb.lib.cyb_expm_small_batched_c128, (1.0, 0.0))):
        arr['n'] = arr['lda'] = arr['lde'] = n
        with pytest.raises(ValueError, match='exceeds the limit'):
            _lib.check(fn(bb.ctx.handle, descs, 1, *args))
    arr['n'] = arr['lda'] = 8
    arr['lde'] = 7
    with pytest.raises(ValueError, match='lde'):
        _lib.check(bb.lib.cyb_expm_small_batched_f64(bb.ctx.handle, descs, 1, 1.0))
    arr['lde'], arr['n'] = 8, -1
    with pytest.raises(ValueError):
        _lib.check(bb.lib.cyb_expm_small_batched_f64(bb.ctx.handle, descs, 1, 1.0))
    with pytest.raises(ValueError):
        bb.matrix_exp_many([bb.as_block(np.zeros((3, 4)))])
    with pytest.raises(ValueError):
        bb.matrix_exp_many([bb.as_block(np.zeros(3))])
    with pytest.raises(ValueError):
        bb.matrix_exp_many([bb.as_block(np.zeros((2, 2), dtype=bool))])
    with pytest.raises(ValueError):
        bb.matrix_exp_many([(3, 'zero')])
    with pytest.raises(ValueError):
        bb.matrix_exp_many([bb.as_block(np.full((LIMIT_F64 + 4, LIMIT_F64 + 4), np.inf))])


# ------------------------------------------------------------------------------------------- tensor level

def _pair(bb, case):
    spec = case['tensor']
    return ab.AbelianTensor.from_spec(bb, spec), ab.AbelianTensor.from_spec(NP, spec)


def _dense_close(bb, got, want, tol=TOL):
    g = got.to_dense(bb)
    assert g.shape == want.shape
    assert np.abs(g - want).max() <= tol * np.abs(want).max()


def _hermitian(bb, t):
    return ab.linear_combination(bb, 0.5, t, 0.5, ab.dagger(bb, t))


@pytest.mark.parametrize('factor', [1.0, 0.3 - 0.4j], ids=['real', 'complex'])
@ALL_CASES
def test_exp_against_the_stand_in(bb, case, factor):
    td, tn = _pair(bb, CASES[case])
    td.labels = tn.labels = [f'l{i}' for i in range(td.nlegs)]
    got, want = ab.exp(bb, td, factor), ab.exp(NP, tn, factor)
    assert np.array_equal(got.block_inds, want.block_inds) and got.labels == want.labels and got.num_codomain == want.num_codomain
    _dense_close(bb, got, want.to_dense(NP))
    if isinstance(factor, complex):
        assert all(b.is_complex for b in got.blocks)


@ALL_CASES
def test_exp_is_the_power_series(bb, case):
    """exp(t) for |t| <= 1/4 against sum_{j <= 12} t^j / j! built from compose, linear_combination and eye only: pins the
    leg convention without any reference (the remainder is below (1/4)^13 / 13! < 3e-18)"""
    c = CASES[case]
    td, _ = _pair(bb, c)
    k = c['k']
    nrm = ab.norm(bb, td)
    t = ab.scale(bb, 0.25 / nrm, td) if nrm > 0 else td
    series = ab.eye(bb, t.symmetry, t.legs[:k])
    power, fact = None, 1.0
    for j in range(1, 13):
        power = t if power is None else ab.compose(bb, power, t, k)
        fact *= j
        if len(power.blocks):
            series = ab.linear_combination(bb, 1.0, series, 1.0 / fact, power)
    _dense_close(bb, ab.exp(bb, t), series.to_dense(bb), 1e-12)


@ALL_CASES
def test_exp_identities(bb, case):
    c = CASES[case]
    td, _ = _pair(bb, c)
    k = c['k']
    one = ab.eye(bb, td.symmetry, td.legs[:k]).to_dense(bb)
    _dense_close(bb, ab.compose(bb, ab.exp(bb, td), ab.exp(bb, td, -1.0), k), one)
    h = _hermitian(bb, td)
    u = ab.exp(bb, h, 1j)
    _dense_close(bb, ab.compose(bb, ab.dagger(bb, u), u, k), one)
    _dense_close(bb, ab.hermitian_function(bb, h, 'exp'), ab.exp(bb, h).to_dense(bb))
    pos = ab.exp(bb, h)
    r = ab.hermitian_function(bb, pos, 'sqrt')
    _dense_close(bb, ab.compose(bb, r, r, k), pos.to_dense(bb))


def test_tensor_level_launches(bb, counted):
    """exp of a tensor whose sectors all fit the kernel: ONE exponential launch, no download; hermitian_function: a number of
    launches that does not depend on the number of sectors"""
    lib, downloads = counted
    for name in ('u1-r4', 'u1u1-r4-missing'):
        td, _ = _pair(bb, CASES[CASE_IDS.index(name)])
        h = _hermitian(bb, td)
        ab.exp(bb, h)                                   # (builds the placement plans of the structure)
        lib.calls.clear()
        del downloads[:]
        ab.exp(bb, h)
        calls = _calls(lib)
        assert calls.get('cyb_expm_small_batched_f64') == 1 and downloads == []
        assert not any(k.startswith(('cyb_gemm', 'cyb_norm1')) for k in calls)
        lib.calls.clear()
        ab.hermitian_function(bb, h, 'square')
        calls = _calls(lib)
        for fn in ('cyb_eigh_batched_f64', 'cyb_unary_batched_f64', 'cyb_scale_axis_batched_f64', 'cyb_gemm_grouped_enqueue_f64'):
            assert calls.get(fn) == 1, (fn, calls)
