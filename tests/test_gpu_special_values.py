"""NaN, +-Inf, signed zeros and values near the ends of the double range through HipBlockBackend and the C-ABI: the cases
of special_value_cases.py against numpy's answers (the reference's NumpyBlockBackend is numpy).  Non-finite results are
compared by class, zeros by sign, finite results against mpmath within the bounds recorded in special_value_cases.py.

Part D (decompositions of blocks with non-finite entries) is the `test_nonfinite_...` group: run it in an invocation of
its own (``-k test_nonfinite``) ahead of the rest.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

import special_value_cases as sv
from cyten_amd import _lib

pytestmark = pytest.mark.gpu


# ---- A. reductions, extrema, comparisons ------------------------------------------------------------------------------------
def _layouts(bb, v):
    """the same data as a contiguous vector, as a view starting at an odd element (8-byte aligned only) and as a 2-D block"""
    n = len(v)
    parent = bb.as_block(np.concatenate([[123.0], v]))
    return [('vector', bb.as_block(v), v), ('odd view', bb.get_item(parent, (slice(1, n + 1),)), v),
            ('2-d', bb.as_block(v.reshape(sv.SHAPE_2D[n])), v.reshape(sv.SHAPE_2D[n]))]


@pytest.mark.parametrize('n', sv.REDUCTION_LENGTHS)
def test_reductions_and_extrema_follow_numpy(bb, n):
    w = np.random.default_rng(5).standard_normal(n)
    for name, v in sv.reduction_vectors(n):
        for lname, blk, arr in _layouts(bb, v):
            what = f'n={n} {name} {lname}'
            wblk = bb.as_block(w.reshape(arr.shape))
            want = sv.reduction_expectations(arr, w.reshape(arr.shape))
            sv.check_scalar(bb.max_abs(blk), want['max_abs'], 0.0, what + ': max_abs')
            # (a maximum over zeros of both signs: numpy's own answer is +0 or -0 depending on the vector length, so only the value)
            for key, got in (('max', bb.max(blk)), ('min', bb.min(blk))):
                if want[key] == 0.0:
                    assert got == 0.0, what + ': ' + key
                else:
                    sv.check_scalar(got, want[key], 0.0, what + ': ' + key)
            assert bb.abs_argmax(blk) == want['abs_argmax'], what + ': abs_argmax'
            assert bb.argmin(blk) == want['argmin'], what + ': argmin'
            # sums of n terms: n 2^-52 times the sum of the magnitudes (any summation order); the 2-norm: the same on the squares
            sv.check_scalar(bb.norm(blk), want['norm2'], n * sv.EPS * abs(want['norm2']), what + ': norm 2')
            sv.check_scalar(bb.norm(blk, 1), want['norm1'], n * sv.EPS * abs(want['norm1']), what + ': norm 1')
            sv.check_scalar(bb.norm(blk, np.inf), want['norminf'], 0.0, what + ': norm inf')
            sv.check_scalar(bb.sum_all(blk), want['sum_all'], n * sv.EPS * want['sum_abs'], what + ': sum_all')
            sv.check_scalar(bb.inner(blk, wblk, True), want['inner'], n * sv.EPS * want['inner_abs'], what + ': inner')


def test_max_abs_many_and_complex_blocks(bb, rng):
    healthy = [rng.standard_normal(s) for s in ((300,), (17, 5), (8193,))]
    assert bb.max_abs_many([bb.as_block(x) for x in healthy]) == max(np.abs(x).max() for x in healthy)
    for pos in (0, 4096, 8192):   # the NaN in the last block of the list, in its first and in its second work item
        bad = [x.copy() for x in healthy]
        bad[2][pos] = np.nan
        assert np.isnan(bb.max_abs_many([bb.as_block(x) for x in bad])), pos
        bad[2][pos] = -np.inf
        assert bb.max_abs_many([bb.as_block(x) for x in bad]) == np.inf
    z = rng.standard_normal(301) + 1j * rng.standard_normal(301)
    assert abs(bb.max_abs(bb.as_block(z)) - np.abs(z).max()) <= 2 * sv.EPS * np.abs(z).max()
    for pos in (0, 150, 300):     # NaN in the imaginary part only
        zz = z.copy()
        zz[pos] = complex(zz[pos].real, np.nan)
        assert np.isnan(bb.max_abs(bb.as_block(zz))), pos
        assert np.isnan(bb.max_abs_many([bb.as_block(z), bb.as_block(healthy[0]), bb.as_block(zz)])), pos


@pytest.mark.parametrize('n', sv.REDUCTION_LENGTHS)
def test_comparisons_follow_numpy(bb, n):
    rng = np.random.default_rng(9 + n)
    for name, v in sv.reduction_vectors(n):
        if not (name.endswith('@0') or name.endswith('@-1') or name in ('plain', 'all-nan', '-0,+0')):
            continue
        other = v.copy()
        flip = rng.random(n) < 0.5
        other[flip] = rng.standard_normal(int(flip.sum()))       # half equal (NaN against NaN, Inf against Inf), half not
        scalar = float(v[np.isfinite(v)][0]) if np.isfinite(v).any() else 0.0
        a, b = bb.as_block(v), bb.as_block(other)
        for k, op in enumerate(sv.COMPARE_OPS):
            for rhs_dev, rhs in ((b, other), (scalar, scalar), (np.inf, np.inf)):
                want = sv.np_eval(sv.NP_COMPARE[op], v, rhs)
                got = bb._compare(a, rhs_dev, k)
                what = f'n={n} {name} {op}'
                assert np.array_equal(bb.to_numpy(got), want), what
                assert bb.any(got) == bool(want.any()) and bb.all(got) == bool(want.all()), what
                assert bb.sum_all(got) == int(want.sum()), what
        nan_here = np.isnan(v)
        if nan_here.any():   # != is True on NaN, every other comparison False
            assert bb.to_numpy(a != a)[nan_here].all() and not bb.to_numpy(a == a)[nan_here].any()
            assert not bb.to_numpy(a <= a)[nan_here].any() and not bb.to_numpy(a >= a)[nan_here].any()


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('shape', [(1,), (37, 21), (8193,)])
def test_allclose_is_numpys_elementwise_rule(bb, shape, cplx):
    for name, a, b, rtol, atol, want in sv.allclose_cases(shape, cplx):
        A, B = bb.as_block(a), bb.as_block(b)
        assert bb.allclose(A, B, rtol, atol) is want, f'{shape} {name}: contiguous'
        if len(shape) == 2:   # permuted views of transposed storage: the same elements, another layout
            At = bb.permute_axes(bb.as_block(np.ascontiguousarray(a.T)), [1, 0])
            Bt = bb.permute_axes(bb.as_block(np.ascontiguousarray(b.T)), [1, 0])
            assert bb.allclose(At, B, rtol, atol) is want, f'{shape} {name}: permuted a'
            assert bb.allclose(At, Bt, rtol, atol) is want, f'{shape} {name}: permuted both'
        if not cplx:          # a real block against a complex one
            assert bb.allclose(A, bb.as_block(b.astype(np.complex128)), rtol, atol) is want, f'{shape} {name}: mixed dtypes'


def test_allclose_count_at_the_c_abi(bb, rng):
    """cyb_allclose_count returns the NUMBER of failing elements; a zero-length call reports none"""
    a = rng.standard_normal(5000)
    b = a.copy()
    bad = [0, 1, 255, 256, 2047, 2048, 4999]
    b[bad] += 1.0
    b[7], a[9] = np.nan, np.inf
    A, B = bb.as_block(a), bb.as_block(b)
    res = bb.ctx.empty(1, 'int64')
    bb.ctx.sync_stream()
    for n, want in ((5000, len(bad) + 2), (0, 0), (256, 5)):
        _lib.check(bb.lib.cyb_allclose_count(bb.ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), n, 0, 1e-5, 1e-8,
                                             C.c_void_p(res.data_ptr())))
        assert int(bb.ctx.d2h(res, 1, np.int64)[0]) == want
    assert bb.lib.cyb_allclose_count(bb.ctx.handle, None, C.c_void_p(B.ptr), 4, 0, 1e-5, 1e-8,
                                     C.c_void_p(res.data_ptr())) == _lib.CYB_ERR_INVALID


def test_seg_reduce_max_min_skip_nan_as_documented(bb):
    """cyb_seg_reduce MAX / MIN are fmax / fmin reductions: a NaN is skipped wherever it stands (unlike np.max, on
    purpose: DESIGN.md 4.12)"""
    segs = [np.array([np.nan, 2.0, -3.0, 1.0]), np.array([2.0, np.nan, -3.0, 1.0]), np.array([2.0, -3.0, 1.0, np.nan]),
            np.array([np.inf, np.nan, -np.inf])]
    blocks = [bb.as_block(s) for s in segs]
    mx = bb.seg_reduce_many(blocks, [len(s) for s in segs], 'max')[:, 0]
    mn = bb.seg_reduce_many(blocks, [len(s) for s in segs], 'min')[:, 0]
    with np.errstate(all='ignore'):
        sv.assert_bits_equal(mx, np.array([np.fmax.reduce(s) for s in segs]), 'seg max')
        sv.assert_bits_equal(mn, np.array([np.fmin.reduce(s) for s in segs]), 'seg min')
    assert list(mx[:3]) == [2.0, 2.0, 2.0] and list(mn[:3]) == [-3.0, -3.0, -3.0] and mx[3] == np.inf and mn[3] == -np.inf


# ---- B. real elementwise ops ---------------------------------------------------------------------------------------------------
def _run_list(bb, fn, xs, ys=None, extra=()):
    """one C-ABI call on a LIST of contiguous float64 blocks; returns the outputs as numpy arrays"""
    X = [bb.as_block(x) for x in xs]
    Y = [bb.as_block(y) for y in ys] if ys is not None else None
    outs = [bb._new(x.shape) for x in xs]
    bb.ctx.sync_stream()
    _lib.check(fn(bb.ctx.handle, bb._vec_descs(X, Y, outs), len(X), *extra))
    return [bb.to_numpy(o) for o in outs]


def _check_real(name, got, want, inputs, mp_fn=None, ulp_bound=None):
    finite = sv.assert_same_class(got, want, name)
    if ulp_bound is None:
        sv.assert_bits_equal(got, want, name)
        return 0.0
    sel = np.flatnonzero(finite)
    err = sv.ulp_errors(got[sel], [mp_fn(*[arr[i] for arr in inputs]) for i in sel])
    worst = float(err.max()) if len(sel) else 0.0
    print(f'{name}: worst error {worst:.3f} ulp (bound {ulp_bound})' + (f' all: {np.round(err, 2).tolist()}' if 0 < len(sel) <= 16 else ''))
    assert worst <= ulp_bound, f'{name}: {worst} ulp at {[arr[sel[int(err.argmax())]] for arr in inputs]}'
    return worst


@pytest.mark.parametrize('n', sv.REAL_LENGTHS)
def test_real_unary_ops_follow_numpy(bb, n):
    xs = [sv.real_vector(n, s) for s in (0, 31, 77)]
    bounds = {'exp': sv.GPU_EXP_ULP, 'log': sv.GPU_LOG_ULP}
    for name, np_fn in sv.REAL_UNARY.items():
        code = sv.REAL_UNARY_OPCODE[name]
        single = {'abs': bb.abs, 'sqrt': bb.sqrt, 'exp': bb.exp, 'log': bb.log}.get(name, lambda a: bb._unary(a, code))
        got_list = _run_list(bb, bb.lib.cyb_unary_batched_f64, xs, None, (code,))
        for k, x in enumerate(xs):
            want = sv.np_eval(np_fn, x)
            mp_fn = (lambda v, nm=name: sv.mp_real(nm, v)) if name in bounds else None
            _check_real(f'{name} n={n} list[{k}]', got_list[k], want, (x,), mp_fn, bounds.get(name))
            if k == 0:
                _check_real(f'{name} n={n} single', bb.to_numpy(single(bb.as_block(x))), want, (x,), mp_fn, bounds.get(name))


@pytest.mark.parametrize('n', sv.REAL_LENGTHS)
def test_real_binary_ops_follow_numpy(bb, n):
    """the grid against a rotated copy of itself: Inf - Inf, 0 * Inf, 0 / 0, x / 0 with both zero signs, overflow, underflow"""
    shifts = (0, 31, 77)
    xs = [sv.real_vector(n, s) for s in shifts]
    ys = [sv.real_vector(n, s + 13 + 3 * k) for k, s in enumerate(shifts)]
    for name, np_fn in sv.REAL_BINARY.items():
        code = sv.REAL_BINARY_OPCODE[name]
        got_list = _run_list(bb, bb.lib.cyb_binary_batched_f64, xs, ys, (code,))
        for k, (x, y) in enumerate(zip(xs, ys)):
            _check_real(f'{name} n={n} list[{k}]', got_list[k], sv.np_eval(np_fn, x, y), (x, y))
        got = bb.to_numpy(bb._binary(bb.as_block(xs[0]), bb.as_block(ys[0]), code))
        _check_real(f'{name} n={n} single', got, sv.np_eval(np_fn, xs[0], ys[0]), (xs[0], ys[0]))


def test_real_binary_ops_meet_the_indeterminate_forms(bb):
    x = np.array([np.inf, np.inf, 0.0, -0.0, 0.0, -0.0, 1.0, 1.0, -1.0, -1.0, np.nan, sv.DBL_MAX, 5e-324, np.inf, 0.0])
    y = np.array([np.inf, -np.inf, np.inf, np.inf, 0.0, 0.0, 0.0, -0.0, 0.0, -0.0, 1.0, sv.DBL_MAX, 0.5, 0.0, -0.0])
    for name, np_fn in sv.REAL_BINARY.items():
        got = bb.to_numpy(bb._binary(bb.as_block(x), bb.as_block(y), sv.REAL_BINARY_OPCODE[name]))
        _check_real(name, got, sv.np_eval(np_fn, x, y), (x, y))


def test_cutoff_inverse_stable_log_and_angle_follow_numpy(bb):
    for a, cutoff in sv.cutoff_cases():
        A = bb.as_block(a)
        _check_real(f'cutoff_inverse {cutoff}', bb.to_numpy(bb.cutoff_inverse(A, cutoff)), sv.np_cutoff_inverse(a, cutoff), (a,))
        _check_real(f'stable_log {cutoff}', bb.to_numpy(bb.stable_log(A, cutoff)), sv.np_stable_log(a, cutoff), (a,),
                    lambda v: sv.mp_real('log', v), sv.GPU_LOG_ULP)
    for n in sv.REAL_LENGTHS:
        x = sv.real_vector(n, 5)
        _check_real(f'cutoff_inverse grid n={n}', bb.to_numpy(bb.cutoff_inverse(bb.as_block(x), 1e-12)), sv.np_cutoff_inverse(x, 1e-12), (x,))
        _check_real(f'stable_log grid n={n}', bb.to_numpy(bb.stable_log(bb.as_block(x), 1e-12)), sv.np_stable_log(x, 1e-12), (x,),
                    lambda v: sv.mp_real('log', v), sv.GPU_LOG_ULP)
        # angle of reals: 0 for x >= +0, pi for negative x and for -0.0, NaN for NaN (np.angle is arctan2(0, x))
        _check_real(f'angle n={n}', bb.to_numpy(bb.angle(bb.as_block(x))), sv.np_eval(np.angle, x), (x,))


@pytest.mark.parametrize('as_block', [True, False])
def test_pow_follows_numpy(bb, as_block):
    """x ** y as a binary op (exponent block) and with a scalar exponent"""
    def power(x, y):
        if as_block:
            return bb.to_numpy(bb._pow(bb.as_block(x), bb.as_block(y)))
        out = np.empty(len(x))
        for e in np.unique(y[~np.isnan(y)]):
            sel = y == e
            out[sel] = bb.to_numpy(bb._pow(bb.as_block(x[sel]), float(e)))
        for i in np.flatnonzero(np.isnan(y)):
            out[i] = bb.to_numpy(bb._pow(bb.as_block(x[i:i + 1]), float('nan')))[0]
        return out

    b, e = sv.pow_exact_cases()                       # the reference's own test (4 ** 3 == 64) and every exact b ** e
    _check_real('exact b ** e', power(b, e), sv.np_eval(np.power, b, e), (b, e))
    x, y = (np.array(v) for v in zip(*sv.POW_SPECIAL))
    _check_real('special x ** y', power(x, y), sv.np_eval(np.power, x, y), (x, y))
    x, y = (np.array(v) for v in zip(*sv.POW_LIBM))   # beyond |y| = 4096, fractional exponents: the library's pow()
    _check_real('pow() cases', power(x, y), sv.np_eval(np.power, x, y), (x, y), sv.mp_pow, sv.GPU_POW_ULP)
    x, y = sv.pow_chain_cases()                       # the squaring chain: |relative error| <= |y| 2^-52
    got = power(x, y)
    with sv.mp_ctx():
        rel = np.array([float(abs(mpmath.mpf(float(g)) - sv.mp_pow(a, b_)) / abs(sv.mp_pow(a, b_))) for g, a, b_ in zip(got, x, y)])
    nz = y != 0
    print(f'squaring chain: worst relative error / (|y| 2^-52) = {(rel[nz] / (np.abs(y[nz]) * sv.EPS)).max():.4f}')
    assert (rel <= np.abs(y) * sv.EPS).all(), f'chain: worst {(rel[nz] / (np.abs(y[nz]) * sv.EPS)).max()} x |y| 2^-52'


# ---- C. complex elementwise ops ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['abs', 'sqrt', 'exp', 'log', 'angle'])
def test_complex_unary_ops_follow_numpy(bb, name):
    z = sv.COMPLEX_GRID
    want = sv.np_eval(sv.COMPLEX_UNARY[name], z)
    fn = {'abs': bb.abs, 'sqrt': bb.sqrt, 'exp': bb.exp, 'log': bb.log, 'angle': bb.angle}[name]
    got = bb.to_numpy(fn(bb.as_block(z)))
    assert got.dtype == want.dtype
    err = sv.complex_error_units(name, got, want, z)
    print(f'complex {name}: worst error {err.max():.3f} units at {z[int(err.argmax())]} (bound {sv.GPU_C_ERR[name]})')
    sv.assert_same_class(got, want, f'complex {name}')
    worst = np.argsort(err)[::-1][:6]
    assert err.max() <= sv.GPU_C_ERR[name], f'complex {name}: ' + '; '.join(f'{err[i]:.3g} units at {z[i]}: got {got[i]}, numpy {want[i]}' for i in worst)


def test_complex_products_follow_numpy(bb):
    z, w = sv.COMPLEX_GRID, sv.complex_partner()
    want = sv.np_eval(np.multiply, z, w)
    got = bb.to_numpy(bb.multiply_blocks(bb.as_block(z), bb.as_block(w)))
    finite = sv.assert_same_class(got, want, 'complex product')
    bre, bim = sv.complex_product_bounds(z, w)
    fr, fi = np.isfinite(want.real) & (want.real != 0), np.isfinite(want.imag) & (want.imag != 0)
    assert (np.abs(got.real - want.real)[fr] <= bre[fr] + sv.DENORM_MIN).all()
    assert (np.abs(got.imag - want.imag)[fi] <= bim[fi] + sv.DENORM_MIN).all()
    assert (fr | fi).sum() >= 50


def test_complex_quotients_follow_numpy(bb):
    z, w = sv.COMPLEX_GRID, sv.complex_partner()
    keep = ~sv.complex_div_dropped(w)
    z, w = z[keep], w[keep]
    want = sv.np_eval(np.divide, z, w)
    got = bb.to_numpy(bb._binary(bb.as_block(z), bb.as_block(w), 3))
    err = sv.complex_error_units('div', got, want, z, w)
    print(f'complex div: worst error {err.max():.3f} units at {z[int(err.argmax())]} / {w[int(err.argmax())]} (bound {sv.GPU_C_ERR["div"]})')
    sv.assert_same_class(got, want, 'complex quotient')
    assert err.max() <= sv.GPU_C_ERR['div']


# ---- D'. GEMM and matrix exponential with non-finite entries -------------------------------------------------------------------
def _gemm_bound(a, b):
    """the bound of the GEMM tests: K 2^-52 |A| |B| per entry (any summation order, FMA or not)"""
    return a.shape[1] * sv.EPS * (np.abs(a) @ np.abs(b)) + sv.DENORM_MIN


@pytest.mark.parametrize('m,n,k', sv.GEMM_NONFINITE_SHAPES)
def test_gemm_propagates_nonfinite_entries_into_their_rows_only(bb, m, n, k):
    rng = np.random.default_rng(m + n + k)
    a, b = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    ref, bound = a @ b, _gemm_bound(a, b)
    for i, kk in ((0, 0), (m // 2, k // 3), (m - 1, k - 1)):
        others = np.arange(m) != i
        bad = a.copy()
        bad[i, kk] = np.nan
        c, = bb.matrix_dot_grouped([[(bb.as_block(bad), bb.as_block(b))]])
        c = bb.to_numpy(c)
        assert np.isnan(c[i]).all(), f'NaN at A[{i},{kk}]: row {i} must be NaN'
        assert (np.abs(c[others] - ref[others]) <= bound[others]).all(), f'NaN at A[{i},{kk}] leaked into other rows'
        # +Inf against a row of B that is half zeros: NaN where B[k, j] == 0, +-Inf elsewhere
        bad[i, kk] = np.inf
        bz = b.copy()
        bz[kk, ::2] = 0.0
        c, = bb.matrix_dot_grouped([[(bb.as_block(bad), bb.as_block(bz))]])
        c = bb.to_numpy(c)
        want = sv.np_eval(np.matmul, bad, bz)
        sv.assert_same_class(c[i], want[i], f'Inf at A[{i},{kk}]: row {i}')
        assert np.isnan(c[i, ::2]).all() and np.isinf(c[i, 1::2]).all()
        refz, boundz = a @ bz, _gemm_bound(a, bz)
        assert (np.abs(c[others] - refz[others]) <= boundz[others]).all(), f'Inf at A[{i},{kk}] leaked into other rows'


@pytest.mark.parametrize('M,N,Ks', [(33, 47, (33, 2, 48)), (5, 2049, (3, 10, 7))])
def test_gemm_k_split_group_propagates_nonfinite_entries(bb, M, N, Ks):
    """K-split groups of tests/gemm_guard_cases.py (several (a, b) pairs summed into one output; SMALL_SHAPES x SMALL_KS and
    a skinny_specs() case of the streaming kernel): a NaN in any one pair's A reaches its row, and only that row"""
    import gemm_guard_cases as gg
    assert (M, N) in gg.SMALL_SHAPES + [(5, 2049)] and Ks in gg.SMALL_KS + [(3, 10, 7)]
    rng = np.random.default_rng(3)
    pairs = [(rng.standard_normal((M, k)), rng.standard_normal((k, N))) for k in Ks]
    ref = sum(a @ b for a, b in pairs)
    bound = sum(_gemm_bound(a, b) for a, b in pairs) + len(pairs) * sv.EPS * np.abs(ref)
    row = M // 2
    others = np.arange(M) != row
    for which in range(len(pairs)):
        bad = [(a.copy(), b) for a, b in pairs]
        bad[which][0][row, Ks[which] - 1] = np.nan
        out, = bb.matrix_dot_grouped([[(bb.as_block(a), bb.as_block(b)) for a, b in bad]])
        c = bb.to_numpy(out)
        assert np.isnan(c[row]).all() and (np.abs(c[others] - ref[others]) <= bound[others]).all(), which


# ---- E. random generators --------------------------------------------------------------------------------------------------------
GUARD = 8
SENTINEL = -6.02214076e+123


def _fill_random(bb, n, seed, uniform, p0, p1=None):
    """the C-ABI generator on a buffer of n elements followed by a guard band of sentinels; returns (values, guard)"""
    buf = bb.as_block(np.full(n + GUARD, SENTINEL))
    bb.ctx.sync_stream()
    if uniform:
        _lib.check(bb.lib.cyb_random_uniform_f64(bb.ctx.handle, C.c_void_p(buf.ptr), n, C.c_uint64(seed), p0, p1))
    else:
        _lib.check(bb.lib.cyb_random_normal_f64(bb.ctx.handle, C.c_void_p(buf.ptr), n, C.c_uint64(seed), p0))
    out = bb.to_numpy(buf)
    return out[:n], out[n:]


@pytest.mark.parametrize('seed', sv.UNIFORM_SEEDS)
def test_random_uniform_is_the_philox_model_bit_for_bit(bb, seed):
    for n in sv.UNIFORM_LENGTHS:
        for lo, hi in sv.UNIFORM_RANGES:
            got, guard = _fill_random(bb, n, seed, True, lo, hi)
            sv.assert_bits_equal(got, sv.model_uniform(n, seed, lo, hi), f'uniform n={n} seed={seed} [{lo}, {hi})')
            assert (guard == SENTINEL).all(), f'uniform n={n}: wrote behind the buffer'
    # through the backend: [-1, 1)
    if seed < 2 ** 63:
        got = bb.to_numpy(bb.random_uniform([4097], seed=seed))
        sv.assert_bits_equal(got, sv.model_uniform(4097, seed, -1.0, 1.0), 'bb.random_uniform')


@pytest.mark.parametrize('n,seed,sigma', [(1, 0, 1.0), (2, 7, 1.0), (3, 7, 2.5), (511, 2 ** 32 + 5, 1.0), (1024, 2 ** 64 - 1, 0.5)])
def test_random_normal_is_box_muller_of_the_model_uniforms(bb, n, seed, sigma):
    got, guard = _fill_random(bb, n, seed, False, sigma)
    want, rad = sv.model_normal(n, seed, sigma)
    err = np.abs(got - want) / (sv.EPS * rad + sv.DENORM_MIN)
    print(f'normal n={n}: worst error {err.max():.3f} units of 2^-52 rad (bound {sv.BOX_MULLER_C})')
    assert (guard == SENTINEL).all(), f'normal n={n}: wrote behind the buffer (odd n writes no element n)'
    assert err.max() <= sv.BOX_MULLER_C


def test_random_streams_are_separate_and_prefix_stable(bb):
    u7, _ = _fill_random(bb, 4097, 7, True, 0.0, 1.0)
    u8, _ = _fill_random(bb, 4097, 8, True, 0.0, 1.0)
    n7, _ = _fill_random(bb, 4097, 7, False, 1.0)
    n8, _ = _fill_random(bb, 4097, 8, False, 1.0)
    assert not np.array_equal(u7, u8) and not np.array_equal(n7, n8) and len(np.unique(u7)) == 4097
    # the normal stream of a seed is not the Box-Muller transform of its uniform stream
    want, _ = sv.model_normal(64, 7, 1.0)
    a, b = u7[0:64:2], u7[1:64:2]
    with np.errstate(all='ignore'):
        from_uniform = np.sqrt(-2 * np.log(np.where(a > 0, a, 1.0))) * np.cos(2 * np.pi * b)
    assert np.abs(from_uniform - n7[0:64:2]).max() > 1e-3 and np.abs(want - n7[:64]).max() < 1e-12
    # the first 4097 values do not depend on n
    for n in (4098, 8193, 20001):
        assert np.array_equal(_fill_random(bb, n, 7, True, 0.0, 1.0)[0][:4097], u7)
        assert np.array_equal(_fill_random(bb, n, 7, False, 1.0)[0][:4097], n7)


# ---- D. decompositions and matrix exponential of blocks with non-finite entries -----------------------------------------------
# Every route's iteration count is bounded by a constant (40 or 80 sweeps, device waits leave on integer tickets or a
# one-second clock), and a non-finite block is recognised before its sweeps start: these tests take no longer than healthy ones.
def _svd_ok(a, U, S, Vh, tol=sv.DECOMP_TOL):
    """the acceptance criteria of helpers.check_svd_invariants, for real and complex blocks"""
    k = min(a.shape)
    assert U.shape == (a.shape[0], k) and S.shape == (k,) and Vh.shape == (k, a.shape[1])
    nrm = np.linalg.norm(a)
    assert np.all(S >= 0) and np.all(S[:-1] >= S[1:] - tol * nrm)
    assert np.abs(S - np.linalg.svd(a, compute_uv=False)).max() <= tol * nrm
    assert np.abs((U * S) @ Vh - a).max() <= tol * nrm
    assert np.abs(U.conj().T @ U - np.eye(k)).max() <= tol and np.abs(Vh @ Vh.conj().T - np.eye(k)).max() <= tol


def _healthy_svd(bb, blocks):
    for a, (U, S, Vh) in zip(blocks, bb.matrix_svd_batched([bb.as_block(x) for x in blocks])):
        _svd_ok(a, bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh))


@pytest.mark.parametrize('route,cplx,shape', sv.SVD_ROUTES, ids=[f'{r}-{s[0]}x{s[1]}' for r, _, s in sv.SVD_ROUTES])
def test_nonfinite_svd_raises_and_leaves_the_backend_usable(bb, route, cplx, shape):
    healthy = [sv.decomp_block(shape, cplx, 10 + k) for k in range(3)]
    for val in (np.nan, np.inf):
        for pos in sv.poison_positions(shape):
            bad = healthy[1].copy()
            bad[pos] = val
            for lst in ([bad], [healthy[0], bad, healthy[2]]):   # alone, and as the middle block of a healthy list
                with pytest.raises(_lib.LinAlgError):
                    bb.matrix_svd_batched([bb.as_block(x) for x in lst])
                _healthy_svd(bb, healthy[:len(lst)])             # no stale flag or workspace: the same shapes decompose
    if cplx:   # a NaN in the imaginary part only
        bad = healthy[1].copy()
        bad[1, 1] = complex(bad[1, 1].real, np.nan)
        with pytest.raises(_lib.LinAlgError):
            bb.matrix_svd_batched([bb.as_block(bad)])
        _healthy_svd(bb, healthy[:1])


@pytest.mark.parametrize('route,cplx,shape', sv.SVD_ROUTES, ids=[f'{r}-{s[0]}x{s[1]}' for r, _, s in sv.SVD_ROUTES])
def test_nonfinite_surroundings_of_a_view_do_not_reach_its_svd(bb, route, cplx, shape):
    """a healthy block as a view (row and column offsets: the strided branch of the range check) into a parent that is NaN
    everywhere else"""
    a = sv.decomp_block(shape, cplx, 21)
    parent = np.full((shape[0] + 5, shape[1] + 7), np.nan, dtype=a.dtype)
    parent[2:2 + shape[0], 3:3 + shape[1]] = a
    view = bb.get_item(bb.as_block(parent), (slice(2, 2 + shape[0]), slice(3, 3 + shape[1])))
    (U, S, Vh), = bb.matrix_svd_batched([view])
    _svd_ok(a, bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh))


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('n', sv.EIGH_SIZES)
def test_nonfinite_eigh_raises_and_leaves_the_backend_usable(bb, n, cplx):
    healthy = [sv.hermitian_block(n, cplx, 30 + k) for k in range(3)]

    def check_healthy(blocks):
        for h, (w, v) in zip(blocks, bb.eigh_batched([bb.as_block(x) for x in blocks])):
            w, v = bb.to_numpy(w), bb.to_numpy(v)
            nrm = np.linalg.norm(h)
            assert np.abs(np.sort(w) - np.linalg.eigvalsh(h)).max() <= sv.DECOMP_TOL * nrm
            assert np.abs(h @ v - v * w).max() <= sv.DECOMP_TOL * nrm
            assert np.abs(v.conj().T @ v - np.eye(n)).max() <= sv.DECOMP_TOL

    for val in (np.nan, np.inf):
        for i, j in sv.poison_positions((n, n)):
            bad = healthy[1].copy()
            bad[i, j] = bad[j, i] = val
            for lst in ([bad], [healthy[0], bad, healthy[2]]):
                with pytest.raises(_lib.LinAlgError):
                    bb.eigh_batched([bb.as_block(x) for x in lst])
                check_healthy(healthy[:len(lst)])
    parent = np.full((n + 4, n + 6), np.nan, dtype=healthy[0].dtype)   # a healthy view into a NaN parent
    parent[1:1 + n, 5:5 + n] = healthy[0]
    view = bb.get_item(bb.as_block(parent), (slice(1, 1 + n), slice(5, 5 + n)))
    (w, v), = bb.eigh_batched([view])
    assert np.abs(np.sort(bb.to_numpy(w)) - np.linalg.eigvalsh(healthy[0])).max() <= sv.DECOMP_TOL * np.linalg.norm(healthy[0])


@pytest.mark.parametrize('route,cplx,shape', sv.SVD_ROUTES, ids=[f'{r}-{s[0]}x{s[1]}' for r, _, s in sv.SVD_ROUTES])
def test_nonfinite_qr_and_lq_never_return_finite_factors(bb, route, cplx, shape):
    """numpy raises nothing here: the call returns factors that show the NaN / Inf, or raises LinAlgError -- never an
    all-finite Q, R"""
    healthy = sv.decomp_block(shape, cplx, 41)
    for val in (np.nan, np.inf):
        for pos in sv.poison_positions(shape):
            bad = healthy.copy()
            bad[pos] = val
            for fn in (bb.matrix_qr_batched, bb.matrix_lq_batched):
                try:
                    (f1, f2), = fn([bb.as_block(bad)])
                except _lib.LinAlgError:
                    continue
                f1, f2 = bb.to_numpy(f1), bb.to_numpy(f2)
                assert not (np.isfinite(f1).all() and np.isfinite(f2).all()), f'{fn.__name__}: finite factors for {val} at {pos}'
    (q, r), = bb.matrix_qr_batched([bb.as_block(healthy)])   # and the backend still factors a healthy block
    q, r = bb.to_numpy(q), bb.to_numpy(r)
    assert np.abs(q @ r - healthy).max() <= sv.DECOMP_TOL * np.linalg.norm(healthy)
    assert np.abs(q.conj().T @ q - np.eye(q.shape[1])).max() <= sv.DECOMP_TOL


def test_nonfinite_matrix_exp(bb):
    """next to the Inf case of test_gpu_tensor_functions.py: a NaN entry.  Beyond the in-LDS limit the 1-norm is NaN and the
    call refuses the block as it refuses Inf; in LDS the result shows the NaN.  Never an all-finite answer."""
    big = _lib.CYB_EXPM_SMALL_MAX_N_F64 + 4
    for n in (12, big):
        for pos in sv.poison_positions((n, n)):
            a = sv.decomp_block((n, n), False, 50) / n
            a[pos] = np.nan
            try:
                out, = bb.matrix_exp_many([bb.as_block(a)])
            except ValueError:
                continue
            assert n == 12, 'a NaN 1-norm beyond the in-LDS limit is refused like an infinite one'
            assert np.isnan(bb.to_numpy(out)).any()
    a = sv.decomp_block((12, 12), False, 51) / 12
    out, = bb.matrix_exp_many([bb.as_block(a)])
    import scipy.linalg
    assert np.abs(bb.to_numpy(out) - scipy.linalg.expm(a)).max() <= sv.DECOMP_TOL
