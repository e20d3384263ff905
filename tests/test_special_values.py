"""The tables of special_value_cases.py themselves, on the CPU: numpy against mpmath on the finite part of every grid (which
measures the recorded bounds), the Philox model against the Random123 known answers, and the cases against
tests/numpy_backend.py where that backend has the operation."""
import mpmath
import numpy as np
import pytest

import special_value_cases as sv
from numpy_backend import NumpyGroupedBackend


def test_comparison_helpers_tell_classes_apart():
    ok = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0])
    assert list(sv.assert_same_class(ok, ok)) == [False, False, False, False, False, True]
    for i, wrong in enumerate([1.0, -np.inf, np.inf, -0.0, 0.0]):
        bad = ok.copy()
        bad[i] = wrong
        with pytest.raises(AssertionError):
            sv.assert_same_class(bad, ok)
    with pytest.raises(AssertionError):
        sv.assert_same_class(np.array([1.0]), np.array([np.nan]))
    sv.assert_bits_equal(ok, ok)
    with pytest.raises(AssertionError):
        sv.assert_bits_equal(np.array([0.0]), np.array([-0.0]))
    with pytest.raises(AssertionError):
        sv.assert_bits_equal(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]))
    assert sv.ulp_of(1.0) == 2.0 ** -52 and sv.ulp_of(0.75) == 2.0 ** -53 and sv.ulp_of(1e-310) == 5e-324


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sv.REDUCTION_LENGTHS)
def test_reduction_vectors_hold_what_they_claim(n):
    """every special set at every position that exists, and numpy's rules for them: NaN wins max / min / argmax / argmin
    (first NaN), +-Inf together with NaN-free data gives Inf norms, both Infs give a NaN sum"""
    cases = sv.reduction_vectors(n)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    for pos in sv.SPECIAL_POSITIONS:
        if (n - 1 if pos < 0 else pos) < n:
            assert f'nan@{pos}' in names and f'+inf@{pos}' in names and f'-inf@{pos}' in names
    w = np.random.default_rng(5).standard_normal(n)
    nb = NumpyGroupedBackend()
    for name, v in cases:
        want = sv.reduction_expectations(v, w)
        if np.isnan(v).any():
            first = int(np.flatnonzero(np.isnan(v))[0])
            assert np.isnan(want['max_abs']) and np.isnan(want['max']) and np.isnan(want['min']), name
            assert want['abs_argmax'] == [first] and want['argmin'] == [first], name
            assert np.isnan(want['norm2']) and np.isnan(want['sum_all']) and np.isnan(want['inner']), name
        elif np.isinf(v).any():
            assert want['max_abs'] == np.inf and want['norm2'] == np.inf and want['norm1'] == np.inf, name
        # the reference-style backend of the suite gives the same norm and inner product
        sv.check_scalar(float(nb.norm_many([v])), want['norm2'], 4 * n * sv.EPS * abs(want['norm2']), f'{name}: norm_many')
        if np.isfinite(v).all():
            sv.check_scalar(float(np.real(nb.inner_many([v], [w]))), want['inner'], 4 * n * sv.EPS * want['inner_abs'],
                            f'{name}: inner_many')
    ties = dict(cases).get('ties')
    if ties is not None:
        assert sv.reduction_expectations(ties, w)['abs_argmax'] == [n // 3]
        assert sv.reduction_expectations(ties, w)['argmin'] == [n // 2]
        assert sv.reduction_expectations(dict(cases)['abs-ties'], w)['abs_argmax'] == [n // 2]
    if n >= 2:
        assert sv.reduction_expectations(dict(cases)['-0,+0'], w)['argmin'] == [0]
        assert sv.reduction_expectations(dict(cases)['+0,-0'], w)['abs_argmax'] == [0]


def test_comparisons_on_nan_are_false_except_ne():
    v = np.array([np.nan, 1.0, np.inf])
    for op in sv.COMPARE_OPS:
        r = sv.np_eval(sv.NP_COMPARE[op], v, v)
        assert bool(r[0]) == (op == 'ne')
        assert bool(sv.np_eval(sv.NP_COMPARE[op], v, 1.0)[0]) == (op == 'ne')


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('shape', [(1,), (37, 21), (8193,)])
def test_allclose_cases_cover_the_counter_examples(shape, cplx):
    cases = {name: (a, b, rtol, atol, want) for name, a, b, rtol, atol, want in sv.allclose_cases(shape, cplx)}
    truth = {'identical': True, 'within rtol': True, 'outside rtol': False, 'within atol': True, 'mixed scales': False,
             'finite vs inf': False, 'inf vs finite': False, 'equal +inf': True, 'equal -inf': True, 'opposite inf': False,
             'nan both': False}
    for name, want in truth.items():
        assert cases[name][4] is want, name
    assert not any(c[4] for n_, c in cases.items() if n_.startswith('nan in'))
    if int(np.prod(shape)) > 1:
        # the global-scale rule (max |a - b| <= atol + rtol max |b|) would accept the mixed-scale case: it is a counter-example
        a, b, rtol, atol, _ = cases['mixed scales']
        assert np.abs(a - b).max() <= atol + rtol * np.abs(b).max()
    # a NaN-dropping max of the difference would accept the one-sided NaN
    a, b, rtol, atol, _ = cases[f'nan in a at {tuple(0 for _ in shape)}']
    d = np.abs(a - b)
    assert np.fmax.reduce(np.append(d.ravel(), 0.0)) <= atol + rtol * np.abs(b).max()   # (fmax skips NaN, as the old kernel did)


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_real_grid_holds_the_listed_values():
    g = sv.REAL_GRID
    for x in (0.0, 5e-324, 2.2e-308, 1.0, sv.DBL_MAX, np.inf, 709.78, 709.79, 1 + sv.EPS, 3.5e38):
        assert (g == x).any() and (g == -x).any() or x in (709.78, 709.79, 1 + sv.EPS)
    assert np.signbit(g[g == 0.0]).any() and not np.signbit(g[g == 0.0]).all()
    assert np.isnan(g).sum() == 1 and (g == -745.2).any() and (g == 1 - sv.EPS).any()
    big = np.abs(g[np.isfinite(g)])
    assert ((big >= 1e-300) & (big <= 1e300)).sum() >= 64
    for n in sv.REAL_LENGTHS:   # every length sees the special values; the longer ones the whole grid
        v = sv.real_vector(n, 12)
        assert len(v) == n and (n < len(g) or set(np.isnan(v)) == {False, True})


@pytest.mark.parametrize('name,recorded', [('exp', sv.NUMPY_EXP_ULP), ('log', sv.NUMPY_LOG_ULP)])
def test_numpy_exp_log_error_is_the_recorded_one(name, recorded):
    x = sv.REAL_GRID
    got = sv.np_eval(sv.REAL_UNARY[name], x)
    sel = np.isfinite(got) & (got != 0) & np.isfinite(x)
    err = sv.ulp_errors(got[sel], [sv.mp_real(name, v) for v in x[sel]])
    print(f'numpy {name}: worst error {err.max():.4f} ulp on {sel.sum()} finite results')
    assert sel.sum() >= 20
    assert err.max() <= recorded
    assert recorded * sv.MARGIN == {'exp': sv.GPU_EXP_ULP, 'log': sv.GPU_LOG_ULP}[name]


def test_float32_rounding_cases():
    r = sv.np_eval(sv.REAL_UNARY['round_f32'], np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 3.5e38, -3.5e38, 1e-40, 2.0 ** -150,
                                                         2.0 ** -150 * (1 + sv.EPS), 3.4028235677973366e38]))
    assert r[0] == 1.0 and r[1] == 1 + 2.0 ** -22                 # ties to even, both directions
    assert r[2] == np.inf and r[3] == -np.inf and r[7] == np.inf   # overflow
    assert 0 < r[4] < 1.2e-38 and r[4] != 1e-40                    # a float32 denormal
    assert r[5] == 0.0 and r[6] == 2.0 ** -149                     # the halfway point below the smallest denormal


def test_cutoff_cases_sit_on_the_threshold():
    for a, c in sv.cutoff_cases():
        inv, lg = sv.np_cutoff_inverse(a, c), sv.np_stable_log(a, c)
        assert inv[0] == 1 / c and inv[1] == 0.0 and inv[2] != 0.0     # |a| < cutoff is strict
        assert lg[0] == 0.0 and lg[1] == 0.0 and lg[2] == np.log(a[2])  # a > cutoff is strict
        assert np.isnan(inv[6]) and lg[6] == 0.0                        # NaN: not below the cutoff; not above it
        assert lg[3] == 0.0 and inv[3] == -1 / c                        # negative elements


def test_pow_cases():
    b, e = sv.pow_exact_cases()
    assert len(b) > 400 and b[0] == 4.0 and e[0] == 3.0
    got = sv.np_eval(np.power, b, e)
    assert got[0] == 64.0
    with sv.mp_ctx():
        for x, y, g in zip(b, e, got):   # numpy's power is exact on every representable case
            assert mpmath.mpf(float(g)) == sv.mp_pow(x, y), (x, y)
    x, y = map(np.array, zip(*sv.POW_SPECIAL))
    got = sv.np_eval(np.power, x, y)
    want = {(repr(a), repr(b_)): g for (a, b_), g in zip(sv.POW_SPECIAL, got)}   # (repr keeps 0.0 and -0.0 apart)
    assert want['0.0', '0.0'] == 1.0 and want['0.0', '-1.0'] == np.inf and want['-0.0', '-1.0'] == -np.inf
    assert want['-0.0', '-2.0'] == np.inf and np.isnan(want['-8.0', repr(1.0 / 3.0)])
    assert want['2.0', '-1074.0'] == 5e-324 and want['2.0', '1074.0'] == np.inf
    assert want['2.0', '1023.0'] == 2.0 ** 1023 and want['2.0', '-1023.0'] == 2.0 ** -1023 and want['4.0', '0.5'] == 2.0
    assert want['nan', '0.0'] == 1.0 and want['1.0', 'nan'] == 1.0
    # the inexact cases and the squaring-chain cases: numpy's own error is the recorded one
    x, y = map(np.array, zip(*sv.POW_LIBM))
    got = sv.np_eval(np.power, x, y)
    assert np.isfinite(got).all() and (got != 0).all()
    err = sv.ulp_errors(got, [sv.mp_pow(a, b_) for a, b_ in zip(x, y)])
    x, y = sv.pow_chain_cases()
    got = sv.np_eval(np.power, x, y)
    ok = np.isfinite(got) & (np.abs(got) >= sv.DBL_MIN)
    assert ok.all() and (np.abs(y) <= 4096).all() and ((x >= 0.9) & (x <= 1.1)).all()
    err2 = sv.ulp_errors(got, [sv.mp_pow(a, b_) for a, b_ in zip(x, y)])
    print(f'numpy pow: worst error {max(err.max(), err2.max()):.4f} ulp')
    assert max(err.max(), err2.max()) <= sv.NUMPY_POW_ULP


# ---- C ---------------------------------------------------------------------------------------------------------------------
def test_complex_grid_holds_the_listed_points():
    g = sv.COMPLEX_GRID
    assert len(g) == 15 * 15 + 12 + 8 + 4
    for z in (complex(710, 0), complex(710, 1e-3), complex(-746, 1), complex(0, 1e6), complex(1, 1e-9), complex(1 - 0.1, 0),
              complex(1.5e308, 1e-310)):
        assert (g == z).any()
    cut = g[(g.real < 0) & (g.imag == 0) & np.isfinite(g.real)]
    assert np.signbit(cut.imag).any() and not np.signbit(cut.imag).all()
    dropped = sv.complex_div_dropped(sv.complex_partner())
    assert 0 < dropped.sum() <= 0.05 * len(g)


@pytest.mark.parametrize('name', ['abs', 'sqrt', 'exp', 'log', 'angle', 'div'])
def test_numpy_complex_error_is_the_recorded_one(name):
    z = sv.COMPLEX_GRID
    if name == 'div':
        w = sv.complex_partner()
        keep = ~sv.complex_div_dropped(w)
        z, w = z[keep], w[keep]
        got = sv.np_eval(np.divide, z, w)
        err = sv.complex_error_units(name, got, got, z, w)
    else:
        got = sv.np_eval(sv.COMPLEX_UNARY[name], z)
        err = sv.complex_error_units(name, got, got, z)
    print(f'numpy complex {name}: worst error {err.max():.4f} units of 2^-52 |result| on {(err > 0).sum()} finite results')
    assert (err > 0).sum() >= 20
    assert err.max() <= sv.NUMPY_C_ERR[name]
    assert sv.GPU_C_ERR[name] == sv.MARGIN * sv.NUMPY_C_ERR[name]


def test_numpy_answers_for_the_four_suspects():
    with np.errstate(all='ignore'):
        assert np.exp(np.complex128(complex(710, 0))) == complex(np.inf, 0)
        r = np.log(np.complex128(complex(1, 1e-9))).real
        assert abs(r - 5e-19) < 1e-30
        s = np.sqrt(np.complex128(complex(1.5e308, 1e308)))
        assert abs(s - complex(1.285e154, 3.89e153)) < 1e151
        assert np.power(2.0, -1074.0) == 5e-324


# ---- D ---------------------------------------------------------------------------------------------------------------------
def test_reference_backend_raises_on_nonfinite_decompositions():
    """the numpy / scipy routines behind the reference refuse non-finite blocks loudly (LinAlgError, or scipy's ValueError of
    its finiteness check); the device path reports LinAlgError for all of them"""
    loud = (np.linalg.LinAlgError, ValueError)
    nb = NumpyGroupedBackend()
    for name, cplx, shape in sv.SVD_ROUTES:
        for val in (np.nan, np.inf):
            a = sv.decomp_block(shape, cplx, 3)
            a[sv.poison_positions(shape)[1]] = val
            with pytest.raises(loud):
                nb.matrix_svd_batched([sv.decomp_block(shape, cplx, 4), a])
    for n in sv.EIGH_SIZES:
        h = sv.hermitian_block(n, True, 5)
        h[0, 0] = np.nan
        try:   # LAPACK's eigh either raises or hands the NaN through: never an all-finite answer
            (w, v), = nb.eigh_batched([h])
        except loud:
            continue
        assert not np.isfinite(w).all()


# ---- E ---------------------------------------------------------------------------------------------------------------------
def test_philox_model_reproduces_the_known_answers():
    for counter, key, out in sv.PHILOX_KAT:
        got = sv.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(x) for x in got] == list(out)
    # vectorised over a batch: the same words
    c = np.array([k[0] for k in sv.PHILOX_KAT], dtype=np.uint64)
    k = np.array([k[1] for k in sv.PHILOX_KAT], dtype=np.uint64)
    assert np.array_equal(sv.philox4x32_10(c, k), np.array([k_[2] for k_ in sv.PHILOX_KAT], dtype=np.uint64))


def test_uniform_and_normal_models():
    u = sv.model_uniform(4097, 7, 0.0, 1.0)
    assert len(u) == 4097 and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 4097
    assert np.array_equal(sv.model_uniform(511, 7, 0.0, 1.0), u[:511])          # a prefix: no dependence on n
    assert not np.array_equal(sv.model_uniform(511, 8, 0.0, 1.0), u[:511])
    assert np.array_equal(sv.model_uniform(3, 2 ** 64 - 1, 1.0, 1.0), np.ones(3))
    assert np.array_equal(sv.model_uniform(64, 2 ** 32 + 5, -3.0, 5.0), -3.0 + 8.0 * sv.model_uniform(64, 2 ** 32 + 5, 0.0, 1.0))
    assert abs(u.mean() - 0.5) < 0.02 and abs(u.std() - 12 ** -0.5) < 0.02
    v, rad = sv.model_normal(511, 7, 2.0)
    assert len(v) == 511 and (np.abs(v) <= rad * (1 + 1e-15)).all()
    assert abs(v.mean()) < 0.3 and abs(v.std() - 2.0) < 0.3
    assert sv.BOX_MULLER_C < 16
