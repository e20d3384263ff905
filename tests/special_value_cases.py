"""Non-finite and extreme inputs for the block kernels, with numpy's answers as the expectation.

The reference's NumpyBlockBackend defines what the library does with NaN, +-Inf, signed zeros and values near the ends of
the double range: whatever numpy does.  This module holds the input grids, numpy's results for them (computed under
``np.errstate(all='ignore')``), mpmath evaluations (240 bits) of the finite results, a Python model of the Philox4x32-10
generator of ``random_uniform`` / ``random_normal``, and the error bounds.  ``test_special_values.py`` checks the tables
themselves on the CPU; ``test_gpu_special_values.py`` runs the same cases through ``HipBlockBackend``.

Comparison rule (``assert_same_class`` + a bound): non-finite results are compared by class (NaN-ness, sign of Inf), zeros
by sign, finite results against mpmath within the bound of their section.
"""
import math

import mpmath
import numpy as np

MP_PREC = 240
EPS = 2.0 ** -52
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
DENORM_MIN = 5e-324
NAN, INF = float('nan'), float('inf')

# ---- error bounds -----------------------------------------------------------------------------------------------------
# Source of the device bounds: the ROCm installation ships no accuracy table for the device math library
# (nothing under share/doc names an ulp bound for exp / log / sincos / hypot / atan2), so each device bound is FOUR TIMES
# numpy's own worst error against mpmath on the same grid ("both libraries claim a few ulp").  The measured values below
# are what test_special_values.py measures (it asserts that the measurement does not exceed the recorded constant, so a
# numpy that got worse shows up there and not as a silently wider device bound).
MARGIN = 4.0
# real exp / log on REAL_GRID, in ulp of the result (measured: exp 0.4881, log 0.5000; recorded rounded up)
NUMPY_EXP_ULP = 0.49
NUMPY_LOG_ULP = 0.51
GPU_EXP_ULP = MARGIN * NUMPY_EXP_ULP
GPU_LOG_ULP = MARGIN * NUMPY_LOG_ULP
# complex functions on the finite part of COMPLEX_GRID: |got - want| in units of 2^-52 |want| + 5e-324 (log: per component).
# Measured: abs 0.4847, sqrt 0.5589, exp 0.4962, log 0.6622, angle 0.2943, div 1.0000; recorded rounded up.
NUMPY_C_ERR = {'abs': 0.49, 'sqrt': 0.56, 'exp': 0.50, 'log': 0.67, 'angle': 0.30, 'div': 1.01}
GPU_C_ERR = {k: MARGIN * v for k, v in NUMPY_C_ERR.items()}
# Box-Muller: rad * (cos | sin)(2 pi u2) with rad = sigma * sqrt(-2 log u1).  Error of the value in units of 2^-52 * rad:
# log (GPU_LOG_ULP, halved by the square root), the product -2 * log and sigma * sqrt (0.5 each), sqrt (0.5), the argument
# 2 pi u2 (0.5 ulp of an angle up to 2 pi moves sin / cos by up to 2 pi * 2^-53 = 3.2 units), sincos itself (same margin rule
# as exp: MARGIN * 0.5) and the final product (0.5).
BOX_MULLER_C = GPU_LOG_ULP / 2 + 0.5 + 0.5 + 0.5 + 3.2 + MARGIN * 0.5 + 0.5


def mp_ctx():
    return mpmath.workprec(MP_PREC)


def ulp_of(x):
    """spacing of doubles at |x| (the denormal spacing below DBL_MIN)"""
    x = abs(float(x))
    if x < DBL_MIN:
        return DENORM_MIN
    return 2.0 ** (math.frexp(x)[1] - 53)


def assert_same_class(got, want, what=''):
    """NaN where numpy has NaN, Inf of the same sign where numpy has Inf, zeros of the same sign; returns the mask of the
    finite non-zero entries (to be checked against a bound by the caller).  Complex arrays: per component."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    if np.iscomplexobj(want) or np.iscomplexobj(got):
        got, want = got.astype(np.complex128), want.astype(np.complex128)
        return assert_same_class(got.real, want.real, what + ' (real part)') & \
            assert_same_class(got.imag, want.imag, what + ' (imaginary part)')
    got, want = got.astype(np.float64), want.astype(np.float64)
    bad = np.flatnonzero((np.isnan(got) != np.isnan(want)).ravel())
    assert bad.size == 0, f'{what}: NaN-ness differs at {bad[:8]}: got {got.ravel()[bad[:8]]}, numpy {want.ravel()[bad[:8]]}'
    inf = np.isinf(want)
    bad = np.flatnonzero(((np.isinf(got) != inf) | (inf & (np.signbit(got) != np.signbit(want)))).ravel())
    assert bad.size == 0, f'{what}: Inf differs at {bad[:8]}: got {got.ravel()[bad[:8]]}, numpy {want.ravel()[bad[:8]]}'
    zero = want == 0.0
    bad = np.flatnonzero((zero & ((got != 0.0) | (np.signbit(got) != np.signbit(want)))).ravel())
    assert bad.size == 0, f'{what}: signed zero differs at {bad[:8]}: got {got.ravel()[bad[:8]]}, numpy {want.ravel()[bad[:8]]}'
    return np.isfinite(want) & ~zero


def assert_bits_equal(got, want, what=''):
    """bit for bit, except that any NaN matches any NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~same.ravel())
    assert bad.size == 0, f'{what}: differs at {bad[:8]}: got {got.ravel()[bad[:8]]!r}, numpy {want.ravel()[bad[:8]]!r}'


def ulp_errors(got, want_mp):
    """|got - want| in ulp of want, for finite doubles `got` and mpmath numbers `want_mp`"""
    out = np.zeros(len(got))
    with mp_ctx():
        for i, (g, w) in enumerate(zip(got, want_mp)):
            out[i] = float(abs(mpmath.mpf(float(g)) - w) / mpmath.mpf(ulp_of(float(w))))
    return out


# ---- A. reductions, extrema, comparisons --------------------------------------------------------------------------------
REDUCTION_LENGTHS = (1, 2, 300, 4097, 8193)   # 4097: three workgroups of the extremum kernel; 8193: a second reduction item
SPECIAL_POSITIONS = (0, 1, 63, 64, 255, 256, 768, -1)
SPECIAL_SETS = {'nan': (NAN,), '+inf': (INF,), '-inf': (-INF,), 'all': (NAN, INF, -INF)}
SHAPE_2D = {1: (1, 1), 2: (1, 2), 300: (15, 20), 4097: (17, 241), 8193: (3, 2731)}


def reduction_vectors(n):
    """[(name, vector)]: standard-normal data of length n with one special set placed at each position, plus an all-NaN
    vector, plain vectors, exact ties and signed zeros"""
    rng = np.random.default_rng(1000 + n)
    base = rng.standard_normal(n)
    out = [('plain', base.copy()), ('plain2', rng.standard_normal(n) * 1e3), ('all-nan', np.full(n, NAN))]
    for sname, vals in SPECIAL_SETS.items():
        for pos in SPECIAL_POSITIONS:
            p = n - 1 if pos < 0 else pos
            if p >= n:
                continue
            v = base.copy()
            if len(vals) == 1:
                v[p] = vals[0]
            else:   # the three together: at p and its cyclic neighbours
                if n < 3:
                    continue
                for k, x in enumerate(vals):
                    v[(p + k) % n] = x
            out.append((f'{sname}@{pos}', v))
    if n >= 300:
        t = base.copy()                         # ties between equal finite values: the lowest index wins
        hi, lo = np.abs(t).max() + 1.0, t.min() - 1.0
        t[[n // 3, n - 1]] = hi
        t[[n // 2, n - 2]] = lo
        out.append(('ties', t))
        t = base.copy()
        t[[n // 2, n - 1]] = [-hi, hi]           # equal magnitude, opposite sign: abs_argmax takes the first
        out.append(('abs-ties', t))
    if n >= 2:
        z = np.zeros(n)
        z[::2] = -0.0
        out.append(('-0,+0', z))
        z = np.zeros(n)
        z[1::2] = -0.0
        out.append(('+0,-0', z))
    return out


def reduction_expectations(v, w):
    """numpy's answers for a vector (or 2-D block) v; w is a second, healthy operand of the same shape for `inner`"""
    with np.errstate(all='ignore'):
        a = np.abs(v)
        return {
            'max_abs': float(np.max(a)),
            'max': float(np.max(v)),
            'min': float(np.min(v)),
            'abs_argmax': [int(i) for i in np.unravel_index(np.argmax(a), v.shape)],
            'argmin': [int(i) for i in np.unravel_index(np.argmin(v), v.shape)],
            'norm2': float(np.linalg.norm(v.ravel())),
            'norm1': float(np.linalg.norm(v.ravel(), 1)),
            'norminf': float(np.linalg.norm(v.ravel(), np.inf)),
            'sum_all': float(np.sum(v)),
            'inner': float(np.sum(v * w)),
            'sum_abs': float(np.sum(a)) if np.isfinite(a).all() else NAN,
            'inner_abs': float(np.sum(np.abs(v * w))) if np.isfinite(v).all() else NAN,
        }


def check_scalar(got, want, bound, what):
    """one reduction result: class as numpy's, finite values within `bound` (absolute)"""
    finite = assert_same_class(np.array([got]), np.array([want]), what)
    if finite[0]:
        assert abs(got - want) <= bound, f'{what}: got {got!r}, numpy {want!r}, bound {bound:.3e}'


COMPARE_OPS = ('lt', 'le', 'gt', 'ge', 'eq', 'ne')
NP_COMPARE = {'lt': np.less, 'le': np.less_equal, 'gt': np.greater, 'ge': np.greater_equal, 'eq': np.equal,
              'ne': np.not_equal}


def allclose_cases(shape, cplx):
    """[(name, a, b, rtol, atol, want)] with want = np.allclose(a, b, rtol, atol)"""
    rng = np.random.default_rng(77 + int(np.prod(shape)) + cplx)

    def rnd():
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if cplx else x

    n = int(np.prod(shape))
    last = tuple(s - 1 for s in shape)
    first = tuple(0 for _ in shape)
    unit = (0.6 + 0.8j) if cplx else 1.0
    out = []

    def add(name, a, b, rtol=1e-5, atol=1e-8):
        with np.errstate(all='ignore'):
            out.append((name, a, b, rtol, atol, bool(np.allclose(a, b, rtol=rtol, atol=atol))))

    b = rnd()
    add('identical', b.copy(), b)
    add('within rtol', b * (1 + 1e-6), b)
    add('outside rtol', b * (1 + 1e-4), b)
    add('within atol', b + 1e-9, b, 0.0, 1e-8)
    # 1. a NaN in one operand only (the difference is NaN there: a NaN-dropping max would not see it)
    for pos in (first, last):
        a = b.copy()
        a[pos] = NAN
        add(f'nan in a at {pos}', a, b)
        add(f'nan in b at {pos}', b, a)
    if cplx:
        a = b.copy()
        a[last] = complex(a[last].real, NAN)
        add('nan in the imaginary part of a', a, b)
    # 2. mixed scales: one entry off by 1e-3 relative next to an entry of 1e6 (elementwise False, global-scale True)
    a, b2 = b.copy(), b.copy()
    a[last], b2[last] = 1.0 * unit, 1.001 * unit
    if n > 1:
        a[first] = b2[first] = 1e6 * unit
    add('mixed scales', a, b2)
    # 3. infinities
    for name, xa, xb in (('finite vs inf', 1.0, INF), ('inf vs finite', INF, 1.0), ('equal +inf', INF, INF),
                         ('equal -inf', -INF, -INF), ('opposite inf', INF, -INF), ('nan both', NAN, NAN)):
        a, b2 = b.copy(), b.copy()
        a[last], b2[last] = xa, xb
        add(name, a, b2)
    if cplx:
        a, b2 = b.copy(), b.copy()
        a[last] = b2[last] = complex(1.0, -INF)
        add('equal inf in the imaginary part', a, b2)
    return out


# ---- B. real elementwise ops ---------------------------------------------------------------------------------------------
def _real_grid():
    rng = np.random.default_rng(2024)
    mags = 10.0 ** rng.uniform(-300, 300, 64)
    mags[::2] *= -1
    fixed = [0.0, -0.0, DENORM_MIN, -DENORM_MIN, 2.2e-308, -2.2e-308, 1.0, -1.0, DBL_MAX, -DBL_MAX, INF, -INF, NAN,
             709.78, 709.79, -745.2, 1 + EPS, 1 - EPS,
             # float32 rounding: ties (1 + 2^-24 is halfway between two floats, 1 + 3*2^-24 too), overflow at 3.5e38, the
             # largest float, float32 denormals (1e-40, the halfway point 2^-150 and just above it)
             1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 3.5e38, -3.5e38, 3.4028234663852886e38, 3.4028235677973366e38,
             1e-40, -1e-40, 2.0 ** -150, 2.0 ** -150 * (1 + EPS), 2.0 ** -149,
             # truncation
             2.5, -2.5, 0.9999999999999999, -0.9999999999999999, 4503599627370496.5, 1e19, -1e19]
    return np.concatenate([np.array(fixed), mags])


REAL_GRID = _real_grid()
REAL_LENGTHS = (1, 255, 257)


def real_vector(n, shift=0):
    """length-n vector that cycles through REAL_GRID starting at `shift`"""
    idx = (np.arange(n) + shift) % len(REAL_GRID)
    return REAL_GRID[idx].copy()


def _np_trunc_to_int(x):
    return np.trunc(x)


REAL_UNARY = {   # name -> (HipBlockBackend call, numpy call of numpy.cpp, exact?)
    'abs': np.abs, 'sqrt': np.sqrt, 'exp': np.exp, 'log': np.log, 'neg': np.negative, 'square': np.square,
    'reciprocal': lambda x: 1.0 / x, 'round_f32': lambda x: x.astype(np.float32).astype(np.float64), 'trunc': np.trunc,
}
REAL_UNARY_OPCODE = {'abs': 0, 'sqrt': 1, 'exp': 2, 'log': 3, 'neg': 4, 'square': 5, 'reciprocal': 6, 'round_f32': 7, 'trunc': 8}
REAL_UNARY_EXACT = ('abs', 'sqrt', 'neg', 'square', 'reciprocal', 'round_f32', 'trunc')
REAL_BINARY = {'add': np.add, 'sub': np.subtract, 'mul': np.multiply, 'div': np.divide}
REAL_BINARY_OPCODE = {'add': 0, 'sub': 1, 'mul': 2, 'div': 3, 'pow': 4}


def np_eval(fn, *args):
    with np.errstate(all='ignore'):
        return fn(*args)


def mp_real(name, x):
    """mpmath value of exp / log at the double x"""
    with mp_ctx():
        return {'exp': mpmath.exp, 'log': mpmath.log}[name](mpmath.mpf(float(x)))


def cutoff_cases():
    """(elements, cutoff): the element equal to the cutoff, one ulp below and above, NaN, negatives, zeros, Inf"""
    out = []
    for c in (1e-12, 1.0, 3.5):
        lo, hi = np.nextafter(c, 0.0), np.nextafter(c, INF)
        out.append((np.array([c, lo, hi, -c, -lo, -hi, NAN, 0.0, -0.0, INF, -INF, 2.0, -2.0, 1e-300, DBL_MAX]), c))
    return out


def np_cutoff_inverse(a, cutoff):
    with np.errstate(all='ignore'):
        return 1 / np.where(np.abs(a) < cutoff, np.inf, a)


def np_stable_log(a, cutoff):
    with np.errstate(all='ignore'):
        return np.where(a > cutoff, np.log(a), 0.0)


def pow_exact_cases():
    """(base, exponent) arrays: 4 ** 3 and every b ** e, b in [-9, 9], e in [-30, 30], whose result is representable
    (checked with exact rational arithmetic)"""
    from fractions import Fraction
    bs, es = [4.0], [3.0]
    for b in range(-9, 10):
        for e in range(-30, 31):
            if b == 0 and e <= 0:
                continue
            exact = Fraction(b) ** e
            try:
                ok = Fraction(float(exact)) == exact
            except OverflowError:
                ok = False
            if ok:
                bs.append(float(b))
                es.append(float(e))
    return np.array(bs), np.array(es)


POW_SPECIAL = [   # (x, y): compared with numpy by class and bit for bit where finite (every finite result is exact)
    (0.0, 0.0), (-0.0, 0.0), (0.0, -1.0), (-0.0, -1.0), (-0.0, -2.0), (-8.0, 1.0 / 3.0), (2.0, 1074.0), (2.0, -1074.0), (2.0, 1023.0),
    (2.0, -1023.0), (2.0, 1024.0), (2.0, -1022.0), (0.5, 1074.0), (0.5, -1023.0), (-2.0, -1073.0), (NAN, 0.0), (1.0, NAN), (INF, -1.0),
    (-INF, 3.0), (-INF, -3.0), (INF, 0.0), (1.0, 4096.0), (-1.0, 4096.0), (-1.0, 4097.0), (-1.0, -4097.0), (1.0, -4096.0),
    (4.0, 0.5), (9.0, 0.5), (0.25, 0.5), (-4.0, 0.5), (0.0, 0.5), (INF, 0.5),
]
# finite, inexact: against mpmath within POW_LIBM_ULP ulp (the pow() of either library; numpy's measured worst is recorded)
POW_LIBM = [(1.0000001, 4097.0), (0.9999999, -4097.0), (1.0000001, -4097.5), (1.0000001, 5000.0),
            (2.0, 0.5), (3.0, 0.5), (1e10, 0.5), (7.3, 0.5), (1.7, 2.5), (1.0 + 2.0 ** -30, 4097.0), (3.0, -650.0)]
NUMPY_POW_ULP = 0.61   # measured 0.6018 on POW_LIBM and the chain cases together
GPU_POW_ULP = MARGIN * NUMPY_POW_ULP


def pow_chain_cases():
    """200 seeded x in [0.9, 1.1] with integer |y| <= 4096 such that |y| * |log2 x| < 500: the squaring chain, every
    intermediate square finite and normal.  Bound: |relative error| <= |y| * 2^-52 (first-order bound of a product of at
    most 2 log2 |y| rounded multiplications, each 2^-53, amplified by the remaining squarings)."""
    rng = np.random.default_rng(4096)
    x = rng.uniform(0.9, 1.1, 200)
    y = rng.integers(-4096, 4097, 200).astype(np.float64)
    y[:4] = [4096.0, -4096.0, 4095.0, -4095.0]
    assert (np.abs(y) * np.abs(np.log2(x)) < 500 + 4096 * 0.14).all()
    return x, y


def mp_pow(x, y):
    with mp_ctx():
        return mpmath.power(mpmath.mpf(float(x)), mpmath.mpf(float(y)))


# ---- C. complex elementwise ops ------------------------------------------------------------------------------------------
_C_AXIS = [0.0, -0.0, 1e-310, -1e-310, 1e-160, -1e-160, 1.0, -1.0, 1e160, -1e160, 1.5e308, -1.5e308, INF, -INF, NAN]


def _complex_grid():
    pts = [complex(x, y) for x in _C_AXIS for y in _C_AXIS]
    for t in (1e-9, -1e-9, 1e-5, -1e-5, 0.1, -0.1):
        pts += [complex(1.0, t), complex(1.0 + t, 0.0)]
    for x in (-1e-300, -0.5, -2.0, -1e300):       # both sides of the negative real axis
        pts += [complex(x, 0.0), complex(x, -0.0)]
    pts += [complex(710.0, 0.0), complex(710.0, 1e-3), complex(-746.0, 1.0), complex(0.0, 1e6)]
    return np.array(pts, dtype=np.complex128)


COMPLEX_GRID = _complex_grid()
COMPLEX_UNARY = {'abs': np.abs, 'sqrt': np.sqrt, 'exp': np.exp, 'log': np.log, 'angle': np.angle}
COMPLEX_OPCODE = {'abs': 0, 'sqrt': 1, 'exp': 2, 'log': 3, 'angle': 4, 'mul': 5, 'div': 6}
MP_COMPLEX = {'abs': lambda z: abs(z), 'sqrt': mpmath.sqrt, 'exp': mpmath.exp, 'log': mpmath.log, 'angle': mpmath.arg}


def mp_c(z):
    return mpmath.mpc(float(z.real), float(z.imag))


def complex_partner():
    """the second operand of products and quotients: the grid rotated by 17 places"""
    return np.roll(COMPLEX_GRID, 17)


def complex_div_dropped(w):
    """Points taken out of the quotient grid (4.8 % of it): a non-zero divisor whose parts are both below 5.6e-309 in
    magnitude.  numpy forms ``1 / (wr + wi * ratio)`` first, which overflows there, and answers Inf or NaN for quotients
    as plain as (-1e-310 + 1e-310j) / 1e-310 = -1 + 1j: indefensible, so not an expectation."""
    w = np.asarray(w)
    return (w != 0) & (np.maximum(np.abs(w.real), np.abs(w.imag)) < 5.6e-309)


def mp_complex(name, z):
    """mpmath value of a unary complex function at the double point z; mpmath has no signed zeros, so a point on a
    branch cut with imag = -0.0 is evaluated as the conjugate of the value at conj(z)"""
    z = complex(z)
    flip = z.imag == 0.0 and math.copysign(1.0, z.imag) < 0
    with mp_ctx():
        v = MP_COMPLEX[name](mpmath.mpc(z.real, 0.0 if flip else z.imag))
        if flip:
            v = -v if name == 'angle' else mpmath.conj(v)
        return mpmath.mpc(v)


def complex_error_units(name, got, want_np, inputs, partner=None):
    """Errors of the finite, non-zero results in units of ``2^-52 |want| + 5e-324`` (one denormal spacing as the absolute
    floor: a denormal result cannot be better than that) against mpmath.  `log` per component, everything else on the
    complex value.  Entries whose numpy result or whose inputs are not finite count as 0 (they are compared by class)."""
    got, want_np = np.asarray(got).astype(np.complex128), np.asarray(want_np).astype(np.complex128)
    err = np.zeros(len(got))
    with mp_ctx():
        for i, (g, w, z) in enumerate(zip(got, want_np, inputs)):
            ok = np.isfinite(w.real) and np.isfinite(w.imag) and np.isfinite(z.real) and np.isfinite(z.imag) and w != 0
            if partner is not None:
                ok = ok and np.isfinite(partner[i].real) and np.isfinite(partner[i].imag)
            if not ok or not (np.isfinite(g.real) and np.isfinite(g.imag)):
                continue
            if name == 'div':
                ex = mp_c(z) / mp_c(partner[i])
            else:
                ex = mp_complex(name, z)
            if name == 'log':
                for gp_, e in ((g.real, ex.real), (g.imag, ex.imag)):
                    if e != 0:
                        err[i] = max(err[i], float(abs(mpmath.mpf(float(gp_)) - e) / (abs(e) * EPS + DENORM_MIN)))
            elif abs(ex) != 0:
                err[i] = float(abs(mp_c(g) - ex) / (abs(ex) * EPS + DENORM_MIN))
    return err


def complex_product_bounds(z, w):
    """the convention of test_device_scale_axis_...: 2^-51 (|p1| + |p2|) per component, where finite"""
    with np.errstate(all='ignore'):
        re = 2.0 ** -51 * (np.abs(z.real * w.real) + np.abs(z.imag * w.imag))
        im = 2.0 ** -51 * (np.abs(z.real * w.imag) + np.abs(z.imag * w.real))
    return re, im


# ---- D. decompositions, matrix exponential and GEMM with non-finite entries ----------------------------------------------
DECOMP_TOL = 1e-10
SVD_ROUTES = [   # (name, complex?, shape)
    ('real in-LDS', False, (12, 10)), ('real in-LDS', False, (64, 64)), ('real pipeline', False, (100, 100)),
    ('real pipeline', False, (130, 70)), ('complex small', True, (20, 20)), ('complex large', True, (100, 100)),
]
EIGH_SIZES = (33, 100)


def decomp_block(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def poison_positions(shape):
    """first, a middle and the last entry"""
    return [(0, 0), (shape[0] // 2, shape[1] // 3), (shape[0] - 1, shape[1] - 1)]


def hermitian_block(n, cplx, seed):
    a = decomp_block((n, n), cplx, seed)
    return (a + a.conj().T) / 2


GEMM_NONFINITE_SHAPES = [(96, 80, 72), (300, 4, 64)]   # (M, N, K): an MFMA tile class; a skinny product (four columns)


# ---- E. random generators -------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
PHILOX_KAT = [   # Random123 known-answer vectors for philox4x32-10: (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: counter (..., 4) and key (..., 2) of 32-bit words held in uint64 -> (..., 4)"""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & _M32 for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & _M32 for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & _M32, (k[1] + np.uint64(0xBB67AE85)) & _M32]
    return np.stack(c, axis=-1)


def _philox_pairs(n, seed, stream):
    """the two 53-bit integers of every element pair: counter (pair lo, pair hi, stream, 0), key (seed lo, seed hi)"""
    npair = (n + 1) // 2
    p = np.arange(npair, dtype=np.uint64)
    counter = np.stack([p & _M32, p >> np.uint64(32), np.full(npair, stream, np.uint64), np.zeros(npair, np.uint64)], axis=-1)
    seed = int(seed) & (2 ** 64 - 1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (npair, 2))
    out = philox4x32_10(counter, key)
    a = ((out[:, 0] << np.uint64(32)) | out[:, 1]) >> np.uint64(11)
    b = ((out[:, 2] << np.uint64(32)) | out[:, 3]) >> np.uint64(11)
    return a, b


def model_uniform(n, seed, lo, hi):
    """random_uniform bit for bit: stream word 1, element 2p from the first 64 output bits, 2p + 1 from the second"""
    a, b = _philox_pairs(n, seed, 1)
    u = np.empty(2 * len(a))
    u[0::2] = a.astype(np.float64) * 2.0 ** -53
    u[1::2] = b.astype(np.float64) * 2.0 ** -53
    return (np.float64(lo) + np.float64(hi - lo) * u)[:n]


def model_normal(n, seed, sigma):
    """random_normal from the model's exact uniforms (stream word 0) and mpmath's Box-Muller: (values, rad)"""
    a, b = _philox_pairs(n, seed, 0)
    two_pi = mpmath.mpf(6.283185307179586)       # the kernel's double constant
    vals, rads = np.empty(2 * len(a)), np.empty(2 * len(a))
    with mp_ctx():
        for p, (ai, bi) in enumerate(zip(a, b)):
            u1 = (mpmath.mpf(int(ai)) + 1) / 2 ** 53
            u2 = mpmath.mpf(int(bi)) / 2 ** 53
            rad = sigma * mpmath.sqrt(-2 * mpmath.log(u1))
            vals[2 * p], vals[2 * p + 1] = float(rad * mpmath.cos(two_pi * u2)), float(rad * mpmath.sin(two_pi * u2))
            rads[2 * p] = rads[2 * p + 1] = float(rad)
    return vals[:n], rads[:n]


UNIFORM_LENGTHS = (1, 2, 3, 511, 4097)
UNIFORM_SEEDS = (0, 7, 2 ** 32 + 5, 2 ** 64 - 1)
UNIFORM_RANGES = ((0.0, 1.0), (-3.0, 5.0), (1.0, 1.0))
