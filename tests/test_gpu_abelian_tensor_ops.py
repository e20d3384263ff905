"""conj, dagger, diagonal tensors, scale_axis, partial_trace, trace_full and dense conversion of cyten_amd.abelian on the
device, and the grouped trace kernel behind them (csrc/trace_grouped.hip), float64 and complex128.

Oracles: the dense operation on the dense array (the reference's own criterion, tests/python_tests/test_tensors.py:3028-3036)
and the plain-numpy statement of the semantics in tests/abelian_tensor_ref.py for block tables.  Data movement (conj, dagger,
dense conversion, block tables) and scale_axis (one rounding per real multiplication, as in numpy) are bit-exact.  Traces
reorder sums: for n addends any order of summation is within gamma_(n-1) sum|x_i| of the exact sum, so two orders differ by at
most 2 n u sum|x_i| with u = 2**-53 -- the bound asserted element-wise here, sum|x_i| being the same trace of abs(dense) and n the
product of the traced dimensions (real and imaginary parts separately for complex data)."""
import collections
import ctypes

import numpy as np
import pytest

import abelian_tensor_ref as ref
from abelian_tensor_cases import CASE_IDS, case_tensor, diagonal_values, trace_cases
from cyten_amd import abelian as ab
from cyten_amd import workloads as wl
from oracle import block_ops as ops

pytestmark = pytest.mark.gpu

CASES = trace_cases()
U = 2.0 ** -53
BOTH = pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
ALL_CASES = pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)


def _same_legs(legs, specs):
    return len(legs) == len(specs) and all(l.sign == s.sign and np.array_equal(l.sectors, s.sectors) and np.array_equal(l.mults, s.mults)
                                           for l, s in zip(legs, specs))


def _identical(bb, got: ab.AbelianTensor, want: wl.TensorSpec):
    """same legs, block table and num_codomain; blocks bit for bit"""
    assert _same_legs(got.legs, want.legs)
    assert got.num_codomain == want.num_codomain
    assert np.array_equal(got.block_inds, np.asarray(want.block_inds).reshape(len(want.blocks), len(want.legs)))
    for x, y in zip(got.blocks, want.blocks):
        z = bb.to_numpy(x)
        assert z.dtype == np.asarray(y).dtype and np.array_equal(z, y)


def _within_bound(got, want, n, abs_sum):
    """|got - want| <= 2 n u sum|x_i| element-wise"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    return bool(np.all(np.abs(got - want) <= 2.0 * n * U * abs_sum))


def _trace_ok(got, want, n, abs_dense_trace):
    """the derived bound; complex data: real and imaginary parts separately (`abs_dense_trace` = (of |Re|, of |Im|))"""
    if np.iscomplexobj(want) or np.iscomplexobj(got):
        got, want = np.asarray(got, dtype=complex), np.asarray(want, dtype=complex)
        return _within_bound(got.real, want.real, n, abs_dense_trace[0]) and _within_bound(got.imag, want.imag, n, abs_dense_trace[1])
    return _within_bound(got, want, n, abs_dense_trace[0])


def _leg(spec, k, flip=False):
    l = spec.legs[k]
    return ab.Leg(ab.Symmetry(spec.moduli), l.sectors, l.mults, -l.sign if flip else l.sign)


class _CountingLib:
    """proxy of the loaded library that counts the C-ABI calls by name (cyten_amd/replay.py records them the same way)"""

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
    lib = _CountingLib(bb.lib)
    monkeypatch.setattr(bb, 'lib', lib)
    return lib


# --------------------------------------------------------------------------------------------- data movement: bit-exact

@BOTH
@ALL_CASES
def test_conj_dagger_are_bit_exact(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    t = ab.AbelianTensor.from_spec(bb, spec)
    _identical(bb, ab.conj(bb, t), ref.conj(spec))
    d = ab.dagger(bb, t)
    _identical(bb, d, ref.dagger(spec))
    assert np.array_equal(d.to_dense(bb), ref.dense_dagger(ref.to_dense(spec)))
    dd = ab.dagger(bb, d)
    _identical(bb, dd, spec)


@BOTH
@ALL_CASES
def test_dense_conversion_is_bit_exact(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    spec = wl.TensorSpec(spec.moduli, spec.legs, spec.block_inds[1:], spec.blocks[1:], spec.num_codomain)   # (an allowed block is absent)
    t = ab.AbelianTensor.from_spec(bb, spec)
    dense = ab.to_dense_block(bb, t)
    want_dense = ref.to_dense(spec)
    got_dense = bb.to_numpy(dense)
    assert got_dense.dtype == want_dense.dtype and np.array_equal(got_dense, want_dense)
    back = ab.from_dense_block(bb, t.symmetry, t.legs, dense, t.num_codomain)
    want, rest = ref.from_dense(spec.moduli, spec.legs, want_dense, spec.num_codomain)
    assert not rest.any() and len(back.blocks) > len(t.blocks)
    _identical(bb, back, want)
    bad = want_dense.copy()
    bad[tuple(np.argwhere(ref.to_dense(wl.TensorSpec(want.moduli, want.legs, want.block_inds, [np.ones(b.shape) for b in want.blocks]))
                          == 0)[0])] = 1.0
    with pytest.raises(ValueError, match='not symmetric'):
        ab.from_dense_block(bb, t.symmetry, t.legs, bb.as_block(bad), t.num_codomain)


@BOTH
@ALL_CASES
def test_scale_axis_is_bit_exact(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    t = ab.AbelianTensor.from_spec(bb, spec)
    for leg in (0, 1, len(spec.legs) - 1):
        vals, blocks = diagonal_values(spec.legs[leg])
        d = ab.DiagonalTensor.from_numpy(bb, _leg(spec, leg, flip=bool(leg)), vals)
        assert np.array_equal(d.to_numpy(bb), vals)
        _identical(bb, ab.scale_axis(bb, t, d, leg), ref.scale_axis(spec, blocks, leg))
        drop = int(spec.block_inds[0, leg])
        _, blocks2 = diagonal_values(spec.legs[leg], drop_sector=drop)
        keep = [i for i in range(len(d.blocks)) if i != drop]
        d2 = ab.DiagonalTensor(d.symmetry, d.leg, [d.blocks[i] for i in keep], np.array(keep))
        got2 = ab.scale_axis(bb, t, d2, leg)
        assert len(got2.blocks) < len(t.blocks)
        _identical(bb, got2, ref.scale_axis(spec, blocks2, leg))
    # a permuted tensor: strided blocks
    perm = list(range(1, len(spec.legs))) + [0]
    tp = ab.permute_legs(bb, t, perm)
    vals, _ = diagonal_values(spec.legs[0])
    d = ab.DiagonalTensor.from_numpy(bb, _leg(spec, 0), vals)
    got = ab.scale_axis(bb, tp, d, len(perm) - 1)
    assert np.array_equal(got.to_dense(bb), np.transpose(ref.to_dense(ref.scale_axis(spec, diagonal_values(spec.legs[0])[1], 0)), perm))


# --------------------------------------------------------------------------------------------- diagonal tensors

_PER_BLOCK = {
    'abs': lambda bb, b, p: bb.abs(b), 'sqrt': lambda bb, b, p: bb.sqrt(b), 'exp': lambda bb, b, p: bb.exp(b),
    'log': lambda bb, b, p: bb.log(b), 'neg': lambda bb, b, p: bb._unary(b, 4), 'square': lambda bb, b, p: bb._unary(b, 5),
    'reciprocal': lambda bb, b, p: bb._unary(b, 6), 'cutoff_inverse': lambda bb, b, p: bb.cutoff_inverse(b, p),
    'stable_log': lambda bb, b, p: bb.stable_log(b, p), 'pow': lambda bb, b, p: bb._pow(b, p)}
# (function, rtol): abs / neg / square / reciprocal / cutoff_inverse are single correctly rounded operations (exact); sqrt 1e-15
# (tests/test_gpu_blockops.py:160); stable_log and pow 1e-14 (tests/test_gpu_api_surface.py:57-61); exp / log: two libm
# implementations, each within a few ulp of the exact value, 1e-14 as for stable_log
_NUMPY = {
    'abs': (np.abs, 0.0), 'sqrt': (np.sqrt, 1e-15), 'exp': (np.exp, 1e-14), 'log': (np.log, 1e-14), 'neg': (np.negative, 0.0),
    'square': (np.square, 0.0), 'reciprocal': (lambda x: 1.0 / x, 0.0), 'cutoff_inverse': (ops.cutoff_inverse, 0.0),
    'stable_log': (ops.stable_log, 1e-14), 'pow': (np.power, 1e-14)}


@pytest.mark.parametrize('func,param', [('abs', None), ('sqrt', None), ('exp', None), ('log', None), ('neg', None), ('square', None),
                                        ('reciprocal', None), ('cutoff_inverse', 1e-10), ('stable_log', 1e-10), ('pow', 1.5)])
def test_diagonal_unary_is_the_per_block_kernel_in_one_launch(bb, func, param):
    leg = wl.u1_leg(300, 2.0)
    vals, _ = diagonal_values(leg)
    L = ab.Leg(ab.Symmetry((0,)), leg.sectors, leg.mults, leg.sign)
    d = ab.DiagonalTensor.from_numpy(bb, L, vals)
    got = ab.diagonal_unary(bb, d, func, param)
    assert np.array_equal(got.block_inds, d.block_inds)
    for g, b in zip(got.blocks, d.blocks):
        assert np.array_equal(bb.to_numpy(g), bb.to_numpy(_PER_BLOCK[func](bb, b, param)))
    np_func, rtol = _NUMPY[func]
    want = np_func(vals) if param is None else np_func(vals, param)
    if rtol:
        np.testing.assert_allclose(got.to_numpy(bb), want, rtol=rtol, atol=0.0)
    else:
        np.testing.assert_array_equal(got.to_numpy(bb), want)
    if func == 'cutoff_inverse':
        assert got.to_numpy(bb)[0] == 0.0          # (the tiny value is cut)
    # absent sectors: left out, or created as zero blocks first
    part = ab.DiagonalTensor(d.symmetry, L, d.blocks[2:], d.block_inds[2:])
    assert np.array_equal(ab.diagonal_unary(bb, part, func, param).block_inds, part.block_inds)
    if func in ('exp', 'cutoff_inverse', 'stable_log'):
        full = ab.diagonal_unary(bb, part, func, param, maps_zero_to_zero=False)
        assert np.array_equal(full.block_inds, np.arange(L.nsec))
        v0 = vals.copy()
        v0[:int(L.slices[2])] = 0.0
        want0 = np_func(v0) if param is None else np_func(v0, param)
        np.testing.assert_allclose(full.to_numpy(bb), want0, rtol=rtol, atol=0.0)


def test_unary_many_refuses_what_it_does_not_serve(bb):
    b = bb.as_block(np.ones(3))
    with pytest.raises(ValueError):
        bb.unary_many([b], 'tanh')
    with pytest.raises(ValueError):
        bb.unary_many([b], 'pow')
    with pytest.raises(ValueError):
        bb.unary_many([b], 'sqrt', 2.0)
    with pytest.raises(NotImplementedError):
        bb.unary_many([bb.as_block(np.ones(3) + 1j)], 'sqrt')
    assert bb.unary_many([], 'sqrt') == []


# --------------------------------------------------------------------------------------------- traces

def _abs_traces(spec, pairs):
    dense = ref.to_dense(spec)
    return (ref.dense_partial_trace(np.abs(dense.real), spec, pairs), ref.dense_partial_trace(np.abs(dense.imag), spec, pairs))


@BOTH
@ALL_CASES
def test_partial_trace_within_the_reordering_bound(bb, case, cplx):
    c = CASES[case]
    spec = case_tensor(c, cplx)
    pairs = c['pairs']
    t = ab.AbelianTensor.from_spec(bb, spec)
    got = ab.partial_trace(bb, t, pairs)
    again = ab.partial_trace(bb, t, pairs)
    want_struct, _ = ref.partial_trace(spec, pairs)
    want = ref.dense_partial_trace(ref.to_dense(spec), spec, pairs)
    n = int(np.prod([int(spec.legs[i].mults.sum()) for i, _ in pairs]))
    sums = _abs_traces(spec, pairs)
    if c['name'] == 'scalar':
        assert isinstance(got, complex if cplx else float)
        print(f'{CASE_IDS[case]} {"c128" if cplx else "f64"}: |got - want| = {abs(got - want):.3e}, bound = {2 * n * U * sums[0]:.3e}')
        assert _trace_ok(got, want, n, sums)
        assert got == again                                     # bit-identical from run to run
        assert ab.trace_full(bb, t) == got
        return
    assert _same_legs(got.legs, want_struct.legs) and got.num_codomain == want_struct.num_codomain
    assert np.array_equal(got.block_inds, want_struct.block_inds)
    got.check_charges()
    got_dense = got.to_dense(bb)
    err = np.abs(got_dense - want)
    print(f'{CASE_IDS[case]} {"c128" if cplx else "f64"}: max |got - want| = {err.max():.3e}, '
          f'max bound = {(2 * n * U * (sums[0] + sums[1])).max():.3e}')
    assert _trace_ok(got_dense, want, n, sums)
    for x, y in zip(got.blocks, again.blocks):
        assert np.array_equal(bb.to_numpy(x), bb.to_numpy(y))      # bit-identical from run to run
    # a permuted tensor (strided blocks) traces to the same thing
    perm = list(range(len(spec.legs)))[::-1]
    tp = ab.permute_legs(bb, t, perm)
    gp = ab.partial_trace(bb, tp, [(perm.index(i), perm.index(j)) for i, j in pairs])
    rem = [k for k in range(len(perm)) if k not in [x for p in pairs for x in p]]
    assert _trace_ok(gp.to_dense(bb), np.transpose(want, list(range(len(rem)))[::-1]), n, tuple(np.transpose(s, list(range(len(rem)))[::-1]) for s in sums))


def test_trace_of_dagger_compose_is_the_squared_norm(bb):
    for c in CASES[:4]:
        for cplx in (False, True):
            a = ab.AbelianTensor.from_spec(bb, case_tensor(c, cplx))
            rho = ab.compose(bb, ab.dagger(bb, a), a, a.nlegs - 1)
            tr = ab.trace_full(bb, rho)
            want = ab.norm(bb, a) ** 2
            assert abs(tr - want) <= 1e-12 * want


def test_partial_trace_keeps_the_labels_of_the_remaining_legs(bb):
    c = CASES[CASE_IDS.index('U1-two_pairs')]
    t = ab.AbelianTensor.from_spec(bb, c['tensor'])
    t.labels = ['a', 'b', 'b*', 'a*', 'c', 'c*']
    assert ab.partial_trace(bb, t, c['pairs']).labels == ['c', 'c*']
    assert ab.partial_trace(bb, ab.AbelianTensor.from_spec(bb, c['tensor']), c['pairs']).labels == []


def test_partial_trace_errors(bb):
    moduli = (0,)
    a = wl.make_leg(moduli, [[-1], [0], [1]], [2, 3, 1], +1)
    other = wl.make_leg(moduli, [[-1], [0], [1]], [2, 2, 1], -1)
    t = ab.AbelianTensor.from_spec(bb, wl.random_tensor(moduli, [a, other], np.random.default_rng(0), num_codomain=1))
    with pytest.raises(ValueError):
        ab.partial_trace(bb, t, [(0, 1)])
    empty = ab.AbelianTensor.from_spec(bb, wl.TensorSpec(moduli, [a, wl.flip(a)], np.zeros((0, 2), int), [], 1))
    assert ab.partial_trace(bb, empty, [(0, 1)]) == 0.0


# --------------------------------------------------------------------------------------------- launch counts

def test_one_launch_per_operation_whatever_the_number_of_blocks(bb, counted):
    c = CASES[CASE_IDS.index('Z3-two_pairs')]
    for cplx in (False, True):
        spec = case_tensor(c, cplx)
        t = ab.AbelianTensor.from_spec(bb, spec)
        assert len(t.blocks) > 100
        suffix = 'c128' if cplx else 'f64'
        counted.calls.clear()
        res = ab.partial_trace(bb, t, c['pairs'])
        assert len(res.blocks) > 1 and dict(counted.calls) == {f'cyb_trace_grouped_{suffix}': 1}
        vals, _ = diagonal_values(spec.legs[0])
        d = ab.DiagonalTensor.from_numpy(bb, _leg(spec, 0), vals)
        counted.calls.clear()
        ab.scale_axis(bb, t, d, 0)
        assert dict(counted.calls) == {'cyb_scale_axis_batched_f64': 1}
        counted.calls.clear()
        dense = ab.to_dense_block(bb, t)
        assert dict(counted.calls) == {'cyb_memset': 1, 'cyb_copy_strided_batched': 1}
        counted.calls.clear()
        ab.from_dense_block(bb, t.symmetry, t.legs, dense, t.num_codomain, tol=None)
        assert dict(counted.calls) == {'cyb_copy_strided_batched': 1}
        counted.calls.clear()
        ab.dagger(bb, t)
        assert dict(counted.calls) == ({'cyb_copy_strided_batched': 1} if cplx else {})
    leg = wl.u1_leg(300, 2.0)
    d = ab.DiagonalTensor.from_numpy(bb, ab.Leg(ab.Symmetry((0,)), leg.sectors, leg.mults, +1), diagonal_values(leg)[0])
    assert len(d.blocks) > 10
    counted.calls.clear()
    ab.diagonal_unary(bb, d, 'sqrt')
    assert dict(counted.calls) == {'cyb_unary_batched_f64': 1}
    counted.calls.clear()
    ab.diagonal_unary(bb, d, 'cutoff_inverse', 1e-10)
    assert dict(counted.calls) == {'cyb_unary_param_batched_f64': 1}
    scalar_case = CASES[CASE_IDS.index('Z3-scalar')]
    t = ab.AbelianTensor.from_spec(bb, scalar_case['tensor'])
    counted.calls.clear()
    ab.trace_full(bb, t)
    assert dict(counted.calls) == {'cyb_trace_grouped_f64': 1}


# --------------------------------------------------------------------------------------------- the kernel, directly

def _einsum_spec(ndim, idcs1, idcs2, remaining):
    letters = 'abcdefgh'
    sub = [None] * ndim
    for k, r in enumerate(remaining):
        sub[r] = letters[k]
    for k, (i, j) in enumerate(zip(idcs1, idcs2)):
        sub[i] = sub[j] = letters[len(remaining) + k]
    return ''.join(sub) + '->' + ''.join(letters[:len(remaining)])


def _check_outputs(bb, outputs_np):
    """outputs_np: [(shape, [(numpy array or (numpy array, view permutation), idcs1, idcs2, remaining)])]; runs ONE grouped
    trace and compares every result with the sum of np.einsum over its terms, within the reordering bound"""
    dev = []
    for shape, terms in outputs_np:
        dterms = []
        for a, i1, i2, rem in terms:
            perm = None
            if isinstance(a, tuple):
                a, perm = a
            blk = bb.as_block(a)
            if perm is not None:
                blk = bb.permute_axes(blk, perm)
            dterms.append((blk, i1, i2, rem))
        dev.append((shape, dterms))
    got = bb.trace_partial_grouped(dev)
    again = bb.trace_partial_grouped(dev)
    assert len(got) == len(outputs_np)
    # (one dtype for the whole call: a list that mixes float64 and complex128 sources is promoted)
    cplx = any(np.iscomplexobj(t[0][0] if isinstance(t[0], tuple) else t[0]) for _, terms in outputs_np for t in terms)
    for g, g2, (shape, terms) in zip(got, again, outputs_np):
        want = np.zeros(shape, dtype=complex if cplx else float)
        s_re, s_im, n = np.zeros(shape), np.zeros(shape), 0
        for a, i1, i2, rem in terms:
            if isinstance(a, tuple):
                a = np.transpose(a[0], a[1])
            es = _einsum_spec(a.ndim, [i % a.ndim for i in i1], [i % a.ndim for i in i2], [i % a.ndim for i in rem])
            want = want + np.einsum(es, a)
            s_re = s_re + np.einsum(es, np.abs(a.real))
            s_im = s_im + np.einsum(es, np.abs(a.imag))
            n += int(np.prod([a.shape[i] for i in i1]))
        res = bb.to_numpy(g)
        assert res.shape == tuple(shape) and res.dtype == want.dtype
        assert _trace_ok(res, want, max(n, 1), (s_re, s_im))
        assert np.array_equal(res, bb.to_numpy(g2))
    return got


@BOTH
def test_kernel_pairs_axes_and_strides(bb, cplx, rng):
    def arr(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a
    outputs = [
        ((3,), [(arr(6, 3, 6), [0], [2], [1])]),                                          # one pair, lane
        ((5,), [(arr(3, 4, 5, 4, 3), [0, 1], [4, 3], [2])]),                              # two pairs
        ((5,), [(arr(2, 3, 4, 5, 4, 3, 2), [0, 1, 2], [6, 5, 4], [3])]),                  # three pairs
        ((), [(arr(2, 3, 2, 3, 3, 2, 3, 2), [0, 1, 2, 3], [7, 6, 5, 4], [])]),            # four pairs, nothing remains
        ((), [(arr(9, 9), [0], [1], [])]),                                                # no remaining axis
        ((7,), [(arr(5, 5, 7), [0], [1], [2])]),                                          # remaining axis innermost
        ((7,), [(arr(7, 5, 5), [1], [2], [0])]),                                          # ... and outermost
        ((7, 4), [(arr(7, 5, 4, 5), [1], [3], [0, 2])]),
        ((4, 7), [(arr(7, 5, 4, 5), [1], [3], [2, 0])]),                                  # remaining axes in another order
        ((5,), [(arr(1, 5, 1), [0], [2], [1])]),                                          # extent 1
        ((5,), [(arr(0, 5, 0), [0], [2], [1])]),                                          # extent 0 traced: zeros
        ((0,), [(arr(4, 0, 4), [0], [2], [1])]),                                          # extent 0 remaining: nothing to write
        ((4, 3), []),                                                                     # no term: zeros
        ((6, 5), [((arr(5, 4, 6, 4), [2, 1, 0, 3]), [1], [3], [0, 2])]),                  # a permuted (strided) source
        ((5,), [((arr(3, 4, 5, 4, 3), [4, 3, 2, 1, 0]), [0, 1], [4, 3], [2]), (arr(2, 5, 2), [0], [2], [1])]),
        ((7,), [(arr(100, 7, 100), [0], [2], [1])]),                                      # 100 addends: a wave per element
        ((3,), [(arr(10, 9, 3, 9, 10), [0, 1], [4, 3], [2])]),                            # wave, two pairs
        ((2, 3), [(arr(2, 70, 3, 70), [1], [3], [0, 2]), ((arr(3, 80, 80, 2), [3, 1, 2, 0]), [1], [2], [0, 3])]),
        ((260, 260), [(arr(8, 8, 260, 260), [0], [1], [2, 3])]),                          # 67600 elements: lanes
    ]
    got = _check_outputs(bb, outputs)
    assert not np.any(bb.to_numpy(got[12])) and not np.any(bb.to_numpy(got[10]))
    assert bb.trace_partial_grouped([]) == []


def test_kernel_mixed_dtypes_are_promoted(bb, rng, counted):
    """float64 sources next to complex128 ones: every float64 source is promoted into its own place (DIFFERENT real arrays of
    equal shape into one sum: a promoted copy whose memory were handed out again before the launch would give a wrong sum), by
    one memset and one batched copy for the whole list"""
    reals = [rng.standard_normal((4, 3, 4)) for _ in range(6)]
    b = rng.standard_normal((5, 3, 5)) + 1j * rng.standard_normal((5, 3, 5))
    strided = rng.standard_normal((3, 6, 6))
    outputs = [((3,), [(reals[0], [0], [2], [1]), (reals[1], [0], [2], [1]), (b, [0], [2], [1])]),
               ((3,), [(a, [0], [2], [1]) for a in reals[2:]] + [((strided, [1, 0, 2]), [0], [2], [1])]),
               ((3,), [(reals[0], [0], [2], [1])])]
    counted.calls.clear()
    got = _check_outputs(bb, outputs)
    assert all(g.dtype == np.dtype('complex128') for g in got)
    # _check_outputs runs the grouped trace twice
    assert dict(counted.calls) == {'cyb_memset': 2, 'cyb_copy_strided_batched': 2, 'cyb_trace_grouped_c128': 2}


def test_kernel_regime_thresholds(bb, rng):
    """the owner of an output element at the thresholds csrc/trace_grouped.hip states: 64 addends per element stay with one lane
    per element once the output has 65536 elements or more; 4096 addends per element stay with one wave per element once the
    output has 1024 elements or more.  (The addends come from many terms with a small traced extent, so that the sources stay small.)"""
    lanes = [(rng.standard_normal((4, 260, 4, 260)), [0], [2], [1, 3]) for _ in range(16)]          # R = 67600, A = 16 * 4 = 64
    _check_outputs(bb, [((260, 260), lanes)])
    waves = [(rng.standard_normal((32, 4, 4, 32)), [1], [2], [0, 3]) for _ in range(1024)]         # R = 1024, A = 1024 * 4 = 4096
    _check_outputs(bb, [((32, 32), waves)])
    group = [(rng.standard_normal((31, 4, 4, 33)), [1], [2], [0, 3]) for _ in range(1024)]         # R = 1023: a workgroup per element
    _check_outputs(bb, [((31, 33), group)])


@BOTH
def test_kernel_many_terms_and_many_outputs(bb, cplx, rng):
    def arr(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a
    fifty = [(arr(int(m), 6, int(m)), [0], [2], [1]) for m in rng.integers(1, 9, 50)]
    _check_outputs(bb, [((6,), fifty)])
    many = [((int(r),), [(arr(int(m), int(r), int(m)), [0], [2], [1])]) for r, m in zip(rng.integers(1, 6, 300), rng.integers(1, 6, 300))]
    _check_outputs(bb, many)


@BOTH
def test_kernel_trace_full_regime_and_streaming_regime(bb, cplx, rng):
    def arr(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a
    _check_outputs(bb, [((), [(arr(4096, 4096), [0], [1], [])])])                        # one element, 4096 addends: a workgroup
    _check_outputs(bb, [((512, 512), [(arr(512, 2, 2, 512), [1], [2], [0, 3])])])        # 262144 elements, 4 addends each: lanes
    _check_outputs(bb, [((), [(arr(68, 64, 68, 64), [0, 1], [2, 3], [])])])              # a workgroup, two pairs (4352 addends)


def test_kernel_argument_checks(bb, rng):
    a = bb.as_block(rng.standard_normal((4, 3, 4)))
    with pytest.raises(ValueError):
        bb.trace_partial_grouped([((3,), [(bb.as_block(rng.standard_normal((4, 3, 5))), [0], [2], [1])])])      # extents differ
    with pytest.raises(ValueError):
        bb.trace_partial_grouped([((4,), [(a, [0], [2], [1])])])                                                 # wrong result shape
    with pytest.raises(ValueError):
        bb.trace_partial_grouped([((3,), [(a, [0], [0], [1])])])                                                 # an axis twice
    ten = bb.as_block(np.zeros((1,) * 10))
    with pytest.raises(ValueError):
        bb.trace_partial_grouped([((), [(ten, [0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [])])])                          # five pairs
    with pytest.raises(TypeError):
        bb.trace_partial_grouped([((3,), [(bb.as_block(np.ones((2, 3, 2), dtype=bool)), [0], [2], [1])])])


def test_descriptor_layouts_match_the_header():
    from cyten_amd import _lib
    assert _lib.CYB_TRACE_MAX_PAIRS == 4
    assert ctypes.sizeof(_lib.TraceOut) == 8 + 4 * 2 + 8 * 2 + 8 * 8
    assert ctypes.sizeof(_lib.TraceTerm) == 8 + 4 * 2 + 8 * 8 + 8 * 4 * 2
    assert _lib.TRACE_OUT_DTYPE.itemsize == 96 and _lib.TRACE_TERM_DTYPE.itemsize == 144
