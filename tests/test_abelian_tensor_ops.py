"""conj, dagger, diagonal tensors, scale_axis, partial_trace, trace_full and dense conversion of cyten_amd.abelian on the CPU:
the host logic on the numpy stand-in against two oracles -- the dense operation on the dense array (the reference's own
criterion, tests/python_tests/test_tensors.py:3028-3036 for partial_trace, :3295 scale_axis, :1885 dagger, :3841 trace) and the
plain-numpy statement of the semantics in tests/abelian_tensor_ref.py (block tables, legs, num_codomain) -- to 1e-12 relative,
plus identities that need no oracle."""
import numpy as np
import pytest

import abelian_tensor_ref as ref
from abelian_tensor_cases import CASE_IDS, case_tensor, diagonal_values, dual_same_sign, trace_cases
from cyten_amd import abelian as ab
from cyten_amd import workloads as wl
from numpy_tensor_backend import NumpyTensorBackend

CASES = trace_cases()
RTOL = 1e-12


def _close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.abs(got - want).max(initial=0.0) <= RTOL * max(1.0, np.abs(want).max(initial=0.0))


def _same_legs(legs, specs):
    return len(legs) == len(specs) and all(l.sign == s.sign and np.array_equal(l.sectors, s.sectors) and np.array_equal(l.mults, s.mults)
                                           for l, s in zip(legs, specs))


def _matches(bb, got: ab.AbelianTensor, want: wl.TensorSpec):
    """same legs, same block table, same num_codomain, blocks to 1e-12"""
    assert _same_legs(got.legs, want.legs)
    assert got.num_codomain == want.num_codomain
    assert np.array_equal(got.block_inds, np.asarray(want.block_inds).reshape(len(want.blocks), len(want.legs)))
    for x, y in zip(got.blocks, want.blocks):
        assert _close(bb.to_numpy(x), y)


def _leg(spec, k, flip=False):
    l = spec.legs[k]
    return ab.Leg(ab.Symmetry(spec.moduli), l.sectors, l.mults, -l.sign if flip else l.sign)


@pytest.fixture
def bb():
    return NumpyTensorBackend()


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
def test_partial_trace_against_both_oracles(bb, case, cplx):
    c = CASES[case]
    spec = case_tensor(c, cplx)
    t = ab.AbelianTensor.from_spec(bb, spec)
    got = ab.partial_trace(bb, t, c['pairs'])
    want, _ = ref.partial_trace(spec, c['pairs'])
    dense = ref.dense_partial_trace(ref.to_dense(spec), spec, c['pairs'])
    if c['name'] == 'scalar':
        assert isinstance(got, complex if cplx else float)
        assert _close(got, want) and _close(got, dense)
        return
    _matches(bb, got, want)
    got.check_charges()
    assert _close(got.to_dense(bb), dense)


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
def test_conj_dagger_against_both_oracles(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    t = ab.AbelianTensor.from_spec(bb, spec)
    dense = ref.to_dense(spec)
    c = ab.conj(bb, t)
    _matches(bb, c, ref.conj(spec))
    c.check_charges()
    assert np.array_equal(c.to_dense(bb), np.conj(dense))
    d = ab.dagger(bb, t)
    _matches(bb, d, ref.dagger(spec))
    d.check_charges()
    assert np.array_equal(d.to_dense(bb), ref.dense_dagger(dense))
    # dagger is an involution, exactly
    dd = ab.dagger(bb, d)
    assert _same_legs(dd.legs, spec.legs) and dd.num_codomain == t.num_codomain and np.array_equal(dd.block_inds, t.block_inds)
    for x, y in zip(dd.blocks, t.blocks):
        assert np.array_equal(bb.to_numpy(x), bb.to_numpy(y))


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
def test_scale_axis_against_both_oracles_and_dropped_sectors(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    t = ab.AbelianTensor.from_spec(bb, spec)
    dense = ref.to_dense(spec)
    for leg in (0, len(spec.legs) - 1):
        vals, blocks = diagonal_values(spec.legs[leg])
        d = ab.DiagonalTensor.from_numpy(bb, _leg(spec, leg, flip=bool(leg)), vals)        # (either sign serves)
        assert np.array_equal(d.to_numpy(bb), vals)
        got = ab.scale_axis(bb, t, d, leg)
        _matches(bb, got, ref.scale_axis(spec, blocks, leg))
        assert _close(got.to_dense(bb), ref.dense_scale_axis(dense, vals, leg))
        # a diagonal that lacks a sector: the blocks of that sector are dropped, the others are scaled
        drop = int(spec.block_inds[0, leg])
        vals2, blocks2 = diagonal_values(spec.legs[leg], drop_sector=drop)
        keep = [i for i in range(len(d.blocks)) if i != drop]
        d2 = ab.DiagonalTensor(d.symmetry, d.leg, [d.blocks[i] for i in keep], np.array(keep))
        got2 = ab.scale_axis(bb, t, d2, leg)
        assert len(got2.blocks) < len(t.blocks) and not np.any(got2.block_inds[:, leg] == drop)
        _matches(bb, got2, ref.scale_axis(spec, blocks2, leg))
        sl = t.legs[leg].slices
        vals2 = vals2.copy()
        vals2[int(sl[drop]):int(sl[drop + 1])] = 0.0
        assert _close(got2.to_dense(bb), ref.dense_scale_axis(dense, vals2, leg))
        assert np.array_equal(d2.to_numpy(bb), vals2)


def test_scale_axis_refuses_another_leg_and_a_complex_diagonal(bb):
    spec = CASES[0]['tensor']
    t = ab.AbelianTensor.from_spec(bb, spec)
    vals, _ = diagonal_values(spec.legs[0])
    d = ab.DiagonalTensor.from_numpy(bb, t.legs[0], vals)
    with pytest.raises(ValueError):
        ab.scale_axis(bb, t, d, 1)
    dc = ab.DiagonalTensor.from_numpy(bb, t.legs[0], vals + 1j)
    with pytest.raises(NotImplementedError):
        ab.scale_axis(bb, t, dc, 0)


@pytest.mark.parametrize('func,param,np_func', [
    ('sqrt', None, np.sqrt), ('abs', None, np.abs), ('exp', None, np.exp), ('log', None, np.log), ('neg', None, np.negative),
    ('square', None, np.square), ('reciprocal', None, lambda x: 1.0 / x),
    ('cutoff_inverse', 1e-10, lambda x: 1.0 / np.where(np.abs(x) < 1e-10, np.inf, x)),
    ('stable_log', 1e-10, lambda x: np.log(np.where(x > 1e-10, x, 1.0))), ('pow', 1.5, lambda x: x ** 1.5)])
def test_diagonal_unary(bb, func, param, np_func):
    vals, _ = diagonal_values(CASES[0]['tensor'].legs[0])
    L = _leg(CASES[0]['tensor'], 0)
    sym = L.symmetry
    d = ab.DiagonalTensor.from_numpy(bb, L, vals)
    got = ab.diagonal_unary(bb, d, func, param)
    assert np.array_equal(got.block_inds, d.block_inds)
    assert _close(got.to_numpy(bb), np_func(vals))
    # a diagonal without its first sector: kept out (maps_zero_to_zero) or created as a zero block first
    part = ab.DiagonalTensor(sym, L, d.blocks[1:], d.block_inds[1:])
    kept = ab.diagonal_unary(bb, part, func, param)
    assert np.array_equal(kept.block_inds, part.block_inds) and len(kept.blocks) == L.nsec - 1
    if func in ('exp', 'cutoff_inverse', 'stable_log'):     # (finite at zero)
        full = ab.diagonal_unary(bb, part, func, param, maps_zero_to_zero=False)
        assert np.array_equal(full.block_inds, np.arange(L.nsec))
        v0 = vals.copy()
        v0[:int(L.slices[1])] = 0.0
        assert _close(full.to_numpy(bb), np_func(v0))
    with pytest.raises(ValueError):
        ab.diagonal_unary(bb, d, 'tanh')


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
def test_dense_round_trip(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    spec = wl.TensorSpec(spec.moduli, spec.legs, spec.block_inds[1:], spec.blocks[1:], spec.num_codomain)   # (an allowed block is absent)
    t = ab.AbelianTensor.from_spec(bb, spec)
    dense = ab.to_dense_block(bb, t)
    assert np.array_equal(bb.to_numpy(dense), ref.to_dense(spec))
    back = ab.from_dense_block(bb, t.symmetry, t.legs, dense, t.num_codomain)
    want, rest = ref.from_dense(spec.moduli, spec.legs, ref.to_dense(spec), spec.num_codomain)
    assert not rest.any()
    assert back.num_codomain == t.num_codomain and np.array_equal(back.block_inds, want.block_inds)
    assert len(back.blocks) > len(t.blocks)          # (the absent allowed blocks come back as zeros)
    have = {tuple(r): b for r, b in zip(t.block_inds.tolist(), t.blocks)}
    for row, blk, w in zip(back.block_inds.tolist(), back.blocks, want.blocks):
        assert np.array_equal(bb.to_numpy(blk), w)
        src = have.get(tuple(row))
        assert np.array_equal(bb.to_numpy(blk), bb.to_numpy(src)) if src is not None else not np.any(bb.to_numpy(blk))
    # one entry outside the allowed blocks: not symmetric
    bad = ref.to_dense(spec).copy()
    allowed = np.zeros(bad.shape, dtype=bool)
    for row in want.block_inds:
        allowed[tuple(slice(int(l.slices[i]), int(l.slices[i + 1])) for l, i in zip(t.legs, row))] = True
    pos = tuple(np.argwhere(~allowed)[0])
    bad[pos] = 1.0
    with pytest.raises(ValueError, match='not symmetric'):
        ab.from_dense_block(bb, t.symmetry, t.legs, bb.as_block(bad), t.num_codomain)
    assert len(ab.from_dense_block(bb, t.symmetry, t.legs, bb.as_block(bad), t.num_codomain, tol=None).blocks) == len(want.blocks)


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
def test_trace_of_dagger_compose_is_the_squared_norm(bb, case, cplx):
    spec = case_tensor(CASES[case], cplx)
    a = ab.AbelianTensor.from_spec(bb, spec)
    for k in (a.nlegs - 1, a.nlegs - 2):                      # (a reduced density matrix on one / two legs)
        rho = ab.compose(bb, ab.dagger(bb, a), a, k)          # legs [a_{n-1}*, ..., a_k*, a_k, ..., a_{n-1}]
        rho.num_codomain = rho.nlegs // 2
        tr = ab.trace_full(bb, rho)
        want = ab.norm(bb, a) ** 2
        assert abs(tr - want) <= RTOL * want
        assert _close(tr, ref.trace_full(wl.TensorSpec(spec.moduli, [wl.LegSpec(l.sectors, l.mults, l.sign) for l in rho.legs],
                                                       rho.block_inds, [bb.to_numpy(b) for b in rho.blocks], rho.num_codomain)))


def test_trace_full_against_the_dense_trace(bb):
    for c in CASES:
        if c['name'] != 'scalar':
            continue
        spec = c['tensor']
        t = ab.AbelianTensor.from_spec(bb, spec)
        want = np.einsum('abba', ref.to_dense(spec))
        assert _close(ab.trace_full(bb, t), want)
        assert _close(ref.trace_full(spec), want)
    with pytest.raises(ValueError):
        ab.trace_full(bb, ab.AbelianTensor.from_spec(bb, CASES[0]['tensor']))      # five legs


def test_partial_trace_keeps_the_labels_of_the_remaining_legs(bb):
    c = CASES[CASE_IDS.index('U1-two_pairs')]
    t = ab.AbelianTensor.from_spec(bb, c['tensor'])
    t.labels = ['a', 'b', 'b*', 'a*', 'c', 'c*']
    assert ab.partial_trace(bb, t, c['pairs']).labels == ['c', 'c*']
    assert ab.partial_trace(bb, ab.AbelianTensor.from_spec(bb, c['tensor']), c['pairs']).labels == []


def test_partial_trace_refuses_legs_that_are_not_dual(bb):
    moduli = (0,)
    a = wl.make_leg(moduli, [[-1], [0], [1]], [2, 3, 1], +1)
    other = wl.make_leg(moduli, [[-1], [0], [1]], [2, 2, 1], -1)          # same sectors, unequal multiplicities
    fewer = wl.make_leg(moduli, [[-1], [0]], [2, 3], -1)
    rng = np.random.default_rng(0)
    for partner in (other, fewer, a):                                      # (a itself: same sign, charges do not cancel)
        spec = wl.random_tensor(moduli, [a, partner], rng, num_codomain=1)
        t = ab.AbelianTensor.from_spec(bb, spec)
        with pytest.raises(ValueError):
            ab.partial_trace(bb, t, [(0, 1)])
        with pytest.raises(ValueError):
            ref.partial_trace(spec, [(0, 1)])
    spec = wl.random_tensor(moduli, [a, wl.flip(a), a, dual_same_sign(a, moduli)], rng, num_codomain=2)
    t = ab.AbelianTensor.from_spec(bb, spec)
    with pytest.raises(ValueError):
        ab.partial_trace(bb, t, [(0, 1), (1, 2)])                          # a leg listed twice
    assert ab.partial_trace(bb, t, [(0, 1), (2, 3)]) == pytest.approx(ref.partial_trace(spec, [(0, 1), (2, 3)])[0], rel=1e-12)


def test_partial_trace_without_a_diagonal_block_is_zero(bb):
    moduli = (0,)
    a = wl.make_leg(moduli, [[0], [1]], [2, 2], +1)
    empty = ab.AbelianTensor.from_spec(bb, wl.TensorSpec(moduli, [a, wl.flip(a)], np.zeros((0, 2), int), [], 1))
    assert ab.partial_trace(bb, empty, [(0, 1)]) == 0.0
    # [a, a^, a*]: a block with sectors (0, 1, ...) is off the diagonal of (0, 1); a tensor holding only such blocks traces to nothing
    legs = [a, dual_same_sign(a, moduli), wl.flip(a)]
    inds = np.array([r for r in wl.allowed_block_inds(moduli, legs) if r[0] == r[1]])      # q_0 - (-q_1) != 0  <=>  same index here
    off = [r for r in inds if np.any(a.sectors[r[0]] + legs[1].sectors[r[1]] != 0)]
    assert off
    spec = wl.TensorSpec(moduli, legs, np.array(off), [np.ones((2, 2, 2)) for _ in off], 2)
    res = ab.partial_trace(bb, ab.AbelianTensor.from_spec(bb, spec), [(0, 1)])
    assert len(res.blocks) == 0 and res.block_inds.shape == (0, 1) and res.num_codomain == 0


def test_trace_descriptor_layouts_match_the_header():
    """ctypes mirrors of cyb_trace_out / cyb_trace_term have the C sizes (LP64), as tests/test_cabi.py checks the others"""
    import ctypes
    from cyten_amd import _lib
    assert _lib.CYB_TRACE_MAX_PAIRS == 4
    assert ctypes.sizeof(_lib.TraceOut) == 8 + 4 * 2 + 8 * 2 + 8 * _lib.CYB_MAX_NDIM
    assert ctypes.sizeof(_lib.TraceTerm) == 8 + 4 * 2 + 8 * _lib.CYB_MAX_NDIM + 8 * 4 * 2
