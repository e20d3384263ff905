"""Diagonal-tensor arithmetic, reductions and device-side masks of cyten_amd.abelian on the two numpy stand-ins (the grouped
one and the per-block loop), against the restatement of the reference one sector at a time (tests/diag_mask_ref.py).  The
stand-ins compute with numpy as the restatement does, so every comparison here is exact (``np.array_equal``; NaN from 0 / 0
equals NaN)."""
import os

import numpy as np
import pytest

import diag_mask_ref as ref
from cyten_amd import abelian as ab
from diag_mask_cases import DTYPES, flags_cases, legs, pair_cases, single_cases, to_diag
from test_golden import GOLD, _load_spec

BACKENDS = {'grouped': ref.NumpySegmentBackend, 'block-loop': ref.NumpyBlockLoopBackend}
PAIR, SINGLE, FLAGS = pair_cases(), single_cases(), flags_cases()


@pytest.fixture(params=list(BACKENDS))
def nb(request):
    return BACKENDS[request.param]()


def _equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind in 'fc')


def _mults(leg):
    return [int(m) for m in leg.mults]


def _ops_for(kinds):
    if kinds == ('bool', 'bool'):
        return list(ref.ARITH) + list(ref.COMPARE) + list(ref.LOGICAL)
    if 'complex' in kinds:
        return list(ref.ARITH) + ['eq', 'ne']
    return list(ref.ARITH) + list(ref.COMPARE)


def _check_diagonal(got, leg, want_inds, want_blocks, want_dtype):
    assert got.leg is leg or ab._same_space(got.leg, leg)
    assert got.block_inds.dtype == np.int64 and got.block_inds.tolist() == list(want_inds)
    assert np.all(np.diff(got.block_inds) > 0)                                   # the block table is sorted
    assert got.dtype == np.dtype(want_dtype)
    assert len(got.blocks) == len(want_blocks)
    for g, w, i in zip(got.blocks, want_blocks, want_inds):
        assert g.shape == (int(leg.mults[i]),) and _equal(g, w)
        assert np.dtype(g.dtype) == got.dtype


@pytest.mark.parametrize('case', range(len(PAIR)), ids=[c['id'] for c in PAIR])
def test_diagonal_binary(nb, case):
    c = PAIR[case]
    leg, (ka, kb) = c['leg'], c['kinds']
    a, b = to_diag(nb, leg, c['a'], ka), to_diag(nb, leg, c['b'], kb)
    for op in _ops_for(c['kinds']):
        for pzz in (True, False):
            got = ab.diagonal_binary(nb, a, b, op, pzz)
            inds, blocks, _ = ref.ref_diagonal_binary(_mults(leg), c['a'], c['b'], op, pzz, DTYPES[ka], DTYPES[kb])
            # one dtype for the whole result: that of func(ones(dtype_a), ones(dtype_b)), which for a result without blocks
            # is the reference's sample rule (:1622-1626)
            want_dtype = ref.block_binary(np.ones(1, DTYPES[ka]), np.ones(1, DTYPES[kb]), op).dtype
            _check_diagonal(got, leg, inds, blocks, want_dtype)


def test_diagonal_binary_is_one_grouped_call_without_zero_blocks():
    nb = ref.NumpySegmentBackend()
    c = [c for c in PAIR if c['id'] == 'u1u1-even-odd-real-real'][0]
    a, b = to_diag(nb, c['leg'], c['a'], 'real'), to_diag(nb, c['leg'], c['b'], 'real')
    made = []
    nb.zeros_many = lambda *args, **kw: made.append(args) or []
    got = ab.diagonal_binary(nb, a, b, 'add', False)
    assert nb.calls == [('seg_binary_many', c['leg'].nsec)] and made == [] and len(got.blocks) == c['leg'].nsec
    nb.calls.clear()
    assert ab.diagonal_binary(nb, a, b, 'mul', True).blocks == [] and nb.calls == []      # no common sector: nothing is launched


def test_diagonal_binary_errors(nb):
    L = legs()
    a = to_diag(nb, L['u1'], ([0], [np.ones(1)]), 'real')
    b = to_diag(nb, L['z2'], ([0], [np.ones(3)]), 'real')
    with pytest.raises(ValueError, match='same leg'):
        ab.diagonal_binary(nb, a, b, 'add', True)
    with pytest.raises(ValueError, match='unknown function'):
        ab.diagonal_binary(nb, a, a, 'hypot', True)
    with pytest.raises(ValueError, match='unknown comparison'):
        ab.diagonal_compare(nb, a, 'add', 0.0)
    with pytest.raises(TypeError, match='not ordered'):
        ab.diagonal_compare(nb, a, 'lt', 1j)


@pytest.mark.parametrize('case', range(len(SINGLE)), ids=[c['id'] for c in SINGLE])
def test_compare_reduce_and_element_access(nb, case):
    c = SINGLE[case]
    leg, kind, (inds, blocks) = c['leg'], c['kind'], c['d']
    d = to_diag(nb, leg, c['d'], kind)
    dense = ref.dense_of(_mults(leg), c['d'], DTYPES[kind])
    assert _equal(ab.diagonal_to_block(nb, d), dense) and ab.diagonal_to_block(nb, d).dtype == DTYPES[kind]
    assert _equal(d.to_numpy(nb) if blocks else dense, dense)
    # comparisons with a number: a sector without a block compares as zeros
    if kind != 'bool':
        for op in (['eq', 'ne'] if kind == 'complex' else list(ref.COMPARE)):
            for scalar in (0.0, 0.3, -0.2):
                got = ab.diagonal_compare(nb, d, op, scalar)
                assert got.dtype == np.bool_ and np.all(np.diff(got.block_inds) > 0)
                assert _equal(ref.dense_of(_mults(leg), (got.block_inds.tolist(), got.blocks), bool), ref.COMPARE[op](dense, scalar))
                zero_holds = bool(ref.COMPARE[op](0.0, scalar))
                assert got.block_inds.tolist() == (list(range(leg.nsec)) if zero_holds else list(inds))
    # reductions over ALL sectors, the numbers combined in ascending sector order
    if kind == 'bool':
        assert ab.diagonal_all(nb, d) == ref.ref_all(_mults(leg), c['d']) == bool(dense.all() and len(inds) == leg.nsec)
        assert ab.diagonal_any(nb, d) == ref.ref_any(c['d']) == bool(dense.any())
    else:
        want = ref.ref_reduce(_mults(leg), c['d'], np.sum, lambda xs: sum(xs[1:], xs[0]), DTYPES[kind])
        assert ab.reduce_diagonal(nb, d, 'sum') == want
        assert ab.reduce_diagonal(nb, d, 'sum', lambda xs: sum(xs[1:], xs[0])) == want
        assert ab.diagonal_trace_full(nb, d) == ref.ref_trace(c['d'], DTYPES[kind])
        if kind == 'real':
            assert ab.reduce_diagonal(nb, d, 'max') == ref.ref_reduce(_mults(leg), c['d'], np.max, max) == dense.max()
            assert ab.reduce_diagonal(nb, d, 'min', min) == ref.ref_reduce(_mults(leg), c['d'], np.min, min) == dense.min()
        else:
            with pytest.raises(TypeError, match='not ordered'):
                ab.reduce_diagonal(nb, d, 'max')
    for idx in (0, leg.dim - 1, leg.dim // 2, -1, int(leg.slices[1])):
        assert ab.get_element_diagonal(nb, d, idx) == dense[idx]
    with pytest.raises(IndexError):
        ab.get_element_diagonal(nb, d, leg.dim)
    t = ab.diagonal_transpose(nb, d)
    assert t.leg.sign == -leg.sign and t.block_inds.tolist() == list(inds) and all(x is y for x, y in zip(t.blocks, d.blocks))


@pytest.mark.parametrize('case', [i for i, c in enumerate(SINGLE) if c['kind'] != 'bool'], ids=[c['id'] for c in SINGLE if c['kind'] != 'bool'])
def test_full_tensor_round_trip(nb, case):
    c = SINGLE[case]
    leg, kind = c['leg'], c['kind']
    d = to_diag(nb, leg, c['d'], kind)
    full = ab.full_from_diagonal(nb, d)
    assert full.nlegs == 2 and full.num_codomain == 1 and full.block_inds.tolist() == [[i, i] for i in c['d'][0]]
    full.check_charges()
    for blk, vec in zip(full.blocks, c['d'][1]):
        assert _equal(blk, np.diag(vec))
    for tol in (None, 0.0):
        back = ab.diagonal_from_full_tensor(nb, full, tol)            # (an AbelianTensor without blocks carries no dtype: float64)
        _check_diagonal(back, leg, c['d'][0], c['d'][1], DTYPES[kind] if c['d'][0] else np.float64)
    big = [i for i, blk in enumerate(full.blocks) if blk.shape[0] > 1]
    if big:
        full.blocks[big[-1]][0, 1] = 1e-3
        assert ab.diagonal_from_full_tensor(nb, full, None).block_inds.tolist() == list(c['d'][0])
        assert ab.diagonal_from_full_tensor(nb, full, 1e-2).block_inds.tolist() == list(c['d'][0])
        with pytest.raises(ValueError, match='Not a diagonal block'):
            ab.diagonal_from_full_tensor(nb, full, 1e-4)


def test_from_full_tensor_rejects_other_tensors(nb):
    L = legs()['u1']
    t = ab.AbelianTensor(L.symmetry, [L, L.dual(), L], [], np.zeros((0, 3), np.int64), 1)
    with pytest.raises(ValueError, match='two legs'):
        ab.diagonal_from_full_tensor(nb, t)
    off = ab.AbelianTensor(L.symmetry, [L, L], [nb.as_block(np.zeros((1, 4)))], np.array([[0, 1]]), 1)
    with pytest.raises(ValueError, match='off the diagonal'):
        ab.diagonal_from_full_tensor(nb, off)
    with pytest.raises(TypeError, match='boolean'):
        ab.full_from_diagonal(nb, to_diag(nb, L, ([0], [np.ones(1, bool)]), 'bool'))


# ------------------------------------------------------------------------------------------- masks

def _bool_diag(nb, leg, flags, drop_empty=False):
    """the boolean DiagonalTensor of a flag vector: a block per sector (or, `drop_empty`, per sector with a true flag)"""
    inds = [i for i in range(leg.nsec) if not drop_empty or flags[int(leg.slices[i]):int(leg.slices[i + 1])].any()]
    return (inds, [flags[int(leg.slices[i]):int(leg.slices[i + 1])].copy() for i in inds])


def _check_mask(nb, m, leg, flags, is_projection=True):
    """`m` against ``Mask.from_flags``: the same small leg, block table, flag blocks, and position tables"""
    want = ab.Mask.from_flags(leg, flags)
    assert m.is_projection == is_projection
    assert np.array_equal(m.small_leg.sectors, want.small_leg.sectors) and np.array_equal(m.small_leg.mults, want.small_leg.mults)
    assert m.small_leg.sign == leg.sign and m.large_leg is leg
    bi = m.block_inds if is_projection else m.block_inds[:, ::-1]
    assert bi.dtype == np.int64 and bi.shape == want.block_inds.shape and np.array_equal(bi, want.block_inds)
    assert len(m.blocks) == len(want.blocks) == len(m.tables)
    for g, w, t in zip(m.blocks, want.blocks, m.tables):
        assert g.dtype == np.bool_ and _equal(g, w) and _equal(t, np.flatnonzero(w))


@pytest.mark.parametrize('case', range(len(FLAGS)), ids=[c['id'] for c in FLAGS])
def test_diagonal_to_mask_and_logic(nb, case):
    c = FLAGS[case]
    leg, flags = c['leg'], c['flags']
    mults = _mults(leg)
    for drop in (False, True):
        d = _bool_diag(nb, leg, flags, drop)
        m = ab.diagonal_to_mask(nb, to_diag(nb, leg, d, 'bool'))
        _check_mask(nb, m, leg, flags)
        large, blocks, small_mults = ref.ref_to_mask(mults, d)
        assert m.block_inds[:, 1].tolist() == large and m.small_leg.mults.tolist() == small_mults
        assert all(_equal(g, w) for g, w in zip(m.blocks, blocks))
    # logical_not changes which sectors have blocks
    inv = ab.mask_unary(nb, m, 'not')
    _check_mask(nb, inv, leg, ~flags)
    large, blocks, small_mults = ref.ref_mask_binary(mults, (m.block_inds[:, 1].tolist(), m.blocks), None, 'not')
    assert inv.block_inds[:, 1].tolist() == large and inv.small_leg.mults.tolist() == small_mults
    _check_mask(nb, ab.mask_unary(nb, inv), leg, flags)
    # a host mask (Mask.from_flags) is a valid operand
    _check_mask(nb, ab.mask_unary(nb, ab.Mask.from_flags(leg, flags)), leg, ~flags)
    for other in [o for o in FLAGS if o['leg'] is leg]:
        m2 = ab.diagonal_to_mask(nb, to_diag(nb, leg, _bool_diag(nb, leg, other['flags'], True), 'bool'))
        for op, fn in ref.LOGICAL.items():
            got = ab.mask_binary(nb, m, m2, op)
            _check_mask(nb, got, leg, fn(flags, other['flags']))
            large, blocks, small_mults = ref.ref_mask_binary(mults, (m.block_inds[:, 1].tolist(), m.blocks),
                                                             (m2.block_inds[:, 1].tolist(), m2.blocks), op)
            assert got.block_inds[:, 1].tolist() == large and got.small_leg.mults.tolist() == small_mults
            assert all(_equal(g, w) for g, w in zip(got.blocks, blocks))


@pytest.mark.parametrize('case', range(len(FLAGS)), ids=[c['id'] for c in FLAGS])
def test_mask_conversions_and_elements(nb, case):
    c = FLAGS[case]
    leg, flags = c['leg'], c['flags']
    m = ab.diagonal_to_mask(nb, to_diag(nb, leg, _bool_diag(nb, leg, flags), 'bool'))
    host = ab.Mask.from_flags(leg, flags)
    assert host.tables is None and host.is_projection                              # the host mask is what it was
    for mask in (m, host):
        blk = ab.mask_to_block(nb, mask)
        assert blk.dtype == np.bool_ and _equal(blk, flags)
        for dtype in (np.float64, np.complex128, np.bool_):
            d = ab.mask_to_diagonal(nb, mask, dtype)
            assert d.dtype == dtype and d.block_inds.tolist() == mask.block_inds[:, 1].tolist()
            assert all(np.dtype(b.dtype) == dtype for b in d.blocks)
            assert _equal(ref.dense_of(_mults(leg), (d.block_inds.tolist(), d.blocks), dtype), flags.astype(dtype))
        full = ab.full_from_mask(nb, mask)
        assert np.array_equal(full.block_inds, mask.block_inds) and full.num_codomain == 1
        dense = np.zeros((int(flags.sum()), leg.dim))
        dense[np.arange(int(flags.sum())), np.flatnonzero(flags)] = 1.0
        assert _equal(full.to_dense(nb), dense)
        for dag in (ab.mask_dagger(nb, mask), ab.mask_transpose(nb, mask)):
            assert not dag.is_projection and np.array_equal(dag.block_inds, mask.block_inds[:, ::-1])
            assert _equal(ab.mask_to_block(nb, dag), flags)
            assert _equal(ab.full_from_mask(nb, dag).to_dense(nb), dense.T)
            assert ab.mask_dagger(nb, dag).is_projection
        assert ab.mask_transpose(nb, mask).large_leg.sign == -leg.sign
        kept = np.flatnonzero(flags)
        rng = np.random.default_rng(case)
        for large in rng.integers(0, leg.dim, 6).tolist() + kept[:3].tolist():
            for small in ([int(np.searchsorted(kept, large))] if len(kept) else []) + [0]:
                if small >= len(kept):
                    continue
                want = bool(flags[large]) and kept[small] == large
                assert ab.get_element_mask(nb, mask, [small, large]) == want
                assert ab.get_element_mask(nb, ab.mask_dagger(nb, mask), [large, small]) == want


@pytest.mark.parametrize('case', range(len(FLAGS)), ids=[c['id'] for c in FLAGS])
def test_mask_contract_and_apply_with_device_tables(nb, case):
    """a device mask (position tables) projects and embeds exactly as the host mask of the same flags"""
    c = FLAGS[case]
    leg, flags = c['leg'], c['flags']
    rng = np.random.default_rng(100 + case)
    m = ab.diagonal_to_mask(nb, to_diag(nb, leg, _bool_diag(nb, leg, flags), 'bool'))
    host = ab.Mask.from_flags(leg, flags)
    other = ab.Leg(leg.symmetry, leg.sectors, np.arange(1, leg.nsec + 1), -leg.sign)
    inds = np.array([[i, i] for i in range(0, leg.nsec)], dtype=np.int64)
    t = ab.AbelianTensor(leg.symmetry, [other, leg], [nb.as_block(rng.standard_normal((int(other.mults[i]), int(leg.mults[i])))) for i in range(leg.nsec)],
                         inds, 1)
    got, want = ab.mask_contract(nb, t, m, 1), ab.mask_contract(nb, t, host, 1)
    assert np.array_equal(got.block_inds, want.block_inds) and all(_equal(g, w) for g, w in zip(got.blocks, want.blocks))
    back, back_want = ab.mask_contract(nb, got, m, 1, large_leg=False), ab.mask_contract(nb, want, host, 1, large_leg=False)
    assert np.array_equal(back.block_inds, back_want.block_inds) and all(_equal(g, w) for g, w in zip(back.blocks, back_want.blocks))
    assert _equal(back.to_dense(nb), t.to_dense(nb) * flags[None, :]) if len(back.blocks) else not flags.any()
    for sc in [s for s in SINGLE if s['leg'] is leg and s['kind'] != 'bool']:
        d = to_diag(nb, leg, sc['d'], sc['kind'])
        for mask in (m, host):
            got = ab.apply_mask_to_diagonal(nb, d, mask)
            w_inds, w_blocks = ref.ref_apply_mask(sc['d'], (m.block_inds[:, 1].tolist(), [np.asarray(b) for b in m.blocks]))
            _check_diagonal(got, m.small_leg, w_inds, w_blocks, DTYPES[sc['kind']])
    with pytest.raises(ValueError, match='projection'):
        ab.apply_mask_to_diagonal(nb, to_diag(nb, leg, ([], []), 'real'), ab.mask_dagger(nb, m))
    with pytest.raises(ValueError, match='large leg'):
        ab.apply_mask_to_diagonal(nb, to_diag(nb, other, ([], []), 'real'), m)


def test_mask_errors(nb):
    L = legs()
    m = ab.Mask.from_flags(L['u1'], np.ones(L['u1'].dim, bool))
    m2 = ab.Mask.from_flags(L['z2'], np.ones(L['z2'].dim, bool))
    with pytest.raises(ValueError, match='same large leg'):
        ab.mask_binary(nb, m, m2, 'and')
    with pytest.raises(ValueError, match='unknown function'):
        ab.mask_binary(nb, m, m, 'nand')
    with pytest.raises(ValueError, match='unknown function'):
        ab.mask_unary(nb, m, 'and')
    with pytest.raises(ValueError, match='projection'):
        ab.mask_binary(nb, ab.mask_dagger(nb, m), m, 'and')
    with pytest.raises(TypeError, match='boolean'):
        ab.diagonal_to_mask(nb, to_diag(nb, L['z2'], ([0], [np.ones(3)]), 'real'))
    with pytest.raises(ValueError, match='two indices'):
        ab.get_element_mask(nb, m, [0])


# ------------------------------------------------------------------------------------------- the users

def svd_tensors(bb, name='theta_u1_chi96.npz'):
    """the golden theta through the existing pieces: (mv, U, S, Vh of the full SVD as tensors / a DiagonalTensor with the new
    leg last / first, what truncated_svd returns for chi_max of the fixture)"""
    z = np.load(os.path.join(GOLD, name))
    a, b = ab.AbelianTensor.from_spec(bb, _load_spec(z, 'A')), ab.AbelianTensor.from_spec(bb, _load_spec(z, 'B'))
    theta = ab.compose(bb, a, b, 1)
    nc = a.nlegs - 1
    mv = ab.combine_legs_to_matrix(bb, theta, nc)
    U, S, Vh = ab.svd(bb, mv)
    sym = theta.symmetry
    new = ab.Leg(sym, mv.charges, [s.shape[0] for s in S], +1)
    rows, cols = ab.Leg(sym, mv.charges, [u.shape[0] for u in U], +1), ab.Leg(sym, mv.charges, [v.shape[1] for v in Vh], -1)
    where = {tuple(q): k for k, q in enumerate(new.sectors.tolist())}
    pos = [where[tuple(q)] for q in sym.reduce(np.asarray(mv.charges)).reshape(len(S), sym.n).tolist()]
    inds = np.array([[p, p] for p in pos], dtype=np.int64)
    order = np.argsort(pos)
    Ut = ab.AbelianTensor(sym, [rows, new.dual()], list(U), inds, 1).sorted()
    Vt = ab.AbelianTensor(sym, [new, cols], list(Vh), inds, 1).sorted()
    St = ab.DiagonalTensor(sym, new, [S[k] for k in order], np.array(pos)[order])
    return theta, nc, int(z['chi_max']), Ut, St, Vt, [pos[k] for k in range(len(S))]


def check_svd_apply_mask(bb, to_np):
    """svd_apply_mask with the mask ``S >= smallest kept value`` reproduces truncated_svd's factors bit for bit"""
    theta, nc, chi_max, U, S, Vh, pos = svd_tensors(bb)
    _, Ut, St, Vt, err, new_norm = ab.truncated_svd(bb, theta, nc, chi_max=chi_max)
    cutoff = min(float(to_np(s).min()) for s in St if s.shape[0])
    mask = ab.diagonal_to_mask(bb, ab.diagonal_compare(bb, S, 'ge', cutoff))
    assert int(mask.small_leg.mults.sum()) == sum(s.shape[0] for s in St) == chi_max
    U2, S2, V2 = ab.svd_apply_mask(bb, U, S, Vh, mask)
    kept = [k for k in range(len(St)) if St[k].shape[0]]
    assert sorted(pos[k] for k in kept) == mask.block_inds[:, 1].tolist()
    small_of = {int(l): int(s) for s, l in mask.block_inds}
    assert len(U2.blocks) == len(S2.blocks) == len(V2.blocks) == len(kept)
    for k in kept:
        j = small_of[pos[k]]
        iu = [r for r, row in enumerate(U2.block_inds) if row[1] == j][0]
        iv = [r for r, row in enumerate(V2.block_inds) if row[0] == j][0]
        i_s = S2.block_inds.tolist().index(j)
        assert np.array_equal(to_np(U2.blocks[iu]), to_np(Ut[k]))
        assert np.array_equal(to_np(S2.blocks[i_s]), to_np(St[k]))
        assert np.array_equal(to_np(V2.blocks[iv]), to_np(Vt[k]))
    assert ab._same_space(U2.legs[1], mask.small_leg) and ab._same_space(V2.legs[0], mask.small_leg) and S2.leg is mask.small_leg
    return S, S2


def test_svd_apply_mask_reproduces_truncated_svd(nb):
    check_svd_apply_mask(nb, np.asarray)


def test_svd_apply_mask_errors(nb):
    _, _, _, U, S, Vh, _ = svd_tensors(nb)
    mask = ab.diagonal_to_mask(nb, ab.diagonal_compare(nb, S, 'ge', 0.0))
    with pytest.raises(ValueError, match='projection'):
        ab.svd_apply_mask(nb, U, S, Vh, ab.mask_dagger(nb, mask))
    with pytest.raises(ValueError, match='not the leg of the mask'):
        ab.svd_apply_mask(nb, U, S, Vh, ab.Mask.from_flags(legs()['z2'], np.ones(8, bool)))


@pytest.mark.parametrize('n', [1, 2, 0.5, 3.5, np.inf])
def test_entropy_against_the_sequence_of_floats_branch(nb, n):
    _, _, _, _, S, _, _ = svd_tensors(nb)
    s = S.to_numpy(nb)
    p = ab.diagonal_binary(nb, S, S, 'mul', True)
    norm2 = ab.diagonal_trace_full(nb, p)
    p = ab.DiagonalTensor(p.symmetry, p.leg, nb.mul_many(1.0 / norm2, p.blocks), p.block_inds)
    want = ref.ref_entropy(s ** 2 / np.sum(s ** 2), n)
    got = ab.entropy(nb, p, n)
    assert abs(got - want) <= 1e-12 * abs(want)
    # missing sectors hold zero probabilities: nothing changes
    some = ab.DiagonalTensor(p.symmetry, p.leg, p.blocks[::2], p.block_inds[::2])
    dense = some.to_numpy(nb)
    assert abs(ab.entropy(nb, some, n) - ref.ref_entropy(dense, n)) <= 1e-12 * abs(ref.ref_entropy(dense, n))


def test_entropy_rejects_other_dtypes(nb):
    L = legs()['z2']
    with pytest.raises(TypeError, match='real'):
        ab.entropy(nb, to_diag(nb, L, ([0], [np.ones(3) + 0j]), 'complex'))
