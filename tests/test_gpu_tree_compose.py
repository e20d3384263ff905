"""Device side of the fusion-tree partial_compose: the cases of tests/test_tree_compose.py through HipBlockBackend (same
inputs, same criteria), and the weighted contraction kernel (csrc/tree_compose.hip) at the C-ABI between guard bands against
an element-by-element numpy model.

Exact data: integers in [-15, 15] under coefficients from {1, -2, 0.5, i, -0.5i, 1+i}, K <= 70, at most three terms -- every
product and partial sum is an integer or half-integer below 2^17 in magnitude, so it is representable and the comparison is
``==`` whatever the summation order or FMA contraction.  Rounded data: ``standard_normal`` against ``np.longdouble`` with the
componentwise bound |err| <= (2 P + 6) 2^-53 S of tests/tree_compose_cases.py, P = sum_t K_t the number of products of an
element of the tile, S = sum_t |c|_1 sum_k |A|_1 |B|_1."""
import ctypes as C

import numpy as np
import pytest

import tree_compose_cases as cases
from cyten_amd import _lib
from cyten_amd import fusion_tree as ft
from test_gpu_tree_trace import COEFFS, SENTINEL, Arena, _upload

pytestmark = pytest.mark.gpu

CONFIG_IDS = ['-'.join(map(str, c)) for c in cases.ABELIAN_CONFIGS]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the host tests on the device

@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=CONFIG_IDS)
def test_device_partial_compose_of_abelian_trees_is_the_dense_contraction(bb, rng, config, kind):
    cases.check_abelian(bb, rng, config, kind)


@pytest.mark.parametrize('cplx_a,cplx_b', [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize('side', cases.SIDES)
def test_device_random_tables_with_complex_amplitudes_match_the_restatement(bb, rng, side, cplx_a, cplx_b):
    cases.check_table(bb, rng, side, cplx_a, cplx_b)


@pytest.mark.parametrize('side', cases.SIDES)
def test_device_real_data_under_real_amplitudes_stays_float64(bb, rng, side):
    cases.check_table(bb, rng, side, False, False, cplx_amps=False)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('side', cases.SIDES)
def test_device_su2_one_leg_operator_at_the_last_leg_equals_compose_with_the_outer_of_the_identity(bb, rng, side, cplx):
    cases.check_su2_last_leg(bb, rng, side, cplx)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('side', cases.SIDES)
def test_device_su2_identity_on_two_spins_at_leg_one_gives_a_again_by_F_unitarity(bb, rng, side, cplx):
    cases.check_su2_identity(bb, rng, side, cplx)


def test_device_conjugate_sits_on_the_new_amplitude_in_the_domain_and_on_the_old_one_in_the_codomain(bb):
    cases.check_conjugate_placement(bb)


@pytest.mark.parametrize('side', cases.SIDES)
def test_device_discard_false_keeps_the_zero_blocks(bb, rng, side):
    cases.check_discard_false_keeps_zero_blocks(bb, rng, side)


@pytest.mark.parametrize('side', cases.SIDES)
def test_device_an_empty_operand_gives_empty_data(bb, rng, side):
    cases.check_empty_operand(bb, rng, side)


@pytest.mark.parametrize('side', cases.SIDES)
def test_device_chain_operator_step_equals_the_direct_call(bb, rng, side):
    cases.check_chain_step(bb, rng, side)


def test_device_partial_compose_is_one_launch(bb, rng, monkeypatch):
    """one C-ABI call for the tensor, counted through a proxy of the library"""
    c = cases.table_case(rng, 'domain', True, False)
    a, b = cases.to_dev(bb, c['a']), cases.to_dev(bb, c['b'])
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith('cyb_') or name in ('cyb_last_error', 'cyb_ctx_set_stream'):
                return fn

            def wrapped(*args):
                calls.append(name)
                return fn(*args)
            return wrapped

    monkeypatch.setattr(bb, 'lib', Counting(bb.lib))
    ft.partial_compose(bb, a, c['a_cod'], c['a_dom'], b, c['b_cod'], c['b_dom'], c['n_cod'], c['n_dom'], c['insert'], discard=False)
    assert calls == ['cyb_compose_weighted_c128']


def test_backend_refuses_bad_views_and_writes_a_strided_destination_in_place(bb, rng):
    blk = lambda *sh, c=False: bb.as_block(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if c else 0))   # noqa: E731
    a, b = blk(4, 12), blk(3, 5)                      # domain: R = 4, m0 = 2, K = 3, m2 = 2, N = 5
    many = bb.tree_compose_many
    with pytest.raises(ValueError, match='2-D'):
        many([(blk(4, 20), 'domain', 2, 2, [(blk(4, 12, 1), b, 1.0)])])
    with pytest.raises(ValueError, match='2-D'):
        many([(blk(80), 'domain', 2, 2, [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='does not factor'):
        many([(blk(4, 21), 'domain', 2, 2, [])])
    with pytest.raises(ValueError, match='shape'):
        many([(blk(4, 24), 'domain', 2, 2, [(a, b, 1.0)])])               # N = 6 of the destination, 5 of b
    with pytest.raises(ValueError, match='shape'):
        many([(blk(5, 20), 'domain', 2, 2, [(a, b, 1.0)])])               # another number of rows
    with pytest.raises(ValueError, match='shape'):
        many([(blk(4, 20), 'codomain', 2, 2, [(a, b, 1.0)])])             # the domain shapes under the other side
    with pytest.raises(ValueError, match='share one dtype'):
        many([(blk(4, 20), 'domain', 2, 2, [(a, b, 1.0)]), (blk(4, 20, c=True), 'domain', 2, 2, [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(blk(4, 20), 'domain', 2, 2, [(a, blk(3, 5, c=True), 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(blk(4, 20), 'domain', 2, 2, [(a, b, 1j)])])
    with pytest.raises(ValueError, match='column stride'):
        many([(bb.permute_axes(blk(20, 4), [1, 0]), 'domain', 2, 2, [(a, b, 1.0)])])
    with pytest.raises(ValueError, match="'domain' or 'codomain'"):
        many([(blk(4, 20), 'both', 2, 2, [(a, b, 1.0)])])
    # a float64 source under a complex destination is read as it stands; a strided destination view is written in place; a
    # transposed source view is read through its strides -- in the domain and in the codomain layout
    A = rng.integers(-15, 16, (3, 8)).astype(float)                                    # R = 3, m0 = 2, K = 2, m2 = 2
    B = rng.integers(-15, 16, (2, 3)) + 1j * rng.integers(-15, 16, (2, 3))             # K = 2, N = 3
    res = np.einsum('rikj,kn->rinj', A.reshape(3, 2, 2, 2), B).reshape(3, 12)
    big = bb.as_block(np.full((7, 17), SENTINEL + 0j))
    many([(bb.get_item(big, (slice(1, 4), slice(2, 14))), 'domain', 2, 2,
           [(bb.permute_axes(bb.as_block(np.ascontiguousarray(A.T)), [1, 0]), bb.as_block(B), 1 + 1j)])])
    want = np.full((7, 17), SENTINEL + 0j)
    want[1:4, 2:14] = (1 + 1j) * res
    assert np.array_equal(bb.to_numpy(big), want)
    big = bb.as_block(np.full((15, 6), SENTINEL + 0j))
    many([(bb.get_item(big, (slice(2, 14), slice(1, 4))), 'codomain', 2, 2,
           [(bb.as_block(np.ascontiguousarray(A.T)), bb.permute_axes(bb.as_block(B), [1, 0]), -0.5j)])])
    want = np.full((15, 6), SENTINEL + 0j)
    want[2:14, 1:4] = -0.5j * res.T
    assert np.array_equal(bb.to_numpy(big), want)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

def out_spec(side, other, m0, N, m2, terms, ld=None, at=(1, 1)):
    """one output in the layout of `side`: 'domain' -- levels (r, i0, n, i2), axis 2, a tile of `other` rows and m0 N m2 columns;
    'codomain' -- levels (i0, n, i2, col), axis 1, a tile of m0 N m2 rows and `other` columns.  The tile sits at row / column
    `at` of a block with the leading dimension `ld` (default: two spare columns at least, odd)"""
    return dict(side=side, other=other, m0=m0, N=N, m2=m2, terms=terms, ld=ld, at=at)


def term_spec(K, coeff=1.0, a_real=False, b_real=False, a_t=False, b_t=False, a_pad=0, b_pad=0, off=1):
    """one term with the contracted extent K; `*_real`: a float64 operand under the c128 entry; `*_t`: the operand is a
    transposed view (row stride 1); `*_pad`: spare elements behind every row of its storage; the views start `off` elements
    into their NaN parents"""
    return dict(K=K, coeff=coeff, real=(a_real, b_real), t=(a_t, b_t), pad=(a_pad, b_pad), off=off)


def _view(shape, transposed, pad):
    """(row stride, column stride, number of elements the storage spans) of a `shape` view"""
    h, w = shape
    if transposed:
        return 1, h + pad, w * (h + pad)
    return w + pad, 1, h * (w + pad)


def _shapes(o, K):
    """(tile shape, shape of A, shape of B)"""
    dom, mine = o['side'] == 'domain', o['m0'] * o['N'] * o['m2']
    if dom:
        return (o['other'], mine), (o['other'], o['m0'] * K * o['m2']), (K, o['N'])
    return (mine, o['other']), (o['m0'] * K * o['m2'], o['other']), (o['N'], K)


def _contract(o, A, B, K):
    """the tile of one term, by numpy: A and B as 2-D arrays"""
    m0, N, m2, other = o['m0'], o['N'], o['m2'], o['other']
    if o['side'] == 'domain':
        return np.tensordot(A.reshape(other, m0, K, m2), B, ([2], [0])).transpose(0, 1, 3, 2).reshape(other, m0 * N * m2)
    return np.tensordot(A.reshape(m0, K, m2, other), B, ([1], [1])).transpose(0, 3, 1, 2).reshape(m0 * N * m2, other)


def run_cabi(bb, rng, outputs, cplx, exact, expect=_lib.CYB_OK, mutate=None):
    """lay the records out (destination tiles inside blocks between SENTINEL bands, source views inside NaN parents), launch
    ONCE and compare: every byte outside the tiles bit for bit with the image before the call, the tiles with the model
    (``==`` for exact data, the bound of the module docstring for rounded data), the sources with themselves.  Then launch
    again: the same bits.  `mutate(oarr, tarr)` may spoil the records; with `expect` an error nothing may have changed."""
    dst_a, src_c, src_r = Arena(cplx, SENTINEL), Arena(True, complex(np.nan, np.nan)), Arena(False, np.nan)
    oarr = np.zeros(max(len(outputs), 1), dtype=_lib.COMPOSE_WEIGHTED_OUT_DTYPE)
    n_terms = sum(len(o['terms']) for o in outputs)
    tarr = np.zeros(max(n_terms, 1), dtype=_lib.COMPOSE_WEIGHTED_TERM_DTYPE)
    lay, t = [], 0
    for k, o in enumerate(outputs):
        dom, m0, N, m2, other = o['side'] == 'domain', o['m0'], o['N'], o['m2'], o['other']
        (H, W), _, _ = _shapes(o, 0)
        r0, c0 = o['at']
        ld = o['ld'] if o['ld'] is not None else W + c0 + 2 + (W + c0 + 1) % 2
        off = dst_a.block((H + r0 + 1) * ld)
        oarr[k]['ext'] = (other, m0, N, m2) if dom else (m0, N, m2, other)
        oarr[k]['sd'] = (ld, N * m2, m2, 1) if dom else (N * m2 * ld, m2 * ld, ld, 1)
        oarr[k]['axis'] = 2 if dom else 1
        oarr[k]['first_term'], oarr[k]['n_terms'] = t, len(o['terms'])
        tl = []
        for tm in o['terms']:
            K = tm['K']
            _, sha, shb = _shapes(o, K)
            ops = []
            for which, shape in enumerate((sha, shb)):
                rs, cs, span = _view(shape, tm['t'][which], tm['pad'][which])
                arena = src_c if cplx and not tm['real'][which] else src_r
                soff = arena.block(span + tm['off']) + tm['off']
                ops.append((arena, soff, span, rs, cs, shape))
            tarr[t]['coeff_re'], tarr[t]['coeff_im'] = complex(tm['coeff']).real, complex(tm['coeff']).imag
            tarr[t]['a_real'], tarr[t]['b_real'] = int(cplx and tm['real'][0]), int(cplx and tm['real'][1])
            ars, acs, brs, bcs = ops[0][3], ops[0][4], ops[1][3], ops[1][4]
            tarr[t]['K'] = K
            tarr[t]['sa'] = (ars, K * m2 * acs, m2 * acs, acs) if dom else (K * m2 * ars, m2 * ars, ars, acs)
            tarr[t]['b_ns'], tarr[t]['b_ks'] = (bcs, brs) if dom else (brs, bcs)
            tl.append(ops)
            t += 1
        lay.append((off + r0 * ld + c0, ld, tl))
    dst, simg_c, simg_r = dst_a.host(), src_c.host(), src_r.host()
    for _, _, tl in lay:
        for ops in tl:
            for arena, soff, span, _, _, _ in ops:
                img = simg_c if arena is src_c else simg_r
                if exact:
                    v = rng.integers(-15, 16, span).astype(float) + (1j * rng.integers(-15, 16, span) if arena is src_c else 0)
                else:
                    v = rng.standard_normal(span) + (1j * rng.standard_normal(span) if arena is src_c else 0)
                img[soff:soff + span] = v
    d_dst, d_c, d_r = _upload(bb, dst), _upload(bb, simg_c), _upload(bb, simg_r)
    es = 16 if cplx else 8
    t = 0
    for k, (doff, _, tl) in enumerate(lay):
        oarr[k]['dst'] = d_dst.data_ptr() + es * doff
        for ops in tl:
            for name, (arena, soff, _, _, _, _) in zip('ab', ops):
                tarr[t][name] = (d_c.data_ptr() + 16 * soff) if arena is src_c else (d_r.data_ptr() + 8 * soff)
            t += 1
    # the model, one output at a time
    want, bound, tiles = dst.copy(), np.zeros(len(dst)), np.zeros(len(dst), dtype=bool)
    wide = np.clongdouble if cplx else np.longdouble
    for o, (doff, ld, tl) in zip(outputs, lay):
        (H, W), _, _ = _shapes(o, 0)
        if H * W == 0:
            continue
        at = (doff + ld * np.arange(H)[:, None] + np.arange(W)[None, :]).ravel()
        acc, S = np.zeros((H, W), dtype=np.complex128 if exact else wide), np.zeros((H, W))
        for tm, ops in zip(o['terms'], tl):
            vals = []
            for arena, soff, _, rs, cs, (h, w) in ops:
                idx = soff + rs * np.arange(h)[:, None] + cs * np.arange(w)[None, :]
                vals.append((simg_c if arena is src_c else simg_r)[idx])
            c = complex(tm['coeff'])
            if exact:
                acc = acc + c * _contract(o, vals[0], vals[1], tm['K'])
            else:
                acc = acc + wide(c if cplx else c.real) * _contract(o, vals[0].astype(wide), vals[1].astype(wide), tm['K'])
            S += cases.abs1(c) * _contract(o, cases.abs1(vals[0]), cases.abs1(vals[1]), tm['K'])
        assert not np.isnan(np.asarray(acc, dtype=np.complex128)).any()                # the model never left a view
        want[at] = (np.asarray(acc, dtype=np.complex128) if cplx else np.asarray(acc.real, dtype=np.float64)).ravel()
        bound[at] = ((2 * sum(tm['K'] for tm in o['terms']) + 6) * 2.0 ** -53 * S).ravel()
        tiles[at] = True
    if mutate is not None:
        mutate(oarr, tarr)
    fn = bb.lib.cyb_compose_weighted_c128 if cplx else bb.lib.cyb_compose_weighted_f64
    args = (bb.ctx.handle, oarr.ctypes.data_as(C.POINTER(_lib.ComposeWeightedOut)), len(outputs),
            tarr.ctypes.data_as(C.POINTER(_lib.ComposeWeightedTerm)), n_terms)
    bb.ctx.sync_stream()
    status = fn(*args)
    assert status == expect, bb.lib.cyb_last_error().decode()
    got = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    if expect != _lib.CYB_OK:
        assert np.array_equal(got.view(np.uint64), dst.view(np.uint64))                # destination and sentinels untouched
        return
    outside = ~tiles
    assert np.array_equal(got[outside].view(np.uint64), dst[outside].view(np.uint64)), 'a guard band or a gap between tile rows was written'
    if exact:
        bad = got[tiles] != want[tiles]
        assert not bad.any(), f'{int(bad.sum())} of {int(tiles.sum())} elements differ'
    else:
        err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
        ok = (err_re[tiles] <= bound[tiles]) & (err_im[tiles] <= bound[tiles])
        assert ok.all(), f'{int((~ok).sum())} elements outside the bound, worst ratio {np.max(np.maximum(err_re, err_im)[tiles] / np.maximum(bound[tiles], 1e-300)):.3g}'
    for d_s, img in ((d_c, simg_c), (d_r, simg_r)):
        back = bb.ctx.d2h(d_s, len(img), img.dtype)
        assert np.array_equal(back.view(np.uint64), img.view(np.uint64))
    _lib.check(fn(*args))
    again = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))                  # bit-identical from run to run


def _coeff(k, cplx):
    return COEFFS[k % len(COEFFS)] if cplx else COEFFS[k % 3]


def _branch_outputs(cplx):
    """the smallest shapes that reach each branch of the kernel as built.  float64: with p the last level whose extent is above
    1, a record runs on pairs of doubles (x_p, x_p + 1) iff sd[p] == 1, ext[p] is even, sd[l] is even for every l < p with
    ext[l] > 1 and dst is 16-byte aligned (blocks of the arena start at even offsets: the base is aligned iff r0 * ld + c0 is
    even); with p == axis the pair shares A and differs in B, else it shares B and differs in A.  Else one double per lane;
    complex: one element per lane.  Every entry: with p != axis n runs in the registers of a lane, four values at a time (N = 5,
    6, 9: a full block and a rest), the flat order is that of the other three levels; with p == axis (m2 = 1 in the domain
    layout, one column in the codomain layout) n runs in the lanes.  Lane offsets are decoded with extents clipped at 64 (the wave); the step of 64 units wraps
    every level of a small tile.  A work item is 1024 units (pairs / elements) while the call has fewer than 8192 * 1024 of
    them; one wave per item, four per workgroup.  The k loop runs K times per term, not at all for K = 0."""
    c = lambda k: _coeff(k, cplx)                                                      # noqa: E731
    T, D, Cd = term_spec, 'domain', 'codomain'
    return [
        out_spec(D, 1, 1, 1, 1, [T(1, c(0))]),                                                         # all extents 1, K = 1: no p, one double
        out_spec(Cd, 1, 1, 1, 1, [T(1, c(1))]),                                                        # ... under axis = 1
        out_spec(D, 3, 2, 3, 2, [T(0, c(2))], ld=14, at=(1, 2)),                                       # K = 0 alone: zeros (in pairs)
        out_spec(D, 3, 2, 3, 3, [T(0, c(2)), T(3, c(3)), T(0, c(4))]),                                 # K = 0 beside K = 3
        out_spec(D, 3, 2, 1, 3, [T(3, c(4))]),                                                         # N = 1, domain
        out_spec(Cd, 3, 2, 1, 3, [T(3, c(5))]),                                                        # N = 1, codomain
        out_spec(D, 3, 2, 2, 5, [T(2, c(0))]),                                                         # p = 3, odd m2: no pairs
        out_spec(D, 3, 2, 2, 6, [T(2, c(1))], ld=28, at=(1, 2)),                                       # p = 3: even m2, ld, base: pairs share B
        out_spec(D, 3, 2, 2, 6, [T(2, c(2))], ld=28, at=(1, 3)),                                       # ... odd column offset: no pairs
        out_spec(D, 3, 2, 2, 6, [T(2, c(3))], ld=27, at=(2, 2)),                                       # ... odd ld, several rows: no pairs
        out_spec(D, 1, 2, 2, 6, [T(2, c(4))], ld=27, at=(2, 2)),                                       # ... odd ld, one row: pairs
        out_spec(D, 3, 2, 5, 4, [T(2, c(2)), T(3, c(3))], ld=42, at=(1, 2)),                           # n in registers, N = 5 = 4 + 1, in pairs
        out_spec(D, 3, 2, 6, 3, [T(2, c(3))]),                                                         # ... N = 6 = 4 + 2, single doubles
        out_spec(Cd, 6, 2, 9, 2, [T(2, c(4)), T(1, c(5), b_t=True)], ld=8, at=(1, 2)),                 # ... N = 9 = 4 + 4 + 1, codomain layout
        out_spec(D, 4, 3, 6, 1, [T(3, c(5))], ld=20, at=(1, 2)),                                       # m2 = 1: p = 2 = axis, n in the lanes, pairs along n share A
        out_spec(D, 4, 3, 5, 1, [T(3, c(0))], ld=20, at=(1, 2)),                                       # ... odd N: no pairs
        out_spec(D, 4, 1, 6, 1, [T(3, c(1)), T(1, c(2), b_t=True)], ld=10, at=(1, 2)),                 # ... m0 = 1; b_ks = 1
        out_spec(D, 4, 6, 1, 1, [T(3, c(2))], ld=10, at=(1, 2)),                                       # m2 = N = 1: p = 1, pairs along i0 differ in A
        out_spec(D, 6, 1, 1, 1, [T(3, c(3))], ld=1, at=(2, 0)),                                        # a column with ld = 1: p = 0, pairs along r
        out_spec(D, 6, 1, 1, 1, [T(3, c(4))], ld=3, at=(2, 0)),                                        # ... ld = 3: sd[p] != 1, no pairs
        out_spec(Cd, 6, 2, 3, 2, [T(2, c(5))], ld=8, at=(1, 2)),                                       # codomain, p = 3: even C, ld, base: pairs
        out_spec(Cd, 6, 2, 3, 2, [T(2, c(0))], ld=9, at=(2, 2)),                                       # ... odd ld: no pairs
        out_spec(Cd, 5, 2, 3, 2, [T(2, c(1))], ld=8, at=(1, 2)),                                       # ... odd C: no pairs
        out_spec(Cd, 6, 1, 1, 1, [T(2, c(2))], ld=9, at=(2, 2)),                                       # ... one row under an odd ld: pairs
        out_spec(Cd, 1, 2, 3, 4, [T(2, c(3))], ld=1, at=(2, 0)),                                       # C = 1, ld = 1: p = 2, pairs along i2
        out_spec(Cd, 1, 3, 4, 1, [T(2, c(4)), T(5, c(5), b_t=True)], ld=1, at=(2, 0)),                 # ... m2 = 1: p = 1 = axis, pairs along n; b_ns = 1
        out_spec(Cd, 1, 3, 4, 1, [T(2, c(0))], ld=2, at=(1, 0)),                                       # ... ld = 2: sd[p] != 1, no pairs
        out_spec(D, 70, 1, 1, 1000, [T(3, c(2), off=2)], ld=1002, at=(1, 2)),                          # 35000 pairs: 35 work items; extents above 64
        out_spec(D, 70, 1, 1, 1001, [T(1, c(3))]),                                                     # 70070 single doubles: 69 work items
        out_spec(D, 5, 3, 4, 2, [T(1, c(4)), T(3, c(5), a_t=True), T(70, c(0), b_t=True, a_pad=3)], ld=30, at=(1, 2)),   # 3 terms, K = 1, 3, 70
        out_spec(Cd, 5, 3, 4, 2, [T(70, c(1), b_pad=2), T(1, c(2), a_t=True), T(3, c(3), a_pad=1, b_pad=1)]),            # ... in the codomain layout
        out_spec(D, 4, 3, 5, 2, []),                                                                   # no terms: zeros are written
        out_spec(D, 4, 3, 5, 2, [], ld=32, at=(0, 2)),                                                 # ... in pairs
        out_spec(D, 0, 3, 2, 2, [T(2, c(1))]),                                                         # a zero in each of the four extents
        out_spec(D, 2, 0, 2, 2, [T(2, c(1))]),
        out_spec(D, 2, 3, 0, 2, [T(2, c(1))]),
        out_spec(D, 2, 3, 2, 0, [T(2, c(1))]),
        out_spec(Cd, 0, 3, 2, 2, [T(2, c(1))]),
        out_spec(D, 3, 2, 4, 2, [T(2, c(2), a_real=True), T(3, c(3), b_real=True), T(1, c(4), a_real=True, b_real=True, b_pad=1), T(2, c(5))],
                 ld=40, at=(1, 4)),                                                                    # real beside complex sources; spare columns
        out_spec(D, 65, 2, 3, 66, [T(2, c(0), b_pad=2), T(1, c(1), a_t=True, b_t=True)], ld=400, at=(0, 0)),   # extents 65 and 66: just above the wave
        out_spec(Cd, 66, 65, 2, 1, [T(3, c(1), a_pad=2)], ld=66, at=(0, 0)),                           # ... in the codomain layout
    ]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'rounded'])
@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_branches_between_guard_bands(bb, rng, cplx, exact):
    run_cabi(bb, rng, _branch_outputs(cplx), cplx, exact)


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_thousands_of_one_by_one_tiles_beside_a_large_one(bb, rng, cplx):
    """3001 waves of one element with 0 to 2 terms each (with the large tile: a number of items that is no multiple of the four
    of a workgroup) and a tile of 24 (pairs of doubles) or 48 (complex) work items in their midst"""
    outs = [out_spec('domain' if k % 2 else 'codomain', 1, 1, 1, 1, [term_spec(1 + k % 2, _coeff(k, cplx), off=k % 2)] * (k % 3), ld=2, at=(0, k % 2))
            for k in range(3001)]
    outs.insert(1500, out_spec('domain', 128, 8, 3, 16, [term_spec(3, _coeff(1, cplx)), term_spec(2, _coeff(3, cplx), a_t=True)], ld=384, at=(0, 0)))
    run_cabi(bb, rng, outs, cplx, True)


def test_kernel_empty_lists(bb):
    for fn in (bb.lib.cyb_compose_weighted_f64, bb.lib.cyb_compose_weighted_c128):
        assert fn(bb.ctx.handle, None, 0, None, 0) == _lib.CYB_OK


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_invalid_records_are_refused_before_anything_is_launched(bb, rng, cplx):
    """negative extents, an extent or K beyond 2^30, a negative K, axis outside {1, 2}, a bad term range, sd[3] != 1 under
    ext[3] > 1, NULL dst / a / b of a non-empty output, a complex coefficient at the float64 entry: the error comes back,
    destination and sentinels stay as they were, and the context serves the next valid call"""
    def outputs():
        return [out_spec('domain', 2, 2, 3, 2, [term_spec(2, 1.0)]), out_spec('codomain', 3, 1, 2, 4, [term_spec(3, -2.0), term_spec(1, 0.5, a_t=True)])]

    def set_(arr, k, field, value, at=None):
        if at is None:
            arr[k][field] = value
        else:
            arr[k][field][at] = value

    spoil = [
        (lambda o, t: set_(o, 1, 'ext', -1, 0), 'negative extent'),
        (lambda o, t: set_(o, 0, 'ext', -2, 3), 'negative extent'),
        (lambda o, t: set_(o, 1, 'ext', 2 ** 30 + 1, 1), 'extent too large'),
        (lambda o, t: set_(t, 1, 'K', 2 ** 30 + 1), 'contracted extent'),
        (lambda o, t: set_(t, 2, 'K', -1), 'contracted extent'),
        (lambda o, t: set_(o, 0, 'axis', 0), 'axis'),
        (lambda o, t: set_(o, 1, 'axis', 3), 'axis'),
        (lambda o, t: set_(o, 1, 'n_terms', 3), 'bad term range'),
        (lambda o, t: set_(o, 1, 'first_term', -1), 'bad term range'),
        (lambda o, t: set_(o, 0, 'sd', 2, 3), 'destination stride 1'),
        (lambda o, t: set_(o, 1, 'dst', 0), 'dst is NULL'),
        (lambda o, t: set_(t, 2, 'a', 0), 'a is NULL'),
        (lambda o, t: set_(t, 1, 'b', 0), 'b is NULL'),
    ]
    if not cplx:
        spoil.append((lambda o, t: set_(t, 0, 'coeff_im', 0.5), 'complex coefficient'))
    for mutate, frag in spoil:
        run_cabi(bb, rng, outputs(), cplx, True, expect=_lib.CYB_ERR_INVALID, mutate=mutate)
        assert frag in bb.lib.cyb_last_error().decode()
    run_cabi(bb, rng, outputs(), cplx, True)
