"""Device side of the fusion-tree outer: the cases of tests/test_tree_outer.py through HipBlockBackend (same inputs, same
criteria), and the weighted Kronecker kernel (csrc/tree_outer.hip) at the C-ABI between guard bands against an
element-by-element numpy model.

Exact data: integers in [-15, 15] under coefficients from {1, -2, 0.5, i, -0.5i, 1+i} -- every product and partial sum is
representable, so the comparison is ``==`` whatever the summation order or FMA contraction.  Rounded data:
``standard_normal`` against ``np.longdouble`` with the componentwise bound |err| <= (n + 6) 2^-53 S, n the number of terms of
the tile, S = sum_t |c|_1 |A|_1 |B|_1: two complex products per term and n - 1 additions."""
import ctypes as C

import numpy as np
import pytest

import tree_outer_cases as cases
from cyten_amd import _lib
from cyten_amd import fusion_tree as ft
from test_gpu_tree_trace import COEFFS, SENTINEL, Arena, _upload

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the host tests on the device

@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=lambda c: 'x'.join(map(str, c)))
def test_device_outer_of_abelian_trees_is_the_dense_tensor_product(bb, rng, config, kind):
    cases.check_abelian(bb, rng, config, kind)


@pytest.mark.parametrize('cplx_a,cplx_b', [(False, False), (True, True), (False, True)])
def test_device_random_tables_with_complex_amplitudes_match_the_restatement(bb, rng, cplx_a, cplx_b):
    cases.check_table(bb, rng, cplx_a, cplx_b)


def test_device_real_data_under_real_amplitudes_stays_float64(bb, rng):
    cases.check_table(bb, rng, False, False, cplx_amps=False)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_su2_interchange_law_with_tables_from_fusion_rules(bb, rng, cplx):
    cases.check_su2_interchange(bb, rng, cplx)


@pytest.mark.parametrize('m', [(1, 1, 1, 1), (2, 1, 3, 2), (3, 2, 1, 3)])
def test_device_su2_identity_times_identity_is_the_identity_by_F_unitarity(bb, m):
    cases.check_su2_identity(bb, m)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_zero_leg_operand_scales_the_other(bb, rng, cplx):
    cases.check_zero_leg(bb, rng, cplx)


def test_device_coefficient_conjugates_the_codomain_amplitude(bb):
    mk = ft.TreeSpace.from_multiplicities
    a_cod, a_dom = mk([[0]], [[(2,)]], None, 1, [['xa']]), mk([[0]], [[(3,)]], None, 1, [['ya']])
    b_cod, b_dom = mk([[0]], [[(2,)]], None, 1, [['xb']]), mk([[0]], [[(2,)]], None, 1, [['yb']])
    n_cod, n_dom = mk([[0]], [[(2, 2)]], None, 2, [['x']]), mk([[0]], [[(3, 2)]], None, 2, [['y']])
    A, B = np.arange(-3.0, 3.0).reshape(2, 3), np.array([[1.0, -2.0], [3.0, 5.0]])
    got = ft.outer(bb, ft.FusionTreeData([(0, 0)], [bb.as_block(A)]), a_cod, a_dom, ft.FusionTreeData([(0, 0)], [bb.as_block(B)]), b_cod, b_dom,
                   n_cod, n_dom, ft.TreeOuter({('xa', 'xb'): [('x', 1j)]}), ft.TreeOuter({('ya', 'yb'): [('y', 1.0)]}))
    assert np.array_equal(bb.to_numpy(got.blocks[0]), -1j * np.kron(A, B))


def test_device_outer_is_one_launch(bb, rng, monkeypatch):
    """one C-ABI call for the tensor, counted through a proxy of the library"""
    c = cases.table_case(rng, True, False)
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
    ft.outer(bb, a, c['a_cod'], c['a_dom'], b, c['b_cod'], c['b_dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt'], discard=False)
    assert calls == ['cyb_outer_weighted_c128']


def test_backend_refuses_bad_views_and_writes_a_strided_destination_in_place(bb, rng):
    blk = lambda *sh, c=False: bb.as_block(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if c else 0))   # noqa: E731
    a, b = blk(2, 3), blk(4, 5)
    with pytest.raises(ValueError, match='2-D'):
        bb.tree_outer_many([(blk(8, 15), [(blk(2, 3, 1), b, 1.0)])])
    with pytest.raises(ValueError, match='2-D'):
        bb.tree_outer_many([(blk(120), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='shape'):
        bb.tree_outer_many([(blk(8, 14), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='shape'):
        bb.tree_outer_many([(blk(15, 8), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='differ in their extents'):
        bb.tree_outer_many([(blk(8, 15), [(a, b, 1.0), (blk(4, 3), blk(2, 5), 1.0)])])
    with pytest.raises(ValueError, match='share one dtype'):
        bb.tree_outer_many([(blk(8, 15), [(a, b, 1.0)]), (blk(8, 15, c=True), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_outer_many([(blk(8, 15), [(a, blk(4, 5, c=True), 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_outer_many([(blk(8, 15), [(a, b, 1j)])])
    with pytest.raises(ValueError, match='column stride'):
        bb.tree_outer_many([(bb.permute_axes(blk(15, 8), [1, 0]), [(a, b, 1.0)])])
    # a float64 source under a complex destination is read as it stands; a strided destination view is written in place; a
    # transposed source view is read through its strides
    big = bb.as_block(np.full((7, 11), SENTINEL + 0j))
    A = rng.integers(-15, 16, (3, 2)).astype(float)
    B = rng.integers(-15, 16, (2, 2)) + 1j * rng.integers(-15, 16, (2, 2))
    bb.tree_outer_many([(bb.get_item(big, (slice(1, 5), slice(2, 8))), [(bb.permute_axes(bb.as_block(A), [1, 0]), bb.as_block(B), 1 + 1j)])])
    want = np.full((7, 11), SENTINEL + 0j)
    want[1:5, 2:8] = (1 + 1j) * np.kron(A.T, B)
    assert np.array_equal(bb.to_numpy(big), want)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

def out_spec(ha, hb, wa, wb, terms, ld=None, at=(1, 1), ldd=None):
    """one output: the tile sits at row / column `at` of a block with the leading dimension `ld` (default: two spare columns at
    least, odd); `ldd`: what the record says instead of `ld` (a tile of one row may say anything)"""
    return dict(ext=(ha, hb, wa, wb), terms=terms, ld=ld, at=at, ldd=ldd)


def term_spec(coeff=1.0, a_real=False, b_real=False, a_t=False, b_t=False, a_pad=0, b_pad=0, off=1):
    """one term; `*_real`: a float64 operand under the c128 entry; `*_t`: the operand is a transposed view (row stride 1);
    `*_pad`: spare elements behind every row of its storage; the views start `off` elements into their NaN parents"""
    return dict(coeff=coeff, real=(a_real, b_real), t=(a_t, b_t), pad=(a_pad, b_pad), off=off)


def _view(shape, transposed, pad):
    """(row stride, column stride, number of elements the storage spans) of a `shape` view"""
    h, w = shape
    if transposed:
        return 1, h + pad, w * (h + pad)
    return w + pad, 1, h * (w + pad)


def _kron(A, B):
    return np.multiply.outer(A, B).transpose(0, 2, 1, 3).reshape(A.shape[0] * B.shape[0], A.shape[1] * B.shape[1])


def run_cabi(bb, rng, outputs, cplx, exact, expect=_lib.CYB_OK, mutate=None):
    """lay the records out (destination tiles inside blocks between SENTINEL bands, source views inside NaN parents), launch
    ONCE and compare: every byte outside the tiles bit for bit with the image before the call, the tiles with the model
    (``==`` for exact data, the bound of the module docstring for rounded data), the sources with themselves.  Then launch
    again: the same bits.  `mutate(oarr, tarr)` may spoil the records; with `expect` an error nothing may have changed."""
    dst_a, src_c, src_r = Arena(cplx, SENTINEL), Arena(True, complex(np.nan, np.nan)), Arena(False, np.nan)
    oarr = np.zeros(max(len(outputs), 1), dtype=_lib.OUTER_WEIGHTED_OUT_DTYPE)
    n_terms = sum(len(o['terms']) for o in outputs)
    tarr = np.zeros(max(n_terms, 1), dtype=_lib.OUTER_WEIGHTED_TERM_DTYPE)
    lay, t = [], 0
    for k, o in enumerate(outputs):
        ha, hb, wa, wb = o['ext']
        H, W = ha * hb, wa * wb
        r0, c0 = o['at']
        ld = o['ld'] if o['ld'] is not None else W + c0 + 2 + (W + c0 + 1) % 2
        off = dst_a.block((H + r0 + 1) * ld)
        oarr[k]['ha'], oarr[k]['hb'], oarr[k]['wa'], oarr[k]['wb'] = ha, hb, wa, wb
        oarr[k]['ldd'] = ld if o['ldd'] is None else o['ldd']
        oarr[k]['first_term'], oarr[k]['n_terms'] = t, len(o['terms'])
        tl = []
        for tm in o['terms']:
            ops = []
            for which, shape in enumerate(((ha, wa), (hb, wb))):
                rs, cs, span = _view(shape, tm['t'][which], tm['pad'][which])
                arena = src_c if cplx and not tm['real'][which] else src_r
                soff = arena.block(span + tm['off']) + tm['off']
                ops.append((arena, soff, span, rs, cs, shape))
            tarr[t]['coeff_re'], tarr[t]['coeff_im'] = complex(tm['coeff']).real, complex(tm['coeff']).imag
            tarr[t]['a_real'], tarr[t]['b_real'] = int(cplx and tm['real'][0]), int(cplx and tm['real'][1])
            tarr[t]['a_rs'], tarr[t]['a_cs'], tarr[t]['b_rs'], tarr[t]['b_cs'] = ops[0][3], ops[0][4], ops[1][3], ops[1][4]
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
        ha, hb, wa, wb = o['ext']
        H, W = ha * hb, wa * wb
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
                acc = acc + c * _kron(vals[0], vals[1])
            else:
                acc = acc + wide(c if cplx else c.real) * _kron(vals[0].astype(wide), vals[1].astype(wide))
            S += cases.abs1(c) * _kron(cases.abs1(vals[0]), cases.abs1(vals[1]))
        assert not np.isnan(np.asarray(acc, dtype=np.complex128)).any()                # the model never left a view
        want[at] = (np.asarray(acc, dtype=np.complex128) if cplx else np.asarray(acc.real, dtype=np.float64)).ravel()
        bound[at] = ((len(o['terms']) + 6) * 2.0 ** -53 * S).ravel()
        tiles[at] = True
    if mutate is not None:
        mutate(oarr, tarr)
    fn = bb.lib.cyb_outer_weighted_c128 if cplx else bb.lib.cyb_outer_weighted_f64
    args = (bb.ctx.handle, oarr.ctypes.data_as(C.POINTER(_lib.OuterWeightedOut)), len(outputs),
            tarr.ctypes.data_as(C.POINTER(_lib.OuterWeightedTerm)), n_terms)
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
    """the smallest shapes that reach each branch of the kernel as built.  float64: a record runs on pairs of doubles iff wb
    is even, ldd is even (or the tile has one row) and dst is 16-byte aligned (blocks of the arena start at even offsets: the
    base is aligned iff r0 * ld + c0 is even); else one double per lane; complex: one element per lane.  Lane offsets are
    decoded with extents clipped at 64 (the wave); the step of 64 units wraps every level of a small tile.  A work item is
    1024 units (pairs / elements) while the call has fewer than 8192 * 1024 of them; one wave per item, four per workgroup."""
    c = lambda k: _coeff(k, cplx)                                                      # noqa: E731
    T = term_spec
    return [
        out_spec(1, 1, 1, 1, [T(c(0))]),                                                               # a 1 x 1 (x) 1 x 1 tile
        out_spec(1, 1, 3, 5, [T(c(1))], ldd=0),                                                        # ha hb = 1: one row, ldd is not read
        out_spec(3, 5, 1, 1, [T(c(2))]),                                                               # wa wb = 1: one column
        out_spec(3, 2, 2, 5, [T(c(3))]),                                                               # odd wb: no pairs
        out_spec(3, 2, 2, 6, [T(c(4))], ld=16, at=(1, 2)),                                             # even wb, ldd, base: pairs
        out_spec(3, 2, 2, 6, [T(c(5))], ld=16, at=(1, 3)),                                             # ... odd column offset: no pairs
        out_spec(3, 2, 2, 6, [T(c(0))], ld=15, at=(2, 2)),                                             # ... odd ldd: no pairs
        out_spec(1, 1, 2, 6, [T(c(1))], ld=15, at=(2, 2), ldd=3),                                      # ... one row under an odd ldd: pairs
        out_spec(70, 1, 1, 1000, [T(c(2), off=2)], ld=1002, at=(1, 2)),                                # 35000 pairs: 35 work items; extents above 64
        out_spec(70, 1, 1, 1001, [T(c(3))]),                                                           # 70070 single doubles: 69 work items
        out_spec(5, 13, 7, 4, [T(c(4)), T(c(5), a_t=True), T(c(0), b_t=True, a_pad=3)], ld=30, at=(1, 2)),   # 3 terms; a_rs = 1; b_rs = 1
        out_spec(4, 3, 5, 2, []),                                                                      # no terms: zeros are written
        out_spec(4, 3, 5, 2, [], ld=12, at=(0, 2)),                                                    # ... in pairs
        out_spec(0, 3, 2, 2, [T(c(1))]),                                                               # zero extents
        out_spec(2, 0, 2, 2, [T(c(1))]),
        out_spec(2, 3, 0, 2, [T(c(1))]),
        out_spec(2, 3, 2, 0, [T(c(1))]),
        out_spec(3, 4, 2, 8, [T(c(2), a_real=True), T(c(3), b_real=True), T(c(4), a_real=True, b_real=True, b_pad=1), T(c(5))],
                 ld=40, at=(1, 4)),                                                                    # real beside complex sources; spare columns
        out_spec(65, 2, 3, 66, [T(c(0), b_pad=2), T(c(1), a_t=True, b_t=True)], ld=200, at=(0, 0)),    # extents 65 and 66: just above the wave
    ]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'rounded'])
@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_branches_between_guard_bands(bb, rng, cplx, exact):
    run_cabi(bb, rng, _branch_outputs(cplx), cplx, exact)


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_thousands_of_one_by_one_tiles_beside_a_large_one(bb, rng, cplx):
    """3001 waves of one element (with the large tile: a number of items that is no multiple of the four of a workgroup) and
    a tile of 24 (pairs of doubles) or 48 (complex) work items in their midst"""
    outs = [out_spec(1, 1, 1, 1, [term_spec(_coeff(k, cplx), off=k % 2)] * (k % 3), ld=2, at=(0, k % 2)) for k in range(3001)]
    outs.insert(1500, out_spec(16, 8, 24, 16, [term_spec(_coeff(1, cplx)), term_spec(_coeff(3, cplx), a_t=True)], ld=384, at=(0, 0)))
    run_cabi(bb, rng, outs, cplx, True)


def test_kernel_empty_lists(bb):
    for fn in (bb.lib.cyb_outer_weighted_f64, bb.lib.cyb_outer_weighted_c128):
        assert fn(bb.ctx.handle, None, 0, None, 0) == _lib.CYB_OK


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_invalid_records_are_refused_before_anything_is_launched(bb, rng, cplx):
    """negative extents, an extent beyond 2^30, a bad term range, ldd below the width of a tile of several rows, NULL dst / a / b
    of a non-empty output, a complex coefficient at the float64 entry: the error comes back, destination and sentinels stay as
    they were, and the context serves the next valid call"""
    def outputs():
        return [out_spec(2, 2, 3, 2, [term_spec(1.0)]), out_spec(3, 1, 2, 4, [term_spec(-2.0), term_spec(0.5, a_t=True)])]

    def set_(arr, k, field, value):
        arr[k][field] = value

    spoil = [
        (lambda o, t: set_(o, 1, 'ha', -1), 'negative extent'),
        (lambda o, t: set_(o, 0, 'wb', -2), 'negative extent'),
        (lambda o, t: set_(o, 1, 'hb', 2 ** 31), 'extent too large'),
        (lambda o, t: set_(o, 1, 'n_terms', 3), 'bad term range'),
        (lambda o, t: set_(o, 1, 'first_term', -1), 'bad term range'),
        (lambda o, t: set_(o, 1, 'ldd', 7), 'ldd'),
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
