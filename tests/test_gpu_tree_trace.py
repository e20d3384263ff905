"""Device side of the fusion-tree partial trace: the cases of tests/test_tree_trace.py through HipBlockBackend (same inputs,
same criteria), and the weighted trace kernel (csrc/tree_trace.hip) at the C-ABI between guard bands against an
element-by-element numpy model.

Exact data: integers in [-15, 15] under coefficients from {1, -2, 0.5, i, -0.5i, 1+i} -- every partial sum is representable,
so the comparison is ``==`` whatever the summation order or FMA contraction.  Rounded data: ``standard_normal`` against
``np.longdouble`` with the componentwise bound |err| <= (N + 4) 2^-53 S, N the number of addends of the element over all its
terms, S = sum_t (|c_re| + |c_im|) sum_tau (|s_re| + |s_im|): N - 1 additions in any order and the roundings of one complex
product per term."""
import ctypes as C

import numpy as np
import pytest

import tree_trace_cases as cases
from cyten_amd import _lib
from cyten_amd import fusion_tree as ft

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 8
COEFFS = [1.0, -2.0, 0.5, 1j, -0.5j, 1 + 1j]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the host tests on the device

@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('name', ['codomain', 'domain', 'both', 'two_pairs', 'between'])
def test_device_partial_trace_of_abelian_trees_is_the_index_paired_sum_of_the_dense_tensor(bb, rng, name, cplx):
    cases.check_abelian(bb, rng, name, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_tiles_without_a_term_are_written_as_zeros(bb, rng, cplx):
    cases.check_abelian(bb, rng, 'between', cplx, starve=True)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_full_trace_is_the_one_by_one_block_and_equals_trace_full(bb, rng, cplx):
    cases.check_full_trace(bb, rng, cplx)


@pytest.mark.parametrize('cplx_data', [False, True])
def test_device_random_tables_with_complex_factors_match_the_restatement(bb, rng, cplx_data):
    cases.check_forest(bb, rng, cplx_data)


def test_device_real_data_under_real_factors_stays_real(bb, rng):
    cases.check_forest(bb, rng, False, cplx_factors=False)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_move_braids_first_and_equals_the_dense_permute_then_trace(bb, rng, cplx):
    cases.check_move(bb, rng, cplx)


def test_device_partial_trace_is_one_launch(bb, rng, monkeypatch):
    """one C-ABI call for the tensor, counted through a proxy of the library"""
    c = cases.forest_case(rng, True)
    dev = cases.to_dev(bb, c['data'])
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith('cyb_') or name in ('cyb_last_error', 'cyb_ctx_set_stream'):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped

    monkeypatch.setattr(bb, 'lib', Counting(bb.lib))
    ft.partial_trace(bb, dev, c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt'], discard=False)
    assert calls == ['cyb_trace_weighted_c128']


def test_backend_refuses_too_many_axes_and_pairs_and_mixed_destinations(bb, rng):
    src9 = bb.as_block(rng.standard_normal((2,) * 9))
    dst1 = bb.as_block(np.zeros(2))
    with pytest.raises(ValueError, match='more than 8 axes'):
        bb.tree_trace_many([(dst1, [(src9, [0, 2, 4, 6], [1, 3, 5, 7], [8], 1.0)])])
    src10 = bb.as_block(rng.standard_normal((2,) * 10))
    with pytest.raises(ValueError, match='more than 4 traced pairs'):
        bb.tree_trace_many([(bb.as_block(np.zeros(())), [(src10, [0, 2, 4, 6, 8], [1, 3, 5, 7, 9], [], 1.0)])])
    with pytest.raises(ValueError, match='more than 8 axes'):
        bb.tree_trace_many([(bb.as_block(np.zeros((1,) * 9)), [])])
    with pytest.raises(ValueError, match='share one dtype'):
        bb.tree_trace_many([(dst1, []), (bb.as_block(np.zeros(2, dtype=complex)), [])])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_trace_many([(dst1, [(bb.as_block(rng.standard_normal((2, 3, 3))), [1], [2], [0], 1j)])])
    with pytest.raises(ValueError, match='do not match'):
        bb.tree_trace_many([(dst1, [(bb.as_block(rng.standard_normal((2, 3, 4))), [1], [2], [0], 1.0)])])
    # a float64 source under a complex destination is read as it stands; a strided destination view is written in place
    big = bb.as_block(np.full((5, 7), SENTINEL + 0j))
    src = rng.integers(-15, 16, (3, 2, 4, 3)).astype(float)
    bb.tree_trace_many([(bb.get_item(big, (slice(1, 3), slice(2, 6))), [(bb.as_block(src), [0], [3], [1, 2], 1 + 1j)])])
    want = np.full((5, 7), SENTINEL + 0j)
    want[1:3, 2:6] = (1 + 1j) * np.einsum('abca->bc', src)
    assert np.array_equal(bb.to_numpy(big), want)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

class Arena:
    """a host image of one device buffer: blocks are carved out between guard bands of `fill`"""

    def __init__(self, cplx, fill):
        self.dtype = np.complex128 if cplx else np.float64
        self.fill = fill
        self.size = GUARD
        self.blocks = []

    def block(self, n):
        off = self.size
        self.blocks.append((off, n))
        self.size += n + GUARD + (n + GUARD) % 2      # blocks start at even offsets: 16-byte aligned float64 blocks
        return off

    def host(self):
        return np.full(self.size, self.fill, dtype=self.dtype)


def _upload(bb, img):
    buf = bb.ctx.empty(len(img), 'complex128' if img.dtype == np.complex128 else 'float64')
    bb.ctx.h2d(buf, img)
    return buf


def _c_strides(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= d
    return st[::-1]


def out_spec(shape, terms, split=0, ld=None, at=(1, 1)):
    """one output: remaining `shape`, the first `split` axes are the rows of the tile, the others its columns; the tile sits at
    row / column `at` of a block with the leading dimension `ld` (default: odd, two spare columns at least)"""
    return dict(shape=tuple(shape), split=split, ld=ld, at=at, terms=terms)


def term_spec(ext, coeff=1.0, real=False, layout='overlap', off=1):
    """one term: pair extents `ext`; `layout` of its source view, which starts `off` elements into its NaN parent:
    'overlap': 1-D windows, ``src[r_linear + tau_linear]`` -- the windows of neighbouring elements overlap;
    'diag': a C-contiguous array (remaining..., n0, n0, n1, n1, ...), a pair walks the sum of its two strides;
    'perm': the same array with the pair axes in front, (n0, n0, ..., remaining...)"""
    return dict(ext=tuple(ext), coeff=coeff, real=real, layout=layout, off=off)


def _source_strides(shape, ext, layout):
    """(rem_strides, pair_strides, number of elements the view spans)"""
    if layout == 'overlap':
        ps = _c_strides(ext[::-1])[::-1] if ext else []
        R, A = int(np.prod(shape, dtype=np.int64)), int(np.prod(ext, dtype=np.int64))
        return _c_strides(shape), ps, (R + A if R and A else 0)
    doubled = [n for n in ext for _ in (0, 1)]
    full = (list(shape) + doubled) if layout == 'diag' else (doubled + list(shape))
    st = _c_strides(full)
    rem = st[:len(shape)] if layout == 'diag' else st[len(doubled):]
    pst = st[len(shape):] if layout == 'diag' else st[:len(doubled)]
    return rem, [pst[2 * p] + pst[2 * p + 1] for p in range(len(ext))], int(np.prod(full, dtype=np.int64))


def run_cabi(bb, rng, outputs, cplx, exact, expect=_lib.CYB_OK, mutate=None):
    """lay the records out (destination tiles inside blocks between SENTINEL bands, source views inside NaN parents), launch
    ONCE and compare: every byte outside the tiles bit for bit with the image before the call, the tiles with the model
    (``==`` for exact data, the bound of the module docstring for rounded data), the sources with themselves.  Then launch
    again: the same bits.  `mutate(oarr, tarr)` may spoil the records; with `expect` an error nothing may have changed."""
    dst_a, src_c, src_r = Arena(cplx, SENTINEL), Arena(True, complex(np.nan, np.nan)), Arena(False, np.nan)
    oarr = np.zeros(max(len(outputs), 1), dtype=_lib.TRACE_WEIGHTED_OUT_DTYPE)
    n_terms = sum(len(o['terms']) for o in outputs)
    tarr = np.zeros(max(n_terms, 1), dtype=_lib.TRACE_WEIGHTED_TERM_DTYPE)
    lay, t = [], 0
    for k, o in enumerate(outputs):
        shape, h = o['shape'], o['split']
        rows, cols = int(np.prod(shape[:h], dtype=np.int64)), int(np.prod(shape[h:], dtype=np.int64))
        r0, c0 = o['at']
        ld = o['ld'] if o['ld'] is not None else cols + c0 + 2 + (cols + c0 + 1) % 2
        n = (rows + r0 + 1) * ld
        off = dst_a.block(n)
        strides = [ld * s for s in _c_strides(shape[:h])] + _c_strides(shape[h:])
        oarr[k]['ndim'], oarr[k]['first_term'], oarr[k]['n_terms'] = len(shape), t, len(o['terms'])
        oarr[k]['shape'][:len(shape)], oarr[k]['dst_strides'][:len(shape)] = shape, strides
        tl = []
        for tm in o['terms']:
            rem, pst, span = _source_strides(shape, tm['ext'], tm['layout'])
            arena = src_c if cplx and not tm['real'] else src_r
            soff = arena.block(span + tm['off']) + tm['off']
            tarr[t]['coeff_re'], tarr[t]['coeff_im'] = complex(tm['coeff']).real, complex(tm['coeff']).imag
            tarr[t]['src_real'], tarr[t]['n_pairs'] = int(cplx and tm['real']), len(tm['ext'])
            tarr[t]['rem_strides'][:len(shape)], tarr[t]['pair_extent'][:len(pst)], tarr[t]['pair_stride'][:len(pst)] = rem, tm['ext'], pst
            tl.append((arena, soff, span, rem, pst))
            t += 1
        lay.append((off + r0 * ld + c0, strides, tl))
    dst, simg_c, simg_r = dst_a.host(), src_c.host(), src_r.host()
    for _, _, tl in lay:
        for arena, soff, span, _, _ in tl:
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
        for arena, soff, _, _, _ in tl:
            tarr[t]['src'] = (d_c.data_ptr() + 16 * soff) if arena is src_c else (d_r.data_ptr() + 8 * soff)
            t += 1
    # the model, one output at a time
    want, bound, tiles = dst.copy(), np.zeros(len(dst)), np.zeros(len(dst), dtype=bool)
    wide = np.clongdouble if cplx else np.longdouble
    for o, (doff, strides, tl) in zip(outputs, lay):
        shape = o['shape']
        R = int(np.prod(shape, dtype=np.int64))
        if R == 0:
            continue
        ridx = np.indices(shape).reshape(len(shape), R) if shape else np.zeros((0, 1), dtype=np.int64)
        at = doff + (np.asarray(strides, dtype=np.int64) @ ridx if shape else np.zeros(1, dtype=np.int64))
        acc, S, N = np.zeros(R, dtype=np.complex128 if exact else wide), np.zeros(R), 0
        for tm, (arena, soff, span, rem, pst) in zip(o['terms'], tl):
            ext = tm['ext']
            A = int(np.prod(ext, dtype=np.int64))
            if A == 0:
                continue
            tau = np.indices(ext).reshape(len(ext), A) if ext else np.zeros((0, 1), dtype=np.int64)
            offs = (soff + (np.asarray(rem, dtype=np.int64) @ ridx if shape else np.zeros(1, dtype=np.int64)))[:, None] \
                + (np.asarray(pst, dtype=np.int64) @ tau if ext else np.zeros(1, dtype=np.int64))[None, :]
            vals = (simg_c if arena is src_c else simg_r)[offs]
            c = complex(tm['coeff'])
            acc = acc + (c if exact else wide(c if cplx else c.real)) * (vals.sum(axis=1) if exact else vals.astype(wide).sum(axis=1))
            S += (abs(c.real) + abs(c.imag)) * (np.abs(vals.real) + np.abs(vals.imag)).sum(axis=1)
            N += A
        assert not np.isnan(np.asarray(acc, dtype=np.complex128)).any()                # the model never left a view
        want[at] = np.asarray(acc, dtype=np.complex128) if cplx else np.asarray(acc.real, dtype=np.float64)
        bound[at] = (N + 4) * 2.0 ** -53 * S
        tiles[at] = True
    if mutate is not None:
        mutate(oarr, tarr)
    fn = bb.lib.cyb_trace_weighted_c128 if cplx else bb.lib.cyb_trace_weighted_f64
    args = (bb.ctx.handle, oarr.ctypes.data_as(C.POINTER(_lib.TraceWeightedOut)), len(outputs),
            tarr.ctypes.data_as(C.POINTER(_lib.TraceWeightedTerm)), n_terms)
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


def _regime_outputs(cplx):
    """the smallest shapes that reach each branch: R elements, A addends (thresholds of the owner rule: A = 64, A = 4096,
    R = 1024, R = 65536; work items of 1024 elements)"""
    c = lambda k: _coeff(k, cplx)                                                      # noqa: E731
    return [
        out_spec((37,), [term_spec((3,), c(0), layout='diag')]),                                       # lane
        out_spec((5,), [term_spec((63,), c(1))]),                                                      # lane, just below the wave threshold
        out_spec((5,), [term_spec((64,), c(2))], split=1),                                             # wave
        out_spec((5,), [term_spec((9, 7), c(3), layout='diag')]),                                      # 63 addends in two pairs: lane
        out_spec((5,), [term_spec((8, 8), c(4), layout='diag')]),                                      # 64: wave
        out_spec((3,), [term_spec((4096,), c(5))]),                                                    # workgroup
        out_spec((3,), [term_spec((4095,), c(0))]),                                                    # wave, just below
        out_spec((3,), [term_spec((2000,), c(1)), term_spec((2000,), c(2), off=3), term_spec((97,), c(3), real=True)], split=1),   # 4097 over 3 terms
        out_spec((1030,), [term_spec((4096,), c(4))]),                                                 # back to waves: R >= 1024
        out_spec((7, 10000), [term_spec((64,), c(5))], split=1),                                       # R = 70000: lanes by element count, several work items
        out_spec((50, 50), [term_spec((3,), c(0), layout='diag'), term_spec((3,), c(1), layout='perm', real=True)], split=1),      # R = 2500: several work items
    ]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'rounded'])
@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_owner_regimes_and_their_thresholds(bb, rng, cplx, exact):
    run_cabi(bb, rng, _regime_outputs(cplx), cplx, exact)


def _shape_outputs(cplx):
    c = lambda k: _coeff(k, cplx)                                                      # noqa: E731
    return [
        out_spec((0, 5), [term_spec((3,), c(0))], split=1),                                            # R = 0
        out_spec((4, 3), [], split=1),                                                                 # no terms: zeros are written
        out_spec((2, 3), [term_spec((0,), c(1))], split=1),                                            # a term without addends
        out_spec((3, 4), [term_spec((2,), c(1), layout='diag'), term_spec((2, 3), c(2), layout='perm'),
                          term_spec((2, 1, 3), c(3), layout='overlap')], split=1),                      # 1, 2 and 3 pairs in one output
        out_spec((), [term_spec((2, 3, 2, 2), c(4), layout='diag'), term_spec((2, 1, 3, 2), c(3)),
                      term_spec((5,), c(0), layout='diag')]),                                          # ndim 0 + 4 pairs = 8 axes, next to 1 pair
        out_spec((3, 2), [term_spec((2, 2, 3), c(5), layout='diag')], split=1),                        # ndim 2 + 3 pairs = 8 axes
        out_spec((2, 3, 2, 2), [term_spec((3, 2), c(0), layout='perm')], split=2),                     # ndim 4 + 2 pairs = 8 axes
        out_spec((2, 2, 1, 2, 1, 3, 1, 2), [], split=3),                                               # ndim 8
        out_spec((3, 5), [term_spec((4,), c(1), real=True, layout='diag'), term_spec((4,), c(3), layout='diag'),
                          term_spec((2, 2), c(5), real=True, layout='perm')], split=1),                 # float64 sources next to complex ones
        out_spec((6, 8), [term_spec((3,), c(2), layout='perm', off=2)], split=1, ld=12, at=(1, 2)),    # every run 16-byte aligned: pairs of doubles
        out_spec((6, 8), [term_spec((3,), c(2), layout='perm', off=1)], split=1, ld=12, at=(1, 2)),    # ... but for the source
        out_spec((50, 50), [term_spec((3,), c(0), layout='perm', off=2), term_spec((2, 2), c(1), layout='perm', off=4)],
                 split=1, ld=54, at=(2, 2)),                                                           # 1250 pairs of doubles: two work items
        out_spec((66, 1), [term_spec((70,), c(4))], split=1),                                          # a wave per row of a one-column tile
    ]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'rounded'])
@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_shapes_pairs_and_mixed_sources(bb, rng, cplx, exact):
    run_cabi(bb, rng, _shape_outputs(cplx), cplx, exact)


def test_kernel_empty_lists(bb):
    for fn in (bb.lib.cyb_trace_weighted_f64, bb.lib.cyb_trace_weighted_c128):
        assert fn(bb.ctx.handle, None, 0, None, 0) == _lib.CYB_OK


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_invalid_records_are_refused_before_anything_is_launched(bb, rng, cplx):
    """too many axes, a bad term range, a NULL destination of a non-empty output, a complex coefficient at the float64 entry:
    the error comes back, destination and sentinels stay as they were, and the context serves the next valid call"""
    def outputs():
        return [out_spec((4, 3), [term_spec((3,), 1.0, layout='diag')], split=1),
                out_spec((2, 2, 2), [term_spec((2, 2), -2.0, layout='diag'), term_spec((5,), 0.5)], split=1)]

    def set_(arr, k, field, value):
        arr[k][field] = value

    spoil = [
        (lambda o, t: set_(o, 1, 'ndim', 9), 'out of range'),
        (lambda o, t: set_(o, 1, 'ndim', -1), 'out of range'),
        (lambda o, t: set_(t, 1, 'n_pairs', 3), 'source axes'),                # 3 + 2 * 3 axes
        (lambda o, t: set_(t, 1, 'n_pairs', 5), 'traced pairs'),
        (lambda o, t: set_(o, 1, 'n_terms', 3), 'bad term range'),
        (lambda o, t: set_(o, 1, 'first_term', -1), 'bad term range'),
        (lambda o, t: set_(o, 1, 'dst', 0), 'dst is NULL'),
        (lambda o, t: set_(t, 2, 'src', 0), 'src is NULL'),
        (lambda o, t: o[1]['shape'].__setitem__(1, -2), 'negative extent'),
        (lambda o, t: t[2]['pair_extent'].__setitem__(0, -5), 'negative extent'),
    ]
    if not cplx:
        spoil.append((lambda o, t: set_(t, 0, 'coeff_im', 0.5), 'complex coefficient'))
    for mutate, frag in spoil:
        run_cabi(bb, rng, outputs(), cplx, True, expect=_lib.CYB_ERR_INVALID, mutate=mutate)
        assert frag in bb.lib.cyb_last_error().decode()
    run_cabi(bb, rng, outputs(), cplx, True)
