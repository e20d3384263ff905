"""Segment kernels of the HIP block backend (csrc/segment_ops.hip: cyb_seg_binary, cyb_seg_reduce, cyb_seg_compact) and
the diagonal-tensor / mask functions of cyten_amd.abelian on the device, through the C-ABI.  Every kernel result is compared
with numpy on the downloaded inputs.

Tolerances, u = 2^-53.  All derived, none tuned.
  * float64 add, sub, mul, div: one correctly rounded operation on both sides -> ``np.array_equal``.
  * comparisons, logical ops, counts, any / all, max / min, index tables, data movement: exact.
  * complex mul: each side rounds a two-term sum of products per component, error <= 2u |a| |b|, and may or may not contract it
    to an FMA -> |got - want| <= 4 * 2^-52 * |a| |b| (the bound of tests/test_gpu_tensor_products.py).
  * complex div: the kernel computes a conj(b) / |b|^2 -- d = fl(b_r^2 + b_i^2), then per component fl(fl(a_r b_r + a_i b_i) / d).
    d carries a relative error <= 2u (two products, one sum, all terms positive); a numerator carries an absolute error
    <= 2u (|a_r b_r| + |a_i b_i|) <= 2u |a| |b|; the division adds u.  Per component |err| <= (2u + 2u + u) |a| |b| / |b|^2 to first
    order, so the complex error is <= sqrt(2) * 5u |a| / |b| = 7.1 u |a| / |b| < 8 * 2^-52 |a| / |b| = 16 u |a| / |b|, the bound asserted.  The
    expectation is numpy's quotient in extended precision (np.clongdouble, error ~2^-63: negligible), so that the bound holds
    the kernel's error alone; |b| is drawn from [0.5, 2], no scaling question arises.  A divisor with zero imaginary part
    takes one correctly rounded division per component (exact agreement with numpy for real / real).
  * sums: 2 n u sum|x_i|, the summation-order bound of DESIGN.md 4.8 (both sides add the same numbers in different orders).
  * pre-mapped sums (x log x, x^p, x^2, |x|): numpy's sum of the terms the EXISTING per-block device functions give
    (``stable_log`` and ``*``, ``pow``, ``abs``), bound (2n + 2) u sum|t_i| -- 2u per term for the product rounding that an FMA
    contraction may remove on either side.
  * entropy end to end against the numpy branch of the reference: 1e-12 relative, the project's line for floats.
The error cases are argument checks on the host: nothing here hands the device anything that could fault it."""
import collections
import ctypes as C

import numpy as np
import pytest

import diag_mask_ref as ref
from cyten_amd import _lib
from cyten_amd import abelian as ab
from diag_mask_cases import flags_cases, pair_cases, to_diag
from test_diag_masks import _bool_diag, check_svd_apply_mask, svd_tensors

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# 0, 1, 2, around the wave (64) and workgroup (256) sizes, either side of every regime threshold (64: lanes | wave,
# 1024: wave | workgroup, 16384: one workgroup | chunks), and a segment of 19 chunks with an odd length
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 300001]
assert _lib.SEG_LANES_MAX == 64 and _lib.SEG_WAVE_MAX == 1024 and _lib.SEG_CHUNK == 16384


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
    """(C-ABI call counter of bb.lib, sizes in bytes of the downloads through bb.ctx.d2h, of the uploads through bb.ctx.h2d)"""
    lib = _CountingLib(bb.lib)
    monkeypatch.setattr(bb, 'lib', lib)
    downloads, uploads, real_d2h, real_h2d = [], [], bb.ctx.d2h, bb.ctx.h2d

    def d2h(src, n, np_dtype, *args, **kw):
        downloads.append(int(n) * np.dtype(np_dtype).itemsize)
        return real_d2h(src, n, np_dtype, *args, **kw)

    def h2d(dst, src, *args, **kw):
        uploads.append(np.asarray(src).nbytes)
        return real_h2d(dst, src, *args, **kw)
    monkeypatch.setattr(bb.ctx, 'd2h', d2h)
    monkeypatch.setattr(bb.ctx, 'h2d', h2d)
    return lib, downloads, uploads


def _calls(lib):
    return {k: v for k, v in lib.calls.items() if k != 'cyb_last_error'}


def _draw(rng, n, kind):
    if kind == 'bool':
        return rng.random(n) < 0.5
    x = np.round(rng.standard_normal(n), 1)            # (ties and exact zeros occur)
    if kind == 'c128':
        return x + 1j * np.round(rng.standard_normal(n), 1)
    return x


def _upload(bb, arrays, odd=False):
    """device blocks of a list of 1-D arrays (None stays None); `odd`: every numeric block starts on an odd double of a shared
    pool, i.e. is 8- but not 16-byte aligned"""
    if not odd:
        return [None if a is None else bb.as_block(a) for a in arrays]
    out = []
    for a in arrays:
        if a is None or a.dtype == bool:
            out.append(None if a is None else bb.as_block(a))
            continue
        host = np.zeros(len(a) + 3, dtype=a.dtype)
        host[1:1 + len(a)] = a
        blk = bb.get_item(bb.as_block(host), (slice(1, 1 + len(a)),))
        if a.dtype == np.float64:
            assert blk.ptr % 16 == 8
        out.append(blk)
    return out


def _with_absent(rng, arrays, p=0.25):
    return [None if (len(a) and rng.random() < p) else a for a in arrays]


def _zeros_like_absent(a, n, kind):
    return np.zeros(n, dtype={'f64': float, 'c128': complex, 'bool': bool}[kind]) if a is None else a


def _check_binary(bb, op, A, B, lengths, kinds, dA, dB, scalar=None, worst=None):
    items = [(x, None if scalar is not None else y, n) for x, y, n in zip(dA, dB, lengths)]
    got = bb.seg_binary_many(items, op, scalar=scalar)
    cplx = any(np.iscomplexobj(x) for x in list(A) + list(B) if x is not None) or np.iscomplexobj(scalar)
    assert len(got) == len(lengths)
    for g, a, b, n in zip(got, A, B, lengths):
        assert g.shape == (n,) and g.is_contiguous()
        a = _zeros_like_absent(a, n, kinds[0])
        b = scalar if scalar is not None else _zeros_like_absent(b, n, kinds[1])
        g = bb.to_numpy(g)
        if op in ref.ARITH:
            assert g.dtype == (np.complex128 if cplx else np.float64)
            fa, fb = ref._num(a), ref._num(b)
            if not cplx:
                with np.errstate(all='ignore'):
                    assert np.array_equal(g, ref.ARITH[op](fa, fb), equal_nan=True), (op, n)
            elif op in ('add', 'sub'):
                assert np.array_equal(g, ref.ARITH[op](fa, fb).astype(complex)), (op, n)
            elif op == 'mul':
                err, bound = np.abs(g - fa * fb), 4 * 2.0 ** -52 * np.abs(fa) * np.abs(fb)
                assert np.all(err <= bound), (op, n)
                if worst is not None and n and bound.max() > 0:
                    worst['cmul'] = max(worst.get('cmul', 0.0), float((err / np.where(bound > 0, bound, 1.0)).max()))
            else:
                fb = np.broadcast_to(np.asarray(fb), (n,))
                ok = np.abs(fb) > 0                                      # (x / 0 is inf or nan on both sides: not compared)
                want = (np.asarray(fa, dtype=np.clongdouble)[ok] / np.asarray(fb, dtype=np.clongdouble)[ok])
                err = np.abs(np.asarray(g[ok], dtype=np.clongdouble) - want).astype(float)
                bound = 8 * 2.0 ** -52 * np.abs(fa[ok]) / np.abs(fb[ok])
                assert np.all(err <= bound), (op, n)
                if worst is not None and err.size and bound.max() > 0:
                    worst['cdiv'] = max(worst.get('cdiv', 0.0), float((err / np.where(bound > 0, bound, 1.0)).max()))
        else:
            assert g.dtype == np.bool_
            if op in ref.LOGICAL or op == 'not':
                a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
            assert np.array_equal(g, ref.block_binary(a, b, op)), (op, n)


KIND_PAIRS = [('f64', 'f64'), ('c128', 'c128'), ('f64', 'c128'), ('c128', 'f64'), ('bool', 'bool'), ('bool', 'f64')]


@pytest.mark.parametrize('kinds', KIND_PAIRS, ids=['-'.join(k) for k in KIND_PAIRS])
@pytest.mark.parametrize('odd', [False, True], ids=['aligned', 'odd-double'])
def test_seg_binary_every_op(bb, kinds, odd):
    """every op on the full list of lengths in ONE call each; operands absent on either side; real beside complex"""
    rng = np.random.default_rng(21)
    A = _with_absent(rng, [_draw(rng, n, kinds[0]) for n in LENGTHS])
    B = _with_absent(rng, [_draw(rng, n, kinds[1]) for n in LENGTHS])
    A[-1], B[-2] = None, None                                         # (the long segment and a chunked one among the absent)
    if 'c128' in kinds:                                               # |b| in [0.5, 2] for the division
        B = [None if b is None else b if not np.iscomplexobj(b) else
             rng.uniform(0.5, 2.0, len(b)) * np.exp(2j * np.pi * rng.random(len(b))) for b in B]
        if kinds[1] == 'f64':
            B = [None if b is None else np.where(b == 0, 0.5, b) for b in B]
    dA, dB = _upload(bb, A, odd), _upload(bb, B, odd)
    cplx = 'c128' in kinds
    ops = list(ref.ARITH) + (['eq', 'ne'] if cplx else list(ref.COMPARE))
    if kinds == ('bool', 'bool'):
        ops += list(ref.LOGICAL) + ['not']
    worst = {}
    for op in ops:
        _check_binary(bb, op, A, B, LENGTHS, kinds, dA, dB, worst=worst)
    for op, scalar in (('ge', 0.3), ('lt', -0.1), ('eq', 0.0), ('mul', 2.5), ('sub', 0.5)) if not cplx else (('eq', 0.3 + 0.1j), ('mul', 1 - 2j), ('div', 0.6 + 0.8j)):
        _check_binary(bb, op, A, B, LENGTHS, kinds, dA, dB, scalar=scalar, worst=worst)
    print(f'seg_binary {kinds} odd={odd}: largest error / bound = {worst}')


@pytest.mark.parametrize('n_segs', [1, 59, 300])
def test_seg_binary_lists_of_mixed_lengths(bb, n_segs):
    rng = np.random.default_rng(22 + n_segs)
    lengths = [int(x) for x in rng.choice([0, 1, 2, 3, 17, 63, 64, 65, 130, 257, 1024, 1025, 2000], n_segs)]
    if n_segs > 1:
        lengths[n_segs // 2] = 16385
    A = _with_absent(rng, [_draw(rng, n, 'f64') for n in lengths])
    B = _with_absent(rng, [_draw(rng, n, 'f64') for n in lengths])
    dA, dB = _upload(bb, A), _upload(bb, B)
    for op in ('add', 'mul', 'le', 'ne'):
        _check_binary(bb, op, A, B, lengths, ('f64', 'f64'), dA, dB)
    assert bb.seg_binary_many([], 'add') == []


def _reduce_want(x, op, pre, param):
    return ref.block_reduce(x, op, pre, param)


@pytest.mark.parametrize('odd', [False, True], ids=['aligned', 'odd-double'])
def test_seg_reduce_every_reduction(bb, odd):
    rng = np.random.default_rng(23)
    worst = {}
    for kind in ('f64', 'c128', 'bool'):
        X = _with_absent(rng, [_draw(rng, n, kind) for n in LENGTHS], 0.15)
        X[3] = None
        dX = _upload(bb, X, odd)
        for op in ('sum', 'count') + (() if kind == 'c128' else ('max', 'min')):
            table = bb.seg_reduce_many(dX, LENGTHS, op)
            assert table.shape == (len(LENGTHS), 2) and table.dtype == np.float64
            for row, x, n in zip(table, X, LENGTHS):
                x = _zeros_like_absent(x, n, kind)
                want = _reduce_want(x, op, None, None)
                got = complex(row[0], row[1]) if kind == 'c128' else row[0]
                if op == 'sum' and kind != 'bool':
                    bound = 2 * n * U * np.abs(x).sum()
                    assert abs(got - want) <= bound, (kind, op, n)
                    if bound > 0:
                        worst['sum'] = max(worst.get('sum', 0.0), abs(got - want) / bound)
                else:
                    assert got == want and row[1] == 0.0, (kind, op, n)           # counts, extrema, sums of 0 / 1: exact
    print(f'seg_reduce odd={odd}: largest error / bound = {worst}')


def test_seg_reduce_pre_maps(bb):
    """the pre-mapped sums against numpy's sum of the terms of the existing per-block device functions"""
    rng = np.random.default_rng(24)
    lengths = [n for n in LENGTHS if n]
    X = [np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-40, 1, n) for n in lengths]       # probabilities down to below the cutoff
    for x in X:
        x[::7] = 0.0
    dX = _upload(bb, X)
    signed = [rng.standard_normal(n) for n in lengths]
    dS = _upload(bb, signed)
    worst = 0.0
    for pre, param, blocks, host in (('xlogx', 1e-30, dX, X), ('pow', 2.5, dX, X), ('pow', 0.5, dX, X), ('square', None, dS, signed), ('abs', None, dS, signed)):
        table = bb.seg_reduce_many(blocks, lengths, 'sum', pre, param)
        for row, blk, x, n in zip(table, blocks, host, lengths):
            if pre == 'xlogx':
                terms = bb.to_numpy(blk * bb.stable_log(blk, param))
            elif pre == 'pow':
                terms = bb.to_numpy(blk.pow(param))
            elif pre == 'square':
                terms = bb.to_numpy(blk * blk)
            else:
                terms = bb.to_numpy(bb.abs(blk))
            bound = (2 * n + 2) * U * np.abs(terms).sum()
            assert abs(row[0] - terms.sum()) <= bound and row[1] == 0.0, (pre, param, n)
            if bound > 0:
                worst = max(worst, abs(row[0] - terms.sum()) / bound)
    # max / min / count see the pre-mapped values too (exact: the same values, no summation)
    table = bb.seg_reduce_many(dS, lengths, 'max', 'abs')
    assert all(row[0] == np.abs(x).max() for row, x in zip(table, signed))
    table = bb.seg_reduce_many(_upload(bb, [x + 1j * x[::-1] for x in signed]), lengths, 'max', 'abs')
    assert all(abs(row[0] - np.abs(x + 1j * x[::-1]).max()) <= 4 * U * row[0] for row, x in zip(table, signed))    # hypot: 1 ulp on each side
    print(f'seg_reduce pre-maps: largest error / bound = {worst:.3f}')


@pytest.mark.parametrize('n_segs', [1, 59, 300])
def test_seg_reduce_and_compact_lists_and_independence(bb, n_segs):
    """lists of mixed lengths; a segment's numbers and tables do not depend on the rest of the list or on the run"""
    rng = np.random.default_rng(25 + n_segs)
    lengths = [int(x) for x in rng.choice([0, 1, 2, 5, 63, 64, 65, 200, 256, 257, 1024, 1025, 3000], n_segs)]
    lengths[n_segs // 2] = 40000
    X = [_draw(rng, n, 'f64') for n in lengths]
    dX = _upload(bb, X)
    table = bb.seg_reduce_many(dX, lengths, 'sum')
    for row, x, n in zip(table, X, lengths):
        assert abs(row[0] - x.sum()) <= 2 * n * U * np.abs(x).sum()
    again = bb.seg_reduce_many(dX, lengths, 'sum')
    assert np.array_equal(table, again)                                                     # run to run
    for s in sorted({0, n_segs // 2, n_segs - 1}):
        alone = bb.seg_reduce_many([dX[s]], [lengths[s]], 'sum')
        assert np.array_equal(alone[0], table[s])                                           # alone or in the list
    tables, counts = bb.seg_compact_many(dX)
    assert counts.dtype == np.int64 and len(tables) == n_segs
    for t, k, x in zip(tables, counts, X):
        assert t.n == k == np.count_nonzero(x)
    pos = _tables_to_numpy(bb, tables)
    assert all(np.array_equal(p, np.flatnonzero(x)) for p, x in zip(pos, X))


def _tables_to_numpy(bb, tables):
    """the kept positions of a list of DeviceIndex tables (they share one owner buffer)"""
    out = []
    for t in tables:
        off = (t.ptr - t.owner.data_ptr()) // 8
        out.append(bb.ctx.d2h(t.owner, t.n, np.int64, off) if t.n else np.zeros(0, np.int64))
    return out


@pytest.mark.parametrize('kind', ['bool', 'f64', 'c128'])
def test_seg_compact_every_length(bb, kind):
    rng = np.random.default_rng(26)
    for density in (0.5, 0.02, 1.0, 0.0):
        F = []
        for n in LENGTHS:
            keep = rng.random(n) < density
            F.append(keep if kind == 'bool' else np.where(keep, _draw(rng, n, kind) + 3.0, 0.0).astype(complex if kind == 'c128' else float))
        if kind == 'c128':
            F = [np.where(rng.random(len(f)) < 0.5, f, 1j * f.real) for f in F]              # kept by the imaginary part alone
        dF = _upload(bb, F, odd=kind == 'f64')
        tables, counts = bb.seg_compact_many(dF)
        assert counts.tolist() == [int(np.count_nonzero(f)) for f in F]
        for p, f in zip(_tables_to_numpy(bb, tables), F):
            assert np.array_equal(p, np.flatnonzero(f))
    assert bb.seg_compact_many([])[0] == []


# ------------------------------------------------------------------------------------------- the C-ABI directly

def _rec(a=0, b=0, out=0, n=0, a_kind=1, b_kind=1, out_kind=1):
    arr = np.zeros(1, dtype=_lib.SEG_DTYPE)
    arr['a'], arr['b'], arr['out'], arr['n'] = a, b, out, n
    arr['a_kind'], arr['b_kind'], arr['out_kind'] = a_kind, b_kind, out_kind
    return arr


def _p(arr):
    return arr.ctypes.data_as(C.POINTER(_lib.SegRec))


@pytest.mark.parametrize('n', [1, 2, 3, 64, 65, 1025, 16385 + 16384])
def test_destination_on_an_odd_double(bb, n):
    """a, b and out all 8- but not 16-byte aligned (and every mix with aligned ones): the words around the output stay untouched"""
    rng = np.random.default_rng(27)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    for la, lb, lo in ((1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 1), (1, 1, 0)):
        da, db = bb.as_block(np.concatenate([np.zeros(la), a])), bb.as_block(np.concatenate([np.zeros(lb), b]))
        out = bb.as_block(np.full(n + lo + 2, -7.0))
        bb.ctx.sync_stream()
        _lib.check(bb.lib.cyb_seg_binary(bb.ctx.handle, _p(_rec(da.ptr + 8 * la, db.ptr + 8 * lb, out.ptr + 8 * lo, n)), 1, _lib.SEG_BINARY_OPS['sub'], 0, 0.0, 0.0))
        got = bb.to_numpy(out)
        assert np.all(got[:lo] == -7.0) and np.all(got[lo + n:] == -7.0) and np.array_equal(got[lo:lo + n], a - b)
        res = bb.as_block(np.zeros(2))
        _lib.check(bb.lib.cyb_seg_reduce(bb.ctx.handle, _p(_rec(da.ptr + 8 * la, n=n)), 1, 0, 0, 0.0, C.c_void_p(res.ptr)))
        aligned = bb.seg_reduce_many([bb.as_block(a)], [n], 'sum')
        assert bb.to_numpy(res)[0] == aligned[0, 0]                       # the order of the sum does not depend on the alignment


def test_argument_checks(bb):
    """host checks only: every bad record is refused before anything is launched"""
    x, out, res = bb.as_block(np.ones(8)), bb.as_block(np.zeros(8)), bb.as_block(np.zeros(2))
    h, add = bb.ctx.handle, _lib.SEG_BINARY_OPS['add']
    bb.ctx.sync_stream()
    good = _rec(x.ptr, x.ptr, out.ptr, 8)
    _lib.check(bb.lib.cyb_seg_binary(h, _p(good), 1, add, 0, 0.0, 0.0))
    assert np.array_equal(bb.to_numpy(out), np.full(8, 2.0))
    assert bb.lib.cyb_seg_binary(h, _p(good), 0, add, 0, 0.0, 0.0) == _lib.CYB_OK                        # empty list
    assert bb.lib.cyb_seg_binary(h, _p(_rec(n=0)), 1, add, 0, 0.0, 0.0) == _lib.CYB_OK                   # zero length: nothing is addressed
    for field, value, match in (('n', -1, 'negative length'), ('a_kind', 4, 'bad kind of a'), ('b_kind', -1, 'bad kind of b'),
                                ('out_kind', 0, 'bad kind of out'), ('a', 0, 'a is NULL'), ('b', 0, 'b is NULL'), ('out', 0, 'out is NULL'),
                                ('a', x.ptr + 4, 'a is misaligned'), ('out', out.ptr + 4, 'out is misaligned'), ('out_kind', 3, 'arithmetic op writes')):
        bad = good.copy()
        bad[field] = value
        status = bb.lib.cyb_seg_binary(h, _p(bad), 1, add, 0, 0.0, 0.0)
        assert status == _lib.CYB_ERR_INVALID, field
        with pytest.raises(ValueError, match=match):
            _lib.check(status)
    for call, match in ((lambda: bb.lib.cyb_seg_binary(h, _p(good), 1, 99, 0, 0.0, 0.0), 'unknown op'),
                        (lambda: bb.lib.cyb_seg_binary(h, _p(good), 1, _lib.SEG_BINARY_OPS['lt'], 0, 0.0, 0.0), 'write bool'),
                        (lambda: bb.lib.cyb_seg_binary(h, _p(_rec(x.ptr, x.ptr, out.ptr, 4, 2, 1, 3)), 1, _lib.SEG_BINARY_OPS['lt'], 0, 0.0, 0.0), 'not ordered'),
                        (lambda: bb.lib.cyb_seg_binary(None, _p(good), 1, add, 0, 0.0, 0.0), 'ctx is NULL'),
                        (lambda: bb.lib.cyb_seg_reduce(h, _p(good), 1, 7, 0, 0.0, C.c_void_p(res.ptr)), 'unknown reduction'),
                        (lambda: bb.lib.cyb_seg_reduce(h, _p(good), 1, 0, 9, 0.0, C.c_void_p(res.ptr)), 'unknown pre-map'),
                        (lambda: bb.lib.cyb_seg_reduce(h, _p(good), 1, 0, 0, 0.0, None), 'result_dev'),
                        (lambda: bb.lib.cyb_seg_reduce(h, _p(_rec(x.ptr, n=4, a_kind=2)), 1, 1, 0, 0.0, C.c_void_p(res.ptr)), 'real segments'),
                        (lambda: bb.lib.cyb_seg_compact(h, _p(good), 1, None, C.c_void_p(res.ptr)), 'keep_idx_dev'),
                        (lambda: bb.lib.cyb_seg_compact(h, _p(good), 1, C.c_void_p(out.ptr), None), 'counts_dev'),
                        (lambda: bb.lib.cyb_seg_compact(h, _p(_rec(n=-2)), 1, C.c_void_p(out.ptr), C.c_void_p(res.ptr)), 'negative length')):
        with pytest.raises(ValueError, match=match):
            _lib.check(call())
    # the backend's own checks
    with pytest.raises(ValueError, match='unknown op'):
        bb.seg_binary_many([(x, x, 8)], 'pow')
    with pytest.raises(ValueError, match='length of its segment'):
        bb.seg_binary_many([(x, x, 7)], 'add')
    with pytest.raises(TypeError, match='boolean operands'):
        bb.seg_binary_many([(x, x, 8)], 'and')
    with pytest.raises(TypeError, match='not ordered'):
        bb.seg_binary_many([(bb.as_block(np.ones(8) + 1j), x, 8)], 'lt')
    with pytest.raises(ValueError, match='do not go together'):
        bb.seg_reduce_many([x], [8], 'sum', 'pow')
    with pytest.raises(TypeError, match='real segments'):
        bb.seg_reduce_many([bb.as_block(np.ones(8) + 1j)], [8], 'max')
    with pytest.raises(ValueError, match='1-D block'):
        bb.seg_compact_many([bb.as_block(np.ones((2, 2)))])


# ------------------------------------------------------------------------------------------- tensor level

PAIR = [c for c in pair_cases() if c['id'].startswith('u1u1')]


@pytest.mark.parametrize('case', range(len(PAIR)), ids=[c['id'] for c in PAIR])
def test_diagonal_binary_against_the_stand_in(bb, case):
    c = PAIR[case]
    nb = ref.NumpySegmentBackend()
    leg, (ka, kb) = c['leg'], c['kinds']
    ops = ['add', 'mul', 'eq'] + (['le', 'gt'] if 'complex' not in c['kinds'] else []) + (['and', 'xor'] if ka == 'bool' else [])
    mults = [int(m) for m in leg.mults]
    abs_a = ref.dense_of(mults, (c['a'][0], [np.abs(x).astype(float) for x in c['a'][1]]), float)
    abs_b = ref.dense_of(mults, (c['b'][0], [np.abs(x).astype(float) for x in c['b'][1]]), float)
    for op in ops:
        for pzz in (True, False):
            got = ab.diagonal_binary(bb, to_diag(bb, leg, c['a'], ka), to_diag(bb, leg, c['b'], kb), op, pzz)
            want = ab.diagonal_binary(nb, to_diag(nb, leg, c['a'], ka), to_diag(nb, leg, c['b'], kb), op, pzz)
            assert got.dtype == want.dtype and np.array_equal(got.block_inds, want.block_inds)
            assert all(np.dtype(g.dtype) == want.dtype and g.shape == w.shape for g, w in zip(got.blocks, want.blocks))
            G = ref.dense_of(mults, (got.block_inds.tolist(), [bb.to_numpy(g) for g in got.blocks]), want.dtype)
            W = ref.dense_of(mults, (want.block_inds.tolist(), want.blocks), want.dtype)
            if op == 'mul' and want.dtype.kind == 'c':
                assert np.all(np.abs(G - W) <= 4 * 2.0 ** -52 * abs_a * abs_b)
            else:
                assert np.array_equal(G, W)


FLAGS = [c for c in flags_cases() if c['id'].startswith(('u1u1', 'u1-'))]


@pytest.mark.parametrize('case', range(len(FLAGS)), ids=[c['id'] for c in FLAGS])
def test_masks_on_the_device(bb, case):
    c = FLAGS[case]
    leg, flags = c['leg'], c['flags']
    m = ab.diagonal_to_mask(bb, to_diag(bb, leg, _bool_diag(bb, leg, flags), 'bool'))
    want = ab.Mask.from_flags(leg, flags)

    def check(mask, w):
        assert np.array_equal(mask.block_inds, w.block_inds) and np.array_equal(mask.small_leg.mults, w.small_leg.mults)
        assert np.array_equal(mask.small_leg.sectors, w.small_leg.sectors)
        assert all(np.array_equal(bb.to_numpy(g), x) for g, x in zip(mask.blocks, w.blocks))
        assert all(np.array_equal(p, np.flatnonzero(x)) for p, x in zip(_tables_to_numpy(bb, mask.tables), w.blocks))
    check(m, want)
    check(ab.mask_unary(bb, m), ab.Mask.from_flags(leg, ~flags))
    other = np.roll(flags, 3)
    m2 = ab.diagonal_to_mask(bb, to_diag(bb, leg, _bool_diag(bb, leg, other, True), 'bool'))
    for op, fn in ref.LOGICAL.items():
        check(ab.mask_binary(bb, m, m2, op), ab.Mask.from_flags(leg, fn(flags, other)))
    check(ab.mask_binary(bb, want, m2, 'or'), ab.Mask.from_flags(leg, flags | other))          # a host mask as an operand
    assert np.array_equal(bb.to_numpy(ab.mask_to_block(bb, m)), flags)
    assert np.array_equal(ab.mask_to_diagonal(bb, m).to_numpy(bb), flags.astype(float))
    dense = np.zeros((int(flags.sum()), leg.dim))
    dense[np.arange(int(flags.sum())), np.flatnonzero(flags)] = 1.0
    assert np.array_equal(ab.full_from_mask(bb, m).to_dense(bb), dense)
    assert np.array_equal(ab.full_from_mask(bb, ab.mask_dagger(bb, m)).to_dense(bb), dense.T)
    kept = np.flatnonzero(flags)
    if len(kept):
        assert ab.get_element_mask(bb, m, [len(kept) - 1, int(kept[-1])])
        assert len(kept) == 1 or not ab.get_element_mask(bb, m, [0, int(kept[-1])])
    # projection and embedding read the device tables: the same blocks as with the host mask
    rng = np.random.default_rng(30 + case)
    t = ab.AbelianTensor(leg.symmetry, [leg.dual(), leg], [bb.as_block(rng.standard_normal((int(k), int(k)))) for k in leg.mults],
                         np.array([[i, i] for i in range(leg.nsec)]), 1)
    got, exp = ab.mask_contract(bb, t, m, 1), ab.mask_contract(bb, t, want, 1)
    assert np.array_equal(got.block_inds, exp.block_inds) and all(np.array_equal(bb.to_numpy(g), bb.to_numpy(w)) for g, w in zip(got.blocks, exp.blocks))
    back, back_exp = ab.mask_contract(bb, got, m, 1, large_leg=False), ab.mask_contract(bb, exp, want, 1, large_leg=False)
    assert all(np.array_equal(bb.to_numpy(g), bb.to_numpy(w)) for g, w in zip(back.blocks, back_exp.blocks))
    d = ab.DiagonalTensor.from_numpy(bb, leg, rng.standard_normal(leg.dim))
    small = ab.apply_mask_to_diagonal(bb, d, m)
    assert np.array_equal(small.to_numpy(bb), d.to_numpy(bb)[flags])
    # conversions of diagonals
    assert np.array_equal(bb.to_numpy(ab.diagonal_to_block(bb, d)), d.to_numpy(bb))
    full = ab.full_from_diagonal(bb, d)
    assert np.array_equal(full.to_dense(bb), np.diag(d.to_numpy(bb)))
    assert np.array_equal(ab.diagonal_from_full_tensor(bb, full, 0.0).to_numpy(bb), d.to_numpy(bb))
    assert np.array_equal(ab.diagonal_from_full_tensor(bb, t).to_numpy(bb), np.diag(t.to_dense(bb)))
    if max(leg.mults) > 1:
        with pytest.raises(ValueError, match='Not a diagonal block'):
            ab.diagonal_from_full_tensor(bb, t, 1e-9)
    assert ab.diagonal_all(bb, ab.diagonal_compare(bb, d, 'lt', 100.0)) and not ab.diagonal_any(bb, ab.diagonal_compare(bb, d, 'gt', 100.0))
    x = d.to_numpy(bb)
    assert ab.reduce_diagonal(bb, d, 'max') == x.max() and ab.reduce_diagonal(bb, d, 'min') == x.min()
    assert abs(ab.diagonal_trace_full(bb, d) - x.sum()) <= 2 * len(x) * U * np.abs(x).sum()
    assert ab.get_element_diagonal(bb, d, leg.dim - 1) == x[-1]


def test_svd_apply_mask_is_bit_identical_to_truncated_svd(bb):
    check_svd_apply_mask(bb, bb.to_numpy)


@pytest.mark.parametrize('n', [1, 2, 0.5, np.inf])
def test_entropy_on_the_device(bb, n):
    _, _, _, _, S, _, _ = svd_tensors(bb)
    s = S.to_numpy(bb)
    p = ab.DiagonalTensor.from_numpy(bb, S.leg, s ** 2 / np.sum(s ** 2))
    want = ref.ref_entropy(s ** 2 / np.sum(s ** 2), n)
    got = ab.entropy(bb, p, n)
    print(f'entropy n={n}: {got!r} vs {want!r}, relative difference {abs(got - want) / abs(want):.2e}')
    assert abs(got - want) <= 1e-12 * abs(want)


# ------------------------------------------------------------------------------------------- launch structure

def test_call_counts(bb, counted):
    lib, downloads, uploads = counted
    _, _, _, U_t, S, Vh, _ = svd_tensors(bb)
    nsec = S.leg.nsec
    assert nsec == len(S.blocks) > 8
    s = S.to_numpy(bb)
    p = ab.DiagonalTensor.from_numpy(bb, S.leg, s ** 2 / np.sum(s ** 2))
    half = ab.DiagonalTensor(S.symmetry, S.leg, S.blocks[::2], S.block_inds[::2])

    def fresh():
        lib.calls.clear()
        del downloads[:], uploads[:]

    fresh()
    ab.diagonal_binary(bb, S, half, 'add', False)                     # missing sectors: the absent kind, no zero block, no memset
    assert _calls(lib) == {'cyb_seg_binary': 1} and downloads == [] and uploads == []
    fresh()
    ab.reduce_diagonal(bb, half, 'max')
    assert _calls(lib) == {'cyb_seg_reduce': 1} and downloads == [16 * nsec] and uploads == []
    for n in (1, 2.0, np.inf):
        fresh()
        ab.entropy(bb, p, n)
        assert _calls(lib) == {'cyb_seg_reduce': 1} and downloads == [16 * nsec] and uploads == []
    fresh()
    flags = ab.diagonal_compare(bb, S, 'ge', float(np.median(s)))
    assert _calls(lib) == {'cyb_seg_binary': 1} and downloads == [] and uploads == []
    fresh()
    mask = ab.diagonal_to_mask(bb, flags)
    assert _calls(lib) == {'cyb_seg_compact': 1} and downloads == [8 * nsec] and uploads == []
    fresh()
    ab.mask_binary(bb, mask, ab.mask_unary(bb, mask), 'or')
    assert _calls(lib) == {'cyb_seg_binary': 2, 'cyb_seg_compact': 2} and downloads == [8 * nsec] * 2 and uploads == []    # (unary + binary)
    fresh()
    ab.mask_binary(bb, mask, mask, 'and')
    assert _calls(lib) == {'cyb_seg_binary': 1, 'cyb_seg_compact': 1} and downloads == [8 * nsec] and uploads == []
    fresh()
    ab.svd_apply_mask(bb, U_t, S, Vh, mask)
    calls = _calls(lib)
    assert calls.get('cyb_mask_gather_batched_f64') == 1 and 'cyb_memcpy_h2d' not in calls and uploads == [] and downloads == []
    assert set(calls) <= {'cyb_mask_gather_batched_f64', 'cyb_copy_strided_batched'}, calls
    fresh()
    small = ab.mask_contract(bb, Vh, mask, 0)
    ab.mask_contract(bb, small, mask, 0, large_leg=False)             # the scatter reads the device tables too
    calls = _calls(lib)
    assert calls.get('cyb_mask_scatter_batched_f64') == 1 and uploads == [] and downloads == []
