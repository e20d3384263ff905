"""Device side of the fusion-tree tensor operations: the cases of tests/test_tree_ops.py through HipBlockBackend (same
inputs, same criteria), the grouped tree-axis kernel (csrc/tree_axis.hip) at the C-ABI on blocks between guard bands
against an element-by-element numpy model, the weighted reduction against math.fsum, and the error paths."""
import ctypes as C
import math

import numpy as np
import pytest

import tree_ops_cases as cases
from cyten_amd import _lib
from cyten_amd.block_backend import DeviceIndex
from cyten_amd.fusion_tree import TreeAxisRecord

pytestmark = pytest.mark.gpu

SCALE, GATHER, SCATTER = 0, 1, 2
SENTINEL = -777.25
GUARD = 8


# ---------------------------------------------------------------------------------------------------------------------------
# cases 1-4 on the device

@pytest.mark.parametrize('cplx,cplx_diag', [(False, False), (True, False), (False, True), (True, True)])
def test_device_scale_axis_is_the_dense_product_along_every_leg_of_abelian_trees(bb, rng, cplx, cplx_diag):
    """bit-exact where an element is one product (a real operand on either side).  Two complex operands: the reference here
    is numpy's own complex product, whose evaluation (fused or not) is not specified, while the kernel rounds every product on
    its own; a component p1 +- p2 carries at most 2u (|p1| + |p2|), u = 2^-53, either way, so the two differ by at most
    2^-51 (|p1| + |p2|) <= 2^-51 times the largest entry of the result's operands.  The kernel's own arithmetic is checked bit
    for bit at the C-ABI below against a model with separately rounded products."""
    cases.check_abelian_scale_axis(bb, rng, cplx, cplx_diag, tol=2.0 ** -51 if cplx and cplx_diag else None)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_mask_contract_is_np_compress_along_every_leg_of_abelian_trees_and_its_inverse(bb, rng, cplx):
    cases.check_abelian_mask_contract(bb, rng, cplx)


@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('cplx', [False, True])
def test_device_forest_with_several_trees_is_treated_per_tree_block(bb, rng, side, cplx):
    cases.check_forest(bb, rng, side, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_vector_space_operations_match_the_restatements(bb, rng, cplx):
    cases.check_vector_ops(bb, rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_truncated_svd_projects_onto_the_kept_singular_vectors(bb, rng, cplx):
    cases.check_truncated_svd(bb, rng, cplx)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

class Arena:
    """a host image of one device buffer: blocks are carved out between guard bands of SENTINEL"""

    def __init__(self, cplx):
        self.dtype = np.complex128 if cplx else np.float64
        self.size = GUARD
        self.blocks = []

    def block(self, n):
        off = self.size
        self.blocks.append((off, n))
        self.size += n + GUARD + (n + GUARD) % 2      # blocks start at even offsets: 16-byte aligned where the row offset is even
        return off

    def host(self, rng=None):
        img = np.full(self.size, SENTINEL, dtype=self.dtype)
        if rng is not None:
            for off, n in self.blocks:
                img[off:off + n] = rng.standard_normal(n) + (1j * rng.standard_normal(n) if self.dtype == np.complex128 else 0)
        return img


def _upload(bb, img):
    buf = bb.ctx.empty(len(img), 'complex128' if img.dtype == np.complex128 else ('int64' if img.dtype == np.int64 else 'float64'))
    bb.ctx.h2d(buf, img)
    return buf


def _download(bb, buf, like):
    return bb.ctx.d2h(buf, len(like), like.dtype)


def _cmul(v, f):
    """complex product with every product and sum rounded on its own (no fused multiply-add), factor with zero imaginary part
    applied per component"""
    v, f = np.asarray(v, dtype=np.complex128), np.asarray(f, dtype=np.complex128)
    re = np.where(f.imag == 0, v.real * f.real, v.real * f.real - v.imag * f.imag)
    im = np.where(f.imag == 0, v.imag * f.real, v.real * f.imag + v.imag * f.real)
    return re + 1j * im


def _model(rec, src, dst, table, cplx):
    """apply one record (dict with element offsets into the host images) to `dst`, one element at a time"""
    mode, A, Ad = rec['mode'], rec['A'], rec['A_dst']
    Ai = Ad if mode == GATHER else A
    o, a, i, x = [g.ravel() for g in np.meshgrid(np.arange(rec['outer']), np.arange(Ai), np.arange(rec['inner']), np.arange(rec['X']), indexing='ij')]
    if mode == SCALE:
        ts = td = (o * A + a) * rec['inner'] + i
    elif mode == GATHER:
        ts, td = (o * A + table[a]) * rec['inner'] + i, (o * Ad + a) * rec['inner'] + i
    else:
        ts, td = (o * A + a) * rec['inner'] + i, (o * Ad + table[a]) * rec['inner'] + i
    v = src[rec['src_off'] + (rec['src_start'] + ts) * rec['src_ts'] + x * rec['src_xs']]
    at = rec['dst_off'] + (rec['dst_start'] + td) * rec['dst_ts'] + x * rec['dst_xs']
    if mode == SCALE:
        v = _cmul(v, table[a]) if cplx else v * table[a]
    dst[at] = v


def _layout(arena, start, T, X, major, ld_odd):
    """(offset, tree stride, x stride, elements) of a block holding the tree rows [start, start + T) and one spare row behind"""
    rows = start + T + 1
    if major == 'row':
        ld = X + 2 + ((X + 2) % 2 != ld_odd)
        n = rows * ld
        return arena.block(n), ld, 1, n
    ld = rows + 1 + ((rows + 1) % 2 != ld_odd)
    n = X * ld
    return arena.block(n), 1, ld, n


def _run(bb, recs, tables, cplx, rng, fills=(), real_src=()):
    """build the images of a record list (dicts with shapes and layouts), launch ONCE, compare every byte of the destination
    image (blocks and guard bands) with the model, and the source image with itself.  Bit for bit: a float64 element is one
    product, and the kernel rounds the four products of a complex one separately (`_cmul` does the same)."""
    src_a, dst_a, rsrc_a = Arena(cplx), Arena(cplx), Arena(False)
    for k, r in enumerate(recs):
        Ts, Td = r['outer'] * r['A'] * r['inner'], r['outer'] * r['A_dst'] * r['inner']
        arena = rsrc_a if k in real_src else src_a
        r['src_off'], r['src_ts'], r['src_xs'], _ = _layout(arena, r['src_start'], Ts, r['X'], r['src_major'], r['ld_odd'])
        r['dst_off'], r['dst_ts'], r['dst_xs'], r['dst_n'] = _layout(dst_a, r['dst_start'], Td, r['X'], r['dst_major'], r['ld_odd'])
    src, rsrc, dst = src_a.host(rng), rsrc_a.host(rng), dst_a.host()
    tab_dtype = np.int64 if recs and recs[0]['mode'] != SCALE else None
    d_src, d_rsrc, d_dst = _upload(bb, src), _upload(bb, rsrc), _upload(bb, dst)
    # tables: int64 positions in one device array; factors in a real and a complex device array
    if tab_dtype is not None:
        flat = np.concatenate([np.asarray(t, dtype=np.int64) for t in tables] + [np.zeros(1, np.int64)])
        d_tab = _upload(bb, flat)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in tables])])
        tab_ptr = [d_tab.data_ptr() + 8 * int(o) for o in offs[:-1]]
        tab_cplx = [0] * len(recs)
    else:
        rt = np.concatenate([np.real(t) for t in tables] + [np.zeros(1)])
        ct = np.concatenate([np.asarray(t, dtype=np.complex128) for t in tables] + [np.zeros(1, np.complex128)])
        d_rt, d_ct = _upload(bb, rt), _upload(bb, ct)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in tables])])
        tab_cplx = [1 if np.iscomplexobj(t) else 0 for t in tables]
        tab_ptr = [(d_ct.data_ptr() + 16 * int(o)) if c else (d_rt.data_ptr() + 8 * int(o)) for o, c in zip(offs[:-1], tab_cplx)]
    es = 16 if cplx else 8
    arr = (_lib.TreeAxisRec * max(len(recs), 1))()
    for k, r in enumerate(recs):
        real = k in real_src
        arr[k].src = (d_rsrc.data_ptr() + 8 * r['src_off']) if real else (d_src.data_ptr() + es * r['src_off'])
        arr[k].dst = d_dst.data_ptr() + es * r['dst_off']
        arr[k].table = tab_ptr[k]
        arr[k].src_ts, arr[k].src_xs, arr[k].dst_ts, arr[k].dst_xs = r['src_ts'], r['src_xs'], r['dst_ts'], r['dst_xs']
        arr[k].src_start, arr[k].dst_start, arr[k].X = r['src_start'], r['dst_start'], r['X']
        arr[k].outer, arr[k].A, arr[k].A_dst, arr[k].inner = r['outer'], r['A'], r['A_dst'], r['inner']
        arr[k].mode, arr[k].src_is_real, arr[k].table_is_complex = r['mode'], 1 if real else 0, tab_cplx[k]
    fl = (_lib.TreeFill * max(len(fills), 1))()
    want = dst.copy()
    for n, k in enumerate(fills):
        fl[n].ptr, fl[n].bytes = d_dst.data_ptr() + es * recs[k]['dst_off'], es * recs[k]['dst_n']
        want[recs[k]['dst_off']:recs[k]['dst_off'] + recs[k]['dst_n']] = 0
    for k, r in enumerate(recs):
        loc = dict(r)
        if k in real_src:
            _model(loc, rsrc, want, tables[k], cplx)
        else:
            _model(loc, src, want, tables[k], cplx)
    fn = bb.lib.cyb_tree_axis_c128 if cplx else bb.lib.cyb_tree_axis_f64
    bb.ctx.sync_stream()
    _lib.check(fn(bb.ctx.handle, arr, len(recs), fl, len(fills)))
    got = _download(bb, d_dst, dst)
    assert np.array_equal(got, want), f'{int((got != want).sum())} elements differ'
    assert np.array_equal(_download(bb, d_src, src), src) and np.array_equal(_download(bb, d_rsrc, rsrc), rsrc)


# (outer, A, inner) of the tree extents 1, 3, 64, 65 and 257: inner = 1, odd and even
SPLITS = [(1, 1, 1), (1, 3, 1), (1, 1, 3), (4, 16, 1), (2, 8, 4), (1, 2, 32), (5, 13, 1), (1, 13, 5), (1, 257, 1), (1, 1, 257)]
EXTENTS_X = [1, 2, 63, 130]


def _edge_records(rng, mode, src_major, dst_major, ld_odd):
    recs, tables = [], []
    for outer, A, inner in SPLITS:
        for X in EXTENTS_X:
            small = (A + 1) // 2
            keep = np.sort(rng.choice(A, size=small, replace=False))
            a_src, a_dst = (A, A) if mode == SCALE else ((A, small) if mode == GATHER else (small, A))
            recs.append(dict(mode=mode, outer=outer, A=a_src, A_dst=a_dst, inner=inner, X=X, src_start=int(rng.integers(0, 4)),
                             dst_start=int(rng.integers(0, 4)), src_major=src_major, dst_major=dst_major, ld_odd=ld_odd))
            tables.append(rng.standard_normal(A) if mode == SCALE else keep)
    return recs, tables


@pytest.mark.parametrize('ld_odd', [False, True])
@pytest.mark.parametrize('majors', [('row', 'row'), ('col', 'col'), ('col', 'row')])
@pytest.mark.parametrize('mode', [SCALE, GATHER, SCATTER])
def test_kernel_edges_f64(bb, rng, mode, majors, ld_odd):
    """tree extents 1 / 3 / 64 / 65 / 257 against X = 1 / 2 / 63 / 130 in one launch: both lane directions, the run and the
    per-element paths, rows that are 16-byte aligned on both sides, on one side, on none"""
    recs, tables = _edge_records(rng, mode, majors[0], majors[1], ld_odd)
    _run(bb, recs, tables, False, rng, fills=range(len(recs)) if mode == SCATTER else ())


@pytest.mark.parametrize('majors', [('row', 'row'), ('col', 'col'), ('col', 'row')])
@pytest.mark.parametrize('mode', [SCALE, GATHER, SCATTER])
def test_kernel_edges_c128(bb, rng, mode, majors):
    """interleaved complex data; every third record reads a float64 source in place, scale records alternate between real
    and complex factors"""
    recs, tables = _edge_records(rng, mode, majors[0], majors[1], True)
    if mode == SCALE:
        tables = [t + 1j * rng.standard_normal(len(t)) if k % 2 == 0 else t for k, t in enumerate(tables)]
    _run(bb, recs, tables, True, rng, fills=range(len(recs)) if mode == SCATTER else (), real_src=set(range(0, len(recs), 3)))


def test_kernel_empty_lists_and_empty_records(bb, rng):
    assert bb.lib.cyb_tree_axis_f64(bb.ctx.handle, None, 0, None, 0) == _lib.CYB_OK
    assert bb.lib.cyb_tree_axis_c128(bb.ctx.handle, None, 0, None, 0) == _lib.CYB_OK
    recs = [dict(mode=GATHER, outer=3, A=5, A_dst=0, inner=2, X=7, src_start=1, dst_start=0, src_major='row', dst_major='row', ld_odd=True),
            dict(mode=GATHER, outer=3, A=5, A_dst=2, inner=2, X=7, src_start=1, dst_start=2, src_major='row', dst_major='row', ld_odd=True),
            dict(mode=GATHER, outer=3, A=5, A_dst=2, inner=2, X=0, src_start=0, dst_start=0, src_major='col', dst_major='col', ld_odd=True)]
    _run(bb, recs, [np.zeros(0, np.int64), np.array([1, 4]), np.array([0, 3])], False, rng)


@pytest.mark.parametrize('major', ['row', 'col'])
def test_kernel_one_record_cut_into_many_work_items(bb, rng, major):
    """1100 x 1030 doubles: the work-item boundaries fall inside rows"""
    for mode in (SCALE, GATHER):
        a_dst = 50 if mode == SCALE else 31
        recs = [dict(mode=mode, outer=2, A=50, A_dst=a_dst, inner=11, X=1030, src_start=0, dst_start=1, src_major=major, dst_major=major,
                     ld_odd=True)]
        table = rng.standard_normal(50) if mode == SCALE else np.sort(rng.choice(50, size=31, replace=False))
        _run(bb, recs, [table], False, rng)


@pytest.mark.parametrize('major', ['row', 'col'])
def test_kernel_runs_longer_than_a_work_item(bb, rng, major):
    """contiguous runs of 2048 elements and more are shared by the four waves of a workgroup, and a run of more than 8192
    elements spans several work items: X = 9000 in row-major blocks; in column-major ones the whole tree extent 9150 (scale)
    and inner = 2100 (gather)"""
    for mode in (SCALE, GATHER):
        if major == 'row':
            shape = dict(outer=1, A=5, A_dst=5 if mode == SCALE else 3, inner=1, X=9000)
        elif mode == SCALE:
            shape = dict(outer=3, A=50, A_dst=50, inner=61, X=7)
        else:
            shape = dict(outer=1, A=5, A_dst=3, inner=2100, X=3)
        recs = [dict(mode=mode, src_start=1, dst_start=0, src_major=major, dst_major=major, ld_odd=True, **shape)]
        table = rng.standard_normal(shape['A']) if mode == SCALE else np.sort(rng.choice(shape['A'], size=shape['A_dst'], replace=False))
        _run(bb, recs, [table], False, rng)
        _run(bb, [dict(r) for r in recs], [table + 1j * rng.standard_normal(len(table)) if mode == SCALE else table], True, rng)


def test_kernel_many_tiny_records(bb, rng):
    """1500 records of at most 12 elements each in one launch"""
    shapes = [(o, a, i, x) for o in (1, 2, 3) for a in (1, 2, 3, 4) for i in (1, 2, 3) for x in (1, 2, 3, 4) if o * a * i * x <= 12]
    recs, tables = [], []
    for k in range(1500):
        o, a, i, x = shapes[int(rng.integers(len(shapes)))]
        small = int(rng.integers(0, a + 1))
        major = ('row', 'col')[k % 2]
        recs.append(dict(mode=GATHER, outer=o, A=a, A_dst=small, inner=i, X=x, src_start=int(rng.integers(0, 3)), dst_start=int(rng.integers(0, 3)),
                         src_major=major, dst_major=('row', 'col')[(k // 2) % 2], ld_odd=bool(k % 3)))
        tables.append(np.sort(rng.choice(a, size=small, replace=False)))
    _run(bb, recs, tables, False, rng)


def test_backend_call_takes_device_and_host_tables_in_one_launch(bb, rng):
    src = rng.standard_normal((3 * 6 * 2 + 5, 9))
    keep_a, keep_b = np.array([0, 2, 5]), np.array([1, 4])
    d_src = bb.as_block(src)
    dev_tab = bb.ctx.empty(3, 'int64')
    bb.ctx.h2d(dev_tab, keep_a.astype(np.int64))
    outs = bb.empty_many([(3 * 3 * 2, 9), (3 * 2 * 2 + 1, 9)])
    recs = [TreeAxisRecord(d_src, outs[0], 0, 5, 0, 3, 6, 3, 2, DeviceIndex(dev_tab.data_ptr(), 3, dev_tab)),
            TreeAxisRecord(d_src, outs[1], 0, 5, 1, 3, 6, 2, 2, keep_b)]
    bb.tree_axis_many(recs, 'gather', fill=[outs[1]])
    t = src[5:].reshape(3, 6, 2, 9)
    assert np.array_equal(bb.to_numpy(outs[0]), t[:, keep_a].reshape(-1, 9))
    got = bb.to_numpy(outs[1])
    assert np.array_equal(got[1:], t[:, keep_b].reshape(-1, 9)) and np.all(got[0] == 0)
    with pytest.raises(ValueError):
        bb.tree_axis_many([TreeAxisRecord(d_src, outs[1], 0, 5, 1, 3, 6, 2, 2, np.array([1, 6]))], 'gather')    # position outside the leg
    with pytest.raises(ValueError):
        bb.tree_axis_many([TreeAxisRecord(d_src, outs[1], 0, 6, 1, 3, 6, 2, 2, keep_b)], 'gather')               # beyond the block


# ---------------------------------------------------------------------------------------------------------------------------
# weighted reduction

SHAPES = [(1, 1), (15, 17), (16, 16), (257, 1), (1, 70001)]          # 1, 255, 256, 257 and 70 001 elements
WEIGHTS = [1.0, 2.0, 3.0, 1.0, 2.0]


def _pairs(rng, cplx):
    xs, ys = [], []
    for sh in SHAPES:
        x = rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0)
        xs.append(x)
        ys.append(x + 0.5 * (rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0)))     # <x, y> of the order of |x|^2
    return xs, ys


def _fsum(vals):
    return complex(math.fsum(np.real(v) for v in vals), math.fsum(np.imag(v) for v in vals))


@pytest.mark.parametrize('cplx', [False, True])
def test_weighted_reduction_against_fsum(bb, rng, cplx):
    xs, ys = _pairs(rng, cplx)
    dx, dy = [bb.as_block(x) for x in xs], [bb.as_block(y) for y in ys]
    dyt = [bb.as_block(np.ascontiguousarray(y.T)) for y in ys]
    want = _fsum([w * np.sum(np.conj(x) * y) for x, y, w in zip(xs, ys, WEIGHTS)])
    got = bb.inner_weighted_many(dx, dy, WEIGHTS, do_dagger=True)
    assert abs(got - want) <= 1e-13 * abs(want)
    assert bb.inner_weighted_many(dx, dy, WEIGHTS, do_dagger=True) == got                 # bit-identical from run to run
    want_t = _fsum([w * np.sum(x * y) for x, y, w in zip(xs, ys, WEIGHTS)])             # a[i, j] b[j, i] with b = y^T, no conjugation
    got_t = bb.inner_weighted_many(dx, dyt, WEIGHTS, do_dagger=False)
    assert abs(got_t - want_t) <= 1e-13 * abs(want_t)
    assert bb.inner_weighted_many(dx, dyt, WEIGHTS, do_dagger=False) == got_t
    # the same through transposed views (strides, not copies)
    assert bb.inner_weighted_many(dx, [bb.permute_axes(y, [1, 0]) for y in dy], WEIGHTS, do_dagger=False) == got_t
    want_n = math.fsum(w * float(np.sum(np.abs(x) ** 2)) for x, w in zip(xs, WEIGHTS))
    got_n = bb.inner_weighted_many(dx, None, WEIGHTS)
    assert isinstance(got_n, float) and abs(got_n - want_n) <= 1e-13 * want_n
    assert bb.inner_weighted_many(dx, None, WEIGHTS) == got_n
    assert bb.inner_weighted_many([], [], []) == 0.0


@pytest.mark.parametrize('cplx', [False, True])
def test_weighted_trace_of_a_view_into_a_larger_block(bb, rng, cplx):
    big = rng.standard_normal((120, 131)) + (1j * rng.standard_normal((120, 131)) if cplx else 0)
    view = bb.get_item(bb.as_block(big), (slice(3, 100), slice(5, 102)))
    small = rng.standard_normal((4, 4))
    want = _fsum([2.0 * np.trace(big[3:100, 5:102]), 3.0 * np.trace(small)])
    got = bb.trace_weighted_many([view, bb.as_block(small)], [2.0, 3.0])
    assert abs(got - want) <= 1e-13 * abs(want)
    assert bb.trace_weighted_many([view, bb.as_block(small)], [2.0, 3.0]) == got


# ---------------------------------------------------------------------------------------------------------------------------
# error paths

def test_invalid_records_are_refused_before_anything_is_launched(bb, rng):
    src = bb.as_block(rng.standard_normal((12, 6)))
    dst = bb.as_block(np.full((12, 6), SENTINEL))
    tab = bb.ctx.empty(4, 'int64')
    bb.ctx.h2d(tab, np.array([0, 1, 2, 3], dtype=np.int64))
    arr = (_lib.TreeAxisRec * 2)()
    fill = (_lib.TreeFill * 1)()

    def good():
        for k in range(2):
            arr[k].src, arr[k].dst, arr[k].table = src.ptr, dst.ptr + 8 * 36 * k, tab.data_ptr()
            arr[k].src_ts, arr[k].src_xs, arr[k].dst_ts, arr[k].dst_xs = 6, 1, 6, 1
            arr[k].src_start, arr[k].dst_start, arr[k].X = 0, 0, 6
            arr[k].outer, arr[k].A, arr[k].A_dst, arr[k].inner = 1, 6, 4, 1
            arr[k].mode, arr[k].src_is_real, arr[k].table_is_complex = GATHER, 0, 0
        fill[0].ptr, fill[0].bytes = dst.ptr, 8 * 72

    for mutate, frag in [
        (lambda: setattr(arr[1], 'src', None), 'src is NULL'),
        (lambda: setattr(arr[1], 'dst', None), 'dst is NULL'),
        (lambda: setattr(arr[1], 'table', None), 'table is NULL'),
        (lambda: setattr(arr[1], 'X', -1), 'negative extent'),
        (lambda: setattr(arr[1], 'inner', -3), 'negative extent'),
        (lambda: setattr(arr[1], 'A_dst', 7), "A' <= A"),
        (lambda: setattr(arr[1], 'mode', 5), 'unknown mode'),
        (lambda: setattr(fill[0], 'bytes', -8), 'negative size'),
    ]:
        good()
        mutate()
        for fn in (bb.lib.cyb_tree_axis_f64, bb.lib.cyb_tree_axis_c128):
            st = fn(bb.ctx.handle, arr, 2, fill, 1)
            assert st == _lib.CYB_ERR_INVALID and frag in bb.lib.cyb_last_error().decode()
            with pytest.raises(ValueError):
                _lib.check(st)
    # neither the valid first record nor the fill has touched the destination
    assert np.all(bb.to_numpy(dst) == SENTINEL)
    good()
    _lib.check(bb.lib.cyb_tree_axis_f64(bb.ctx.handle, arr, 2, None, 0))
    assert np.array_equal(bb.to_numpy(dst)[:4], bb.to_numpy(src)[:4]) and np.array_equal(bb.to_numpy(dst)[6:10], bb.to_numpy(src)[:4])

    d = (_lib.WDotDesc * 1)()
    res = bb.ctx.empty(2)
    d[0].x, d[0].y, d[0].rows, d[0].cols, d[0].x_rs, d[0].x_cs, d[0].w = None, None, 3, 2, 2, 1, 1.0
    assert bb.lib.cyb_dot_weighted_f64(bb.ctx.handle, d, 1, C.c_void_p(res.data_ptr())) == _lib.CYB_ERR_INVALID
    d[0].x, d[0].rows = src.ptr, -3
    assert bb.lib.cyb_dot_weighted_c128(bb.ctx.handle, d, 1, 1, C.c_void_p(res.data_ptr())) == _lib.CYB_ERR_INVALID
    assert bb.lib.cyb_dot_weighted_f64(bb.ctx.handle, d, 1, None) == _lib.CYB_ERR_INVALID
