"""The packers of cyten_amd.tree_records on the host: no device anywhere.  Views are HipBlocks over CPU torch buffers.

Three things are checked.  Argument checks: the CPU twins of the ``pytest.raises`` cases of tests/test_gpu_tree_*.py that the
Python layer raises (same shapes, same ``match``).  Reach: for every record a packer emits, the lowest and highest byte its
fields let the kernel touch in every buffer it names (base pointer, extents, strides and the ``*_real`` flags, in the meaning
of include/cyten_amd.h) lie between the first and the last element of the view that was passed, inside the torch buffer it
was cut from; where a record stands for a whole view, tree block, strip, tile or region, they are exactly its first and last
byte, computed from the arguments.  Books: the term ranges tile the term list in order, padded slots are zero, and the float64
entry carries no ``*_real`` flag and no imaginary coefficient.  Addresses are checked, not values: values stay with the GPU
tests.
"""
import numpy as np
import pytest
import torch

from cyten_amd import _lib
from cyten_amd import tree_records as tr
from cyten_amd.block_backend import HipBlock
from cyten_amd.fusion_tree import TreeAxisRecord


# ---------------------------------------------------------------------------------------------------------------------------
# views over CPU buffers

def blk(*shape, c=False, dtype=None):
    """a contiguous block in a buffer of its own"""
    n = int(np.prod(shape, dtype=np.int64))
    buf = torch.zeros(max(n, 1), dtype=dtype or (torch.complex128 if c else torch.float64))
    return HipBlock(None, buf, 0, shape, tr.c_strides(tuple(shape)))


def transposed(v, axes=None):
    axes = list(range(v.ndim))[::-1] if axes is None else axes
    return HipBlock(None, v.buf, v.offset, [v.shape[a] for a in axes], [v.strides[a] for a in axes])


def window(v, *ranges):
    """the view ``v[a0:b0:s0, a1:b1:s1, ..]`` (a < b; a negative step walks the same elements from the last one down)"""
    off, shape, strides = v.offset, [], []
    for (a, b, s), st in zip(ranges, v.strides):
        n = len(range(a, b, abs(s)))
        off += (a if s > 0 or not n else a + (n - 1) * abs(s)) * st
        shape.append(n)
        strides.append(s * st)
    return HipBlock(None, v.buf, off, shape, strides)


def tile(shape, c=False, at=None, room=None):
    """a view of `shape` with an offset inside a larger block (`room` per axis, default shape + 3; `at`, default 1 per axis)"""
    room = room or [s + 3 for s in shape]
    at = at or [1] * len(shape)
    return window(blk(*room, c=c), *[(a, a + s, 1) for a, s in zip(at, shape)])


class Uploads:
    """the `upload` argument of a packer: keeps the host array and hands out its address"""

    def __init__(self):
        self.kept = []

    def __call__(self, host):
        host = np.ascontiguousarray(host)
        self.kept.append(host)
        return host.ctypes.data, host

    def holds(self, lo, hi):
        return any(h.ctypes.data <= lo and hi <= h.ctypes.data + h.nbytes for h in self.kept)


# ---------------------------------------------------------------------------------------------------------------------------
# reach: what the fields of a record let the kernel touch

def span(ptr, es, levels, first=0):
    """[lo, hi) in bytes of the elements ``ptr + es * (first + sum_l x_l * stride_l)``, x_l < extent_l; None if there is none"""
    levels = [(int(e), int(s)) for e, s in levels]
    if any(e <= 0 for e, _ in levels):
        return None
    lo = first + sum(min(0, (e - 1) * s) for e, s in levels)
    hi = first + sum(max(0, (e - 1) * s) for e, s in levels)
    return int(ptr) + es * lo, int(ptr) + es * (hi + 1)


def inside(rng, view):
    """`rng` lies between the first and the last byte of the view's own elements, and those inside the view's buffer"""
    own = span(view.ptr, view.buf.element_size(), zip(view.shape, view.strides))
    lo, hi = view.buf.data_ptr(), view.buf.data_ptr() + view.buf.numel() * view.buf.element_size()
    assert own is None or lo <= own[0] and own[1] <= hi
    return rng is None or (own is not None and own[0] <= rng[0] and rng[1] <= own[1])


def covers(rng, view, first=0, shape=None):
    """`rng` is exactly what the view's own elements span (or its region of `shape` whose first element is `first`)"""
    own = span(view.ptr, view.buf.element_size(), zip(view.shape if shape is None else shape, view.strides), first)
    return inside(own, view) and rng == own


def es_of(cplx, real_flag=0):
    return 16 if cplx and not real_flag else 8


def arrays(launch):
    return [arr[:n] for arr, _, n in launch.arrays]


def check_books(launch, outs, terms, real_fields):
    """term ranges tile the term list in order; the float64 entry has neither ``*_real`` flags nor imaginary coefficients"""
    nxt = 0
    for o in outs:
        assert o['first_term'] == nxt and o['n_terms'] >= 0
        nxt += int(o['n_terms'])
    assert nxt == len(terms)
    for arr, struct, n in launch.arrays:
        assert arr.dtype == np.dtype(struct) and len(arr) == max(n, 1)
    if not launch.cplx:
        for t in terms:
            assert all(t[f] == 0 for f in real_fields)
            assert 'coeff_im' not in t.dtype.names or t['coeff_im'] == 0


def zero_beyond(rec, used, *fields):
    assert all(not np.any(rec[f][used:]) for f in fields)


def tree_block(view, side, start, extent):
    """`first` and `shape` (for `covers`) of the tree block of `extent` positions from `start` on, on the side's axis of a view"""
    ax = side if view.ndim == 2 else 0
    return start * view.strides[ax], [extent if a == ax else n for a, n in enumerate(view.shape)]


def reach_axis(args, up):
    records, mode, fill = args[0], args[1], (args[2] if len(args) > 2 else ())
    launch = tr.pack_axis(*args, upload=up)
    if launch is None:
        assert not records and not fill
        return
    recs, fills = arrays(launch)
    assert launch.stem == 'cyb_tree_axis' and len(recs) == len(records) and len(fills) == len(fill)
    for rec, r in zip(recs, records):
        assert rec['mode'] == _lib.TREE_AXIS_MODES[mode] and rec['reserved'] == 0
        assert launch.cplx or r.src.is_complex is False
        src_es = 8 if rec['src_is_real'] or not launch.cplx else 16
        assert (src_es == 16) == r.src.is_complex
        t_src, t_dst = rec['outer'] * rec['A'] * rec['inner'], rec['outer'] * rec['A_dst'] * rec['inner']
        assert (t_src, t_dst) == (r.outer * r.A * r.inner, r.outer * r.A_dst * r.inner)
        assert covers(span(rec['src'], src_es, [(t_src, rec['src_ts']), (rec['X'], rec['src_xs'])], rec['src_start'] * rec['src_ts']),
                      r.src, *tree_block(r.src, r.side, r.src_start, t_src))
        assert covers(span(rec['dst'], es_of(launch.cplx), [(t_dst, rec['dst_ts']), (rec['X'], rec['dst_xs'])], rec['dst_start'] * rec['dst_ts']),
                      r.dst, *tree_block(r.dst, r.side, r.dst_start, t_dst))
        if mode == 'scale':
            assert inside(span(rec['table'], 16 if rec['table_is_complex'] else 8, [(rec['A'], 1)]), r.table)
        else:
            n_tab = rec['A_dst'] if mode == 'gather' else rec['A']
            rng = span(rec['table'], 8, [(n_tab, 1)])
            if isinstance(r.table, tr.DeviceIndex):
                assert rng is None or (r.table.ptr, r.table.ptr + 8 * r.table.n) == rng
            else:
                assert rng is None or up.holds(*rng)
    for f, b in zip(fills, fill):
        assert f['bytes'] == 0 or inside((int(f['ptr']), int(f['ptr']) + int(f['bytes'])), b)


def reach_trace(outputs):
    launch = tr.pack_trace(outputs)
    outs, terms = arrays(launch)
    assert launch.stem == 'cyb_trace_weighted'
    check_books(launch, outs, terms, ['src_real'])
    srcs = [tm[0] for _, tms in outputs for tm in tms]
    for o, (dst, tms) in zip(outs, outputs):
        nd = int(o['ndim'])
        assert nd == dst.ndim
        zero_beyond(o, nd, 'shape', 'dst_strides')
        assert covers(span(o['dst'], es_of(launch.cplx), zip(o['shape'][:nd], o['dst_strides'][:nd])), dst)
        for t, a in zip(terms[o['first_term']:o['first_term'] + o['n_terms']], srcs[o['first_term']:]):
            npair = int(t['n_pairs'])
            zero_beyond(t, nd, 'rem_strides')
            zero_beyond(t, npair, 'pair_extent', 'pair_stride')
            levels = list(zip(o['shape'][:nd], t['rem_strides'][:nd])) + list(zip(t['pair_extent'][:npair], t['pair_stride'][:npair]))
            assert covers(span(t['src'], es_of(launch.cplx, t['src_real']), levels), a)
            assert bool(t['src_real']) == (launch.cplx and not a.is_complex)


def reach_outer(outputs):
    launch = tr.pack_outer(outputs)
    outs, terms = arrays(launch)
    assert launch.stem == 'cyb_outer_weighted'
    check_books(launch, outs, terms, ['a_real', 'b_real'])
    flat = [tm for _, tms in outputs for tm in tms]
    for o, (dst, tms) in zip(outs, outputs):
        assert covers(span(o['dst'], es_of(launch.cplx), [(o['ha'] * o['hb'], o['ldd']), (o['wa'] * o['wb'], 1)]), dst)
        assert (o['ha'] * o['hb'], o['wa'] * o['wb']) == dst.shape
        for t, (a, b, _) in zip(terms[o['first_term']:o['first_term'] + o['n_terms']], flat[o['first_term']:]):
            assert covers(span(t['a'], es_of(launch.cplx, t['a_real']), [(o['ha'], t['a_rs']), (o['wa'], t['a_cs'])]), a)
            assert covers(span(t['b'], es_of(launch.cplx, t['b_real']), [(o['hb'], t['b_rs']), (o['wb'], t['b_cs'])]), b)


def reach_compose(outputs):
    launch = tr.pack_compose(outputs)
    outs, terms = arrays(launch)
    assert launch.stem == 'cyb_compose_weighted'
    check_books(launch, outs, terms, ['a_real', 'b_real'])
    flat = [tm for o in outputs for tm in o[4]]
    for o, (dst, side, m0, m2, tms) in zip(outs, outputs):
        ax = int(o['axis'])
        assert ax == (2 if side == 'domain' else 1) and o['reserved'] == 0
        assert covers(span(o['dst'], es_of(launch.cplx), zip(o['ext'], o['sd'])), dst)
        assert int(np.prod(o['ext'])) == dst.size
        for t, (a, b, _) in zip(terms[o['first_term']:o['first_term'] + o['n_terms']], flat[o['first_term']:]):
            a_levels = [(t['K'] if l == ax else o['ext'][l], t['sa'][l]) for l in range(4)]
            assert covers(span(t['a'], es_of(launch.cplx, t['a_real']), a_levels), a)
            assert inside(span(t['b'], es_of(launch.cplx, t['b_real']), [(o['ext'][ax], t['b_ns']), (t['K'], t['b_ks'])]), b)


def window_span(rec, es):
    return span(rec['dst'], es, [(rec['h'], rec['ldd']), (rec['nq'], rec['cp']), (rec['wn'], 1)])


def source_levels(rec):
    nr, nc = int(rec['n_row_levels']), int(rec['n_col_levels'])
    zero_beyond(rec, nr, 'rext', 'rs')
    zero_beyond(rec, nc, 'cext', 'cs')
    return list(zip(rec['rext'][:nr], rec['rs'][:nr])) + list(zip(rec['cext'][:nc], rec['cs'][:nc]))


def reach_place(records):
    launch = tr.pack_place(records)
    recs, = arrays(launch)
    assert launch.stem == 'cyb_tree_place' and len(recs) == len(records)
    for rec, (dst, src, n_row, coeff) in zip(recs, records):
        assert covers(window_span(rec, es_of(launch.cplx)), dst) and rec['h'] * rec['nq'] * rec['wn'] == dst.size
        assert rec['reserved'] == 0 and (launch.cplx or (rec['src_real'] == 0 and rec['coeff_im'] == 0))
        if src is None:
            assert rec['src'] == 0
            continue
        assert covers(span(rec['src'], es_of(launch.cplx, rec['src_real']), source_levels(rec)), src)
        assert complex(rec['coeff_re'], rec['coeff_im']) == complex(coeff)


def reach_strip(outs_arg):
    launch = tr.pack_strip(outs_arg)
    outs, terms = arrays(launch)
    assert launch.stem == 'cyb_tree_strip'
    check_books(launch, outs, terms, ['src_real'])
    flat = [tm for o in outs_arg for tm in o[6]]
    for o, (dst, side, start, stop, dims, axes, tms) in zip(outs, outs_arg):
        strip = [stop - start if ax == side else n for ax, n in enumerate(dst.shape)]
        assert covers(window_span(o, es_of(launch.cplx)), dst, start * dst.strides[side], strip)
        assert o['h'] * o['nq'] * o['wn'] == (stop - start) * dst.shape[1 - side]
        levels = source_levels(o)
        assert (o['n_row_levels'], o['n_col_levels']) == ((len(dims), 1) if side == 0 else (1, len(dims)))
        for t, (src, _, _) in zip(terms[o['first_term']:o['first_term'] + o['n_terms']], flat[o['first_term']:]):
            assert t['reserved'] == 0
            assert inside(span(t['src'], es_of(launch.cplx, t['src_real']), levels, int(t['base'])), src)


def reach_to_dense(dst_view, regions):
    up = Uploads()
    launch = tr.pack_to_dense(dst_view, regions, up)
    outs, terms = arrays(launch)
    assert launch.stem == 'cyb_tree_to_dense'
    check_books(launch, outs, terms, ['block_real', 's_real'])
    flat = [tm for r in regions for tm in r[4]]
    table, = launch.tail
    assert (table == 0) == (not up.kept) and len(up.kept) <= 1
    for o, (starts, dims, mults, J, tms) in zip(outs, regions):
        nl = int(o['n_levels'])
        assert nl == 2 * dst_view.ndim and o['reserved'] == 0
        zero_beyond(o, nl, 'ext', 'sd', 'ss', 'sr', 'sc')
        ext = o['ext'][:nl]
        region = [d * m for d, m in zip(dims, mults)]
        assert covers(span(o['dst'], es_of(launch.cplx), zip(ext, o['sd'][:nl])), dst_view, sum(x * st for x, st in zip(starts, dst_view.strides)), region)
        for t, (b, r0, c0, S) in zip(terms[o['first_term']:o['first_term'] + o['n_terms']], flat[o['first_term']:]):
            rows, cols = span(0, 1, zip(ext, o['sr'][:nl]), int(t['first_row'])), span(0, 1, zip(ext, o['sc'][:nl]), int(t['first_col']))
            if rows is None:
                continue
            H, W = int(np.prod(mults[:J], dtype=np.int64)), int(np.prod(mults[J:], dtype=np.int64))
            assert rows == (r0, r0 + H) and cols == (c0, c0 + W)               # the tile of the term, all of it and no more
            assert covers(span(t['block'], es_of(launch.cplx, t['block_real']), [(H, t['rs']), (W, t['cs'])], r0 * int(t['rs']) + c0 * int(t['cs'])),
                          b, r0 * b.strides[0] + c0 * b.strides[1], [H, W])
            assert up.holds(*span(table, es_of(launch.cplx, t['s_real']), zip(ext, o['ss'][:nl]), int(t['s_off'])))
            assert bool(t['s_real']) == (launch.cplx and not np.iscomplexobj(up.kept[0]))


def reach_from_dense(outputs):
    up = Uploads()
    launch = tr.pack_from_dense(outputs, up)
    outs, terms = arrays(launch)
    assert launch.stem == 'cyb_tree_from_dense'
    check_books(launch, outs, terms, ['src_real', 's_real'])
    flat = [tm for o in outputs for tm in o[5]]
    table, = launch.tail
    assert (table == 0) == (not up.kept) and len(up.kept) <= 1
    for o, (dst, div, dims, mults, J, tms) in zip(outs, outputs):
        nl, nk = int(o['n_levels']), int(o['n_k'])
        assert nl == nk == len(dims) and o['divisor'] == div
        zero_beyond(o, nl, 'ext', 'sd', 'ss')
        zero_beyond(o, nk, 'kext', 'ks')
        assert covers(span(o['dst'], es_of(launch.cplx), zip(o['ext'][:nl], o['sd'][:nl])), dst)
        assert int(np.prod(o['ext'][:nl])) == dst.size
        for t, (a, starts, S) in zip(terms[o['first_term']:o['first_term'] + o['n_terms']], flat[o['first_term']:]):
            levels = list(zip(o['ext'][:nl], o['ss'][:nl])) + list(zip(o['kext'][:nk], o['ks'][:nk]))
            assert covers(span(t['src'], es_of(launch.cplx, t['src_real']), levels), a, sum(x * st for x, st in zip(starts, a.strides)),
                          [d * m for d, m in zip(dims, mults)])
            assert up.holds(*span(table, es_of(launch.cplx, t['s_real']), [(int(np.prod(o['kext'][:nk])), 1)], int(t['s_off'])))


def reach_wdot(launch, xs, ys, whole=True):
    descs, = arrays(launch)
    assert launch.stem == 'cyb_dot_weighted' and len(descs) == len(xs)
    es = es_of(launch.cplx)
    for d, x, y in zip(descs, xs, ys):
        assert (covers if whole else inside)(span(d['x'], es, [(d['rows'], d['x_rs']), (d['cols'], d['x_cs'])]), x)
        assert (d['y'] == 0) == (y is None)
        if y is not None:
            assert inside(span(d['y'], es, [(d['rows'], d['y_rs']), (d['cols'], d['y_cs'])]), y)


# ---------------------------------------------------------------------------------------------------------------------------
# the argument lists: one case per branch of a packer

def axis_lists(c):
    """(records, mode, fill) lists; `c`: complex destinations"""
    src, dst = tile((14, 5), c), tile((14, 5), c)
    real_src = tile((14, 5))                                     # a real source under the complex entry
    dst_small = blk(9, 5, c=c)
    fac = blk(3, c=c)
    yield [TreeAxisRecord(src, dst, 0, 2, 2, 2, 3, 3, 2, fac), TreeAxisRecord(real_src, dst, 0, 0, 0, 1, 2, 2, 1, blk(2))], 'scale', [dst_small]
    yield [TreeAxisRecord(transposed(src), transposed(dst), 1, 2, 2, 2, 3, 3, 2, blk(3))], 'scale'            # side 1: column ranges
    yield [TreeAxisRecord(window(src, (0, 14, 2), (0, 5, -1)), dst_small, 0, 1, 0, 1, 3, 3, 2, blk(3))], 'scale'   # strided rows, reversed columns
    yield [TreeAxisRecord(blk(12, c=c), blk(12, c=c), 0, 0, 0, 2, 3, 3, 2, blk(3))], 'scale'                  # 1-D (diagonal) blocks
    yield [TreeAxisRecord(src, dst_small, 0, 1, 2, 2, 3, 1, 2, np.array([2])),
           TreeAxisRecord(real_src, dst_small, 0, 0, 6, 1, 3, 0, 2, np.zeros(0, dtype=np.int64))], 'gather'     # A_dst == 0: nothing kept
    tab = torch.tensor([0, 2])
    yield [TreeAxisRecord(src, dst, 0, 1, 0, 2, 3, 2, 2, tr.DeviceIndex(tab.data_ptr(), 2, tab))], 'gather'   # a table on the device
    whole = blk(14, 5, c=c)
    yield [TreeAxisRecord(transposed(dst_small), transposed(whole), 1, 0, 1, 2, 2, 3, 2, [2, 0])], 'scatter', [whole]
    yield [TreeAxisRecord(src, dst, 0, 14, 14, 0, 3, 3, 2, blk(3))], 'scale'                                  # outer == 0
    yield [], 'scatter', [dst_small]                                                                          # a fill alone
    yield [], 'gather'


def trace_lists(c):
    a, ar = tile((3, 4, 3, 2), c), tile((3, 4, 3, 2))
    yield [(tile((4, 2), c), [(a, [0], [2], [1, 3], 2.0), (transposed(ar, [2, 3, 0, 1]), [0], [-2], [-1, 1], -1.0)]),
           (tile((2,), c), []), (blk(c=c), [(tile((3, 2, 2, 3), c), [0, 1], [3, 2], [], 0.5)])]
    yield [(transposed(tile((2, 4), c)), [(a, [2], [0], [1, 3], 1.0)]), (blk(0, 2, c=c), [(blk(3, 0, 3, 2, c=c), [0], [2], [1, 3], 1.0)])]
    yield [(blk(2, c=c), [(blk(2, 0, 0, c=c), [1], [2], [0], 1.0)])]                                          # a traced extent of zero


def outer_lists(c):
    a, b, ar = tile((2, 3), c), tile((4, 5), c), tile((2, 3))
    yield [(tile((8, 15), c), [(a, b, 1.5), (ar, transposed(tile((5, 4), c)), -1.0)]), (tile((3, 2), c), []),
           (tile((6, 1), c), [(tile((2, 1), c), blk(3, 1), 1.0)])]
    yield [(window(blk(8, 30, c=c), (0, 8, 1), (15, 21, 1)), [(window(a, (0, 2, -1), (0, 3, 2)), window(b, (0, 4, 1), (0, 5, 2)), 1.0)])]
    yield [(blk(0, 15, c=c), [(blk(0, 3, c=c), blk(4, 5, c=c), 1.0)]), (blk(1, 6, c=c), [(blk(1, 2, c=c), blk(1, 3, c=c), 2.0)])]


def compose_lists(c):
    a, b = tile((4, 12), c), tile((3, 5), c)                     # domain: R = 4, m0 = m2 = 2, K = 3, N = 5
    yield [(tile((4, 20), c), 'domain', 2, 2, [(a, b, 1.0), (tile((4, 8)), transposed(tile((5, 2), c)), 0.5)]),
           (tile((4, 20), c), 'domain', 2, 2, []),
           (tile((20, 4), c), 'codomain', 2, 2, [(transposed(a), transposed(b), 2.0), (tile((8, 4), c), tile((5, 2)), 1.0)])]
    yield [(tile((4, 10), c), 'domain', 2, 1, [(blk(4, 0, c=c), blk(0, 5, c=c), 1.0)]),                       # K == 0
           (blk(0, 6, c=c), 'domain', 2, 1, [(blk(0, 4, c=c), blk(2, 3, c=c), 1.0)]),
           (tile((3, 1), c), 'codomain', 1, 1, [(tile((2, 1), c), tile((3, 2), c), 1.0)])]


def place_lists(c):
    dst = window(blk(5, 20, c=c), (1, 5, 1), (2, 14, 1))         # 4 rows, 2 runs of 3 columns every 6
    dst = HipBlock(None, dst.buf, dst.offset, (4, 2, 3), (20, 6, 1))
    yield [(dst, tile((2, 2, 3, 2), c), 2, 2.0), (tile((4, 2, 3), c), None, 0, 1.0), (tile((4, 2, 3), c), tile((4, 6)), 1, 1.0),
           (tile((4, 2, 3), c), transposed(tile((6, 4), c)), 1, -1.0), (tile((1, 2, 3), c), tile((6,), c), 0, 1.0),
           (tile((6, 1, 1), c), tile((2, 3), c), 2, 1.0)]
    yield [(blk(0, 2, 3, c=c), blk(0, 6, c=c), 1, 1.0), (blk(4, 0, 3, c=c), None, 0, 1.0)]


def strip_lists(c):
    dst, src, src_r = tile((8, 5), c), tile((9, 5), c), tile((9, 5))
    yield [(dst, 0, 1, 7, (2, 3), (1, 0), [(src, 2, 1.0), (src, 0, -0.5)]), (dst, 0, 7, 8, (1,), (0,), []),
           (tile((6, 5), c), 0, 0, 6, (3, 2), (0, 1), [(src_r, 3, 1.0)]), (tile((6, 5), c), 0, 0, 6, (1, 2, 3), (2, 0, 1), [(transposed(tile((5, 7), c)), 1, 1.0)])]
    yield [(transposed(blk(6, 5, c=c), [0, 1]), 1, 0, 4, (2, 2), (1, 0), [(tile((6, 6), c), 1, 2.0), (tile((6, 6), c), 2, 1.0)]),
           (tile((5, 8), c), 1, 2, 8, (3, 2), (1, 0), [(transposed(tile((9, 5), c)), 0, 1.0)]), (tile((5, 8), c), 1, 0, 0, (0, 2), (1, 0), [])]
    yield [(blk(0, 4, c=c), 0, 0, 0, (0,), (0,), [(blk(0, 4, c=c), 0, 1.0)]), (blk(3, 1, c=c), 0, 0, 1, (), (), [(blk(2, 1, c=c), 1, 1.0)])]


def dense_parts(c, cs):
    """a dense view of three legs (sectors of d * m = 2*2, 1*3, 2*1 at the starts 1, 0, 2), a coupled block and tree tensors"""
    S = np.ones((2, 1, 2), dtype=complex if cs else float)
    return (1, 0, 2), (2, 1, 2), (2, 3, 1), S


def to_dense_lists(c, cs=False):
    starts, dims, mults, S = dense_parts(c, cs)
    S2 = 2 * S
    dense = tile((6, 3, 6), c)
    for J, shape in ((0, (1, 6)), (1, (2, 3)), (3, (6, 1))):
        b, br = tile((shape[0] + 1, shape[1] + 2), c), tile(shape)
        yield dense, [(starts, dims, mults, J, [(b, 1, 2, S), (br, 0, 0, S2), (transposed(tile(shape[::-1], c)), 0, 0, S)]),
                      ((0, 0, 0), (1, 1, 1), (1, 3, 2), J, [])]
    yield transposed(tile((6, 3, 6), c), [2, 0, 1]), [((2, 1, 0), (2, 2, 1), (1, 2, 3), 2, [(tile((2, 3), c), 0, 0, np.ones((2, 2, 1)))])]
    yield blk(4, 0, c=c), [((0, 0), (2, 1), (2, 0), 1, [(blk(2, 0, c=c), 0, 0, np.ones((2, 1)))])]
    yield blk(c=c), [((), (), (), 0, [(blk(1, 1, c=c), 0, 0, np.ones(()))])]


def from_dense_lists(c, cs=False):
    starts, dims, mults, S = dense_parts(c, cs)
    dense, dense_r = tile((6, 3, 6), c), tile((6, 3, 6))
    for J, shape in ((0, (1, 6)), (1, (2, 3)), (3, (6, 1))):
        yield [(tile(shape, c), 2.0, dims, mults, J, [(dense, starts, S), (dense, (0, 0, 0), 3 * S)]), (tile(shape, c), 1.0, dims, mults, J, []),
               (transposed(tile(shape[::-1], c)), 4.0, dims, mults, J, [(dense_r, starts, S)])]
    yield [(tile((2, 3), c), 1.0, (2, 2, 1), (1, 2, 3), 2, [(transposed(tile((6, 3, 6), c), [2, 0, 1]), (2, 1, 0), np.ones((2, 2, 1)))])]
    yield [(blk(2, 0, c=c), 1.0, (2, 1), (2, 0), 1, [(blk(4, 0, c=c), (0, 0), np.ones((2, 1)))]), (blk(1, 1, c=c), 1.0, (), (), 0, [(blk(c=c), (), np.ones(()))])]


def wdot_inner_lists(c):
    a, b = tile((3, 4), c), tile((3, 4), c)
    yield [a, transposed(tile((4, 3), c)), blk(5, c=c), blk(0, 2, c=c)], [b, b, window(blk(10, c=c), (0, 10, -2)), blk(0, 2, c=c)], [1.0, 2.0, 0.5, 1.0], True
    yield [a, window(blk(6, 8, c=c), (0, 6, 2), (1, 8, 2))], [transposed(b), tile((4, 3), c)], [1.0, -1.0], False
    yield [a, blk(5, c=c)], None, [1.0, 3.0], False
    yield [], [], [], True


def wdot_trace_lists(c):
    yield [tile((3, 3), c), transposed(tile((4, 4), c)), blk(0, 0, c=c)], [1.0, 2.0, 1.0]
    yield [], []


ENTRIES = pytest.mark.parametrize('c', [False, True], ids=['f64', 'c128'])


@ENTRIES
def test_axis_records_stay_inside_their_blocks_and_tables(c):
    for args in axis_lists(c):
        reach_axis(args, Uploads())


@ENTRIES
def test_trace_records_stay_inside_their_views(c):
    for outputs in trace_lists(c):
        reach_trace(outputs)


@ENTRIES
def test_outer_records_stay_inside_their_views(c):
    for outputs in outer_lists(c):
        reach_outer(outputs)


@ENTRIES
def test_compose_records_stay_inside_their_views(c):
    for outputs in compose_lists(c):
        reach_compose(outputs)


@ENTRIES
def test_place_records_stay_inside_their_views(c):
    for records in place_lists(c):
        reach_place(records)


@ENTRIES
def test_strip_records_stay_inside_their_blocks(c):
    for outs in strip_lists(c):
        reach_strip(outs)


@pytest.mark.parametrize('c,cs', [(False, False), (True, False), (True, True)], ids=['f64', 'c128-real-tables', 'c128-complex-tables'])
def test_dense_records_stay_inside_their_views_and_the_table(c, cs):
    for dst_view, regions in to_dense_lists(c, cs):
        reach_to_dense(dst_view, regions)
    for outputs in from_dense_lists(c, cs):
        reach_from_dense(outputs)


@ENTRIES
def test_wdot_descriptors_stay_inside_their_blocks(c):
    for a_blocks, b_blocks, weights, dagger in wdot_inner_lists(c):
        launch = tr.pack_wdot_inner(a_blocks, b_blocks, weights, dagger)
        assert launch.cplx == (c and bool(a_blocks)) and launch.tail == (1 if dagger or b_blocks is None else 0,)
        reach_wdot(launch, a_blocks, b_blocks if b_blocks is not None else [None] * len(a_blocks))
    one = blk(1, c=c)
    for blocks, weights in wdot_trace_lists(c):
        launch = tr.pack_wdot_trace(blocks, weights, one)
        assert launch.tail == (0,)
        reach_wdot(launch, blocks, [one] * len(blocks), whole=False)          # the diagonals only


def test_nothing_to_launch_is_none():
    assert tr.pack_axis([], 'scale', upload=None) is None
    for pack in (tr.pack_trace, tr.pack_outer, tr.pack_compose, tr.pack_place, tr.pack_strip):
        assert pack([]) is None
    assert tr.pack_to_dense(blk(2, 2), [], None) is None and tr.pack_from_dense([], None) is None


def test_host_tables_are_uploaded_once_and_device_tables_not_at_all():
    src, dst = blk(12, 5), blk(12, 5)
    tab = torch.tensor([1])
    up = Uploads()
    launch = tr.pack_axis([TreeAxisRecord(src, dst, 0, 0, 0, 2, 3, 2, 2, [0, 2]), TreeAxisRecord(src, dst, 0, 0, 8, 1, 3, 1, 1, tr.DeviceIndex(tab.data_ptr(), 1, tab)),
                           TreeAxisRecord(src, dst, 0, 0, 9, 1, 3, 1, 1, np.array([1]))], 'gather', upload=up)
    assert len(up.kept) == 1 and up.kept[0].tolist() == [0, 2, 1] and up.kept[0].dtype == np.int64 and launch.keep == (up.kept[0],)
    tables = arrays(launch)[0]['table']
    assert list(tables) == [up.kept[0].ctypes.data, tab.data_ptr(), up.kept[0].ctypes.data + 16]
    up = Uploads()
    assert tr.pack_axis([TreeAxisRecord(src, dst, 0, 0, 8, 1, 3, 1, 1, tr.DeviceIndex(tab.data_ptr(), 1, tab))], 'gather', upload=up).keep == ()
    assert not up.kept
    S = np.arange(2.0)
    up = Uploads()
    launch = tr.pack_to_dense(blk(4, c=True), [((0,), (2,), (2,), 1, [(blk(2, 1), 0, 0, S), (blk(2, 1), 0, 0, S), (blk(2, 1), 0, 0, 1j * S)])], up)
    assert len(up.kept) == 1 and up.kept[0].tolist() == [0, 1, 0, 1j]          # every tensor once, one complex table
    assert arrays(launch)[1]['s_off'].tolist() == [0, 0, 2] and launch.keep == (up.kept[0],)


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks: the cases of the device tests, raised before any device is needed

def test_axis_errors():
    src, out = blk(41, 9), blk(13, 9)                 # the shapes of the device test: 5 + 3 * 6 * 2 == 41, 1 + 3 * 2 * 2 == 13
    keep_b = np.array([1, 4])
    assert tr.pack_axis([TreeAxisRecord(src, out, 0, 5, 1, 3, 6, 2, 2, keep_b)], 'gather', upload=Uploads()) is not None   # fits exactly
    with pytest.raises(ValueError, match='a kept position lies outside the large leg'):
        tr.pack_axis([TreeAxisRecord(src, out, 0, 5, 1, 3, 6, 2, 2, np.array([1, 6]))], 'gather', upload=Uploads())
    with pytest.raises(ValueError, match='a tree block reaches beyond its coupled block'):
        tr.pack_axis([TreeAxisRecord(src, out, 0, 6, 1, 3, 6, 2, 2, keep_b)], 'gather', upload=Uploads())               # the source
    with pytest.raises(ValueError, match='a tree block reaches beyond its coupled block'):
        tr.pack_axis([TreeAxisRecord(src, out, 0, 5, 2, 3, 6, 2, 2, keep_b)], 'gather', upload=Uploads())               # the destination
    with pytest.raises(ValueError, match='tree_axis_many: a 1-D source block has a codomain side only'):
        tr.pack_axis([TreeAxisRecord(blk(6), blk(6), 1, 0, 0, 1, 6, 6, 1, blk(6))], 'scale', upload=None)
    with pytest.raises(ValueError, match='stride 1'):
        tr.pack_axis([TreeAxisRecord(blk(6), blk(6), 0, 0, 0, 1, 6, 6, 1, window(blk(12), (0, 12, 2)))], 'scale', upload=None)
    with pytest.raises(ValueError, match='unknown mode'):
        tr.pack_axis([], 'shuffle', upload=None)
    with pytest.raises(TypeError, match='boolean'):
        tr.pack_axis([], 'scale', [blk(3, dtype=torch.bool)], upload=None)


def test_trace_errors():
    src9 = blk(*(2,) * 9)
    dst1 = blk(2)
    many = tr.pack_trace
    with pytest.raises(ValueError, match='more than 8 axes'):
        many([(dst1, [(src9, [0, 2, 4, 6], [1, 3, 5, 7], [8], 1.0)])])
    src10 = blk(*(2,) * 10)
    with pytest.raises(ValueError, match='more than 4 traced pairs'):
        many([(blk(), [(src10, [0, 2, 4, 6, 8], [1, 3, 5, 7, 9], [], 1.0)])])
    with pytest.raises(ValueError, match='more than 8 axes'):
        many([(blk(*(1,) * 9), [])])
    with pytest.raises(ValueError, match='share one dtype'):
        many([(dst1, []), (blk(2, c=True), [])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(dst1, [(blk(2, 3, 3), [1], [2], [0], 1j)])])
    with pytest.raises(ValueError, match='do not match'):
        many([(dst1, [(blk(2, 3, 4), [1], [2], [0], 1.0)])])


def test_outer_errors():
    a, b = blk(2, 3), blk(4, 5)
    many = tr.pack_outer
    with pytest.raises(ValueError, match='2-D'):
        many([(blk(8, 15), [(blk(2, 3, 1), b, 1.0)])])
    with pytest.raises(ValueError, match='2-D'):
        many([(blk(120), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='shape'):
        many([(blk(8, 14), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='shape'):
        many([(blk(15, 8), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='differ in their extents'):
        many([(blk(8, 15), [(a, b, 1.0), (blk(4, 3), blk(2, 5), 1.0)])])
    with pytest.raises(ValueError, match='share one dtype'):
        many([(blk(8, 15), [(a, b, 1.0)]), (blk(8, 15, c=True), [(a, b, 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(blk(8, 15), [(a, blk(4, 5, c=True), 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(blk(8, 15), [(a, b, 1j)])])
    with pytest.raises(ValueError, match='column stride'):
        many([(transposed(blk(15, 8)), [(a, b, 1.0)])])


def test_compose_errors():
    a, b = blk(4, 12), blk(3, 5)
    many = tr.pack_compose
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
        many([(transposed(blk(20, 4)), 'domain', 2, 2, [(a, b, 1.0)])])
    with pytest.raises(ValueError, match="'domain' or 'codomain'"):
        many([(blk(4, 20), 'both', 2, 2, [(a, b, 1.0)])])


def test_place_errors():
    dst = blk(4, 2, 3)
    many = tr.pack_place
    with pytest.raises(ValueError, match='3-D'):
        many([(blk(4, 6), blk(4, 6), 1, 1.0)])
    with pytest.raises(ValueError, match='share one dtype'):
        many([(dst, None, 0, 1.0), (blk(4, 2, 3, c=True), None, 0, 1.0)])
    with pytest.raises(ValueError, match='complex destination'):
        many([(dst, blk(4, 6, c=True), 1, 1.0)])
    with pytest.raises(ValueError, match='complex destination'):
        many([(dst, blk(4, 6), 1, 1j)])
    with pytest.raises(ValueError, match='stride 1'):
        many([(transposed(blk(3, 2, 4)), blk(4, 6), 1, 1.0)])
    with pytest.raises(ValueError, match='for a window of'):
        many([(dst, blk(6, 4), 1, 1.0)])
    with pytest.raises(ValueError, match='at most 6'):
        many([(blk(1, 1, 1), blk(*(1,) * 8), 7, 1.0)])


def test_strip_errors():
    dst, src = blk(6, 5), blk(8, 5)
    many = tr.pack_strip
    with pytest.raises(ValueError, match='2-D'):
        many([(blk(6, 5, 1), 0, 0, 6, (2, 3), (1, 0), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='share one dtype'):
        many([(dst, 0, 0, 6, (6,), (0,), []), (blk(6, 5, c=True), 0, 0, 6, (6,), (0,), [])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(dst, 0, 0, 6, (2, 3), (1, 0), [(blk(8, 5, c=True), 0, 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        many([(dst, 0, 0, 6, (2, 3), (1, 0), [(src, 0, 1j)])])
    with pytest.raises(ValueError, match='leaves axis 0'):
        many([(dst, 0, 1, 7, (2, 3), (1, 0), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='for a strip of 6'):
        many([(dst, 0, 0, 6, (2, 2), (1, 0), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='for a strip of 6'):
        many([(dst, 0, 0, 6, (2, 3), (1, 1), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='of a source of shape'):
        many([(dst, 0, 0, 6, (2, 3), (1, 0), [(src, 3, 1.0)])])
    with pytest.raises(ValueError, match='of a source of shape'):
        many([(dst, 0, 0, 6, (2, 3), (1, 0), [(blk(8, 4), 0, 1.0)])])
    with pytest.raises(ValueError, match='differ in their strides'):
        many([(dst, 0, 0, 6, (2, 3), (1, 0), [(src, 0, 1.0), (transposed(blk(5, 8)), 0, 1.0)])])
    with pytest.raises(ValueError, match='at most 6'):
        many([(blk(1, 1), 0, 0, 1, (1,) * 7, tuple(range(7)), [])])
    with pytest.raises(ValueError, match='side is'):
        many([(dst, 2, 0, 6, (6,), (0,), [])])


def test_dense_errors():
    S = np.ones((2, 1))
    up = Uploads()

    def to(dst_view, regions):
        return tr.pack_to_dense(dst_view, regions, up)

    def frm(outputs):
        return tr.pack_from_dense(outputs, up)

    with pytest.raises(ValueError, match='more than 6 axes'):
        to(blk(*(1,) * 7), [((0,) * 7, (1,) * 7, (1,) * 7, 3, [])])
    with pytest.raises(ValueError, match='leaves the view'):
        to(blk(6, 4), [((1, 0), (2, 1), (3, 4), 1, [])])
    with pytest.raises(ValueError, match='leaves its block'):
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(blk(3, 4), 1, 0, S)])])
    with pytest.raises(ValueError, match='tree tensor pair of shape'):
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(blk(3, 4), 0, 0, np.ones((2, 2)))])])
    with pytest.raises(ValueError, match='complex destination'):
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(blk(3, 4, c=True), 0, 0, S)])])
    with pytest.raises(ValueError, match='complex destination'):
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(blk(3, 4), 0, 0, S * 1j)])])
    with pytest.raises(ValueError, match='2-D'):
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(blk(12), 0, 0, S)])])
    with pytest.raises(TypeError, match='boolean'):
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(blk(3, 4, dtype=torch.bool), 0, 0, S)])])
    a = blk(6, 4)
    with pytest.raises(ValueError, match='destination view of shape'):
        frm([(blk(3, 5), 2.0, (2, 1), (3, 4), 1, [(a, (0, 0), S)])])
    with pytest.raises(ValueError, match='leaves the view'):
        frm([(blk(3, 4), 2.0, (2, 1), (3, 4), 1, [(a, (0, 1), S)])])
    with pytest.raises(ValueError, match='share one dtype'):
        frm([(blk(3, 4), 2.0, (2, 1), (3, 4), 1, [(a, (0, 0), S)]), (blk(3, 4, c=True), 2.0, (2, 1), (3, 4), 1, [(a, (0, 0), S)])])
    with pytest.raises(ValueError, match='complex destination'):
        frm([(blk(3, 4), 2.0, (2, 1), (3, 4), 1, [(blk(6, 4, c=True), (0, 0), S)])])
    with pytest.raises(ValueError, match='divisor'):
        frm([(blk(3, 4), 0.0, (2, 1), (3, 4), 1, [(a, (0, 0), S)])])
    with pytest.raises(ValueError, match='at most 6'):
        frm([(blk(1, 1), 1.0, (1,) * 7, (1,) * 7, 3, [])])


def test_wdot_errors():
    a, b = blk(3, 4), blk(3, 4)
    with pytest.raises(ValueError, match='one weight and one partner'):
        tr.pack_wdot_inner([a], [b, b], [1.0])
    with pytest.raises(ValueError, match='shape mismatch'):
        tr.pack_wdot_inner([a], [b], [1.0])                       # do_dagger=False: the partner is read transposed
    with pytest.raises(ValueError, match='needs 2-D'):
        tr.pack_wdot_inner([blk(3)], [blk(3)], [1.0])
    with pytest.raises(ValueError, match='1-D or 2-D'):
        tr.pack_wdot_inner([blk(3, 1, 1)], None, [1.0])
    with pytest.raises(TypeError, match='boolean'):
        tr.pack_wdot_inner([blk(3, dtype=torch.bool)], None, [1.0])
    with pytest.raises(ValueError, match='widen'):
        tr.pack_wdot_inner([a], [blk(3, 4, c=True)], [1.0], True)
    with pytest.raises(ValueError, match='one weight per block'):
        tr.pack_wdot_trace([a], [], blk(1))
    with pytest.raises(ValueError, match='square'):
        tr.pack_wdot_trace([a], [1.0], blk(1))
