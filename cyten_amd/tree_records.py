"""Descriptor records of the fusion-tree launches, packed on the host.

One ``pack_*`` function per launch of ``HipBlockBackend``'s ``tree_*_many`` / ``*_weighted_many`` methods: it takes the
arguments of that method, makes every check the method promises and returns the record arrays of ``include/cyten_amd.h`` as
a :class:`Launch`, or ``None`` when there is nothing to launch.  Nothing here touches a device, a context or the loaded
library (no torch, no :mod:`cyten_amd.block_backend`): a view is whatever has ``ptr``, ``shape``, ``strides``, ``ndim``,
``size``, ``is_complex``, ``is_bool`` and ``is_contiguous()``, so the stride arithmetic runs, and is tested, without a GPU.
Where packing needs data on the device in its middle (the index tables of ``pack_axis``, the tree-pair table of the two
dense packers) the caller passes `upload`: a contiguous host array -> (device address, object that keeps it alive).
"""
from __future__ import annotations

import functools
import itertools
import math
from typing import NamedTuple

import numpy as np

from . import _lib

__all__ = ['Launch', 'DeviceIndex', 'c_strides', 'numeric_only', 'tree_entry', 'pack_axis', 'pack_trace', 'pack_outer',
           'pack_compose', 'pack_place', 'pack_strip', 'pack_to_dense', 'pack_from_dense', 'pack_wdot_inner', 'pack_wdot_trace']


class Launch(NamedTuple):
    """what one launch hands to the library: the entry is ``{stem}_c128`` or ``{stem}_f64``"""
    stem: str
    cplx: bool
    arrays: tuple        # ((record array, its ctypes struct, number of records), ...) in argument order
    tail: tuple = ()     # the scalar arguments after the arrays
    keep: tuple = ()     # what must outlive the launch


class DeviceIndex:
    """`n` ascending int64 positions in device memory at `ptr` (one sector's kept singular values as written by
    ``truncate_select``); accepted by ``mask_gather_many`` in place of a host mask.  `owner` keeps the table alive."""

    __slots__ = ('ptr', 'n', 'owner')

    def __init__(self, ptr, n, owner):
        self.ptr, self.n, self.owner = int(ptr), int(n), owner


@functools.lru_cache(maxsize=16384)
def _c_strides_cached(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= max(int(s), 1)
    return tuple(reversed(st))


def c_strides(shape):
    """C-order element strides of `shape` (block shapes repeat: memoised)."""
    return _c_strides_cached(shape if type(shape) is tuple else tuple(int(x) for x in shape))


# ---------------------------------------------------------------------------------------------- what the packers share
def numeric_only(blocks, what):
    """The float64 / complex128 kernels address 8-byte words: a boolean block (1-byte storage) must be converted with
    ``to_dtype`` first -- fail loudly instead of reading past its buffer."""
    for b in blocks:
        if b is not None and b.is_bool:
            raise TypeError(f'{what}: boolean block where a float64 / complex128 block is required (use to_dtype)')


def tree_entry(what, dsts, srcs, ndim_error=None):
    """What the ``tree_*_many`` methods ask of their views before they look at one: no boolean view; `ndim_error`, the
    complaint about views with the wrong number of axes where there are some; destination views of one dtype.  Returns
    whether the call takes the complex128 entry."""
    numeric_only(dsts + srcs, what)
    if ndim_error:
        raise ValueError(f'{what}: {ndim_error}')
    kinds = {d.is_complex for d in dsts}
    if len(kinds) > 1:
        raise ValueError(f'{what}: the destination views of one call share one dtype')
    return kinds.pop()


_ZEROS = [(0,) * k for k in range(max(_lib.CYB_MAX_NDIM, _lib.CYB_TREE_DENSE_MAX_LEVELS) + 1)]


def _padded(values, width):
    """the tuple `values` at the fixed width of its ABI array: zeros behind what is used, cut where it is longer"""
    return (values + _ZEROS[width])[:width]


def _real_flag(cplx, view):
    """the ``*_real`` flag of an operand: float64 data read as it stands under the complex128 entry (0 under the float64 one)"""
    return 0 if view.is_complex or not cplx else 1


def _term_ranges(counts):
    """the books of a term table: per output its ``first_term`` and ``n_terms``; the ranges tile the table in order"""
    return list(itertools.accumulate(counts, initial=0))[:-1], counts


def _coefficients(what, cplx, coeffs, sources, noun='views'):
    """The ``coeff_re`` and ``coeff_im`` columns of the coefficients of a call.  The float64 entry takes neither a complex
    coefficient nor a complex source: the complaint is made for the whole call, before a term is looked at."""
    c = np.array([complex(x) for x in coeffs], dtype=np.complex128)
    if not cplx and (c.imag.any() or any([s.is_complex for s in sources])):
        raise ValueError(f'{what}: a complex source or coefficient needs complex destination {noun}')
    return c.real, c.imag


def _term_columns(tarr, cplx, coefficients, **operands):
    """the coefficient columns of a term table and, per operand column, its pointers and ``*_real`` flags"""
    tarr['coeff_re'], tarr['coeff_im'] = coefficients
    for name, views in operands.items():
        tarr[name] = [v.ptr for v in views]
        if cplx:         # (zeros under the float64 entry: `_real_flag`)
            tarr[name + '_real'] = [0 if v.is_complex else 1 for v in views]


def _tree_view(blk, side: int, what: str):
    """(stride of the tree index, stride of the other index, extent of the other index) of a coupled block whose tree
    blocks are row ranges (side 0, codomain) or column ranges (side 1, domain); a 1-D block is a one-column matrix"""
    if blk.ndim == 1:
        if side != 0:
            raise ValueError(f'tree_axis_many: a 1-D {what} block has a codomain side only')
        return blk.strides[0], 0, 1
    if blk.ndim != 2:
        raise ValueError(f'tree_axis_many: {what} blocks are coupled blocks (2-D) or diagonal blocks (1-D)')
    return (blk.strides[0], blk.strides[1], blk.shape[1]) if side == 0 else (blk.strides[1], blk.strides[0], blk.shape[0])


def _tree_pair_table(tensors, upload):
    """the tree-pair tensors of one call (host arrays, each once) as ONE device table: (its address or 0, what keeps it
    alive, offset of every tensor by id, whether the table is complex)"""
    uniq, offs, tot = [], {}, 0
    for s in tensors:
        if id(s) not in offs:
            offs[id(s)] = tot
            tot += s.size
            uniq.append(s)
    cplx = any(np.iscomplexobj(s) for s in uniq)
    if not tot:
        return 0, (), offs, cplx
    flat = np.concatenate([np.asarray(s, dtype=np.complex128 if cplx else np.float64).ravel() for s in uniq])
    addr, keep = upload(flat)
    return addr, (keep,), offs, cplx


def _tree_dense_region(what, view, starts, dims, mults, J):
    """checks one region of a dense view (axes in leg order) and returns its element offset inside the view"""
    L = view.ndim
    if not (len(starts) == len(dims) == len(mults) == L and 0 <= J <= L):
        raise ValueError(f'{what}: a region names {len(starts)} starts, {len(dims)} dimensions and {len(mults)} multiplicities for a view of {L} axes')
    if any(d < 1 or m < 0 or s < 0 or s + d * m > n for s, d, m, n in zip(starts, dims, mults, view.shape)):
        raise ValueError(f'{what}: the region at {tuple(starts)} with the dimensions {tuple(dims)} and multiplicities {tuple(mults)} leaves the '
                         f'view of shape {view.shape}')
    return sum(s * st for s, st in zip(starts, view.strides))


def _as_matrix(b):
    """(rows, cols, row stride, column stride) of a 1-D or 2-D block"""
    if b.ndim == 1:
        return b.shape[0], 1, b.strides[0], 0
    if b.ndim != 2:
        raise ValueError('inner_weighted_many: blocks are 1-D or 2-D')
    return b.shape[0], b.shape[1], b.strides[0], b.strides[1]


# ---------------------------------------------------------------------------------------------- one packer per launch
def pack_axis(records, mode, fill=(), *, upload):
    """records of ``tree_axis_many``.  The factors of a 'scale' record have the stride 1 (the caller copies others first);
    the host tables of 'gather' / 'scatter' go through `upload` once, concatenated ('scale' never calls it)."""
    if mode not in _lib.TREE_AXIS_MODES:
        raise ValueError(f'tree_axis_many: unknown mode {mode!r}')
    records, fill = list(records), list(fill)
    numeric_only([r.src for r in records] + [r.dst for r in records] + fill, 'tree_axis_many')
    kinds = {r.dst.is_complex for r in records} | {b.is_complex for b in fill}
    if len(kinds) > 1:
        raise ValueError('tree_axis_many: the destination blocks of one call share one dtype')
    cplx = bool(kinds and kinds.pop())
    n = len(records)
    arr = np.zeros(max(n, 1), dtype=_lib.TREE_AXIS_DTYPE)
    keep = ()
    if mode == 'scale':
        tables = [None] * n
        for i, r in enumerate(records):
            f = r.table
            if f.is_bool or f.ndim != 1 or f.shape[0] != r.A:
                raise ValueError('tree_axis_many: the factors of a record are a 1-D numeric block of A entries')
            if f.is_complex and not cplx:
                raise ValueError('tree_axis_many: complex factors need complex destination blocks')
            if f.strides[0] != 1 and f.shape[0] > 1:
                raise ValueError('tree_axis_many: the factors of a record are read with the stride 1')
            tables[i] = (f.ptr, 1 if f.is_complex else 0)
    else:
        host = [np.ascontiguousarray(r.table, dtype=np.int64) for r in records if not isinstance(r.table, DeviceIndex)]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in host])]).astype(np.int64)
        base = 0
        if offs[-1]:     # (nothing is allocated or uploaded when every table already is on the device)
            base, didx = upload(np.concatenate(host))
            keep = (didx,)
        tables, h = [None] * n, 0
        for i, r in enumerate(records):
            if isinstance(r.table, DeviceIndex):
                ptr, cnt = r.table.ptr, r.table.n
            else:
                ptr, cnt = (base + 8 * int(offs[h]) if len(host[h]) else 0), len(host[h])
                large = r.A if mode == 'gather' else r.A_dst
                if len(host[h]) and not (0 <= host[h].min() and host[h].max() < large):
                    raise ValueError('tree_axis_many: a kept position lies outside the large leg')
                h += 1
            if cnt != (r.A_dst if mode == 'gather' else r.A):
                raise ValueError('tree_axis_many: the table of a record does not match its small extent')
            tables[i] = (ptr, 0)
    for i, r in enumerate(records):
        s_ts, s_xs, X = _tree_view(r.src, r.side, 'source')
        d_ts, d_xs, Xd = _tree_view(r.dst, r.side, 'destination')
        if X != Xd:
            raise ValueError('tree_axis_many: source and destination differ in the extent of the other index')
        if r.src.is_complex and not cplx:
            raise ValueError('tree_axis_many: a complex source needs complex destination blocks')
        ext_s, ext_d = r.outer * r.A * r.inner, r.outer * r.A_dst * r.inner
        if min(r.src_start, r.dst_start, r.outer, r.A, r.A_dst, r.inner) >= 0 and (
                r.src_start + ext_s > r.src.shape[r.side if r.src.ndim == 2 else 0]
                or r.dst_start + ext_d > r.dst.shape[r.side if r.dst.ndim == 2 else 0]):
            raise ValueError('tree_axis_many: a tree block reaches beyond its coupled block')
        arr[i] = (r.src.ptr, r.dst.ptr, tables[i][0], s_ts, s_xs, d_ts, d_xs, r.src_start, r.dst_start, X, r.outer, r.A, r.A_dst,
                  r.inner, _lib.TREE_AXIS_MODES[mode], 0 if r.src.is_complex else 1, tables[i][1], 0)
    fills = np.zeros(max(len(fill), 1), dtype=_lib.TREE_FILL_DTYPE)
    for i, b in enumerate(fill):
        if not b.is_contiguous():
            raise ValueError('tree_axis_many: only contiguous blocks can be zero-filled')
        fills[i] = (b.ptr, b.size * (16 if b.is_complex else 8))
    if not n and not fill:
        return None
    return Launch('cyb_tree_axis', cplx, ((arr, _lib.TreeAxisRec, n), (fills, _lib.TreeFill, len(fill))), keep=keep)


def pack_trace(outputs):
    """records of ``tree_trace_many``"""
    what = 'tree_trace_many'
    outputs = [(dst, list(terms)) for dst, terms in outputs]
    if not outputs:
        return None
    dsts = [dst for dst, _ in outputs]
    srcs = [tm[0] for _, terms in outputs for tm in terms]
    cplx = tree_entry(what, dsts, srcs)
    coefficients = _coefficients(what, cplx, [tm[4] for _, terms in outputs for tm in terms], srcs)
    o_first, o_n = _term_ranges([len(terms) for _, terms in outputs])
    nd_max, np_max = _lib.CYB_MAX_NDIM, _lib.CYB_TRACE_MAX_PAIRS
    o_shape, o_str, t_pairs, t_rem, t_ext, t_str = [], [], [], [], [], []
    for dst, terms in outputs:
        shape = dst.shape
        if len(shape) > nd_max:
            raise ValueError(f'{what}: a destination view with more than {nd_max} axes')
        o_shape.append(_padded(shape, nd_max))
        o_str.append(_padded(dst.strides, nd_max))
        for a, idcs1, idcs2, remaining, _ in terms:
            nd = a.ndim
            if len(idcs1) > np_max:
                raise ValueError(f'{what}: more than {np_max} traced pairs')
            if nd > nd_max:
                raise ValueError(f'{what}: a source view with more than {nd_max} axes')
            idcs1, idcs2, remaining = [i % nd for i in idcs1], [i % nd for i in idcs2], [i % nd for i in remaining]
            if len(idcs1) != len(idcs2) or sorted(idcs1 + idcs2 + remaining) != list(range(nd)):
                raise ValueError(f'{what}: idcs1, idcs2 and remaining_idcs must list every axis once, in pairs')
            sh, st = a.shape, a.strides
            if any(sh[p] != sh[q] for p, q in zip(idcs1, idcs2)):
                raise ValueError(f'{what}: traced legs do not match')
            if tuple(sh[k] for k in remaining) != shape:
                raise ValueError(f'{what}: remaining axes {tuple(sh[k] for k in remaining)} of a term do not have the '
                                 f'shape {shape} of its destination view')
            t_pairs.append(len(idcs1))
            t_rem.append(_padded(tuple(st[k] for k in remaining), nd_max))
            t_ext.append(_padded(tuple(sh[p] for p in idcs1), np_max))
            t_str.append(_padded(tuple(st[p] + st[q] for p, q in zip(idcs1, idcs2)), np_max))
    oarr = np.zeros(len(outputs), dtype=_lib.TRACE_WEIGHTED_OUT_DTYPE)
    oarr['dst'], oarr['ndim'] = [d.ptr for d in dsts], [d.ndim for d in dsts]
    oarr['first_term'], oarr['n_terms'], oarr['shape'], oarr['dst_strides'] = o_first, o_n, o_shape, o_str
    n_t = len(srcs)
    tarr = np.zeros(max(n_t, 1), dtype=_lib.TRACE_WEIGHTED_TERM_DTYPE)
    if n_t:
        _term_columns(tarr, cplx, coefficients, src=srcs)
        tarr['n_pairs'], tarr['rem_strides'], tarr['pair_extent'], tarr['pair_stride'] = t_pairs, t_rem, t_ext, t_str
    return Launch('cyb_trace_weighted', cplx, ((oarr, _lib.TraceWeightedOut, len(outputs)), (tarr, _lib.TraceWeightedTerm, n_t)))


def pack_outer(outputs):
    """records of ``tree_outer_many``"""
    what = 'tree_outer_many'
    outputs = [(dst, list(terms)) for dst, terms in outputs]
    if not outputs:
        return None
    dsts = [dst for dst, _ in outputs]
    a_srcs = [tm[0] for _, terms in outputs for tm in terms]
    b_srcs = [tm[1] for _, terms in outputs for tm in terms]
    cplx = tree_entry(what, dsts, a_srcs + b_srcs,
                      any(x.ndim != 2 for x in dsts + a_srcs + b_srcs) and 'destinations and sources are 2-D views')
    coefficients = _coefficients(what, cplx, [tm[2] for _, terms in outputs for tm in terms], a_srcs + b_srcs)
    o_first, o_n = _term_ranges([len(terms) for _, terms in outputs])
    o_ext, o_ldd = [], []
    for dst, terms in outputs:
        H, W = dst.shape
        if dst.strides[1] != 1 and W > 1:
            raise ValueError(f'{what}: a destination view needs the column stride 1')
        ext = (H, 1, 1, W)          # (an output without terms: zeros, whatever the factorisation)
        for k, (a, b, _) in enumerate(terms):
            e = (a.shape[0], b.shape[0], a.shape[1], b.shape[1])
            if k and e != ext:
                raise ValueError(f'{what}: the terms of one output differ in their extents, {ext} and {e}')
            ext = e
            if (e[0] * e[1], e[2] * e[3]) != (H, W):
                raise ValueError(f'{what}: a destination view of shape {(H, W)} for sources of the shapes '
                                 f'{tuple(a.shape)} and {tuple(b.shape)}')
        o_ext.append(ext)
        o_ldd.append(dst.strides[0] if H > 1 else W)
    oarr = np.zeros(len(outputs), dtype=_lib.OUTER_WEIGHTED_OUT_DTYPE)
    ext = np.array(o_ext, dtype=np.int64).reshape(len(outputs), 4)
    oarr['dst'], oarr['ha'], oarr['hb'], oarr['wa'], oarr['wb'] = [d.ptr for d in dsts], ext[:, 0], ext[:, 1], ext[:, 2], ext[:, 3]
    oarr['ldd'], oarr['first_term'], oarr['n_terms'] = o_ldd, o_first, o_n
    n_t = len(a_srcs)
    tarr = np.zeros(max(n_t, 1), dtype=_lib.OUTER_WEIGHTED_TERM_DTYPE)
    if n_t:
        _term_columns(tarr, cplx, coefficients, a=a_srcs, b=b_srcs)
        tarr['a_rs'], tarr['a_cs'] = [a.strides[0] for a in a_srcs], [a.strides[1] for a in a_srcs]
        tarr['b_rs'], tarr['b_cs'] = [b.strides[0] for b in b_srcs], [b.strides[1] for b in b_srcs]
    return Launch('cyb_outer_weighted', cplx, ((oarr, _lib.OuterWeightedOut, len(outputs)), (tarr, _lib.OuterWeightedTerm, n_t)))


def pack_compose(outputs):
    """records of ``tree_compose_many``"""
    what = 'tree_compose_many'
    outputs = [(dst, side, int(m0), int(m2), list(terms)) for dst, side, m0, m2, terms in outputs]
    if not outputs:
        return None
    dsts = [o[0] for o in outputs]
    a_srcs = [tm[0] for o in outputs for tm in o[4]]
    b_srcs = [tm[1] for o in outputs for tm in o[4]]
    cplx = tree_entry(what, dsts, a_srcs + b_srcs,
                      any(x.ndim != 2 for x in dsts + a_srcs + b_srcs) and 'destinations and sources are 2-D views')
    coefficients = _coefficients(what, cplx, [tm[2] for o in outputs for tm in o[4]], a_srcs + b_srcs)
    o_first, o_n = _term_ranges([len(o[4]) for o in outputs])
    o_ext, o_sd, o_axis, t_K, t_sa, t_bn, t_bk = [], [], [], [], [], [], []
    for dst, side, m0, m2, terms in outputs:
        if side not in ('domain', 'codomain'):
            raise ValueError(f"{what}: side is 'domain' or 'codomain', not {side!r}")
        dom = side == 'domain'
        H, W = dst.shape
        if dst.strides[1] != 1 and W > 1:
            raise ValueError(f'{what}: a destination view needs the column stride 1')
        other, mine = (H, W) if dom else (W, H)          # the untouched extent, the extent m0 * N * m2
        N = mine // (m0 * m2) if m0 > 0 and m2 > 0 else 0
        if m0 < 0 or m2 < 0 or m0 * N * m2 != mine:
            raise ValueError(f'{what}: a destination view of shape {(H, W)} does not factor as m0 * N * m2 with '
                             f'm0 = {m0}, m2 = {m2} in the {side}')
        ldd = dst.strides[0]
        for a, b, _ in terms:
            K = b.shape[0] if dom else b.shape[1]
            want_a = (other, m0 * K * m2) if dom else (m0 * K * m2, other)
            want_b = (K, N) if dom else (N, K)
            if tuple(a.shape) != want_a or tuple(b.shape) != want_b:
                raise ValueError(f'{what}: a destination view of shape {(H, W)} with m0 = {m0}, m2 = {m2} in the {side} '
                                 f'for sources of the shapes {tuple(a.shape)} and {tuple(b.shape)}')
            ars, acs = a.strides
            t_K.append(K)
            t_sa.append((ars, K * m2 * acs, m2 * acs, acs) if dom else (K * m2 * ars, m2 * ars, ars, acs))
            t_bn.append(b.strides[1] if dom else b.strides[0])
            t_bk.append(b.strides[0] if dom else b.strides[1])
        o_ext.append((other, m0, N, m2) if dom else (m0, N, m2, other))
        o_sd.append((ldd, N * m2, m2, 1) if dom else (N * m2 * ldd, m2 * ldd, ldd, 1))
        o_axis.append(2 if dom else 1)
    oarr = np.zeros(len(outputs), dtype=_lib.COMPOSE_WEIGHTED_OUT_DTYPE)
    oarr['dst'], oarr['ext'], oarr['sd'], oarr['axis'] = [d.ptr for d in dsts], o_ext, o_sd, o_axis
    oarr['first_term'], oarr['n_terms'] = o_first, o_n
    n_t = len(a_srcs)
    tarr = np.zeros(max(n_t, 1), dtype=_lib.COMPOSE_WEIGHTED_TERM_DTYPE)
    if n_t:
        _term_columns(tarr, cplx, coefficients, a=a_srcs, b=b_srcs)
        tarr['K'], tarr['sa'], tarr['b_ns'], tarr['b_ks'] = t_K, t_sa, t_bn, t_bk
    return Launch('cyb_compose_weighted', cplx, ((oarr, _lib.ComposeWeightedOut, len(outputs)), (tarr, _lib.ComposeWeightedTerm, n_t)))


def pack_place(records):
    """records of ``tree_place_many``"""
    what = 'tree_place_many'
    records = [(dst, src, int(n_row), complex(coeff)) for dst, src, n_row, coeff in records]
    if not records:
        return None
    dsts = [r[0] for r in records]
    cplx = tree_entry(what, dsts, [r[1] for r in records if r[1] is not None],
                      any(d.ndim != 3 for d in dsts) and 'destinations are 3-D views (rows, runs, columns of a run)')
    with_src = [r for r in records if r[1] is not None]
    _coefficients(what, cplx, [r[3] for r in with_src], [r[1] for r in with_src])
    nl = _lib.CYB_TREE_PLACE_MAX_LEVELS
    pad = _ZEROS[nl]
    arr = np.zeros(len(records), dtype=_lib.TREE_PLACE_DTYPE)
    for i, (dst, src, n_row, coeff) in enumerate(records):
        h, nq, wn = dst.shape
        if dst.strides[2] != 1 and wn > 1:
            raise ValueError(f'{what}: a destination view needs the stride 1 on its last axis')
        if src is None:
            arr[i] = (dst.ptr, 0, h, nq, wn, dst.strides[1], dst.strides[0], 0, 0, pad, pad, pad, pad, 0.0, 0.0, 0, 0)
            continue
        n_col = src.ndim - n_row
        if not (0 <= n_row <= nl and 0 <= n_col <= nl):
            raise ValueError(f'{what}: a source view with {n_row} row axes and {n_col} column axes, at most {nl} each')
        if (math.prod(src.shape[:n_row]), math.prod(src.shape[n_row:])) != (h, nq * wn):
            raise ValueError(f'{what}: a source view of shape {tuple(src.shape)} with {n_row} row axes for a window of {h} rows and '
                             f'{nq} x {wn} columns')
        rpad, cpad = _ZEROS[nl - n_row], _ZEROS[nl - n_col]
        arr[i] = (dst.ptr, src.ptr, h, nq, wn, dst.strides[1], dst.strides[0], n_row, n_col,
                  src.shape[:n_row] + rpad, src.strides[:n_row] + rpad, src.shape[n_row:] + cpad, src.strides[n_row:] + cpad,
                  coeff.real, coeff.imag, _real_flag(cplx, src), 0)
    return Launch('cyb_tree_place', cplx, ((arr, _lib.TreePlaceRec, len(records)),))


def pack_strip(outs):
    """records of ``tree_strip_many``"""
    what = 'tree_strip_many'
    outs = [(dst, side, start, stop, tuple(dims), tuple(axes), list(terms)) for dst, side, start, stop, dims, axes, terms in outs]
    if not outs:
        return None
    dsts = [o[0] for o in outs]
    srcs = [tm[0] for o in outs for tm in o[6]]
    cplx = tree_entry(what, dsts, srcs, any(x.ndim != 2 for x in dsts + srcs) and 'destinations and sources are 2-D blocks')
    coefficients = _coefficients(what, cplx, [tm[2] for o in outs for tm in o[6]], srcs, 'blocks')
    o_first = _term_ranges([len(o[6]) for o in outs])[0]
    nl = _lib.CYB_TREE_PLACE_MAX_LEVELS
    pad = _ZEROS[nl]
    es = 16 if cplx else 8
    rows, splits = [], {}         # one record per row, as the int64 words of cyb_tree_strip_out
    t_base = []
    for (dst, side, start, stop, dims, axes, terms), first in zip(outs, o_first):
        if side not in (0, 1):
            raise ValueError(f'{what}: side is 0 (rows) or 1 (columns), not {side}')
        if dst.strides[1] != 1 and dst.shape[1] > 1:
            raise ValueError(f'{what}: a destination block needs the column stride 1')
        if not 0 <= start <= stop <= dst.shape[side]:
            raise ValueError(f'{what}: the strip {start}:{stop} leaves axis {side} of its block of shape {tuple(dst.shape)}')
        n, other = stop - start, dst.shape[1 - side]
        split = splits.get((dims, axes))
        if split is None:                # (the strips of one side share the permutation and, per class of trees, the dimensions)
            if len(dims) > nl:
                raise ValueError(f'{what}: a strip of {len(dims)} levels, at most {nl}')
            if sorted(axes) != list(range(len(dims))) or min(dims, default=1) < 0:
                raise ValueError(f'{what}: the dimensions {dims} under the axes {axes} for a strip of {n}')
            old = c_strides(dims)
            split = splits[(dims, axes)] = (math.prod(dims), _padded(tuple(dims[a] for a in axes), nl), tuple(old[a] for a in axes))
        if split[0] != n:
            raise ValueError(f'{what}: the dimensions {dims} under the axes {axes} for a strip of {n}')
        ext, lev, strides = split[1], (), None
        for src, src_start, _ in terms:
            if src.shape[1 - side] != other or not 0 <= src_start <= src_start + n <= src.shape[side]:
                raise ValueError(f'{what}: the strip {src_start}:{src_start + n} of axis {side} of a source of shape {tuple(src.shape)} '
                                 f'for a destination of shape {tuple(dst.shape)}')
            if strides is None:
                strides = src.strides
                lev = tuple(u * strides[side] for u in split[2])
            elif src.strides != strides:
                raise ValueError(f'{what}: the sources of one strip differ in their strides, {strides} and {src.strides}')
            t_base.append(src_start * strides[side])
        across = strides[1 - side] if terms else 0
        ldd = dst.strides[0]
        one, step = (other,) + pad[1:], (across,) + pad[1:]
        lev = _padded(lev, nl)
        if side == 0:     # (the two int32 level counts share a word: rows low, columns high)
            rows.append((dst.ptr + start * ldd * es, n, 1, other, other, ldd, len(dims) | 1 << 32) + ext + lev + one + step
                        + (first, len(terms)))
        else:
            rows.append((dst.ptr + start * es, other, 1, n, n, ldd, 1 | len(dims) << 32) + one + step + ext + lev
                        + (first, len(terms)))
    oarr = np.array(rows, dtype=np.int64).view(_lib.TREE_STRIP_OUT_DTYPE).reshape(len(outs))
    n_t = len(srcs)
    tarr = np.zeros(max(n_t, 1), dtype=_lib.TREE_STRIP_TERM_DTYPE)
    if n_t:
        _term_columns(tarr, cplx, coefficients, src=srcs)
        tarr['base'] = t_base
    return Launch('cyb_tree_strip', cplx, ((oarr, _lib.TreeStripOut, len(outs)), (tarr, _lib.TreeStripTerm, n_t)))


def pack_to_dense(dst_view, regions, upload):
    """records of ``tree_to_dense_many``; the tree-pair tensors go through `upload` as one table"""
    what = 'tree_to_dense_many'
    regions = [(tuple(st), tuple(d), tuple(m), int(J), list(terms)) for st, d, m, J, terms in regions]
    if not regions:
        return None
    blocks = [tm[0] for r in regions for tm in r[4]]
    L, cplx = dst_view.ndim, tree_entry(what, [dst_view], blocks)
    if L > _lib.CYB_TREE_DENSE_MAX_LEGS:
        raise ValueError(f'{what}: a destination view with more than {_lib.CYB_TREE_DENSE_MAX_LEGS} axes')
    if any(b.ndim != 2 for b in blocks):
        raise ValueError(f'{what}: blocks are 2-D views')
    table, keep, s_offs, s_cplx = _tree_pair_table([tm[3] for r in regions for tm in r[4]], upload)
    if not cplx and (s_cplx or any(b.is_complex for b in blocks)):
        raise ValueError(f'{what}: a complex block or tree tensor needs a complex destination view')
    order = sorted(range(L), key=lambda l: -abs(dst_view.strides[l]))       # the last level: the contiguous run of the destination
    pad = _ZEROS[_lib.CYB_TREE_DENSE_MAX_LEVELS - 2 * L]      # (every region of a call has the 2 L levels of the view)
    o_first = _term_ranges([len(r[4]) for r in regions])[0]
    oarr = np.zeros(len(regions), dtype=_lib.TREE_TO_DENSE_OUT_DTYPE)
    tarr = np.zeros(max(len(blocks), 1), dtype=_lib.TREE_TO_DENSE_TERM_DTYPE)
    es, s_real = (16 if cplx else 8), (0 if s_cplx or not cplx else 1)
    for i, (starts, dims, mults, J, terms) in enumerate(regions):
        off = _tree_dense_region(what, dst_view, starts, dims, mults, J)
        s_str = c_strides(dims)
        r_str, c_str = c_strides(mults[:J]), c_strides(mults[J:])
        ext, sd, ss, sr, sc = [], [], [], [], []
        for l in order:
            ext += [dims[l], mults[l]]
            sd += [mults[l] * dst_view.strides[l], dst_view.strides[l]]
            ss += [s_str[l], 0]
            sr += [0, r_str[l] if l < J else 0]
            sc += [0, c_str[l - J] if l >= J else 0]
        H, W = math.prod(mults[:J]), math.prod(mults[J:])
        for t, (blk, r0, c0, S) in enumerate(terms, o_first[i]):
            if tuple(S.shape) != dims:
                raise ValueError(f'{what}: a tree tensor pair of shape {tuple(S.shape)} for the sector dimensions {dims}')
            if r0 < 0 or c0 < 0 or r0 + H > blk.shape[0] or c0 + W > blk.shape[1]:
                raise ValueError(f'{what}: the tile at ({r0}, {c0}) of {H} x {W} elements leaves its block of shape {blk.shape}')
            tarr[t] = (blk.ptr, r0, c0, blk.strides[0], blk.strides[1], s_offs[id(S)], _real_flag(cplx, blk), s_real)
        oarr[i] = (dst_view.ptr + es * off, 2 * L, 0, tuple(ext) + pad, tuple(sd) + pad, tuple(ss) + pad, tuple(sr) + pad,
                   tuple(sc) + pad, o_first[i], len(terms))
    return Launch('cyb_tree_to_dense', cplx, ((oarr, _lib.TreeToDenseOut, len(regions)), (tarr, _lib.TreeToDenseTerm, len(blocks))),
                  (table,), keep)


def pack_from_dense(outputs, upload):
    """records of ``tree_from_dense_many``; the tree-pair tensors go through `upload` as one table"""
    what = 'tree_from_dense_many'
    outputs = [(dst, float(div), tuple(d), tuple(m), int(J), list(terms)) for dst, div, d, m, J, terms in outputs]
    if not outputs:
        return None
    dsts = [o[0] for o in outputs]
    srcs = [tm[0] for o in outputs for tm in o[5]]
    cplx = tree_entry(what, dsts, srcs, any(d.ndim != 2 for d in dsts) and 'destinations are 2-D views')
    table, keep, s_offs, s_cplx = _tree_pair_table([tm[2] for o in outputs for tm in o[5]], upload)
    if not cplx and (s_cplx or any(a.is_complex for a in srcs)):
        raise ValueError(f'{what}: a complex source or tree tensor needs complex destination views')
    nk = _lib.CYB_TREE_DENSE_MAX_LEGS
    o_first = _term_ranges([len(o[5]) for o in outputs])[0]
    oarr = np.zeros(len(outputs), dtype=_lib.TREE_FROM_DENSE_OUT_DTYPE)
    tarr = np.zeros(max(len(srcs), 1), dtype=_lib.TREE_FROM_DENSE_TERM_DTYPE)
    s_real = 0 if s_cplx or not cplx else 1
    for i, (dst, div, dims, mults, J, terms) in enumerate(outputs):
        L = len(dims)
        if L > nk or len(mults) != L or not 0 <= J <= L:
            raise ValueError(f'{what}: {len(dims)} dimensions and {len(mults)} multiplicities, at most {nk} legs')
        if dst.shape != (math.prod(mults[:J]), math.prod(mults[J:])):
            raise ValueError(f'{what}: a destination view of shape {dst.shape} for the multiplicities {mults[:J]} and {mults[J:]}')
        if div == 0.0 or div != div:
            raise ValueError(f'{what}: the divisor is zero or NaN')
        a_str = terms[0][0].strides if terms else (0,) * L
        for t, (a, starts, S) in enumerate(terms, o_first[i]):
            off = _tree_dense_region(what, a, starts, dims, mults, J)
            if a.strides != a_str:
                raise ValueError(f'{what}: the source views of one output share their strides')
            if tuple(S.shape) != dims:
                raise ValueError(f'{what}: a tree tensor pair of shape {tuple(S.shape)} for the sector dimensions {dims}')
            tarr[t] = (a.ptr + (16 if a.is_complex else 8) * off, s_offs[id(S)], _real_flag(cplx, a), s_real)
        order = sorted(range(L), key=lambda l: -abs(a_str[l]))              # the last level: the contiguous run of the source
        d_str = [x * dst.strides[0] for x in c_strides(mults[:J])] + [x * dst.strides[1] for x in c_strides(mults[J:])]
        pad = _ZEROS[nk - L]
        oarr[i] = (dst.ptr, L, L, tuple(mults[l] for l in order) + pad, tuple(d_str[l] for l in order) + pad,
                   tuple(a_str[l] for l in order) + pad, dims + pad, tuple(m * s for m, s in zip(mults, a_str)) + pad, div,
                   o_first[i], len(terms))
    return Launch('cyb_tree_from_dense', cplx, ((oarr, _lib.TreeFromDenseOut, len(outputs)), (tarr, _lib.TreeFromDenseTerm, len(srcs))),
                  (table,), keep)


def _wdot_launch(what, operands, descs, conj):
    """the descriptor list of the weighted reduction; `conj` is the extra argument of the complex128 entry.  The kernel
    reads every operand in the element size of its entry, so the operands are of one dtype."""
    kinds = {x.is_complex for x in operands}
    if len(kinds) > 1:
        raise ValueError(f'{what}: float64 beside complex128 blocks, widen them first')
    arr = np.zeros(max(len(descs), 1), dtype=_lib.WDOT_DTYPE)
    for i, d in enumerate(descs):
        arr[i] = d
    return Launch('cyb_dot_weighted', bool(kinds and kinds.pop()), ((arr, _lib.WDotDesc, len(descs)),), (1 if conj else 0,))


def pack_wdot_inner(a_blocks, b_blocks, weights, do_dagger=False):
    """descriptors of ``inner_weighted_many``; the blocks of one call are of one dtype (the caller widens mixed ones)"""
    a_blocks, weights = list(a_blocks), [float(w) for w in weights]
    norm = b_blocks is None
    b_blocks = a_blocks if norm else list(b_blocks)
    if not (len(a_blocks) == len(b_blocks) == len(weights)):
        raise ValueError('inner_weighted_many: one weight and one partner per block')
    numeric_only(a_blocks + b_blocks, 'inner_weighted_many')
    descs = []
    for x, y, w in zip(a_blocks, b_blocks, weights):
        rows, cols, x_rs, x_cs = _as_matrix(x)
        yr, yc, y_rs, y_cs = _as_matrix(y)
        if not (do_dagger or norm):
            if x.ndim != 2 or y.ndim != 2:
                raise ValueError('inner_weighted_many: do_dagger=False needs 2-D blocks')
            yr, yc, y_rs, y_cs = yc, yr, y_cs, y_rs
        if (rows, cols) != (yr, yc):
            raise ValueError('inner: shape mismatch')
        descs.append((x.ptr, 0 if norm else y.ptr, rows, cols, x_rs, x_cs, y_rs, y_cs, w))
    return _wdot_launch('inner_weighted_many', a_blocks + b_blocks, descs, do_dagger or norm)


def pack_wdot_trace(blocks, weights, one):
    """descriptors of ``trace_weighted_many``: the diagonals (element stride ld + 1) against `one`, the constant one of the
    blocks' dtype on the device"""
    blocks, weights = list(blocks), list(weights)
    if len(blocks) != len(weights):
        raise ValueError('trace_weighted_many: one weight per block')
    numeric_only(blocks, 'trace_weighted_many')
    descs = []
    for b, w in zip(blocks, weights):
        if b.ndim != 2 or b.shape[0] != b.shape[1]:
            raise ValueError('trace_weighted_many: blocks must be square matrices')
        descs.append((b.ptr, one.ptr, b.shape[0], 1, b.strides[0] + b.strides[1], 0, 0, 0, float(w)))
    return _wdot_launch('trace_weighted_many', blocks + [one] if blocks else [], descs, False)
