"""Guard-band cases for the data-movement kernels of csrc/blockops.hip at the C ABI: the strided copy (row, shared-row,
elementwise and the two LDS-tiled transposing kernels), mask gather / scatter, scale_axis, the complex operand expansion
and the strided linear combination.  Builder, runner, checker and a numpy stand-in, all on the host (no device, no
torch), after the pattern of tests/gemm_guard_cases.py, whose SENTINEL and HostMemory are used here.

Arenas.  A case is ONE call: a list of records in the form the C ABI takes them (CopyDesc, MaskDesc, ScaleAxisDesc,
CExpandDesc, LincombDesc / LincombTerm[C128] of cyten_amd._lib) over two byte arenas.  `ain` holds everything the call
only reads, `aout0` everything it writes (and `x` of an in-place scale_axis).  Every view has a parent of its own inside
its arena: at least 64 bytes before and after it, the gaps of a strided view between its elements.  A parent of `aout0`
is pre-filled with a pattern that is unique per position (8- and 16-byte elements: the distinct finite doubles
SENTINEL * (1 + k 2^-40); 1- and 4-byte elements: a fixed pseudo-random byte stream), a parent of `ain` with values that
are unique per position, the view being a part of that pattern: a wrong index reads a value no other index has.

Every operation is exact -- pure data movement, or one IEEE rounding per element (scale_axis), or sums of integers times
powers of two (lincomb) -- so `check` compares raw bytes:
  sentinel  a byte of `aout0` outside the addressed elements changed (a write out of bounds, the gaps included),
  interior  an addressed element differs from the reference, bit for bit (-0.0 and NaN payloads count),
  source    a byte of `ain` changed.
The reference of a record is written by its builder with numpy views (as_strided); `NumpyMove`, the stand-in for the
device, evaluates the filled descriptor arrays by index arithmetic instead, on the path `classify_copy` (a mirror of
normalize_copy and classify_transpose of csrc/copy_kernels.h) says the device takes."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from cyten_amd import _lib
from gemm_guard_cases import SENTINEL, HostMemory, _odd_above   # noqa: F401  (HostMemory: re-exported for the model test)

MAXD = _lib.CYB_MAX_NDIM
ROW_MIN, SHARED_ROW_MIN = 16, 2048          # copy_strided_body: row path from 16 elements, waves share a row from 2048
TILE_MIN = 16                               # classify_transpose: both tiled extents at least 16
ITEM = 8192                                 # chunk_real of every list here (lists below 16 M elements)
CLASSES = ('row', 'shared-row', 'elementwise', 'tiled32', 'tiled64')
FAULT_KINDS = ('past_row', 'odd_tail', 'j1_eq_j0', 'expand_sign', 'no_conj', 'composite_div', 'scatter_no_zero', 'src_at_dst_strides')


# ---- the host mirror of the copy classification -----------------------------------------------------------------------

def normalize_copy(shape, ds, ss):
    """Singleton axes dropped, axes that are contiguous in BOTH operands merged: [[extent, dst stride, src stride], ...]
    and the number of elements (normalize_copy of csrc/copy_kernels.h)."""
    out = []
    for n, d, s in zip(shape, ds, ss):
        if n == 1:
            continue
        if out and out[-1][1] == d * n and out[-1][2] == s * n:
            out[-1] = [out[-1][0] * n, d, s]
        else:
            out.append([n, d, s])
    return out, math.prod(shape)


def classify_transpose(axes, total):
    """The tiled form of a normalized copy, or None (classify_transpose of csrc/copy_kernels.h)."""
    nd = len(axes)
    aS = next((k for k in range(nd) if axes[k][2] == 1), -1)
    aD = next((k for k in range(nd) if axes[k][1] == 1), -1)
    pD = pS = -1
    if aS >= 0 and aD >= 0 and aS != aD:
        if axes[aD][0] < TILE_MIN:
            for k in range(nd):
                if k != aD and k != aS and axes[k][1] == axes[aD][0]:
                    pD = k
        if axes[aS][0] < TILE_MIN:
            for k in range(nd):
                if k != aS and k != aD and k != pD and axes[k][2] == axes[aS][0]:
                    pS = k
    extS = axes[aS][0] * (axes[pS][0] if pS >= 0 else 1) if aS >= 0 else 0
    extD = axes[aD][0] * (axes[pD][0] if pD >= 0 else 1) if aD >= 0 else 0
    if not (total > 0 and aS >= 0 and aD >= 0 and aS != aD and extS >= TILE_MIN and extD >= TILE_MIN):
        return None
    t = dict(nS=extS, nD=extD, composite=pD >= 0 or pS >= 0)
    t.update(dict(nD2=axes[aD][0], ssD=axes[pD][2], ssD2=axes[aD][2]) if pD >= 0 else dict(nD2=1, ssD=axes[aD][2], ssD2=0))
    t.update(dict(nS2=axes[aS][0], dsS=axes[pS][1], dsS2=axes[aS][1]) if pS >= 0 else dict(nS2=1, dsS=axes[aS][1], dsS2=0))
    t['outer'] = [axes[k] for k in range(nd) if k not in (aS, aD, pS, pD)]
    return t


@dataclass
class CopyClass:
    name: str                 # one of CLASSES, or 'empty'
    composite: bool
    axes: list                # the normalized copy
    tiled: dict | None
    tiles: int = 0


def classify_copy(shape, ds, ss, elem_size, conj=0) -> CopyClass:
    """The kernel class cyb_copy_strided_batched gives a record."""
    axes, total = normalize_copy(shape, ds, ss)
    if total == 0:
        return CopyClass('empty', False, axes, None)
    t = classify_transpose(axes, total)
    if t is not None:
        tsz = 64 if elem_size == 8 else 32
        tiles = math.prod(a[0] for a in t['outer']) * -(-t['nS'] // tsz) * -(-t['nD'] // tsz)
        return CopyClass('tiled64' if elem_size == 8 else 'tiled32', t['composite'], axes, t, tiles)
    if axes and axes[-1][1] == 1 and axes[-1][2] == 1 and axes[-1][0] >= ROW_MIN and not (elem_size == 16 and conj):
        return CopyClass('shared-row' if axes[-1][0] >= SHARED_ROW_MIN else 'row', False, axes, None)
    return CopyClass('elementwise', False, axes, None)


# ---- arenas and views -------------------------------------------------------------------------------------------------

def _offsets(shape, strides):
    """Element offsets of all index tuples of a strided view, in C order."""
    off = np.zeros((), np.int64)
    for n, s in zip(shape, strides):
        off = off[..., None] + np.arange(n, dtype=np.int64) * s
    return off.reshape(-1)


def _c_strides(shape):
    out, s = [], 1
    for n in reversed(shape):
        out.append(s)
        s *= max(n, 1)
    return tuple(reversed(out))


def _pad8(seq, fill):
    seq = list(seq)
    return seq + [fill] * (MAXD - len(seq))


@dataclass
class View:
    side: str                 # 'in' | 'out'
    chunk: int
    off: int                  # byte offset of the origin inside its parent
    gbyte: int                # the same inside the arena
    es: int
    shape: tuple
    strides: tuple            # in elements

    @property
    def ptr(self):
        return (self.side, self.gbyte)

    def bytes(self, parent):
        """uint8 array of shape + (es,) over `parent` (the parent's own bytes, or a copy of the same size)."""
        st = tuple(s * self.es for s in self.strides) + (1,)
        return np.lib.stride_tricks.as_strided(parent[self.off:self.off + 1], tuple(self.shape) + (self.es,), st)

    def f64(self, parent):
        return self.bytes(parent).view(np.float64)[..., 0]

    def c128(self, parent):
        return self.bytes(parent).view(np.complex128)[..., 0]


@dataclass
class Case:
    op: str                   # copy | gather | scatter | scale | cexpand | lincomb_f64 | lincomb_c128
    elem_size: int
    ain: np.ndarray           # uint8
    aout0: np.ndarray         # uint8, before the call
    expect: np.ndarray        # uint8, what the call must leave
    addressed: np.ndarray     # bool per byte of aout0
    recs: list = field(default_factory=list)
    parents: list = field(default_factory=list)      # per record: [start, end) of its destination parent, origin byte

    def descriptors(self, base_in, base_out):
        """The filled ctypes arrays of the call for arenas at the byte addresses `base_in` / `base_out`."""
        if base_in % 16 or base_out % 16:
            raise ValueError('guard cases need 16-byte aligned arenas')
        base = {'in': base_in, 'out': base_out}

        def at(p):
            return base[p[0]] + p[1]

        n = len(self.recs)
        if self.op == 'copy':
            arr = (_lib.CopyDesc * max(n, 1))()
            for d, r in zip(arr, self.recs):
                d.dst, d.src, d.ndim, d.conj = at(r['dst']), at(r['src']), len(r['shape']), r['conj']
                d.shape[:], d.dst_strides[:], d.src_strides[:] = _pad8(r['shape'], 1), _pad8(r['ds'], 0), _pad8(r['ss'], 0)
            return (arr, n)
        if self.op in ('gather', 'scatter'):
            arr = (_lib.MaskDesc * max(n, 1))()
            for d, r in zip(arr, self.recs):
                d.x, d.out, d.idx = at(r['x']), at(r['out']), at(r['idx'])
                d.outer, d.axis, d.inner, d.n_keep = r['outer'], r['axis'], r['inner'], r['n_keep']
            return (arr, n)
        if self.op == 'scale':
            arr = (_lib.ScaleAxisDesc * max(n, 1))()
            for d, r in zip(arr, self.recs):
                d.x, d.f, d.out, d.outer, d.axis, d.inner = at(r['x']), at(r['f']), at(r['out']), r['outer'], r['axis'], r['inner']
            return (arr, n)
        if self.op == 'cexpand':
            arr = (_lib.CExpandDesc * max(n, 1))()
            for d, r in zip(arr, self.recs):
                d.src, d.rs, d.cs, d.K, d.N, d.dst = at(r['src']), r['rs'], r['cs'], r['K'], r['N'], at(r['dst'])
            return (arr, n)
        cplx = self.op == 'lincomb_c128'
        n_terms = sum(len(r['terms']) for r in self.recs)
        arr = (_lib.LincombDesc * max(n, 1))()
        terms = ((_lib.LincombTermC128 if cplx else _lib.LincombTerm) * max(n_terms, 1))()
        k = 0
        for d, r in zip(arr, self.recs):
            d.dst, d.ndim, d.accumulate, d.term_begin = at(r['dst']), len(r['shape']), r['accumulate'], k
            d.shape[:], d.dst_strides[:] = _pad8(r['shape'], 1), _pad8(r['ds'], 0)
            for t in r['terms']:
                terms[k].src = at(t['src'])
                terms[k].src_strides[:] = _pad8(t['ss'], 0)
                if cplx:
                    terms[k].coeff_re, terms[k].coeff_im, terms[k].src_real = t['coeff'].real, t['coeff'].imag, t['src_real']
                else:
                    terms[k].coeff = t['coeff']
                k += 1
            d.term_end = k
        return (arr, n, terms, n_terms)


_STREAM = np.random.default_rng(20240229).integers(0, 256, size=1 << 16, dtype=np.uint8)   # the fixed byte stream


def _stream(start, n):
    return np.take(_STREAM, np.arange(start, start + n) % _STREAM.size)


class _Builder:
    def __init__(self, op, elem_size=8, seed=0):
        self.op, self.es, self.rng = op, elem_size, np.random.default_rng(seed)
        self.chunks = {'in': [], 'out': []}
        self.size = {'in': 0, 'out': 0}
        self.count = {'in': 0, 'out': 0}
        self.expect, self.addr, self.start = [], [], {'in': [], 'out': []}
        self.recs, self.parents = [], []

    def _pattern(self, side, es, nbytes):
        c = self.count[side]
        self.count[side] += nbytes
        if es in (8, 16):
            k = np.arange(c // 8, c // 8 + nbytes // 8, dtype=np.float64)
            vals = SENTINEL * (1.0 + k * 2.0 ** -40) if side == 'out' else k + 1.0
            return vals.view(np.uint8).copy()
        if es == 4 and side == 'in':
            k = np.arange(c // 4 + 1, c // 4 + 1 + nbytes // 4, dtype=np.uint64)
            return ((k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.uint8).copy()
        return _stream(c + (7 if side == 'in' else 0), nbytes)

    def place(self, side, es, shape, strides, mis=0) -> View:
        """A parent for the strided view, its origin `mis` elements past a 16-byte boundary (modulo 16 bytes)."""
        shape, strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
        empty = any(n == 0 for n in shape)
        lo = 0 if empty else sum(min(0, (n - 1) * s) for n, s in zip(shape, strides))
        hi = 0 if empty else sum(max(0, (n - 1) * s) for n, s in zip(shape, strides))
        pad = max(4, 64 // es)
        origin = pad - lo
        while (origin - mis) * es % 16:
            origin += 1
        nbytes = -(-(origin + hi + 1 + pad) * es // 16) * 16
        chunk = self._pattern(side, es, nbytes)
        self.chunks[side].append(chunk)
        self.start[side].append(self.size[side])
        v = View(side, len(self.chunks[side]) - 1, origin * es, self.size[side] + origin * es, es, shape, strides)
        self.size[side] += nbytes
        if side == 'out':
            self.expect.append(chunk.copy())
            self.addr.append(np.zeros(nbytes, dtype=bool))
        return v

    def parent(self, v):
        return self.chunks[v.side][v.chunk]

    def wanted(self, v):
        """The reference image of a destination view, marked as addressed."""
        v.bytes(self.addr[v.chunk])[...] = True
        return self.expect[v.chunk]

    def add(self, dview: View, **rec):
        self.recs.append(rec)
        s = self.start['out'][dview.chunk]
        self.parents.append((s, s + self.chunks['out'][dview.chunk].size, dview.gbyte))

    def case(self) -> Case:
        def cat(chunks, dtype=np.uint8):
            return np.concatenate(chunks) if chunks else np.zeros(16, dtype)

        return Case(self.op, self.es, cat(self.chunks['in']), cat(self.chunks['out']), cat(self.expect), cat(self.addr, bool),
                    self.recs, self.parents)


# ---- runner and checker -----------------------------------------------------------------------------------------------

def run(case, launch, memory=None, launches=1):
    """Upload both arenas through `memory`, hand the filled descriptor arrays to `launch(op, arrays, elem_size)`
    (`launches` times) and return (ain, aout) after the call(s), as bytes."""
    memory = memory if memory is not None else HostMemory()
    base_in, base_out = memory.upload(case.ain.view(np.float64)), memory.upload(case.aout0.view(np.float64))
    arrays = case.descriptors(base_in, base_out)
    for _ in range(launches):
        launch(case.op, arrays, case.elem_size)
    return (memory.download(base_in, case.ain.size // 8).view(np.uint8), memory.download(base_out, case.aout0.size // 8).view(np.uint8))


@dataclass
class Report:
    interior: list      # (record, element offset from the destination's origin): addressed, but not the reference's bits
    sentinel: list      # (record, element offset from the destination's origin): a byte outside the addressed set changed
    source: list        # byte offsets into `ain` that changed
    n_bad: dict

    @property
    def clean(self):
        return not (self.interior or self.sentinel or self.source)

    def __str__(self):
        out = [f'{k}: {self.n_bad[k]} byte(s), first {v[0]}' for k, v in
               (('interior', self.interior), ('sentinel', self.sentinel), ('source', self.source)) if v]
        return '; '.join(out) if out else 'clean'


def check(case, got, expect=None) -> Report:
    """`got`: (ain, aout) after the call; `expect` replaces the stored image of aout (a call run twice)."""
    gin, gout = got
    want = case.expect if expect is None else expect
    starts = np.array([p[0] for p in case.parents]) if case.parents else np.zeros(0)

    def where(mask):
        bad = np.flatnonzero(mask)
        rows = []
        for b in bad[:4]:
            r = int(np.searchsorted(starts, b, side='right') - 1) if starts.size else -1
            rows.append((r, int(b - case.parents[r][2]) // case.elem_size if r >= 0 else int(b)))
        return rows, int(bad.size)

    interior, n_i = where((gout != want) & case.addressed)
    sentinel, n_s = where((gout != case.aout0) & ~case.addressed)
    src = np.flatnonzero(gin != case.ain)
    return Report(interior, sentinel, [int(b) for b in src[:4]], {'interior': n_i, 'sentinel': n_s, 'source': int(src.size)})


def view_only_ok(case, got):
    """What the wrapper-level tests compare today (tests/test_gpu_blockops.py and callers): the elements of the view they
    asked for, nothing around them -- kept to SHOW what that misses."""
    return bool(np.array_equal(got[1][case.addressed], case.expect[case.addressed]))


def cexpand_normwise_ok(case, got, tol=1e-10):
    """The only check the complex expansion has today: the complex GEMM behind it, `|got - ref| <= tol * max|ref|`
    (tests/test_gpu_gemm.py).  A = ones(1, 2K) real-interleaved times the expanded B, against the reference's."""
    for r in case.recs:
        K, N = r['K'], r['N']
        if K * N == 0:
            continue
        o = r['dst'][1]
        B = got[1][o:o + 32 * K * N].view(np.float64).reshape(2 * K, 2 * N)
        ref = case.expect[o:o + 32 * K * N].view(np.float64).reshape(2 * K, 2 * N)
        a = np.ones((3, 2 * K))
        if not np.abs(a @ B - a @ ref).max() <= tol * max(1.0, float(np.abs(a @ ref).max())):
            return False
    return True


# ---- numpy stand-in ---------------------------------------------------------------------------------------------------

class NumpyMove:
    """Evaluates the descriptor arrays through their strides on the parent buffers, a copy on the path `classify_copy`
    gives it.  `fault` (a dict with 'kind' in FAULT_KINDS and 'rec') makes it wrong in one of the ways these kernels can
    be wrong.  `classes` collects (elem_size, class, composite) of every copy record it ran."""

    def __init__(self, memory, fault=None):
        self.memory, self.fault, self.classes = memory, fault, []

    def _buf(self, addr):
        for arr in self.memory.arrays:
            d = addr - arr.ctypes.data
            if 0 <= d < arr.nbytes:
                return arr.view(np.uint8), d
        raise ValueError('address outside every uploaded buffer')

    def _f64(self, addr):
        b, o = self._buf(addr)
        if o % 8:
            raise ValueError('a double at an address that is no multiple of 8')
        return b.view(np.float64), o // 8

    def _move(self, dst, dof, src, so, es, conj=False):
        db, d0 = self._buf(dst)
        sb, s0 = self._buf(src)
        lane = np.arange(es)
        vals = sb[np.clip(s0 + np.asarray(so)[:, None] * es + lane, 0, sb.size - 1)]
        if conj:
            vals[:, 15] ^= 0x80
        db[d0 + np.asarray(dof)[:, None] * es + lane] = vals

    def __call__(self, op, arrays, es):
        f = self.fault or {}
        for i in range(arrays[1]):
            kind = f.get('kind') if f.get('rec') == i else None
            getattr(self, '_' + op.split('_')[0])(arrays, i, es, kind, op)

    def _copy(self, arrays, i, es, kind, op):
        d = arrays[0][i]
        nd = d.ndim
        shape, ds, ss = list(d.shape[:nd]), list(d.dst_strides[:nd]), list(d.src_strides[:nd])
        cls = classify_copy(shape, ds, ss, es, d.conj)
        self.classes.append((es, cls.name, cls.composite))
        if cls.name == 'empty':
            return
        conj = bool(d.conj) and kind != 'no_conj'
        if cls.tiled is not None:
            t = cls.tiled
            # the fault: i / n2 for both halves of a composite index (on the source side where D is one, else on S)
            bad_d = kind == 'composite_div' and t['nD2'] > 1
            bad_s = kind == 'composite_div' and not bad_d
            dI, sI = np.arange(t['nD'], dtype=np.int64), np.arange(t['nS'], dtype=np.int64)
            so_t = sI[:, None] + ((dI // t['nD2']) * t['ssD'] + (dI // t['nD2'] if bad_d else dI % t['nD2']) * t['ssD2'])[None, :]
            do_t = dI[None, :] + ((sI // t['nS2']) * t['dsS'] + (sI // t['nS2'] if bad_s else sI % t['nS2']) * t['dsS2'])[:, None]
            oshape = [a[0] for a in t['outer']]
            so = (_offsets(oshape, [a[2] for a in t['outer']])[:, None] + so_t.reshape(-1)[None, :]).reshape(-1)
            dof = (_offsets(oshape, [a[1] for a in t['outer']])[:, None] + do_t.reshape(-1)[None, :]).reshape(-1)
        else:
            ax = cls.axes
            nshape = [a[0] for a in ax]
            dof = _offsets(nshape, [a[1] for a in ax])
            so = _offsets(nshape, [a[1 if kind == 'src_at_dst_strides' else 2] for a in ax])
            if kind == 'odd_tail' and ax and ax[-1][0] % 2:
                keep = (np.arange(dof.size) % ax[-1][0]) != ax[-1][0] - 1
                dof, so = dof[keep], so[keep]
            if kind == 'past_row' and ax:
                dof = np.append(dof, dof[ax[-1][0] - 1] + ax[-1][1])
                so = np.append(so, so[ax[-1][0] - 1] + ax[-1][2])
        self._move(d.dst, dof, d.src, so, es, conj)

    def _mask(self, arrays, i, es, kind, scatter):
        d = arrays[0][i]
        small = d.outer * d.n_keep * d.inner
        if scatter and kind != 'scatter_no_zero' and d.outer * d.axis * d.inner:
            out, o0 = self._f64(d.out)
            out[o0:o0 + d.outer * d.axis * d.inner] = 0.0
        if small == 0:
            return
        ib, i0 = self._buf(d.idx)
        idx = ib[i0:i0 + 8 * d.n_keep].view(np.int64)
        e = np.arange(small, dtype=np.int64)
        t, inn = e // d.inner, e % d.inner
        big = ((t // d.n_keep) * d.axis + idx[t % d.n_keep]) * d.inner + inn
        if kind == 'odd_tail' and d.inner % 2:
            e, big = e[inn != d.inner - 1], big[inn != d.inner - 1]
        if kind == 'past_row':          # (after the LAST row: the small side is contiguous, every other row has a successor)
            e, big = np.append(e, e[-1] + 1), np.append(big, big[-1] + 1)
        if scatter:
            self._move(d.out, big, d.x, e, 8)
        else:
            self._move(d.out, e, d.x, big, 8)

    def _gather(self, arrays, i, es, kind, op):
        self._mask(arrays, i, es, kind, False)

    def _scatter(self, arrays, i, es, kind, op):
        self._mask(arrays, i, es, kind, True)

    def _scale(self, arrays, i, es, kind, op):
        d = arrays[0][i]
        n = d.outer * d.axis * d.inner
        if n == 0:
            return
        x, x0 = self._f64(d.x)
        fa, f0 = self._f64(d.f)
        out, o0 = self._f64(d.out)
        e = np.arange(n, dtype=np.int64)
        j = (e // d.inner) % d.axis
        if kind == 'j1_eq_j0' and d.x % 16 == 0 and d.out % 16 == 0:
            # the pair path: elements (e, e + 1) of an even e; the second one takes the factor of the first
            second = (e % 2 == 1) & ((e % ITEM) < (np.minimum(n - e // ITEM * ITEM, ITEM) // 2) * 2)
            j = np.where(second, j[np.maximum(e - 1, 0)], j)
        out[o0:o0 + n] = x[x0:x0 + n] * fa[f0 + j]

    def _cexpand(self, arrays, i, es, kind, op):
        d = arrays[0][i]
        if d.K * d.N == 0:
            return
        src, s0 = self._f64(d.src)
        dst, d0 = self._f64(d.dst)
        k, n = (a.reshape(-1) for a in np.meshgrid(np.arange(d.K), np.arange(d.N), indexing='ij'))
        b = s0 + 2 * (k * d.rs + n * d.cs)
        br, bi = src[b], src[b + 1]
        r0, r1 = d0 + (2 * k) * (2 * d.N) + 2 * n, d0 + (2 * k + 1) * (2 * d.N) + 2 * n
        dst[r0], dst[r0 + 1] = br, bi
        dst[r1], dst[r1 + 1] = (bi if kind == 'expand_sign' else -bi), br

    def _lincomb(self, arrays, i, es, kind, op):
        d = arrays[0][i]
        cplx = op == 'lincomb_c128'
        shape = list(d.shape[:d.ndim])
        if math.prod(shape) == 0:
            return
        dof = _offsets(shape, list(d.dst_strides[:d.ndim]))
        dst, d0 = self._f64(d.dst)
        w = 2 if cplx else 1

        def load(arr, base, off, real=False):
            return arr[base + off] + 0j if real else arr[base + 2 * off] + 1j * arr[base + 2 * off + 1]

        acc = np.zeros(dof.size, dtype=np.complex128 if cplx else np.float64)
        if d.accumulate:
            acc = load(dst, d0, dof) if cplx else dst[d0 + dof].copy()
        for k in range(d.term_begin, d.term_end):
            t = arrays[2][k]
            so = _offsets(shape, list((d.dst_strides if kind == 'src_at_dst_strides' else t.src_strides)[:d.ndim]))
            src, s0 = self._f64(t.src)
            if cplx:
                acc = acc + complex(t.coeff_re, t.coeff_im) * load(src, s0, so, bool(t.src_real))
            else:
                acc = acc + t.coeff * src[s0 + so]
        if cplx:
            dst[d0 + w * dof], dst[d0 + w * dof + 1] = acc.real, acc.imag
        else:
            dst[d0 + dof] = acc


# ---- case builders: copy ----------------------------------------------------------------------------------------------

def _copy_rec(b, shape, ds, ss, mis_d=0, mis_s=0, conj=0, tag=''):
    """One copy record with a reference written through numpy views."""
    es = b.es
    dst, src = b.place('out', es, shape, ds, mis_d), b.place('in', es, shape, ss, mis_s)
    vals = src.bytes(b.parent(src)).copy()
    if conj:
        vals[..., 15] ^= 0x80
    dst.bytes(b.wanted(dst))[...] = vals
    b.add(dst, dst=dst.ptr, src=src.ptr, conj=conj, shape=list(shape), ds=list(ds), ss=list(ss), tag=tag)


ROW_LENGTHS = (15, 16, 17, 255, 256, 257, 2047, 2048, 2049)


def copy_row_case(es, seed=1) -> Case:
    """Unit stride on both sides of the last axis: every inner length around the thresholds of the row path (15 stays
    elementwise; 256: the 4 x 64 unroll; 2048: the waves share a row) with odd leading dimensions, every start parity of
    source and destination (8 bytes: aligned, peel, 8-byte run), one record above 8192 elements whose rows do not divide
    an item, a 3-d record with permuted outer axes and one with a negative leading stride on either side."""
    b = _Builder('copy', es, seed)
    per16 = 16 // es
    starts = [(0, 0), (1, 1), (0, 1), (1, 0)] if per16 > 1 else [(0, 0)]
    for L in ROW_LENGTHS:
        for md, ms in starts:
            _copy_rec(b, (3, L), (_odd_above(L) + 2, 1), (_odd_above(L), 1), md, ms, tag=f'{L}')
            if es == 8 and L in (16, 17, 256, 257):     # even leading dimensions: every row of the record has that parity
                _copy_rec(b, (3, L), (L + 4 + L % 2, 1), (L + 2 + L % 2, 1), md, ms, tag=f'{L} even ld')
    _copy_rec(b, (37, 257), (259, 1), (261, 1), 1, 0, tag='items end mid-row')
    _copy_rec(b, (3, 4, 33), (4 * 35, 35, 1), (37, 3 * 37, 1), 0, 1 % per16, tag='3-d permuted')
    _copy_rec(b, (5, 20), (23, 1), (-21, 1), tag='negative source stride')
    _copy_rec(b, (5, 20), (-23, 1), (21, 1), tag='negative destination stride')
    _copy_rec(b, (4, 5, 6), (30, 6, 1), (30, 6, 1), 1 % per16, 0, tag='axes merge into one row')
    return b.case()


def copy_elementwise_case(es, seed=2) -> Case:
    """The per-element path: a short inner axis, non-unit last strides, conj over a long unit-stride axis (16 bytes),
    ndim 0 and 8, singleton, merging and empty axes, a broadcast read, negative leading strides."""
    b = _Builder('copy', es, seed)
    _copy_rec(b, (5, 15), (17, 1), (19, 1), tag='inner below 16')
    _copy_rec(b, (7, 9), (20, 2), (30, 3), 1 % (16 // es), 0, tag='non-unit last stride')
    _copy_rec(b, (), (), (), tag='ndim 0')
    _copy_rec(b, (2,) * 8, tuple(2 * s for s in _c_strides((3,) * 8)), tuple(3 * s for s in reversed(_c_strides((2,) * 8))), tag='ndim 8')
    _copy_rec(b, (1, 5, 1, 6), (99, 14, 7, 2), (1, 3, 5, 15), tag='singleton axes')
    _copy_rec(b, (4, 5), (10, 2), (15, 3), tag='axes merge')
    _copy_rec(b, (3, 0, 4), (8, 4, 1), (8, 4, 1), tag='zero extent')
    _copy_rec(b, (6, 7), (9, 1), (0, 1), tag='broadcast read')
    _copy_rec(b, (5, 7), (9, 1), (-11, 1), tag='negative source stride')
    _copy_rec(b, (5, 7), (-9, 1), (11, 1), tag='negative destination stride')
    _copy_rec(b, (2, 9000), (18001, 2), (27001, 3), tag='more than one item')
    if es == 16:
        _copy_rec(b, (3, 40), (43, 1), (41, 1), conj=1, tag='conj long rows')
        _copy_rec(b, (2, 2100), (2101, 1), (2103, 1), conj=1, tag='conj rows of 2048 and more')
    return b.case()


TILE_EXTENTS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
# (shape of a contiguous source, permutation): tests/test_gpu_blockops.py::test_permutations_with_short_inner_axes
SHORT_AXIS_PERMUTES = [((2, 5, 37, 41, 2), (3, 4, 0, 2, 1)), ((5, 2, 2, 33, 29), (1, 2, 3, 4, 0)), ((29, 3, 33, 5), (2, 3, 0, 1)),
                       ((7, 3, 40, 2), (3, 2, 1, 0)), ((4, 50, 3), (2, 1, 0)), ((3, 70, 4, 5), (1, 3, 0, 2)), ((17, 2, 19, 3), (2, 3, 0, 1)),
                       ((2, 2, 2, 2, 2, 2, 2, 2), (7, 6, 5, 4, 3, 2, 1, 0)), ((64, 5, 65), (2, 1, 0)), ((130, 6), (1, 0)), ((6, 130), (1, 0))]


def copy_transpose_case(es, aligned=True, conj=0, seed=3) -> Case:
    """The unit-stride axes of source (S, axis 0) and destination (D, axis 1) differ: every pair of extents around the tile
    edges (an extent of 15 falls back to the per-element path: tiled and strided records in ONE call), with and without
    outer axes; 129 x 129 is more tiles than one item holds, with a ragged last item.  `aligned`: even leading dimensions
    and aligned starts (the 16-byte accesses of the 64 x 64 kernel), else odd ones (its scalar fallback in both phases)."""
    b = _Builder('copy', es, seed)
    mis = 0 if aligned else 1 % (16 // es)
    for nS in TILE_EXTENTS:
        for nD in TILE_EXTENTS:
            ld_s, ld_d = (nS + 2 + nS % 2, nD + 4 + nD % 2) if aligned else (_odd_above(nS), _odd_above(nD) + 2)
            _copy_rec(b, (nS, nD), (ld_d, 1), (1, ld_s), mis, mis, conj, tag=f'{nS}x{nD}')
    for nS, nD in ((17, 33), (64, 15), (33, 65), (65, 16)):
        ld_s, ld_d = (nS + 2 + nS % 2, nD + 4 + nD % 2) if aligned else (_odd_above(nS), _odd_above(nD) + 2)
        _copy_rec(b, (3, nS, 2, nD), (nS * 2 * ld_d, 2 * ld_d, ld_d, 1), (ld_s * nD, 1, 3 * ld_s * nD, ld_s), mis, mis, conj,
                  tag=f'outer {nS}x{nD}')
    return b.case()


def copy_composite_case(es, conj=0, seed=4) -> Case:
    """Leg rotations with short innermost axes: a short unit-stride axis of the destination with a partner, of the source
    with a partner, both at once, and short axes without a partner -- into a contiguous destination and into the interior
    of a larger one (gaps on every axis)."""
    b = _Builder('copy', es, seed)
    for shape, perm in SHORT_AXIS_PERMUTES:
        ss = tuple(_c_strides(shape)[p] for p in perm)
        pshape = tuple(shape[p] for p in perm)
        _copy_rec(b, pshape, _c_strides(pshape), ss, 0, 0, conj, tag=f'{shape} {perm}')
        _copy_rec(b, pshape, _c_strides(tuple(n + 1 for n in pshape)), ss, 1 % (16 // es), 0, conj, tag=f'{shape} {perm} into a larger block')
    # the three composite forms on their own, with gaps on the side that is not flattened, plain and under an outer axis:
    # (partner 20, S 3, D 40), (S 40, partner 20, D 3), (partner 20, S 3, partner 18, D 4)
    for outer in ((), (2,)):
        for tag, shape, ds, ss in (('composite S', (20, 3, 40), (45, 907, 1), (3, 1, 61)),
                                   ('composite D', (40, 20, 3), (61, 3, 1), (1, 45, 907)),
                                   ('composite S and D', (20, 3, 18, 4), (221, 73, 4, 1), (3, 1, 247, 61))):
            top_d = 1 + sum((n - 1) * d for n, d in zip(shape, ds)) + 3
            top_s = 1 + sum((n - 1) * d for n, d in zip(shape, ss)) + 2
            _copy_rec(b, outer + shape, tuple(top_d for _ in outer) + ds, tuple(top_s for _ in outer) + ss, 0, 1 % (16 // es), conj,
                      tag=tag + (' under an outer axis' if outer else ''))
    return b.case()


def copy_cases():
    """name -> builder of every copy case of the device test."""
    out = {}
    for es in (1, 4, 8, 16):
        out[f'row es{es}'] = lambda es=es: copy_row_case(es)
        out[f'elementwise es{es}'] = lambda es=es: copy_elementwise_case(es)
        out[f'transpose es{es} aligned'] = lambda es=es: copy_transpose_case(es, True)
        out[f'composite es{es}'] = lambda es=es: copy_composite_case(es)
    out['transpose es8 odd'] = lambda: copy_transpose_case(8, False)
    out['transpose es4 odd'] = lambda: copy_transpose_case(4, False)
    out['transpose es16 conj'] = lambda: copy_transpose_case(16, True, 1)
    out['composite es16 conj'] = lambda: copy_composite_case(16, 1)
    return out


def negative_stride_case(es=8) -> Case:
    """Negative strides alone, on every kernel class (the header allows them)."""
    b = _Builder('copy', es, 5)
    _copy_rec(b, (5, 20), (23, 1), (-21, 1), tag='row, source')
    _copy_rec(b, (5, 20), (-23, 1), (21, 1), tag='row, destination')
    _copy_rec(b, (3, 33, 40), (33 * 41, 41, 1), (-40 * 35, 1, 35), tag='tiled, outer source')
    _copy_rec(b, (3, 33, 40), (-33 * 41, 41, 1), (40 * 35, 1, 35), tag='tiled, outer destination')
    _copy_rec(b, (33, 40), (41, 1), (1, -35), tag='tiled, source stride of D')
    _copy_rec(b, (6, 7), (-9, 1), (-11, 1), tag='elementwise, both')
    return b.case()


# ---- case builders: mask ----------------------------------------------------------------------------------------------

MASK_INNER = (1, 2, 3, 15, 16, 17, 64, 257)
MASK_AXIS = 9
MASK_KEPT = {'none': [], 'one': [4], 'all': list(range(MASK_AXIS)), 'first and last': [0, 3, 4, 8],
             'unsorted': [8, 0, 5, 3], 'repeated': [2, 2, 8, 0, 2]}


def _mask_rec(b, scatter, outer, axis, inner, kept, mis_x=0, mis_o=0, tag=''):
    nk = len(kept)
    big_shape, small_shape = (outer, axis, inner), (outer, nk, inner)
    xs, os_ = (small_shape, big_shape) if scatter else (big_shape, small_shape)
    x = b.place('in', 8, xs, _c_strides(xs), mis_x)
    out = b.place('out', 8, os_, _c_strides(os_), mis_o)
    idx = b.place('in', 8, (nk,), (1,))
    idx.bytes(b.parent(idx)).view(np.int64)[..., 0][...] = kept
    xa = x.f64(b.parent(x))
    xa[..., ::3] = -xa[..., ::3]                  # both signs; the values stay unique
    want = out.f64(b.wanted(out))
    if scatter:
        want[...] = 0.0
        want[:, kept, :] = xa
    else:
        want[...] = xa[:, kept, :]
    b.add(out, x=x.ptr, out=out.ptr, idx=idx.ptr, outer=outer, axis=axis, inner=inner, n_keep=nk, tag=tag)


def mask_case(scatter, seed=6) -> Case:
    """(outer, axis, inner) blocks with inner through the row path (inner >= 16: aligned, peeled and 8-byte rows) and the
    32-bit path; no, one, all and first-and-last kept positions; gathers also with unsorted and repeated indices; two
    records above 8192 small-side elements (items end mid-row, and inside a 32-bit run)."""
    b = _Builder('scatter' if scatter else 'gather', 8, seed)
    k = 0
    for inner in MASK_INNER:
        for outer in (1, 3):
            for name, kept in MASK_KEPT.items():
                if scatter and name in ('unsorted', 'repeated'):
                    continue
                for mx, mo in ([(0, 0), (1, 1), (0, 1)] if inner >= 16 else [((k // 2) % 2, k % 2)]):
                    _mask_rec(b, scatter, outer, MASK_AXIS, inner, kept, mx, mo, tag=f'inner {inner} outer {outer} {name}')
                k += 1
    rng = np.random.default_rng(seed)
    _mask_rec(b, scatter, 3, 40, 257, sorted(rng.permutation(40)[:31].tolist()), 1, 0, tag='rows across items')
    _mask_rec(b, scatter, 1, 4000, 3, sorted(rng.permutation(4000)[:3001].tolist()), 0, 1, tag='32-bit run across items')
    return b.case()


# ---- case builders: scale_axis ----------------------------------------------------------------------------------------

SCALE_SHAPES = [(1, 1, 1), (3, 5, 1), (2, 3, 7), (4, 9, 5), (2, 1, 33), (3, 4, 16), (3, 41, 69)]   # the last: 8487 elements, odd inner


def scale_case(in_place=False, seed=7) -> Case:
    """Every shape with x and out both 16-byte aligned (the pair path), x odd, out odd, both odd -- or in place
    (out == x: aligned, odd).  Data and factors include -0.0 and +0.0.  Reference: x * f in float64."""
    b = _Builder('scale', 8, seed)
    rng = b.rng
    for outer, axis, inner in SCALE_SHAPES:
        shape = (outer, axis, inner)
        for mx, mo in ([(0, 0), (1, 1)] if in_place else [(0, 0), (1, 0), (0, 1), (1, 1)]):
            data = rng.standard_normal(shape)
            data.reshape(-1)[::5] = -0.0
            data.reshape(-1)[3::7] = 0.0
            fac = rng.standard_normal(axis)
            if axis > 2:
                fac[axis - 1], fac[1] = -0.0, -2.0
            f = b.place('in', 8, (axis,), (1,), (mx + mo) % 2)
            f.f64(b.parent(f))[...] = fac
            out = b.place('out', 8, shape, _c_strides(shape), mo)
            x = out if in_place else b.place('in', 8, shape, _c_strides(shape), mx)
            x.f64(b.parent(x))[...] = data
            out.f64(b.wanted(out))[...] = data * fac[None, :, None]
            b.add(out, x=x.ptr, f=f.ptr, out=out.ptr, outer=outer, axis=axis, inner=inner, tag=f'{shape} x{mx} out{mo}', fac=fac, data=data)
    return b.case()


def scale_twice_expect(case):
    """What an in-place case holds after the same call ran twice: (x * f) * f, each product rounded."""
    want = case.expect.copy()
    for r in case.recs:
        o = r['out'][1]
        n = r['data'].size
        want[o:o + 8 * n] = ((r['data'] * r['fac'][None, :, None]) * r['fac'][None, :, None]).reshape(-1).view(np.uint8)
    return want


# ---- case builders: complex expansion ---------------------------------------------------------------------------------

CEXPAND_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 29), (0, 4), (4, 0)]


def _cexpand_rec(b, K, N, layout, tag='', real=False):
    rs, cs = {'row-major': (N, 1), 'transposed': (1, K), 'sub-view': (N + 5, 1)}[layout]
    src = b.place('in', 16, (K, N), (rs, cs))
    dst = b.place('out', 8, (2 * K, 2 * N), (2 * N, 1))
    z = src.c128(b.parent(src))
    if K * N:
        im = z.imag.copy()
        im.reshape(-1)[::3] = 0.0                 # imaginary parts of +0.0 and -0.0: row 2k + 1 holds -0.0 and +0.0
        im.reshape(-1)[1::3] = -0.0
        im[(K - 1) // 2, (N - 1) // 2] = -im[(K - 1) // 2, (N - 1) // 2]
        if real:                                  # a real matrix promoted to complex128: every imaginary part a zero
            im[...] = np.where(np.arange(K * N).reshape(K, N) % 2, -0.0, 0.0)
        z.imag[...] = im
        z.real[..., ::2] = -z.real[..., ::2]
    want = dst.f64(b.wanted(dst))
    want[0::2, 0::2], want[0::2, 1::2] = z.real, z.imag
    want[1::2, 0::2], want[1::2, 1::2] = -z.imag, z.real
    b.add(dst, src=src.ptr, rs=rs, cs=cs, K=K, N=N, dst=dst.ptr, tag=tag or f'{K}x{N} {layout}')


def cexpand_case(seed=8) -> Case:
    """Every (K, N) in every source layout; 38 more descriptors and one of 257 x 257 (above the 65536 elements of one
    item: an item ends inside it).  Destinations are 16-byte aligned, contiguous and guarded on both sides."""
    b = _Builder('cexpand', 8, seed)
    for K, N in CEXPAND_SHAPES:
        for layout in ('row-major', 'transposed', 'sub-view'):
            _cexpand_rec(b, K, N, layout)
    for k in range(38):
        _cexpand_rec(b, 3 + k % 5, 2 + k % 7, ('row-major', 'transposed', 'sub-view')[k % 3])
    _cexpand_rec(b, 257, 257, 'transposed')
    return b.case()


def cexpand_real_case(seed=10) -> Case:
    """Real matrices promoted to complex128 (what `_complex_gemm` gets for a real B beside a complex A): every imaginary
    part is +0.0 or -0.0, so that the sign of row 2k + 1 shows in the sign bits alone."""
    b = _Builder('cexpand', 8, seed)
    for K, N in ((5, 3), (33, 29), (1, 7)):
        for layout in ('row-major', 'transposed', 'sub-view'):
            _cexpand_rec(b, K, N, layout, f'{K}x{N} {layout} real', real=True)
    return b.case()


def cexpand_misaligned(case, which):
    """The descriptors of `case` for aligned arenas, with the first non-empty record's `which` pointer 8 bytes further."""
    def descs(base_in, base_out):
        arr, n = case.descriptors(base_in, base_out)
        i = next(i for i, r in enumerate(case.recs) if r['K'] * r['N'])
        setattr(arr[i], which, getattr(arr[i], which) + 8)
        return arr, n
    return descs


# ---- case builders: strided linear combination ------------------------------------------------------------------------

LINCOMB_SHAPES = [(), (23,), (3, 4, 5, 6), (2,) * 8, (10, 9, 11, 10)]          # the last: 9900 elements, two items


def lincomb_case(cplx, seed=9) -> Case:
    """dst = (accumulate ? dst : 0) + sum_t c_t src_t with 0, 1 and 3 terms, accumulate 0 and 1, destinations with gaps on
    every axis, sources with permuted strides, ndim 0, 1, 4 and 8; complex: real sources beside complex ones.  Data are
    the unique integers of the arenas times 2^-3 .. 2^3 per operand, coefficients +-2^k (complex: Gaussian integers times
    2^k): every partial sum is an integer multiple of 2^-5 below 2^40, exact in any order and with or without fused
    multiply-adds."""
    b = _Builder('lincomb_c128' if cplx else 'lincomb_f64', 16 if cplx else 8, seed)
    rng = b.rng
    es = b.es
    coeffs = [1.0, -2.0, 0.5, -0.25, 4.0]
    ccoeffs = [1.0 + 0j, -2.0j, 0.5 - 0.5j, -1.0 + 2.0j, 0.25j]
    k = 0
    for shape in LINCOMB_SHAPES:
        for n_terms in (0, 1, 3):
            for accumulate in (0, 1):
                nd = len(shape)
                ds = _c_strides(tuple(n + 1 for n in shape)) if nd <= 4 else tuple(2 * s for s in _c_strides(shape))
                dst = b.place('out', es, shape, ds, 0 if cplx else k % 2)
                d0 = (dst.c128 if cplx else dst.f64)(b.parent(dst))
                own = np.arange(d0.size, dtype=np.float64).reshape(shape)                   # unique integers, no zeros
                d0[...] = (own + 11.0) - 1j * (own + 500009.0) if cplx else -(own + 11.0)
                acc = d0.copy() if accumulate else np.zeros(shape, dtype=d0.dtype)
                terms = []
                for t in range(n_terms):
                    perm = tuple(rng.permutation(nd).tolist())
                    pshape = tuple(shape[p] for p in perm)
                    base = _c_strides(tuple(n + (t % 2) for n in pshape))
                    ss = tuple(base[perm.index(a)] for a in range(nd))
                    real = cplx and t == 1
                    src = b.place('in', 8 if (real or not cplx) else 16, shape, ss, (k + t) % 2 if (real or not cplx) else 0)
                    sa = (src.f64 if (real or not cplx) else src.c128)(b.parent(src))
                    sa[...] = sa * 2.0 ** int(rng.integers(-3, 4))
                    c = (ccoeffs if cplx else coeffs)[(k + t) % 5]
                    acc = acc + c * sa
                    terms.append(dict(src=src.ptr, coeff=c, src_real=int(real), ss=list(ss)))
                (dst.c128 if cplx else dst.f64)(b.wanted(dst))[...] = acc
                b.add(dst, dst=dst.ptr, accumulate=accumulate, shape=list(shape), ds=list(ds), terms=terms,
                      tag=f'{shape} terms {n_terms} acc {accumulate}')
                k += 1
    return b.case()


def all_cases():
    """name -> builder of every case of the device test, by group."""
    groups = {'copy': copy_cases()}
    groups['copy']['negative strides'] = negative_stride_case
    groups['mask'] = {'gather': lambda: mask_case(False), 'scatter': lambda: mask_case(True)}
    groups['scale'] = {'out of place': lambda: scale_case(False), 'in place': lambda: scale_case(True)}
    groups['cexpand'] = {'all': cexpand_case, 'promoted real': cexpand_real_case}
    groups['lincomb'] = {'f64': lambda: lincomb_case(False), 'c128': lambda: lincomb_case(True)}
    return groups


def copy_coverage(names=None):
    """{(elem_size, class): [case names]} and {(elem_size, 'composite'): [...]} over the copy cases, from the classification
    alone: a threshold that moves in csrc/copy_kernels.h without this mirror shows as a stand-in mismatch, one that moves
    in both as a class no case reaches."""
    cover = {}
    for name, build in copy_cases().items():
        if names is not None and name not in names:
            continue
        case = build()
        for r in case.recs:
            c = classify_copy(r['shape'], r['ds'], r['ss'], case.elem_size, r['conj'])
            cover.setdefault((case.elem_size, c.name), set()).add(name)
            if c.composite:
                form = 'composite ' + ' and '.join(x for x, n2 in (('S', c.tiled['nS2']), ('D', c.tiled['nD2'])) if n2 > 1)
                for key in ('composite', form):
                    cover.setdefault((case.elem_size, key), set()).add(name)
    return {k: sorted(v) for k, v in cover.items()}
