"""Guard-band cases for the batched decompositions at the C ABI (cyb_{svd,eigh,qr}_batched_f64, the two _ex_f64 entries
with their flags, the three _c128 entries): builder, runner, checker, route mirror and a numpy stand-in, all on the host
(no device, no torch), after the pattern of tests/gemm_guard_cases.py and tests/move_guard_cases.py, whose SENTINEL,
HostMemory and _odd_above are used here; the measures are those of tests/decomp_accuracy_cases.py.

Arenas.  A case is ONE call of one entry: a descriptor list (SvdDesc / EighDesc / QrDesc of cyten_amd._lib) over an input
arena `ain` (every A) and an output arena `aout0` (every U, S, Vh, W, V, Q, R).  Every matrix is a view with a parent of its
own: at least 64 bytes before and after it; a float64 view starts on an ODD float64 element of its 16-byte aligned parent
(8-byte but not 16-byte aligned) and has an odd leading dimension above its extent; a complex view is 16-byte aligned, its
leading dimension odd, counted in complex elements.  S and W are contiguous vectors between the same guards.  A parent of
`aout0` is pre-filled with the distinct finite doubles SENTINEL * (1 + k 2^-40); a parent of `ain` with the unique finite
values k + 1 -- or, in the NaN variant (`ain_nan`), with NaN in every gap and guard byte: a kernel that reads outside a view
then makes the block a "NaN block" (info = -1, CYB_ERR_NOCONV) or poisons its result.

Checks (`check`); every one must hold:
  sentinel   a byte of `aout0` outside the addressed elements changed (the gaps between rows included),
  source     a byte of the input arena changed ("A is not modified": range-scaled blocks too),
  twin       an addressed element differs, bit for bit, from the result of the SAME list (same order, same flags) decomposed
             from contiguous, 16-byte aligned copies in the same process; status, info and rank are compared too.  Under
             CYB_SVD_SKIP_NULL_VECTORS the vectors beyond rank[i] are unspecified (they may stay unwritten, and an unwritten
             element holds the sentinel of its own arena): the comparison covers the first rank[i] vectors and all of S,
  measure    orth and resid of decomp_accuracy_cases at its CAP (1e-13) on the strided result, and `values` against LAPACK at
             the same cap for the standard_normal blocks (LAPACK itself stays below 24 EPS on these sizes),
  structure  exactly: the strict lower triangle of R and rows k .. m-1 of a full R are +0.0 bitwise; S descending, W
             ascending; every value of an embedded result twice.

`NumpyDecomp`, the stand-in for the device, evaluates the filled descriptor arrays with LAPACK by index arithmetic through
the leading dimensions; `fault` makes it wrong in one of the ways of FAULT_KINDS.  `routes` mirrors svd_split_list
(csrc/svd_plan.h) and the thresholds of the other entries; `source_constants` reads the constants it copies back from the
sources."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np

import decomp_accuracy_cases as dac
from cyten_amd import _lib
from gemm_guard_cases import SENTINEL, HostMemory, _odd_above   # noqa: F401  (HostMemory: re-exported for the model test)

CYB_OK, CYB_ERR_INVALID, CYB_ERR_NOCONV = 0, 1, 3
SKIP_NULL, EMBEDDED = 1, 2                  # CYB_SVD_SKIP_NULL_VECTORS, CYB_{SVD,EIGH}_EMBEDDED_COMPLEX
ENTRY = {'svd': 'cyb_svd_batched_f64', 'svd_ex': 'cyb_svd_batched_ex_f64', 'eigh': 'cyb_eigh_batched_f64',
         'eigh_ex': 'cyb_eigh_batched_ex_f64', 'qr': 'cyb_qr_batched_f64', 'csvd': 'cyb_svd_batched_c128',
         'ceigh': 'cyb_eigh_batched_c128', 'cqr': 'cyb_qr_batched_c128'}
FAULT_KINDS = ('ld_as_extent', 'lda_as_n', 'cols_to_32', 'rows_to_32', 's_pad_64', 'transposed', 'scale_in_place',
               'r_lower_unwritten', 'gap_read')
# the check every mutant must fail (it may fail others too)
FAULT_FLAGGED_AS = {'ld_as_extent': 'sentinel', 'lda_as_n': 'twin', 'cols_to_32': 'sentinel', 'rows_to_32': 'sentinel',
                    's_pad_64': 'sentinel', 'transposed': 'measure', 'scale_in_place': 'source', 'r_lower_unwritten': 'structure',
                    'gap_read': 'twin'}

# ---- the route mirror -------------------------------------------------------------------------------------------------
SMALL_MAXN, SMALL_MAXM = 64, 128            # svd_small.hip / csvd_small.hip: MAXN, MAXM
SMALL_LIST_MIN = 16                         # svd_split_list: the in-LDS kernel for a mixed list from 16 fitting blocks
PIPELINE_MIN, PIPELINE_MIN_EMBEDDED = 2, 1  # svd_split_list: large_min
EIGH_SMALL_MAX = 64                         # eigh_batched_impl: the in-LDS route only if every n <= 64
QR_BLOCKED_MIN = 96                         # qr_householder.hip: kBlockedMin
CSVD_LDS_BUDGET = 150 * 1024                # csvd_small.hip: LDS_BUDGET
CQR_SINGLE_ELEMS = 96 * 96                  # cqr_house.hip: kSingleElems
XPOSE_TILE = 32                             # the transposing write-outs tile at 32


def svd_small_fits(m, n):
    return 1 <= min(m, n) <= SMALL_MAXN and max(m, n) <= SMALL_MAXM


def csvd_small_fits(m, n):
    """fits of csvd_small.hip: the real limits and the LDS bound of the header."""
    M, N = max(m, n), min(m, n)
    Np = (N + 1) & ~1
    return svd_small_fits(m, n) and 16 * (Np * (M | 1) + Np * (Np | 1)) <= CSVD_LDS_BUDGET


def routes(kind, shapes, flags=0, full=0):
    """The route of every block of one list: 'empty' for a zero extent, else
    svd / svd_ex: 'tiny' | 'pipeline' | 'direct' (svd_split_list); eigh / eigh_ex: 'small' | 'jacobi';
    qr: 'unblocked' | 'blocked'; csvd / ceigh / cqr: 'small' | 'large'."""
    live = [(m, n) for m, n in shapes if m > 0 and n > 0]
    if kind in ('svd', 'svd_ex'):
        embedded = bool(flags & EMBEDDED)
        n_fit = sum(svd_small_fits(m, n) for m, n in live)
        use_small = not embedded and (n_fit == len(live) or n_fit >= SMALL_LIST_MIN)
        large_min = PIPELINE_MIN_EMBEDDED if embedded else PIPELINE_MIN

        def one(m, n):
            return 'tiny' if use_small and svd_small_fits(m, n) else 'pipeline' if min(m, n) >= large_min else 'direct'
    elif kind in ('eigh', 'eigh_ex'):
        all_small = bool(live) and not (flags & EMBEDDED) and all(n <= EIGH_SMALL_MAX for _, n in live)

        def one(m, n):
            return 'small' if all_small else 'jacobi'
    elif kind == 'qr':
        def one(m, n):
            return 'blocked' if min(m, n) >= QR_BLOCKED_MIN else 'unblocked'
    elif kind in ('csvd', 'ceigh'):
        def one(m, n):
            return 'small' if csvd_small_fits(m, n) else 'large'
    elif kind == 'cqr':
        def one(m, n):
            return 'small' if m * max(n, m if full else min(m, n)) <= CQR_SINGLE_ELEMS else 'large'
    else:
        raise ValueError(kind)
    return ['empty' if m == 0 or n == 0 else one(m, n) for m, n in shapes]


def source_constants(csrc=None):
    """The constants the mirror copies, read back from the sources: {name: value}."""
    csrc = csrc or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cyten_amd', 'csrc')

    def grab(name, pattern):
        with open(os.path.join(csrc, name)) as f:
            m = re.search(pattern, f.read())
        if m is None:
            raise AssertionError(f'{name}: no match for {pattern!r}')
        return [int(g) for g in m.groups()]

    out = {}
    out['SMALL_MAXN'], out['SMALL_MAXM'] = grab('svd_small.hip', r'constexpr int MAXN = (\d+), MAXM = (\d+);')
    out['CSMALL_MAXN'], out['CSMALL_MAXM'] = grab('csvd_small.hip', r'constexpr int MAXN = (\d+), MAXM = (\d+);')
    out['SMALL_LIST_MIN'], = grab('svd_plan.h', r'n_fit == blocks\.size\(\) \|\| n_fit >= (\d+)\)')
    out['PIPELINE_MIN_EMBEDDED'], _, out['PIPELINE_MIN'] = grab('svd_plan.h', r'large_min = embedded \? (\d+) : sw\.nomerge \? (\d+) : (\d+);')
    out['EIGH_SMALL_MAX'], = grab('svd_jacobi.hip', r'all_small = all_small && d\.n <= (\d+);')
    out['QR_BLOCKED_MIN'], = grab('qr_householder.hip', r'kBlockedMin = (\d+);')
    a, b = grab('csvd_small.hip', r'LDS_BUDGET = (\d+) \* (\d+);')
    out['CSVD_LDS_BUDGET'] = a * b
    a, b = grab('cqr_house.hip', r'kSingleElems = (\d+) \* (\d+);')
    out['CQR_SINGLE_ELEMS'] = a * b
    out['XPOSE_TILE'], _ = grab('svd_jacobi.hip', r'__shared__ double tile\[(\d+)\]\[(\d+)\];')
    return out


# ---- arenas and views -------------------------------------------------------------------------------------------------

@dataclass
class Mat:
    side: str                 # 'in' | 'out'
    gbyte: int                # byte offset of element (0, 0) inside its arena
    rows: int
    cols: int
    ld: int                   # in elements
    es: int                   # 8 | 16
    parent: tuple             # [start, end) of its parent in the arena

    def view(self, arena):
        """rows x cols float64 / complex128 view over `arena` (uint8)."""
        dt = np.float64 if self.es == 8 else np.complex128
        if self.rows == 0 or self.cols == 0:
            return np.zeros((self.rows, self.cols), dt)
        flat = arena[self.gbyte:self.parent[1]]
        flat = flat[:flat.size // self.es * self.es].view(dt)
        return np.lib.stride_tricks.as_strided(flat, (self.rows, self.cols), (self.ld * self.es, self.es))

    def mark(self, mask):
        if self.rows and self.cols:
            e = (np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]).reshape(-1) * self.es + self.gbyte
            mask[(e[:, None] + np.arange(self.es)[None, :]).reshape(-1)] = True


@dataclass
class Block:
    m: int
    n: int
    a: np.ndarray             # the input, contiguous
    A: Mat
    out: dict                 # name -> Mat | None: U S Vh / W V / Q R
    full: int = 0
    values: bool = False      # hold `values` against LAPACK (standard_normal data)
    tag: str = ''


@dataclass
class Case:
    name: str
    kind: str                 # key of ENTRY
    flags: int
    want_rank: bool
    strided: bool
    ain: np.ndarray           # uint8: finite gaps
    ain_nan: np.ndarray       # uint8: NaN in every gap and guard byte
    aout0: np.ndarray         # uint8, before the call
    addressed: np.ndarray     # bool per byte of aout0
    blocks: list = field(default_factory=list)
    expect_routes: list = field(default_factory=list)

    @property
    def cplx(self):
        return self.kind in ('csvd', 'ceigh', 'cqr')

    @property
    def family(self):
        return 'qr' if self.kind in ('qr', 'cqr') else 'eigh' if self.kind in ('eigh', 'eigh_ex', 'ceigh') else 'svd'

    def shapes(self):
        return [(b.m, b.n) for b in self.blocks]

    def routes(self):
        return routes(self.kind, self.shapes(), self.flags, self.blocks[0].full if self.blocks else 0)

    def descriptors(self, base_in, base_out):
        """The filled ctypes array of the call for arenas at the byte addresses `base_in` / `base_out`."""
        if base_in % 16 or base_out % 16:
            raise ValueError('guard cases need 16-byte aligned arenas')
        base = {'in': base_in, 'out': base_out}

        def at(mat):
            return None if mat is None else base[mat.side] + mat.gbyte

        def ld(mat):
            return 0 if mat is None else mat.ld

        fam = self.family
        arr = ({'svd': _lib.SvdDesc, 'eigh': _lib.EighDesc, 'qr': _lib.QrDesc}[fam] * max(len(self.blocks), 1))()
        for d, b in zip(arr, self.blocks):
            d.A, d.lda, d.n = at(b.A), b.A.ld, b.n
            o = b.out
            if fam == 'svd':
                d.m, d.U, d.ldu, d.S, d.Vh, d.ldvh = b.m, at(o['U']), ld(o['U']), at(o['S']), at(o['Vh']), ld(o['Vh'])
            elif fam == 'eigh':
                d.W, d.V, d.ldv = at(o['W']), at(o['V']), ld(o['V'])
            else:
                d.m, d.Q, d.ldq, d.R, d.ldr, d.full = b.m, at(o['Q']), ld(o['Q']), at(o['R']), ld(o['R']), b.full
        return arr


class _Builder:
    def __init__(self, name, kind, flags=0, want_rank=False, strided=True):
        self.name, self.kind, self.flags, self.want_rank, self.strided = name, kind, flags, want_rank, strided
        self.chunks = {'in': [], 'out': []}
        self.nan_chunks = []
        self.size = {'in': 0, 'out': 0}
        self.addr = []
        self.blocks = []

    def place(self, side, es, rows, cols, vector=False) -> Mat:
        ld = max(cols, 1) if (vector or not self.strided) else _odd_above(max(cols, 1))
        span = (rows - 1) * ld + cols if rows > 0 and cols > 0 else 0
        pad = 64 // es
        origin = pad + (1 if es == 8 and self.strided else 0)         # float64: an odd element of a 16-byte aligned parent
        nbytes = -(-(origin + span + pad) * es // 16) * 16
        k = np.arange(self.size[side] // 8, (self.size[side] + nbytes) // 8, dtype=np.float64)
        chunk = (SENTINEL * (1.0 + k * 2.0 ** -40) if side == 'out' else k + 1.0).view(np.uint8).copy()
        start = self.size[side]
        self.chunks[side].append(chunk)
        mat = Mat(side, start + origin * es, rows, cols, ld, es, (start, start + nbytes))
        self.size[side] += nbytes
        if side == 'in':
            self.nan_chunks.append(np.full(nbytes // 8, np.nan).view(np.uint8).copy())
        else:
            mask = np.zeros(nbytes, dtype=bool)
            self.addr.append(mask)
        return mat

    def block(self, a, full=0, no_v=False, values=False, tag=''):
        a = np.ascontiguousarray(a)
        m, n = a.shape
        es = 16 if np.iscomplexobj(a) else 8
        A = self.place('in', es, m, n)
        local = Mat('in', A.gbyte - A.parent[0], m, n, A.ld, es, (0, A.parent[1] - A.parent[0]))
        for chunk in (self.chunks['in'][-1], self.nan_chunks[-1]):
            local.view(chunk)[...] = a
        k = min(m, n)
        fam = 'qr' if self.kind in ('qr', 'cqr') else 'eigh' if self.kind in ('eigh', 'eigh_ex', 'ceigh') else 'svd'
        if fam == 'svd':
            out = {'U': self.place('out', es, m, k), 'S': self.place('out', 8, 1, k, True), 'Vh': self.place('out', es, k, n)}
        elif fam == 'eigh':
            out = {'W': self.place('out', 8, 1, n, True), 'V': None if no_v else self.place('out', es, n, n)}
        else:
            kq = m if full else k
            out = {'Q': self.place('out', es, m, kq), 'R': self.place('out', es, kq, n)}
        self.blocks.append(Block(m, n, a, A, out, full, values, tag))

    def case(self, expect_routes) -> Case:
        def cat(chunks):
            return np.concatenate(chunks) if chunks else np.zeros(16, np.uint8)

        addressed = np.zeros(max(self.size['out'], 16), dtype=bool)
        for b in self.blocks:
            for mat in b.out.values():
                if mat is not None:
                    mat.mark(addressed)
        return Case(self.name, self.kind, self.flags, self.want_rank, self.strided, cat(self.chunks['in']), cat(self.nan_chunks),
                    cat(self.chunks['out']), addressed, self.blocks, list(expect_routes))


# ---- runner and checker -----------------------------------------------------------------------------------------------

@dataclass
class Got:
    ain: np.ndarray           # uint8, after the call(s)
    aout: np.ndarray
    status: int
    info: list | None
    rank: list | None


def run(case, launch, memory=None, nan=False, launches=1) -> Got:
    """Upload both arenas through `memory` and hand the filled descriptor array to
    `launch(kind, descs, n, flags, want_info, want_rank) -> (status, info | None, rank | None)`, `launches` times."""
    memory = memory if memory is not None else HostMemory()
    ain = case.ain_nan if nan else case.ain
    base_in, base_out = memory.upload(ain.view(np.float64)), memory.upload(case.aout0.view(np.float64))
    descs = case.descriptors(base_in, base_out)
    for _ in range(launches):
        status, info, rank = launch(case.kind, descs, len(case.blocks), case.flags, case.family != 'qr', case.want_rank)
    return Got(memory.download(base_in, ain.size // 8).view(np.uint8), memory.download(base_out, case.aout0.size // 8).view(np.uint8),
               status, info, rank)


def results(case, got):
    """Per block: {name: array} of the addressed elements (copies)."""
    return [{k: (None if mat is None else mat.view(got.aout).copy()) for k, mat in b.out.items()} for b in case.blocks]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@dataclass
class Report:
    sentinel: list = field(default_factory=list)
    source: list = field(default_factory=list)
    twin: list = field(default_factory=list)
    measure: list = field(default_factory=list)
    structure: list = field(default_factory=list)
    status: list = field(default_factory=list)
    measures: list = field(default_factory=list)      # per block: {measure: value in EPS}

    KINDS = ('sentinel', 'source', 'twin', 'measure', 'structure', 'status')

    @property
    def clean(self):
        return not any(getattr(self, k) for k in self.KINDS)

    def failed(self):
        return {k for k in self.KINDS if getattr(self, k)}

    def __str__(self):
        out = [f'{k}: {len(getattr(self, k))}, first {getattr(self, k)[0]}' for k in self.KINDS if getattr(self, k)]
        return '; '.join(out) if out else 'clean'


def _kept(case, got, i):
    """How many vectors of block i are specified."""
    b = case.blocks[i]
    k = min(b.m, b.n)
    if case.flags & SKIP_NULL and got.rank is not None:
        return max(0, min(k, int(got.rank[i])))
    return k


def _locate(case, byte):
    for i, b in enumerate(case.blocks):
        for name, mat in b.out.items():
            if mat is not None and mat.parent[0] <= byte < mat.parent[1]:
                e = (byte - mat.gbyte) // mat.es
                return (i, name, int(e // mat.ld), int(e % mat.ld))
    return (-1, '', int(byte), 0)


def check(case, got, twin=None, nan=False) -> Report:
    """`got`: the call on `case`; `twin`: (contiguous case, its Got) or None (no twin check)."""
    rep = Report()
    bad = np.flatnonzero((got.aout != case.aout0) & ~case.addressed)
    rep.sentinel = [_locate(case, int(b)) for b in bad[:4]] + [None] * max(0, min(int(bad.size) - 4, 1))
    ain = case.ain_nan if nan else case.ain
    src = np.flatnonzero(got.ain != ain)
    rep.source = [int(b) for b in src[:4]]
    if got.status != CYB_OK:
        rep.status.append(f'status {got.status}, info {got.info}')
    res = results(case, got)
    if twin is not None:
        tcase, tgot = twin
        if (got.status, got.info, got.rank) != (tgot.status, tgot.info, tgot.rank):
            rep.twin.append(f'status / info / rank {(got.status, got.info, got.rank)} against {(tgot.status, tgot.info, tgot.rank)}')
        for i, (r, t) in enumerate(zip(res, results(tcase, tgot))):
            kept = _kept(case, got, i)
            for name in r:
                if r[name] is None:
                    continue
                x, y = r[name], t[name]
                if name == 'U':
                    x, y = x[:, :kept], y[:, :kept]
                if name == 'Vh':
                    x, y = x[:kept], y[:kept]
                if not np.array_equal(_bits(x), _bits(y)):
                    rep.twin.append(f'block {i} {name}: {int((_bits(x) != _bits(y)).sum())} word(s) differ')
    for i, (b, r) in enumerate(zip(case.blocks, res)):
        m = _measure(case, b, r, _kept(case, got, i), rep, i)
        rep.measures.append(m)
        for key, val in m.items():
            if not val <= dac.CAP_EPS:           # (NaN fails)
                rep.measure.append(f'block {i} {b.tag} {b.m}x{b.n}: {key} = {val:.1f} eps')
    return rep


def _twice(x):
    return x.size % 2 == 0 and np.array_equal(_bits(x[0::2]), _bits(x[1::2]))


def _measure(case, b, r, kept, rep, i):
    """The measures of one block in EPS; structure failures go to `rep`."""
    fam = case.family
    a = b.a
    if b.m == 0 or b.n == 0:
        return {}
    embedded = bool(case.flags & EMBEDDED)
    try:
        if fam == 'svd':
            U, S, Vh = r['U'], r['S'][0], r['Vh']
            if embedded and not _twice(S):
                rep.structure.append(f'block {i}: S of an embedded block does not hold every value twice')
            ref = dac._ld(np.linalg.svd(a, compute_uv=False)) if b.values else None
            c = dac.Case(b.tag, a, ref)
            if kept == min(b.m, b.n):
                return dac.svd_measures(c, U, S, Vh)
            dac.svd_measures(c, np.zeros_like(U), S, np.zeros_like(Vh))      # (the exact facts about S)
            Uk, Sk, Vk = U[:, :kept], S[:kept], Vh[:kept]
            s1 = dac.LD(S[0]) if S[0] > 0 else dac.LD(1)
            out = {'orth_u': dac.orth(np.ascontiguousarray(Uk)), 'orth_v': dac.orth(np.ascontiguousarray(Vk.conj().T)),
                   'resid': float(np.abs((dac._ld(Uk) * dac._ld(Sk)) @ dac._ld(Vk) - dac._ld(a)).max() / s1 / dac.EPS)}
            if ref is not None:
                out['values'] = float(np.abs(dac._ld(S) - ref).max() / ref[0] / dac.EPS)
            return out
        if fam == 'eigh':
            W, V = r['W'][0], r['V']
            if embedded and not _twice(W):
                rep.structure.append(f'block {i}: W of an embedded block does not hold every value twice')
            ref = dac._ld(np.linalg.eigvalsh(a)) if b.values else None
            c = dac.Case(b.tag, a, ref)
            if V is not None:
                return dac.eigh_measures(c, W, V)
            if not np.all(W[:-1] <= W[1:]):
                rep.structure.append(f'block {i}: W is not ascending')
            fro = np.sqrt((np.abs(dac._ld(a)) ** 2).sum())
            return {'values': float(np.abs(dac._ld(W) - ref).max() / (fro if fro > 0 else 1) / dac.EPS)} if ref is not None else {}
        Q, R = r['Q'], r['R']
        k = min(b.m, b.n)
        low = np.tril(R, -1)
        low[k:] = R[k:]
        if _bits(low.real).any() or (np.iscomplexobj(low) and _bits(low.imag).any()):
            rep.structure.append(f'block {i}: R is not +0.0 below its diagonal / beyond row k')
        return dac.qr_measures(dac.Case(b.tag, a), Q, R, full=bool(b.full), positive_diagonal=case.cplx)
    except dac.AccuracyError as e:
        rep.structure.append(f'block {i}: {e}')
        return {}


# ---- numpy stand-in ---------------------------------------------------------------------------------------------------

def embed(z):
    """The interleaved real embedding M(z): entry a + ib -> [[a, -b], [b, a]]."""
    out = np.zeros((2 * z.shape[0], 2 * z.shape[1]))
    out[0::2, 0::2], out[0::2, 1::2], out[1::2, 0::2], out[1::2, 1::2] = z.real, -z.imag, z.imag, z.real
    return out


def unembed(M):
    return M[0::2, 0::2] + 1j * M[1::2, 0::2]


def range_scale(amax):
    """range_scale of csrc/scaling.hip."""
    if not (amax > 0.0) or not (amax <= 1.7e308) or 1e-90 <= amax <= 1e90:
        return 1.0
    return float(np.ldexp(1.0, -np.frexp(amax)[1]))


class NumpyDecomp:
    """`launch` of `run` on host memory: reads every A and writes every result through the descriptor's own pointers and
    leading dimensions.  `fault`: {'kind': one of FAULT_KINDS, 'block': index} makes it wrong in that way."""

    def __init__(self, memory, fault=None):
        self.memory, self.fault = memory, fault or {}

    def _flat(self, addr, dt):
        for arr in self.memory.arrays:
            d = addr - arr.ctypes.data
            if 0 <= d < arr.nbytes:
                b = arr.view(np.uint8)[d:]
                return b[:b.size // dt.itemsize * dt.itemsize].view(dt)
        raise ValueError('address outside every uploaded buffer')

    def _read(self, addr, ld, rows, cols, dt):
        flat = self._flat(addr, dt)
        return flat[(np.arange(rows)[:, None] * ld + np.arange(cols)[None, :])].copy()

    def _write(self, addr, ld, x, dt, kind=None):
        """x (2-d) to the rows x cols view at `addr`; `kind`: the write-out faults."""
        if addr is None:
            return
        flat = self._flat(addr, dt)
        rows, cols = x.shape
        if kind == 'ld_as_extent':
            ld = cols
        if kind == 'transposed':
            x, rows, cols = x.T, cols, rows
        if kind in ('cols_to_32', 'rows_to_32'):        # the tile runs on to its edge: zeros first, the rows afterwards
            pr = -(-rows // XPOSE_TILE) * XPOSE_TILE if kind == 'rows_to_32' else rows
            pc = -(-cols // XPOSE_TILE) * XPOSE_TILE if kind == 'cols_to_32' else cols
            idx = (np.arange(pr)[:, None] * ld + np.arange(pc)[None, :]).reshape(-1)
            flat[idx[idx < flat.size]] = 0.0
        idx = (np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).reshape(-1)
        keep = idx < flat.size
        flat[idx[keep]] = np.asarray(x, dtype=dt).reshape(-1)[keep]

    def __call__(self, kind, descs, n, flags, want_info, want_rank):
        fam = 'qr' if kind in ('qr', 'cqr') else 'eigh' if kind in ('eigh', 'eigh_ex', 'ceigh') else 'svd'
        cplx = kind in ('csvd', 'ceigh', 'cqr')
        dt = np.dtype(np.complex128 if cplx else np.float64)
        f8 = np.dtype(np.float64)
        shapes = [((d.n if fam == 'eigh' else d.m), d.n) for d in descs[:n]]
        full = descs[0].full if fam == 'qr' and n else 0
        route = routes(kind, shapes, flags, full)
        info, rank, status = [0] * n, [min(s) for s in shapes], CYB_OK
        for i in range(n):
            d, (m, nn) = descs[i], shapes[i]
            if m == 0 or nn == 0:
                continue
            fk = self.fault.get('kind') if self.fault.get('block') == i else None
            a = self._read(d.A, nn if fk == 'lda_as_n' else d.lda, m, nn, dt)
            if fk == 'gap_read':
                a[0, 0] = self._flat(d.A, dt)[nn]            # the element behind the first row: a gap
            if fk == 'scale_in_place' and range_scale(np.abs(a).max()) != 1.0:
                self._write(d.A, d.lda, a * range_scale(np.abs(a).max()), dt)
            if not np.isfinite(a).all() and not cplx and fam != 'qr':       # a NaN block (batched_ranged of svd_jacobi.hip)
                info[i], rank[i], status = -1, 0, CYB_ERR_NOCONV
                continue
            wk = fk if fk in ('ld_as_extent', 'cols_to_32', 'rows_to_32', 'transposed') else None
            w2 = None if wk == 'transposed' else wk          # (the transposed write-out: the first factor only)
            if not np.isfinite(a).all():                     # no NaN handling on these entries: the result is poisoned
                a = np.zeros_like(a)
                poison = np.nan
            else:
                poison = 0.0
            if fam == 'svd':
                if flags & EMBEDDED:
                    u, s, vh = np.linalg.svd(unembed(a), full_matrices=False)
                    u, s, vh = embed(u), np.repeat(s, 2), embed(vh)
                else:
                    u, s, vh = np.linalg.svd(a, full_matrices=False)
                if route[i] == 'pipeline':
                    rank[i] = int((s > np.linalg.norm(a) * max(m, nn) * 2.0 ** -52).sum())
                self._write(d.U, d.ldu, u + poison, dt, wk)
                if fk == 's_pad_64':
                    s = np.r_[s, np.zeros(-len(s) % 64)]
                self._write(d.S, len(s), s[None, :], f8)
                self._write(d.Vh, d.ldvh, vh, dt, w2)
            elif fam == 'eigh':
                if flags & EMBEDDED:
                    w, v = np.linalg.eigh(unembed(a))
                    w, v = np.repeat(w, 2), embed(v)
                else:
                    w, v = np.linalg.eigh(a)
                if fk == 's_pad_64':
                    w = np.r_[w, np.zeros(-len(w) % 64)]
                self._write(d.W, len(w), w[None, :], f8)
                self._write(d.V, d.ldv, v + poison, dt, wk)
            else:
                q, r = np.linalg.qr(a, mode='complete' if d.full else 'reduced')
                if cplx:                                      # diag(R) real and non-negative
                    dg = np.diagonal(r)
                    ph = np.where(np.abs(dg) > 0, dg / np.where(np.abs(dg) > 0, np.abs(dg), 1), 1)
                    ph = np.r_[ph, np.ones(q.shape[1] - ph.size)]
                    q, r = q * ph[None, :], np.conj(ph)[:r.shape[0], None] * r
                    r[np.arange(dg.size), np.arange(dg.size)] = np.abs(dg)
                r = np.triu(r) + 0.0
                self._write(d.Q, d.ldq, q + poison, dt, wk)
                if fk == 'r_lower_unwritten':
                    old = self._read(d.R, d.ldr, r.shape[0], r.shape[1], dt)
                    low = np.tril(np.ones(r.shape, bool), -1)
                    r = np.where(low, old, r)
                self._write(d.R, d.ldr, r, dt, w2)
        return status, (info if want_info else None), (rank if want_rank else None)


# ---- data -------------------------------------------------------------------------------------------------------------

def _normal(rng, m, n, cplx=False):
    return dac.crandn(rng, (m, n)) if cplx else rng.standard_normal((m, n))


def _herm(rng, n, cplx=False):
    z = _normal(rng, n, n, cplx)
    return z + z.conj().T


BIG = 2.0 ** 400

# ---- the cases --------------------------------------------------------------------------------------------------------
SVD_TINY = [(1, 1), (3, 5), (5, 3), (31, 33), (33, 31), (64, 128), (128, 64), (0, 5)]
SVD_MIXED = [(65, 65), (2, 2), (5, 130), (130, 5), (1, 9), (9, 1), (40, 30)]          # the last: rank 10
SVD_SIXTEEN = [(3, 5), (5, 3), (4, 4), (7, 2)] * 4 + [(65, 65)]
SVD_EMBEDDED = [(6, 4), (4, 6), (66, 66)]
EIGH_SMALL, EIGH_JACOBI, EIGH_EMBEDDED = (1, 3, 33, 64), (65, 3, 1), (2, 6, 66)
QR_UNBLOCKED = [(1, 1), (6, 4), (4, 6), (95, 95), (130, 5)]
QR_BLOCKED = [(96, 96), (97, 129), (129, 97)]
# complex, either side of each limit.  (64, 128) has the real limits but not the LDS bound (198656 bytes above 150 KB): the
# large route, with (65, 65) and (12, 129); (10, 129) holds 1290 elements, below kSingleElems: the one-workgroup kernel.
CSVD_SMALL, CSVD_LARGE = [(5, 3), (64, 64), (40, 128)], [(64, 128), (65, 65), (12, 129)]
CEIGH_SMALL, CEIGH_LARGE = (9, 64), (65,)
CQR_SMALL, CQR_LARGE = [(96, 96), (4, 6), (10, 129)], [(97, 97), (72, 129), (129, 72)]


def _svd_case(name, shapes, expect, kind='svd', flags=0, want_rank=False, strided=True, seed=1, scaled=()):
    b = _Builder(name, kind, flags, want_rank, strided)
    rng = np.random.default_rng(seed)
    cplx = kind == 'csvd'
    for i, (m, n) in enumerate(shapes):
        if flags & EMBEDDED:
            a, values, tag = embed(_normal(rng, m // 2, n // 2, True)), True, 'embedded'
        elif (m, n) == (40, 30):
            a, values, tag = _normal(rng, 40, 10) @ _normal(rng, 10, 30), False, 'rank 10'
        else:
            a, values, tag = _normal(rng, m, n, cplx), True, 'normal'
        if i in scaled:
            a, tag = a * BIG, 'normal 2^400'
        b.block(a, values=values, tag=tag)
    return b.case(expect)


def _eigh_case(name, sizes, expect, kind='eigh', flags=0, no_v=False, strided=True, seed=2, scaled=()):
    b = _Builder(name, kind, flags, False, strided)
    rng = np.random.default_rng(seed)
    for i, n in enumerate(sizes):
        a = embed(_herm(rng, n // 2, True)) if flags & EMBEDDED else _herm(rng, n, kind == 'ceigh')
        b.block(a * BIG if i in scaled else a, no_v=no_v, values=True, tag='hermitian 2^400' if i in scaled else 'hermitian')
    return b.case(expect)


def _qr_case(name, shapes, expect, kind='qr', full=0, strided=True, seed=3, scaled=()):
    b = _Builder(name, kind, 0, False, strided)
    rng = np.random.default_rng(seed)
    for i, (m, n) in enumerate(shapes):
        a = _normal(rng, m, n, kind == 'cqr')
        b.block(a * BIG if i in scaled else a, full=full, tag='normal 2^400' if i in scaled else 'normal')
    return b.case(expect)


def all_cases():
    """{family: {name: builder(strided=True)}}: every case of the device test."""
    T, P, D = 'tiny', 'pipeline', 'direct'
    g = {'svd': {}, 'eigh': {}, 'qr': {}, 'complex': {}}
    s = g['svd']
    s['tiny'] = lambda strided=True: _svd_case('tiny', SVD_TINY, [T] * 7 + ['empty'], strided=strided)
    mixed = [P, P, P, P, D, D, P]
    s['pipeline + direct'] = lambda strided=True: _svd_case('pipeline + direct', SVD_MIXED, mixed, strided=strided, seed=4)
    s['pipeline + direct, skip null vectors'] = lambda strided=True: _svd_case(
        'pipeline + direct, skip null vectors', SVD_MIXED, mixed, 'svd_ex', SKIP_NULL, True, strided, seed=4)
    s['tiny + pipeline'] = lambda strided=True: _svd_case('tiny + pipeline', SVD_SIXTEEN, [T] * 16 + [P], strided=strided, seed=5)
    s['embedded'] = lambda strided=True: _svd_case('embedded', SVD_EMBEDDED, [P] * 3, 'svd_ex', EMBEDDED, False, strided, seed=6)
    s['range scale'] = lambda strided=True: _svd_case('range scale', [(33, 31), (5, 3)], [T, T], strided=strided, seed=7, scaled=(0,))
    s['range scale, pipeline'] = lambda strided=True: _svd_case('range scale, pipeline', [(66, 70), (5, 3)], [P, P], strided=strided,
                                                                 seed=8, scaled=(0,))
    e = g['eigh']
    for tag, no_v in (('', False), (', no V', True)):
        e['small' + tag] = lambda strided=True, no_v=no_v, tag=tag: _eigh_case('small' + tag, EIGH_SMALL, ['small'] * 4, no_v=no_v, strided=strided)
        e['jacobi' + tag] = lambda strided=True, no_v=no_v, tag=tag: _eigh_case('jacobi' + tag, EIGH_JACOBI, ['jacobi'] * 3, no_v=no_v,
                                                                               strided=strided, seed=9)
    e['embedded'] = lambda strided=True: _eigh_case('embedded', EIGH_EMBEDDED, ['jacobi'] * 3, 'eigh_ex', EMBEDDED, strided=strided, seed=10)
    e['range scale'] = lambda strided=True: _eigh_case('range scale', (33, 3), ['small'] * 2, strided=strided, seed=11, scaled=(0,))
    q = g['qr']
    for full in (0, 1):
        tag = ', full' if full else ', economic'
        q['unblocked' + tag] = lambda strided=True, full=full, tag=tag: _qr_case('unblocked' + tag, QR_UNBLOCKED, ['unblocked'] * 5, full=full,
                                                                                 strided=strided)
        q['blocked' + tag] = lambda strided=True, full=full, tag=tag: _qr_case('blocked' + tag, QR_BLOCKED, ['blocked'] * 3, full=full,
                                                                             strided=strided, seed=12)
        q['range scale' + tag] = lambda strided=True, full=full, tag=tag: _qr_case('range scale' + tag, [(6, 4), (4, 6)], ['unblocked'] * 2,
                                                                                 full=full, strided=strided, seed=13, scaled=(0,))
    c = g['complex']
    c['svd small'] = lambda strided=True: _svd_case('svd small', CSVD_SMALL, ['small'] * 3, 'csvd', strided=strided, seed=14)
    c['svd large'] = lambda strided=True: _svd_case('svd large', CSVD_LARGE, ['large'] * 3, 'csvd', strided=strided, seed=15)
    c['eigh small'] = lambda strided=True: _eigh_case('eigh small', CEIGH_SMALL, ['small'] * 2, 'ceigh', strided=strided, seed=16)
    c['eigh large'] = lambda strided=True: _eigh_case('eigh large', CEIGH_LARGE, ['large'], 'ceigh', strided=strided, seed=17)
    for full in (0, 1):
        tag = ', full' if full else ', economic'
        c['qr small' + tag] = lambda strided=True, full=full, tag=tag: _qr_case('qr small' + tag, CQR_SMALL, ['small'] * 3, 'cqr', full, strided,
                                                                              seed=18)
        c['qr large' + tag] = lambda strided=True, full=full, tag=tag: _qr_case('qr large' + tag, CQR_LARGE, ['large'] * 3, 'cqr', full, strided,
                                                                              seed=19)
    return g
