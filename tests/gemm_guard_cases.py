"""Guard-band cases for the descriptor-driven grouped GEMM: builder, runner and checker, all on the host.

A case is a list of problems ``C_p = alpha_p * sum_s A_s B_s + beta_p * C0_p`` in the form the C ABI takes them
(``GemmProb`` / ``GemmSeg`` of cyten_amd._lib).  This module knows nothing about the device: `run` hands the filled
descriptor arrays to a callable and moves the buffers through a `memory` object, so the same cases serve the numpy
stand-in below (tests/test_gemm_guard_model.py), the C ABI on the device (tests/test_gpu_gemm_guard.py) and, later, the
other descriptor-driven kernels.

Buffers.  Every A, B and C is a view into a larger parent buffer.  The view starts at an ODD element offset of a
16-byte aligned parent (8-byte but not 16-byte aligned) and its leading dimension is odd and larger than the extent.
Everything of an A / B parent outside the view is NaN -- the gaps between the rows too -- so a read outside a view
poisons the result.  A C parent holds a fixed finite sentinel in the guard rows before and after the view and in the gap
columns ``N .. ldc-1``; its interior is NaN when ``beta == 0`` (the header promises that C is not read then), else C0.

Exact data.  Integer entries in [-15, 15]; row i of A is scaled by 2^r_i, column j of B by 2^c_j, column k of A by 2^g_k
and row k of B by 2^-g_k (all exponents in [-30, 30]), C0 is an integer times 2^(r_i + c_j), alpha and beta are powers of
two or zero.  Every product of element (i, j) is then an integer times 2^(r_i + c_j): with a total K of at most 512 all
partial sums are exactly representable, ANY correct summation order gives the same bits, the reference is float64 numpy
and the comparison is `==` with no tolerance -- while the grading makes a lost term of a small row or column (1e-16 of
the largest entry of the result, invisible to a normwise tolerance) a plain mismatch.

Rounded data.  standard_normal entries with the same grading, reference in np.longdouble (at least 64 mantissa bits, or
the helper refuses), componentwise bound ``|got - ref| <= (Ktot + 4) * 2^-53 * (|alpha| sum_k |A||B| + |beta| |C0|)``:
Ktot products accumulated in any order (Higham, Accuracy and Stability of Numerical Algorithms, (3.5): gamma_K <= K u
to first order, one more u for an fma-free product) plus the three roundings of the epilogue -- derived, not tuned."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from cyten_amd import _lib

SENTINEL = np.float64(-6.02214076e+123)
COEFFS = (1.0, -2.0, 0.5, 0.0)                      # alpha / beta: powers of two (exact) and zero
LAYOUTS = {'rr': (False, False), 'rc': (False, True), 'cr': (True, False), 'cc': (True, True)}   # (A, B) column-major?
K_TOTAL_MAX = 512
U = 2.0 ** -53


@dataclass
class Spec:
    """One problem: extents, K of every segment (an empty tuple: empty segment range), per-segment (A column-major,
    B column-major) flags, coefficients, `data` in {'exact', 'normal'}."""
    M: int
    N: int
    Ks: tuple
    layouts: tuple
    alpha: float = 1.0
    beta: float = 0.0
    data: str = 'exact'
    tag: str = ''


def alternating(layout, n):
    """Layouts of an n-segment list that starts at `layout` and changes from segment to segment:
    (a, b), (!a, !b), (a, !b), (!a, b), ..."""
    a, b = LAYOUTS[layout] if isinstance(layout, str) else layout
    return tuple((a ^ bool(s & 1), b ^ bool(((s + 1) // 2) & 1)) for s in range(n))


def spec(M, N, Ks, layout='rr', alpha=1.0, beta=0.0, data='exact', tag=''):
    Ks = tuple(int(k) for k in ([Ks] if np.isscalar(Ks) else Ks))
    return Spec(int(M), int(N), Ks, alternating(layout, len(Ks)), float(alpha), float(beta), data, tag)


def _odd_above(n):
    return n + 1 if n % 2 == 0 else n + 2


@dataclass
class _Seg:
    a_off: int
    b_off: int
    K: int
    a_rs: int
    a_cs: int
    b_rs: int
    b_cs: int


@dataclass
class _Prob:
    spec: Spec
    c_off: int
    ldc: int
    seg_begin: int
    seg_end: int
    ref: np.ndarray
    bound: np.ndarray | None
    parent: tuple      # [start, end) of the C parent in the output arena


@dataclass
class Case:
    ain: np.ndarray                 # arena of all A / B parents (NaN outside the views)
    cout0: np.ndarray               # arena of all C parents before the call
    guard: np.ndarray               # True where cout0 holds a sentinel
    probs: list = field(default_factory=list)
    segs: list = field(default_factory=list)

    def descriptors(self, base_in, base_out):
        """Filled GemmProb / GemmSeg arrays for arenas that live at the byte addresses `base_in` / `base_out`."""
        if base_in % 16 or base_out % 16:
            raise ValueError('guard cases need 16-byte aligned arenas (the views are placed at odd element offsets of them)')
        probs = (_lib.GemmProb * max(len(self.probs), 1))()
        segs = (_lib.GemmSeg * max(len(self.segs), 1))()
        for d, s in zip(segs, self.segs):
            d.A = base_in + 8 * s.a_off if s.a_off >= 0 else None
            d.B = base_in + 8 * s.b_off if s.b_off >= 0 else None
            d.K, d.a_rs, d.a_cs, d.b_rs, d.b_cs = s.K, s.a_rs, s.a_cs, s.b_rs, s.b_cs
        for d, p in zip(probs, self.probs):
            d.C, d.M, d.N, d.ldc = base_out + 8 * p.c_off, p.spec.M, p.spec.N, p.ldc
            d.seg_begin, d.seg_end, d.alpha, d.beta = p.seg_begin, p.seg_end, p.spec.alpha, p.spec.beta
        return probs, segs


def _place(ext_rows, ext_cols, col_major):
    """Geometry of a rows x cols view inside its parent: (odd offset of the view, row stride, column stride, size)."""
    n_lines, line = (ext_cols, ext_rows) if col_major else (ext_rows, ext_cols)
    ld = _odd_above(max(line, 1))
    pre, post = ld + 2, ld + 3
    size = pre + n_lines * ld + post
    size += size % 2                                 # the next parent starts 16-byte aligned again
    return pre, (1, ld) if col_major else (ld, 1), size


def _view(arena, off, shape, strides):
    item = arena.itemsize
    return np.lib.stride_tricks.as_strided(arena[off:], shape, (item * strides[0], item * strides[1]))


def require_longdouble():
    eps = np.finfo(np.longdouble).eps
    if not eps <= 2.0 ** -63:
        raise RuntimeError(f'the rounded-data reference needs np.longdouble with eps <= 2^-63 (x87 extended or wider); '
                           f'this platform has eps = {float(eps):.3g}, no better than the float64 under test')


def build_case(specs, seed=0) -> Case:
    rng = np.random.default_rng(seed)
    specs = list(specs)
    # first pass: geometry
    geo, n_in, n_out = [], 0, 0
    for sp in specs:
        if sum(sp.Ks) > K_TOTAL_MAX:
            raise ValueError(f'total K {sum(sp.Ks)} > {K_TOTAL_MAX}: the exact-data argument needs exactly representable partial sums')
        if len(sp.layouts) != len(sp.Ks):
            raise ValueError('one layout per segment')
        sg = []
        for K, (a_cm, b_cm) in zip(sp.Ks, sp.layouts):
            if K == 0:
                sg.append(None)
                continue
            pa = _place(sp.M, K, a_cm)
            pb = _place(K, sp.N, b_cm)
            sg.append((n_in, pa, n_in + pa[2], pb))
            n_in += pa[2] + pb[2]
        pc = _place(sp.M, sp.N, False)
        geo.append((sg, n_out, pc))
        n_out += pc[2]
    ain = np.full(max(n_in, 2), np.nan)
    cout0 = np.full(max(n_out, 2), SENTINEL)
    guard = np.ones(cout0.shape, dtype=bool)
    case = Case(ain, cout0, guard)
    for sp, (sg, c_start, (c_pre, (ldc, _), c_size)) in zip(specs, geo):
        M, N = sp.M, sp.N
        exact = sp.data == 'exact'
        if not exact:
            require_longdouble()
        wide = np.float64 if exact else np.longdouble
        r, c = rng.integers(-30, 31, size=M), rng.integers(-30, 31, size=N)

        def entries(shape):
            return rng.integers(-15, 16, size=shape).astype(np.float64) if exact else rng.standard_normal(shape)

        acc = np.zeros((M, N), dtype=wide)
        mag = np.zeros((M, N), dtype=wide)
        seg_begin = len(case.segs)
        for K, s in zip(sp.Ks, sg):
            if s is None:
                case.segs.append(_Seg(-1, -1, 0, 0, 0, 0, 0))      # K = 0: NULL operands are allowed
                continue
            a_start, (a_pre, a_str, _), b_start, (b_pre, b_str, _) = s
            g = rng.integers(-30, 31, size=K)
            A = np.ldexp(entries((M, K)), r[:, None] + g[None, :])
            B = np.ldexp(entries((K, N)), c[None, :] - g[:, None])
            _view(ain, a_start + a_pre, (M, K), a_str)[...] = A
            _view(ain, b_start + b_pre, (K, N), b_str)[...] = B
            acc += A.astype(wide) @ B.astype(wide)
            if not exact:
                mag += np.abs(A).astype(wide) @ np.abs(B).astype(wide)
            case.segs.append(_Seg(a_start + a_pre, b_start + b_pre, K, a_str[0], a_str[1], b_str[0], b_str[1]))
        C0 = np.ldexp(entries((M, N)), r[:, None] + c[None, :])
        ref = wide(sp.alpha) * acc
        if sp.beta != 0.0:
            ref = ref + wide(sp.beta) * C0.astype(wide)
        bound = None
        if not exact:
            bound = (sum(sp.Ks) + 4) * wide(U) * (abs(sp.alpha) * mag + abs(sp.beta) * np.abs(C0).astype(wide))
        c_off = c_start + c_pre
        _view(cout0, c_off, (M, N), (ldc, 1))[...] = C0 if sp.beta != 0.0 else np.nan
        _view(guard, c_off, (M, N), (ldc, 1))[...] = False
        case.probs.append(_Prob(sp, c_off, ldc, seg_begin, len(case.segs), ref, bound, (c_start, c_start + c_size)))
    return case


class HostMemory:
    """The stand-in's device memory: `upload` copies a host array and returns the byte address of the copy."""

    def __init__(self):
        self.arrays = []

    def upload(self, arr):
        copy = np.empty(arr.size + 1)
        copy = copy[(copy.ctypes.data // 8) % 2:][:arr.size]      # 16-byte aligned start
        copy[...] = arr
        self.arrays.append(copy)
        return copy.ctypes.data

    def download(self, addr, n):
        arr, i = self.locate(addr)
        return arr[i:i + n].copy()

    def locate(self, addr):
        for arr in self.arrays:
            d = addr - arr.ctypes.data
            if 0 <= d < arr.nbytes:
                return arr, d // 8
        raise ValueError('address outside every uploaded buffer')


def run(case, launch, memory=None, launches=1):
    """Upload the arenas through `memory`, hand the filled GemmProb / GemmSeg arrays to `launch(probs, n_probs, segs,
    n_segs)` (`launches` times) and return the C arena after the call(s)."""
    memory = memory if memory is not None else HostMemory()
    base_in, base_out = memory.upload(case.ain), memory.upload(case.cout0)
    probs, segs = case.descriptors(base_in, base_out)
    for _ in range(launches):
        launch(probs, len(case.probs), segs, len(case.segs))
    return memory.download(base_out, case.cout0.size)


@dataclass
class Report:
    interior: list      # (problem, row, column, got, want): finite but wrong
    nan: list           # (problem, row, column): NaN in the interior -- a read outside a view, or of C under beta == 0
    sentinel: list      # (problem, offset from the view's first element): a guard element changed -- a write out of bounds
    max_ratio: float    # rounded data: largest |err| / bound (0.0 for exact cases)
    n_bad: dict
    ratios: list        # the same per problem

    def ratio_by_tag(self, case):
        out = {}
        for p, r in zip(case.probs, self.ratios):
            if p.bound is not None:
                out[p.spec.tag] = max(out.get(p.spec.tag, 0.0), r)
        return out

    @property
    def clean(self):
        return not (self.interior or self.nan or self.sentinel)

    def __str__(self):
        out = [f'{k}: {self.n_bad[k]} element(s), first {v[0]}' for k, v in
               (('interior', self.interior), ('nan', self.nan), ('sentinel', self.sentinel)) if v]
        return '; '.join(out) if out else 'clean'


def check(case, got, refs=None) -> Report:
    """Compare the C arena after a call with the references (`refs` replaces the stored ones: a plan run twice)."""
    interior, nan, sentinel = [], [], []
    n_bad = {'interior': 0, 'nan': 0, 'sentinel': 0}
    max_ratio, ratios = 0.0, [0.0] * len(case.probs)
    changed = np.flatnonzero((got.view(np.uint64) != case.cout0.view(np.uint64)) & case.guard)   # bitwise
    if changed.size:
        starts = np.array([p.parent[0] for p in case.probs])
        n_bad['sentinel'] = int(changed.size)
        for idx in changed[:4]:
            p = int(np.searchsorted(starts, idx, side='right') - 1)
            sentinel.append((p, int(idx) - case.probs[p].c_off))
    for pi, p in enumerate(case.probs):
        M, N = p.spec.M, p.spec.N
        if M == 0 or N == 0:
            continue
        view = _view(got, p.c_off, (M, N), (p.ldc, 1))
        ref = p.ref if refs is None else refs[pi]
        isnan = np.isnan(view)
        if p.bound is None:
            bad = (view != ref) & ~isnan
        else:
            err = np.abs(view.astype(np.longdouble) - ref)
            with np.errstate(divide='ignore', invalid='ignore'):
                ratio = np.where(err == 0, 0.0, err / p.bound)
            bad = ~(err <= p.bound) & ~isnan
            if not isnan.all():
                ratios[pi] = float(np.max(ratio[~isnan]))
                max_ratio = max(max_ratio, ratios[pi])
        for name, mask, rows in (('nan', isnan, nan), ('interior', bad, interior)):
            if mask.any():
                n_bad[name] += int(mask.sum())
                if len(rows) < 4:
                    i, j = (int(x) for x in np.argwhere(mask)[0])
                    rows.append((pi, i, j) if name == 'nan' else (pi, i, j, float(view[i, j]), float(ref[i, j])))
    return Report(interior, nan, sentinel, max_ratio, n_bad, ratios)


def normwise_ok(case, got, tol=1e-10):
    """The criterion of tests/test_gpu_gemm.py (`|got - ref| <= tol * max|ref|` per problem) -- kept to SHOW what it misses."""
    for p in case.probs:
        if p.spec.M == 0 or p.spec.N == 0:
            continue
        view = _view(got, p.c_off, (p.spec.M, p.spec.N), (p.ldc, 1))
        if not np.abs(view - p.ref).max() <= tol * max(1.0, float(np.abs(p.ref).max())):
            return False
    return True


# ---- numpy stand-in -------------------------------------------------------------------------------------------------

class NumpyGemm:
    """Evaluates the descriptors through their strides on the parent buffers.  `fault` (a dict with 'kind', 'prob' and
    the parameters of that kind) makes it wrong in one of the ways a tile kernel can be wrong."""

    def __init__(self, memory, fault=None):
        self.memory, self.fault = memory, fault

    def _gather(self, addr, rows, cols, rs, cs):
        arr, i = self.memory.locate(addr)
        return arr[i + np.arange(rows)[:, None] * rs + np.arange(cols)[None, :] * cs], arr, i

    def __call__(self, probs, n_probs, segs, n_segs):
        f = self.fault or {}
        for pi in range(n_probs):
            q = probs[pi]
            M, N = q.M, q.N
            if M == 0 or N == 0:
                continue
            hit = f.get('prob') == pi
            kind = f.get('kind') if hit else None
            acc = np.zeros((M, N))
            live = [s for s in range(q.seg_begin, q.seg_end) if segs[s].K > 0]
            for s in live:
                g = segs[s]
                A, a_arr, a0 = self._gather(g.A, M, g.K, g.a_rs, g.a_cs)
                B, _, _ = self._gather(g.B, g.K, N, g.b_rs, g.b_cs)
                K = g.K
                if kind == 'drop_k_tail' and s == live[-1]:
                    K -= K % 16
                term = A[:, :K] @ B[:K, :]
                if kind == 'drop_last_k_of_row' and s == live[-1]:
                    i = f['row']
                    term[i, :] -= A[i, K - 1] * B[K - 1, :]
                if kind == 'read_row_M' and s == live[-1]:
                    term[M - 1, :] += 0.0 * a_arr[a0 + M * g.a_rs + (K - 1) * g.a_cs]
                if kind == 'read_col_K' and s == live[-1]:
                    term[f['row'], :] += 0.0 * a_arr[a0 + f['row'] * g.a_rs + K * g.a_cs]
                acc += term
            c_arr, c0 = self.memory.locate(q.C)
            idx = c0 + np.arange(M)[:, None] * q.ldc + np.arange(N)[None, :]
            out = q.alpha * acc
            if q.beta != 0.0:
                out = out + q.beta * c_arr[idx]
            elif kind == 'read_c_beta0':
                out = out + 0.0 * c_arr[idx]
            t = (slice(*f['rows']), slice(*f['cols'])) if kind in ('skip_tile', 'tile_twice') else None
            if kind == 'tile_twice':
                out[t] = q.alpha * acc[t] + q.beta * out[t]
            if kind == 'skip_tile':
                keep = c_arr[idx][t].copy()
                c_arr[idx] = out
                c_arr[idx[t]] = keep
            else:
                c_arr[idx] = out
            if kind == 'store_col_N':
                c_arr[c0 + f['row'] * q.ldc + N] = 1.0
            if kind == 'store_row_M':
                c_arr[c0 + M * q.ldc + f['col']] = 1.0


# ---- the case lists -------------------------------------------------------------------------------------------------

SMALL_SHAPES = [(1, 1), (1, 19), (19, 1), (5, 7), (19, 19),                 # class 3: 16 x 16, waves split along K
                (20, 20), (33, 47), (39, 255),                              # class 2: 32 x 32, waves split along K
                (7, 256), (19, 300),                                        # class 5: 16 x 128 strips
                (300, 7),                                                   # class 6: 128 x 16
                (25, 257),                                                  # class 7: 32 x 128
                (257, 25),                                                  # class 8: 128 x 32
                (40, 40), (64, 64), (65, 81), (95, 97), (64 + 33, 300)]     # class 1: 64 x 64 with ragged remainders
SMALL_KS = [1, 3, 15, 16, 17, 31, 32, 33, 69, (1, 16, 7), (33, 2, 48), (5, 0, 12)]   # (one K = 0 in the middle of a list)
SMALL_GROUPS = {'16x16 k-split': SMALL_SHAPES[:5], '32x32 k-split': SMALL_SHAPES[5:8], 'strips 16/32 x 128': SMALL_SHAPES[8:13],
                '64x64 ragged': SMALL_SHAPES[13:]}


def small_class_specs(layout, data='exact'):
    """Every small tile class with every k-tile branch (full, partial, one double) in ONE call; alpha and beta cycle
    through all sixteen pairs; two problems with an empty segment range (the result is beta * C0, or zeros)."""
    out, i = [], 0
    for Ks in SMALL_KS:
        for M, N in SMALL_SHAPES:
            out.append(spec(M, N, Ks, layout, COEFFS[i % 4], COEFFS[(i // 4 + i // 16) % 4], data, f'{M}x{N}'))
            i += 1
    out.append(spec(33, 47, (), layout, 1.0, 0.0, data, 'empty'))
    out.append(spec(19, 300, (), layout, -2.0, 0.5, data, 'empty'))
    return out


CLASS0_SHAPES = [(128, 128), (129, 144), (145, 160), (161, 192), (193, 255), (272, 161), (128 + 65, 128 + 1)]
CLASS0_KS = [16, 40, 69, (48, 5)]


def filler_spec(n_cu):
    """Enough 128 x 128 tiles (at least one per CU) that the planner keeps class 0 for the whole call."""
    return spec(128 * 16, 128 * math.ceil(n_cu / 16), 4, 'rr', 1.0, 0.0, 'exact', 'filler')


def class0_specs(n_cu, layout, beta, data='exact'):
    """128 x 128 tiles with the pointer-increment loop and every strip the planner cuts from their ragged edges
    (128x64, 64x128, 128x32, 32x128, 128x16, 16x128, the corner squares); the filler (exact data, checked too) first."""
    out = [filler_spec(n_cu)]
    i = 0
    for Ks in CLASS0_KS:
        for M, N in CLASS0_SHAPES:
            out.append(spec(M, N, Ks, layout, COEFFS[i % 3], beta, data, f'{M}x{N}'))
            i += 1
    return out


def degenerate_specs():
    """Extents 1 and 2 with K = 48 (three full k-tiles) in the mn-contiguous layouts, the k-contiguous ones beside them:
    `load_tile`'s scalar fallback for `MN < 2` and its `MN - 2` clamp with shift at an extent of exactly 2.  Every such
    shape is planned into class 3, 5 or 6, none of which has the pointer-increment loop: the `M >= 2 && N >= 2` gate of
    that loop is NOT reached from here (at the C ABI only a problem with a left factor brings an extent below 20 into a
    class that has the loop).  The loop's own `MN - 2` clamp runs in the class-0 / class-1 cases with odd extents."""
    out = []
    for i, (M, N) in enumerate([(1, 67), (67, 1), (1, 1), (2, 67), (67, 2), (2, 2), (1, 131), (131, 1), (2, 131), (131, 2),
                                (1, 300), (300, 1), (2, 301), (301, 2)]):
        for layout in ('cr', 'rc', 'cc', 'rr'):
            out.append(spec(M, N, 48, layout, COEFFS[i % 3], COEFFS[(i + 1) % 4], 'exact', f'{M}x{N}'))
    return out


def many_tiles_specs(n_cu):
    """More tiles than workgroup slots: several rounds of the atomic tile queue."""
    return [spec(16, 16, 5, ('rr', 'rc', 'cr', 'cc')[i % 4], 1.0, 1.0) for i in range(2 * n_cu + 37)]


def tail_split_specs(n_cu):
    """One problem whose last, partly filled queue round is cut into 128 x 64 halves (or 128 x 32 quarters)."""
    T = math.ceil(math.sqrt(2 * n_cu)) + 1
    return [spec((T - 1) * 128 + 21, (T - 1) * 128 + 33, 8, 'rr', 1.0, 1.0)]


def xcd_specs():
    """Demoted to 64 x 64: two equal runs of 16 tiles (dealt as a pair over four XCDs each), a run of 12 and one of 5."""
    return [spec(256, 256, 24, 'rr', 1.0, 1.0), spec(256, 256, 24, 'rc', 1.0, 1.0), spec(192, 256, 24, 'cr', 1.0, 1.0),
            spec(64, 320, 24, 'cc', 1.0, 1.0)]


ORDINARY = (70, 90, 40)


def skinny_specs():
    """The streaming kernel (M <= 16, N >= 2048, every K <= 32, B row-major) next to one ordinary problem (last)."""
    out = []
    for M in (1, 5, 16):
        for N in (2048, 2049, 4097):
            for Ks in ((1,), (32,), (3, 10, 7)):
                for beta in (0.0, 0.5):
                    lay = tuple((a, False) for a, _ in alternating('rr', len(Ks)))   # A alternates, B stays row-major
                    out.append(Spec(M, N, Ks, lay, -2.0, beta, 'exact', f'{M}x{N}'))
    out.append(spec(*ORDINARY[:2], ORDINARY[2], 'rr', 1.0, 0.0))
    return out


def skinny_neighbour_specs():
    """Just outside the streaming kernel's conditions: 17 rows, a K of 33, a column-major B, 2047 columns."""
    return [spec(17, 2048, 10, 'rr', -2.0, 0.5), spec(5, 2049, 33, 'rr', -2.0, 0.0), spec(5, 2049, 10, 'rc', -2.0, 0.5),
            spec(16, 2047, 10, 'rr', -2.0, 0.0)]
