"""Call lists for the tests of what one C-ABI call leaves behind for the next (descriptor ring, workspaces, stream switch).

A :class:`Call` is ONE call of one entry point with its own inputs, its own output buffers and the numpy result those buffers
must hold afterwards.  Nothing here touches a device: ``launch(lib, handle, p)`` receives the addresses ``p[name]`` of the
buffers the runner made for ``inputs`` / ``outputs`` and builds the descriptors from them.  The same list is run on a quiet
context (synchronised around every call) and behind a gate with the host far ahead; every kernel used here documents a fixed
summation order without float atomics, so the two runs must agree byte for byte, and the quiet run is held against
``expected`` so that "equal but wrong" cannot pass.

Tolerances are those of the entry's own test file (named at each builder); 0 means ``np.array_equal``.
"""
import ctypes as C
import os
import re

import numpy as np

from cyten_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0      # what an output buffer holds before the call (test_gpu_diag_masks.py uses the same guard value)
MIB = 1 << 20


def ring_constants():
    """kSlots, kEvStride, kBig, kBigBytes as csrc/common.h declares them."""
    text = open(os.path.join(ROOT, 'cyten_amd', 'csrc', 'common.h')).read()
    out = {}
    for name in ('kSlots', 'kEvStride', 'kBig', 'kBigBytes'):
        m = re.search(r'static constexpr \w+ ' + name + r' = ([0-9 *]+);', text)
        assert m, f'{name} not found in common.h'
        out[name] = int(np.prod([int(f) for f in m.group(1).split('*')]))
    return out


def workspace_capacity(bytes_asked: int) -> int:
    """what cyb_ctx_s::workspace allocates when a slot has to grow (api.hip)"""
    return bytes_asked + bytes_asked // 4 + MIB


class Call:
    def __init__(self, entry, inputs, outputs, launch, expected, tol, uploads=1, big_uploads=0, extra_check=None, ws_bytes=None):
        self.entry = entry              # C-ABI name
        self.inputs = inputs            # name -> host array (read only on the device)
        self.outputs = outputs          # name -> host array the output buffer starts from (SENTINEL, or an in-place operand)
        self.launch = launch            # (lib, handle, p) -> status
        self.expected = expected        # name -> numpy result
        self.tol = tol                  # name -> absolute tolerance (scalar or array); 0: exact
        self.uploads = uploads          # descriptor uploads through the small ring (read from the entry's code)
        self.big_uploads = big_uploads  # ... through the ring of images above kBigBytes
        self.extra_check = extra_check  # optional (got: name -> array) -> None
        self.ws_bytes = ws_bytes        # (slot, bytes) the call asks cyb_ctx_s::workspace for, where a test depends on it

    def check(self, got):
        for name, want in self.expected.items():
            g = got[name]
            assert g.shape == want.shape and g.dtype == want.dtype, (self.entry, name, g.shape, want.shape)
            tol = self.tol[name]
            if np.ndim(tol) == 0 and tol == 0:
                assert np.array_equal(g, want), f'{self.entry}: {name} differs in {int((g != want).sum())} elements'
            else:
                err = np.abs(g - want)
                assert np.all(err <= tol), f'{self.entry}: {name} off by {np.max(err - tol):.3e} beyond its tolerance'
        if self.extra_check is not None:
            self.extra_check(got)


def _vp(addr):
    return C.c_void_p(int(addr))


def _a8(vals, ctype=C.c_int64, n=_lib.CYB_MAX_NDIM):
    vals = list(vals)
    return (ctype * n)(*(vals + [0] * (n - len(vals))))


def _sentinel(shape, dtype=np.float64):
    return np.full(shape, SENTINEL, dtype=dtype)


def _vec_descs(p, triples):
    return (_lib.VecDesc * len(triples))(*[_lib.VecDesc(p.get(x), p.get(y) if y else None, p.get(o) if o else None, n)
                                           for x, y, o, n in triples])


# ---------------------------------------------------------------------------------------------------------------- builders
# Each takes a numpy Generator and returns one Call.  Shapes: the smallest that still take a descriptor upload and more than
# one workgroup (three blocks around 17 x 33, vectors of a few thousand elements).

def copy_case(rng):
    """cyb_copy_strided_batched: three column slices of wider parents into contiguous blocks (test_gpu_blockops.py: exact)"""
    rows = (17, 18, 19)
    ins = {f'a{i}': rng.standard_normal((r, 40)) for i, r in enumerate(rows)}
    outs = {f'o{i}': _sentinel((r, 33)) for i, r in enumerate(rows)}

    def launch(lib, h, p):
        d = (_lib.CopyDesc * 3)(*[_lib.CopyDesc(p[f'o{i}'], p[f'a{i}'], 2, 0, _a8([r, 33]), _a8([33, 1]), _a8([40, 1]))
                                  for i, r in enumerate(rows)])
        return lib.cyb_copy_strided_batched(h, d, 3, 8)
    return Call('cyb_copy_strided_batched', ins, outs, launch, {f'o{i}': ins[f'a{i}'][:, :33].copy() for i in range(3)},
                {f'o{i}': 0 for i in range(3)})


def binary_case(rng):
    """cyb_binary_batched_f64, op 2 (mul): one correctly rounded operation (test_gpu_special_values.py: exact)"""
    ns = (3001, 257, 4100)
    ins, outs, exp = {}, {}, {}
    for i, n in enumerate(ns):
        ins[f'x{i}'], ins[f'y{i}'] = rng.standard_normal(n), rng.standard_normal(n)
        outs[f'o{i}'] = _sentinel(n)
        exp[f'o{i}'] = ins[f'x{i}'] * ins[f'y{i}']

    def launch(lib, h, p):
        return lib.cyb_binary_batched_f64(h, _vec_descs(p, [(f'x{i}', f'y{i}', f'o{i}', n) for i, n in enumerate(ns)]), 3, 2)
    return Call('cyb_binary_batched_f64', ins, outs, launch, exp, {k: 0 for k in exp})


def axpby_case(rng):
    """cyb_axpby_batched_f64 (test_gpu_complex.py: atol 1e-14 for entries of order one)"""
    ns = (3001, 33, 5000)
    a, b = 0.75, -1.5
    ins, outs, exp = {}, {}, {}
    for i, n in enumerate(ns):
        ins[f'x{i}'], ins[f'y{i}'] = rng.standard_normal(n), rng.standard_normal(n)
        outs[f'o{i}'] = _sentinel(n)
        exp[f'o{i}'] = a * ins[f'x{i}'] + b * ins[f'y{i}']

    def launch(lib, h, p):
        return lib.cyb_axpby_batched_f64(h, _vec_descs(p, [(f'x{i}', f'y{i}', f'o{i}', n) for i, n in enumerate(ns)]), 3, a, b)
    return Call('cyb_axpby_batched_f64', ins, outs, launch, exp,
                {k: 1e-14 * max(1.0, np.abs(v).max()) for k, v in exp.items()})


def lincomb_case(rng):
    """cyb_lincomb_strided_batched_f64: dst = 0.5 s0 - 1.25 s1^T, the transpose in the source strides (test_gpu_complex.py:
    atol 1e-13)"""
    shapes = ((17, 33), (18, 31), (16, 35))
    ins, outs, exp = {}, {}, {}
    for i, (r, c) in enumerate(shapes):
        ins[f's{i}'], ins[f't{i}'] = rng.standard_normal((r, c)), rng.standard_normal((c, r))
        outs[f'o{i}'] = _sentinel((r, c))
        exp[f'o{i}'] = 0.5 * ins[f's{i}'] - 1.25 * ins[f't{i}'].T

    def launch(lib, h, p):
        d = (_lib.LincombDesc * 3)(*[_lib.LincombDesc(p[f'o{i}'], 2, 0, 2 * i, 2 * i + 2, _a8([r, c]), _a8([c, 1]))
                                     for i, (r, c) in enumerate(shapes)])
        t = []
        for i, (r, c) in enumerate(shapes):
            t += [_lib.LincombTerm(p[f's{i}'], 0.5, _a8([c, 1])), _lib.LincombTerm(p[f't{i}'], -1.25, _a8([1, r]))]
        return lib.cyb_lincomb_strided_batched_f64(h, d, 3, (_lib.LincombTerm * 6)(*t), 6)
    return Call('cyb_lincomb_strided_batched_f64', ins, outs, launch, exp, {k: 1e-13 for k in exp})


def lincomb_c128_case(rng):
    """cyb_lincomb_strided_batched_c128: a complex and a real source under complex coefficients (atol 1e-13 as above)"""
    shapes = ((9, 17), (10, 15), (8, 19))
    c0, c1 = 0.5 - 2.0j, 1.25j
    ins, outs, exp = {}, {}, {}
    for i, (r, c) in enumerate(shapes):
        ins[f's{i}'] = rng.standard_normal((r, c)) + 1j * rng.standard_normal((r, c))
        ins[f't{i}'] = rng.standard_normal((r, c))
        outs[f'o{i}'] = _sentinel((r, c), np.complex128)
        exp[f'o{i}'] = c0 * ins[f's{i}'] + c1 * ins[f't{i}']

    def launch(lib, h, p):
        d = (_lib.LincombDesc * 3)(*[_lib.LincombDesc(p[f'o{i}'], 2, 0, 2 * i, 2 * i + 2, _a8([r, c]), _a8([c, 1]))
                                     for i, (r, c) in enumerate(shapes)])
        t = []
        for i, (r, c) in enumerate(shapes):
            t += [_lib.LincombTermC128(p[f's{i}'], c0.real, c0.imag, 0, 0, _a8([c, 1])),
                  _lib.LincombTermC128(p[f't{i}'], c1.real, c1.imag, 1, 0, _a8([c, 1]))]
        return lib.cyb_lincomb_strided_batched_c128(h, d, 3, (_lib.LincombTermC128 * 6)(*t), 6)
    return Call('cyb_lincomb_strided_batched_c128', ins, outs, launch, exp, {k: 1e-13 for k in exp})


def scale_axis_case(rng):
    """cyb_scale_axis_batched_f64 (test_gpu_complex.py: atol 1e-15)"""
    shapes = ((5, 17, 7), (3, 33, 4), (6, 9, 11))
    ins, outs, exp = {}, {}, {}
    for i, (o, a, n) in enumerate(shapes):
        ins[f'x{i}'], ins[f'f{i}'] = rng.standard_normal((o, a, n)), rng.standard_normal(a)
        outs[f'o{i}'] = _sentinel((o, a, n))
        exp[f'o{i}'] = ins[f'x{i}'] * ins[f'f{i}'][None, :, None]

    def launch(lib, h, p):
        d = (_lib.ScaleAxisDesc * 3)(*[_lib.ScaleAxisDesc(p[f'x{i}'], p[f'f{i}'], p[f'o{i}'], o, a, n)
                                       for i, (o, a, n) in enumerate(shapes)])
        return lib.cyb_scale_axis_batched_f64(h, d, 3)
    return Call('cyb_scale_axis_batched_f64', ins, outs, launch, exp, {k: 1e-15 * max(1.0, np.abs(v).max()) for k, v in exp.items()})


def _mask_case(rng, scatter):
    shapes = ((5, 17, 7), (3, 33, 4), (6, 9, 11))
    ins, outs, exp = {}, {}, {}
    keeps = []
    for i, (o, a, n) in enumerate(shapes):
        idx = np.sort(rng.choice(a, size=a // 2 + 1, replace=False)).astype(np.int64)
        keeps.append(len(idx))
        ins[f'i{i}'] = idx
        if scatter:
            ins[f'x{i}'] = rng.standard_normal((o, len(idx), n))
            outs[f'o{i}'] = _sentinel((o, a, n))
            exp[f'o{i}'] = np.zeros((o, a, n))
            exp[f'o{i}'][:, idx, :] = ins[f'x{i}']
        else:
            ins[f'x{i}'] = rng.standard_normal((o, a, n))
            outs[f'o{i}'] = _sentinel((o, len(idx), n))
            exp[f'o{i}'] = ins[f'x{i}'][:, idx, :].copy()

    def launch(lib, h, p):
        d = (_lib.MaskDesc * 3)(*[_lib.MaskDesc(p[f'x{i}'], p[f'o{i}'], p[f'i{i}'], o, a, n, keeps[i])
                                  for i, (o, a, n) in enumerate(shapes)])
        return (lib.cyb_mask_scatter_batched_f64 if scatter else lib.cyb_mask_gather_batched_f64)(h, d, 3)
    name = 'cyb_mask_scatter_batched_f64' if scatter else 'cyb_mask_gather_batched_f64'
    return Call(name, ins, outs, launch, exp, {k: 0 for k in exp})


def mask_gather_case(rng):
    """cyb_mask_gather_batched_f64 (test_gpu_complex.py / test_gpu_abelian.py: exact)"""
    return _mask_case(rng, False)


def mask_scatter_case(rng):
    """cyb_mask_scatter_batched_f64: scatter into zeros (exact)"""
    return _mask_case(rng, True)


SEG_F64, SEG_BOOL = 1, 3


def seg_binary_case(rng):
    """cyb_seg_binary, add: one owner class per segment -- 16 lanes, a wave, chunks of 16384 (test_gpu_diag_masks.py: exact)"""
    ns = (50, 900, 20000)
    ins, outs, exp = {}, {}, {}
    for i, n in enumerate(ns):
        ins[f'a{i}'], ins[f'b{i}'] = rng.standard_normal(n), rng.standard_normal(n)
        outs[f'o{i}'] = _sentinel(n)
        exp[f'o{i}'] = ins[f'a{i}'] + ins[f'b{i}']

    def launch(lib, h, p):
        r = (_lib.SegRec * 3)(*[_lib.SegRec(p[f'a{i}'], p[f'b{i}'], p[f'o{i}'], n, SEG_F64, SEG_F64, SEG_F64, 0) for i, n in enumerate(ns)])
        return lib.cyb_seg_binary(h, r, 3, 0, 0, 0.0, 0.0)
    return Call('cyb_seg_binary', ins, outs, launch, exp, {k: 0 for k in exp})


SEG_CHUNK = 16384    # kChunk of segment_ops.hip: longer segments leave chunk partials and a ticket in workspace slot 6


def seg_reduce_case(rng, ns=(50, 900, 40000)):
    """cyb_seg_reduce, sum: the last segment has three chunks, whose partials and ticket live in workspace slot 6
    (test_gpu_diag_masks.py: 1e-12 relative, here of sum |x|)"""
    ins = {f'a{i}': rng.standard_normal(n) for i, n in enumerate(ns)}
    want = np.zeros(2 * len(ns))
    want[0::2] = [ins[f'a{i}'].sum() for i in range(len(ns))]
    tol = np.zeros(2 * len(ns))
    tol[0::2] = [1e-12 * np.abs(ins[f'a{i}']).sum() for i in range(len(ns))]

    def launch(lib, h, p):
        r = (_lib.SegRec * len(ns))(*[_lib.SegRec(p[f'a{i}'], None, None, n, SEG_F64, 0, 0, 0) for i, n in enumerate(ns)])
        return lib.cyb_seg_reduce(h, r, len(ns), 0, 0, 0.0, _vp(p['r']))
    parts = sum(-(-n // SEG_CHUNK) for n in ns if n > SEG_CHUNK)
    multi = sum(1 for n in ns if n > SEG_CHUNK)
    return Call('cyb_seg_reduce', ins, {'r': _sentinel(2 * len(ns))}, launch, {'r': want}, {'r': tol}, ws_bytes=(6, 16 * parts + 4 * multi))


def seg_compact_case(rng):
    """cyb_seg_compact of boolean flags: ascending kept positions and counts; entries beyond a segment's count are not
    written and keep the sentinel (test_gpu_diag_masks.py: exact)"""
    ns = (50, 900, 20000)
    ins = {f'a{i}': rng.random(n) < 0.4 for i, n in enumerate(ns)}
    keep = np.full(sum(ns), -1, dtype=np.int64)
    off = 0
    for i, n in enumerate(ns):
        pos = np.flatnonzero(ins[f'a{i}'])
        keep[off:off + len(pos)] = pos
        off += n
    counts = np.array([ins[f'a{i}'].sum() for i in range(3)], dtype=np.int64)

    def launch(lib, h, p):
        r = (_lib.SegRec * 3)(*[_lib.SegRec(p[f'a{i}'], None, None, n, SEG_BOOL, 0, 0, 0) for i, n in enumerate(ns)])
        return lib.cyb_seg_compact(h, r, 3, _vp(p['keep']), _vp(p['counts']))
    return Call('cyb_seg_compact', ins, {'keep': np.full(sum(ns), -1, dtype=np.int64), 'counts': np.full(3, -1, dtype=np.int64)}, launch,
                {'keep': keep, 'counts': counts}, {'keep': 0, 'counts': 0})


def trace_case(rng):
    """cyb_trace_grouped_f64: out[r] = sum_t src[t, r, t] (test_gpu_abelian_tensor_ops.py compares at 1e-12 of the scale; here
    1e-13 of sum |addends| per element)"""
    shapes = ((6, 17, 6), (4, 33, 4), (9, 5, 9))
    ins = {f's{i}': rng.standard_normal(s) for i, s in enumerate(shapes)}
    outs = {f'o{i}': _sentinel(s[1]) for i, s in enumerate(shapes)}
    exp = {f'o{i}': np.trace(ins[f's{i}'], axis1=0, axis2=2) for i in range(3)}
    tol = {f'o{i}': 1e-13 * np.trace(np.abs(ins[f's{i}']), axis1=0, axis2=2) for i in range(3)}

    def launch(lib, h, p):
        o = (_lib.TraceOut * 3)(*[_lib.TraceOut(p[f'o{i}'], 1, 0, i, 1, _a8([s[1]])) for i, s in enumerate(shapes)])
        t = (_lib.TraceTerm * 3)(*[_lib.TraceTerm(p[f's{i}'], 1, 0, _a8([s[2]]), _a8([s[0]], n=4), _a8([s[1] * s[2] + 1], n=4))
                                   for i, s in enumerate(shapes)])
        return lib.cyb_trace_grouped_f64(h, o, 3, t, 3)
    return Call('cyb_trace_grouped_f64', ins, outs, launch, exp, tol)


def outer_case(rng):
    """cyb_outer_grouped_f64 with k = n_a: dst[i, j] = a[i] b[j], one product per element (test_gpu_tensor_products.py: exact)"""
    shapes = ((17, 33), (40, 9), (5, 64))
    ins, outs, exp = {}, {}, {}
    for i, (na, nb) in enumerate(shapes):
        ins[f'a{i}'], ins[f'b{i}'] = rng.standard_normal(na), rng.standard_normal(nb)
        outs[f'o{i}'] = _sentinel((na, nb))
        exp[f'o{i}'] = np.multiply.outer(ins[f'a{i}'], ins[f'b{i}'])

    def launch(lib, h, p):
        r = (_lib.OuterRec * 3)(*[_lib.OuterRec(p[f'o{i}'], p[f'a{i}'], p[f'b{i}'], 1, 1, 1, 0, 0, 0, _a8([na]), _a8([1]), _a8([nb]), _a8([1]))
                                  for i, (na, nb) in enumerate(shapes)])
        return lib.cyb_outer_grouped_f64(h, r, 3)
    return Call('cyb_outer_grouped_f64', ins, outs, launch, exp, {k: 0 for k in exp})


def tree_axis_case(rng):
    """cyb_tree_axis_f64, CYB_TREE_SCALE on codomain records: dst(t, x) = table[(t / inner) % A] src(t, x), one product per
    element (test_gpu_tree_ops.py: exact)"""
    shapes = ((2, 5, 3, 33), (3, 4, 2, 17), (1, 9, 4, 21))   # outer, A, inner, X
    ins, outs, exp = {}, {}, {}
    for i, (o, a, n, x) in enumerate(shapes):
        ins[f's{i}'], ins[f'f{i}'] = rng.standard_normal((o * a * n, x)), rng.standard_normal(a)
        outs[f'o{i}'] = _sentinel((o * a * n, x))
        exp[f'o{i}'] = ins[f's{i}'] * ins[f'f{i}'][(np.arange(o * a * n) // n) % a][:, None]

    def launch(lib, h, p):
        r = (_lib.TreeAxisRec * 3)(*[_lib.TreeAxisRec(p[f's{i}'], p[f'o{i}'], p[f'f{i}'], x, 1, x, 1, 0, 0, x, o, a, a, n, 0, 0, 0, 0)
                                     for i, (o, a, n, x) in enumerate(shapes)])
        return lib.cyb_tree_axis_f64(h, r, 3, None, 0)
    return Call('cyb_tree_axis_f64', ins, outs, launch, exp, {k: 0 for k in exp})


def expm_case(rng):
    """cyb_expm_small_batched_f64 against scipy.linalg.expm at 1e-10 max |want| (test_gpu_tensor_functions.py)"""
    import scipy.linalg
    ns = (17, 33, 9)
    alpha = -0.5
    ins = {f'a{i}': rng.standard_normal((n, n)) * (2.0 / np.sqrt(n)) for i, n in enumerate(ns)}
    outs = {f'e{i}': _sentinel((n, n)) for i, n in enumerate(ns)}
    exp = {f'e{i}': scipy.linalg.expm(alpha * ins[f'a{i}']) for i in range(3)}

    def launch(lib, h, p):
        d = (_lib.ExpmDesc * 3)(*[_lib.ExpmDesc(p[f'a{i}'], n, n, 0, 0, p[f'e{i}'], n) for i, n in enumerate(ns)])
        return lib.cyb_expm_small_batched_f64(h, d, 3, alpha)
    return Call('cyb_expm_small_batched_f64', ins, outs, launch, exp, {k: 1e-10 * np.abs(v).max() for k, v in exp.items()})


def dot_c128_case(rng, ns=(3001, 257, 4100)):
    """cyb_dot_batched_c128: sum over the list of <x, y>; more than one entry, so the descriptors are uploaded; partials in
    workspace slot 0 (test_krylov.py / test_gpu_complex.py: 1e-13 of sum |x| |y|)"""
    ins = {}
    for i, n in enumerate(ns):
        ins[f'x{i}'] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        ins[f'y{i}'] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    z = sum(np.vdot(ins[f'x{i}'], ins[f'y{i}']) for i in range(len(ns)))
    scale = sum(np.abs(ins[f'x{i}']) @ np.abs(ins[f'y{i}']) for i in range(len(ns)))

    def launch(lib, h, p):
        return lib.cyb_dot_batched_c128(h, _vec_descs(p, [(f'x{i}', f'y{i}', None, n) for i, n in enumerate(ns)]), len(ns), _vp(p['r']))
    chunk = min(1 << 15, max(4096, ((sum(ns) // 2048) + 511) & ~511))      # chunk_complex of flat_items.h
    items = sum(-(-n // chunk) for n in ns)
    return Call('cyb_dot_batched_c128', ins, {'r': _sentinel(2)}, launch, {'r': np.array([z.real, z.imag])}, {'r': 1e-13 * scale},
                uploads=1 if len(ns) > 1 else 0, ws_bytes=(0, 16 * max(items, 1)))


def gemm_case(rng, shapes=((17, 21, 33), (40, 7, 9), (70, 64, 90))):
    """cyb_gemm_grouped_enqueue_f64, one segment per problem (test_gpu_gemm.py: 1e-10 of the scale; here the forward bound
    K eps |A| |B| per element with a factor 4, far below it)"""
    ins, outs, exp, tol = {}, {}, {}, {}
    for i, (m, k, n) in enumerate(shapes):
        ins[f'a{i}'], ins[f'b{i}'] = rng.standard_normal((m, k)), rng.standard_normal((k, n))
        outs[f'c{i}'] = _sentinel((m, n))
        exp[f'c{i}'] = ins[f'a{i}'] @ ins[f'b{i}']
        tol[f'c{i}'] = 4 * k * np.finfo(float).eps * (np.abs(ins[f'a{i}']) @ np.abs(ins[f'b{i}']))

    def launch(lib, h, p):
        pr = (_lib.GemmProb * len(shapes))(*[_lib.GemmProb(p[f'c{i}'], m, n, n, i, i + 1, 1.0, 0.0) for i, (m, k, n) in enumerate(shapes)])
        sg = (_lib.GemmSeg * len(shapes))(*[_lib.GemmSeg(p[f'a{i}'], p[f'b{i}'], k, k, 1, n, 1) for i, (m, k, n) in enumerate(shapes)])
        return lib.cyb_gemm_grouped_enqueue_f64(h, pr, len(shapes), sg, len(shapes))
    return Call('cyb_gemm_grouped_enqueue_f64', ins, outs, launch, exp, tol)


TRUNC_LDS_MAX = 8192     # NMAX of truncation.hip: longer lists sort in chunks with keys, indices and flags in workspace slot 2
TRUNC_MAX = 65536        # NBIG: more values are CYB_ERR_UNSUPPORTED


def truncate_ws_bytes(n):
    """what cyb_truncate_select_f64 asks workspace slot 2 for (truncation.hip)"""
    if n <= TRUNC_LDS_MAX:
        return 8 * n
    n2 = 2
    while n2 < n:
        n2 <<= 1
    n2 = max(n2, 2 * TRUNC_LDS_MAX)
    off_key = (8 * n + 255) & ~255
    return off_key + 8 * n2 + 4 * n2 + n2


def truncate_case(rng, sizes=(40, 60, 33), chi_max=50, chi_min=1):
    """cyb_truncate_select_f64 against the host selection cyten_amd.abelian.truncation_selection: identical mask and tables,
    err / new_norm at 1e-13 of their sum (1e-12 beyond one LDS sort), as test_gpu_abelian.py.  chi_min = 0 (CYB_ERR_INVALID) and
    more than 65536 values (CYB_ERR_UNSUPPORTED) are the failing forms: `expected` is then what the outputs started from."""
    from cyten_amd import abelian as ab
    S = [np.sort(np.abs(rng.standard_normal(k)) + 1e-3)[::-1].copy() for k in sizes]
    n = sum(sizes)
    mask, err, norm = ab.truncation_selection(np.concatenate(S), chi_max=chi_max)
    mask = np.asarray(mask, dtype=bool)
    keep = np.full(n, -1, dtype=np.int64)
    counts = np.zeros(len(sizes), dtype=np.int64)
    off = 0
    for s, k in enumerate(sizes):
        pos = np.flatnonzero(mask[off:off + k])
        keep[off:off + len(pos)] = pos
        counts[s] = len(pos)
        off += k
    res = np.concatenate([[err, norm], counts.view(np.float64)])
    tol = np.zeros(2 + len(sizes))
    tol[:2] = (1e-13 if n <= TRUNC_LDS_MAX else 1e-12) * (err + norm)
    ins = {f's{i}': s for i, s in enumerate(S)}

    def launch(lib, h, p):
        opts = _lib.TruncOpts(chi_max, chi_min, 0.0, 0.0, 0.0, 0, 1)
        return lib.cyb_truncate_select_f64(h, _vec_descs(p, [(f's{i}', None, None, k) for i, k in enumerate(sizes)]), len(sizes),
                                           C.byref(opts), _vp(p['keep']), _vp(p['mask']), _vp(p['res']))
    outs = {'keep': np.full(n, -1, dtype=np.int64), 'mask': np.full(n, 7, dtype=np.uint8), 'res': _sentinel(2 + len(sizes))}
    if chi_min < 1 or n > TRUNC_MAX:     # rejected before anything is enqueued
        return Call('cyb_truncate_select_f64', ins, outs, launch, {k: v.copy() for k, v in outs.items()}, {k: 0 for k in outs}, uploads=0)
    return Call('cyb_truncate_select_f64', ins, outs, launch,
                {'keep': keep, 'mask': mask.astype(np.uint8), 'res': res}, {'keep': 0, 'mask': 0, 'res': tol}, ws_bytes=(2, truncate_ws_bytes(n)))


def extremum_case(rng, n=5000):
    """cyb_extremum_f64, mode 2 (max |x|) with its index; partials in workspace slot 2 (test_gpu_special_values.py: exact)"""
    x = rng.standard_normal(n)
    i = int(np.argmax(np.abs(x)))
    want = np.array([np.abs(x[i]), np.array([i], dtype=np.int64).view(np.float64)[0]])

    def launch(lib, h, p):
        return lib.cyb_extremum_f64(h, _vp(p['x']), n, 2, _vp(p['r']))
    return Call('cyb_extremum_f64', {'x': x}, {'r': _sentinel(2)}, launch, {'r': want}, {'r': 0}, uploads=0,
                ws_bytes=(2, 16 * min(-(-n // 2048), 1024)))


GS_MAX_M, GS_MAX_GRID, GS_TILE_F64 = 64, 2048, 256   # krylov_vec.hip


def gs_ws_bytes(n, m):
    """what cyb_gram_schmidt_f64 / cyb_multi_dot_f64 ask workspace slot 0 for (gs_grid and gs_workspace of krylov_vec.hip)"""
    tiles = -(-n // GS_TILE_F64)
    tpg = max(1, -(-tiles // GS_MAX_GRID))
    groups = max(-(-tiles // tpg), 1)
    return 8 * (groups * (m + 1) * 2 + 4 * GS_MAX_M)


def gram_schmidt_case(rng, n=4099, m=3, alias=False):
    """cyb_gram_schmidt_f64, one pass: coefficients at 1e-13 |v_j| |w|, w at 1e-12 |w|, the norm at 1e-13 of the norm of the
    returned w (test_krylov_gmres.py).  The basis pointers travel as kernel arguments: no descriptor upload.  `alias`: all m
    pointers name ONE unit vector (classical Gram-Schmidt then subtracts m times its component), which keeps the large case
    small; the basis is then not orthonormal and w is held to 1e-12 (|w| + sum |h_j| |v_j|), that file's rule for such bases."""
    w0 = rng.standard_normal(n)
    if alias:
        v = rng.standard_normal(n)
        v /= np.linalg.norm(v)
        V = np.broadcast_to(v, (m, n))
        ins = {'V': v.copy()}
    else:
        V = np.linalg.qr(rng.standard_normal((n, m)))[0].T.copy()
        ins = {'V': V}
    h = V @ w0
    w = w0 - h @ V
    nw0 = np.linalg.norm(w0)
    out = np.concatenate([h, [np.linalg.norm(w)]])
    tol_w = 1e-12 * (nw0 + (np.abs(h) @ np.linalg.norm(V, axis=1) if alias else 0.0))
    tol_out = np.concatenate([1e-13 * np.linalg.norm(V, axis=1) * nw0, [np.sqrt(n) * tol_w]])   # (| |a| - |b| | <= |a - b|)

    def launch(lib, hd, p):
        ptrs = (C.c_void_p * m)(*[p['V'] + (0 if alias else 8 * n * j) for j in range(m)])
        return lib.cyb_gram_schmidt_f64(hd, ptrs, m, _vp(p['w']), n, 1, _vp(p['out']))

    def norm_of_returned_w(got):
        nw = np.linalg.norm(got['w'])
        assert abs(got['out'][m] - nw) <= 1e-13 * max(nw, 1e-300)
    if m > GS_MAX_M:     # CYB_ERR_UNSUPPORTED: nothing is enqueued, the buffers keep what they held
        return Call('cyb_gram_schmidt_f64', ins, {'w': w0.copy(), 'out': _sentinel(m + 1)}, launch, {'w': w0.copy(), 'out': _sentinel(m + 1)},
                    {'w': 0, 'out': 0}, uploads=0)
    return Call('cyb_gram_schmidt_f64', ins, {'w': w0.copy(), 'out': _sentinel(m + 1)}, launch, {'w': w, 'out': out},
                {'w': tol_w, 'out': tol_out}, uploads=0, extra_check=norm_of_returned_w, ws_bytes=(0, gs_ws_bytes(n, m)))


SMALL_RING_BUILDERS = [copy_case, binary_case, axpby_case, lincomb_case, lincomb_c128_case, scale_axis_case, mask_gather_case,
                       mask_scatter_case, seg_binary_case, seg_reduce_case, seg_compact_case, trace_case, outer_case, tree_axis_case,
                       expm_case, dot_c128_case, gemm_case, truncate_case, gram_schmidt_case]


def small_ring_sequence(seed=0, rounds=5):
    """`rounds` passes over every entry, each call with inputs of its own: 18 entries of one descriptor upload each and the
    Gram-Schmidt step (no upload) per pass -- 90 uploads in 95 calls, so that every ring slot is refilled at least twice."""
    return [b(np.random.default_rng([seed, r, i])) for r in range(rounds) for i, b in enumerate(SMALL_RING_BUILDERS)]


def dummy_upload_calls(k, seed=99):
    """k calls of one upload each, to move the ring's phase before a sequence starts"""
    return [copy_case(np.random.default_rng([seed, i])) for i in range(k)]


def big_copy_case(rng):
    """cyb_copy_strided_batched of so many tiny row copies that the descriptor image exceeds kBigBytes: the library's device
    descriptor (CopyDev, copy_kernels.h) is no smaller than cyb_copy_desc, so counting with the latter is safe.  Row i of the
    source goes to row perm[i] of the destination."""
    n = ring_constants()['kBigBytes'] // C.sizeof(_lib.CopyDesc) + 1
    src = rng.standard_normal((n, 4))
    perm = rng.permutation(n)
    want = np.empty_like(src)
    want[perm] = src

    def launch(lib, h, p):
        d = np.zeros(n, dtype=_lib.COPY_DTYPE)
        d['dst'] = p['o'] + 32 * perm
        d['src'] = p['s'] + 32 * np.arange(n)
        d['ndim'] = 1
        d['shape'][:, 0] = 4
        d['dst_strides'][:, 0] = 1
        d['src_strides'][:, 0] = 1
        return lib.cyb_copy_strided_batched(h, d.ctypes.data_as(C.POINTER(_lib.CopyDesc)), n, 8)
    c = Call('cyb_copy_strided_batched', {'s': src}, {'o': _sentinel((n, 4))}, launch, {'o': want}, {'o': 0}, uploads=0, big_uploads=1)
    c.image_bytes_min = n * C.sizeof(_lib.CopyDesc)
    return c


def big_ring_sequence(seed=1, n_big=20):
    """n_big calls through the big ring, each followed by one small-ring call of another entry"""
    small = [axpby_case, seg_compact_case, gemm_case, trace_case, lincomb_case]
    out = []
    for i in range(n_big):
        out.append(big_copy_case(np.random.default_rng([seed, i, 0])))
        out.append(small[i % len(small)](np.random.default_rng([seed, i, 1])))
    return out


def growth_sequences(seed=2):
    """Per workspace slot: small calls, a call that needs more than the capacity they left, the small calls again.

    slot 0: Gram-Schmidt (n = 4099, m = 3) and dot_batched_c128, then Gram-Schmidt with 64 basis pointers on 2048 workgroups
            (2.1 MB of partials; the basis aliases one vector: 8 MiB of operands).  dot_batched_c128 alone cannot outgrow the
            first megabyte below 4 GB of operands.
    slot 2: cyb_extremum_f64 and a 133-value truncate_select, then a truncate_select of 60000 values (chunked sort: 1.3 MB).
            The extremum partials never exceed 16 KiB.
    slot 6 is left out: seg_reduce takes 16 bytes per 16384-element chunk, so outgrowing the first megabyte needs more than
            65536 chunks -- 1 GiB of flags or 8 GiB of doubles, far beyond 64 MiB.  Its first allocation in flight is part of
            the small-ring sequence (seg_reduce_case)."""
    def r(*k):
        return np.random.default_rng([seed, *k])
    sizes_big = tuple([60000 - 36 * 1500] + [1500] * 36)
    return {
        0: dict(before=[gram_schmidt_case(r(0, 0)), dot_c128_case(r(0, 1))],
                grow=gram_schmidt_case(r(0, 2), n=GS_MAX_GRID * GS_TILE_F64 - 3, m=GS_MAX_M, alias=True),
                after=[gram_schmidt_case(r(0, 3)), dot_c128_case(r(0, 4))]),
        2: dict(before=[extremum_case(r(2, 0)), truncate_case(r(2, 1))],
                grow=truncate_case(r(2, 2), sizes=sizes_big, chi_max=20000),
                after=[extremum_case(r(2, 3)), truncate_case(r(2, 4))]),
    }


def stream_chain(seed=3):
    """A dependent chain in ONE buffer namespace (the runner shares the buffers between the calls):
    first half   c = a b (GEMM); ct = c^T (strided copy); d0 = <x, y> (slot 0)
    second half  r = sum ct (seg_reduce, three chunks: slot 6); z = 2 ct (axpby); d1 = <c, c> read as complex (slot 0)
    final        f = ct + z (binary add)."""
    rng = np.random.default_rng(seed)
    m, k, n = 192, 48, 256          # c has 49152 elements: three chunks of the segment reduction
    a, b = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    x, y = (rng.standard_normal(3000) + 1j * rng.standard_normal(3000) for _ in range(2))
    c = a @ b
    tol_c = 4 * k * np.finfo(float).eps * (np.abs(a) @ np.abs(b))
    cz = c.reshape(-1).view(np.complex128)
    d0, d1 = np.vdot(x, y), np.vdot(cz, cz)
    tiny = 1e-12 * np.abs(c).max()
    calls = [
        Call('cyb_gemm_grouped_enqueue_f64', {'a': a, 'b': b}, {'c': _sentinel((m, n))},
             lambda lib, h, p: lib.cyb_gemm_grouped_enqueue_f64(h, (_lib.GemmProb * 1)(_lib.GemmProb(p['c'], m, n, n, 0, 1, 1.0, 0.0)), 1,
                                                                (_lib.GemmSeg * 1)(_lib.GemmSeg(p['a'], p['b'], k, k, 1, n, 1)), 1),
             {'c': c}, {'c': tol_c}),
        Call('cyb_copy_strided_batched', {}, {'ct': _sentinel((n, m))},
             lambda lib, h, p: lib.cyb_copy_strided_batched(h, (_lib.CopyDesc * 1)(_lib.CopyDesc(p['ct'], p['c'], 2, 0, _a8([n, m]), _a8([m, 1]),
                                                                                                 _a8([1, n]))), 1, 8),
             {'ct': c.T.copy()}, {'ct': tol_c.T}),
        Call('cyb_dot_batched_c128', {'x': x, 'y': y, 'pad': np.zeros(2)}, {'d0': _sentinel(2)},
             lambda lib, h, p: lib.cyb_dot_batched_c128(h, _vec_descs(p, [('x', 'y', None, 3000), ('pad', 'pad', None, 1)]), 2, _vp(p['d0'])),
             {'d0': np.array([d0.real, d0.imag])}, {'d0': 1e-13 * (np.abs(x) @ np.abs(y))}),
        Call('cyb_seg_reduce', {}, {'r': _sentinel(2)},
             lambda lib, h, p: lib.cyb_seg_reduce(h, (_lib.SegRec * 1)(_lib.SegRec(p['ct'], None, None, m * n, SEG_F64, 0, 0, 0)), 1, 0, 0, 0.0,
                                                  _vp(p['r'])),
             {'r': np.array([c.sum(), 0.0])}, {'r': np.array([1e-12 * np.abs(c).sum(), 0.0])}),
        Call('cyb_axpby_batched_f64', {}, {'z': _sentinel((n, m))},
             lambda lib, h, p: lib.cyb_axpby_batched_f64(h, _vec_descs(p, [('ct', None, 'z', m * n), ('pad', None, 'pad2', 2)]), 2, 2.0, 0.0),
             {'z': 2 * c.T}, {'z': 2 * tol_c.T + tiny}),
        Call('cyb_dot_batched_c128', {}, {'d1': _sentinel(2)},
             lambda lib, h, p: lib.cyb_dot_batched_c128(h, _vec_descs(p, [('c', 'c', None, m * n // 2), ('pad', 'pad', None, 1)]), 2, _vp(p['d1'])),
             {'d1': np.array([d1.real, d1.imag])}, {'d1': 2 * (np.abs(c) * tol_c).sum() + 1e-13 * abs(d1)}),   # (error of c, then of the sum)
        Call('cyb_binary_batched_f64', {}, {'f': _sentinel((n, m))},
             lambda lib, h, p: lib.cyb_binary_batched_f64(h, _vec_descs(p, [('ct', 'z', 'f', m * n), ('pad', 'pad', 'pad2', 2)]), 2, 0),
             {'f': 3 * c.T}, {'f': 3 * tol_c.T + tiny}),
    ]
    calls[4].outputs['pad2'] = _sentinel(2)
    return dict(calls=calls, first=calls[:3], second=calls[3:6], final=calls[6:])


def count_uploads(calls):
    return sum(c.uploads for c in calls), sum(c.big_uploads for c in calls)


# ---------------------------------------------------------------------------------------------------------------- ring model

def gate_points(calls, k):
    """Indices of the calls in front of which a gate goes.  The ring makes the host wait for the device by itself (upload()
    synchronises on an event at most kSlots/2 uploads old, counted per ring), so ONE gate in front of a long sequence is gone
    by the time upload kSlots is made.  A new gate in front of every call that starts a stretch of kEvStride small or kBig/4
    big uploads keeps the device behind the host across those waits: whatever event upload() waits for, a younger gate is
    already queued behind it."""
    pts, small, big = [0], 0, 0
    for i, c in enumerate(calls):
        if i and (small >= k['kEvStride'] or big >= k['kBig'] // 4):
            pts.append(i)
            small = big = 0
        small += c.uploads
        big += c.big_uploads
    return pts


def waited_event(j, k_slots, k_stride):
    """the upload index whose event upload j waits for (cyb_ctx_s::upload, small ring), or None"""
    if j < k_slots:
        return None
    return (j - k_slots // 2 + k_stride - 1) // k_stride * k_stride


def waited_event_big(j, k_big):
    """the same for the ring of big images: every big upload records an event"""
    return None if j < k_big else j - k_big // 2
