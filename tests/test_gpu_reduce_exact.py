"""The fixed-order reductions at the edges of their work items, with data on which every order gives the same bits.

Elements are integers of magnitude at most 4 (Gaussian integers for complex data) and weights are powers of two, so every
product and every partial sum is an exact double whatever the order of summation: the results must EQUAL numpy's.  What
this pins down is therefore not the order but the cover -- every element exactly once, the tails of the 16-byte paths,
the item and tile boundaries, the alignment fallbacks, the segment table of the per-entry form.
"""
import ctypes as C

import numpy as np
import pytest

from cyten_amd import _lib

pytestmark = pytest.mark.gpu

REAL_N = (0, 1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 16385)
CPLX_N = (0, 1, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8193)
GRANULE = 256  # elements per entry of a weight table of the projection kernels


def _ints(rng, shape, cplx=False):
    a = rng.integers(-4, 5, size=shape).astype(np.float64)
    return a + 1j * rng.integers(-4, 5, size=shape) if cplx else a


def _vec(bb, a, shift):
    """1-D block of `a`; shift: at an odd float64 element of its buffer, so that it is not 16-byte aligned"""
    if not shift:
        x = bb.as_block(a)
        assert a.size == 0 or x.ptr % 16 == 0
        return x
    x = bb.get_item(bb.as_block(np.concatenate([[7.0], a])), (slice(1, None),))
    assert x.ptr % 16 == 8 and x.is_contiguous()
    return x


def _dot(bb, xs, ys=None):
    return float(bb._reduce(bb.lib.cyb_dot_batched_f64, xs, ys)[0])


def test_real_reductions_at_item_edges(bb, rng):
    for n in REAL_N:
        a, b = _ints(rng, n), _ints(rng, n)
        for sx, sy in ((False, False), (True, False), (False, True)):
            x, y = _vec(bb, a, sx), _vec(bb, b, sy)
            what = f'n={n} x shifted={sx} y shifted={sy}'
            assert bb.inner_many([x], [y]) == float(np.dot(a, b)), what
            assert _dot(bb, [x]) == float(np.dot(a, a)), what
            assert bb.max_abs_many([x]) == (float(np.max(np.abs(a))) if n else 0.0), what


def test_max_abs_keeps_a_nan_in_the_last_element(bb, rng):
    a = _ints(rng, 8193)
    a[8192] = np.nan
    for shift in (False, True):
        assert np.isnan(bb.max_abs_many([_vec(bb, a, shift)]))
    a[8192] = 3.0
    assert bb.max_abs_many([_vec(bb, a, False)]) == float(np.max(np.abs(a)))


def test_real_lists_equal_their_one_vector_calls(bb, rng):
    sizes = (0, 1, 8193, 3)
    A, B = [_ints(rng, n) for n in sizes], [_ints(rng, n) for n in sizes]
    X, Y = [bb.as_block(a) for a in A], [bb.as_block(b) for b in B]
    one_xy = [bb.inner_many([x], [y]) for x, y in zip(X, Y)]
    one_xx = [_dot(bb, [x]) for x in X]
    one_max = [bb.max_abs_many([x]) for x in X]
    assert one_xy == [float(np.dot(a, b)) for a, b in zip(A, B)]
    assert bb.inner_many(X, Y) == sum(one_xy)
    assert _dot(bb, X) == sum(one_xx) == float(sum(np.dot(a, a) for a in A))
    assert bb.max_abs_many(X) == max(one_max) == max(float(np.max(np.abs(a))) for a in A if a.size)
    # one result per entry: the segment table of stage 2
    each = bb._reduce(bb.lib.cyb_dot_each_f64, X, Y, n_results=len(X))
    assert each.tolist() == one_xy
    each = bb._reduce(bb.lib.cyb_dot_each_f64, X, None, n_results=len(X))
    assert each.tolist() == one_xx


def test_empty_list_at_the_c_abi_writes_its_zero(bb):
    """n = 0 with descs = NULL: "0 for an empty list" (the Python wrappers return before they would make this call)"""
    for name, k in (('cyb_dot_batched_f64', 1), ('cyb_maxabs_batched_f64', 1), ('cyb_dot_batched_c128', 2)):
        res = bb.as_block(np.full(k, 7.0))
        bb.ctx.sync_stream()
        _lib.check(getattr(bb.lib, name)(bb.ctx.handle, None, 0, C.c_void_p(res.ptr)))
        assert bb.to_numpy(res).tolist() == [0.0] * k, name
    # one result per entry: no entry, nothing written
    res = bb.as_block(np.full(1, 7.0))
    bb.ctx.sync_stream()
    _lib.check(bb.lib.cyb_dot_each_f64(bb.ctx.handle, None, 0, C.c_void_p(res.ptr)))
    assert bb.to_numpy(res).tolist() == [7.0]


def test_complex_inner_at_item_edges(bb, rng):
    for n in CPLX_N:
        a, b = _ints(rng, n, True), _ints(rng, n, True)
        got = bb.inner_many([bb.as_block(a)], [bb.as_block(b)])
        assert got == complex(np.vdot(a, b)), f'n={n}'
    sizes = (0, 1, 4097, 3)
    A, B = [_ints(rng, n, True) for n in sizes], [_ints(rng, n, True) for n in sizes]
    got = bb.inner_many([bb.as_block(a) for a in A], [bb.as_block(b) for b in B])
    assert got == complex(sum(np.vdot(a, b) for a, b in zip(A, B)))


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('do_dagger', [False, True])
def test_inner_weighted_on_strided_and_flat_views(bb, rng, cplx, do_dagger):
    shapes = ((1, 1), (3, 5), (64, 129), (91, 91))  # 91 x 91 = 8281 elements: two work items
    weights = [0.5, 2.0, 4.0, 1.0]
    A = [_ints(rng, s, cplx) for s in shapes]
    B = [_ints(rng, s if do_dagger else s[::-1], cplx) for s in shapes]
    want = sum(w * (np.vdot(a, b) if do_dagger else np.sum(a * b.T)) for w, a, b in zip(weights, A, B))
    want = complex(want) if cplx else float(want)
    flat_a, flat_b = [bb.as_block(a) for a in A], [bb.as_block(b) for b in B]
    assert bb.inner_weighted_many(flat_a, flat_b, weights, do_dagger) == want
    # a: the left columns of a wider matrix (row stride above the row length); b: the transposed view of its transpose
    wide_a = [bb.get_item(bb.as_block(np.concatenate([a, a + 1], axis=1)), (slice(None), slice(0, a.shape[1]))) for a in A]
    tr_b = [bb.permute_axes(bb.as_block(np.ascontiguousarray(b.T)), [1, 0]) for b in B]
    assert bb.inner_weighted_many(wide_a, tr_b, weights, do_dagger) == want
    if do_dagger:  # the weighted square norm reads one operand
        assert bb.inner_weighted_many(wide_a, None, weights) == float(sum(w * np.vdot(a, a).real for w, a in zip(weights, A)))


def _multi_dot(bb, V, w, cplx, wt=None):
    m, k = len(V), 2 if cplx else 1
    res = bb.ctx.empty(k * m)
    ptrs = (C.c_void_p * m)(*[v.ptr for v in V])
    name = 'cyb_multi_dot' + ('_weighted' if wt is not None else '') + ('_c128' if cplx else '_f64')
    args = [bb.ctx.handle, ptrs, m, C.c_void_p(w.ptr), w.size]
    if wt is not None:
        args.append(C.c_void_p(wt.ptr))
    bb.ctx.sync_stream()
    _lib.check(getattr(bb.lib, name)(*args, C.c_void_p(res.data_ptr())))
    r = bb.ctx.d2h(res, k * m, np.float64)
    return r[0::2] + 1j * r[1::2] if cplx else r


@pytest.mark.parametrize('cplx', [False, True])
def test_multi_dot_at_tile_edges(bb, rng, cplx):
    for n in (1, 255, 256, 257, 1025, 524545):  # 524545: two tiles per workgroup
        for m in ((1,) if n == 524545 else (1, 4, 5, 17)):
            V, w = _ints(rng, (m, n), cplx), _ints(rng, n, cplx)
            d = 2.0 ** rng.integers(-1, 3, size=-(-n // GRANULE))
            Vb, wb = [bb.as_block(v) for v in V], bb.as_block(w)
            assert np.array_equal(_multi_dot(bb, Vb, wb, cplx), V.conj() @ w), f'n={n} m={m}'
            want = V.conj() @ (np.repeat(d, GRANULE)[:n] * w)
            assert np.array_equal(_multi_dot(bb, Vb, wb, cplx, bb.as_block(d)), want), f'weighted n={n} m={m}'
