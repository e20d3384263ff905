"""Device side of to_dense_block / from_dense_block on fusion-tree tensors: the cases of tests/test_tree_dense.py through
HipBlockBackend (same inputs, same criteria), and the two kernels (csrc/tree_dense.hip) at the C-ABI between guard bands
against a numpy model.

Exact data at the C-ABI: integers in [-15, 15] under tree-pair tensors with integer entries in [-2, 2] (+ i [-2, 2]), at most
three terms, at most 36 contracted positions, divisors 2 and 4 -- every product, partial sum and quotient is representable, so
the comparison is ``==`` whatever the summation order or FMA contraction."""
import ctypes as C

import numpy as np
import pytest

import tree_dense_cases as cases
from cyten_amd import _lib
from cyten_amd import fusion_tree as ft
from test_gpu_tree_trace import SENTINEL, Arena, _upload

pytestmark = pytest.mark.gpu

CONFIG_IDS = ['-'.join(map(str, c)) for c in cases.ABELIAN_CONFIGS]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the host tests on the device

@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=CONFIG_IDS)
def test_device_abelian_trees_give_the_dense_tensor_and_come_back_exactly(bb, rng, config, cplx):
    cases.check_abelian(bb, rng, config, cplx)


@pytest.mark.parametrize('cplx_data,cplx_tables', [(False, False), (True, True), (False, True), (True, False)])
def test_device_random_isometric_tables_match_the_restatement_in_both_directions(bb, rng, cplx_data, cplx_tables):
    cases.check_table(bb, rng, cplx_data, cplx_tables)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_device_su2_to_dense_is_a_homomorphism_keeps_the_norm_and_commutes_with_dagger(bb, rng, cplx):
    cases.check_su2_homomorphism(bb, rng, cplx)


def test_device_su2_heisenberg_coupling_has_the_blocks_minus_three_quarters_and_one_quarter(bb):
    cases.check_su2_heisenberg(bb)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_device_su2_three_spins_one_half_with_a_two_tree_forest(bb, rng, cplx):
    cases.check_su2_three_spins(bb, rng, cplx)


def test_device_a_block_that_is_not_symmetric_raises_and_is_projected_with_tol_zero(bb):
    cases.check_projection(bb)


def test_device_an_absent_block_gives_written_zeros_and_discard_false_keeps_zero_blocks(bb, rng):
    cases.check_absent_block_and_discard(bb, rng)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_device_an_empty_domain(bb, rng, cplx):
    cases.check_empty_domain(bb, rng, cplx)


def test_device_seven_legs_raise(bb, rng):
    cases.check_seven_legs_raise(bb, rng)


def test_device_errors(bb, rng):
    cases.check_errors(bb, rng)


# ---------------------------------------------------------------------------------------------------------------------------
# device only

class Counting:
    """proxy of the library that lists the C-ABI calls made through the backend"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('cyb_') or name in ('cyb_last_error', 'cyb_ctx_set_stream'):
            return fn

        def wrapped(*args):
            self._calls.append(name)
            return fn(*args)
        return wrapped


def test_device_to_dense_block_is_one_launch_and_the_projection_of_from_dense_block_another(bb, rng, monkeypatch):
    """one C-ABI call of the backend per direction (the table of tree-pair tensors travels in one host-to-device copy of the
    context before it); the tolerance check and the discard of from_dense_block are reductions of their own"""
    c = cases.table_case(rng, False, True)
    sp = (c['cod'], c['dom'], c['cd'], c['dd'])
    data = cases.to_dev(bb, c['data'])
    calls = []
    monkeypatch.setattr(bb, 'lib', Counting(bb.lib, calls))
    dense = ft.to_dense_block(bb, data, *sp)
    assert calls == ['cyb_tree_to_dense_c128']
    del calls[:]
    ft.from_dense_block(bb, dense, *sp, tol=0.0, discard=False)
    assert calls == ['cyb_tree_from_dense_c128']


def _strides_of(shape, order):
    """element strides of `shape` when the axes are laid out in memory in `order` (last: contiguous)"""
    st, n = [0] * len(shape), 1
    for ax in reversed(order):
        st[ax] = n
        n *= shape[ax]
    return st, n


def _interleave(S, T, L):
    """[k_1.., m_1..] -> [(k_1, m_1), ..] merged per leg"""
    x = np.multiply.outer(S, T).transpose([p for l in range(L) for p in (l, L + l)])
    return x.reshape([S.shape[l] * T.shape[l] for l in range(L)])


def _ints(rng, shape, lim, cplx):
    return rng.integers(-lim, lim + 1, shape).astype(float) + (1j * rng.integers(-lim, lim + 1, shape) if cplx else 0)


def _dense_layout(dims, mults, J, starts, pads):
    """the dense tensor in memory: axes (codomain legs..., domain legs reversed), every axis `starts + d * m + pads` long"""
    L = len(dims)
    shape = [s + d * m + p for s, d, m, p in zip(starts, dims, mults, pads)]
    order = list(range(J)) + list(range(L - 1, J - 1, -1))
    return shape, order, *_strides_of(shape, order)


def run_to_dense(bb, rng, cplx, dims, mults, J, n_terms, starts, pads, shift, block_real=False, s_cplx=None, transposed=False):
    """one region record at the C-ABI: the dense tensor lies between SENTINEL bands, `shift` doubles / elements into its
    arena block (an odd shift: a float64 base that is not 16-byte aligned)"""
    L = len(dims)
    s_cplx = cplx if s_cplx is None else s_cplx
    shape, order, st, size = _dense_layout(dims, mults, J, starts, pads)
    dst_a = Arena(cplx, SENTINEL)
    base = dst_a.block(size + shift) + shift
    dst = dst_a.host()
    H, W = int(np.prod(mults[:J])), int(np.prod(mults[J:]))
    want, val = dst.copy(), 0
    Ss, blocks, tarr = [], [], np.zeros(max(n_terms, 1), dtype=_lib.TREE_TO_DENSE_TERM_DTYPE)
    s_off = 0
    for t in range(n_terms):
        S = _ints(rng, dims, 2, s_cplx)
        r0, c0, bh, bw = t, 2 * t + 1, H + t + 2, W + 2 * t + 3
        B = _ints(rng, (bh, bw), 15, cplx and not block_real)
        val = val + _interleave(S, B[r0:r0 + H, c0:c0 + W].reshape(mults), L)
        dev = bb.as_block(np.ascontiguousarray(B.T) if transposed else B)
        blocks.append(dev)
        tarr[t] = (dev.ptr, r0, c0, 1 if transposed else bw, bh if transposed else 1, s_off, int(cplx and block_real), int(cplx and not s_cplx))
        Ss.append(S.ravel())
        s_off += S.size
    table = bb.as_block(np.concatenate(Ss).astype(np.complex128 if s_cplx else np.float64)) if Ss else None
    offs = base + sum(((starts[l] + np.arange(dims[l] * mults[l])) * st[l]).reshape([-1 if a == l else 1 for a in range(L)]) for l in range(L))
    region = [d * m for d, m in zip(dims, mults)]
    want[np.broadcast_to(offs, region).ravel()] = np.broadcast_to(val, region).ravel()
    touched = np.zeros(len(dst), dtype=bool)
    touched[np.broadcast_to(offs, region).ravel()] = True
    d_dst = _upload(bb, dst)
    oarr = np.zeros(1, dtype=_lib.TREE_TO_DENSE_OUT_DTYPE)
    s_str, r_str, c_str = _strides_of(dims, range(L))[0], _strides_of(mults[:J], range(J))[0], _strides_of(mults[J:], range(L - J))[0]
    ext, sd, ss, sr, sc = [], [], [], [], []
    for l in order:
        ext += [dims[l], mults[l]]
        sd += [mults[l] * st[l], st[l]]
        ss += [s_str[l], 0]
        sr += [0, r_str[l] if l < J else 0]
        sc += [0, c_str[l - J] if l >= J else 0]
    pad = [0] * (12 - 2 * L)
    oarr[0] = (d_dst.data_ptr() + (16 if cplx else 8) * (base + sum(s * x for s, x in zip(starts, st))), 2 * L, 0, tuple(ext + pad), tuple(sd + pad),
               tuple(ss + pad), tuple(sr + pad), tuple(sc + pad), 0, n_terms)
    fn = bb.lib.cyb_tree_to_dense_c128 if cplx else bb.lib.cyb_tree_to_dense_f64
    args = (bb.ctx.handle, oarr.ctypes.data_as(C.POINTER(_lib.TreeToDenseOut)), 1, tarr.ctypes.data_as(C.POINTER(_lib.TreeToDenseTerm)), n_terms,
            C.c_void_p(table.ptr if table is not None else 0))
    bb.ctx.sync_stream()
    _lib.check(fn(*args))
    got = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    assert np.array_equal(got[~touched].view(np.uint64), dst[~touched].view(np.uint64)), 'a guard band or a gap of the dense tensor was written'
    bad = got != want
    assert not bad.any(), f'{int(bad.sum())} of {int(np.prod([d * m for d, m in zip(dims, mults)]))} elements differ'
    _lib.check(fn(*args))
    again = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))                  # bit-identical from run to run
    del blocks


TO_DENSE_CASES = {
    'one-element': dict(dims=(1,), mults=(1,), J=1, n_terms=1, starts=(1,), pads=(1,), shift=0),
    'four-legs-small': dict(dims=(2, 3, 1, 2), mults=(3, 1, 2, 5), J=2, n_terms=3, starts=(1, 0, 2, 1), pads=(0, 2, 1, 1), shift=0),
    'odd-base': dict(dims=(2, 3, 1, 2), mults=(3, 1, 2, 5), J=2, n_terms=2, starts=(0, 1, 0, 0), pads=(1, 0, 0, 2), shift=1),
    'no-terms': dict(dims=(2, 2), mults=(3, 4), J=1, n_terms=0, starts=(1, 1), pads=(1, 1), shift=1),
    'several-items': dict(dims=(3, 2, 2, 3), mults=(40, 1, 1, 41), J=2, n_terms=2, starts=(1, 0, 1, 2), pads=(0, 1, 0, 1), shift=1),   # 59 040 elements
    'six-legs': dict(dims=(2, 1, 2, 1, 3, 2), mults=(2, 3, 1, 2, 2, 3), J=3, n_terms=2, starts=(0, 1, 0, 2, 0, 1), pads=(1, 0, 1, 0, 1, 0), shift=0),
    'codomain-only': dict(dims=(2, 3), mults=(5, 66), J=2, n_terms=2, starts=(0, 0), pads=(0, 0), shift=0),
    'transposed-blocks': dict(dims=(2, 2, 2), mults=(3, 2, 65), J=1, n_terms=2, starts=(0, 0, 1), pads=(0, 0, 0), shift=0, transposed=True),
}


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('name', list(TO_DENSE_CASES))
def test_to_dense_kernel_between_guard_bands(bb, rng, name, cplx):
    run_to_dense(bb, rng, cplx, **TO_DENSE_CASES[name])


@pytest.mark.parametrize('block_real,s_cplx', [(True, True), (False, False), (True, False)])
def test_to_dense_kernel_reads_a_real_operand_beside_a_complex_one_as_it_stands(bb, rng, block_real, s_cplx):
    run_to_dense(bb, rng, True, block_real=block_real, s_cplx=s_cplx, **TO_DENSE_CASES['four-legs-small'])


def run_from_dense(bb, rng, cplx, dims, mults, J, n_terms, starts, pads, at, ld_extra, div, src_real=False, s_cplx=None):
    """one tile record at the C-ABI: the tile lies at row / column `at` of a block between SENTINEL bands, its source is a
    region of a dense tensor with the axes (codomain legs..., domain legs reversed)"""
    L = len(dims)
    s_cplx = cplx if s_cplx is None else s_cplx
    shape, order, st, size = _dense_layout(dims, mults, J, starts, pads)
    H, W = int(np.prod(mults[:J])), int(np.prod(mults[J:]))
    ld = W + at[1] + ld_extra
    dst_a = Arena(cplx, SENTINEL)
    base = dst_a.block((H + at[0] + 1) * ld) + at[0] * ld + at[1]
    dst = dst_a.host()
    want, acc = dst.copy(), 0
    Ss, srcs, tarr = [], [], np.zeros(max(n_terms, 1), dtype=_lib.TREE_FROM_DENSE_TERM_DTYPE)
    s_off = 0
    sl = tuple(slice(s, s + d * m) for s, d, m in zip(starts, dims, mults))
    for t in range(n_terms):
        S = _ints(rng, dims, 2, s_cplx)
        A = _ints(rng, shape, 15, cplx and not src_real)                     # indexed by leg
        mem = np.ascontiguousarray(A.transpose(order))                        # as it lies in memory
        dev = bb.as_block(mem)
        srcs.append(dev)
        reg = A[sl].reshape([x for d, m in zip(dims, mults) for x in (d, m)]).transpose([2 * l for l in range(L)] + [2 * l + 1 for l in range(L)])
        acc = acc + np.tensordot(np.conj(S), reg, L).reshape(H, W)
        tarr[t] = (dev.ptr + (8 if src_real or not cplx else 16) * sum(s * x for s, x in zip(starts, st)), s_off, int(cplx and src_real),
                   int(cplx and not s_cplx))
        Ss.append(S.ravel())
        s_off += S.size
    table = bb.as_block(np.concatenate(Ss).astype(np.complex128 if s_cplx else np.float64)) if Ss else None
    idx = (base + ld * np.arange(H)[:, None] + np.arange(W)[None, :]).ravel()
    want[idx] = (np.zeros((H, W)) + acc / div).ravel()
    d_dst = _upload(bb, dst)
    oarr = np.zeros(1, dtype=_lib.TREE_FROM_DENSE_OUT_DTYPE)
    d_str = [x * ld for x in _strides_of(mults[:J], range(J))[0]] + _strides_of(mults[J:], range(L - J))[0]
    pad = [0] * (6 - L)
    oarr[0] = (d_dst.data_ptr() + (16 if cplx else 8) * base, L, L, tuple([mults[l] for l in order] + pad), tuple([d_str[l] for l in order] + pad),
               tuple([st[l] for l in order] + pad), tuple(list(dims) + pad), tuple([m * s for m, s in zip(mults, st)] + pad), div, 0, n_terms)
    fn = bb.lib.cyb_tree_from_dense_c128 if cplx else bb.lib.cyb_tree_from_dense_f64
    args = (bb.ctx.handle, oarr.ctypes.data_as(C.POINTER(_lib.TreeFromDenseOut)), 1, tarr.ctypes.data_as(C.POINTER(_lib.TreeFromDenseTerm)), n_terms,
            C.c_void_p(table.ptr if table is not None else 0))
    bb.ctx.sync_stream()
    _lib.check(fn(*args))
    got = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    tile = np.zeros(len(dst), dtype=bool)
    tile[idx] = True
    assert np.array_equal(got[~tile].view(np.uint64), dst[~tile].view(np.uint64)), 'a guard band or a gap between tile rows was written'
    bad = got[tile] != want[tile]
    assert not bad.any(), f'{int(bad.sum())} of {H * W} elements differ'
    _lib.check(fn(*args))
    again = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))                  # bit-identical from run to run
    del srcs


FROM_DENSE_CASES = {
    'one-element': dict(dims=(1,), mults=(1,), J=1, n_terms=1, starts=(1,), pads=(1,), at=(1, 1), ld_extra=2, div=2.0),
    'four-legs-small': dict(dims=(2, 3, 1, 2), mults=(3, 1, 2, 5), J=2, n_terms=1, starts=(1, 0, 2, 1), pads=(0, 2, 1, 1), at=(1, 2), ld_extra=3, div=4.0),
    'odd-base': dict(dims=(2, 3, 1, 2), mults=(3, 1, 2, 5), J=2, n_terms=2, starts=(0, 1, 0, 0), pads=(1, 0, 0, 2), at=(2, 1), ld_extra=2, div=2.0),
    'no-terms': dict(dims=(2, 2), mults=(3, 4), J=1, n_terms=0, starts=(1, 1), pads=(1, 1), at=(0, 1), ld_extra=1, div=2.0),
    'several-items': dict(dims=(3, 2, 2, 3), mults=(40, 1, 1, 41), J=2, n_terms=1, starts=(1, 0, 1, 2), pads=(0, 1, 0, 1), at=(1, 1), ld_extra=2, div=4.0),
    'six-legs': dict(dims=(2, 1, 2, 1, 3, 2), mults=(2, 3, 1, 2, 2, 3), J=3, n_terms=1, starts=(0, 1, 0, 2, 0, 1), pads=(1, 0, 1, 0, 1, 0), at=(1, 2), ld_extra=1, div=2.0),
    'codomain-only': dict(dims=(2, 3), mults=(5, 66), J=2, n_terms=1, starts=(0, 0), pads=(0, 0), at=(0, 0), ld_extra=0, div=1.0),
    'wide-tile': dict(dims=(2, 2), mults=(70, 900), J=1, n_terms=1, starts=(0, 3), pads=(1, 0), at=(1, 1), ld_extra=1, div=2.0),                       # 63 000 elements
}


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
@pytest.mark.parametrize('name', list(FROM_DENSE_CASES))
def test_from_dense_kernel_between_guard_bands(bb, rng, name, cplx):
    run_from_dense(bb, rng, cplx, **FROM_DENSE_CASES[name])


@pytest.mark.parametrize('src_real,s_cplx', [(True, True), (False, False), (True, False)])
def test_from_dense_kernel_reads_a_real_operand_beside_a_complex_one_as_it_stands(bb, rng, src_real, s_cplx):
    run_from_dense(bb, rng, True, src_real=src_real, s_cplx=s_cplx, **FROM_DENSE_CASES['four-legs-small'])


def test_kernels_accept_empty_lists(bb):
    for fn in (bb.lib.cyb_tree_to_dense_f64, bb.lib.cyb_tree_to_dense_c128, bb.lib.cyb_tree_from_dense_f64, bb.lib.cyb_tree_from_dense_c128):
        assert fn(bb.ctx.handle, None, 0, None, 0, None) == _lib.CYB_OK


def test_invalid_records_are_refused_before_anything_is_launched(bb):
    """too many levels, a negative extent, a bad term range, a NULL destination, a zero divisor: CYB_ERR_INVALID with a message"""
    o = np.zeros(1, dtype=_lib.TREE_TO_DENSE_OUT_DTYPE)
    t = np.zeros(1, dtype=_lib.TREE_TO_DENSE_TERM_DTYPE)
    po, pt = o.ctypes.data_as(C.POINTER(_lib.TreeToDenseOut)), t.ctypes.data_as(C.POINTER(_lib.TreeToDenseTerm))
    for field, value, frag in (('n_levels', 13, 'levels'), ('n_terms', 2, 'bad term range'), ('n_levels', 0, 'dst is NULL')):
        o[0] = np.zeros(1, dtype=o.dtype)[0]
        o[0][field] = value
        assert bb.lib.cyb_tree_to_dense_f64(bb.ctx.handle, po, 1, pt, 1, None) == _lib.CYB_ERR_INVALID
        assert frag in bb.lib.cyb_last_error().decode()
    o[0] = np.zeros(1, dtype=o.dtype)[0]
    o[0]['n_levels'] = 1
    o[0]['ext'][0] = -1
    assert bb.lib.cyb_tree_to_dense_c128(bb.ctx.handle, po, 1, pt, 1, None) == _lib.CYB_ERR_INVALID
    assert 'negative extent' in bb.lib.cyb_last_error().decode()
    f = np.zeros(1, dtype=_lib.TREE_FROM_DENSE_OUT_DTYPE)
    ftm = np.zeros(1, dtype=_lib.TREE_FROM_DENSE_TERM_DTYPE)
    pf, pft = f.ctypes.data_as(C.POINTER(_lib.TreeFromDenseOut)), ftm.ctypes.data_as(C.POINTER(_lib.TreeFromDenseTerm))
    assert bb.lib.cyb_tree_from_dense_f64(bb.ctx.handle, pf, 1, pft, 1, None) == _lib.CYB_ERR_INVALID
    assert 'divisor' in bb.lib.cyb_last_error().decode()
    f[0]['n_k'] = 7
    assert bb.lib.cyb_tree_from_dense_c128(bb.ctx.handle, pf, 1, pft, 1, None) == _lib.CYB_ERR_INVALID
    assert 'levels' in bb.lib.cyb_last_error().decode()


def test_backend_refuses_bad_regions_and_views(bb, rng):
    blk = lambda *sh, c=False: bb.as_block(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if c else 0))   # noqa: E731
    S = np.ones((2, 1))
    to, frm = bb.tree_to_dense_many, bb.tree_from_dense_many
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
        to(blk(6, 4), [((0, 0), (2, 1), (3, 4), 1, [(bb.as_block(np.ones((3, 4), bool)), 0, 0, S)])])
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
