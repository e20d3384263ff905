"""Device side of from_grid / from_tree_pairs / eye on fusion-tree tensors: the cases of tests/test_tree_grid.py through
HipBlockBackend (same inputs, same criteria), and the window-copy kernel (csrc/tree_place.hip) at the C-ABI.

At the C-ABI every window lies inside a region that is pre-filled with NaNs of distinct payloads; after the call every element
outside the windows must hold the bits it held before.  Sources hold integers in [-15, 15] (and, under the coefficient 1, a
-0.0 and a NaN with a payload, which must arrive bit for bit); coefficients come from {1, -2, 0.5, i, -0.5i, 1 + i}: every
product is representable, so the comparison with the numpy model is ``==`` whatever the contraction."""
import ctypes as C

import numpy as np
import pytest

import tree_grid_cases as cases
from cyten_amd import _lib
from cyten_amd import fusion_tree as ft
from test_gpu_tree_trace import COEFFS, _upload

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the host tests on the device

@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=lambda c: 'x'.join(map(str, c)))
def test_device_grid_of_abelian_trees_is_the_concatenated_dense_tensor(bb, rng, config, kind):
    cases.check_abelian(bb, rng, config, kind)


@pytest.mark.parametrize('kinds', cases.KINDS)
def test_device_forests_of_several_trees_match_the_restatement(bb, rng, kinds):
    cases.check_table(bb, rng, kinds)


@pytest.mark.parametrize('kinds', cases.KINDS)
def test_device_complex_factors_on_real_and_complex_entries(bb, rng, kinds):
    cases.check_table(bb, rng, kinds, cases.COMPLEX_FACTORS)


def test_device_real_factors_on_real_entries_stay_float64(bb, rng):
    have = cases.check_table(bb, rng, 'real', cases.REAL_FACTORS)
    assert all(b.dtype == np.float64 for b in have.values())


@pytest.mark.parametrize('cplx', [False, True])
def test_device_su2_grid_through_to_dense_block(bb, rng, cplx):
    cases.check_su2_grid(bb, rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_su2_direct_sum_adds_the_squared_norms(bb, rng, cplx):
    cases.check_su2_direct_sum(bb, rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_device_compose_with_eye_is_the_identity(bb, rng, cplx):
    cases.check_eye(bb, rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('config', cases.TREE_PAIR_CONFIGS, ids=lambda c: 'x'.join(map(str, c)))
def test_device_tree_pairs_give_the_blocks_they_were_cut_from(bb, rng, config, cplx):
    cases.check_tree_pairs(bb, rng, config, cplx)


def test_device_tree_pairs_missing_tiles_absent_sectors_and_errors(bb, rng):
    cases.check_tree_pairs_structure(bb, rng)


def test_device_zero_blocks_are_discarded_unless_asked_otherwise(bb, rng):
    cases.check_discard(bb, rng)


def test_device_every_error_path_of_from_grid(bb, rng):
    cases.check_errors(bb, rng)


class _Counting:
    """a proxy of the library that lists the C-ABI calls made through it"""

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


def test_device_from_grid_and_from_tree_pairs_are_one_launch_each(bb, rng, monkeypatch):
    _, dev, n_cod, n_dom, left, right = cases.table_case(bb, rng, 'mixed')
    dagger_entry = dev[1][0]
    assert all(b.strides == (1, b.shape[0]) for b in dagger_entry.blocks if min(b.shape) > 1)      # read in place as a transposed view
    cod, dom, _, trees = cases.tree_pairs_case(bb, rng, (2, 2), False)
    calls = []
    monkeypatch.setattr(bb, 'lib', _Counting(bb.lib, calls))
    ft.from_grid(bb, dev, n_cod, n_dom, left, right, factors=cases.COMPLEX_FACTORS, discard=False)
    assert calls == ['cyb_tree_place_c128']
    del calls[:]
    ft.from_tree_pairs(bb, trees, cod, dom)
    assert calls == ['cyb_tree_place_f64']


def test_backend_refuses_bad_views(bb, rng):
    blk = lambda *sh, c=False: bb.as_block(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if c else 0))   # noqa: E731
    dst = blk(4, 2, 3)
    with pytest.raises(ValueError, match='3-D'):
        bb.tree_place_many([(blk(4, 6), blk(4, 6), 1, 1.0)])
    with pytest.raises(ValueError, match='share one dtype'):
        bb.tree_place_many([(dst, None, 0, 1.0), (blk(4, 2, 3, c=True), None, 0, 1.0)])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_place_many([(dst, blk(4, 6, c=True), 1, 1.0)])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_place_many([(dst, blk(4, 6), 1, 1j)])
    with pytest.raises(ValueError, match='stride 1'):
        bb.tree_place_many([(bb.permute_axes(blk(3, 2, 4), [2, 1, 0]), blk(4, 6), 1, 1.0)])
    with pytest.raises(ValueError, match='for a window of'):
        bb.tree_place_many([(dst, blk(6, 4), 1, 1.0)])
    with pytest.raises(ValueError, match='at most 6'):
        bb.tree_place_many([(blk(1, 1, 1), blk(*(1,) * 8), 7, 1.0)])
    bb.tree_place_many([])


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

GUARD = 8
NAN_BITS = 0x7FF8000000000000


def _nan_pattern(n):
    """n float64 NaNs of distinct payloads"""
    return (np.uint64(NAN_BITS) | (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFFFF))).view(np.float64)


def win(h, nq, wn, cp=None, ldd=None, off=0, src=None, n_row=1, coeff=1.0, real=False, special=False):
    """one window, `off` elements into its region; `src`: None (zeros) or ``(parent shape, view of the parent)`` with the first
    `n_row` axes of the view the row levels; `real`: a float64 source under the c128 entry; `special`: -0.0 and a NaN with a payload
    among the source values (coefficient 1 only)"""
    cp = wn if cp is None else cp
    ldd = (max(nq, 1) - 1) * cp + wn + 3 if ldd is None else ldd
    return dict(h=h, nq=nq, wn=wn, cp=cp, ldd=ldd, off=off, src=src, n_row=n_row, coeff=coeff, real=real, special=special)


def mat(h, w, t=False, pad=0):
    """an h x w source: C-contiguous with `pad` spare columns, or the transposed view of a w x h parent"""
    if t:
        return ((w, h + pad), lambda p: p[:, :h].T)
    return ((h, w + pad), lambda p: p[:, :w])


def run_place(bb, rng, wins, cplx, expect=_lib.CYB_OK, mutate=None):
    """lay the windows out, launch ONCE and compare: outside the windows bit for bit with the image before the call, inside
    with the model; then launch again: the same bits.  `mutate(arr)` may spoil the records; with `expect` an error nothing may
    have changed."""
    es = 2 if cplx else 1
    n_dst, lay = GUARD, []
    for w in wins:
        n_dst += n_dst % 2                                                  # regions start 16-byte aligned
        span = w['off'] + max(w['h'] - 1, 0) * w['ldd'] + max(w['nq'] - 1, 0) * w['cp'] + w['wn']
        lay.append(n_dst + w['off'])
        n_dst += span + GUARD
    dst = _nan_pattern(n_dst * es)
    dimg = dst.view(np.complex128) if cplx else dst
    arr = np.zeros(len(wins), dtype=_lib.TREE_PLACE_DTYPE)
    parents, want, inside = [], dimg.copy(), np.zeros(n_dst, dtype=bool)
    for k, (w, base) in enumerate(zip(wins, lay)):
        rec = arr[k]
        rec['h'], rec['nq'], rec['wn'], rec['cp'], rec['ldd'] = w['h'], w['nq'], w['wn'], w['cp'], w['ldd']
        c = complex(w['coeff'])
        rec['coeff_re'], rec['coeff_im'] = c.real, c.imag
        idx = (base + w['ldd'] * np.arange(w['h'])[:, None, None] + w['cp'] * np.arange(w['nq'])[None, :, None] + np.arange(w['wn'])[None, None, :])
        inside[idx.ravel()] = True
        if w['src'] is None:
            parents.append(None)
            want[idx.ravel()] = 0
            continue
        shape, view_of = w['src']
        s_cplx = cplx and not w['real']
        n = int(np.prod(shape))
        p = rng.integers(-15, 16, n).astype(float) + (1j * rng.integers(-15, 16, n) if s_cplx else 0)
        if w['special'] and n >= 2:
            p[0], p[1] = -0.0, np.uint64(NAN_BITS | 0xBEEF).view(np.float64)
        p = p.reshape(shape)
        v = view_of(p)
        parents.append((p, (v.__array_interface__['data'][0] - p.__array_interface__['data'][0]) // p.itemsize))
        rec['n_row_levels'], rec['n_col_levels'] = w['n_row'], v.ndim - w['n_row']
        rec['src_real'] = int(cplx and w['real'])
        for l in range(v.ndim):
            name = ('rext', 'rs', l) if l < w['n_row'] else ('cext', 'cs', l - w['n_row'])
            rec[name[0]][name[2]], rec[name[1]][name[2]] = v.shape[l], v.strides[l] // p.itemsize
        vals = np.ascontiguousarray(v).reshape(w['h'], w['nq'], w['wn'])
        want[idx.ravel()] = (vals if c == 1 else c * vals).ravel() if cplx else (vals if c == 1 else c.real * vals).ravel()
    d_dst = _upload(bb, dimg)
    d_src = [None if p is None else _upload(bb, p[0].ravel() if p[0].size else np.zeros(1, dtype=p[0].dtype)) for p in parents]
    for k, (w, base) in enumerate(zip(wins, lay)):
        arr[k]['dst'] = d_dst.data_ptr() + 8 * es * base
        if parents[k] is not None:
            arr[k]['src'] = d_src[k].data_ptr() + parents[k][0].itemsize * parents[k][1]
    if mutate is not None:
        mutate(arr)
    fn = bb.lib.cyb_tree_place_c128 if cplx else bb.lib.cyb_tree_place_f64
    args = (bb.ctx.handle, arr.ctypes.data_as(C.POINTER(_lib.TreePlaceRec)), len(wins))
    bb.ctx.sync_stream()
    status = fn(*args)
    assert status == expect, bb.lib.cyb_last_error().decode()
    got = bb.ctx.d2h(d_dst, len(dimg), dimg.dtype)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64).reshape(len(a), -1)            # noqa: E731
    if expect != _lib.CYB_OK:
        assert np.array_equal(bits(got), bits(dimg))                                    # nothing was written
        return
    assert np.array_equal(bits(got)[~inside], bits(dimg)[~inside]), 'an element outside the windows was written'
    unit = np.zeros(n_dst, dtype=bool)
    for w, base in zip(wins, lay):
        if w['src'] is not None and complex(w['coeff']) == 1 and not (cplx and w['real']):
            unit[(base + w['ldd'] * np.arange(w['h'])[:, None, None] + w['cp'] * np.arange(w['nq'])[None, :, None]
                  + np.arange(w['wn'])[None, None, :]).ravel()] = True
    assert np.array_equal(bits(got)[unit], bits(want)[unit]), 'the coefficient 1 did not copy the bits'
    rest = inside & ~unit
    assert not np.isnan(got[rest]).any()
    bad = got[rest] != want[rest]
    assert not bad.any(), f'{int(bad.sum())} of {int(rest.sum())} elements differ'
    for d, p in zip(d_src, parents):
        if p is not None and p[0].size:
            back = bb.ctx.d2h(d, p[0].size, p[0].dtype)
            assert np.array_equal(bits(back), bits(p[0].ravel()))
    _lib.check(fn(*args))
    again = bb.ctx.d2h(d_dst, len(dimg), dimg.dtype)
    assert np.array_equal(bits(again), bits(got))                                       # bit-identical from run to run


def _coeff(k, cplx):
    return COEFFS[k % len(COEFFS)] if cplx else COEFFS[k % 3]


def _branch_windows(cplx):
    """the smallest shapes that reach each path of the kernel as built.  float64: a record runs on pairs of doubles iff wn is
    even, cp is even (or nq = 1), ldd is even (or h = 1), dst is 16-byte aligned (regions start aligned: iff `off` is even) and the
    innermost source level has an even extent; the pair of the source is one 16-byte load iff that level has the stride 1, the
    source is 16-byte aligned and every other stride is even; else one double per lane.  complex: one element per lane.  A work
    item is 1024 units (pairs / elements) for a call of this size; one wave per item, four per workgroup; the lane offsets are
    decoded with extents clipped at 64."""
    c = lambda k: _coeff(k, cplx)                                                      # noqa: E731
    return [
        win(1, 1, 1, src=mat(1, 1), special=False),                                                    # a 1 x 1 window
        win(0, 3, 2, src=mat(0, 6)), win(3, 0, 2, src=mat(3, 0)), win(3, 2, 0, src=mat(3, 0)),          # zero extents
        win(3, 2, 4, cp=5, src=None), win(4, 2, 6, cp=8, ldd=20, src=None),                             # zeros; ... in pairs
        win(3, 3, 5, cp=9, ldd=29, off=1, src=mat(3, 15), coeff=c(1)),                                  # odd everything: 8-byte aligned runs
        win(3, 3, 5, cp=9, ldd=29, off=1, src=mat(3, 15, pad=2), special=True),                         # ... bits under the coefficient 1
        win(2, 70, 1, cp=3, src=mat(2, 70, t=True), coeff=c(2)),                                        # wn = 1: lanes across runs and rows
        win(130, 2, 67, cp=70, ldd=141, src=mat(130, 134, pad=1), coeff=c(3)),                          # 18 items: cuts inside rows and runs
        win(64, 2, 66, cp=66, ldd=132, src=mat(64, 132), coeff=c(4)),                                   # pairs, 16-byte loads, 5 items
        win(4, 2, 6, cp=8, ldd=20, src=mat(4, 12), special=True),                                       # pairs, 16-byte loads
        win(4, 2, 6, cp=8, ldd=20, src=mat(4, 12, t=True), coeff=c(5)),                                 # pairs, two loads per pair
        win(4, 2, 6, cp=8, ldd=20, off=1, src=mat(4, 12)),                                              # ... an odd offset: no pairs
        win(4, 2, 6, cp=8, ldd=20, src=mat(4, 12, pad=1), coeff=c(1)),                                  # an odd source row stride: two loads
        win(6, 3, 4, cp=6, ldd=19, src=((3, 2, 2, 2, 3), lambda p: p.transpose(1, 0, 4, 3, 2)), n_row=2, coeff=c(2)),
        #                                   row levels (2, 3) with permuted strides, column levels (3, 2, 2) with reversed strides
        win(5, 1, 7, src=((1, 7), lambda p: np.broadcast_to(p, (5, 7))), coeff=c(3)),                   # a zero stride: one row for all
        win(5, 2, 4, cp=4, src=((5, 8), lambda p: p[::-1, ::-1]), coeff=c(4)),                          # negative strides
        win(4, 2, 6, cp=8, ldd=20, src=((4, 12), lambda p: p[::-1, ::-1])),                             # ... under the conditions of pairs
        win(3, 2, 2, cp=2, src=((12,), lambda p: p.reshape(1, 3, 1, 4)), n_row=2, coeff=c(5)),          # levels of extent 1
        win(1, 1, 1, src=((), lambda p: p), n_row=0, coeff=c(0)),                                       # no levels at all
        win(66, 1, 65, src=mat(66, 65, t=True), coeff=c(1)),                                            # extents just above the wave
    ]


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_paths_between_nan_sentinels(bb, rng, cplx):
    run_place(bb, rng, _branch_windows(cplx), cplx)


def test_kernel_float64_sources_under_the_complex_entry(bb, rng):
    """a float64 source read as it stands beside complex ones, under real, imaginary and complex coefficients"""
    wins = [win(3, 2, 4, cp=5, src=mat(3, 8), real=True, coeff=1 + 1j), win(3, 2, 4, cp=5, src=mat(3, 8, t=True), coeff=-0.5j),
            win(5, 1, 3, src=mat(5, 3, pad=2), real=True, coeff=1.0), win(2, 70, 1, cp=1, src=mat(2, 70), real=True, coeff=1j),
            win(6, 3, 4, cp=6, ldd=19, src=((3, 2, 2, 2, 3), lambda p: p.transpose(1, 0, 4, 3, 2)), n_row=2, real=True, coeff=-2.0)]
    run_place(bb, rng, wins, True)


def test_kernel_empty_list(bb):
    for fn in (bb.lib.cyb_tree_place_f64, bb.lib.cyb_tree_place_c128):
        assert fn(bb.ctx.handle, None, 0) == _lib.CYB_OK


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_invalid_records_are_refused_before_anything_is_launched(bb, rng, cplx):
    """level counts, negative extents, an extent beyond 2^30, level products, cp below wn, ldd below the span, a NULL dst, a complex
    coefficient at the float64 entry: the error comes back, the destination stays as it was, and the context serves the next
    valid call"""
    def wins():
        return [win(2, 2, 3, cp=4, src=mat(2, 6)), win(3, 2, 2, cp=3, src=mat(3, 4, t=True), coeff=-2.0), win(2, 1, 3, src=None)]

    def set_(arr, k, field, value, at=None):
        if at is None:
            arr[k][field] = value
        else:
            arr[k][field][at] = value

    spoil = [
        (lambda a: set_(a, 1, 'n_row_levels', 7), 'at most 6'),
        (lambda a: set_(a, 0, 'n_col_levels', -1), 'at most 6'),
        (lambda a: set_(a, 1, 'h', -1), 'negative extent'),
        (lambda a: set_(a, 0, 'cext', -2, 0), 'negative extent'),
        (lambda a: set_(a, 2, 'wn', 2 ** 30 + 1), 'extent too large'),
        (lambda a: set_(a, 1, 'rext', 2 ** 31, 0), 'extent too large'),
        (lambda a: set_(a, 1, 'rext', 4, 0), 'row levels do not multiply'),
        (lambda a: set_(a, 0, 'cext', 5, 0), 'column levels do not multiply'),
        (lambda a: set_(a, 0, 'cp', 2), 'cp 2 below'),
        (lambda a: set_(a, 1, 'ldd', 4), 'ldd 4 below'),
        (lambda a: set_(a, 2, 'dst', 0), 'dst is NULL'),
    ]
    if not cplx:
        spoil.append((lambda a: set_(a, 1, 'coeff_im', 0.5), 'complex coefficient'))
    for mutate, frag in spoil:
        run_place(bb, rng, wins(), cplx, expect=_lib.CYB_ERR_INVALID, mutate=mutate)
        assert frag in bb.lib.cyb_last_error().decode()
    run_place(bb, rng, wins(), cplx)
