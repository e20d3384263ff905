"""Device side of the factorized tree moves: the cases of tests/test_tree_strip.py through HipBlockBackend (same inputs, same
criteria), the launches of one call counted through a proxy of the library, and the strip kernel (csrc/tree_strip.hip) at the
C-ABI.

At the C-ABI every window lies inside a block between guard bands of SENTINEL, the destination prefilled with it; after the call
every element outside the windows must hold the bits it held before.  Sources hold integers in [-15, 15] (and, under ONE term
with the coefficient 1, a -0.0, which must arrive bit for bit); coefficients come from {1, -2, 0.5, i, -0.5i, 1 + i}: every
product and sum is representable, so the comparison with the numpy model is ``==`` whatever the contraction."""
import ctypes as C

import numpy as np
import pytest

import tree_strip_cases as cases
from cyten_amd import _lib
from test_gpu_tree_trace import COEFFS, SENTINEL, Arena, _c_strides, _upload

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the host tests on the device

@pytest.mark.parametrize('real', [False, True], ids=['complex', 'real'])
@pytest.mark.parametrize('case', cases.STRIP_CASES, ids=[c['name'] for c in cases.STRIP_CASES])
def test_device_golden_strips_reproduce_the_reference_expectation(bb, rng, case, real):
    cases.check_golden(bb, rng, case, real)


@pytest.mark.parametrize('kind', cases.KINDS, ids=lambda k: ('c' if k[0] else 'r') + 'data-' + ('c' if k[1] else 'r') + 'map')
@pytest.mark.parametrize('cod_perm', cases.COD_PERMS, ids=lambda p: ''.join(map(str, p)))
@pytest.mark.parametrize('sides', cases.SIDES)
def test_device_exact_data_equals_the_pair_route_and_the_restatement(bb, rng, sides, cod_perm, kind):
    cases.check_exact(bb, rng, sides, cod_perm, *kind)


@pytest.mark.parametrize('kind', cases.KINDS, ids=lambda k: ('c' if k[0] else 'r') + 'data-' + ('c' if k[1] else 'r') + 'map')
@pytest.mark.parametrize('sides', cases.SIDES)
def test_device_rounded_data_is_within_the_derived_bound_of_the_wide_evaluation(bb, rng, sides, kind):
    cases.check_rounded(bb, rng, sides, cases.COD_PERMS[2], *kind)


def test_device_real_data_stays_float64_and_is_read_in_place_under_a_complex_map(bb, rng):
    cases.check_dtypes(bb, rng)


def test_device_an_identity_side_is_no_launch(bb, rng):
    cases.check_identities(bb, rng)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_device_a_braid_and_its_inverse_give_the_input_back(bb, rng, cplx):
    cases.check_round_trip(bb, rng, cplx)


def test_device_every_error_path(bb, rng):
    cases.check_errors(bb, rng)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
def test_device_chain_operator_step_is_the_direct_call(bb, rng, cplx):
    cases.check_chain_step(bb, rng, cplx)


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


@pytest.mark.parametrize('sides', cases.SIDES)
def test_device_factorized_move_is_at_most_two_launches_and_no_zero_fill(bb, rng, sides, monkeypatch):
    """real data under a complex map, the case that would tempt a promotion pass: one ``cyb_tree_strip_c128`` per side that is
    no identity and nothing else -- no memset, no fill, no ``cyb_lincomb_*``, no copy"""
    c = cases.table_case(rng, sides, cases.COD_PERMS[0], True, False, True)
    r = cases.table_case(rng, sides, cases.COD_PERMS[0], True, False, False)
    dev_c, dev_r = cases.to_dev(bb, c['data']), cases.to_dev(bb, r['data'])
    calls = []
    monkeypatch.setattr(bb, 'lib', _Counting(bb.lib, calls))
    cases.run(bb, c, dev_c)
    assert calls == ['cyb_tree_strip_c128'] * (2 if sides == 'both' else 1)
    del calls[:]
    cases.run(bb, r, dev_r)
    assert calls == ['cyb_tree_strip_f64'] * (2 if sides == 'both' else 1)


def test_backend_refuses_bad_records(bb, rng):
    blk = lambda *sh, c=False: bb.as_block(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if c else 0))   # noqa: E731
    dst, src = blk(6, 5), blk(8, 5)
    with pytest.raises(ValueError, match='2-D'):
        bb.tree_strip_many([(blk(6, 5, 1), 0, 0, 6, (2, 3), (1, 0), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='share one dtype'):
        bb.tree_strip_many([(dst, 0, 0, 6, (6,), (0,), []), (blk(6, 5, c=True), 0, 0, 6, (6,), (0,), [])])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 3), (1, 0), [(blk(8, 5, c=True), 0, 1.0)])])
    with pytest.raises(ValueError, match='complex destination'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 3), (1, 0), [(src, 0, 1j)])])
    with pytest.raises(ValueError, match='leaves axis 0'):
        bb.tree_strip_many([(dst, 0, 1, 7, (2, 3), (1, 0), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='for a strip of 6'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 2), (1, 0), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='for a strip of 6'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 3), (1, 1), [(src, 0, 1.0)])])
    with pytest.raises(ValueError, match='of a source of shape'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 3), (1, 0), [(src, 3, 1.0)])])
    with pytest.raises(ValueError, match='of a source of shape'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 3), (1, 0), [(blk(8, 4), 0, 1.0)])])
    with pytest.raises(ValueError, match='differ in their strides'):
        bb.tree_strip_many([(dst, 0, 0, 6, (2, 3), (1, 0), [(src, 0, 1.0), (bb.permute_axes(blk(5, 8), [1, 0]), 0, 1.0)])])
    with pytest.raises(ValueError, match='at most 6'):
        bb.tree_strip_many([(blk(1, 1), 0, 0, 1, (1,) * 7, tuple(range(7)), [])])
    with pytest.raises(ValueError, match='side is'):
        bb.tree_strip_many([(dst, 2, 0, 6, (6,), (0,), [])])
    bb.tree_strip_many([])
    # a transposed (dagger) source is read in place; a strip without a term becomes zeros
    big = bb.as_block(np.full((7, 5), SENTINEL))
    t = rng.integers(-15, 16, (5, 8)).astype(float)
    bb.tree_strip_many([(big, 0, 0, 6, (2, 3), (1, 0), [(bb.permute_axes(bb.as_block(t), [1, 0]), 1, -2.0)]), (big, 0, 6, 7, (1,), (0,), [])])
    want = np.zeros((7, 5))
    want[:6] = -2.0 * t.T[1:7].reshape(2, 3, 5).transpose(1, 0, 2).reshape(6, 5)
    assert np.array_equal(bb.to_numpy(big), want)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel at the C-ABI

def window(h, nq, wn, rext, rs, cext, cs, terms, span, cp=None, ldd=None, off=0, special=False):
    """one output: the window (h, nq, wn, cp, ldd) `off` elements into its block, the source levels, and its terms
    ``(coeff, real, base)`` -- every term reads a parent of its own of `span` elements beyond its base; `real`: a float64 source
    under the c128 entry; `special`: a -0.0 among the source values"""
    cp = wn if cp is None else cp
    ldd = (max(nq, 1) - 1) * cp + wn + 3 if ldd is None else ldd
    return dict(h=h, nq=nq, wn=wn, cp=cp, ldd=ldd, off=off, rext=tuple(rext), rs=tuple(rs), cext=tuple(cext), cs=tuple(cs),
                terms=[(complex(c), bool(real), int(base)) for c, real, base in terms], span=int(span), special=special)


def row_strip(dims, axes, width, coeffs, ldd=None, off=0, pad=1, real=(), special=False):
    """the strip of a codomain pass: prod(dims) rows under the permutation `axes`, `width` columns; term t reads the rows from
    t % 3 on of an old block of prod(dims) + 2 rows with the leading dimension width + pad"""
    n, lds = int(np.prod(dims)), width + pad
    old = _c_strides(dims)
    return window(n, 1, width, [dims[a] for a in axes], [old[a] * lds for a in axes], [width], [1],
                  [(c, t in real, (t % 3) * lds) for t, c in enumerate(coeffs)], (n + 2) * lds, ldd=ldd, off=off, special=special)


def col_strip(dims, axes, height, coeffs, ldd=None, off=0, pad=1, real=(), special=False):
    """the strip of a domain pass: prod(dims) columns under the permutation `axes`, `height` rows; term t reads the columns from
    t % 3 on of an old block of prod(dims) + 2 + pad columns"""
    n = int(np.prod(dims))
    lds = n + 2 + pad
    old = _c_strides(dims)
    return window(height, 1, n, [height], [lds], [dims[a] for a in axes], [old[a] for a in axes],
                  [(c, t in real, t % 3) for t, c in enumerate(coeffs)], height * lds, ldd=ldd, off=off, special=special)


def run_strip(bb, rng, wins, cplx, expect=_lib.CYB_OK, mutate=None):
    """lay the windows out, launch ONCE and compare: outside the windows bit for bit with the image before the call, inside with
    the model (``==``; bits under one term with the coefficient 1); then launch again: the same bits.  `mutate(oarr, tarr)` may
    spoil the records; with `expect` an error nothing may have changed."""
    dst_a, src_c, src_r = Arena(cplx, SENTINEL), Arena(True, complex(np.nan, np.nan)), Arena(False, np.nan)
    nl = _lib.CYB_TREE_PLACE_MAX_LEVELS
    oarr = np.zeros(max(len(wins), 1), dtype=_lib.TREE_STRIP_OUT_DTYPE)
    n_terms = sum(len(w['terms']) for w in wins)
    tarr = np.zeros(max(n_terms, 1), dtype=_lib.TREE_STRIP_TERM_DTYPE)
    lay, t = [], 0
    for k, w in enumerate(wins):
        span = w['off'] + max(w['h'] - 1, 0) * w['ldd'] + max(w['nq'] - 1, 0) * w['cp'] + w['wn']
        base = dst_a.block(span) + w['off']
        rec = oarr[k]
        rec['h'], rec['nq'], rec['wn'], rec['cp'], rec['ldd'] = w['h'], w['nq'], w['wn'], w['cp'], w['ldd']
        rec['n_row_levels'], rec['n_col_levels'], rec['first_term'], rec['n_terms'] = len(w['rext']), len(w['cext']), t, len(w['terms'])
        rec['rext'][:len(w['rext'])], rec['rs'][:len(w['rs'])] = w['rext'], w['rs']
        rec['cext'][:len(w['cext'])], rec['cs'][:len(w['cs'])] = w['cext'], w['cs']
        assert max(len(w['rext']), len(w['cext'])) <= nl
        tl = []
        for c, real, tb in w['terms']:
            arena = src_c if cplx and not real else src_r
            soff = arena.block(w['span'] + tb)                               # (16-byte aligned: the term's base decides about its pairs)
            tarr[t]['coeff_re'], tarr[t]['coeff_im'], tarr[t]['src_real'], tarr[t]['base'] = c.real, c.imag, int(cplx and real), tb
            tl.append((arena, soff, c, tb))
            t += 1
        lay.append((base, tl))
    dst, simg_c, simg_r = dst_a.host(), src_c.host(), src_r.host()
    for w, (_, tl) in zip(wins, lay):
        for arena, soff, _, tb in tl:
            n = w['span'] + tb
            v = rng.integers(-15, 16, n).astype(float) + (1j * rng.integers(-15, 16, n) if arena is src_c else 0)
            if w['special']:
                v[tb] = -0.0
            (simg_c if arena is src_c else simg_r)[soff:soff + n] = v
    d_dst, d_c, d_r = _upload(bb, dst), _upload(bb, simg_c), _upload(bb, simg_r)
    es = 16 if cplx else 8
    t = 0
    for k, (base, tl) in enumerate(lay):
        oarr[k]['dst'] = d_dst.data_ptr() + es * base
        for arena, soff, _, _ in tl:
            tarr[t]['src'] = (d_c.data_ptr() + 16 * soff) if arena is src_c else (d_r.data_ptr() + 8 * soff)
            t += 1
    # the model
    want, inside, unit = dst.copy(), np.zeros(len(dst), dtype=bool), np.zeros(len(dst), dtype=bool)
    for w, (base, tl) in zip(wins, lay):
        if w['h'] * w['nq'] * w['wn'] == 0:
            continue
        at = (base + w['ldd'] * np.arange(w['h'])[:, None, None] + w['cp'] * np.arange(w['nq'])[None, :, None] + np.arange(w['wn'])[None, None, :]).ravel()
        inside[at] = True
        acc = None
        if tl:
            ext, st = w['rext'] + w['cext'], w['rs'] + w['cs']
            offs = (np.asarray(st, dtype=np.int64) @ np.indices(ext).reshape(len(ext), -1)) if ext else np.zeros(1, dtype=np.int64)
            assert len(offs) == len(at) and offs.min() >= 0 and offs.max() < w['span']        # the model never leaves a parent
        for arena, soff, c, tb in tl:
            vals = (simg_c if arena is src_c else simg_r)[soff + tb + offs]
            v = vals if c == 1 else (c if cplx else c.real) * vals
            acc = v if acc is None else acc + v
        assert acc is None or not np.isnan(acc).any()
        want[at] = 0 if acc is None else acc
        if len(tl) == 1 and tl[0][2] == 1 and (not cplx or tl[0][0] is src_c):
            unit[at] = True
    if mutate is not None:
        mutate(oarr, tarr)
    fn = bb.lib.cyb_tree_strip_c128 if cplx else bb.lib.cyb_tree_strip_f64
    args = (bb.ctx.handle, oarr.ctypes.data_as(C.POINTER(_lib.TreeStripOut)), len(wins), tarr.ctypes.data_as(C.POINTER(_lib.TreeStripTerm)), n_terms)
    bb.ctx.sync_stream()
    status = fn(*args)
    assert status == expect, bb.lib.cyb_last_error().decode()
    got = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64).reshape(len(a), -1)            # noqa: E731
    if expect != _lib.CYB_OK:
        assert np.array_equal(bits(got), bits(dst))                                         # nothing was written
        return
    assert np.array_equal(bits(got)[~inside], bits(dst)[~inside]), 'a guard band or a gap between the runs of a window was written'
    assert np.array_equal(bits(got)[unit], bits(want)[unit]), 'one term with the coefficient 1 did not copy the bits'
    assert not np.isnan(got[inside]).any()
    bad = got[inside] != want[inside]
    assert not bad.any(), f'{int(bad.sum())} of {int(inside.sum())} elements differ'
    for d_s, img in ((d_c, simg_c), (d_r, simg_r)):
        back = bb.ctx.d2h(d_s, len(img), img.dtype)
        assert np.array_equal(bits(back), bits(img))
    _lib.check(fn(*args))
    again = bb.ctx.d2h(d_dst, len(dst), dst.dtype)
    assert np.array_equal(bits(again), bits(got))                                           # bit-identical from run to run


def _c(k, cplx, n=1):
    """n coefficients from the exact set, starting at k"""
    pool = COEFFS if cplx else COEFFS[:3]
    return [pool[(k + i) % len(pool)] for i in range(n)]


def _path_windows(cplx):
    """the smallest shapes that reach each path of the kernel as built.  float64: a record runs on pairs of doubles iff wn is
    even, ldd is even (or h = 1), dst is 16-byte aligned (blocks start aligned: iff `off` is even) and the innermost merged source
    level has an even extent; the pair of a source is one 16-byte load iff that level has the stride 1, every other stride is
    even and every term's first element is 16-byte aligned; else one double per lane.  complex: one element per lane.  A work
    item is 1024 units for a call of this size, one wave per item; the lane offsets are decoded with extents clipped at 64."""
    c = lambda k, n=1: _c(k, cplx, n)                                                      # noqa: E731
    wins = []
    for width in (1, 2, 3, 64, 65, 130):                                # strip widths; ldd odd (default: width + 3 is odd for even widths) and even
        wins.append(row_strip((2, 3), (1, 0), width, c(width, 2), ldd=width + 3))
        wins.append(row_strip((2, 3), (1, 0), width, c(width + 1, 2), ldd=width + 4, pad=2 if width % 2 == 0 else 1))
    wins += [
        row_strip((2, 3), (1, 0), 64, c(1, 2), ldd=66, off=1, pad=2),                      # dst 8-byte aligned only: 8-byte stores
        row_strip((2, 1, 3), (2, 1, 0), 4, c(2, 2), ldd=4, pad=0),                         # the unit level is dropped
        row_strip((2, 3, 4), (1, 2, 0), 6, c(3, 3), ldd=8, pad=2),                         # cyclic: levels 3 and 4 stay adjacent and merge
        row_strip((2, 3, 4), (2, 0, 1), 5, c(4, 2)),                                       # the other cyclic one: 2 and 3 merge
        row_strip((2, 3, 4), (0, 1, 2), 6, c(5, 1), ldd=6, pad=0),                         # the identity on a contiguous block: ONE level
        col_strip((3, 4), (0, 1), 5, c(0, 2), ldd=16, pad=0),                              # column pass, innermost kept, even extent: pairs
        col_strip((4, 3), (0, 1), 5, c(1, 2), ldd=16, pad=1),                              # ... odd extent
        col_strip((2, 3, 4), (1, 0, 2), 7, c(2, 3), ldd=26, pad=0),                        # ... kept under a swap of the outer two, three terms
        col_strip((3, 4), (1, 0), 5, c(3, 2), ldd=16, pad=0),                              # innermost moved: gathered loads
        col_strip((2, 3, 4), (2, 0, 1), 6, c(4, 3), ldd=24),                               # ... cyclic
        row_strip((2, 3), (1, 0), 4, [], ldd=6), col_strip((2, 2), (1, 0), 3, [], ldd=7, off=1),      # no terms: zeros
        row_strip((2, 3), (1, 0), 4, [1.0], ldd=4, pad=0, special=True),                   # one term, c = 1: bits, pairs
        col_strip((3, 3), (1, 0), 4, [1.0], special=True),                                 # ... one element per lane
        row_strip((3, 2), (1, 0), 3, c(0, 3)),                                             # three terms
        row_strip((1,), (0,), 1, c(1, 1)), row_strip((1,), (0,), 1, []),                   # 1 x 1 records ...
        row_strip((8, 12), (1, 0), 700, c(2, 2), ldd=700, pad=0),                          # ... beside 96 x 700: 33 items (66 complex), cuts inside a level
        row_strip((1,), (0,), 1, c(3, 2)),
        window(3, 2, 4, [3], [10], [2, 4], [5, 1], [(x, False, 2) for x in c(4, 2)], 32, cp=6, ldd=15),   # two runs per row
        window(0, 1, 4, [0], [4], [4], [1], [(1.0, False, 0)], 8), window(4, 1, 0, [4], [1], [0], [1], [], 8),   # zero extents
    ]
    return wins


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_kernel_paths_between_sentinel_bands(bb, rng, cplx):
    run_strip(bb, rng, _path_windows(cplx), cplx)


def test_kernel_float64_sources_under_the_complex_entry(bb, rng):
    """float64 sources read as they stand beside complex ones in ONE record, under real, imaginary and complex coefficients"""
    wins = [row_strip((2, 3), (1, 0), 5, [1 + 1j, -0.5j, 1.0], real=(0, 2)), col_strip((3, 4), (1, 0), 5, [1j, -2.0], real=(0, 1)),
            row_strip((2, 2), (1, 0), 64, [1.0], real=(0,), ldd=64, pad=0), col_strip((2, 3, 4), (1, 0, 2), 3, [0.5, 1j, 1.0], real=(1,))]
    run_strip(bb, rng, wins, True)


def test_kernel_empty_lists(bb):
    for fn in (bb.lib.cyb_tree_strip_f64, bb.lib.cyb_tree_strip_c128):
        assert fn(bb.ctx.handle, None, 0, None, 0) == _lib.CYB_OK


@pytest.mark.parametrize('cplx', [False, True], ids=['f64', 'c128'])
def test_invalid_records_are_refused_before_anything_is_launched(bb, rng, cplx):
    """a bad term range, a NULL dst of a non-empty record, a complex coefficient at the float64 entry, too many levels, and the
    window checks: the error comes back, the destination stays as it was, and the context serves the next valid call"""
    def wins():
        return [row_strip((2, 3), (1, 0), 4, _c(0, cplx, 2)), col_strip((3, 2), (1, 0), 3, _c(1, cplx, 1)), row_strip((2, 2), (1, 0), 3, [])]

    def set_(field, k, value, at=None, terms=False):
        def mutate(oarr, tarr):
            a = tarr if terms else oarr
            if at is None:
                a[k][field] = value
            else:
                a[k][field][at] = value
        return mutate

    spoil = [
        (set_('first_term', 1, 3), 'bad term range'),
        (set_('n_terms', 0, 4), 'bad term range'),
        (set_('first_term', 2, -1), 'bad term range'),
        (set_('dst', 1, 0), 'dst is NULL'),
        (set_('dst', 2, 0), 'dst is NULL'),
        (set_('src', 0, 0, terms=True), 'src is NULL'),
        (set_('n_row_levels', 0, 7), 'at most 6'),
        (set_('n_col_levels', 1, -1), 'at most 6'),
        (set_('h', 0, -1), 'negative extent'),
        (set_('cext', 1, 2 ** 31, 0), 'extent too large'),
        (set_('rext', 0, 5, 0), 'row levels do not multiply'),
        (set_('cext', 1, 5, 0), 'column levels do not multiply'),
        (set_('ldd', 0, 3), 'ldd 3 below'),
    ]
    if not cplx:
        spoil.append((set_('coeff_im', 2, 0.5, terms=True), 'complex coefficient'))
    for mutate, frag in spoil:
        run_strip(bb, rng, wins(), cplx, expect=_lib.CYB_ERR_INVALID, mutate=mutate)
        assert frag in bb.lib.cyb_last_error().decode()
    run_strip(bb, rng, wins(), cplx)
