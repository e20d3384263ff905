"""combine_legs / split_legs of cyten_amd.abelian on the device and the placement plans behind them (csrc/place_plan.hip),
through the C-ABI.  Everything here is data movement: every comparison is BIT-EXACT, against the numpy stand-in's result
(tests/numpy_tensor_backend.py, the generic zeros_many + copy_many route) for tensors and against numpy indexing for plans
whose records are built by hand.  The error cases are argument checks on the host; nothing provokes a device fault, and the
hand-built records are checked against the sizes of their buffers before they are handed over."""
import collections

import numpy as np
import pytest

from cyten_amd import _lib
from cyten_amd import abelian as ab
from cyten_amd import workloads as wl
from leg_pipe_cases import CASE_IDS, cases, covered
from numpy_tensor_backend import NumpyTensorBackend

pytestmark = pytest.mark.gpu

CASES = cases()
ALL_CASES = pytest.mark.parametrize('case', range(len(CASES)), ids=CASE_IDS)
NP = NumpyTensorBackend()


class _CountingLib:
    """proxy of the loaded library that counts the C-ABI calls by name (cyten_amd/replay.py records them the same way)"""

    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


@pytest.fixture
def counted(bb, monkeypatch):
    lib = _CountingLib(bb.lib)
    monkeypatch.setattr(bb, 'lib', lib)
    return lib


def _identical(bb, got: ab.AbelianTensor, want: ab.AbelianTensor):
    """the device tensor against the stand-in's: legs, table, num_codomain, blocks bit for bit"""
    assert len(got.legs) == len(want.legs)
    for x, y in zip(got.legs, want.legs):
        assert x.sign == y.sign and np.array_equal(x.sectors, y.sectors) and np.array_equal(x.mults, y.mults)
        assert isinstance(x, ab.LegPipe) == isinstance(y, ab.LegPipe)
        if isinstance(x, ab.LegPipe):
            assert x.cstyle == y.cstyle and np.array_equal(x.block_ind_map, y.block_ind_map)
    assert got.num_codomain == want.num_codomain
    assert np.array_equal(got.block_inds, want.block_inds)
    for x, y in zip(got.blocks, want.blocks):
        z = bb.to_numpy(x)
        assert z.shape == y.shape and z.dtype == y.dtype and np.array_equal(z, y)


def _both(bb, case, permuted=False):
    """(device tensor, stand-in tensor) of a case after its preliminary combination; `permuted`: both as the strided views
    permute_legs leaves (legs reversed), with the groups renamed accordingly"""
    spec = case['tensor']
    td, tn = ab.AbelianTensor.from_spec(bb, spec), ab.AbelianTensor.from_spec(NP, spec)
    if case['pre'] is not None:
        g, s, c = case['pre']
        td, tn = ab.combine_legs(bb, td, g, signs=s, cstyle=c), ab.combine_legs(NP, tn, g, signs=s, cstyle=c)
    groups = case['groups']
    if permuted:
        n = td.nlegs
        rev = list(range(n - 1, -1, -1))
        td, tn = ab.permute_legs(bb, td, rev), ab.permute_legs(NP, tn, rev)
        groups = [[n - 1 - i for i in g] for g in groups]
    return td, tn, groups


@pytest.mark.parametrize('permuted', [False, True], ids=['contiguous', 'permuted'])
@ALL_CASES
def test_combine_split_bit_exact(bb, case, permuted):
    """combine (f64, c128, both styles, nested, strided sources), split as views, split contiguous, round trip"""
    c = CASES[case]
    td, tn, groups = _both(bb, c, permuted)
    got = ab.combine_legs(bb, td, groups, signs=c['signs'], cstyle=c['cstyle'])
    want = ab.combine_legs(NP, tn, groups, signs=c['signs'], cstyle=c['cstyle'])
    _identical(bb, got, want)
    assert all(b.is_contiguous() for b in got.blocks)
    want_split = ab.split_legs(NP, want)
    _identical(bb, ab.split_legs(bb, got), want_split)
    packed = ab.split_legs(bb, got, contiguous=True)
    _identical(bb, packed, want_split)
    assert all(b.is_contiguous() for b in packed.blocks)
    # round trip: every block of the tensor comes back bit for bit
    first, grouped, order = {g[0]: g for g in groups}, {j for g in groups for j in g}, []
    for i in range(td.nlegs):
        order += first[i] if i in first else [] if i in grouped else [i]
    if c['pre'] is None:
        back = {tuple(r): b for r, b in zip(packed.block_inds.tolist(), packed.blocks)}
        src = ab.permute_legs(NP, tn, order)
        for row, blk in zip(src.block_inds.tolist(), src.blocks):
            assert np.array_equal(bb.to_numpy(back[tuple(row)]), blk)


def _call_counts(counted):
    return {k: v for k, v in counted.calls.items() if k != 'cyb_last_error'}


def test_call_counts(bb, counted):
    c = CASES[CASE_IDS.index('u1-r5-nonadjacent')]
    spec = c['tensor']
    for drop in range(len(spec.blocks)):     # (an allowed block is absent, so that the old blocks do not cover the result)
        keep = [i for i in range(len(spec.blocks)) if i != drop]
        holey = wl.TensorSpec(spec.moduli, spec.legs, spec.block_inds[keep], [spec.blocks[i] for i in keep], spec.num_codomain)
        if not covered(holey, c['groups']):
            break
    else:
        pytest.fail('the case must leave part of the result uncovered')
    t1, t2 = ab.AbelianTensor.from_spec(bb, holey), ab.AbelianTensor.from_spec(bb, holey)
    ref1 = ab.combine_legs(NP, ab.AbelianTensor.from_spec(NP, holey), c['groups'])
    ab._COMBINE_CACHE.clear()
    ab._SPLIT_CACHE.clear()
    counted.calls.clear()
    first = ab.combine_legs(bb, t1, c['groups'])
    assert _call_counts(counted) == {'cyb_place_plan_create': 1, 'cyb_memset': 1, 'cyb_place_plan_enqueue': 1}
    counted.calls.clear()
    second = ab.combine_legs(bb, t2, c['groups'])
    assert _call_counts(counted) == {'cyb_memset': 1, 'cyb_place_plan_enqueue': 1}
    counted.calls.clear()
    views = ab.split_legs(bb, first)
    assert _call_counts(counted) == {}
    packed = ab.split_legs(bb, second, contiguous=True)
    assert _call_counts(counted) == {'cyb_place_plan_create': 1, 'cyb_place_plan_enqueue': 1}
    counted.calls.clear()
    ab.split_legs(bb, first, contiguous=True)
    assert _call_counts(counted) == {'cyb_place_plan_enqueue': 1}
    _identical(bb, first, ref1)
    _identical(bb, second, ref1)
    _identical(bb, views, ab.split_legs(NP, ref1))
    _identical(bb, packed, ab.split_legs(NP, ref1))
    # a combination whose old blocks cover the result issues no memset
    full = ab.AbelianTensor.from_spec(bb, spec)
    ref_full = ab.combine_legs(NP, ab.AbelianTensor.from_spec(NP, spec), c['groups'])
    assert covered(spec, c['groups'])
    counted.calls.clear()
    got = ab.combine_legs(bb, full, c['groups'])
    assert _call_counts(counted) == {'cyb_place_plan_create': 1, 'cyb_place_plan_enqueue': 1}
    _identical(bb, got, ref_full)


# --------------------------------------------------------------------------------------------- the plan alone

def _rec(src_block, dst_block, shape, src_strides, dst_strides, src_offset=0, dst_offset=0):
    return dict(src_block=src_block, dst_block=dst_block, shape=tuple(shape), src_strides=tuple(src_strides),
                dst_strides=tuple(dst_strides), src_offset=src_offset, dst_offset=dst_offset)


def _span(rec, side):
    """one past the last element a record touches on `side`"""
    if int(np.prod(rec['shape'])) == 0:
        return 0
    assert all(s >= 0 for s in rec[side + '_strides'])
    return rec[side + '_offset'] + sum((n - 1) * s for n, s in zip(rec['shape'], rec[side + '_strides'])) + 1


def _view(flat, rec, side):
    item = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat[rec[side + '_offset']:], rec['shape'], [s * item for s in rec[side + '_strides']])


def _run_plan(bb, recs, src_sizes, dst_sizes, dtype=np.float64, seed=0, check_reverse=True):
    """Build the plan of `recs`, run it forward on random sources and sentinel destinations and compare with numpy indexing;
    then run it in reverse into fresh sources and expect the elements the records name back, bit for bit."""
    rng = np.random.default_rng(seed)
    esz = np.dtype(dtype).itemsize
    for r in recs:      # bounds first: nothing out of range ever reaches the device
        assert 0 <= r['src_block'] < len(src_sizes) and 0 <= r['dst_block'] < len(dst_sizes)
        assert _span(r, 'src') <= src_sizes[r['src_block']] and _span(r, 'dst') <= dst_sizes[r['dst_block']]
    srcs = [rng.standard_normal(n).astype(dtype) + (1j * rng.standard_normal(n) if esz == 16 else 0) for n in src_sizes]
    srcs = [s.astype(dtype) for s in srcs]
    dsts = [np.full(n, -7.0, dtype=dtype) for n in dst_sizes]
    arr = np.zeros(len(recs), dtype=_lib.PLACE_DTYPE)
    for a, r in zip(arr, recs):
        nd = len(r['shape'])
        a['src_block'], a['dst_block'], a['ndim'] = r['src_block'], r['dst_block'], nd
        a['src_offset'], a['dst_offset'] = r['src_offset'], r['dst_offset']
        a['shape'][:nd], a['src_strides'][:nd], a['dst_strides'][:nd] = r['shape'], r['src_strides'], r['dst_strides']
    plan = bb.place_plan(arr, len(srcs), len(dsts), esz)
    d_src = [bb.block_from_numpy(s) for s in srcs]
    d_dst = [bb.block_from_numpy(d) for d in dsts]
    bb.place_enqueue(plan, [b.ptr for b in d_src], [b.ptr for b in d_dst])
    want = [d.copy() for d in dsts]
    for r in recs:
        if int(np.prod(r['shape'])):
            _view(want[r['dst_block']], r, 'dst')[...] = _view(srcs[r['src_block']], r, 'src')
    got = [bb.to_numpy(b) for b in d_dst]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if check_reverse:
        blank = [np.full(n, -3.0, dtype=dtype) for n in src_sizes]
        d_back = [bb.block_from_numpy(s) for s in blank]
        bb.place_enqueue(plan, [b.ptr for b in d_back], [b.ptr for b in d_dst], reverse=True)
        bb.place_enqueue(plan, [b.ptr for b in d_back], [b.ptr for b in d_dst], reverse=True)   # (the built direction is reused)
        want_back = [s.copy() for s in blank]
        for r in recs:
            if int(np.prod(r['shape'])):
                _view(want_back[r['src_block']], r, 'src')[...] = _view(srcs[r['src_block']], r, 'src')
        for b, w in zip(d_back, want_back):
            assert np.array_equal(bb.to_numpy(b), w)
    bb.synchronize()
    return got


def _c_strides(shape):
    out, acc = [], 1
    for n in reversed(shape):
        out.append(acc)
        acc *= n
    return out[::-1]


DTYPES = pytest.mark.parametrize('dtype', [np.float64, np.complex128], ids=['f64', 'c128'])


@DTYPES
def test_plan_rank_1_to_8(bb, dtype):
    """one record per rank in ONE plan, each read through permuted strides"""
    rng = np.random.default_rng(1)
    recs, src_sizes, dst_sizes = [], [], []
    for nd in range(1, 9):
        shape = [int(x) for x in rng.integers(2, 4, nd)]
        shape[-1] = 17 if nd % 2 else 3
        perm = rng.permutation(nd)
        pshape = [shape[p] for p in perm]
        pst = _c_strides(pshape)
        src_strides = [0] * nd
        for k, p in enumerate(perm):
            src_strides[p] = pst[k]
        n = int(np.prod(shape))
        recs.append(_rec(len(recs), len(recs), shape, src_strides, _c_strides(shape)))
        src_sizes.append(n)
        dst_sizes.append(n)
    _run_plan(bb, recs, src_sizes, dst_sizes, dtype)


@DTYPES
def test_plan_transposing_beside_row_run(bb, dtype):
    """a transposed 40 x 48 record (LDS tiles), a record whose short unit-stride destination axis is flattened with its
    neighbour into one tiled axis, two row-run records and one with a short inner axis (decoded per element), in one plan"""
    recs = [_rec(0, 0, (40, 48), (1, 40), (48, 1)),
            _rec(1, 1, (10, 100), (100, 1), (100, 1)),
            _rec(2, 0, (6, 33), (40, 1), (33, 1), src_offset=3, dst_offset=40 * 48),
            _rec(3, 2, (3, 70, 5), (5, 15, 1), (350, 5, 1)),
            _rec(4, 3, (40, 20, 5), (1, 200, 40), (100, 5, 1))]
    _run_plan(bb, recs, [40 * 48, 1000, 300, 3 * 70 * 5, 4000], [40 * 48 + 6 * 33, 1000, 3 * 70 * 5, 4000], dtype)


def test_plan_extents_0_and_1(bb):
    recs = [_rec(0, 0, (0, 5), (5, 1), (5, 1)), _rec(0, 0, (1, 1, 1), (7, 3, 1), (1, 1, 1), src_offset=2, dst_offset=1),
            _rec(1, 1, (1, 20), (99, 1), (55, 1)), _rec(1, 0, (), (), (), src_offset=4, dst_offset=9), _rec(1, 1, (3, 0, 2), (2, 2, 1), (2, 2, 1))]
    _run_plan(bb, recs, [10, 20], [10, 20])
    # a plan of nothing is valid and launches nothing
    plan = bb.place_plan(np.zeros(0, dtype=_lib.PLACE_DTYPE), 0, 0, 8)
    bb.place_enqueue(plan, [], [])


@pytest.mark.parametrize('inner', [15, 16, 17, 2047, 2048])
def test_plan_row_lengths_at_the_path_thresholds(bb, inner):
    """rows one either side of the 16-element row-run threshold and of the 2048-element shared-row threshold, the rows apart
    in the source (so that they do not merge into one run)"""
    rows = 5
    recs = [_rec(0, 0, (rows, inner), (inner + 3, 1), (inner, 1))]
    _run_plan(bb, recs, [rows * (inner + 3)], [rows * inner])


@pytest.mark.parametrize('so, do', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_plan_alignment(bb, so, do):
    """source and destination 16-byte aligned or not, the same way and differently (8-byte elements)"""
    recs = [_rec(0, 0, (7, 33), (35, 1), (33, 1), src_offset=so, dst_offset=do), _rec(1, 1, (40, 48), (1, 41), (49, 1), src_offset=so, dst_offset=do)]
    _run_plan(bb, recs, [7 * 35 + 1, 41 * 48 + 1], [7 * 33 + 1, 40 * 49 + 1])


def test_plan_300_records_into_3_destinations(bb):
    recs = [_rec(k, k % 3, (4, 20), (20, 1), (20, 1), dst_offset=80 * (k // 3)) for k in range(300)]
    _run_plan(bb, recs, [80] * 300, [8000] * 3)


def test_plan_one_4096_square_record(bb):
    n = 4096
    _run_plan(bb, [_rec(0, 0, (n, n), (1, n), (n, 1))], [n * n], [n * n], check_reverse=False)
    _run_plan(bb, [_rec(0, 0, (n, n), (n, 1), (n, 1))], [n * n], [n * n], check_reverse=False)


def test_plan_errors(bb):
    def make(n_src=1, n_dst=1, esz=8, **kw):
        arr = np.zeros(1, dtype=_lib.PLACE_DTYPE)
        arr['ndim'] = 1
        arr['shape'][0, 0] = 4
        arr['src_strides'][0, 0] = arr['dst_strides'][0, 0] = 1
        for k, v in kw.items():
            arr[k] = v
        return bb.place_plan(arr, n_src, n_dst, esz)
    make()
    with pytest.raises(ValueError, match='ndim'):
        make(ndim=9)
    with pytest.raises(ValueError, match='src_block'):
        make(src_block=1)
    with pytest.raises(ValueError, match='dst_block'):
        make(dst_block=-1)
    with pytest.raises(ValueError, match='elem_size'):
        make(esz=4)
    with pytest.raises(ValueError, match='offset'):
        make(src_offset=-1)
    plan = make()
    with pytest.raises(ValueError):
        bb.place_enqueue(plan, [0], [0])            # a block a record names has no address
    with pytest.raises(ValueError):
        bb.place_enqueue(plan, [], [])              # tables of the wrong length
    # Python level
    t = ab.AbelianTensor.from_spec(bb, CASES[CASE_IDS.index('u1-r4-middle')]['tensor'])
    with pytest.raises(ValueError):
        ab.combine_legs(bb, t, [[0, 1], [1, 2]])
    sym = ab.Symmetry((0,))
    leg = ab.Leg(sym, [[0]], [1], +1)
    nine = ab.AbelianTensor(sym, [leg] * 9, [bb.block_from_numpy(np.ones([1] * 9))], np.zeros((1, 9), np.int64), 4)
    with pytest.raises(ValueError):
        ab.combine_legs(bb, nine, [[0, 1]])


# --------------------------------------------------------------------------------------------- sizes a user runs

@pytest.mark.parametrize('config', ['u1', 'u1u1'])
def test_theta_chi4096_matches_combine_legs_to_matrix(bb, config):
    """the two-site theta at chi = 4096, groups (0, 1), (2, 3): blocks bit-identical to combine_legs_to_matrix on the same
    theta, and the round trip returns theta bit for bit"""
    A, B = wl.config_u1_mps(4096) if config == 'u1' else wl.config_u1u1_mps(4096)
    theta = ab.compose(bb, ab.AbelianTensor.from_spec(bb, A), ab.AbelianTensor.from_spec(bb, B), 1)
    mv = ab.combine_legs_to_matrix(bb, theta, 2)
    got = ab.combine_legs(bb, theta, [[0, 1], [2, 3]], signs=[+1, -1])
    assert len(got.blocks) == len(mv.blocks) > 0
    assert np.array_equal(got.legs[0].sectors[got.block_inds[:, 0]], mv.charges)
    for x, y in zip(got.blocks, mv.blocks):
        assert x.shape == y.shape and np.array_equal(bb.to_numpy(x), bb.to_numpy(y))
    for back in (ab.split_legs(bb, got), ab.split_legs(bb, got, contiguous=True)):
        assert np.array_equal(back.block_inds, theta.block_inds)
        for x, y in zip(back.blocks, theta.blocks):
            assert np.array_equal(bb.to_numpy(x), bb.to_numpy(y))
