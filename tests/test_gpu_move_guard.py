"""The data-movement kernels of csrc/blockops.hip at the C ABI on guard-band cases (tests/move_guard_cases.py): every
source and destination a view into a larger arena, every byte compared -- the addressed elements against a numpy
reference bit for bit, everything around them and every source against what was uploaded.
tests/test_move_guard_model.py shows on the host that each kind of fault is flagged, and which kernel class each copy
record reaches."""
import functools

import numpy as np
import pytest

import move_guard_cases as mc
from gemm_guard_worker import DeviceMemory
from move_guard_worker import mask_desc, refused, run_case, status

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()


@functools.lru_cache(maxsize=4)
def _case(group, name):
    """Cases are immutable (a run uploads copies of the arenas)."""
    return CASES[group][name]()


def _assert_clean(bb, case, launches=1, expect=None):
    rep = mc.check(case, run_case(bb, case, launches), expect)
    assert rep.clean, str(rep)


@pytest.mark.parametrize('name', list(CASES['copy']))
def test_strided_copy(bb, name):
    """Row, shared-row, elementwise, 32 x 32 and 64 x 64 tiled and composite records for elem_size 1, 4, 8 and 16, plain and
    conjugated, aligned and not, tiled and strided records in one call, negative and zero strides."""
    _assert_clean(bb, _case('copy', name))


@pytest.mark.parametrize('name', list(CASES['mask']))
def test_mask_gather_and_scatter(bb, name):
    """After a scatter every position that was not kept is +0.0 bitwise, and everything outside `out` is untouched."""
    _assert_clean(bb, _case('mask', name))


@pytest.mark.parametrize('name', list(CASES['scale']))
def test_scale_axis(bb, name):
    """x * f in float64, bit for bit: the pair path with its `j1` wrap at inner == 1, odd totals, x and out aligned
    differently, item boundaries, -0.0 in data and factors, out of place and in place."""
    _assert_clean(bb, _case('scale', name))


@pytest.mark.parametrize('name', list(CASES['cexpand']))
def test_complex_expand(bb, name):
    """[[br, bi], [-bi, br]] per element, row 2k + 1 holding -bi bitwise (also for +0.0 and -0.0), from row-major,
    transposed and sub-view sources, items that end inside a descriptor."""
    _assert_clean(bb, _case('cexpand', name))


@pytest.mark.parametrize('name', list(CASES['lincomb']))
def test_strided_linear_combination(bb, name):
    """Exact data: 0, 1 and 3 terms, accumulate 0 and 1 (no terms: zeros, or dst unchanged), gaps in dst, permuted source
    strides, ndim 0 to 8, real sources beside complex ones."""
    _assert_clean(bb, _case('lincomb', name))


@pytest.mark.parametrize('group,name', [('copy', 'row es1'), ('copy', 'composite es8'), ('copy', 'transpose es16 conj'), ('mask', 'gather'),
                                        ('mask', 'scatter'), ('scale', 'out of place'), ('cexpand', 'all')])
def test_a_second_launch_gives_the_same_bytes(bb, group, name):
    _assert_clean(bb, _case(group, name), launches=2)


def test_scale_axis_in_place_twice_applies_the_factors_twice(bb):
    case = _case('scale', 'in place')
    _assert_clean(bb, case, launches=2, expect=mc.scale_twice_expect(case))


def _uploaded(bb, case):
    mem = DeviceMemory(bb)
    bases = mem.upload(case.ain.view(np.float64)), mem.upload(case.aout0.view(np.float64))
    return mem, bases


def _untouched(mem, bases, case):
    gin = mem.download(bases[0], case.ain.size // 8).view(np.uint8)
    gout = mem.download(bases[1], case.aout0.size // 8).view(np.uint8)
    return np.array_equal(gin, case.ain) and np.array_equal(gout, case.aout0)


def test_refused_calls_launch_nothing(bb):
    """elem_size 2 and 3, conj on anything but 16-byte elements and a complex expansion whose src or dst is not 16-byte
    aligned are CYB_ERR_INVALID, and the arenas stay as they were; an empty list is CYB_OK."""
    case = mc.copy_elementwise_case(1)
    mem, bases = _uploaded(bb, case)
    for es in (2, 3, 0, 32):
        assert refused(bb, 'copy', case.descriptors(*bases), es)
    assert _untouched(mem, bases, case)
    case = mc.copy_transpose_case(16, True, 1)
    mem, bases = _uploaded(bb, case)
    for es in (1, 4, 8):
        assert refused(bb, 'copy', case.descriptors(*bases), es)
    assert _untouched(mem, bases, case)
    case = mc.cexpand_real_case()
    mem, bases = _uploaded(bb, case)
    for which in ('src', 'dst'):
        assert refused(bb, 'cexpand', mc.cexpand_misaligned(case, which)(*bases), 8)
    assert _untouched(mem, bases, case)
    assert status(bb, 'copy', (None, 0), 8) == 0 and status(bb, 'cexpand', (None, 0), 8) == 0 and status(bb, 'gather', (None, 0), 8) == 0


# ---- the index range of 2^31 elements and beyond ----------------------------------------------------------------------

BIG = (1 << 31) + 16            # doubles in the large buffer: 16 GiB and 128 bytes


def _positions(axis):
    """64 distinct kept positions: the first 16, 16 around the middle, the last 32 -- in a mixed order."""
    pos = np.concatenate([np.arange(16), axis // 2 - 8 + np.arange(16), axis - 32 + np.arange(32)]).astype(np.int64)
    return pos[np.random.default_rng(5).permutation(pos.size)]


def _small_arena(torch, n):
    """n + 32 doubles of distinct finite sentinels on the device, and the same on the host; the view starts at element 16."""
    host = mc.SENTINEL * (1.0 + np.arange(n + 32) * 2.0 ** -40)
    return torch.from_numpy(host).to('cuda:0'), host


def _kept_values(n_keep, inner):
    vals = np.arange(1, n_keep * inner + 1, dtype=np.float64).reshape(n_keep, inner)
    vals[::3] = -vals[::3]
    return vals


def test_mask_beyond_32_bit_indices(bb):
    """A float64 block of just over 2^31 elements: gathers of 64 kept slices through the 16-byte pair branch (inner 2,
    aligned), the 64-bit scalar branch (inner 3) and, with `axis` reduced to a product just under 2^31, the 32-bit branch
    at its upper end; scatters into such a block through the pair and the scalar branch.  Only the kept slices of the large
    buffer are written or read back; the small side sits between guard bands."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * (1 << 30):
        pytest.skip(f'needs 40 GiB of free device memory for a 16 GiB block, {free / (1 << 30):.0f} GiB are free')
    dev = 'cuda:0'
    x = torch.empty(BIG, dtype=torch.float64, device=dev)
    assert x.data_ptr() % 16 == 0
    # (inner, axis): products 2^31 + 16 (pair branch; 64-bit scalar branch) and 2^31 - 2 (the 32-bit branch, even and odd inner)
    for inner, axis in ((2, BIG // 2), (3, BIG // 3), (2, (1 << 30) - 1), (3, ((1 << 31) - 2) // 3)):
        assert (axis * inner >= 1 << 31) == (axis * inner == BIG) and axis * inner <= BIG
        pos = _positions(axis)
        vals = _kept_values(pos.size, inner)
        where = torch.from_numpy((pos[:, None] * inner + np.arange(inner)).reshape(-1)).to(dev)
        x[where] = torch.from_numpy(vals.reshape(-1)).to(dev)
        idx = torch.from_numpy(pos).to(dev)
        out, host = _small_arena(torch, vals.size)
        torch.cuda.synchronize()
        arrays = mask_desc(x.data_ptr(), out.data_ptr() + 128, idx.data_ptr(), 1, axis, inner, pos.size)
        assert status(bb, 'gather', arrays, 8) == 0
        bb.synchronize()
        host[16:16 + vals.size] = vals.reshape(-1)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), host.view(np.uint64)), f'gather inner {inner} axis {axis}'
        del out, idx, where
    del x
    torch.cuda.empty_cache()
    big = torch.empty(BIG, dtype=torch.float64, device=dev)
    for inner, axis in ((2, BIG // 2), (3, BIG // 3)):
        pos = _positions(axis)
        vals = _kept_values(pos.size, inner)
        small, _ = _small_arena(torch, vals.size)
        small[16:16 + vals.size] = torch.from_numpy(vals.reshape(-1)).to(dev)
        idx = torch.from_numpy(pos).to(dev)
        torch.cuda.synchronize()
        arrays = mask_desc(small.data_ptr() + 128, big.data_ptr(), idx.data_ptr(), 1, axis, inner, pos.size)
        assert status(bb, 'scatter', arrays, 8) == 0
        bb.synchronize()
        where = (pos[:, None] * inner + np.arange(inner)).reshape(-1)
        got = big[torch.from_numpy(where).to(dev)].cpu().numpy()
        assert np.array_equal(got.view(np.uint64), vals.reshape(-1).view(np.uint64)), f'scatter inner {inner}'
        kept = set(where.tolist())
        zeros = np.array(sorted(set(np.concatenate([where - inner, where + inner, np.random.default_rng(7).integers(0, BIG, 4096),
                                                    [0, BIG - 1, (1 << 31) - 1, 1 << 31]]).tolist()) - kept))
        zeros = zeros[(zeros >= 0) & (zeros < BIG)]
        got = big[torch.from_numpy(zeros).to(dev)].cpu().numpy()
        assert not got.view(np.uint64).any(), f'scatter inner {inner}: a position that was not kept is not +0.0'
        del small, idx
    del big
    torch.cuda.empty_cache()
