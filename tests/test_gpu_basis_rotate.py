"""cyb_basis_rotate_f64 (krylov_vec.hip) at the C-ABI, through cyten_amd._lib: dst[i] = sum_j q[j, i] src[j], the in-place
basis rotation of thick-restart Lanczos.  Every vector lives inside a larger device buffer with sentinel bands before and
after it, so a read or write outside [0, n) of a vector shows."""
import ctypes as C

import numpy as np
import pytest

from cyten_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 1234.5
TILE = 512                      # positions per workgroup step of the 16-byte path (256 on the 8-byte path)
GRID_CAP = 2048                 # workgroups at most: more tiles than that are shared out, a fixed number per workgroup
SHAPES = [(1, 1), (2, 2), (5, 3), (33, 17), (64, 32)]
SIZES = [1, 255, 256, 257, 3 * TILE + 5]
MODES = ['in_place', 'out_of_place', 'reversed']
ALIGNED, ODD = GUARD, GUARD + 1  # first element of a vector in its buffer: 16-byte aligned / 8-byte aligned only


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _ptrs(addresses):
    return (C.c_void_p * max(len(addresses), 1))(*addresses)


class Vectors:
    """the rows of V, each in a device buffer of its own between two sentinel bands"""

    def __init__(self, V, first):
        self.first, self.n = first, V.shape[1]
        self.before = []
        for v in V:
            h = np.full(first + self.n + GUARD, SENTINEL)
            h[first:first + self.n] = v
            self.before.append(h)
        self.dev = [_dev(h) for h in self.before]
        assert all(t.data_ptr() % 16 == 0 for t in self.dev)
        self.ptrs = [t.data_ptr() + 8 * first for t in self.dev]

    def after(self):
        """(the vectors now, True if every sentinel band is bit-unchanged)"""
        hosts = [t.cpu().numpy() for t in self.dev]
        bands = all(h[:self.first].tobytes() == b[:self.first].tobytes() and
                    h[self.first + self.n:].tobytes() == b[self.first + self.n:].tobytes() for h, b in zip(hosts, self.before))
        return np.array([h[self.first:self.first + self.n] for h in hosts]).reshape(len(hosts), self.n), bands

    def unchanged(self):
        return all(t.cpu().numpy().tobytes() == b.tobytes() for t, b in zip(self.dev, self.before))


def _call(bb, src, m, dst, k, Q, n):
    """the status of one call on raw addresses (None: a NULL table)"""
    import torch
    bb.ctx.sync_stream()
    q = None if Q is None else np.ascontiguousarray(Q, dtype=np.float64)
    rc = bb.lib.cyb_basis_rotate_f64(bb.ctx.handle, None if src is None else _ptrs(src), m, None if dst is None else _ptrs(dst), k,
                                     None if q is None else q.ctypes.data_as(C.c_void_p), n)
    torch.cuda.synchronize()
    return rc


def _rotate(bb, V, Q, mode, first):
    """(results k x n, rows of V afterwards, every band intact)"""
    m, n = V.shape
    k = Q.shape[1]
    S = Vectors(V, first)
    if mode == 'in_place':
        D, dst = S, S.ptrs[:k]
    elif mode == 'reversed':
        D, dst = S, [S.ptrs[m - 1 - i] for i in range(k)]
    else:
        D = Vectors(np.full((k, n), -77.0), first)
        dst = D.ptrs
    _lib.check(_call(bb, S.ptrs, m, dst, k, Q, n))
    src_after, ok = S.after()
    if mode == 'in_place':
        return src_after[:k], src_after, ok
    if mode == 'reversed':
        return src_after[[m - 1 - i for i in range(k)]], src_after, ok
    out, ok_d = D.after()
    return out, src_after, ok and ok_d


def _untouched_rows(m, k, mode):
    return {'in_place': list(range(k, m)), 'reversed': list(range(0, m - k)), 'out_of_place': list(range(m))}[mode]


def _integers(rng, shape, bound):
    return rng.integers(-bound, bound + 1, size=shape).astype(np.float64)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('m,k', SHAPES, ids=lambda v: str(v))
def test_exact_products_in_every_aliasing_mode_and_alignment(bb, rng, m, k, mode):
    """integer data |x| <= 8, |q| <= 4: every partial sum is an integer below 2^53, so any order of summation gives numpy's
    result exactly -- what differs is a missed, repeated or overwritten-before-read element"""
    for n in SIZES:
        V, Q = _integers(rng, (m, n), 8), _integers(rng, (m, k), 4)
        want = (V.T @ Q).T
        for first in (ALIGNED, ODD):
            got, rows, bands = _rotate(bb, V, Q, mode, first)
            assert np.array_equal(got, want), (n, first)
            keep = _untouched_rows(m, k, mode)
            assert rows[keep].tobytes() == V[keep].tobytes(), (n, first)     # nothing else moves
            assert bands, (n, first)


@pytest.mark.parametrize('first', [ALIGNED, ODD], ids=['aligned16', 'aligned8'])
def test_more_tiles_than_the_grid_cap(bb, rng, first):
    """two tiles (16-byte path) or three (8-byte path) per workgroup; m = 2, k = 1: three vectors only"""
    n = GRID_CAP * TILE + TILE + 3
    V, Q = _integers(rng, (2, n), 8), _integers(rng, (2, 1), 4)
    got, rows, bands = _rotate(bb, V, Q, 'out_of_place', first)
    assert np.array_equal(got, (V.T @ Q).T) and rows.tobytes() == V.tobytes() and bands


def test_rounding_bound_repeatability_and_alignment_independence(bb, rng):
    """one fma per term in ascending j: |err| <= gamma_m (|Q|^T |V|) with gamma_m = m eps / (1 - m eps) < 2 m eps (Higham,
    Accuracy and Stability, (3.5)), eps the unit roundoff 2^-53 -- the bound is derived, not measured"""
    m, k, n = 33, 17, 3 * TILE + 5
    V, Q = rng.standard_normal((m, n)), rng.standard_normal((m, k))
    want = (V.astype(np.longdouble).T @ Q.astype(np.longdouble)).T
    bound = 2 * m * 2.0 ** -53 * (np.abs(Q).T @ np.abs(V))
    runs = [_rotate(bb, V, Q, mode, first)[0] for mode in MODES for first in (ALIGNED, ODD)]
    runs.append(_rotate(bb, V, Q, 'in_place', ALIGNED)[0])          # the same call again
    err = np.abs(runs[0].astype(np.longdouble) - want)
    print('largest error / bound:', float((err / bound).max()))
    assert np.all(err <= bound)
    for r in runs[1:]:
        assert r.tobytes() == runs[0].tobytes()


@pytest.mark.parametrize('mode', ['in_place', 'out_of_place'])
def test_a_permutation_matrix_copies_bits(bb, rng, mode):
    m, n = 7, 1029
    V = rng.standard_normal((m, n))
    perm = rng.permutation(m)
    Q = np.zeros((m, m))
    Q[perm, np.arange(m)] = 1.0                                      # column i picks row perm[i]
    for first in (ALIGNED, ODD):
        got, _, bands = _rotate(bb, V, Q, mode, first)
        assert got.tobytes() == V[perm].tobytes() and bands


def test_a_nan_stays_at_its_position(bb, rng):
    m, k, n, j, p = 5, 3, 777, 2, 300
    V, Q = rng.standard_normal((m, n)), rng.standard_normal((m, k))
    Q[j, 1] = 0.0                                                     # 0 * NaN is NaN as well
    clean = _rotate(bb, V, Q, 'in_place', ALIGNED)[0]
    bad = V.copy()
    bad[j, p] = np.nan
    for first in (ALIGNED, ODD):
        got, rows, bands = _rotate(bb, bad, Q, 'in_place', first)
        assert np.all(np.isnan(got[:, p])) and bands
        assert np.delete(got, p, axis=1).tobytes() == np.delete(clean, p, axis=1).tobytes()
        assert rows[k:].tobytes() == bad[k:].tobytes()


def test_bad_arguments_launch_nothing(bb, rng):
    n = 100
    V = _integers(rng, (65, n), 8)
    S = Vectors(V, ALIGNED)
    D = Vectors(np.full((33, n), -77.0), ALIGNED)
    Q = np.ones((65, 33))
    lib, INVALID = bb.lib, _lib.CYB_ERR_INVALID

    def refused(rc, word):
        return rc == INVALID and word in lib.cyb_last_error().decode()

    assert refused(_call(bb, S.ptrs, 65, D.ptrs[:4], 4, Q, n), '65')
    assert refused(_call(bb, S.ptrs[:8], 8, D.ptrs, 33, Q, n), '33')
    assert refused(_call(bb, None, 8, D.ptrs[:4], 4, Q, n), 'NULL')
    assert refused(_call(bb, S.ptrs[:8], 8, None, 4, Q, n), 'NULL')
    assert refused(_call(bb, S.ptrs[:8], 8, D.ptrs[:4], 4, None, n), 'NULL')
    assert refused(_call(bb, [S.ptrs[0], 0], 2, D.ptrs[:1], 1, Q, n), 'NULL')
    assert refused(_call(bb, S.ptrs[:8], 8, [D.ptrs[0], D.ptrs[1], D.ptrs[0]], 3, Q, n), 'overlap')          # two equal dst
    assert refused(_call(bb, S.ptrs[:8], 8, [S.ptrs[0], S.ptrs[0]], 2, Q, n), 'overlap')
    assert refused(_call(bb, S.ptrs[:8], 8, [D.ptrs[0], D.ptrs[0] + 8], 2, Q, n), 'overlap')                  # partly: dst / dst
    assert refused(_call(bb, S.ptrs[:8], 8, [S.ptrs[3] + 8 * (n - 1)], 1, Q, n), 'overlap')                   # partly: dst / src
    assert refused(_call(bb, S.ptrs[:8], 8, [S.ptrs[3] - 8], 1, Q, n), 'overlap')
    assert refused(_call(bb, S.ptrs[:8], 8, [D.ptrs[0] + 4], 1, Q, n), 'misaligned')
    with pytest.raises(ValueError):
        _lib.check(_call(bb, S.ptrs, 65, D.ptrs[:4], 4, Q, n))
    for m, k, nn in ((0, 4, n), (8, 0, n), (8, 4, 0)):
        assert _call(bb, S.ptrs[:8], m, D.ptrs[:4], k, Q, nn) == _lib.CYB_OK
    assert _call(bb, None, 0, None, 0, None, 0) == _lib.CYB_OK
    assert S.unchanged() and D.unchanged()


def test_a_complex_pool_is_rotated_as_twice_as_many_doubles(bb, rng):
    m, k, n = 6, 4, 515
    V = _integers(rng, (m, n), 8) + 1j * _integers(rng, (m, n), 8)
    Q = _integers(rng, (m, k), 4)
    got, rows, bands = _rotate(bb, np.ascontiguousarray(V).view(np.float64).reshape(m, 2 * n), Q, 'in_place', ALIGNED)
    assert np.array_equal(np.ascontiguousarray(got).view(np.complex128), (V.T @ Q).T) and bands
    assert rows[k:].view(np.complex128).tobytes() == V[k:].tobytes()
