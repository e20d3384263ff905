"""numpy side of the tests of the operator-building functions of cyten_amd.abelian (outer, tensor_from_grid, trivial legs):
the numpy stand-in backend with ``tensor_outer_many``, the dense expectations the reference's own tests use, and the
site operators / known Hamiltonians of the model layer (toycodes/tenpy_toycodes/b_model.py) restated with numpy only."""
import numpy as np

from cyten_amd import abelian as ab
from numpy_tensor_backend import NumpyTensorBackend


class NumpyOuterBackend(NumpyTensorBackend):
    def add_axis(self, a, pos):
        return np.expand_dims(a, pos)

    def squeeze_axes(self, a, idcs):
        return np.squeeze(a, tuple(idcs))

    def tensor_outer_many(self, pairs, K):
        outs = []
        for a, b in pairs:
            if a.ndim + b.ndim > 8:
                raise ValueError('more than 8 axes')
            outs.append(np.ascontiguousarray(dense_outer(a, b, K)))
        cplx = any(np.iscomplexobj(o) for o in outs)
        return [o.astype(complex) for o in outs] if cplx else outs


class NumpyPairLoopBackend(NumpyTensorBackend):
    """a backend WITHOUT ``tensor_outer_many`` and without placement plans: ``outer`` must loop over ``tensor_outer``"""

    def tensor_outer(self, a, b, K):
        return dense_outer(a, b, K)


# ------------------------------------------------------------------------------------------- dense expectations

def dense_outer(A, B, K):
    """tests/python_tests/test_tensors.py:2768-2772 with cA = K: the axes of B between the first K and the other axes of A"""
    nA, nB = np.ndim(A), np.ndim(B)
    perm = [*range(K), *range(nA, nA + nB), *range(K, nA)]
    return np.transpose(np.tensordot(A, B, [(), ()]), perm)


def assert_products_equal(got, want, A, B, K):
    """float64: every element is ONE correctly rounded product on both sides, so the arrays are equal.  complex: each side
    rounds a two-term sum of products per component, error at most 2u (|a_r b_r| + |a_i b_i|) <= 2u |a| |b| with u = 2^-53 (and
    may or may not contract it to an FMA), so the two differ by at most 4 * 2^-52 * |a| |b| per element."""
    assert got.shape == want.shape and got.dtype == want.dtype
    if np.iscomplexobj(want):
        assert np.all(np.abs(got - want) <= 4 * 2.0 ** -52 * dense_outer(np.abs(A), np.abs(B), K))
    else:
        assert np.array_equal(got, want)


def dense_grid(grid_dense, num_codomain):
    """test_tensors.py:3809-3813: concatenate along axis ``num_codomain`` inside a row, along axis 0 over the rows (a ``None``
    cell must have been replaced by zeros of its shape).  This is the stacked tensor in the basis of the concatenation; see
    `stacked_basis` for the basis of the direct sum."""
    return np.concatenate([np.concatenate(row, axis=num_codomain) for row in grid_dense], axis=0)


def stacked_basis(spaces):
    """The direct sum of `spaces` (objects with ``sectors`` and ``mults``, sectors sorted) orders its basis by sector and,
    inside a sector, by space; the concatenation orders it by space.  Entry j of the result is the position in the
    concatenation of basis state j of the direct sum (the ``basis_perm`` the reference gives the direct sum, through which
    its ``to_numpy`` of a stacked tensor is the plain concatenation)."""
    offs = np.concatenate([[0], np.cumsum([int(np.sum(sp.mults)) for sp in spaces])])
    union = sorted({tuple(s) for sp in spaces for s in np.asarray(sp.sectors).tolist()}, key=lambda q: tuple(reversed(q)))
    out = []
    for sec in union:
        for sp, off in zip(spaces, offs):
            sl = np.concatenate([[0], np.cumsum(sp.mults)])
            for k, s in enumerate(np.asarray(sp.sectors).tolist()):
                if tuple(s) == sec:
                    out += list(range(int(off + sl[k]), int(off + sl[k + 1])))
    return np.array(out, dtype=np.int64)


# ------------------------------------------------------------------------------------------- site operators

SX = np.array([[0.0, 1.0], [1.0, 0.0]])
SY = np.array([[0.0, -1.0j], [1.0j, 0.0]])
SZ = np.array([[1.0, 0.0], [0.0, -1.0]])
SP = np.array([[0.0, 1.0], [0.0, 0.0]])      # sigma^+ = (X + iY) / 2
SM = SP.T.copy()
ID = np.eye(2)


def site_op(bb, sym, p, mat, q_left, q_right):
    """the 2 x 2 matrix `mat` on site leg `p` as the MPO entry ``[wL, p, wR, p*]`` (num_codomain 2) with single-sector bond
    legs of charges `q_left` (sign +1) and `q_right` (sign -1); the charge rule is checked"""
    wl, wr = ab.Leg(sym, [q_left], [1], +1), ab.Leg(sym, [q_right], [1], -1)
    inds = [(0, i, 0, j) for i in range(2) for j in range(2) if mat[i, j] != 0]
    t = ab.AbelianTensor.from_numpy_blocks(bb, sym, [wl, p, wr, p.dual()], [np.full((1, 1, 1, 1), mat[i, j]) for _, i, _, j in inds],
                                           np.array(inds, dtype=np.int64).reshape(len(inds), 4), 2)
    t.check_charges()
    return t


def two_leg_op(bb, sym, p, mat):
    """a charge-conserving 2 x 2 matrix as the tensor ``[p, p*]`` (num_codomain 1)"""
    inds = [(i, j) for i in range(2) for j in range(2) if mat[i, j] != 0]
    t = ab.AbelianTensor.from_numpy_blocks(bb, sym, [p, p.dual()], [np.full((1, 1), mat[i, j]) for i, j in inds],
                                           np.array(inds, dtype=np.int64).reshape(len(inds), 2), 1)
    t.check_charges()
    t.labels = ['p', 'p*']
    return t


def with_trivial_bonds(bb, op2):
    """``[p, p*]`` -> ``[wL, p, wR, p*]`` with trivial bond legs, through add_trivial_leg"""
    return ab.add_trivial_leg(bb, ab.add_trivial_leg(bb, op2, 0, label='wL'), 2, to_domain=True, label='wR')


def stacked_index(total, spaces, i):
    """dense index, on the direct sum `total` of `spaces`, of the (single) basis state of ``spaces[i]``"""
    sec = spaces[i].sectors[0]
    where = [k for k, s in enumerate(total.sectors) if np.array_equal(s, sec)][0]
    before = sum(int(sp.mults[0]) for sp in spaces[:i] if np.array_equal(sp.sectors[0], sec))
    return int(total.slices[where]) + before


def mpo_to_matrix(W, L, i_left, i_right):
    """the dense ``[wL, p, wR, p*]`` array `W` on L sites between the boundary states `i_left` / `i_right` as a 2^L x 2^L matrix"""
    acc = W[i_left][None]                                  # [1, p, wR, p*] -> rows, bond, cols
    acc = np.transpose(acc, (0, 1, 3, 2)).reshape(2, 2, W.shape[2])
    for _ in range(L - 1):
        acc = np.einsum('rcw,wpvq->rpcqv', acc, W)
        r, p, c, q, v = acc.shape
        acc = acc.reshape(r * p, c * q, v)
    return acc[:, :, i_right]


def kron_all(ops):
    out = np.eye(1)
    for o in ops:
        out = np.kron(out, o)
    return out


def chain_hamiltonian(L, two_site_terms, one_site_terms=()):
    """sum_i sum_(c, A, B) c A_i B_{i+1} + sum_i sum_(c, A) c A_i as a dense matrix (the Kronecker construction of
    b_model.py:175-206)"""
    H = np.zeros((2 ** L, 2 ** L), dtype=complex)
    for i in range(L - 1):
        for c, A, B in two_site_terms:
            H += c * kron_all([ID] * i + [A, B] + [ID] * (L - i - 2))
    for i in range(L):
        for c, A in one_site_terms:
            H += c * kron_all([ID] * i + [A] + [ID] * (L - i - 1))
    return H


def tfi_mpo(bb, J, g):
    """(W, left boundary index, right boundary index): the TFI MPO tensor from the grid of b_model.py:74-78, Z2 parity"""
    sym = ab.Symmetry([2])
    p = ab.Leg(sym, [[0], [1]], [1, 1], +1)
    I = with_trivial_bonds(bb, two_leg_op(bb, sym, p, ID))
    Z = with_trivial_bonds(bb, two_leg_op(bb, sym, p, SZ))
    XL, XR = site_op(bb, sym, p, SX, [0], [1]), site_op(bb, sym, p, SX, [1], [0])
    grid = [[I, ab.scale(bb, -J, XL), ab.scale(bb, -g, Z)],
            [None, None, XR],
            [None, None, I]]
    W = ab.tensor_from_grid(bb, grid, labels=['wL', 'p', 'wR', 'p*'])
    lefts, rights = [I.legs[0], XR.legs[0], I.legs[0]], [I.legs[2], XL.legs[2], I.legs[2]]
    return W, stacked_index(W.legs[0], lefts, 0), stacked_index(W.legs[2], rights, 2)


def heisenberg_mpo(bb, J):
    """the same for J (XX + YY + ZZ) = J (2 s+ s- + 2 s- s+ + ZZ) with U(1) (2 Sz) and charged s+- bonds"""
    sym = ab.Symmetry([0])
    p = ab.Leg(sym, [[1], [-1]], [1, 1], +1)       # (Leg sorts: sector -1 first; the matrices below are in that order)
    up_first = [1, 0]                              # basis order of SP / SM / SZ is (up, down): reorder to (down, up)
    m = {k: v[np.ix_(up_first, up_first)] for k, v in dict(I=ID, Z=SZ, P=SP, M=SM).items()}
    I = with_trivial_bonds(bb, two_leg_op(bb, sym, p, m['I']))
    Z = with_trivial_bonds(bb, two_leg_op(bb, sym, p, m['Z']))
    row0 = [I, ab.scale(bb, 2 * J, site_op(bb, sym, p, m['P'], [0], [2])), ab.scale(bb, 2 * J, site_op(bb, sym, p, m['M'], [0], [-2])),
            ab.scale(bb, J, Z), None]
    last = [None, site_op(bb, sym, p, m['M'], [2], [0]), site_op(bb, sym, p, m['P'], [-2], [0]), Z, I]
    grid = [row0] + [[None] * 4 + [op] for op in last[1:]]
    W = ab.tensor_from_grid(bb, grid, labels=['wL', 'p', 'wR', 'p*'])
    lefts = [I.legs[0]] + [op.legs[0] for op in last[1:]]
    rights = [op.legs[2] for op in row0[:4]] + [I.legs[2]]
    return W, stacked_index(W.legs[0], lefts, 0), stacked_index(W.legs[2], rights, 4), up_first


def heisenberg_bond(bb, J):
    """(h, dense 4 x 4 matrix in the (down, up) basis per site): J (XX + YY + ZZ) on two sites as the tensor
    ``[p0, p1, p1*, p0*]`` built with outer: the charged s+- factors carry a third, single-sector leg that is traced out"""
    sym = ab.Symmetry([0])
    p = ab.Leg(sym, [[-1], [1]], [1, 1], +1)
    flip = [1, 0]
    sp, sm, sz = SP[np.ix_(flip, flip)], SM[np.ix_(flip, flip)], SZ[np.ix_(flip, flip)]

    def charged(mat, legs, where, ncod):
        inds = [(i, j) for i in range(2) for j in range(2) if mat[i, j] != 0]
        rows = [[0 if k == where else (i if k == legs.index(p) else j) for k in range(3)] for i, j in inds]
        t = ab.AbelianTensor.from_numpy_blocks(bb, sym, legs, [np.full((1, 1, 1), mat[i, j]) for i, j in inds], np.array(rows).reshape(len(rows), 3), ncod)
        t.check_charges()
        return t
    terms = []
    for first, second in ((sp, sm), (sm, sp)):
        # first: [p, p*, c] sheds the charge it changes; second: [c', p, p*] takes it up
        q = 2 if first is sp else -2
        co, ci = ab.Leg(sym, [[q]], [1], -1), ab.Leg(sym, [[q]], [1], +1)
        a = charged(first, [p, p.dual(), co], 2, 1)
        b = charged(second, [ci, p, p.dual()], 0, 2)
        t = ab.outer(bb, a, b)                                  # [p0, c', p1, p1*, p0*, c]
        terms.append(ab.partial_trace(bb, t, [(1, 5)]))
    zz = ab.outer(bb, two_leg_op(bb, sym, p, sz), two_leg_op(bb, sym, p, sz), {'p': 'p0', 'p*': 'p0*'}, {'p': 'p1', 'p*': 'p1*'})
    h = ab.linear_combination(bb, 2 * J, terms[0], 2 * J, terms[1])
    h = ab.linear_combination(bb, 1.0, h, J, zz)
    dense = J * (2 * np.kron(sp, sm) + 2 * np.kron(sm, sp) + np.kron(sz, sz))
    return h, dense
