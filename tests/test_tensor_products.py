"""outer, direct_sum, tensor_from_grid, add_trivial_leg and squeeze_legs of cyten_amd.abelian on the numpy stand-in: the host
logic (block tables, legs, labels, placement) against the dense expectations of the reference's own tests, and the known
Hamiltonians of the model layer built from site operators."""
import numpy as np
import pytest

import tensor_product_ref as ref
from cyten_amd import abelian as ab
from tensor_product_cases import GRID_IDS, OUTER_IDS, dense_of, grid_cases, outer_cases, to_tensor

NP = ref.NumpyOuterBackend()
LOOP = ref.NumpyPairLoopBackend()
OUTER = outer_cases()
GRID = grid_cases()
ALL_OUTER = pytest.mark.parametrize('case', range(len(OUTER)), ids=OUTER_IDS)
ALL_GRID = pytest.mark.parametrize('case', range(len(GRID)), ids=GRID_IDS)


def _is_sorted(t):
    return np.array_equal(t.block_inds, t.block_inds[np.lexsort(t.block_inds.T)]) if len(t.blocks) else True


def _labelled(bb, case):
    a, b = to_tensor(bb, case['a'], case['views']), to_tensor(bb, case['b'], case['views'])
    a.labels, b.labels = list('abcdefg')[:a.nlegs], list('hijklmn')[:b.nlegs]
    return a, b


# ------------------------------------------------------------------------------------------- outer

@pytest.mark.parametrize('bb', [NP, LOOP], ids=['grouped', 'pair-loop'])
@ALL_OUTER
def test_outer_dense(case, bb):
    c = OUTER[case]
    a, b = _labelled(bb, c)
    K = a.num_codomain
    got = ab.outer(bb, a, b, {'a': 'x'}, {'h': 'y'})
    A, B = dense_of(c['a']), dense_of(c['b'])
    want = ref.dense_outer(A, B, K)
    if np.iscomplexobj(want) and not len(got.blocks):
        want = want.real                                     # (no block: to_dense cannot know the dtype)
    ref.assert_products_equal(got.to_dense(bb), want, A, B, K)
    assert _is_sorted(got)
    got.check_charges()
    assert len(got.blocks) == len(a.blocks) * len(b.blocks)
    assert got.num_codomain == K + b.num_codomain
    assert got.legs == a.legs[:K] + b.legs + a.legs[K:]
    la, lb = ['x'] + a.labels[1:], ['y'] + b.labels[1:]
    assert got.labels == la[:K] + lb + la[K:]
    for blk, row in zip(got.blocks, got.block_inds):
        assert blk.shape == got.block_shape(row) and blk.flags['C_CONTIGUOUS']
    if any(np.iscomplexobj(x) for x in list(a.blocks) + list(b.blocks)):
        assert all(np.iscomplexobj(x) for x in got.blocks)


def test_outer_errors():
    a, b = _labelled(NP, OUTER[0])
    other = to_tensor(NP, OUTER[OUTER_IDS.index('z2-03x20')]['a'])
    with pytest.raises(ValueError, match='different symmetries'):
        ab.outer(NP, a, other)
    with pytest.raises(ValueError, match='duplicate labels'):
        ab.outer(NP, a, b, None, {'h': 'a'})
    big = ab.outer(NP, a, b)                              # 6 legs
    with pytest.raises(ValueError, match='more than 8 legs'):
        ab.outer(NP, big, a)
    assert ab.outer(NP, ab.AbelianTensor(a.symmetry, a.legs, [], np.zeros((0, 3)), 1), b).blocks == []


def test_outer_without_labels():
    c = OUTER[0]
    a, b = to_tensor(NP, c['a']), to_tensor(NP, c['b'])
    assert ab.outer(NP, a, b).labels == []
    b.labels = ['h', 'i', 'j']
    assert ab.outer(NP, a, b).labels == [None, 'h', 'i', 'j', None, None]


# ------------------------------------------------------------------------------------------- direct_sum

def test_direct_sum():
    sym = ab.Symmetry([0])
    s = ab.direct_sum([ab.Leg(sym, [[1], [-1]], [2, 3], -1), ab.Leg(sym, [[0], [1]], [4, 5], -1), ab.Leg(sym, [[-1]], [1], -1)])
    assert s.sectors.tolist() == [[-1], [0], [1]] and s.mults.tolist() == [4, 4, 7] and s.sign == -1
    with pytest.raises(ValueError, match='same symmetry and sign'):
        ab.direct_sum([ab.Leg(sym, [[0]], [1], +1), ab.Leg(sym, [[0]], [1], -1)])
    with pytest.raises(ValueError, match='same symmetry and sign'):
        ab.direct_sum([ab.Leg(sym, [[0]], [1], +1), ab.Leg(ab.Symmetry([2]), [[0]], [1], +1)])
    leg = ab.Leg(sym, [[0], [1]], [1, 1], +1)
    with pytest.raises(RuntimeError, match='ElementarySpace'):
        ab.direct_sum([leg, ab.LegPipe.from_legs(sym, [leg, leg])])
    with pytest.raises(ValueError):
        ab.direct_sum([])


# ------------------------------------------------------------------------------------------- tensor_from_grid

def _grid(bb, case):
    return [[None if s is None else to_tensor(bb, s, case['views']) for s in row] for row in case['grid']]


def _dense_grid(case):
    """None cells as zeros of the shape their row and column give them"""
    grid, n_cod = case['grid'], case['num_codomain']
    rows = []
    for i, row in enumerate(grid):
        out = []
        for j, s in enumerate(row):
            if s is None:
                in_row = next(x for x in row if x is not None)
                in_col = next(r[j] for r in grid if r[j] is not None)
                shape = list(dense_of(in_row).shape)
                shape[n_cod] = dense_of(in_col).shape[n_cod]
                out.append(np.zeros(shape))
            else:
                out.append(dense_of(s))
        rows.append(out)
    lefts = [next(x for x in row if x is not None).legs[0] for row in grid]
    rights = [next(r[j] for r in grid if r[j] is not None).legs[n_cod] for j in range(len(grid[0]))]
    want = ref.dense_grid(rows, n_cod)
    return np.take(np.take(want, ref.stacked_basis(lefts), axis=0), ref.stacked_basis(rights), axis=n_cod)


@ALL_GRID
def test_grid_dense(case):
    c = GRID[case]
    grid = _grid(NP, c)
    n = grid[0][0].nlegs
    labels = [f'l{k}' for k in range(n)]
    got = ab.tensor_from_grid(NP, grid, labels=labels)
    want = _dense_grid(c)
    dense = got.to_dense(NP)
    assert dense.shape == want.shape and np.array_equal(dense, want)
    assert _is_sorted(got) and len({tuple(r) for r in got.block_inds.tolist()}) == len(got.blocks)
    got.check_charges()
    assert got.num_codomain == c['num_codomain'] and got.labels == labels
    specs = [s for row in c['grid'] for s in row if s is not None]
    if any(np.iscomplexobj(b) for s in specs for b in s.blocks):
        assert all(np.iscomplexobj(b) for b in got.blocks)
    for k in range(n):
        if k not in (0, c['num_codomain']):
            assert got.legs[k] is grid[0][0].legs[k]


@ALL_GRID
def test_grid_commutes_with_permute_legs(case):
    """test_tensors.py:3816-3828: permuting the other legs before or after stacking is the same"""
    c = GRID[case]
    grid = _grid(NP, c)
    n, n_cod = grid[0][0].nlegs, c['num_codomain']
    rng = np.random.default_rng(case)
    others = [k for k in range(n) if k not in (0, n_cod)]
    perm = list(range(n))
    for k, src in zip(others, rng.permutation(others).tolist()):
        perm[k] = src
    res1 = ab.permute_legs(NP, ab.tensor_from_grid(NP, grid), perm)
    res2 = ab.tensor_from_grid(NP, [[None if op is None else ab.permute_legs(NP, op, perm) for op in row] for row in grid])
    assert np.array_equal(res1.block_inds, res2.block_inds)
    assert all(ab._same_leg(x, y) for x, y in zip(res1.legs, res2.legs))
    for x, y in zip(res1.blocks, res2.blocks):
        assert np.array_equal(x, y)


def test_grid_dtype_and_default_labels():
    c = GRID[GRID_IDS.index('z2-21-2x3-full')]
    grid = _grid(NP, c)
    grid[0][0].labels = ['wL', 'p', 'wR', 'p*'][:grid[0][0].nlegs]
    got = ab.tensor_from_grid(NP, grid, dtype='complex128')
    assert all(np.iscomplexobj(b) for b in got.blocks) and got.labels == grid[0][0].labels
    assert np.array_equal(got.to_dense(NP), _dense_grid(c))
    cz = GRID[GRID_IDS.index('u1-31-2x2-complex')]
    with pytest.raises(ValueError, match='real dtype'):
        ab.tensor_from_grid(NP, _grid(NP, cz), dtype='float64')


def test_grid_errors():
    c = GRID[GRID_IDS.index('z2-21-2x3-full')]
    g = _grid(NP, c)
    with pytest.raises(ValueError, match='grid must contain at least one tensor'):
        ab.tensor_from_grid(NP, [[None, None], [None, None]])
    with pytest.raises(ValueError, match='grid rows must have equal length'):
        ab.tensor_from_grid(NP, [g[0], g[1][:2]])
    with pytest.raises(ValueError, match='Must have at least one nonzero entry in each column.'):
        ab.tensor_from_grid(NP, [[g[0][0], None, g[0][2]], [g[1][0], None, g[1][2]]])
    with pytest.raises(ValueError, match='Must have at least one nonzero entry in each row.'):
        ab.tensor_from_grid(NP, [g[0], [None, None, None]])
    fewer = ab.AbelianTensor(g[0][0].symmetry, g[0][0].legs[:2], [], np.zeros((0, 2)), 1)
    with pytest.raises(RuntimeError, match='inconsistent number of legs in grid'):
        ab.tensor_from_grid(NP, [[g[0][0], fewer, g[0][2]], g[1]])
    t = g[0][1]
    other = ab.AbelianTensor(t.symmetry, [t.legs[0], t.legs[1].dual(), t.legs[2]], [], np.zeros((0, 3)), t.num_codomain)
    with pytest.raises(RuntimeError, match='inconsistent legs in grid'):
        ab.tensor_from_grid(NP, [[g[0][0], other, g[0][2]], g[1]])
    swapped = [[g[0][0], g[1][1], g[0][2]], [g[1][0], g[0][1], g[1][2]]]      # cells whose row legs do not match their row
    if not ab._same_leg(g[0][0].legs[0], g[1][0].legs[0]):
        with pytest.raises(RuntimeError, match='inconsistent legs in grid'):
            ab.tensor_from_grid(NP, swapped)
    pipe = ab.LegPipe.from_legs(t.symmetry, [t.legs[0], t.legs[1]])
    piped = ab.AbelianTensor(t.symmetry, [pipe, t.legs[1], t.legs[2]], [], np.zeros((0, 3)), t.num_codomain)
    with pytest.raises(RuntimeError, match='stacking legs must be ElementarySpace'):
        ab.tensor_from_grid(NP, [[piped]])
    z2 = g[0][0]
    u1 = to_tensor(NP, GRID[GRID_IDS.index('u1-11-3x3')]['grid'][0][0])
    with pytest.raises(ValueError, match='different symmetries'):
        ab.tensor_from_grid(NP, [[z2, u1]])
    with pytest.raises(ValueError, match='labels expected'):
        ab.tensor_from_grid(NP, g, labels=['a'])
    no_domain = ab.AbelianTensor(t.symmetry, t.legs, [], np.zeros((0, 3)), 3)
    with pytest.raises(ValueError, match='at least one codomain and one domain leg'):
        ab.tensor_from_grid(NP, [[no_domain]])


# ------------------------------------------------------------------------------------------- trivial legs

@ALL_OUTER
def test_trivial_legs_round_trip(case):
    t = to_tensor(NP, OUTER[case]['a'])
    t.labels = list('abcdefg')[:t.nlegs]
    K = t.num_codomain
    for pos, to_domain in [(0, False), (K, False), (K, True), (t.nlegs, True)]:
        if (pos > K and not to_domain) or (pos < K and to_domain):
            continue
        u = ab.add_trivial_leg(NP, t, pos, to_domain=to_domain, label='triv')
        assert u.nlegs == t.nlegs + 1 and u.labels[pos] == 'triv' and u.num_codomain == K + (0 if to_domain else 1)
        leg = u.legs[pos]
        assert leg.nsec == 1 and leg.dim == 1 and not leg.sectors.any() and leg.sign == (-1 if to_domain else +1)
        assert _is_sorted(u)
        u.check_charges()
        assert np.array_equal(u.to_dense(NP), np.expand_dims(t.to_dense(NP), pos))
        for back in (ab.squeeze_legs(NP, u), ab.squeeze_legs(NP, u, [pos]), ab.squeeze_legs(NP, u, pos - u.nlegs)):
            assert np.array_equal(back.block_inds, t.block_inds) and back.labels == t.labels and back.num_codomain == K
            assert back.legs == t.legs
            assert all(np.array_equal(x, y) for x, y in zip(back.blocks, t.blocks))


def test_trivial_leg_errors():
    t = to_tensor(NP, OUTER[0]['a'])                     # 1 codomain, 2 domain legs
    with pytest.raises(ValueError, match='not trivial'):
        ab.squeeze_legs(NP, t, [0])
    with pytest.raises(ValueError, match='outside'):
        ab.add_trivial_leg(NP, t, 5)
    with pytest.raises(ValueError, match='does not lie in the codomain'):
        ab.add_trivial_leg(NP, t, 3)
    with pytest.raises(ValueError, match='does not lie in the domain'):
        ab.add_trivial_leg(NP, t, 0, to_domain=True)
    assert ab.squeeze_legs(NP, t).nlegs == t.nlegs       # (nothing to squeeze)


# ------------------------------------------------------------------------------------------- known answers

L_SITES = 6


def check_tfi(bb, J=1.3, g=0.7):
    W, i_left, i_right = ref.tfi_mpo(bb, J, g)
    assert W.labels == ['wL', 'p', 'wR', 'p*'] and W.num_codomain == 2
    W.check_charges()
    assert W.legs[0].can_contract_with(W.legs[2])
    H = ref.mpo_to_matrix(W.to_dense(bb), L_SITES, i_left, i_right)
    want = ref.chain_hamiltonian(L_SITES, [(-J, ref.SX, ref.SX)], [(-g, ref.SZ)]).real
    err = np.abs(H - want).max()
    print(f'TFI MPO, L = {L_SITES}: max |H - H_kron| = {err:.3e} (max |H| = {np.abs(want).max():.3f})')
    assert err <= 1e-12 * np.abs(want).max()


def check_heisenberg(bb, J=0.9):
    W, i_left, i_right, order = ref.heisenberg_mpo(bb, J)
    W.check_charges()
    assert W.legs[0].can_contract_with(W.legs[2]) and W.legs[0].dim == 5
    H = ref.mpo_to_matrix(W.to_dense(bb), L_SITES, i_left, i_right)
    x, y, z = (m[np.ix_(order, order)] for m in (ref.SX, ref.SY, ref.SZ))
    want = ref.chain_hamiltonian(L_SITES, [(J, x, x), (J, y, y), (J, z, z)])
    assert np.abs(want.imag).max() == 0
    err = np.abs(H - want.real).max()
    print(f'Heisenberg MPO, L = {L_SITES}: max |H - H_kron| = {err:.3e} (max |H| = {np.abs(want).max():.3f})')
    assert err <= 1e-12 * np.abs(want).max()


def bond_hamiltonian(bb, J=1.0, gL=0.5, gR=0.25):
    """(-J XX - gL ZI - gR IZ as a tensor [p0, p1, p1*, p0*] built with outer and linear_combination, its np.kron form)"""
    sym = ab.Symmetry([2])
    p = ab.Leg(sym, [[0], [1]], [1, 1], +1)
    I, Z = ref.two_leg_op(bb, sym, p, ref.ID), ref.two_leg_op(bb, sym, p, ref.SZ)
    IZ = ab.outer(bb, I, Z, {'p': 'p0', 'p*': 'p0*'}, {'p': 'p1', 'p*': 'p1*'})
    ZI = ab.outer(bb, Z, I, {'p': 'p0', 'p*': 'p0*'}, {'p': 'p1', 'p*': 'p1*'})
    assert IZ.labels == ['p0', 'p1', 'p1*', 'p0*'] and IZ.num_codomain == 2
    xx = np.kron(ref.SX, ref.SX).reshape(2, 2, 2, 2).transpose(0, 1, 3, 2)       # [p0, p1, p0*, p1*] -> [p0, p1, p1*, p0*]
    XX = ab.from_dense_block(bb, sym, IZ.legs, bb.as_block(np.ascontiguousarray(xx)), 2)
    h = ab.linear_combination(bb, 1.0, ab.linear_combination(bb, -gL, ZI, -gR, IZ), -J, XX)
    want = -J * np.kron(ref.SX, ref.SX) - gL * np.kron(ref.SZ, ref.ID) - gR * np.kron(ref.ID, ref.SZ)
    return h, want


def as_matrix(dense):
    """[p0, p1, p1*, p0*] -> (p0 p1) x (p0* p1*)"""
    return np.transpose(dense, (0, 1, 3, 2)).reshape(4, 4)


def test_tfi_mpo_is_the_kronecker_hamiltonian():
    check_tfi(NP)


def test_heisenberg_mpo_is_the_kronecker_hamiltonian():
    check_heisenberg(NP)


def test_bond_hamiltonian_is_its_kron_form():
    h, want = bond_hamiltonian(NP)
    h.check_charges()
    assert np.array_equal(as_matrix(h.to_dense(NP)), want)


def test_heisenberg_bond_from_outer():
    h, want = ref.heisenberg_bond(NP, 0.9)
    h.check_charges()
    assert h.num_codomain == 2 and h.nlegs == 4
    assert np.array_equal(as_matrix(h.to_dense(NP)), want)
