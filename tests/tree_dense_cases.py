"""Inputs and checks of to_dense_block / from_dense_block on fusion-tree tensors shared by tests/test_tree_dense.py (numpy
stand-in: the record building without a device) and tests/test_gpu_tree_dense.py (HipBlockBackend: the same inputs, the same
criteria).

(1) abelian trees against the dense tensor the blocks were cut from -- the independent check: every d = 1, every X = 1, every
    element has one term with the weight 1, so the comparison is ``==``.
(2) made-up trees with random isometric tables (the columns of a random unitary per uncoupled tuple, dealt out to (coupled
    sector, tree, kc)) against the restatement tests/tree_dense_ref.py.
(3) SU(2) with Clebsch-Gordan tensors from sympy: homomorphism with compose, S.S, a two-tree forest, norm, dagger.
(4) projection and tolerance, (5) structure and errors.

Bound of (2).  Forward, an element is sum_t S_t T_t with P terms; backward it is (sum_k conj(S_k) a_k) / d_c with P = prod d products.
A (complex) product is two real products and a sum per component, each rounded once or fused, the P - 1 additions add one
rounding each, the division one more: the computed value is within (P + 6) u S of the exact one, u = 2^-53, S the same sum on
|.|_1 = |re| + |im| (divided by d_c), componentwise.  The restatement runs in longdouble on the same float64 tables S (they are
inputs of both sides), so its own error is below u S; ``2 (P + 6) u S`` covers both directions, the division included.  P and S
come from the restatement run on ones and on absolute values.  Round trip: the forward error of at most (P_f + 6) u A per
element of the dense tensor (A its absolute-value run) goes through the backward sum, which adds (P_b + 6) u of its own:
(max P_f + P_b + 12) u from_dense(A), and the check allows twice that against the restatement's round trip.

Bound of (3).  Clebsch-Gordan coefficients are rounded once (sympy evaluates the exact radical), relative error u each.  A
dense element of to_dense(a) is a sum of P_a products S T of which S is a product of two coefficients summed over kc; the
contraction of two dense tensors multiplies two such sums over K_c positions.  With every factor within 4 u relative and every
sum adding one rounding per term, both sides of the homomorphism are within (2 (P_a + P_b + K_c) + 32) u of the exact value
times the same expression on absolute values."""
import contextlib
import functools
import itertools

import numpy as np

import tree_dense_ref as ref
from cyten_amd import fusion_tree as ft
from fusion_tree_cases import AbelianTrees
from tree_ops_cases import KeyedAbelianTrees, NumpyTreeBackend, to_dev
from tree_outer_cases import _spin_leg, _two_leg_space

U = 2.0 ** -53
abs1 = ref.abs1


class NumpyDenseBackend(NumpyTreeBackend):
    """the stand-in of the tree operations + looped ``tree_to_dense_many`` / ``tree_from_dense_many``"""

    def norm(self, a, order=2, axis=None):
        return float(np.sqrt(np.sum(np.abs(a) ** 2)))

    def norm_many(self, blocks):
        return float(np.sqrt(sum(np.sum(np.abs(b) ** 2) for b in blocks)))

    def tree_to_dense_many(self, dst_view, regions):
        L = dst_view.ndim
        for starts, dims, mults, J, terms in regions:
            sl = tuple(slice(s, s + d * m) for s, d, m in zip(starts, dims, mults))
            acc = np.zeros([d * m for d, m in zip(dims, mults)], dtype=dst_view.dtype)
            H, W = int(np.prod(mults[:J], dtype=np.int64)), int(np.prod(mults[J:], dtype=np.int64))
            for blk, r0, c0, S in terms:
                assert np.iscomplexobj(dst_view) or not (np.iscomplexobj(blk) or np.iscomplexobj(S))
                assert S.shape == tuple(dims) and r0 + H <= blk.shape[0] and c0 + W <= blk.shape[1]
                T = blk[r0:r0 + H, c0:c0 + W].reshape(mults)
                acc = acc + np.multiply.outer(S, T).transpose([p for l in range(L) for p in (l, L + l)]).reshape(acc.shape)
            dst_view[sl] = acc

    def tree_from_dense_many(self, outputs):
        for dst, div, dims, mults, J, terms in outputs:
            L = len(dims)
            acc = np.zeros(dst.shape, dtype=dst.dtype)
            for a, starts, S in terms:
                assert np.iscomplexobj(dst) or not (np.iscomplexobj(a) or np.iscomplexobj(S))
                reg = a[tuple(slice(s, s + d * m) for s, d, m in zip(starts, dims, mults))]
                reg = reg.reshape([x for d, m in zip(dims, mults) for x in (d, m)]).transpose([2 * l for l in range(L)] + [2 * l + 1 for l in range(L)])
                acc = acc + (np.tensordot(np.conj(S), reg, L) if L else np.conj(S) * reg).reshape(dst.shape)
            dst[...] = acc / div


def host(bb, x):
    return np.asarray(bb.to_numpy(x))


def blocks_of(bb, data):
    return {tuple(r): host(bb, b) for r, b in zip(data.block_inds.tolist(), data.blocks)}


@contextlib.contextmanager
def nan_filled(bb):
    """every block ``empty_many`` hands out is NaN: an element that nobody writes shows"""
    orig = bb.empty_many

    def empty_many(shapes, dtype=None, device=None):
        outs = orig(shapes, dtype=dtype)
        cplx = dtype is not None and np.dtype(dtype).kind == 'c'
        bb.copy_many([(o, bb.as_block(np.full(tuple(sh), complex(np.nan, np.nan) if cplx else np.nan))) for o, sh in zip(outs, shapes)
                      if int(np.prod(sh, dtype=np.int64))])
        return outs

    bb.empty_many = empty_many
    try:
        yield
    finally:
        del bb.empty_many


def within(got, want, P, S, factor=2):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and not np.isnan(got).any()
    bound = factor * (np.asarray(P, dtype=np.float64) + 6) * U * np.asarray(S, dtype=np.float64)
    err_re = np.abs(np.real(got) - np.real(want)).astype(np.float64)
    err_im = np.abs(np.imag(got) - np.imag(want)).astype(np.float64)
    assert np.all(err_re <= bound) and np.all(err_im <= bound), float(np.max(np.maximum(err_re, err_im) / np.maximum(bound, 1e-300)))


# ---------------------------------------------------------------------------------------------------------------------------
# (1) abelian trees

ABELIAN_CONFIGS = [(1, 1, 'drawn'), (2, 2, 'drawn'), (3, 2, 'drawn'), (2, 1, 'ones'), (2, 2, 'odd'), (3, 3, 'drawn')]     # (J, K, multiplicities)


def abelian_dense(at, factors):
    """TreeDense of the product of `factors`: every sector has the dimension 1, every tree tensor is 1"""
    sp = at.space(factors)
    n = len(factors)
    legs = tuple([(int(q), int(m)) for q, m in zip(*at.legs[f])] for f in factors)
    dims = {int(q): 1 for f in factors for q in at.legs[f][0]}
    return sp, ft.TreeDense(legs, dims, {tb.tree: np.ones((1,) * (n + 1)) for tbs in sp.tree_blocks for tb in tbs})


def abelian_case(rng, config, cplx):
    J, K, how = config
    at = KeyedAbelianTrees(rng, J=J, K=K)
    if how == 'ones':           # runs of one element
        at.legs = [(q, np.ones_like(m)) for q, m in at.legs]
    elif how == 'odd':
        at.legs = [(q, 2 * m + 1) for q, m in at.legs]
    T = at.dense(rng, cplx)
    cf, df = list(range(J)), list(range(J, J + K))
    cod, dom, data = at.to_blocks(T, cf, df)
    (cod, cd), (dom, dd) = abelian_dense(at, cf), abelian_dense(at, df)
    dense = np.ascontiguousarray(T.transpose(cf + df[::-1]))
    return dict(at=at, data=data, cod=cod, dom=dom, cd=cd, dd=dd, dense=dense)


def check_abelian(bb, rng, config, cplx):
    c = abelian_case(rng, config, cplx)
    assert len(c['data'].blocks) > 0
    with nan_filled(bb):
        got = host(bb, ft.to_dense_block(bb, to_dev(bb, c['data']), c['cod'], c['dom'], c['cd'], c['dd']))
        back = ft.from_dense_block(bb, bb.as_block(c['dense']), c['cod'], c['dom'], c['cd'], c['dd'])
    assert got.shape == c['dense'].shape and np.iscomplexobj(got) == cplx
    assert np.array_equal(got, c['dense'])
    want = {tuple(r): b for r, b in zip(c['data'].block_inds.tolist(), c['data'].blocks)}
    have = blocks_of(bb, back)
    assert sorted(have) == sorted(want) and [tuple(r) for r in back.block_inds.tolist()] == sorted(want)
    for k, w in want.items():
        assert np.iscomplexobj(have[k]) == cplx and np.array_equal(have[k], w), k
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (2) made-up trees with random isometric tables

SECTOR_DIMS = {'x': 2, 'y': 3}
COUPLED_DIMS = [1, 2, 3]
# uncoupled tuple -> [(coupled sector, number of trees)], sum of d_c * trees = product of the leg dimensions; the coupled
# sector 1 is reached from three tuples, holds a forest of three trees and one of two
DEAL = {('x', 'x'): [(0, 1), (2, 1)], ('x', 'y'): [(1, 3)], ('y', 'x'): [(1, 2), (0, 2)], ('y', 'y'): [(2, 2), (1, 1), (0, 1)]}


def table_side(rng, tag, mults, cplx):
    """a two-leg side: (TreeSpace, TreeDense).  The trees of a coupled sector alternate between the forests, so a forest is
    no contiguous run of rows."""
    trees: dict = {c: [] for c in range(3)}
    tensors = {}
    for u, deal in DEAL.items():
        D = SECTOR_DIMS[u[0]] * SECTOR_DIMS[u[1]]
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)) + (1j * rng.standard_normal((D, D)) if cplx else 0))
        col = 0
        for c, n in deal:
            for t in range(n):
                key = (tag, u, c, t)
                d = COUPLED_DIMS[c]
                tensors[key] = np.ascontiguousarray(Q[:, col:col + d]).reshape(SECTOR_DIMS[u[0]], SECTOR_DIMS[u[1]], d)
                col += d
                trees[c].append((t, key, u))
        assert col == D
    names, tm, unc = [], [], []
    for c in range(3):
        order = sorted(trees[c], key=lambda x: (x[0], x[2]))           # by tree number first: the forests interleave
        names.append([k for _, k, _ in order])
        tm.append([(mults[0][u[0]], mults[1][u[1]]) for _, _, u in order])
        unc.append([u for _, _, u in order])
    space = ft.TreeSpace.from_multiplicities([[0], [1], [2]], tm, np.array([1.0, 2.0, 3.0]), 2, names, unc)
    legs = tuple([(k, mults[l][k]) for k in ('x', 'y')] for l in range(2))
    return space, ft.TreeDense(legs, dict(SECTOR_DIMS), tensors)


def table_case(rng, cplx_data, cplx_tables, present=(0, 1, 2)):
    cod, cd = table_side(rng, 'c', [{'x': 2, 'y': 3}, {'x': 1, 'y': 2}], cplx_tables)
    dom, dd = table_side(rng, 'd', [{'x': 3, 'y': 1}, {'x': 2, 'y': 2}], cplx_tables)
    rows, blocks = [], []
    for s in present:
        sh = (cod.block_size(s), dom.block_size(s))
        rows.append((s, s))
        blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx_data else 0))
    return dict(data=ft.FusionTreeData(rows, blocks), cod=cod, dom=dom, cd=cd, dd=dd)


def _spaces(c):
    return c['cod'], c['dom'], c['cd'], c['dd']


def check_table(bb, rng, cplx_data, cplx_tables):
    c = table_case(rng, cplx_data, cplx_tables)
    sp = _spaces(c)
    assert max(len(f) for f in ft._dense_side(c['cod'], c['cd'], 'codomain', 't')[2][1].values()) == 3
    with nan_filled(bb):
        dense = ft.to_dense_block(bb, to_dev(bb, c['data']), *sp)
    got = host(bb, dense)
    assert np.iscomplexobj(got) == (cplx_data or cplx_tables)
    want, Pf, A = ref.to_dense(c['data'], *sp), ref.to_dense(c['data'], *sp, count=True), ref.to_dense(c['data'], *sp, absolute=True)
    assert Pf.max() >= 6 and (Pf == 0).any()                 # nine tree pairs in one region; combinations nothing fuses to
    within(got, want, Pf, A)
    # backward, from an unrelated dense tensor (not symmetric: tol = 0)
    a = rng.standard_normal(got.shape) + (1j * rng.standard_normal(got.shape) if cplx_data else 0)
    with nan_filled(bb):
        proj = ft.from_dense_block(bb, bb.as_block(a), *sp, tol=0.0)
    have, wb = blocks_of(bb, proj), ref.from_dense(a, *sp)
    Pb, Sb = ref.from_dense(a, *sp, count=True), ref.from_dense(a, *sp, absolute=True)
    assert sorted(have) == sorted(wb) == [(0, 0), (1, 1), (2, 2)]
    for k in wb:
        assert np.iscomplexobj(have[k]) == (cplx_data or cplx_tables)
        within(have[k], wb[k], Pb[k], Sb[k])
    # round trip
    back = blocks_of(bb, ft.from_dense_block(bb, dense, *sp))
    chain, SA = ref.from_dense(want, *sp), ref.from_dense(A, *sp, absolute=True)
    for (k, w), blk in zip(chain.items(), c['data'].blocks):
        within(back[k], w, float(Pf.max()) + Pb[k] + 6, SA[k])
        assert np.abs(back[k] - blk).max() <= 1e-13 * np.abs(blk).max()          # the tables are isometric to rounding
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (3) SU(2); sectors are 2 j, the index i of a sector counts m = -j + i

@functools.lru_cache(maxsize=None)
def cg(a2, ma2, b2, mb2, c2, mc2):
    from sympy import Rational
    from sympy.physics.quantum.cg import CG
    return float(CG(Rational(a2, 2), Rational(ma2, 2), Rational(b2, 2), Rational(mb2, 2), Rational(c2, 2), Rational(mc2, 2)).doit())


def cg_tensor(a2, b2, c2):
    """X[ma, mb, mc] = <ja ma jb mb | jc mc>"""
    X = np.zeros((a2 + 1, b2 + 1, c2 + 1))
    for ia, ib, ic in itertools.product(range(a2 + 1), range(b2 + 1), range(c2 + 1)):
        if (-a2 + 2 * ia) + (-b2 + 2 * ib) == -c2 + 2 * ic:
            X[ia, ib, ic] = cg(a2, -a2 + 2 * ia, b2, -b2 + 2 * ib, c2, -c2 + 2 * ic)
    return X


def _leg_list(sp: ft.TreeSpace):
    return [(j, tbs[0].multiplicities[0]) for (j,), tbs in zip(sp.sectors.tolist(), sp.tree_blocks)]


def one_leg_dense(sp: ft.TreeSpace):
    return ft.TreeDense((_leg_list(sp),), {j: j + 1 for (j,) in sp.sectors.tolist()}, {tbs[0].tree: np.eye(j + 1) for (j,), tbs in zip(sp.sectors.tolist(), sp.tree_blocks)})


def two_leg_dense(tag, left: ft.TreeSpace, right: ft.TreeSpace, both: ft.TreeSpace):
    dims = {j: j + 1 for sp in (left, right) for (j,) in sp.sectors.tolist()}
    return ft.TreeDense((_leg_list(left), _leg_list(right)), dims, {tb.tree: cg_tensor(*tb.tree[1:]) for tbs in both.tree_blocks for tb in tbs})


def random_data(rng, cod, dom, cplx, skip=()):
    rows, blocks = [], []
    for i, j in ft.common_sectors(cod, dom):
        if (i, j) in skip:
            continue
        sh = (cod.block_size(i), dom.block_size(j))
        rows.append((i, j))
        blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0))
    return ft.FusionTreeData(rows, blocks)


def su2_pair(tag, mults_l, mults_r):
    left, right = _spin_leg(tag + 'l', mults_l), _spin_leg(tag + 'r', mults_r)
    both = _two_leg_space(tag, left, right)
    return both, two_leg_dense(tag, left, right, both)


def check_su2_homomorphism(bb, rng, cplx):
    """to_dense(compose(a, b)) == tensordot(to_dense(a), to_dense(b)) over axis J + K - 1 - k of a and axis k of b; with the norm
    and the dagger of the operands"""
    X, xd = su2_pair('x', {0: 2, 1: 1, 2: 1}, {0: 1, 1: 2, 2: 1})
    Y, yd = su2_pair('y', {0: 1, 1: 2}, {1: 1, 2: 2})
    Z, zd = su2_pair('z', {0: 1, 2: 2}, {0: 2, 1: 1})
    a, b = random_data(rng, X, Y, cplx), random_data(rng, Y, Z, cplx)
    da, db = to_dev(bb, a), to_dev(bb, b)
    Da, Db = host(bb, ft.to_dense_block(bb, da, X, Y, xd, yd)), host(bb, ft.to_dense_block(bb, db, Y, Z, yd, zd))
    Dab = host(bb, ft.to_dense_block(bb, ft.compose(bb, da, db), X, Z, xd, zd))
    assert np.iscomplexobj(Dab) == cplx and Dab.shape == Da.shape[:2] + Db.shape[2:]
    Aa, Ab = ref.to_dense(a, X, Y, xd, yd, absolute=True), ref.to_dense(b, Y, Z, yd, zd, absolute=True)
    Pa, Pb = ref.to_dense(a, X, Y, xd, yd, count=True).max(), ref.to_dense(b, Y, Z, yd, zd, count=True).max()
    Kc = Da.shape[2] * Da.shape[3]
    bound = (2 * float(Pa + Pb + Kc) + 32) * U * np.tensordot(Aa, Ab, ([3, 2], [0, 1])).astype(np.float64)
    err = Dab - np.tensordot(Da, Db, ([3, 2], [0, 1]))
    assert np.all(np.abs(err.real) <= bound) and np.all(np.abs(err.imag) <= bound)
    assert np.abs(Dab).max() > 0.1
    # |to_dense(t)|_F^2 = norm(t)^2 (the quantum dimensions weight the blocks)
    for t, cod, D in ((da, X, Da), (db, Y, Db)):
        n2 = ft.norm(bb, t, cod) ** 2
        assert abs(np.sum(np.abs(D) ** 2) - n2) <= 1e-13 * n2
    # to_dense(dagger(t)) is the conjugate transpose
    Dd = host(bb, ft.to_dense_block(bb, ft.dagger(bb, da), Y, X, yd, xd))
    within(Dd, np.conj(Da).transpose(3, 2, 1, 0), ref.to_dense(a, X, Y, xd, yd, count=True).transpose(3, 2, 1, 0), Aa.transpose(3, 2, 1, 0))
    within(Da, ref.to_dense(a, X, Y, xd, yd), ref.to_dense(a, X, Y, xd, yd, count=True), Aa)


def spin_half_pair(m=1):
    return su2_pair('s', {1: m}, {1: m})


def heisenberg():
    """S.S on two spins 1/2 as the block (s1, s2, s2', s1')"""
    sz, sp = np.diag([-0.5, 0.5]), np.array([[0.0, 0.0], [1.0, 0.0]])          # index 0: m = -1/2; S+ raises it
    ss = np.kron(sz, sz) + 0.5 * (np.kron(sp, sp.T) + np.kron(sp.T, sp))
    return np.ascontiguousarray(ss.reshape(2, 2, 2, 2).transpose(0, 1, 3, 2)), np.ascontiguousarray(np.kron(sz, np.eye(2)).reshape(2, 2, 2, 2).transpose(0, 1, 3, 2))


def check_su2_heisenberg(bb):
    """from_dense_block of S.S: the 1 x 1 blocks -3/4 (J = 0) and +1/4 (J = 1).  Every block entry is a sum of 16 products of
    four coefficients of magnitude <= 1, each within u: 64 u is generous."""
    W, wd = spin_half_pair()
    ss, _ = heisenberg()
    got = blocks_of(bb, ft.from_dense_block(bb, bb.as_block(ss), W, W, wd, wd))
    assert sorted(got) == [(0, 0), (1, 1)] and W.sectors.tolist() == [[0], [2]]
    assert got[(0, 0)].shape == (1, 1) and abs(got[(0, 0)][0, 0] + 0.75) <= 64 * U and abs(got[(1, 1)][0, 0] - 0.25) <= 64 * U
    back = host(bb, ft.to_dense_block(bb, ft.from_dense_block(bb, bb.as_block(ss), W, W, wd, wd), W, W, wd, wd))
    assert np.abs(back - ss).max() <= 64 * U


def three_spin_side(m):
    """three spins 1/2 with the multiplicities m: trees ((1/2, 1/2) -> e, 1/2 -> J); J = 1/2 holds the forest e = 0, e = 1"""
    trees = {1: [0, 2], 3: [2]}
    names = [[('t', e, J) for e in trees[J]] for J in (1, 3)]
    sp = ft.TreeSpace.from_multiplicities([[1], [3]], [[tuple(m)] * len(trees[J]) for J in (1, 3)], np.array([2.0, 4.0]), 3, names,
                                          [[(1, 1, 1)] * len(trees[J]) for J in (1, 3)])
    tensors = {('t', e, J): np.einsum('abe,ecj->abcj', cg_tensor(1, 1, e), cg_tensor(e, 1, J)) for J in (1, 3) for e in trees[J]}
    return sp, ft.TreeDense(tuple([(1, mm)] for mm in m), {1: 2}, tensors)


def check_su2_three_spins(bb, rng, cplx):
    cod, cd = three_spin_side((2, 1, 3))
    dom = _spin_leg('o', {1: 3, 3: 2})
    dd = one_leg_dense(dom)
    t = random_data(rng, cod, dom, cplx)
    sp = (cod, dom, cd, dd)
    assert [len(x) for x in cod.tree_blocks] == [2, 1]
    with nan_filled(bb):
        dense = ft.to_dense_block(bb, to_dev(bb, t), *sp)
    D = host(bb, dense)
    P, A = ref.to_dense(t, *sp, count=True), ref.to_dense(t, *sp, absolute=True)
    assert P.max() == 2                                   # the two trees of J = 1/2 feed the same region
    within(D, ref.to_dense(t, *sp), P, A)
    n2 = ft.norm(bb, to_dev(bb, t), cod) ** 2
    assert abs(np.sum(np.abs(D) ** 2) - n2) <= 1e-13 * n2
    back = blocks_of(bb, ft.from_dense_block(bb, dense, *sp))
    for r, blk in zip(t.block_inds.tolist(), t.blocks):
        assert np.abs(back[tuple(r)] - blk).max() <= 1e-13 * np.abs(blk).max()


# ---------------------------------------------------------------------------------------------------------------------------
# (4) projection and tolerance

def check_projection(bb):
    import pytest
    W, wd = spin_half_pair()
    ss, sz1 = heisenberg()
    with pytest.raises(ValueError, match='not symmetric up to tolerance'):
        ft.from_dense_block(bb, bb.as_block(sz1), W, W, wd, wd)
    for a in (sz1, ss + sz1):
        with pytest.raises(ValueError, match='not symmetric up to tolerance'):
            ft.from_dense_block(bb, bb.as_block(a), W, W, wd, wd)
        p = ft.from_dense_block(bb, bb.as_block(a), W, W, wd, wd, tol=0.0, discard=False)
        D = host(bb, ft.to_dense_block(bb, p, W, W, wd, wd))
        assert abs(np.sum(D * (a - D))) <= 64 * U            # the projection is orthogonal to the remainder
        want = {(0, 0): 0.0, (1, 1): 0.0} if a is sz1 else {(0, 0): -0.75, (1, 1): 0.25}
        got = blocks_of(bb, p)
        assert sorted(got) == sorted(want) and all(abs(got[k][0, 0] - v) <= 64 * U for k, v in want.items())
    # a symmetric block passes the default tolerance
    assert len(ft.from_dense_block(bb, bb.as_block(ss), W, W, wd, wd).blocks) == 2


# ---------------------------------------------------------------------------------------------------------------------------
# (5) structure and errors

def check_absent_block_and_discard(bb, rng):
    c = table_case(rng, False, False, present=(0, 2))
    sp = _spaces(c)
    with nan_filled(bb):
        D = host(bb, ft.to_dense_block(bb, to_dev(bb, c['data']), *sp))
    assert not np.isnan(D).any()
    want, P = ref.to_dense(c['data'], *sp), ref.to_dense(c['data'], *sp, count=True)
    within(D, want, P, ref.to_dense(c['data'], *sp, absolute=True))
    assert (P == 0).any() and np.all(D[P == 0] == 0)          # regions only the absent block feeds are zeros, and written
    kept = ft.from_dense_block(bb, bb.as_block(D), *sp)
    every = ft.from_dense_block(bb, bb.as_block(D), *sp, discard=False)
    assert kept.block_inds.tolist() == [[0, 0], [2, 2]] and every.block_inds.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert np.abs(host(bb, every.blocks[1])).max() <= 1e-14
    zero = ft.from_dense_block(bb, bb.as_block(np.zeros(D.shape)), *sp)
    assert len(zero.blocks) == 0 and zero.block_inds.shape == (0, 2)
    assert len(ft.from_dense_block(bb, bb.as_block(np.zeros(D.shape)), *sp, discard=False).blocks) == 3


def check_empty_domain(bb, rng, cplx):
    """K = 0: the domain is the space without legs (the trivial coupled sector, one tree, block size 1)"""
    cod, cd = spin_half_pair(2)
    dom = ft.TreeSpace.from_multiplicities([[0]], [[()]], np.array([1.0]), 0, [['e']], [[()]])
    dd = ft.TreeDense((), {}, {'e': np.ones(1)})
    sh = (cod.block_size(0), 1)
    t = ft.FusionTreeData([(0, 0)], [rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0)])
    sp = (cod, dom, cd, dd)
    dense = ft.to_dense_block(bb, to_dev(bb, t), *sp)
    D = host(bb, dense)
    assert D.shape == (4, 4)
    within(D, ref.to_dense(t, *sp), 1, ref.to_dense(t, *sp, absolute=True))
    psi = D.reshape(2, 2, 2, 2)                                # (k1, m1, k2, m2): a singlet in k for every (m1, m2)
    assert np.abs(psi + psi.transpose(2, 1, 0, 3)).max() <= 8 * U * np.abs(D).max() and np.abs(D).max() > 0
    back = blocks_of(bb, ft.from_dense_block(bb, dense, *sp))
    assert sorted(back) == [(0, 0)] and np.abs(back[(0, 0)] - t.blocks[0]).max() <= 64 * U * np.abs(t.blocks[0]).max()


def check_seven_legs_raise(bb, rng):
    import pytest
    at = KeyedAbelianTrees(rng, J=4, K=3)
    cf, df = list(range(4)), list(range(4, 7))
    (cod, cd), (dom, dd) = abelian_dense(at, cf), abelian_dense(at, df)
    with pytest.raises(ValueError, match='at most 6'):
        ft.to_dense_block(bb, ft.FusionTreeData(np.zeros((0, 2), np.int64), []), cod, dom, cd, dd)
    with pytest.raises(ValueError, match='at most 6'):
        ft.from_dense_block(bb, bb.as_block(np.zeros((1,) * 7)), cod, dom, cd, dd)


def check_errors(bb, rng):
    import pytest
    c = abelian_case(rng, (2, 2, 'drawn'), False)
    at, data, cod, dom, cd, dd = c['at'], to_dev(bb, c['data']), c['cod'], c['dom'], c['cd'], c['dd']
    dense = bb.as_block(c['dense'])

    def both(match, cod_=cod, dom_=dom, cd_=cd, dd_=dd):
        with pytest.raises(ValueError, match=match):
            ft.to_dense_block(bb, data, cod_, dom_, cd_, dd_)
        with pytest.raises(ValueError, match=match):
            ft.from_dense_block(bb, dense, cod_, dom_, cd_, dd_)

    both('lacks the uncoupled', cod_=AbelianTrees.space(at, [0, 1]))                        # a tree without `uncoupled`
    some = cod.tree_blocks[0][0].tree
    both('no tensor for the tree', cd_=cd._replace(tensors={k: v for k, v in cd.tensors.items() if k != some}))
    both('has the shape', dd_=dd._replace(tensors={**dd.tensors, dom.tree_blocks[0][0].tree: np.ones((1, 2, 1))}))
    both('has the shape', dd_=dd._replace(tensors={**dd.tensors, dom.tree_blocks[0][0].tree: np.ones((1, 1))}))
    legs = list(cd.legs)
    legs[1] = [(q, m + 1) for q, m in legs[1]]
    both('multiplicity', cd_=cd._replace(legs=tuple(legs)))
    both('flat legs', cd_=cd._replace(legs=cd.legs[:1]))
    shape = list(c['dense'].shape)
    shape[2] += 1
    with pytest.raises(ValueError, match='dense block of shape'):
        ft.from_dense_block(bb, bb.as_block(np.zeros(shape)), cod, dom, cd, dd)
    with pytest.raises(ValueError, match='dense block of shape'):
        ft.from_dense_block(bb, bb.as_block(np.zeros(shape[:3])), cod, dom, cd, dd)
