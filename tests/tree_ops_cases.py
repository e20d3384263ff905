"""Inputs and checks of the fusion-tree tensor operations shared by tests/test_tree_ops.py (numpy stand-in: the record
building without a device) and tests/test_gpu_tree_ops.py (HipBlockBackend: the same inputs, the same criteria)."""
import copy

import numpy as np

import tree_ops_ref as ref
from cyten_amd import fusion_tree as ft
from fusion_tree_cases import AbelianTrees
from numpy_backend import NumpyGroupedBackend


class NumpyTreeBackend(NumpyGroupedBackend):
    """numpy stand-in + the calls the tree operations add; ``tree_axis_many`` and ``inner_weighted_many`` loop over the
    records.  ``empty_many`` hands out NaN so that a result element nobody writes or zero-fills shows."""
    TRUNCATE_MAX = 0

    def as_block(self, a, dtype=None, device=None):
        return np.array(a)

    def empty_many(self, shapes, dtype=None, device=None):
        return [np.full(sh, np.nan, dtype=dtype or float) for sh in shapes]

    def max_abs(self, a):
        return float(np.abs(a).max(initial=0.0))

    def copy_many(self, pairs, conj=False):
        for d, s in pairs:
            d[...] = np.conj(s) if conj else s

    def allclose(self, a, b, rtol=1e-5, atol=1e-8):
        return bool(np.abs(a - b).max(initial=0.0) <= atol + rtol * np.abs(b).max(initial=0.0))

    def tree_axis_many(self, records, mode, fill=()):
        for b in fill:
            b[...] = 0
        for r in records:
            vs = (r.src if r.side == 0 else r.src.T) if r.src.ndim == 2 else r.src[:, None]
            vd = (r.dst if r.side == 0 else r.dst.T) if r.dst.ndim == 2 else r.dst[:, None]
            Ai = r.A_dst if mode == 'gather' else r.A
            o, a, i = [x.ravel() for x in np.meshgrid(np.arange(r.outer), np.arange(Ai), np.arange(r.inner), indexing='ij')]
            if mode == 'scale':
                assert r.A == r.A_dst and len(r.table) == r.A
                ts = td = (o * r.A + a) * r.inner + i
                vd[r.dst_start + td, :] = vs[r.src_start + ts, :] * np.asarray(r.table)[a][:, None]
                continue
            idx = np.asarray(r.table)
            assert len(idx) == Ai and r.A_dst <= r.A if mode == 'gather' else r.A <= r.A_dst
            ts = (o * r.A + (idx[a] if mode == 'gather' else a)) * r.inner + i
            td = (o * r.A_dst + (a if mode == 'gather' else idx[a])) * r.inner + i
            vd[r.dst_start + td, :] = vs[r.src_start + ts, :]

    def inner_weighted_many(self, a_blocks, b_blocks, weights, do_dagger=False):
        if b_blocks is None:
            return float(sum(w * np.sum(np.abs(x) ** 2) for x, w in zip(a_blocks, weights)))
        if do_dagger:
            return sum(w * np.sum(np.conj(x) * y) for x, y, w in zip(a_blocks, b_blocks, weights))
        return sum(w * np.sum(x * y.T) for x, y, w in zip(a_blocks, b_blocks, weights))

    def trace_weighted_many(self, blocks, weights):
        return sum(w * np.trace(b) for b, w in zip(blocks, weights))


# a v + b w on complex data: four products and three sums per component, each rounded once or fused with its neighbour --
# results of different contraction agree to 8 roundings of terms no larger than the largest entry of the result's inputs
LINCOMB_TOL = 8 * 2.0 ** -52


def to_dev(bb, data):
    return ft.FusionTreeData(data.block_inds, [bb.as_block(b) for b in data.blocks])


def to_host(bb, data):
    return {tuple(r): np.asarray(bb.to_numpy(b)) for r, b in zip(data.block_inds.tolist(), data.blocks)}


def assert_same(got: dict, want: dict, tol=None):
    """the same coupled sectors and the same blocks: bit-exact (value equality), or to `tol` times the largest entry"""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape
        if tol is None:
            assert np.array_equal(g, w), k
        else:
            assert np.abs(g - w).max(initial=0.0) <= tol * max(1.0, np.abs(w).max(initial=0.0)), k


# ---------------------------------------------------------------------------------------------------------------------------
# case 1: abelian trees against the dense tensor

class KeyedAbelianTrees(AbelianTrees):
    """AbelianTrees whose spaces carry the charge of every leg as the ``uncoupled`` key"""

    def space(self, factors):
        sp = super().space(factors)
        blocks = [[ft.TreeBlock(tb.tree, tb.start, tb.stop, tb.multiplicities,
                                tuple(int(self.legs[f][0][k]) for f, k in zip(tb.tree[0], tb.tree[1]))) for tb in tbs]
                  for tbs in sp.tree_blocks]
        return ft.TreeSpace(sp.sectors, sp.qdims, blocks, sp.num_legs)

    def leg_number(self, axis):
        """leg number (as in transform_tensor) of dense axis `axis`"""
        return axis if axis < self.J else (self.J + self.K - 1) - (axis - self.J)


def _as_dict(data):
    return {tuple(r): b for r, b in zip(data.block_inds.tolist(), data.blocks)}


def check_abelian_scale_axis(bb, rng, cplx, cplx_diag=False, tol=None):
    at = KeyedAbelianTrees(rng, J=3, K=2)
    T = at.dense(rng, cplx)
    cf, df = list(range(at.J)), list(range(at.J, at.J + at.K))
    cod, dom, data = at.to_blocks(T, cf, df)
    dev = to_dev(bb, data)
    for axis in range(at.J + at.K):
        q, m = at.legs[axis]
        diag_space = at.space([axis])
        present = [k for k in range(len(q)) if not (axis % 2 == 1 and k == 0)]      # odd axes: the first charge has no block
        vals = [rng.standard_normal(int(m[k])) + (1j * rng.standard_normal(int(m[k])) if cplx_diag else 0) for k in range(len(q))]
        d = np.concatenate([vals[k] if k in present else np.zeros(int(m[k])) for k in range(len(q))])
        shape = [1] * T.ndim
        shape[axis] = len(d)
        _, _, want = at.to_blocks(T * d.reshape(shape), cf, df)
        diag = ft.FusionTreeData([(k, k) for k in present], [bb.as_block(vals[k]) for k in present])
        got = ft.scale_axis(bb, dev, cod, dom, diag, diag_space, at.leg_number(axis))
        assert len(want.blocks) > 0
        assert_same(to_host(bb, got), _as_dict(want), tol)


def check_abelian_mask_contract(bb, rng, cplx):
    at = KeyedAbelianTrees(rng, J=3, K=2)
    T = at.dense(rng, cplx)
    cf, df = list(range(at.J)), list(range(at.J, at.J + at.K))
    cod, dom, data = at.to_blocks(T, cf, df)
    dev = to_dev(bb, data)
    for axis in range(at.J + at.K):
        q, m = at.legs[axis]
        keep = []
        for k in range(len(q)):     # nothing of the first charge, everything of the last, a random choice of the others
            keep.append(np.zeros(int(m[k]), bool) if k == 0 else (np.ones(int(m[k]), bool) if k == len(q) - 1 else rng.random(int(m[k])) < 0.5))
        mask = ft.TreeMask([int(c) for c in q], [int(x) for x in m], [np.flatnonzero(x) if x.any() else None for x in keep])
        flat = np.concatenate(keep)
        small = copy.copy(at)
        small.legs = list(at.legs)
        small.legs[axis] = (q[[x.any() for x in keep]], np.array([int(x.sum()) for x in keep if x.any()]))
        ncod, ndom, want = small.to_blocks(np.compress(flat, T, axis=axis), cf, df)
        got, gcod, gdom = ft.mask_contract(bb, dev, cod, dom, mask, at.leg_number(axis), True)
        for g, w in ((gcod, ncod), (gdom, ndom)):       # the derived space: same sectors, same trees in the same order
            assert np.array_equal(g.sectors, w.sectors)
            assert [[tb.multiplicities for tb in tbs] for tbs in g.tree_blocks] == [[tb.multiplicities for tb in tbs] for tbs in w.tree_blocks]
        assert len(want.blocks) > 0
        assert_same(to_host(bb, got), _as_dict(want))
        # large_leg=False: the inverse on the kept positions, zero elsewhere
        side_target = dom if axis >= at.J else cod
        back, bcod, bdom = ft.mask_contract(bb, got, gcod, gdom, mask, at.leg_number(axis), False, target=side_target)
        shape = [1] * T.ndim
        shape[axis] = len(flat)
        _, _, want_back = at.to_blocks(T * flat.reshape(shape), cf, df)
        assert (bdom if axis >= at.J else bcod) is side_target
        assert_same(to_host(bb, back), _as_dict(want_back))


# ---------------------------------------------------------------------------------------------------------------------------
# case 2: a forest with several trees, shaped like 1/2 x 1/2 x 1/2 -> 1/2 (sector keys are 2 j)

def forest_spaces():
    """(three-leg space, one-leg space).  Coupled sector 1 holds three trees, two of them with the uncoupled sectors
    (1, 1, 1) (they differ in the intermediate sector); multiplicities (2, 3, 2) and (1, 3, 2); qdims 1, 2, 3."""
    forest = ft.TreeSpace.from_multiplicities(
        [[0], [1], [3]], [[(1, 3, 2)], [(2, 3, 2), (1, 3, 2), (2, 3, 2)], [(2, 3, 2)]], np.array([1.0, 2.0, 3.0]), 3,
        [[('t', 0, 1, 1, 'via 1', 'to 0')], [('t', 1, 1, 1, 'via 0', 'to 1'), ('t', 0, 1, 1, 'via 1', 'to 1'), ('t', 1, 1, 1, 'via 2', 'to 1')],
         [('t', 1, 1, 1, 'via 2', 'to 3')]],
        [[(0, 1, 1)], [(1, 1, 1), (0, 1, 1), (1, 1, 1)], [(1, 1, 1)]])
    leg = ft.TreeSpace.from_multiplicities([[0], [1], [3]], [[(5,)], [(7,)], [(3,)]], np.array([1.0, 2.0, 3.0]), 1,
                                           [[('l', 0)], [('l', 1)], [('l', 3)]], [[(0,)], [(1,)], [(3,)]])
    return forest, leg


def forest_data(rng, side, cplx):
    """blocks in the coupled sectors 0, 1 and 3; the forest is the codomain (side 0) or the domain (side 1).  Sector 0 holds
    one tree, with bond sector 0: scaled by a diagonal without that sector its block is absent from the result, and a mask that
    keeps nothing of it drops the coupled sector"""
    forest, leg = forest_spaces()
    rows, blocks = [], []
    for s in (0, 1, 2):
        sh = (forest.block_size(s), leg.block_size(s))
        b = rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0)
        rows.append((s, s))
        blocks.append(b if side == 0 else np.ascontiguousarray(b.T))
    return forest, leg, ft.FusionTreeData(rows, blocks)


def check_forest(bb, rng, side, cplx):
    forest, leg, data = forest_data(rng, side, cplx)
    cod, dom = (forest, leg) if side == 0 else (leg, forest)
    dev = to_dev(bb, data)
    mults = [{0: 1, 1: 2}, {1: 3}, {1: 2}]           # multiplicity of every sector of the three legs of the forest
    for idx in range(3):
        number = idx if side == 0 else (1 + 3 - 1) - idx
        # scale: leg 0 has factors for sector 1 only (the trees with sector 0 there give zeros)
        fac = {k: rng.standard_normal(m) for k, m in mults[idx].items() if not (idx == 0 and k == 0)}
        keys = sorted(mults[idx])
        dspace = ft.TreeSpace.from_multiplicities([[k] for k in keys], [[(mults[idx][k],)] for k in keys], None, 1, None, [[(k,)] for k in keys])
        diag = ft.FusionTreeData([(n, n) for n, k in enumerate(keys) if k in fac], [bb.as_block(fac[k]) for k in keys if k in fac])
        got = ft.scale_axis(bb, dev, cod, dom, diag, dspace, number)
        assert_same(to_host(bb, got), ref.scale_axis(data, forest, side, idx, fac))
        # the coupled block of sector 0 has one tree, with sector 0 on leg 0: no factors there, no block in the result
        assert ((0, 0) in to_host(bb, got)) == (idx != 0) and len(got.blocks) == (2 if idx == 0 else 3)
        # gather, then scatter back
        keep = {k: np.sort(rng.choice(m, size=max(1, m - 1), replace=False)) for k, m in mults[idx].items()}
        if idx == 0:
            keep[0] = None                            # nothing kept of sector 0: its trees go, and with them coupled sector 0
        mask = ft.TreeMask(keys, [mults[idx][k] for k in keys], [keep[k] for k in keys])
        small, scod, sdom = ft.mask_contract(bb, dev, cod, dom, mask, number, True)
        new_forest = sdom if side else scod
        assert (scod if side else sdom) is leg
        if idx == 0:
            assert new_forest.sectors.tolist() == [[1], [3]] and [len(t) for t in new_forest.tree_blocks] == [2, 1]
        kept = {k: v for k, v in keep.items() if v is not None}
        want_small = ref.mask_contract(data, forest, new_forest, leg, side, idx, kept, True)
        assert_same(to_host(bb, small), want_small)
        back, _, _ = ft.mask_contract(bb, small, scod, sdom, mask, number, False, target=forest)
        small_host = ft.FusionTreeData(small.block_inds, [np.asarray(bb.to_numpy(b)) for b in small.blocks])
        assert_same(to_host(bb, back), ref.mask_contract(small_host, new_forest, forest, leg, side, idx, kept, False))


# ---------------------------------------------------------------------------------------------------------------------------
# case 3: vector-space operations

def vector_inputs(rng, cplx):
    """v and w on (forest, forest) with different block sets, and u on (forest, leg)"""
    forest, leg = forest_spaces()

    def rand(rows, cod, dom, c):
        blocks = []
        for i, j in rows:
            sh = (cod.block_size(i), dom.block_size(j))
            blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if c else 0))
        return ft.FusionTreeData(rows, blocks)

    v = rand([(0, 0), (1, 1)], forest, forest, cplx)
    w = rand([(1, 1), (2, 2)], forest, forest, False)
    u = rand([(0, 0), (2, 2)], forest, leg, cplx)
    x = rand([(0, 0), (1, 1), (2, 2)], forest, leg, cplx)
    return forest, leg, v, w, u, x


def check_vector_ops(bb, rng, cplx):
    forest, leg, v, w, u, x = vector_inputs(rng, cplx)
    q = forest.qdims
    dv, dw, du, dx = (to_dev(bb, t) for t in (v, w, u, x))

    def close(got, want, tol=1e-13):
        assert abs(complex(got) - complex(want)) <= tol * max(1.0, abs(want)), (got, want)

    close(ft.norm(bb, dv, forest), ref.norm(v, q))
    close(ft.norm(bb, dx, forest), ref.norm(x, q))
    n2 = ft.inner(bb, dx, dx, forest, do_dagger=True)
    assert abs(n2 - ft.norm(bb, dx, forest) ** 2) <= 1e-14 * abs(n2) and abs(complex(n2).imag) <= 1e-14 * abs(n2)
    close(ft.inner(bb, dv, dw, forest, do_dagger=True), ref.inner(v, w, q, True))
    close(ft.inner(bb, du, dx, forest, do_dagger=True), ref.inner(u, x, q, True))
    # do_dagger=False: trace(a b) with b on (leg, forest); against the dagger built explicitly
    xd = ft.dagger(bb, dx)
    assert_same(to_host(bb, xd), ref.dagger(x))
    close(ft.inner(bb, du, xd, forest, do_dagger=False), ref.inner(u, ft.FusionTreeData(*zip(*sorted(ref.dagger(x).items()))), q, False))
    close(ft.inner(bb, du, xd, forest, do_dagger=False), ft.inner(bb, dx, du, forest, do_dagger=True))      # trace(u x^dagger) = <x|u>
    close(ft.trace_full(bb, dv, forest), ref.trace_full(v, q))
    a, b = (0.75 - 0.5j, -1.25) if cplx else (0.75, -1.25)
    assert_same(to_host(bb, ft.linear_combination(bb, a, dv, b, dw)), ref.linear_combination(a, v, b, w), tol=LINCOMB_TOL)
    assert_same(to_host(bb, ft.mul(bb, a, dv)), {tuple(r): a * blk for r, blk in zip(v.block_inds.tolist(), v.blocks)}, tol=LINCOMB_TOL)
    zero = ft.mul(bb, 0.0, dv)
    assert len(zero.blocks) == 0 and zero.block_inds.shape == (0, 2)
    # almost_equal: a perturbation below / above the tolerance, and a block only one of them holds
    near = ft.FusionTreeData(v.block_inds, [blk + 1e-12 for blk in v.blocks])
    far = ft.FusionTreeData(v.block_inds, [blk + 1e-3 for blk in v.blocks])
    assert ft.almost_equal(bb, dv, to_dev(bb, near)) and not ft.almost_equal(bb, dv, to_dev(bb, far))
    tiny = ft.FusionTreeData(np.vstack([v.block_inds, [[2, 2]]]), v.blocks + [np.full((forest.block_size(2),) * 2, 1e-10)])
    assert ft.almost_equal(bb, dv, to_dev(bb, tiny)) and ft.almost_equal(bb, to_dev(bb, tiny), dv)
    assert not ft.almost_equal(bb, dv, dw)


# ---------------------------------------------------------------------------------------------------------------------------
# case 4: truncated SVD

def check_truncated_svd(bb, rng, cplx):
    forest, leg = forest_spaces()
    wide = ft.TreeSpace.from_multiplicities([[0], [1], [3], [5]], [[(9,)], [(11,)], [(8,)], [(4,)]], np.array([1.0, 2.0, 3.0, 4.0]), 1,
                                            None, [[(0,)], [(1,)], [(3,)], [(5,)]])
    rows, blocks = [], []
    for s in (0, 1):                                   # no block in coupled sector 3: its U and Vh come from the identity
        sh = (forest.block_size(s), wide.block_size(s))
        rows.append((s, s))
        blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0))
    t = ft.FusionTreeData(rows, blocks)
    dt = to_dev(bb, t)
    opts = dict(chi_max=9, trunc_cut=1e-3)
    # the untruncated factors, handed to truncated_svd so that both see the same decomposition
    U0, S0, Vh0 = ft.svd(bb, dt, forest, wide)
    U, S, Vh, new_leg, err, new_norm = ft.truncated_svd(bb, dt, forest, wide, factors=(U0, S0, Vh0), **opts)
    U1, S1, Vh1, leg1, err1, norm1 = ft.truncated_svd(bb, dt, forest, wide, **opts)         # ... and decomposing itself
    assert leg1.multiplicities.tolist() == new_leg.multiplicities.tolist() and abs(err1 - err) <= 1e-12 and abs(norm1 - new_norm) <= 1e-12 * new_norm
    for x, y in zip(S1.blocks, S.blocks):
        assert np.abs(np.asarray(bb.to_numpy(x)) - np.asarray(bb.to_numpy(y))).max(initial=0.0) <= 1e-12
    common = ft.common_sectors(forest, wide)
    sec = forest.sectors[[i for i, _ in common]]
    mid = ft.TreeSpace.from_multiplicities(sec, [[(min(forest.block_size(i), wide.block_size(j)),)] for i, j in common],
                                           forest.qdims[[i for i, _ in common]], 1)
    mb, mi, err0, norm0 = ft.truncate_singular_values(bb, S0, mid, **opts)
    assert err == err0 and new_norm == norm0 and 0 < sum(int(m.sum()) for m in mb) <= 9
    kept = {int(j): m for m, (_, j) in zip(mb, mi.tolist())}
    assert new_leg.sectors.tolist() == [sec[j].tolist() for j in sorted(kept)]
    assert new_leg.multiplicities.tolist() == [int(kept[j].sum()) for j in sorted(kept)]
    new_of = {j: k for k, j in enumerate(sorted(kept))}
    u0, s0, v0 = to_host(bb, U0), to_host(bb, S0), to_host(bb, Vh0)
    u, s, vh = to_host(bb, U), to_host(bb, S), to_host(bb, Vh)
    assert sorted(s) == [(new_of[j], new_of[j]) for j in sorted(kept) if (j, j) in s0]
    for k, (i, j) in enumerate(common):
        if k not in kept:
            assert all(key[1] != new_of.get(k, -1) for key in u)
            continue
        m, kk = kept[k], new_of[k]
        assert np.array_equal(u[(i, kk)], u0[(i, k)][:, m]) and np.array_equal(vh[(kk, j)], v0[(k, j)][m, :])
        if (k, k) in s0:
            assert np.array_equal(s[(kk, kk)], s0[(k, k)][m])
    assert len(u) == len(kept) and len(vh) == len(kept)
    # U diag(S) Vh composed back (scale_axis on U's one-leg domain, then compose) is t projected onto the kept singular vectors
    US = ft.scale_axis(bb, U, forest, new_leg, S, new_leg, forest.num_legs)
    back = to_host(bb, ft.compose(bb, US, Vh))
    assert sorted(back) == [(i, j) for k, (i, j) in enumerate(common) if k in kept and (k, k) in s0]
    for k, (i, j) in enumerate(common):
        if (i, j) in back:
            p, blk = u0[(i, k)][:, kept[k]], _as_dict(t)[(i, j)]
            assert np.abs(back[(i, j)] - p @ (np.conj(p.T) @ blk)).max() <= 1e-12 * np.abs(blk).max()
