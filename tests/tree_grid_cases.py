"""Inputs and checks of from_grid / from_tree_pairs / eye on fusion-tree tensors shared by tests/test_tree_grid.py (numpy
stand-in: the record building without a device) and tests/test_gpu_tree_grid.py (HipBlockBackend: the same inputs, the same
criteria).

(a) abelian trees against the dense tensor -- the independent check: U(1) legs, the grid of dense entries concatenated along
    the first codomain axis and the last domain axis (zeros for None), brought into the sector order of the new legs and cut
    into blocks.  A placement with the factor 1 is exact: ``np.array_equal``.
(b) made-up spaces (forests of two and more trees on both sides, three coupled sectors, an entry that lacks a block, an entry
    that is a dagger view) against the restatement of the reference's forest-wise loop, tests/tree_grid_ref.py.  Without
    factors ``np.array_equal``; with complex factors every element is ONE complex product c x on both sides, each within 2 u
    |c|_1 |x|_1 of the exact value however it is contracted (two real products and one sum per component, each rounded once or
    fused), u = 2^-53: componentwise within 4 u |c|_1 |x|_1.
(c) SU(2) through to_dense_block, the norm of a direct sum, compose with eye.     (d) from_tree_pairs.     (e) error paths."""
import contextlib
import copy

import numpy as np
import pytest

import tree_dense_cases as dense
import tree_dense_ref
import tree_grid_ref as ref
from cyten_amd import fusion_tree as ft
from tree_dense_cases import NumpyDenseBackend, two_leg_dense
from tree_ops_cases import KeyedAbelianTrees, to_dev, to_host
from tree_outer_cases import _spin_leg, _two_leg_space

U = 2.0 ** -53


class NumpyLoopBackend(NumpyDenseBackend):
    """the stand-in of the tree operations WITHOUT ``tree_place_many``: from_grid takes zeros_many and get_item / set_item"""

    def set_item(self, a, key, value):
        a[key] = value

    def eye_matrix(self, dim, dtype=None, device=None):
        return np.eye(dim, dtype=dtype or float)


class NumpyGridBackend(NumpyLoopBackend):
    """... + a looped ``tree_place_many``; remembers (window shape, whether it has a source) of every record of every call"""

    def __init__(self):
        self.place_calls = []

    def tree_place_many(self, records):
        records = list(records)
        self.place_calls.append([(tuple(dst.shape), src is not None) for dst, src, _, _ in records])
        for dst, src, n_row, coeff in records:
            assert dst.ndim == 3 and dst.base is not None                  # a window of a block, written in place
            if src is None:
                dst[...] = 0
                continue
            assert np.iscomplexobj(dst) or not (np.iscomplexobj(src) or complex(coeff).imag != 0)
            assert int(np.prod(src.shape[:n_row], dtype=np.int64)) == dst.shape[0]
            v = np.reshape(src, dst.shape)
            dst[...] = v if coeff == 1 else coeff * v


@contextlib.contextmanager
def captured_windows():
    """the window lists ``fusion_tree._place_windows`` is handed, whatever the backend"""
    seen, orig = [], ft._place_windows

    def spy(bb, shapes, cplx, windows):
        seen.append(list(windows))
        return orig(bb, shapes, cplx, windows)

    ft._place_windows = spy
    try:
        yield seen
    finally:
        ft._place_windows = orig


def tensor(bb, data, cod, dom):
    return ft.TreeTensor(to_dev(bb, data), cod, dom)


def within_product(got, want, S):
    """componentwise within 4 u S, S = |c|_1 |x|_1"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and not np.isnan(got).any()
    bound = 4 * U * np.asarray(S, dtype=np.float64)
    assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees against the dense tensor

ABELIAN_CONFIGS = [(1, 1, 3, 3), (2, 1, 2, 3), (2, 2, 2, 2), (3, 1, 2, 2), (1, 3, 2, 2)]       # (J, K, grid rows, grid columns)
KINDS = ['real', 'complex', 'mixed']


class GridAbelianTrees(KeyedAbelianTrees):
    """KeyedAbelianTrees of which a leg can be given other multiplicities: the charges of the leg stay, so the trees (tuples of
    sector indices) keep their keys"""

    def with_mults(self, changes: dict):
        other = copy.copy(self)
        other.legs = list(self.legs)
        for f, m in changes.items():
            other.legs[f] = (self.legs[f][0], np.asarray(m, dtype=np.int64))
        return other


def _sector_order(mults_of_parts):
    """positions of the concatenated axis (part after part, every part sector-major) in the order of the new leg: sector-major,
    the parts in their order inside a sector"""
    labels = np.concatenate([np.repeat(np.arange(len(m)), m) for m in mults_of_parts])
    return np.argsort(labels, kind='stable')


def abelian_case(rng, config, kind):
    J, K, nr, nc = config
    at = GridAbelianTrees(rng, J=J, K=K)
    first, last = 0, J + K - 1
    row_m = [rng.integers(1, 4, len(at.legs[first][0])) for _ in range(nr)]
    col_m = [rng.integers(1, 4, len(at.legs[last][0])) for _ in range(nc)]
    row_m[nr - 1][0] = 0                                                   # a sector of multiplicity 0 in one row
    holes = {(0, nc - 1)} | ({(1, 0)} if nr > 2 else set())                # every row and every column keeps an entry
    cf, df = list(range(J)), list(range(J, J + K))
    grid, dense_rows = [], []
    for i in range(nr):
        g_row, d_row = [], []
        for j in range(nc):
            at_ij = at.with_mults({first: row_m[i], last: col_m[j]})
            cplx = kind == 'complex' or (kind == 'mixed' and (i + j) % 2 == 1)
            T = at_ij.dense(rng, cplx)
            if (i, j) in holes:
                g_row.append(None)
                d_row.append(np.zeros(T.shape))
            else:
                g_row.append(at_ij.to_blocks(T, cf, df))
                d_row.append(T)
        grid.append(g_row)
        dense_rows.append(np.concatenate(d_row, axis=-1))
    big = np.concatenate(dense_rows, axis=0)
    big = np.take(np.take(big, _sector_order(row_m), axis=0), _sector_order(col_m), axis=-1)
    new = at.with_mults({first: sum(row_m), last: sum(col_m)})
    n_cod, n_dom, want = new.to_blocks(big, cf, df)
    left = {int(q): [0] + np.cumsum([m[k] for m in row_m]).tolist() for k, q in enumerate(at.legs[first][0])}
    right = {int(q): [0] + np.cumsum([m[k] for m in col_m]).tolist() for k, q in enumerate(at.legs[last][0])}
    return dict(grid=grid, n_cod=n_cod, n_dom=n_dom, left=left, right=right, want={tuple(r): b for r, b in zip(want.block_inds.tolist(), want.blocks)},
                cplx=kind != 'real')


def check_abelian(bb, rng, config, kind):
    c = abelian_case(rng, config, kind)
    grid = [[None if e is None else tensor(bb, e[2], e[0], e[1]) for e in row] for row in c['grid']]
    with captured_windows() as seen, dense.nan_filled(bb):
        got = ft.from_grid(bb, grid, c['n_cod'], c['n_dom'], c['left'], c['right'])
    assert len(c['want']) > 0
    assert got.block_inds.tolist() == sorted(got.block_inds.tolist())
    host = to_host(bb, got)
    assert sorted(host) == sorted(c['want'])
    for k, w in c['want'].items():
        assert np.iscomplexobj(host[k]) == c['cplx'] and np.array_equal(host[k], w), k
    (windows,) = seen
    per_tile: dict = {}
    for w in windows:
        per_tile.setdefault((w.n, w.x0, w.y0), []).append(w)
    assert any(w.src is None and w.h * w.nq * w.wn > 0 for w in windows)                 # a zero cell occurred ...
    assert any(len(ws) >= 2 for ws in per_tile.values())                                   # ... and a tile of two or more cells
    return c, windows


# ---------------------------------------------------------------------------------------------------------------------------
# (b) made-up spaces against the restatement

# coupled sector -> [(sector of the stacked leg, sector of the other leg, number of trees)]: forests of one, two and three trees,
# a stacked sector in several forests of one coupled sector
DEAL = {0: [('a', 'p', 2), ('b', 'p', 1)], 1: [('a', 'q', 2), ('b', 'q', 2), ('a', 'p', 1)], 2: [('b', 'q', 3)]}
OTHER = {'cod': {'p': 2, 'q': 3}, 'dom': {'p': 3, 'q': 1}}


def table_side(side, stacked: dict):
    """a two-leg side: the stacked leg is the first leg of the codomain / the last of the domain"""
    names, mults, unc = [], [], []
    for c in range(3):
        nm, mm, uu = [], [], []
        for s, o, n in DEAL[c]:
            for t in range(n):
                u = (s, o) if side == 'cod' else (o, s)
                nm.append((side, u, c, t))
                mm.append((stacked[s], OTHER[side][o]) if side == 'cod' else (OTHER[side][o], stacked[s]))
                uu.append(u)
        names.append(nm), mults.append(mm), unc.append(uu)
    return ft.TreeSpace.from_multiplicities([[0], [1], [2]], mults, np.array([1.0, 2.0, 3.0]), 2, names, unc)


def _random_blocks(rng, cod, dom, cplx, skip=()):
    rows, blocks = [], []
    for s in range(3):
        if s in skip:
            continue
        sh = (cod.block_size(s), dom.block_size(s))
        rows.append((s, s))
        blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0))
    return ft.FusionTreeData(rows, blocks)


ROW_M = [{'a': 2, 'b': 1}, {'a': 1, 'b': 3}]
COL_M = [{'a': 1, 'b': 2}, {'a': 3, 'b': 1}, {'a': 2, 'b': 2}]


def table_case(bb, rng, kinds='mixed'):
    """a 2 x 3 grid: (0, 1) is None, (0, 2) lacks the block of coupled sector 1, (1, 0) is the dagger of a tensor on the
    swapped spaces (a transposed view on the device).  -> (host grid for the restatement, device grid, spaces, tables)"""
    host, dev = [], []
    for i, rm in enumerate(ROW_M):
        h_row, d_row = [], []
        for j, cm in enumerate(COL_M):
            cod, dom = table_side('cod', rm), table_side('dom', cm)
            if (i, j) == (0, 1):
                h_row.append(None), d_row.append(None)
                continue
            cplx = kinds == 'complex' or (kinds == 'mixed' and (i + j) % 2 == 1)
            if (i, j) == (1, 0):
                raw = _random_blocks(rng, dom, cod, False)                 # real: its dagger is a view
                d = ft.dagger(bb, to_dev(bb, raw))
                h = ft.FusionTreeData(raw.block_inds[:, ::-1], [np.ascontiguousarray(b.T) for b in raw.blocks])
                h_row.append(ft.TreeTensor(h, cod, dom)), d_row.append(ft.TreeTensor(d, cod, dom))
                continue
            data = _random_blocks(rng, cod, dom, cplx, skip=(1,) if (i, j) == (0, 2) else ())
            h_row.append(ft.TreeTensor(data, cod, dom)), d_row.append(tensor(bb, data, cod, dom))
        host.append(h_row), dev.append(d_row)
    total = lambda ms: {k: sum(m[k] for m in ms) for k in 'ab'}                           # noqa: E731
    left = {k: [0] + np.cumsum([m[k] for m in ROW_M]).tolist() for k in 'ab'}
    right = {k: [0] + np.cumsum([m[k] for m in COL_M]).tolist() for k in 'ab'}
    return host, dev, table_side('cod', total(ROW_M)), table_side('dom', total(COL_M)), left, right


COMPLEX_FACTORS = [[0.75 - 0.5j, 2.0, -1.25j], [1.0, -0.5 + 2.0j, 0.375 + 0.25j]]
REAL_FACTORS = [[0.75, 2.0, -1.25], [1.0, -0.5, 0.375]]


def check_table(bb, rng, kinds, factors=None):
    host, dev, n_cod, n_dom, left, right = table_case(bb, rng, kinds)
    with dense.nan_filled(bb):
        got = ft.from_grid(bb, dev, n_cod, n_dom, left, right, factors=factors)
    want = ref.from_grid_ref(host, n_cod, n_dom, left, right, factors=factors)
    have = to_host(bb, got)
    assert sorted(have) == sorted(want) == [(0, 0), (1, 1), (2, 2)] and got.block_inds.tolist() == sorted(got.block_inds.tolist())
    cplx = kinds != 'real' or (factors is not None and any(complex(f).imag != 0 for row in factors for f in row))
    if factors is None:
        for k, w in want.items():
            assert np.iscomplexobj(have[k]) == cplx and np.array_equal(have[k], w), k
    else:
        S = ref.from_grid_ref(host, n_cod, n_dom, left, right, factors=factors, absolute=True, discard=False)
        for k, w in want.items():
            assert np.iscomplexobj(have[k]) == cplx
            within_product(have[k], w, S[k])
    assert max(len(ref.forests(n_cod, 1)), len(ref.forests(n_dom, 1))) == 3 and len(n_cod.tree_blocks[2]) == 3
    return have


# ---------------------------------------------------------------------------------------------------------------------------
# (c) SU(2); sectors are 2 j

def _dense_map(new_leg: ft.TreeSpace, part: ft.TreeSpace, slices: dict, pos: int):
    """where the dense positions of a one-leg space `part` (sector j: d * m positions, index k * m + mu) lie on the dense axis of
    the stacked leg `new_leg`, whose sector j holds `part` at the multiplicities ``slices[j][pos] : slices[j][pos + 1]``"""
    start, off = {}, 0
    for (j,), tbs in zip(new_leg.sectors.tolist(), new_leg.tree_blocks):
        m = tbs[0].multiplicities[0]
        start[j] = (off, m)
        off += (j + 1) * m
    out = []
    for (j,), tbs in zip(part.sectors.tolist(), part.tree_blocks):
        m = tbs[0].multiplicities[0]
        o, M = start[j]
        out += [o + k * M + slices[j][pos] + mu for k in range(j + 1) for mu in range(m)]
    return np.array(out, dtype=np.int64)


def _stack(parts):
    """(the stacked one-leg multiplicities, slice table) of one-leg multiplicity dicts"""
    keys = sorted({j for p in parts for j in p})
    table = {j: [0] + np.cumsum([p.get(j, 0) for p in parts]).tolist() for j in keys}
    return {j: table[j][-1] for j in keys}, table


def check_su2_grid(bb, rng, cplx):
    """a 2 x 2 grid of (w, p) <- (p, w') tensors with different spin content on the stacked legs, (1, 0) is None:
    to_dense_block(from_grid(grid)) is the grid of to_dense_block of the entries, placed by sector.

    Bound: both sides are to_dense_block results, each within (P + 6) u S of the exact value (tests/tree_dense_cases.py, P terms
    per element, S the sum on absolute values); the placement adds nothing: ``tree_dense_cases.within`` with its factor 2."""
    rows, cols = [{0: 2, 2: 1}, {1: 1, 2: 2}], [{0: 1, 1: 2}, {1: 1, 2: 1}]
    P, Pd = _spin_leg('p', {1: 2}), _spin_leg('q', {1: 1, 2: 1})
    (wm, left), (vm, right) = _stack(rows), _stack(cols)
    Wn, Vn = _spin_leg('w', wm), _spin_leg('v', vm)
    n_cod, n_dom = _two_leg_space('c', Wn, P), _two_leg_space('d', Pd, Vn)
    n_cd, n_dd = two_leg_dense('c', Wn, P, n_cod), two_leg_dense('d', Pd, Vn, n_dom)
    grid, pieces = [], []
    for i, rm in enumerate(rows):
        g_row = []
        for j, cm in enumerate(cols):
            if (i, j) == (1, 0):
                g_row.append(None)
                continue
            W, V = _spin_leg('w', rm), _spin_leg('v', cm)
            cod, dom = _two_leg_space('c', W, P), _two_leg_space('d', Pd, V)
            cd, dd = two_leg_dense('c', W, P, cod), two_leg_dense('d', Pd, V, dom)
            data = dense.random_data(rng, cod, dom, cplx and (i + j) % 2 == 0)
            t = tensor(bb, data, cod, dom)
            g_row.append(t)
            D = dense.host(bb, ft.to_dense_block(bb, t.data, cod, dom, cd, dd))
            Pn = tree_dense_ref.to_dense(data, cod, dom, cd, dd, count=True)
            A = tree_dense_ref.to_dense(data, cod, dom, cd, dd, absolute=True)
            pieces.append((_dense_map(Wn, W, left, i), _dense_map(Vn, V, right, j), D, Pn, A))
        grid.append(g_row)
    with dense.nan_filled(bb):
        got = ft.from_grid(bb, grid, n_cod, n_dom, left, right)
    G = dense.host(bb, ft.to_dense_block(bb, got, n_cod, n_dom, n_cd, n_dd))
    want, Pw, Sw = np.zeros(G.shape, dtype=G.dtype), np.zeros(G.shape), np.zeros(G.shape)
    for m0, m2, D, Pn, A in pieces:                                        # dense axes: (w, p, v, q)
        sel = np.ix_(m0, np.arange(G.shape[1]), m2, np.arange(G.shape[3]))
        want[sel], Pw[sel], Sw[sel] = D, Pn, A
    assert np.iscomplexobj(G) == cplx and np.abs(want).max() > 0.1 and (Pw == 0).any()
    dense.within(G, want, Pw, Sw)
    return got


def check_su2_direct_sum(bb, rng, cplx):
    """[[A, None], [None, B]] of (v, p) <- v' tensors: norm^2 = norm(A)^2 + norm(B)^2 to 1e-13 relative"""
    P = _spin_leg('p', {1: 1})
    rows, cols = [{0: 3, 1: 2, 2: 1}, {0: 1, 1: 4}], [{0: 2, 1: 3}, {1: 2, 2: 2}]
    (wm, left), (vm, right) = _stack(rows), _stack(cols)
    n_cod, n_dom = _two_leg_space('c', _spin_leg('w', wm), P), _spin_leg('v', vm)
    ts = []
    for rm, cm in zip(rows, cols):
        cod, dom = _two_leg_space('c', _spin_leg('w', rm), P), _spin_leg('v', cm)
        ts.append(tensor(bb, dense.random_data(rng, cod, dom, cplx), cod, dom))
    with dense.nan_filled(bb):
        got = ft.from_grid(bb, [[ts[0], None], [None, ts[1]]], n_cod, n_dom, left, right)
    n2 = ft.norm(bb, got, n_cod) ** 2
    parts = sum(ft.norm(bb, t.data, t.codomain) ** 2 for t in ts)
    assert len(got.blocks) >= 2 and parts > 1.0 and abs(n2 - parts) <= 1e-13 * parts
    return got


def check_eye(bb, rng, cplx):
    """compose(eye(codomain), a) is a: products with 1 and 0 and sums with 0 are exact"""
    cod = _two_leg_space('c', _spin_leg('w', {0: 2, 1: 1, 2: 2}), _spin_leg('p', {1: 2}))
    dom = _spin_leg('v', {0: 1, 1: 3, 2: 2})
    a = dense.random_data(rng, cod, dom, cplx)
    e = ft.eye(bb, cod, dtype=np.complex128 if cplx else None)
    assert e.block_inds.tolist() == [[i, i] for i in range(cod.num_sectors)]
    assert all(tuple(b.shape) == (cod.block_size(i),) * 2 for i, b in enumerate(e.blocks))
    got = to_host(bb, ft.compose(bb, e, to_dev(bb, a)))
    want = {tuple(r): b for r, b in zip(a.block_inds.tolist(), a.blocks)}
    assert sorted(got) == sorted(want) and len(want) >= 2
    for k, w in want.items():
        assert np.array_equal(got[k], w), k


# ---------------------------------------------------------------------------------------------------------------------------
# (d) from_tree_pairs

TREE_PAIR_CONFIGS = [(0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3), (3, 3), (0, 3), (3, 0)]     # (J, K)


def tree_pairs_case(bb, rng, config, cplx):
    """random blocks cut into tiles on the host, every tile reshaped and permuted to (m_1 .. m_J, n_K .. n_1) and handed over as
    a non-contiguous view of the device copy of another axis order"""
    J, K = config
    for _ in range(100):                    # (a side without legs holds the charge 0 only: draw until the sides share a sector)
        at = KeyedAbelianTrees(rng, J=J, K=K)
        cod, dom = at.space(list(range(J))), at.space(list(range(J, J + K)))
        common = ft.common_sectors(cod, dom)
        if len(common) >= (2 if min(J, K) > 0 else 1):
            break
    blocks, trees = {}, {}
    for i, j in common:
        sh = (cod.block_size(i), dom.block_size(j))
        blocks[(i, j)] = rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0)
        for xb in cod.tree_blocks[i]:
            for yb in dom.tree_blocks[j]:
                tile = blocks[(i, j)][xb.start:xb.stop, yb.start:yb.stop].reshape(xb.multiplicities + yb.multiplicities)
                T = tile.transpose(list(range(J)) + list(range(J + K - 1, J - 1, -1)))
                perm = rng.permutation(J + K).tolist()
                stored = bb.as_block(np.ascontiguousarray(T.transpose(perm)))
                trees[(xb.tree, yb.tree)] = bb.permute_axes(stored, np.argsort(perm).tolist())
    return cod, dom, blocks, trees


def check_tree_pairs(bb, rng, config, cplx):
    cod, dom, blocks, trees = tree_pairs_case(bb, rng, config, cplx)
    with dense.nan_filled(bb):
        got = ft.from_tree_pairs(bb, trees, cod, dom)
    have = to_host(bb, got)
    assert sorted(have) == sorted(blocks) and got.block_inds.tolist() == sorted(got.block_inds.tolist())
    for k, w in blocks.items():
        assert np.iscomplexobj(have[k]) == cplx and np.array_equal(have[k], w), k
    host_trees = {k: np.asarray(bb.to_numpy(v)) for k, v in trees.items()}
    want = ref.from_tree_pairs_ref(host_trees, cod, dom, np.complex128 if cplx else np.float64)
    assert all(np.array_equal(have[k], want[k]) for k in want)
    return cod, dom, blocks, trees


def check_tree_pairs_structure(bb, rng):
    """a missing tile comes back as zeros, a coupled sector without entries is absent, an uncovered key raises, a complex
    dtype promotes, a wrong shape and a seventh leg raise"""
    cod, dom, blocks, trees = tree_pairs_case(bb, rng, (2, 2), False)
    multi = [(i, j) for i, j in blocks if len(cod.tree_blocks[i]) * len(dom.tree_blocks[j]) >= 2]
    assert multi and len(blocks) >= 2
    i0, j0 = multi[0]
    gone = (cod.tree_blocks[i0][0], dom.tree_blocks[j0][-1])
    empty = next(k for k in blocks if k != (i0, j0))
    some = {k: v for k, v in trees.items() if k != (gone[0].tree, gone[1].tree)
            and k[0] not in {tb.tree for tb in cod.tree_blocks[empty[0]]}}
    with dense.nan_filled(bb):
        got = ft.from_tree_pairs(bb, some, cod, dom, dtype=np.complex128)
    have = to_host(bb, got)
    assert sorted(have) == sorted(k for k in blocks if k != empty)
    want = blocks[(i0, j0)].copy()
    want[gone[0].start:gone[0].stop, gone[1].start:gone[1].stop] = 0
    assert np.iscomplexobj(have[(i0, j0)]) and np.array_equal(have[(i0, j0)], want)
    key = next(iter(trees))
    with pytest.raises(ValueError, match='uncovered tree pair'):
        ft.from_tree_pairs(bb, {**trees, ('no', 'tree'): trees[key]}, cod, dom)
    with pytest.raises(ValueError, match='has the shape'):
        ft.from_tree_pairs(bb, {**trees, key: bb.as_block(np.zeros(tuple(trees[key].shape) + (1,)))}, cod, dom)
    with pytest.raises(ValueError, match='complex block'):
        ft.from_tree_pairs(bb, {key: bb.as_block(np.zeros(tuple(trees[key].shape), dtype=complex))}, cod, dom, dtype=np.float64)
    seven = KeyedAbelianTrees(rng, J=7, K=1)
    with pytest.raises(ValueError, match='at most 6'):
        ft.from_tree_pairs(bb, {}, seven.space(list(range(7))), seven.space([7]))
    none = ft.from_tree_pairs(bb, {}, cod, dom)
    assert len(none.blocks) == 0 and none.block_inds.shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) structure and error paths of from_grid

def check_discard(bb, rng):
    """a result block whose only entries are zeros is dropped unless ``discard=False``; coupled sectors no entry holds are absent"""
    cod, dom = table_side('cod', ROW_M[0]), table_side('dom', COL_M[0])
    data = _random_blocks(rng, cod, dom, False, skip=(2,))
    data.blocks[0] = np.zeros_like(data.blocks[0])
    left, right = {k: [0, ROW_M[0][k]] for k in 'ab'}, {k: [0, COL_M[0][k]] for k in 'ab'}
    grid = [[tensor(bb, data, cod, dom)]]
    kept = ft.from_grid(bb, grid, cod, dom, left, right)
    every = ft.from_grid(bb, grid, cod, dom, left, right, discard=False)
    assert kept.block_inds.tolist() == [[1, 1]] and every.block_inds.tolist() == [[0, 0], [1, 1]]
    assert np.array_equal(to_host(bb, every)[(1, 1)], data.blocks[1]) and not to_host(bb, every)[(0, 0)].any()
    big = ft.from_grid(bb, grid, cod, dom, left, right, eps=1e300)
    assert len(big.blocks) == 0 and big.block_inds.shape == (0, 2)


def check_errors(bb, rng):
    _, dev, n_cod, n_dom, left, right = table_case(bb, rng, 'real')
    run = lambda g=dev, c=n_cod, d=n_dom, l=left, r=right, **kw: ft.from_grid(bb, g, c, d, l, r, **kw)   # noqa: E731
    with pytest.raises(ValueError, match='empty grid'):
        run(g=[])
    with pytest.raises(ValueError, match='empty grid'):
        run(g=[[]])
    with pytest.raises(ValueError, match='differ in their length'):
        run(g=[dev[0], dev[1][:2]])
    with pytest.raises(ValueError, match='row 0 of the grid has no entry'):
        run(g=[[None, None, None], dev[1]])
    with pytest.raises(ValueError, match='column 1 of the grid has no entry'):
        run(g=[dev[0], [dev[1][0], None, dev[1][2]]])
    with pytest.raises(ValueError, match='factors'):
        run(factors=[[1.0, 2.0, 3.0]])
    with pytest.raises(ValueError, match="left_slices has no entry for the sector 'b'"):
        run(l={'a': left['a']})
    with pytest.raises(ValueError, match="right_slices has no entry for the sector 'a'"):
        run(r={'b': right['b']})
    with pytest.raises(ValueError, match='ascending table'):
        run(l={**left, 'a': left['a'][:-1]})
    with pytest.raises(ValueError, match='ends at'):
        run(r={**right, 'b': right['b'][:-1] + [right['b'][-1] + 1]})
    # a slice width that is not the entry's own multiplicity (the total is kept)
    bad = {**left, 'a': [0, left['a'][1] + 1, left['a'][2]]}
    with pytest.raises(ValueError, match='its slice is'):
        run(l=bad)
    # a multiplicity other than the stacked one
    t = dev[0][0]
    wrong_cod = table_side('cod', ROW_M[0])
    wrong_cod = ft.TreeSpace(wrong_cod.sectors, wrong_cod.qdims,
                             [[ft.TreeBlock(tb.tree, 2 * tb.start, 2 * tb.stop, (tb.multiplicities[0], 2 * tb.multiplicities[1]), tb.uncoupled)
                               for tb in tbs] for tbs in wrong_cod.tree_blocks], 2)
    wide = ft.FusionTreeData(t.block_inds, [bb.as_block(np.zeros((wrong_cod.block_size(s), t.domain.block_size(s)))) for s in range(3)])
    with pytest.raises(ValueError, match='other than the stacked one'):
        run(g=[[ft.TreeTensor(wide, wrong_cod, t.domain)] + dev[0][1:], dev[1]])
    # a tree of an entry that the new space does not hold
    renamed = ft.TreeSpace(t.domain.sectors, t.domain.qdims,
                           [[ft.TreeBlock(('elsewhere',) + tb.tree, tb.start, tb.stop, tb.multiplicities, tb.uncoupled) for tb in tbs]
                            for tbs in t.domain.tree_blocks], 2)
    with pytest.raises(ValueError, match='has no tree'):
        run(g=[[ft.TreeTensor(t.data, t.codomain, renamed)] + dev[0][1:], dev[1]])
    # trees without the uncoupled keys
    bare = ft.TreeSpace(t.codomain.sectors, t.codomain.qdims,
                        [[ft.TreeBlock(tb.tree, tb.start, tb.stop, tb.multiplicities) for tb in tbs] for tbs in t.codomain.tree_blocks], 2)
    with pytest.raises(ValueError, match='lacks the uncoupled'):
        run(g=[[ft.TreeTensor(t.data, bare, t.domain)] + dev[0][1:], dev[1]])
    one = ft.TreeSpace.from_multiplicities([[0]], [[()]], None, 0, [['e']], [[()]])
    with pytest.raises(ValueError, match='both sides need a leg'):
        run(c=one)
