"""Inputs and checks of the fusion-tree partial trace shared by tests/test_tree_trace.py (numpy stand-in: the record building
without a device) and tests/test_gpu_tree_trace.py (HipBlockBackend: the same inputs, the same criteria).

(a) abelian trees against the dense tensor -- the independent check: U(1) legs, the second leg of a traced pair is the dual
    of the first (negated charges, the same multiplicities), every factor is 1 and the dense answer is an index-paired sum.
(b) random tables (complex factors, a third of the trees off the diagonal, forests) against the restatement of the
    reference's loop, tests/tree_trace_ref.py.
(c) `move`: an abelian braid first.   (d) the error paths.

Tolerance.  Both sides add the same N addends per element in some order and multiply each term's sum by its coefficient
once: each is within (N + 4) u S of the exact value, u = 2^-53, S = sum_t (|c_re| + |c_im|) sum_tau (|s_re| + |s_im|) -- N - 1
additions in any order and the roundings of one complex product per term, componentwise -- so two such results differ by at
most 2 (N + 4) u S.  N and S come from the reference (dense or restated) run on ones and on the absolute values."""
import copy
import dataclasses

import numpy as np

import tree_trace_ref as ref
from cyten_amd import fusion_tree as ft
from oracle import block_ops as ops
from tree_ops_cases import KeyedAbelianTrees, NumpyTreeBackend, to_dev, to_host

U = 2.0 ** -53


class NumpyTraceBackend(NumpyTreeBackend):
    """the stand-in of the tree operations + ``transform_blocks`` and a looped ``tree_trace_many``; remembers the records of
    the last call, so that a test can see which tiles got how many terms"""

    def __init__(self):
        self.trace_calls = []

    def transform_blocks(self, old_blocks, new_shapes, updates):
        return ops.transform_blocks(old_blocks, new_shapes, updates)

    def tree_trace_many(self, outputs):
        outputs = list(outputs)
        self.trace_calls.append([(tuple(dst.shape), len(terms)) for dst, terms in outputs])
        for dst, terms in outputs:
            acc = np.zeros(dst.shape, dtype=dst.dtype)
            for src, idcs1, idcs2, remaining, coeff in terms:
                assert np.iscomplexobj(dst) or not (np.iscomplexobj(src) or isinstance(coeff, complex))
                acc = acc + coeff * ref.trace_partial(src, idcs1, idcs2, remaining)
            dst[...] = acc


def assert_within(got: dict, want: dict, N: dict, S: dict):
    """the same coupled sectors, every element componentwise within 2 (N + 4) u S"""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and not np.isnan(g).any(), k
        bound = 2 * (N[k] + 4) * U * S[k]
        assert np.all(np.abs(np.real(g) - np.real(w)) <= bound) and np.all(np.abs(np.imag(g) - np.imag(w)) <= bound), k


# ---------------------------------------------------------------------------------------------------------------------------
# (a), (c): abelian trees

class DualAbelianTrees(KeyedAbelianTrees):
    """AbelianTrees (with ``uncoupled`` keys) in which factor g of every ``(f, g)`` in `duals` is the dual of factor f"""

    def __init__(self, rng, J, K, duals):
        super().__init__(rng, J=J, K=K)
        for f, g in duals:
            q, m = self.legs[f]
            order = np.argsort(-q)
            self.legs[g] = ((-q)[order], m[order])

    def pairing(self, f, g):
        """index on factor g that is paired with every index of factor f (the same position inside the dual sector)"""
        (qf, mf), (qg, mg) = self.legs[f], self.legs[g]
        off_g = np.concatenate([[0], np.cumsum(mg)])
        p = []
        for q, m in zip(qf, mf):
            s = int(np.flatnonzero(qg == -q)[0])
            assert mg[s] == m
            p.append(off_g[s] + np.arange(m))
        return np.concatenate(p)

    def trace_table(self, factors, positions):
        """(TreeTrace, remaining factors) of tracing the factors at `positions` / `positions + 1` of a side: a tree is on the
        diagonal if the two charges of every pair cancel; all factors are 1 (U(1): B symbols and Frobenius-Schur signs are 1)"""
        factors = list(factors)
        dropped = {a for k in positions for a in (k, k + 1)}
        new_f = tuple(f for a, f in enumerate(factors) if a not in dropped)
        table = {}
        for tbs in self.space(factors).tree_blocks:
            for tb in tbs:
                idx = tb.tree[1]
                if all(self.legs[factors[k]][0][idx[k]] == -self.legs[factors[k + 1]][0][idx[k + 1]] for k in positions):
                    table[tb.tree] = ((new_f, tuple(i for a, i in enumerate(idx) if a not in dropped)), 1.0)
        return ft.TreeTrace(tuple(positions), table), list(new_f)

    def dense_trace(self, T, pairs):
        """index-paired sum over the dense axes ``(a, a + 1)`` that carry the factors ``(f, g)``, for ``(a, f, g)`` in `pairs`"""
        for a, f, g in sorted(pairs, reverse=True):
            T = np.trace(np.take(T, self.pairing(f, g), axis=a + 1), axis1=a, axis2=a + 1)
        return np.asarray(T)


# (J, K, traced codomain positions, traced domain positions)
ABELIAN_CONFIGS = {
    'codomain': (3, 2, (0,), ()),
    'domain': (2, 3, (), (1,)),
    'both': (3, 3, (1,), (0,)),
    'two_pairs': (5, 1, (0, 3), ()),
    'between': (4, 3, (1,), ()),
    'full': (4, 0, (0, 2), ()),
}


def abelian_case(rng, name, cplx, starve=False):
    """everything of case (a) on the host: spaces, tables, numpy data, the dense answer and its N / S as block dicts"""
    J, K, cpos, dpos = ABELIAN_CONFIGS[name]
    at = DualAbelianTrees(rng, J, K, [(k, k + 1) for k in cpos] + [(J + k, J + k + 1) for k in dpos])
    cf, df = list(range(J)), list(range(J, J + K))
    ct, ncf = at.trace_table(cf, cpos) if cpos else (None, cf)
    dt, ndf = at.trace_table(df, dpos) if dpos else (None, df)
    T = at.dense(rng, cplx)
    if starve:
        # one new codomain tree loses its feeders: they count as off the diagonal, and the tensor vanishes on them, so
        # that the dense answer stays right -- the tiles of that tree then receive no term
        victim = at.space(ncf).tree_blocks[len(at.space(ncf).tree_blocks) // 2][0].tree
        offs = [np.concatenate([[0], np.cumsum(at.legs[f][1])]) for f in range(J + K)]
        sl = [slice(None)] * (J + K)
        for f, i in zip(victim[0], victim[1]):
            sl[f] = slice(int(offs[f][i]), int(offs[f][i + 1]))
        T[tuple(sl)] = 0
        ct = ft.TreeTrace(ct.positions, {k: v for k, v in ct.table.items() if v[0] != victim})
    cod, dom, data = at.to_blocks(T, cf, df)
    pairs = [(k, cf[k], cf[k + 1]) for k in cpos] + [(J + k, df[k], df[k + 1]) for k in dpos]
    n_cod, n_dom = at.space(ncf), at.space(ndf)

    def blocks_of(D):
        _, _, d = at.to_blocks(D, ncf, ndf)
        return {tuple(r): b for r, b in zip(d.block_inds.tolist(), d.blocks)}

    want = blocks_of(at.dense_trace(T, pairs))
    S = blocks_of(at.dense_trace(np.abs(T.real) + np.abs(T.imag), pairs))
    N = int(np.prod([int(at.legs[f][1].sum()) for _, f, _ in pairs]))
    return dict(at=at, T=T, cod=cod, dom=dom, data=data, n_cod=n_cod, n_dom=n_dom, ct=ct, dt=dt, want=want, S=S, N=N, pairs=pairs)


def check_abelian(bb, rng, name, cplx, starve=False):
    c = abelian_case(rng, name, cplx, starve)
    got = ft.partial_trace(bb, to_dev(bb, c['data']), c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt'])
    assert len(c['want']) > 0
    host = to_host(bb, got)
    assert all(np.iscomplexobj(b) == cplx for b in host.values())
    assert_within(host, c['want'], {k: c['N'] for k in c['want']}, c['S'])
    return c, got


def check_full_trace(bb, rng, cplx):
    """all legs traced: the single 1 x 1 block, equal to the dense paired sum and to ``ft.trace_full`` of the same numbers
    read as a tensor with the codomain (a, b) and the domain (a, b): T2[i, j, k, l] = T[i, p_a(k), j, p_b(l)]"""
    c = abelian_case(rng, 'full', cplx)
    at, T = c['at'], c['T']
    got = ft.partial_trace(bb, to_dev(bb, c['data']), c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt'])
    assert got.block_inds.tolist() == [[0, 0]] and tuple(got.blocks[0].shape) == (1, 1)
    val = complex(bb.to_numpy(got.blocks[0])[0, 0])
    want = complex(at.dense_trace(T, c['pairs']))
    bound = 2 * (c['N'] + 4) * U * float(at.dense_trace(np.abs(T.real) + np.abs(T.imag), c['pairs']))
    assert abs(val.real - want.real) <= bound and abs(val.imag - want.imag) <= bound
    sq = copy.copy(at)
    sq.J, sq.K, sq.legs = 2, 2, [at.legs[0], at.legs[2], at.legs[0], at.legs[2]]
    T2 = np.take(np.take(T, at.pairing(0, 1), axis=1), at.pairing(2, 3), axis=3).transpose(0, 2, 1, 3)
    cod2, _, data2 = sq.to_blocks(T2, [0, 1], [2, 3])
    full = complex(ft.trace_full(bb, to_dev(bb, data2), cod2))
    assert abs(full.real - want.real) <= bound and abs(full.imag - want.imag) <= bound
    # a tensor without the block of the trivial sector: still the 1 x 1 block, zero, written by a record without terms
    none = ft.partial_trace(bb, ft.FusionTreeData(np.zeros((0, 2), np.int64), []), c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt'])
    assert none.block_inds.tolist() == [[0, 0]] and complex(bb.to_numpy(none.blocks[0])[0, 0]) == 0
    return c


def check_move(bb, rng, cplx):
    """codomain (a, b, a-bar, c), domain (d, e): the braid (a, a-bar, b, c), (e, d) first, then the pair at position 0 -- against
    the dense permute-then-trace"""
    at = DualAbelianTrees(rng, 4, 2, [(0, 2)])
    T = at.dense(rng, cplx)
    cf, df = [0, 1, 2, 3], [4, 5]
    cod, dom, data = at.to_blocks(T, cf, df)
    codomain_idcs, domain_idcs, mcf, mdf, mapping = at.braid([0, 2, 1, 3], [1, 0])
    ct, ncf = at.trace_table(mcf, (0,))
    move = (at.space(mcf), at.space(mdf), codomain_idcs, domain_idcs, mapping)
    got = ft.partial_trace(bb, to_dev(bb, data), cod, dom, at.space(ncf), at.space(mdf), ct, None, move=move)
    Tm = T.transpose(mcf + mdf)
    pairs = [(0, mcf[0], mcf[1])]

    def blocks_of(D):
        _, _, d = at.to_blocks(D, ncf, mdf)
        return {tuple(r): b for r, b in zip(d.block_inds.tolist(), d.blocks)}

    want = blocks_of(at.dense_trace(Tm, pairs))
    S = blocks_of(at.dense_trace(np.abs(Tm.real) + np.abs(Tm.imag), pairs))
    assert len(want) > 1
    assert_within(to_host(bb, got), want, {k: int(at.legs[0][1].sum()) for k in want}, S)


# ---------------------------------------------------------------------------------------------------------------------------
# (b), (d): forests with made-up trees and random tables

def _forest_side(rng, tag, old_sectors, new_sectors, positions, first_leg_remains, cplx_factors):
    """one side with three legs, two of them a traced pair: per coupled sector six old trees and up to three new ones.  Every
    third old tree is off the diagonal (absent from the table, unequal pair multiplicities); the first old tree of a sector
    feeds its first new tree, whose multiplicity is 2 in every sector; the last new tree of a sector may stay without feeders."""
    new_mults, new_names = [], []
    for s in new_sectors:
        k = int(rng.integers(2, 4))
        new_mults.append([(2,)] + [(int(rng.integers(1, 4)),) for _ in range(k - 1)])
        new_names.append([(tag, 'new', s, t) for t in range(k)])
    new = ft.TreeSpace.from_multiplicities(np.array(new_sectors)[:, None], new_mults, None, 1, new_names,
                                           [[(f'{tag}{s}.{t}',) for t in range(len(m))] for s, m in zip(new_sectors, new_mults)])
    old_mults, old_names, table = [], [], {}
    for s in old_sectors:
        mults, names = [], []
        for t in range(6):
            name = (tag, 'old', s, t)
            f = complex(rng.standard_normal(), rng.standard_normal() if cplx_factors else 0.0)
            if t % 3 == 2:
                pair, rem = (int(rng.integers(1, 4)), int(rng.integers(1, 4)) + 3), int(rng.integers(1, 4))
            elif s in new_sectors:
                i = new_sectors.index(s)
                k = 0 if t == 0 else int(rng.integers(0, max(1, len(new_mults[i]) - 1)))
                pair, rem = (int(rng.integers(1, 4)),) * 2, new_mults[i][k][0]
                table[name] = (new_names[i][k], f if cplx_factors else f.real)
            else:                 # a sector that does not survive: the symmetry layer lists its trees all the same
                pair, rem = (int(rng.integers(1, 4)),) * 2, int(rng.integers(1, 4))
                table[name] = ((tag, 'gone', s, t), f if cplx_factors else f.real)
            mults.append((rem,) + pair if first_leg_remains else pair + (rem,))
            names.append(name)
        old_mults.append(mults)
        old_names.append(names)
    old = ft.TreeSpace.from_multiplicities(np.array(old_sectors)[:, None], old_mults, None, 3, old_names,
                                           [[tuple(f'{tag}{s}.{t}.{a}' for a in range(3)) for t in range(6)] for s in old_sectors])
    return old, new, ft.TreeTrace(tuple(positions), table)


def forest_case(rng, cplx_data, cplx_factors=True):
    """codomain (x, t, t-bar) with sectors 0..3, domain (t, t-bar, y) with sectors 1..4: the data holds the sectors 1, 2, 3; the
    new spaces hold 0, 1, 2 and 1, 2, 4, so that sector 3 of the data is skipped"""
    cod, n_cod, ct = _forest_side(rng, 'c', [0, 1, 2, 3], [0, 1, 2], (1,), True, cplx_factors)
    dom, n_dom, dt = _forest_side(rng, 'd', [1, 2, 3, 4], [1, 2, 4], (0,), False, cplx_factors)
    rows, blocks = [], []
    for i, j in ft.common_sectors(cod, dom):
        sh = (cod.block_size(i), dom.block_size(j))
        rows.append((i, j))
        blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx_data else 0))
    return dict(cod=cod, dom=dom, n_cod=n_cod, n_dom=n_dom, ct=ct, dt=dt, data=ft.FusionTreeData(rows, blocks))


def check_forest(bb, rng, cplx_data, cplx_factors=True):
    c = forest_case(rng, cplx_data, cplx_factors)
    args = (c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['ct'], c['dt'])
    got = to_host(bb, ft.partial_trace(bb, to_dev(bb, c['data']), *args))
    want = ref.partial_trace_ref(c['data'], *args)
    assert len(want) == 2                                    # the sectors 1 and 2
    assert all(np.iscomplexobj(b) == (cplx_data or cplx_factors) for b in got.values())
    N = ref.partial_trace_ref(c['data'], *args, count=True)
    assert_within(got, want, N, ref.partial_trace_ref(c['data'], *args, absolute=True))
    return c


def replace_tree(space: ft.TreeSpace, tree, **changes) -> ft.TreeSpace:
    """the space with some fields of one tree replaced (start / stop stay: the error paths never reach the blocks)"""
    blocks = [[dataclasses.replace(tb, **changes) if tb.tree == tree else tb for tb in tbs] for tbs in space.tree_blocks]
    return ft.TreeSpace(space.sectors, space.qdims, blocks, space.num_legs)
