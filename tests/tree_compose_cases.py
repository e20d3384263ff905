"""Inputs and checks of the fusion-tree partial_compose shared by tests/test_tree_compose.py (numpy stand-in: the record
building without a device) and tests/test_gpu_tree_compose.py (HipBlockBackend: the same inputs, the same criteria).

(a) abelian trees against the dense contraction -- the independent check: U(1) legs, every amplitude is 1, the new tree is the
    spliced one, and the answer is ``np.tensordot`` of the dense tensors.
(b) random made-up tables (complex amplitudes, several old and several new trees per lookup, terms of different K in one
    strip, empty lists, a strip without a term) against the restatement of the reference's loop, tests/tree_compose_ref.py.
(c) SU(2): a one-leg b at the last leg (tables from fusion rules alone: the two routes through the project agree), and the
    identity on 1/2 x 1/2 at leg 1 with F symbols (F unitarity: the result is a again).
(d) the placement of the conjugate, (e) errors, discard=False, empty operands, dtype, the TreeChainOperator step.

Tolerance.  An element is sum_t c_t sum_k A B with P products in total and n <= P terms.  A complex product is two real
products and one sum per component, the k sum adds one rounding per product, c_t times the sum two products and a sum, the
sum over t one rounding per term: no more than 2 P + 6 roundings of numbers whose absolute values sum to at most
S = sum_t |c|_1 sum_k |A|_1 |B|_1, |z|_1 = |re| + |im| (to first order in u = 2^-53; the slack of the count covers the second
order).  Either side is therefore componentwise within (2 P + 6) u S of exact, and two results differ by at most
2 (2 P + 6) u S.  P and S come from the restatement, or the dense contraction, run on ones and on the absolute values."""
import itertools

import numpy as np

import tree_compose_ref as ref
from cyten_amd import fusion_tree as ft
from cyten_amd import krylov
from tree_ops_cases import KeyedAbelianTrees, to_dev, to_host
from tree_outer_cases import NumpyOuterBackend, _dense_on, _fusion_table, _racah_F, _random_data, _spin_leg, _two_leg_space, abs1

U = 2.0 ** -53
KINDS = ['real', 'complex', 'mixed']                                               # mixed: real a, complex b
SIDES = ['domain', 'codomain']


class NumpyComposeBackend(NumpyOuterBackend):
    """the stand-in of the tree operations (a ``NumpyTreeBackend``; with the looped ``tree_outer_many``, for the check against
    compose with an outer) + a looped ``tree_compose_many``; remembers (strip shape, side, m0, m2, [K of every term]) of every
    record of every call"""

    def __init__(self):
        super().__init__()
        self.compose_calls = []

    def tree_compose_many(self, outputs):
        outputs = [(dst, side, m0, m2, list(terms)) for dst, side, m0, m2, terms in outputs]
        self.compose_calls.append([(tuple(dst.shape), side, m0, m2, [b.shape[0] if side == 'domain' else b.shape[1] for _, b, _ in terms])
                                   for dst, side, m0, m2, terms in outputs])
        for dst, side, m0, m2, terms in outputs:
            acc = np.zeros(dst.shape, dtype=dst.dtype)
            for a, b, coeff in terms:
                assert np.iscomplexobj(dst) or not (np.iscomplexobj(a) or np.iscomplexobj(b) or isinstance(coeff, complex))
                if side == 'domain':
                    (K, N), R = b.shape, a.shape[0]
                    s = np.einsum('rikj,kn->rinj', a.reshape(R, m0, K, m2), b).reshape(R, m0 * N * m2)
                else:
                    (N, K), Cc = b.shape, a.shape[1]
                    s = np.einsum('ikjc,nk->injc', a.reshape(m0, K, m2, Cc), b).reshape(m0 * N * m2, Cc)
                acc = acc + coeff * s
            dst[...] = acc


def bound_two(P, S):
    """two computed results of one element: 2 (2 P + 6) u S"""
    return 2 * (2 * np.asarray(P) + 6) * U * S


def assert_within(got: dict, want: dict, bound: dict):
    """the same coupled sectors, every element componentwise within its bound"""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and not np.isnan(g).any(), k
        assert np.all(np.abs(np.real(g) - np.real(w)) <= bound[k]) and np.all(np.abs(np.imag(g) - np.imag(w)) <= bound[k]), k


def run_compose(bb, c, **kw):
    return ft.partial_compose(bb, to_dev(bb, c['a']), c['a_cod'], c['a_dom'], to_dev(bb, c['b']), c['b_cod'], c['b_dom'], c['n_cod'], c['n_dom'],
                              c['insert'], **kw)


def run_ref(c, **kw):
    return ref.partial_compose_ref(c['a'], c['a_cod'], c['a_dom'], c['b'], c['b_cod'], c['b_dom'], c['n_cod'], c['n_dom'], c['insert'], **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees

# (side of a that is contracted, legs of that side before / after the contracted run, contracted legs of b, surviving legs of b)
ABELIAN_CONFIGS = [('domain', 0, 1, 1, 1), ('domain', 1, 1, 2, 1), ('domain', 1, 0, 1, 2), ('domain', 0, 0, 2, 2), ('domain', 1, 1, 2, 0),
                   ('codomain', 0, 1, 1, 1), ('codomain', 1, 1, 1, 2), ('codomain', 1, 0, 2, 1), ('codomain', 0, 0, 2, 2),
                   ('codomain', 1, 0, 2, 0)]


def abelian_case(rng, config, kind):
    side, n_before, n_after, n_contr, n_surv = config
    dom = side == 'domain'
    total = 2 + n_before + n_contr + n_after + n_surv
    want = {}
    for _ in range(500):            # (a b without surviving legs needs the charge 0 on its contracted legs: draw again)
        at = KeyedAbelianTrees(rng, J=total, K=0)
        f = iter(range(total))
        other, before, contr, after, surv = ([next(f) for _ in range(n)] for n in (2, n_before, n_contr, n_after, n_surv))
        mine, new_mine = before + contr + after, before + surv + after
        (acf, adf), (bcf, bdf), (ncf, ndf) = ((other, mine), (contr, surv), (other, new_mine)) if dom else \
            ((mine, other), (surv, contr), (new_mine, other))
        Ta = _dense_on(at, rng, acf, adf, kind == 'complex')
        Tb = _dense_on(at, rng, bcf, bdf, kind != 'real')
        a_cod, a_dom, a = at.to_blocks(Ta, acf, adf)
        b_cod, b_dom, b = at.to_blocks(Tb, bcf, bdf)
        a_axes, b_axes = [(acf + adf).index(x) for x in contr], [(bcf + bdf).index(x) for x in contr]
        n_rem, pos = Ta.ndim - n_contr, (2 + n_before if dom else n_before)
        perm = list(range(pos)) + list(range(n_rem, n_rem + n_surv)) + list(range(pos, n_rem))

        def blocks_of(Ta_, Tb_):
            """the dense contraction: the surviving axes of b take the place of the contracted axes of a"""
            _, _, d = at.to_blocks(np.tensordot(Ta_, Tb_, (a_axes, b_axes)).transpose(perm), ncf, ndf)
            return {tuple(r): blk for r, blk in zip(d.block_inds.tolist(), d.blocks)}

        want = blocks_of(Ta, Tb)
        if a.blocks and b.blocks and want:
            break
    assert want
    charge = lambda fs, idx: int(sum(at.legs[x][0][i] for x, i in zip(fs, idx)))       # noqa: E731
    mult = lambda fs, idx: int(np.prod([at.legs[x][1][i] for x, i in zip(fs, idx)], dtype=np.int64))   # noqa: E731
    every = lambda fs: itertools.product(*[range(len(at.legs[x][0])) for x in fs])     # noqa: E731
    present = sorted({int(b_dom.sectors[j][0]) for _, j in b.block_inds.tolist()})     # eff_space: the coupled sectors of b's blocks
    outer_trees, table = {}, {}
    for ib_ in every(before):
        for q in present:
            for ia_ in every(after):
                key = ('outer', ib_, q, ia_)
                c = charge(before, ib_) + q + charge(after, ia_)
                outer_trees.setdefault((c,), []).append((key, (q,), mult(before, ib_), mult(after, ia_)))
                for fs, spliced in ((contr, mine), (surv, new_mine)):
                    for idx in every(fs):
                        if charge(fs, idx) == q:
                            table[(key, (tuple(fs), idx))] = [((tuple(spliced), ib_ + idx + ia_), 1.0)]
    return dict(at=at, a=a, b=b, a_cod=a_cod, a_dom=a_dom, b_cod=b_cod, b_dom=b_dom, n_cod=at.space(ncf), n_dom=at.space(ndf),
                insert=ft.TreeInsert(side, n_before, outer_trees, table), want=want,
                P=blocks_of((Ta != 0).astype(float), (Tb != 0).astype(float)), S=blocks_of(abs1(Ta), abs1(Tb)))


def check_abelian(bb, rng, config, kind):
    c = abelian_case(rng, config, kind)
    got = run_compose(bb, c)
    assert got.block_inds.tolist() == sorted(got.block_inds.tolist())
    host = to_host(bb, got)
    assert all(np.iscomplexobj(blk) == (kind != 'real') for blk in host.values())
    assert_within(host, c['want'], {k: bound_two(c['P'][k], c['S'][k]) for k in c['want']})
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (b) made-up trees and random tables

def table_case(rng, side, cplx_a, cplx_b, cplx_amps=True):
    """Two coupled sectors, two outer trees each with their own (m_before, m_after) and b-sector.  b holds the sectors 0 (two
    trees of the contracted side with K = 1 and 2, two of the surviving side with N = 2 and 1) and 1 (K = 3; N = 2).  Every
    (outer tree, tree of b) owns two old or new trees and its lookup returns 0, 1 or 2 of them: both for the outer tree
    ('o', 0, 0) -- its new strips are fed by terms with K = 1 and K = 2 --, none for the old lookups of ('o', 1, 0), at least one
    for ('o', 1, 1).  Every
    coupled sector of the new space also holds one tree nothing feeds."""
    dom = side == 'domain'
    mk = ft.TreeSpace.from_multiplicities
    kept = mk([[0], [1]], [[(3,)], [(2,)]], None, 1, [[('kept', 0)], [('kept', 1)]])
    Ks, Ns = [[1, 2], [3]], [[2, 1], [2]]
    b_contr = mk([[0], [1]], [[(k,) for k in Ks[s]] for s in range(2)], None, 1, [[('bk', s, t) for t in range(len(Ks[s]))] for s in range(2)])
    b_surv = mk([[0], [1]], [[(n,) for n in Ns[s]] for s in range(2)], None, 1, [[('bn', s, t) for t in range(len(Ns[s]))] for s in range(2)])
    outers = {0: [(('o', 0, 0), 0, 2, 1), (('o', 0, 1), 1, 1, 3)], 1: [(('o', 1, 0), 1, 1, 1), (('o', 1, 1), 0, 2, 2)]}
    names = {'old': [[], []], 'new': [[], []]}
    mults = {'old': [[], []], 'new': [[], []]}
    table = {}
    for s in (0, 1):
        for key, bs, m0, m2 in outers[s]:
            for what, tag, sizes in (('old', 'bk', Ks[bs]), ('new', 'bn', Ns[bs])):
                for t, size in enumerate(sizes):
                    pair = [(what, key, t, v) for v in range(2)]
                    names[what][s] += pair
                    mults[what][s] += [(m0, size, m2)] * 2
                    k = 2 if key == ('o', 0, 0) else (0 if key == ('o', 1, 0) and what == 'old' else int(rng.integers(1 if key == ('o', 1, 1) else 0, 3)))
                    lst = []
                    for v in sorted(rng.choice(2, size=k, replace=False).tolist()):
                        amp = complex(rng.standard_normal(), rng.standard_normal() if cplx_amps else 0.0)
                        lst.append((pair[v], amp if cplx_amps else amp.real))
                    table[(key, (tag, bs, t))] = lst
        names['new'][s].append(('idle', s))
        mults['new'][s].append((2, 2))
    old_space = mk([[0], [1]], mults['old'], None, 3, names['old'])
    new_space = mk([[0], [1]], mults['new'], None, 3, names['new'])
    (a_cod, a_dom), (b_cod, b_dom), (n_cod, n_dom) = ((kept, old_space), (b_contr, b_surv), (kept, new_space)) if dom else \
        ((old_space, kept), (b_surv, b_contr), (new_space, kept))
    insert = ft.TreeInsert(side, 1, {(s,): [(key, (bs,), m0, m2) for key, bs, m0, m2 in outers[s]] for s in (0, 1)}, table)
    return dict(a=_random_data(rng, a_cod, a_dom, cplx_a), b=_random_data(rng, b_cod, b_dom, cplx_b), a_cod=a_cod, a_dom=a_dom,
                b_cod=b_cod, b_dom=b_dom, n_cod=n_cod, n_dom=n_dom, insert=insert)


def check_table(bb, rng, side, cplx_a, cplx_b, cplx_amps=True):
    c = table_case(rng, side, cplx_a, cplx_b, cplx_amps)
    got = to_host(bb, run_compose(bb, c))
    want = run_ref(c)
    assert len(want) == 2
    assert all(np.iscomplexobj(blk) == (cplx_a or cplx_b or cplx_amps) for blk in got.values())
    P, S = run_ref(c, count=True), run_ref(c, absolute=True)
    assert_within(got, want, {k: bound_two(P[k], S[k]) for k in want})
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (c) SU(2); sectors are 2 j

def su2_last_leg_case(rng, side, cplx):
    """a on (x, v (x) pc) and b: pc -> ps (domain), or a on (v (x) pc, x) and b: ps -> pc (codomain): the one-leg b sits at the
    last leg, its trees have no vertex, and ``insert_at`` returns the tree itself with the amplitude 1
    (src/symmetries/trees.cpp:1248-1255): the tables follow from the fusion rules alone"""
    dom = side == 'domain'
    V, Pc, Ps = _spin_leg('v', {0: 2, 1: 3, 2: 1}), _spin_leg('pc', {1: 2, 2: 3}), _spin_leg('ps', {1: 3, 2: 1})
    X = _spin_leg('x', {0: 2, 1: 1, 2: 3, 3: 2, 4: 1})
    OLD, NEW = _two_leg_space('old', V, Pc), _two_leg_space('new', V, Ps)
    outer_trees, table = {}, {}
    for (jv,), tv in zip(V.sectors.tolist(), V.tree_blocks):
        for e in (1, 2):
            for J in range(abs(jv - e), jv + e + 1, 2):
                key = ('o', jv, e, J)
                outer_trees.setdefault((J,), []).append((key, (e,), tv[0].multiplicities[0], 1))
                table[(key, ('pc', e))] = [(('old', jv, e, J), 1.0)]
                table[(key, ('ps', e))] = [(('new', jv, e, J), 1.0)]
    (a_cod, a_dom), (b_cod, b_dom), (n_cod, n_dom) = ((X, OLD), (Pc, Ps), (X, NEW)) if dom else ((OLD, X), (Ps, Pc), (NEW, X))
    return dict(a=_random_data(rng, a_cod, a_dom, cplx), b=_random_data(rng, b_cod, b_dom, cplx), a_cod=a_cod, a_dom=a_dom, b_cod=b_cod,
                b_dom=b_dom, n_cod=n_cod, n_dom=n_dom, insert=ft.TreeInsert(side, 1, outer_trees, table), V=V, OLD=OLD, NEW=NEW)


def check_su2_last_leg(bb, rng, side, cplx):
    """partial_compose(a, b) == compose(a, outer(id_v, b)) (domain) or compose(outer(id_v, b), a) (codomain), the tables of the
    outer being those of ``check_su2_interchange`` (fusion rules, amplitude 1).

    Bound.  The partial_compose route is within (2 P + 6) u S of exact (module docstring).  The other route: an element of
    outer(id_v, b) is 1 * 1 * b or 1 * 0 * b, exact; a (complex) dot product of length Kc of a with such numbers is within
    (2 Kc + 14) u S' whatever its order (the bound ``check_su2_interchange`` states for ``compose``), Kc the size of the coupled
    block of v (x) pc, and S' = sum |a|_1 |id_v (x) b|_1 = S, since the zeros of id_v (x) b contribute nothing.  So the two routes
    differ by at most ((2 P + 6) + (2 Kc + 14)) u S; P and S from the restatement."""
    c = su2_last_leg_case(rng, side, cplx)
    dom = side == 'domain'
    V, OLD, NEW = c['V'], c['OLD'], c['NEW']
    got = to_host(bb, run_compose(bb, c))
    idv = ft.FusionTreeData([(k, k) for k in range(V.num_sectors)], [bb.as_block(np.eye(V.block_size(k))) for k in range(V.num_sectors)])
    t_old, t_new = _fusion_table('old', V, c['b_cod' if dom else 'b_dom']), _fusion_table('new', V, c['b_dom' if dom else 'b_cod'])
    if dom:
        ob = ft.outer(bb, idv, V, V, to_dev(bb, c['b']), c['b_cod'], c['b_dom'], OLD, NEW, t_old, t_new)
        want = to_host(bb, ft.compose(bb, to_dev(bb, c['a']), ob))
    else:
        ob = ft.outer(bb, idv, V, V, to_dev(bb, c['b']), c['b_cod'], c['b_dom'], NEW, OLD, t_new, t_old)
        want = to_host(bb, ft.compose(bb, ob, to_dev(bb, c['a'])))
    P, S = run_ref(c, count=True), run_ref(c, absolute=True)
    assert len(want) == OLD.num_sectors >= 4
    bound = {}
    for k in want:
        Kc = OLD.block_size(k[1] if dom else k[0])                  # (old and new hold the same coupled sectors, in the same order)
        bound[k] = ((2 * P[k] + 6) + (2 * Kc + 14)) * U * S[k]
        assert np.iscomplexobj(got[k]) == cplx
    assert OLD.sectors.tolist() == NEW.sectors.tolist()
    assert_within(got, want, bound)
    return c


def su2_identity_case(rng, side, cplx, m=(2, 3)):
    """a on (x, v (x) 1/2 (x) 1/2) (or its mirror image), b = the identity on 1/2 (x) 1/2 with the multiplicities m, inserted at
    leg 1 of the outer trees (j_v, e; c).  Trees of the three-leg space: (j_v, 1/2, 1/2; inner f, coupled c); the amplitude of
    (j_v, e; c) with (1/2, 1/2; e) inserted on the tree (j_v, f; c) is F^{j_v 1/2 1/2}_c[f, e] from the Racah formula of
    scripts/make_su2_golden.py."""
    dom = side == 'domain'
    mv = {0: 2, 1: 1, 2: 2}
    pair = ft.TreeSpace.from_multiplicities([[0], [2]], [[tuple(m)], [tuple(m)]], np.array([1.0, 3.0]), 2, [[('b', 0)], [('b', 2)]],
                                            [[(1, 1)], [(1, 1)]])
    trees = {}                      # coupled 2c -> [(2 j_v, 2 f)]
    for jv in mv:
        for f in (jv - 1, jv + 1):
            for c in (f - 1, f + 1):
                if f >= 0 and c >= 0:
                    trees.setdefault(c, []).append((jv, f))
    cs = sorted(trees)
    T3 = ft.TreeSpace.from_multiplicities([[c] for c in cs], [[(mv[jv],) + tuple(m) for jv, _ in trees[c]] for c in cs],
                                          np.array([c + 1.0 for c in cs]), 3, [[('t', jv, f, c) for jv, f in trees[c]] for c in cs],
                                          [[(jv, 1, 1) for jv, _ in trees[c]] for c in cs])
    outer_trees, table = {}, {}
    for jv in mv:
        for e in (0, 2):
            for c in range(abs(jv - e), jv + e + 1, 2):
                key = ('o', jv, e, c)
                outer_trees.setdefault((c,), []).append((key, (e,), mv[jv], 1))
                table[(key, ('b', e))] = [(('t', jv, f, c), _racah_F(jv, 1, 1, c, f, e)) for jv_, f in trees[c] if jv_ == jv]
    X = _spin_leg('x', {c: 1 + c % 3 for c in cs})
    b = ft.FusionTreeData([(0, 0), (1, 1)], [np.eye(pair.block_size(i)) * (1 + 0j if cplx else 1) for i in range(2)])
    (a_cod, a_dom) = (X, T3) if dom else (T3, X)
    return dict(a=_random_data(rng, a_cod, a_dom, cplx), b=b, a_cod=a_cod, a_dom=a_dom, b_cod=pair, b_dom=pair, n_cod=a_cod, n_dom=a_dom,
                insert=ft.TreeInsert(side, 1, outer_trees, table))


def check_su2_identity(bb, rng, side, cplx):
    """a with the identity on 1/2 (x) 1/2 applied is a again, by the unitarity of F: sum_e F[f, e] F[f', e] = delta(f, f').

    Bound.  The computed result is within (2 P + 6) u S of the exact result FOR THE TABLE IN USE (module docstring).  The table
    holds every F symbol rounded to float64, relative error at most u / 2, so a coefficient F F' of the exact table differs
    from the one in use by at most (u + u^2 / 4) |F F'|, and the exact results of the two tables by at most 2 u S.  Against a
    itself: (2 P + 8) u S; P and S from the restatement."""
    c = su2_identity_case(rng, side, cplx)
    got = to_host(bb, run_compose(bb, c))
    want = {tuple(r): blk for r, blk in zip(c['a'].block_inds.tolist(), c['a'].blocks)}
    P, S = run_ref(c, count=True), run_ref(c, absolute=True)
    assert len(want) >= 4 and all(np.iscomplexobj(blk) == cplx for blk in got.values())
    assert_within(got, want, {k: (2 * P[k] + 8) * U * S[k] for k in want})
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the placement of the conjugate

def check_conjugate_placement(bb):
    """one outer tree, one tree everywhere, small integers: domain gives amp_old conj(amp_new) (:2817), codomain
    conj(amp_old) amp_new (:2847); compared with =="""
    mk = ft.TreeSpace.from_multiplicities
    kept, old, new = mk([[0]], [[(2,)]], None, 1, [['kept']]), mk([[0]], [[(1, 3, 1)]], None, 3, [['old']]), mk([[0]], [[(1, 2, 1)]], None, 3, [['new']])
    bk, bn = mk([[0]], [[(3,)]], None, 1, [['bk']]), mk([[0]], [[(2,)]], None, 1, [['bn']])
    A, B = np.arange(-3.0, 3.0).reshape(2, 3), np.array([[1.0, -2.0], [3.0, 5.0], [-1.0, 4.0]])
    for amp_old, amp_new in ((1j, 1.0), (1.0, 1j), (1j, 1j)):
        table = {('o', 'bk'): [('old', amp_old)], ('o', 'bn'): [('new', amp_new)]}
        trees = {(0,): [('o', (0,), 1, 1)]}
        got = ft.partial_compose(bb, ft.FusionTreeData([(0, 0)], [bb.as_block(A)]), kept, old, ft.FusionTreeData([(0, 0)], [bb.as_block(B)]), bk, bn,
                                 kept, new, ft.TreeInsert('domain', 0, trees, table))
        assert got.block_inds.tolist() == [[0, 0]]
        assert np.array_equal(bb.to_numpy(got.blocks[0]), (amp_old * np.conj(amp_new)) * (A @ B))
        got = ft.partial_compose(bb, ft.FusionTreeData([(0, 0)], [bb.as_block(np.ascontiguousarray(A.T))]), old, kept,
                                 ft.FusionTreeData([(0, 0)], [bb.as_block(np.ascontiguousarray(B.T))]), bn, bk,
                                 new, kept, ft.TreeInsert('codomain', 0, trees, table))
        assert np.array_equal(bb.to_numpy(got.blocks[0]), (np.conj(amp_old) * amp_new) * (B.T @ A.T))


# ---------------------------------------------------------------------------------------------------------------------------
# (e) discard, empty operands, the chain step

def check_discard_false_keeps_zero_blocks(bb, rng, side):
    """coupled sector 1 of b is zeroed and the outer trees of the coupled sector 0 of a lead there only: the result block of
    sector 0 is all zeros -- dropped by default, kept (and written, not left as allocated) with discard=False"""
    c = table_case(rng, side, False, False, cplx_amps=False)
    ot = dict(c['insert'].outer_trees)
    ot[(0,)] = [t for t in ot[(0,)] if t[1] == (1,)]
    c['insert'] = c['insert']._replace(outer_trees=ot)
    c['b'] = ft.FusionTreeData(c['b'].block_inds, [blk * (0.0 if n == 1 else 1.0) for n, blk in enumerate(c['b'].blocks)])
    kept = to_host(bb, run_compose(bb, c, discard=False))
    dropped = to_host(bb, run_compose(bb, c))
    assert sorted(kept) == [(0, 0), (1, 1)] and sorted(dropped) == [(1, 1)]
    assert np.all(kept[(0, 0)] == 0) and np.array_equal(kept[(1, 1)], dropped[(1, 1)])


def check_empty_operand(bb, rng, side):
    c = table_case(rng, side, False, False)
    empty = ft.FusionTreeData(np.zeros((0, 2), np.int64), [])
    for which in 'ab':
        got = run_compose(bb, dict(c, **{which: empty}))
        assert got.blocks == [] and got.block_inds.shape == (0, 2)


def check_chain_step(bb, rng, side):
    """the TreeChainOperator step equals the direct call, bit for bit; is_complex sees B's blocks and the amplitudes"""
    for cplx_b, cplx_amps in ((False, False), (True, False), (False, True)):
        c = table_case(rng, side, False, cplx_b, cplx_amps)
        step = ('partial_compose', to_dev(bb, c['b']), c['b_cod'], c['b_dom'], c['n_cod'], c['n_dom'], c['insert'])
        op = krylov.TreeChainOperator(bb, [step], c['a_cod'], c['a_dom'])
        assert op.is_complex == (cplx_b or cplx_amps)
        assert op.out_codomain is c['n_cod'] and op.out_domain is c['n_dom']
        y = op.matvec(ft.TreeTensor(to_dev(bb, c['a']), c['a_cod'], c['a_dom']))
        assert y.codomain is c['n_cod'] and y.domain is c['n_dom']
        got, want = to_host(bb, y.data), to_host(bb, run_compose(bb, c))
        assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)
    return c
