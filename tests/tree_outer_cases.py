"""Inputs and checks of the fusion-tree outer shared by tests/test_tree_outer.py (numpy stand-in: the record building without
a device) and tests/test_gpu_tree_outer.py (HipBlockBackend: the same inputs, the same criteria).

(a) abelian trees against the dense tensor -- the independent check: U(1) legs, every amplitude is 1, the new tree is the
    concatenation, and the dense answer is the plain tensor product on the axes (a.cod, b.cod, a.dom, b.dom).
(b) random tables (complex amplitudes, several pairs per new tree, several coupled sectors per pair, empty lists) against
    the restatement of the reference's loop, tests/tree_outer_ref.py.
(c) SU(2): tables from fusion rules alone (one-leg right operand, every amplitude 1: the interchange law with compose) and
    from F symbols (identities on 1/2 x 1/2: F unitarity).      (d) a zero-leg operand.

Tolerance.  An element with n terms is sum_t c_t A_t B_t: two complex products per term and n - 1 additions.  Both sides are
within (n + 6) u S of the exact value, u = 2^-53, S = sum_t |c|_1 |A|_1 |B|_1 with |z|_1 = |re| + |im|, componentwise, so two such
results differ by at most 2 (n + 6) u S.  n and S come from the reference (dense or restated) run on ones and on the absolute
values."""
import functools
import os
import sys

import numpy as np

import tree_outer_ref as ref
from cyten_amd import fusion_tree as ft
from tree_ops_cases import KeyedAbelianTrees, NumpyTreeBackend, to_dev, to_host

U = 2.0 ** -53


class NumpyOuterBackend(NumpyTreeBackend):
    """the stand-in of the tree operations + a looped ``tree_outer_many``; remembers (tile shape, number of terms) of every
    record of every call"""

    def __init__(self):
        self.outer_calls = []

    def tree_outer_many(self, outputs):
        outputs = [(dst, list(terms)) for dst, terms in outputs]
        self.outer_calls.append([(tuple(dst.shape), len(terms)) for dst, terms in outputs])
        for dst, terms in outputs:
            acc = np.zeros(dst.shape, dtype=dst.dtype)
            for a, b, coeff in terms:
                assert np.iscomplexobj(dst) or not (np.iscomplexobj(a) or np.iscomplexobj(b) or isinstance(coeff, complex))
                acc = acc + coeff * np.kron(a, b)
            dst[...] = acc


def abs1(x):
    x = np.asarray(x)
    return np.abs(x.real) + np.abs(x.imag)


def assert_within(got: dict, want: dict, N: dict, S: dict, extra=0):
    """the same coupled sectors, every element componentwise within 2 (n + 6 + extra) u S"""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and not np.isnan(g).any(), k
        bound = 2 * (np.asarray(N[k]) + 6 + extra) * U * S[k]
        assert np.all(np.abs(np.real(g) - np.real(w)) <= bound) and np.all(np.abs(np.imag(g) - np.imag(w)) <= bound), k


def outer_args(c):
    return (c['a_cod'], c['a_dom']), (c['b_cod'], c['b_dom']), (c['n_cod'], c['n_dom'], c['ct'], c['dt'])


def run_outer(bb, c, **kw):
    (ac, ad), (bc, bd), rest = outer_args(c)
    return ft.outer(bb, to_dev(bb, c['a']), ac, ad, to_dev(bb, c['b']), bc, bd, *rest, **kw)


def run_ref(c, **kw):
    (ac, ad), (bc, bd), rest = outer_args(c)
    return ref.outer_ref(c['a'], ac, ad, c['b'], bc, bd, *rest, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees

ABELIAN_CONFIGS = [(1, 1, 1, 1), (2, 1, 1, 2), (2, 2, 1, 0), (0, 2, 2, 0)]         # (Ja, Ka, Jb, Kb)
KINDS = ['real', 'complex', 'mixed']                                               # mixed: real a, complex b


def _dense_on(at, rng, cod_f, dom_f, cplx):
    """charge-conserving dense tensor over the axes (cod_f..., dom_f...)"""
    fs = list(cod_f) + list(dom_f)
    dims = [int(at.legs[f][1].sum()) for f in fs]
    T = rng.standard_normal(dims) + (1j * rng.standard_normal(dims) if cplx else 0)
    grids = np.meshgrid(*[np.repeat(*at.legs[f]) for f in fs], indexing='ij') if fs else []
    tot = sum(grids[:len(cod_f)]) - sum(grids[len(cod_f):]) if fs else np.zeros(())
    return T * (tot == 0)


def _concat_table(at, fa, fb):
    """every pair of trees goes to the tree of the concatenated factors and sector indices, amplitude 1"""
    return ft.TreeOuter({(xa.tree, xb.tree): [((tuple(fa) + tuple(fb), xa.tree[1] + xb.tree[1]), 1.0)]
                         for ta in at.space(fa).tree_blocks for xa in ta for tb in at.space(fb).tree_blocks for xb in tb})


def abelian_case(rng, config, kind):
    Ja, Ka, Jb, Kb = config
    J, K = Ja + Jb, Ka + Kb
    for _ in range(100):            # (an operand with legs on one side only needs the charge 0 there: draw again)
        at = KeyedAbelianTrees(rng, J=J, K=K)
        acf, bcf = list(range(Ja)), list(range(Ja, J))
        adf, bdf = list(range(J, J + Ka)), list(range(J + Ka, J + K))
        Ta = _dense_on(at, rng, acf, adf, kind == 'complex')
        Tb = _dense_on(at, rng, bcf, bdf, kind != 'real')
        a_cod, a_dom, a = at.to_blocks(Ta, acf, adf)
        b_cod, b_dom, b = at.to_blocks(Tb, bcf, bdf)
        if a.blocks and b.blocks:
            break
    perm = list(range(Ja)) + list(range(Ja + Ka, Ja + Ka + Jb)) + list(range(Ja, Ja + Ka)) + list(range(Ja + Ka + Jb, J + K))
    cf, df = list(range(J)), list(range(J, J + K))

    def blocks_of(Ta_, Tb_):
        _, _, d = at.to_blocks(np.multiply.outer(Ta_, Tb_).transpose(perm), cf, df)
        return {tuple(r): blk for r, blk in zip(d.block_inds.tolist(), d.blocks)}

    return dict(at=at, a=a, b=b, a_cod=a_cod, a_dom=a_dom, b_cod=b_cod, b_dom=b_dom, n_cod=at.space(cf), n_dom=at.space(df),
                ct=_concat_table(at, acf, bcf), dt=_concat_table(at, adf, bdf), want=blocks_of(Ta, Tb), S=blocks_of(abs1(Ta), abs1(Tb)),
                Ja=Ja, Ka=Ka)


def check_abelian(bb, rng, config, kind):
    """-> (case, number of tiles whose a-side charges disagree: they were asserted to be zeros)"""
    c = abelian_case(rng, config, kind)
    got = run_outer(bb, c)
    assert len(c['want']) > 0
    assert got.block_inds.tolist() == sorted(got.block_inds.tolist())
    host = to_host(bb, got)
    assert all(np.iscomplexobj(blk) == (kind != 'real') for blk in host.values())
    assert_within(host, c['want'], {k: 1 for k in c['want']}, c['S'])
    at, Ja, Ka, disagree = c['at'], c['Ja'], c['Ka'], 0
    for (i, j), blk in host.items():
        for xb in c['n_cod'].tree_blocks[i]:
            for yb in c['n_dom'].tree_blocks[j]:
                qc = sum(int(at.legs[f][0][k]) for f, k in zip(xb.tree[0][:Ja], xb.tree[1][:Ja]))
                qd = sum(int(at.legs[f][0][k]) for f, k in zip(yb.tree[0][:Ka], yb.tree[1][:Ka]))
                if qc != qd:
                    disagree += 1
                    assert np.all(blk[xb.start:xb.stop, yb.start:yb.stop] == 0)
    return c, disagree


# ---------------------------------------------------------------------------------------------------------------------------
# (b) made-up trees and random tables

def _table_side(rng, tag, cplx_amps):
    """spaces of one leg for a and b (sectors 0 and 1, two trees each, multiplicities 1 or 2) and the new space of two legs
    (sectors 0, 1, 2).  A pair of trees goes to zero, one or two coupled sectors; the new tree of a sector is decided by the
    multiplicities of the pair, so that several pairs share one new tree.  Every sector of the new space also holds one tree
    nothing feeds.  The first pair goes to two sectors, the second one to none."""
    def leg(who):
        mults = [[(int(rng.integers(1, 3)),) for _ in range(2)] for _ in range(2)]
        names = [[(tag, who, s, t) for t in range(2)] for s in range(2)]
        return ft.TreeSpace.from_multiplicities([[0], [1]], mults, None, 1, names)

    sa, sb = leg('a'), leg('b')
    table, fed = {}, {s: [] for s in range(3)}
    pairs = [(xa, xb) for ta in sa.tree_blocks for xa in ta for tb in sb.tree_blocks for xb in tb]
    for n, (xa, xb) in enumerate(pairs):
        k = 2 if n == 0 else (0 if n == 1 else int(rng.integers(0, 3)))
        lst = []
        for s in sorted(rng.choice(3, size=k, replace=False).tolist()):
            m = xa.multiplicities + xb.multiplicities
            if m not in fed[s]:
                fed[s].append(m)
            amp = complex(rng.standard_normal(), rng.standard_normal() if cplx_amps else 0.0)
            lst.append(((tag, 'new', s, m), amp if cplx_amps else amp.real))
        table[(xa.tree, xb.tree)] = lst
    mults = [fed[s] + [(3, 1)] for s in range(3)]
    names = [[(tag, 'new', s, m) for m in fed[s]] + [(tag, 'idle', s)] for s in range(3)]
    new = ft.TreeSpace.from_multiplicities([[0], [1], [2]], mults, None, 2, names)
    return sa, sb, new, ft.TreeOuter(table)


def _random_data(rng, cod, dom, cplx):
    rows, blocks = [], []
    for i, j in ft.common_sectors(cod, dom):
        sh = (cod.block_size(i), dom.block_size(j))
        rows.append((i, j))
        blocks.append(rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0))
    return ft.FusionTreeData(rows, blocks)


def table_case(rng, cplx_a, cplx_b, cplx_amps=True):
    a_cod, b_cod, n_cod, ct = _table_side(rng, 'c', cplx_amps)
    a_dom, b_dom, n_dom, dt = _table_side(rng, 'd', cplx_amps)
    return dict(a=_random_data(rng, a_cod, a_dom, cplx_a), b=_random_data(rng, b_cod, b_dom, cplx_b), a_cod=a_cod, a_dom=a_dom,
                b_cod=b_cod, b_dom=b_dom, n_cod=n_cod, n_dom=n_dom, ct=ct, dt=dt)


def check_table(bb, rng, cplx_a, cplx_b, cplx_amps=True):
    c = table_case(rng, cplx_a, cplx_b, cplx_amps)
    got = to_host(bb, run_outer(bb, c))
    want = run_ref(c)
    assert len(want) >= 2
    assert all(np.iscomplexobj(blk) == (cplx_a or cplx_b or cplx_amps) for blk in got.values())
    assert_within(got, want, run_ref(c, count=True), run_ref(c, absolute=True))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (c) SU(2); sectors are 2 j

@functools.lru_cache(maxsize=None)
def _racah_F(a2, b2, c2, J2, e2, f2):
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts')
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    from make_su2_golden import racah_F
    return racah_F(a2, b2, c2, J2, e2, f2)


def _spin_leg(tag, mults: dict):
    """one-leg space: sector 2j with the multiplicity mults[2j], one tree each"""
    js = sorted(mults)
    return ft.TreeSpace.from_multiplicities([[j] for j in js], [[(mults[j],)] for j in js], np.array([j + 1.0 for j in js]), 1,
                                            [[(tag, j)] for j in js], [[(j,)] for j in js])


def _two_leg_space(tag, left: ft.TreeSpace, right: ft.TreeSpace):
    """left (x) right by the SU(2) fusion rules: a tree (ja, jb; J) for every J in |ja - jb| .. ja + jb"""
    by_J: dict = {}
    for (ja,), ta in zip(left.sectors.tolist(), left.tree_blocks):
        for (jb,), tb in zip(right.sectors.tolist(), right.tree_blocks):
            for J in range(abs(ja - jb), ja + jb + 1, 2):
                by_J.setdefault(J, []).append(((tag, ja, jb, J), ta[0].multiplicities + tb[0].multiplicities, (ja, jb)))
    Js = sorted(by_J)
    return ft.TreeSpace.from_multiplicities([[J] for J in Js], [[m for _, m, _ in by_J[J]] for J in Js], np.array([J + 1.0 for J in Js]), 2,
                                            [[k for k, _, _ in by_J[J]] for J in Js], [[u for _, _, u in by_J[J]] for J in Js])


def _fusion_table(tag, left: ft.TreeSpace, right: ft.TreeSpace):
    """the right tree has no vertex: ``insert_at`` returns the amplitude 1 for every new coupled sector
    (src/symmetries/trees.cpp:1248-1258 under ``FusionTree::outer`` :1382-1391)"""
    return ft.TreeOuter({(ta[0].tree, tb[0].tree): [((tag, ja, jb, J), 1.0) for J in range(abs(ja - jb), ja + jb + 1, 2)]
                         for (ja,), ta in zip(left.sectors.tolist(), left.tree_blocks)
                         for (jb,), tb in zip(right.sectors.tolist(), right.tree_blocks)})


def check_su2_interchange(bb, rng, cplx):
    """compose(outer(a, b), outer(a2, b2)) == outer(compose(a, a2), compose(b, b2)) for a: X -> Y, a2: Y -> Z, b: X' -> Y',
    b2: Y' -> Z' on one-leg SU(2) spaces.

    Bound.  Left: an element of outer has one term and is within 7 u |p|_1 of exact (module docstring); a (complex) dot product
    of length K of such numbers is within (2 K + 14) u sum |p|_1 |q|_1 whatever its order (2 K real products and their sums
    per component).  Right: the two small products are within 2 K_a u and 2 K_b u of exact, K_a + K_b <= K + 1, and the outer
    of them adds 7 u: within (2 K + 9) u of the same sum.  So the two differ by at most 2 (2 K + 14) u S, S = sum |p|_1 |q|_1
    over the inner index of the coupled block, K its extent."""
    X, Y, Z = _spin_leg('x', {0: 2, 1: 3, 2: 1}), _spin_leg('y', {0: 1, 1: 2, 2: 3}), _spin_leg('z', {0: 3, 1: 1, 2: 2})
    X2, Y2, Z2 = _spin_leg('x2', {1: 2, 2: 2}), _spin_leg('y2', {1: 3, 2: 1}), _spin_leg('z2', {1: 1, 2: 2})
    a, a2 = _random_data(rng, X, Y, cplx), _random_data(rng, Y, Z, cplx)
    b, b2 = _random_data(rng, X2, Y2, cplx), _random_data(rng, Y2, Z2, cplx)
    XX, YY, ZZ = _two_leg_space('xx', X, X2), _two_leg_space('yy', Y, Y2), _two_leg_space('zz', Z, Z2)
    tx, ty, tz = _fusion_table('xx', X, X2), _fusion_table('yy', Y, Y2), _fusion_table('zz', Z, Z2)
    dev = lambda t: to_dev(bb, t)                                                      # noqa: E731
    left = ft.compose(bb, ft.outer(bb, dev(a), X, Y, dev(b), X2, Y2, XX, YY, tx, ty),
                      ft.outer(bb, dev(a2), Y, Z, dev(b2), Y2, Z2, YY, ZZ, ty, tz))
    right = ft.outer(bb, ft.compose(bb, dev(a), dev(a2)), X, Z, ft.compose(bb, dev(b), dev(b2)), X2, Z2, XX, ZZ, tx, tz)
    P = ref.outer_ref(a, X, Y, b, X2, Y2, XX, YY, tx, ty, absolute=True)
    Q = ref.outer_ref(a2, Y, Z, b2, Y2, Z2, YY, ZZ, ty, tz, absolute=True)
    got, want = to_host(bb, left), to_host(bb, right)
    assert sorted(got) == sorted(want) and len(want) == XX.num_sectors >= 4
    for k, w in want.items():
        K = YY.block_size(k[0])
        bound = 2 * (2 * K + 14) * U * (P[k] @ Q[k])
        g = got[k]
        assert np.iscomplexobj(g) == cplx and g.shape == w.shape
        assert np.all(np.abs(g.real - w.real) <= bound) and np.all(np.abs(g.imag - w.imag) <= bound), k
    assert max(len(t) for t in XX.tree_blocks) >= 3                                    # several trees per coupled sector


def su2_identity_case(m):
    """a = b = the identity on 1/2 x 1/2 with the leg multiplicities m = (m1, m2, m3, m4); four-leg trees (1/2, 1/2, 1/2, 1/2;
    inner ca, f; coupled c).  The amplitude of (1/2, 1/2 -> ca) (x) (1/2, 1/2 -> cb) -> (ca, f; c) is F^{ca 1/2 1/2}_c[cb, f] from
    the Racah formula of scripts/make_su2_golden.py."""
    def pair_space(tag, m1, m2):
        return ft.TreeSpace.from_multiplicities([[0], [2]], [[(m1, m2)], [(m1, m2)]], np.array([1.0, 3.0]), 2, [[(tag, 0)], [(tag, 2)]],
                                                [[(1, 1)], [(1, 1)]])

    sa, sb = pair_space('a', m[0], m[1]), pair_space('b', m[2], m[3])
    trees = {}                      # coupled 2c -> [(2ca, 2f)]
    for ca in (0, 2):
        for f in ([1] if ca == 0 else [1, 3]):
            for c in (f - 1, f + 1):
                trees.setdefault(c, []).append((ca, f))
    cs = sorted(trees)
    new = ft.TreeSpace.from_multiplicities([[c] for c in cs], [[tuple(m)] * len(trees[c]) for c in cs], np.array([c + 1.0 for c in cs]), 4,
                                           [[('t', ca, f, c) for ca, f in trees[c]] for c in cs], [[(1, 1, 1, 1)] * len(trees[c]) for c in cs])
    table = {}
    for ca in (0, 2):
        for cb in (0, 2):
            table[(('a', ca), ('b', cb))] = [(('t', ca, f, c), _racah_F(ca, 1, 1, c, f, cb)) for c in cs for ca_, f in trees[c]
                                            if ca_ == ca and abs(ca - cb) <= c <= ca + cb]
    eye = lambda sp: ft.FusionTreeData([(0, 0), (1, 1)], [np.eye(sp.block_size(i)) for i in range(2)])   # noqa: E731
    return dict(a=eye(sa), b=eye(sb), a_cod=sa, a_dom=sa, b_cod=sb, b_dom=sb, n_cod=new, n_dom=new, ct=ft.TreeOuter(table),
                dt=ft.TreeOuter(table))


def check_su2_identity(bb, m):
    """id (x) id = id in every coupled block, by the unitarity of F, to 1e-14.  The check does not see which index of F is e
    and which is f: transposing an orthogonal matrix leaves it orthogonal.  (The placement of the conjugate is pinned by the
    coefficient test, the index order by the reference's ``insert_at``.)"""
    c = su2_identity_case(m)
    got = to_host(bb, run_outer(bb, c))
    assert sorted(got) == [(0, 0), (1, 1), (2, 2)]
    sizes = [2, 3, 1]
    for k, blk in got.items():
        n = sizes[k[0]] * int(np.prod(m))
        assert blk.shape == (n, n) and not np.iscomplexobj(blk)
        assert np.abs(blk - np.eye(n)).max() <= 1e-14
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# (d) a zero-leg operand

def check_zero_leg(bb, rng, cplx):
    """b on spaces without legs holds the 1 x 1 block [[s]]: the result is s a, on a's own spaces"""
    c = table_case(rng, cplx, False)
    one = ft.TreeSpace.from_multiplicities([[0]], [[()]], None, 0, [['e']], [[()]])
    s = (0.75 - 1.5j) if cplx else -1.25
    for sp in (c['a_cod'], c['a_dom']):
        assert all(tb.multiplicities + () == tb.multiplicities for tbs in sp.tree_blocks for tb in tbs)
    ident = lambda sp: ft.TreeOuter({(tb.tree, 'e'): [(tb.tree, 1.0)] for tbs in sp.tree_blocks for tb in tbs})   # noqa: E731
    b = ft.FusionTreeData([(0, 0)], [np.array([[s]])])
    got = ft.outer(bb, to_dev(bb, c['a']), c['a_cod'], c['a_dom'], to_dev(bb, b), one, one, c['a_cod'], c['a_dom'],
                   ident(c['a_cod']), ident(c['a_dom']))
    want = {tuple(r): s * blk for r, blk in zip(c['a'].block_inds.tolist(), c['a'].blocks)}
    S = {tuple(r): abs1(s) * abs1(blk) for r, blk in zip(c['a'].block_inds.tolist(), c['a'].blocks)}
    assert_within(to_host(bb, got), want, {k: 1 for k in want}, S)
