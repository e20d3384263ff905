"""Inputs and checks of ``fusion_tree.transform_tensor_factorized`` shared by tests/test_tree_strip.py (numpy stand-in: the
record building without a device) and tests/test_gpu_tree_strip.py (HipBlockBackend: the same inputs, the same criteria).

(a) the eight ``axis`` 0 / 1 cases of tests/golden/ref_tree_move_cases.json (Fibonacci and SU(3)_3 ``c_exchange_legs_*``), which
    the reference's tests write as strips: one tree per ``row_tree.width`` rows / ``col_tree.width`` columns, the strip map read
    off the statements, the permutation found as ``tree_move_fixture._axis_perm`` finds it.  Tolerance: the 1e-14 on uniform
    [0, 1) inputs those cases carry in tests/test_gpu_tree_moves.py.
(b) made-up spaces (three codomain legs, two domain legs, four coupled sectors; classes of two and three trees of equal
    multiplicities, so that a new tree has up to three old trees; a new tree without a term; a sector none of whose codomain
    strips has a term; a sector the old data lacks) against ``transform_tensor`` fed the multiplied-out pair mapping and
    against the restatement tests/tree_strip_ref.py.
      exact data -- integers in [-15, 15], coefficients from {1, -2, 0.5, i, -0.5i, 1 + i}, at most three terms per side: every
        product and sum is representable, the comparison is ``==``;
      ``standard_normal`` data against the ``np.longdouble`` evaluation of the restatement.  One pass of T terms: a term c x
        is two real products and a sum per component (or one product), within 2 u |c|_1 |x|_1 of its exact value, u = 2^-53; the
        T - 1 sums add u times the partial sums: |err| <= (T + 2) u sum_t |c_t|_1 |x_t|_1 componentwise.  Two passes: the second
        pass carries the error of the first through sums on absolute values and adds its own:
        |err| <= (T_c + T_d + 4) u sum_X sum_Y |a_X|_1 |b_Y|_1 |x|_1.  T_c / T_d are those of the element's own row / column strip.
(c) dtypes, identities, a braid and its inverse.     (d) error paths, the chain operator step."""
import numpy as np
import pytest

import tree_move_fixture as golden
import tree_strip_ref as ref
from cyten_amd import fusion_tree as ft
from cyten_amd import krylov
from tree_krylov_cases import NumpyKrylovBackend
from tree_ops_cases import to_dev, to_host

U = 2.0 ** -53
COEFFS = [1.0, -2.0, 0.5, 1j, -0.5j, 1 + 1j]


class NumpyStripBackend(NumpyKrylovBackend):
    """the stand-in of the tree operations (``empty_many`` hands out NaN) + ``transform_blocks`` + a looped ``tree_strip_many``;
    remembers per call the records as (block shape, side, start, stop, number of terms, whether every source is float64)"""

    def __init__(self):
        self.strip_calls = []

    def tree_strip_many(self, outs):
        outs = list(outs)
        self.strip_calls.append([(tuple(dst.shape), side, start, stop, len(terms), all(not np.iscomplexobj(t[0]) for t in terms))
                                 for dst, side, start, stop, _, _, terms in outs])
        for dst, side, start, stop, dims, axes, terms in outs:
            n, acc = stop - start, None
            for src, s0, c in terms:
                part = src[s0:s0 + n, :] if side == 0 else src[:, s0:s0 + n]
                v = part if c == 1 else c * part
                acc = v if acc is None else acc + v
            value = 0 if acc is None else ref.permute_combined_idx(acc, side, dims, axes)
            assert np.iscomplexobj(dst) or not np.iscomplexobj(value)
            if side == 0:
                dst[start:stop, :] = value
            else:
                dst[:, start:stop] = value


def strip_launches(bb, fn):
    """(result of fn(), the number of ``tree_strip_many`` calls it made): the stand-in's own list, a wrapper on a device backend"""
    if hasattr(bb, 'strip_calls'):
        n0 = len(bb.strip_calls)
        out = fn()
        return out, len(bb.strip_calls) - n0
    calls, orig = [], bb.tree_strip_many
    bb.tree_strip_many = lambda outs: (calls.append(1), orig(outs))[1]
    try:
        out = fn()
    finally:
        del bb.tree_strip_many
    return out, len(calls)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the golden strips

GOLDEN_CASES, SYM = golden.load()
STRIP_CASES = [c for c in GOLDEN_CASES if c['axis'] in (0, 1)]


def golden_setup(case):
    """(codomain, domain, new_codomain, new_domain, codomain_idcs, domain_idcs, splitting, fusion) of an ``axis`` 0 / 1 case: one
    coupled sector per block, one tree per `width` rows / columns with the multiplicities `dims`; the moved side's new trees
    carry the permuted multiplicities"""
    axis = case['axis']
    rt, ct = case['row_tree'], case['col_tree']
    d1, d2 = [int(d) for d in rt['dims']], [int(d) for d in ct['dims']]
    J, K = len(d1), len(d2)
    assert case['old_shapes'] == case['new_shapes']
    moved = rt if axis == 0 else ct
    w, dims = moved['width'], (d1, d2)[axis]
    table, perm = {}, None
    for st in case['statements']:
        nb, dst = st['nb'], st['dst']
        for i0 in range(0, len(dst), w):
            d = dst[i0:i0 + w]
            assert d == list(range(d[0], d[0] + w)) and d[0] % w == 0
            for t in st['terms']:
                assert t['ob'] == nb                                          # a braid stays inside its coupled sector
                s = t['src'][i0:i0 + w]
                base = min(s)
                assert base % w == 0
                p = golden._axis_perm(dims, [x - base for x in s])
                assert perm is None or perm == p
                perm = p
                targets = table.setdefault(('old', axis, nb, base // w), {})
                assert ('new', axis, nb, d[0] // w) not in targets
                targets[('new', axis, nb, d[0] // w)] = SYM[t['coeff']]
    n_blocks = len(case['old_shapes'])
    sectors = [[b] for b in range(n_blocks)]

    def space(side, kind, mults, width):
        per = [case['old_shapes'][b][side] // width for b in range(n_blocks)]
        return ft.TreeSpace.from_multiplicities(sectors, [[tuple(mults)] * n for n in per], None, len(mults),
                                                [[(kind, side, b, t) for t in range(n)] for b, n in enumerate(per)])

    cod, dom = space(0, 'old', d1, rt['width']), space(1, 'old', d2, ct['width'])
    new_dims = [dims[a] for a in perm]
    N = J + K
    if axis == 0:
        return cod, dom, space(0, 'new', new_dims, w), dom, perm, list(range(N - 1, J - 1, -1)), table, None
    return cod, dom, cod, space(1, 'new', new_dims, w), list(range(J)), [(N - 1) - a for a in perm], None, table


def check_golden(bb, rng, case, real):
    old = golden.inputs(case, rng, real=real)
    want, mask = golden.expected(case, SYM, old)
    cod, dom, n_cod, n_dom, c_idcs, d_idcs, splitting, fusion = golden_setup(case)
    n = len(old)
    data = ft.FusionTreeData([(b, b) for b in range(n)], [bb.as_block(o) for o in old])
    got, launches = strip_launches(bb, lambda: ft.transform_tensor_factorized(bb, data, cod, dom, n_cod, n_dom, c_idcs, d_idcs, splitting, fusion))
    assert launches == 1
    have = to_host(bb, got)
    cplx = not real or any(abs(SYM[t['coeff']].imag) > 0 for st in case['statements'] for t in st['terms'])
    assert any(m.any() for m in mask)
    for b in range(n):
        if (b, b) not in have:
            assert not mask[b].any()                                          # no statement names the block: every strip is empty
            continue
        g = have[(b, b)]
        assert np.iscomplexobj(g) == cplx and g.shape == want[b].shape and not np.isnan(g).any()
        assert np.abs(g - want[b])[mask[b]].max(initial=0.0) <= 1e-14
        assert np.abs(g[~mask[b]]).max(initial=0.0) == 0.0                    # a new tree without a term: zeros
    return have


# ---------------------------------------------------------------------------------------------------------------------------
# (b) made-up spaces

J, K = 3, 2
N = J + K
COD_MULTS = [[(2, 1, 3)] * 3 + [(1, 2, 2)] * 2, [(2, 3, 4)] * 2 + [(3, 1, 1)], [(1, 1, 2)] * 2, [(2, 2, 1)] * 2]
DOM_MULTS = [[(3, 2)] * 3 + [(1, 4)], [(2, 5)] * 2 + [(1, 1)], [(2, 2)], [(3, 1)] * 2]
SECTORS = [[0], [1], [2], [3]]
QDIMS = np.array([1.0, 2.0, 3.0, 1.5])
COD_PERMS = [[1, 0, 2], [0, 2, 1], [2, 0, 1], [1, 2, 0]]     # a swap beside the unit level, a swap, the two cyclic ones
DOM_AXES = [1, 0]
ABSENT = 3                                                   # the coupled sector the old data lacks
EMPTY = 2                                                    # the coupled sector none of whose codomain / domain strips has a term


def _spaces(kind, mults, axes):
    """(old space, new space): the new trees carry the multiplicities permuted by `axes`, in reversed order inside a sector"""
    n_legs = len(axes)
    old = ft.TreeSpace.from_multiplicities(SECTORS, mults, QDIMS, n_legs, [[(kind, s, t) for t in range(len(m))] for s, m in enumerate(mults)])
    new_m = [[tuple(m[a] for a in axes) for m in reversed(ms)] for ms in mults]
    new = ft.TreeSpace.from_multiplicities(SECTORS, new_m, QDIMS, n_legs, [[(kind.upper(), s, t) for t in range(len(m))] for s, m in enumerate(new_m)])
    return old, new


def _table(rng, old, new, axes, coeffs, skip_sector, skip_tree):
    """{old tree: {new tree: coefficient}}: per new tree 3, 1, 2, 3, .. of the old trees of its multiplicities (as many as there
    are), none for the new tree `skip_tree` and for the sector `skip_sector`; `coeffs`: a list to cycle through, or None for
    standard normal ones (complex if `coeffs` is the string 'complex')"""
    inv = ref.inverse_permutation(axes)
    table, k = {}, 0
    for s, tbs in enumerate(new.tree_blocks):
        if s == skip_sector:
            continue
        for t, x2 in enumerate(tbs):
            if x2.tree == skip_tree:
                continue
            want = tuple(x2.multiplicities[i] for i in inv)
            cand = [xb.tree for xb in old.tree_blocks[s] if tuple(xb.multiplicities) == want]
            T = min(len(cand), (3, 1, 2)[t % 3])
            for idx in rng.choice(len(cand), size=T, replace=False):
                if isinstance(coeffs, list):
                    c = coeffs[k % len(coeffs)]
                else:
                    c = rng.standard_normal() + (1j * rng.standard_normal() if coeffs == 'complex' else 0)
                table.setdefault(cand[idx], {})[x2.tree] = c
                k += 1
    return table


def product_mapping(cod, dom, splitting, fusion):
    """the two maps multiplied out into the data of a TreePairMapping; None: the identity over the trees of the old space"""
    a = splitting if splitting is not None else {tb.tree: {tb.tree: 1.0} for tbs in cod.tree_blocks for tb in tbs}
    b = fusion if fusion is not None else {tb.tree: {tb.tree: 1.0} for tbs in dom.tree_blocks for tb in tbs}
    mapping = {}
    for X, ta in a.items():
        sx = cod.tree_block_slice(X)[0]
        for Y, tb in b.items():
            if dom.tree_block_slice(Y)[0] != sx:
                continue
            mapping[(X, Y)] = {(x2, y2): ca * cb for x2, ca in ta.items() for y2, cb in tb.items()}
    return mapping


def table_case(rng, sides, cod_perm, exact, cplx_data, cplx_coeff):
    """sides: 'both', 'cod' (fusion None) or 'dom' (splitting None)"""
    cod, n_cod = _spaces('c', COD_MULTS, cod_perm)
    dom, n_dom = _spaces('d', DOM_MULTS, DOM_AXES)
    coeffs = (COEFFS if cplx_coeff else COEFFS[:3]) if exact else ('complex' if cplx_coeff else 'real')
    splitting = _table(rng, cod, n_cod, cod_perm, coeffs, EMPTY if sides != 'dom' else None, n_cod.tree_blocks[0][-1].tree)
    fusion = _table(rng, dom, n_dom, DOM_AXES, coeffs, EMPTY if sides == 'dom' else None, n_dom.tree_blocks[1][-1].tree)
    c_idcs, d_idcs = list(cod_perm), [(N - 1) - a for a in DOM_AXES]
    if sides == 'cod':
        fusion, n_dom, d_idcs = None, dom, list(range(N - 1, J - 1, -1))
    if sides == 'dom':
        splitting, n_cod, c_idcs = None, cod, list(range(J))
    rows, blocks = [], []
    for s in range(len(SECTORS)):
        if s == ABSENT:
            continue
        sh = (cod.block_size(s), dom.block_size(s))
        if exact:
            b = rng.integers(-15, 16, sh).astype(float) + (1j * rng.integers(-15, 16, sh) if cplx_data else 0)
        else:
            b = rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx_data else 0)
        rows.append((s, s)), blocks.append(b)
    data = ft.FusionTreeData(rows, blocks)
    return dict(data=data, cod=cod, dom=dom, n_cod=n_cod, n_dom=n_dom, c_idcs=c_idcs, d_idcs=d_idcs, splitting=splitting, fusion=fusion,
                cplx=cplx_data or cplx_coeff, sides=sides)


def run(bb, c, data=None):
    data = to_dev(bb, c['data']) if data is None else data
    return ft.transform_tensor_factorized(bb, data, c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['c_idcs'], c['d_idcs'], c['splitting'], c['fusion'])


def restated(c, **kw):
    return ref.transform_tensor(c['data'], c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['c_idcs'], c['d_idcs'], c['splitting'], c['fusion'], **kw)


def bound_factor(c, key):
    """T_c + T_d + 4 per element of the block `key` (T + 2 where one side is the identity)"""
    i, j = key
    tc, td = ref.term_counts(c['n_cod'], i, c['splitting']), ref.term_counts(c['n_dom'], j, c['fusion'])
    return tc[:, None] + td[None, :] + (4 if c['sides'] == 'both' else 2)


def within(got, want, bound):
    got = np.asarray(got)
    assert got.shape == want.shape and not np.isnan(got).any()
    err_re = np.abs((got.real.astype(np.longdouble) - want.real)).astype(np.float64)
    err_im = np.abs((got.imag.astype(np.longdouble) - want.imag)).astype(np.float64)
    assert np.all(err_re <= bound) and np.all(err_im <= bound), f'worst ratio {np.max(np.maximum(err_re, err_im) / np.maximum(bound, 1e-300)):.3g}'


SIDES = ['both', 'cod', 'dom']
KINDS = [(False, False), (False, True), (True, False), (True, True)]         # (complex data, complex coefficients)


def check_exact(bb, rng, sides, cod_perm, cplx_data, cplx_coeff):
    c = table_case(rng, sides, cod_perm, True, cplx_data, cplx_coeff)
    dev = to_dev(bb, c['data'])
    got, launches = strip_launches(bb, lambda: run(bb, c, dev))
    assert launches == (2 if sides == 'both' else 1)
    have = to_host(bb, got)
    pair = to_host(bb, ft.transform_tensor(bb, dev, c['cod'], c['dom'], c['n_cod'], c['n_dom'], c['c_idcs'], c['d_idcs'],
                                           product_mapping(c['cod'], c['dom'], c['splitting'], c['fusion'])))
    want = restated(c)
    assert sorted(have) == sorted(pair) == sorted(want) == [(0, 0), (1, 1)]           # EMPTY is dropped, ABSENT has no block
    assert got.block_inds.tolist() == sorted(got.block_inds.tolist())
    for k in want:
        assert np.iscomplexobj(have[k]) == c['cplx'] and not np.isnan(have[k]).any()
        assert np.array_equal(have[k], pair[k]) and np.array_equal(have[k], want[k]), k
    # the structure the case is about: three terms on a strip, a strip without a term (zeros)
    counts = [ref.term_counts(c['n_cod'], s, c['splitting']) for s in (0, 1)] + [ref.term_counts(c['n_dom'], s, c['fusion']) for s in (0, 1)]
    assert max(int(n.max(initial=0)) for n in counts) == 3
    if sides != 'dom':
        x2 = c['n_cod'].tree_blocks[0][-1]
        assert not have[(0, 0)][x2.start:x2.stop, :].any() and have[(0, 0)].any()
    if sides != 'cod':
        y2 = c['n_dom'].tree_blocks[1][-1]
        assert not have[(1, 1)][:, y2.start:y2.stop].any() and have[(1, 1)].any()
    return have


def check_rounded(bb, rng, sides, cod_perm, cplx_data, cplx_coeff):
    c = table_case(rng, sides, cod_perm, False, cplx_data, cplx_coeff)
    have = to_host(bb, run(bb, c))
    wide = restated(c, dtype=np.clongdouble if c['cplx'] else np.longdouble)
    S = restated(c, dtype=np.float64, absolute=True)
    assert sorted(have) == sorted(wide) == [(0, 0), (1, 1)]
    for k, w in wide.items():
        assert np.iscomplexobj(have[k]) == c['cplx']
        within(have[k], w, bound_factor(c, k) * U * S[k])
    return have


# ---------------------------------------------------------------------------------------------------------------------------
# (c) dtypes, identities, a braid and its inverse

def check_dtypes(bb, rng):
    """real data under real maps stays float64; under a complex map it becomes complex128 with the float64 blocks read as they
    stand: they are the sources of the first launch and hold what they held"""
    c = table_case(rng, 'both', COD_PERMS[0], True, False, False)
    assert all(b.dtype == np.float64 for b in to_host(bb, run(bb, c)).values())
    c = table_case(rng, 'both', COD_PERMS[0], True, False, True)
    dev = to_dev(bb, c['data'])
    have = to_host(bb, run(bb, c, dev))
    assert all(b.dtype == np.complex128 for b in have.values())
    for b, d in zip(c['data'].blocks, dev.blocks):
        back = np.asarray(bb.to_numpy(d))
        assert back.dtype == np.float64 and np.array_equal(back, b)
    if hasattr(bb, 'strip_calls'):
        first, second = bb.strip_calls[-2:]
        assert all(real for *_, n_terms, real in first if n_terms) and not any(real for *_, n_terms, real in second if n_terms)


def check_identities(bb, rng):
    """one side None: one launch; both None: no launch, the old block objects themselves"""
    for sides in ('cod', 'dom'):
        c = table_case(rng, sides, COD_PERMS[1], True, True, True)
        _, launches = strip_launches(bb, lambda: run(bb, c))
        assert launches == 1
    c = table_case(rng, 'cod', COD_PERMS[1], True, True, True)
    dev = to_dev(bb, c['data'])
    got, launches = strip_launches(bb, lambda: ft.transform_tensor_factorized(
        bb, dev, c['cod'], c['dom'], c['cod'], c['dom'], list(range(J)), list(range(N - 1, J - 1, -1)), None, None))
    assert launches == 0 and got.block_inds.tolist() == dev.block_inds.tolist()
    assert all(g is d for g, d in zip(got.blocks, dev.blocks))


# invertible maps between the trees of one class whose inverse is representable: the round trip is the identity in exact arithmetic
_A2, _A2_INV = np.array([[0.5, 0.5], [0.5, -0.5]]), np.array([[1.0, 1.0], [1.0, -1.0]])
_A3 = np.array([[1.0, 0.0, 0.0], [2.0, 1.0, 0.0], [-1.0, 0.5, 1.0]])
_A3_INV = np.array([[1.0, 0.0, 0.0], [-2.0, 1.0, 0.0], [2.0, -0.5, 1.0]])


def _invertible_tables(old, new, axes, phase):
    """(map old -> new, its inverse new -> old): per class of n = 1, 2, 3 trees `phase` times 1, _A2, _A3 / the inverses"""
    assert np.array_equal(_A2 @ _A2_INV, np.eye(2)) and np.array_equal(_A3 @ _A3_INV, np.eye(3))
    inv = ref.inverse_permutation(axes)
    fwd, back = {}, {}
    for s, tbs in enumerate(new.tree_blocks):
        classes = {}
        for x2 in tbs:
            classes.setdefault(tuple(x2.multiplicities[i] for i in inv), []).append(x2.tree)
        for want, news in classes.items():
            olds = [xb.tree for xb in old.tree_blocks[s] if tuple(xb.multiplicities) == want]
            n = len(olds)
            assert n == len(news) and n in (1, 2, 3)
            A, Ai = {1: (np.eye(1), np.eye(1)), 2: (_A2, _A2_INV), 3: (_A3, _A3_INV)}[n]
            for p, X in enumerate(olds):
                for q, x2 in enumerate(news):
                    if A[p, q] != 0:
                        fwd.setdefault(X, {})[x2] = phase * A[p, q]
                    if Ai[q, p] != 0:
                        back.setdefault(x2, {})[X] = Ai[q, p] / phase
    return fwd, back


def check_round_trip(bb, rng, cplx):
    """A braid followed by the inverse map gives the input back.  Bound: the first move's result is within k_1 u S_1 of its exact
    value (item (b), k_1 = T_c + T_d + 4 of the element, S_1 the sum on absolute values); the second move carries that error
    through its own sum on absolute values and adds k_2 u of it: |err| <= (max k_1 + k_2) u S, S the absolute evaluation of the
    second move on S_1."""
    perm = COD_PERMS[2]
    cod, n_cod = _spaces('c', COD_MULTS, perm)
    dom, n_dom = _spaces('d', DOM_MULTS, DOM_AXES)
    phase = 1j if cplx else 1.0
    a, a_inv = _invertible_tables(cod, n_cod, perm, phase)
    b, b_inv = _invertible_tables(dom, n_dom, DOM_AXES, phase)
    c_idcs, d_idcs = list(perm), [(N - 1) - x for x in DOM_AXES]
    c_back, d_back = ref.inverse_permutation(c_idcs), [(N - 1) - x for x in ref.inverse_permutation(DOM_AXES)]
    rows = [(s, s) for s in range(len(SECTORS)) if s != ABSENT]
    blocks = [rng.standard_normal((cod.block_size(s), dom.block_size(s))) + (1j * rng.standard_normal((cod.block_size(s), dom.block_size(s))) if cplx else 0)
              for s, _ in rows]
    data = ft.FusionTreeData(rows, blocks)
    mid = ft.transform_tensor_factorized(bb, to_dev(bb, data), cod, dom, n_cod, n_dom, c_idcs, d_idcs, a, b)
    got = to_host(bb, ft.transform_tensor_factorized(bb, mid, n_cod, n_dom, cod, dom, c_back, d_back, a_inv, b_inv))
    S1 = ref.transform_tensor(data, cod, dom, n_cod, n_dom, c_idcs, d_idcs, a, b, dtype=np.float64, absolute=True)
    S1 = ft.FusionTreeData(sorted(S1), [S1[k] for k in sorted(S1)])
    S = ref.transform_tensor(S1, n_cod, n_dom, cod, dom, c_back, d_back, a_inv, b_inv, dtype=np.float64, absolute=True)
    assert sorted(got) == sorted(rows) == sorted(S)
    k1 = 3 + 3 + 4
    for (s, _), x in zip(rows, blocks):
        k2 = ref.term_counts(cod, s, a_inv)[:, None] + ref.term_counts(dom, s, b_inv)[None, :] + 4
        assert np.iscomplexobj(got[(s, s)]) == cplx
        within(got[(s, s)], x.astype(np.clongdouble if cplx else np.longdouble), (k1 + k2) * U * S[(s, s)])


# ---------------------------------------------------------------------------------------------------------------------------
# (d) error paths, the chain operator

def check_errors(bb, rng):
    c = table_case(rng, 'both', COD_PERMS[0], True, False, False)
    dev = to_dev(bb, c['data'])

    def call(**kw):
        a = {**c, **kw}
        return ft.transform_tensor_factorized(bb, a.get('dev', dev), a['cod'], a['dom'], a['n_cod'], a['n_dom'], a['c_idcs'], a['d_idcs'],
                                              a['splitting'], a['fusion'])

    with pytest.raises(ValueError, match='mixes the sides'):
        call(c_idcs=[0, 1, 3])
    with pytest.raises(ValueError, match='mixes the sides'):
        call(c_idcs=[0, 1, 1])
    with pytest.raises(ValueError, match='mixes the sides'):
        call(d_idcs=[4, 2])
    with pytest.raises(ValueError, match='mixes the sides'):
        call(d_idcs=[4])
    some_new = c['n_cod'].tree_blocks[0][0]
    with pytest.raises(ValueError, match='holds no tree'):
        call(splitting={**c['splitting'], ('nowhere',): {some_new.tree: 1.0}})
    # an old tree of the sector 1 feeds a new tree of the sector 0
    with pytest.raises(ValueError, match='different coupled sectors'):
        call(splitting={**c['splitting'], c['cod'].tree_blocks[1][0].tree: {some_new.tree: 1.0}})
    # an old tree of the other class of the same sector
    inv = ref.inverse_permutation(c['c_idcs'])
    want = tuple(some_new.multiplicities[i] for i in inv)
    other = next(xb for xb in c['cod'].tree_blocks[0] if tuple(xb.multiplicities) != want)
    with pytest.raises(ValueError, match='has the multiplicities'):
        call(splitting={**c['splitting'], other.tree: {some_new.tree: 1.0}})
    with pytest.raises(ValueError, match='has the multiplicities'):
        d_new = c['n_dom'].tree_blocks[0][0]
        d_want = tuple(d_new.multiplicities[i] for i in ref.inverse_permutation(DOM_AXES))
        d_other = next(yb for yb in c['dom'].tree_blocks[0] if tuple(yb.multiplicities) != d_want)
        call(fusion={**c['fusion'], d_other.tree: {d_new.tree: 1.0}})
    # old blocks with a row or a column too few: a strip of an old tree leaves its block; an untouched side of another size
    cut_rows = ft.FusionTreeData(c['data'].block_inds, [bb.as_block(b[:-1, :]) for b in c['data'].blocks])
    cut_cols = ft.FusionTreeData(c['data'].block_inds, [bb.as_block(b[:, :-1]) for b in c['data'].blocks])
    with pytest.raises(ValueError, match='does not fit its block'):
        call(dev=cut_rows)
    with pytest.raises(ValueError, match='does not fit its block'):
        call(dev=cut_cols)
    one = table_case(rng, 'cod', COD_PERMS[0], True, False, False)
    with pytest.raises(ValueError, match='does not fit its block'):
        ft.transform_tensor_factorized(bb, cut_cols, one['cod'], one['dom'], one['n_cod'], one['n_dom'], one['c_idcs'], one['d_idcs'],
                                       one['splitting'], None)
    # more levels than the kernel takes
    seven = ft.TreeSpace.from_multiplicities([[0]], [[(1,) * 7]], None, 7, [['t']])
    leg = ft.TreeSpace.from_multiplicities([[0]], [[(1,)]], None, 1, [['y']])
    with pytest.raises(ValueError, match='at most 6'):
        ft.transform_tensor_factorized(bb, ft.FusionTreeData([(0, 0)], [bb.as_block(np.ones((1, 1)))]), seven, leg, seven, leg,
                                       list(range(7)), [7], {'t': {'t': 1.0}}, None)
    # after the refusals the same backend serves the valid call
    assert sorted(to_host(bb, call())) == [(0, 0), (1, 1)]


def check_chain_step(bb, rng, cplx):
    """a ``TreeChainOperator`` with a 'transform_factorized' step is the direct call"""
    c = table_case(rng, 'both', COD_PERMS[3], True, cplx, cplx)
    dev = to_dev(bb, c['data'])
    op = krylov.TreeChainOperator(bb, [('transform_factorized', c['n_cod'], c['n_dom'], c['c_idcs'], c['d_idcs'], c['splitting'], c['fusion'])],
                                  c['cod'], c['dom'])
    assert op.is_complex == cplx and op.out_codomain is c['n_cod'] and op.out_domain is c['n_dom']
    y = op.matvec(ft.TreeTensor(dev, c['cod'], c['dom']))
    direct = to_host(bb, run(bb, c, dev))
    got = to_host(bb, y.data)
    assert y.codomain is c['n_cod'] and y.domain is c['n_dom'] and sorted(got) == sorted(direct) and len(direct) == 2
    assert all(np.array_equal(got[k], direct[k]) for k in direct)
    with pytest.raises(ValueError, match='transform_factorized'):
        krylov.TreeChainOperator(bb, [('transform_factorized', c['n_cod'], c['n_dom'], c['c_idcs'], c['d_idcs'], c['splitting'])], c['cod'], c['dom'])
