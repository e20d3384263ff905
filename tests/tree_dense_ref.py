"""numpy restatement of the two definitions of cyten_amd.fusion_tree.to_dense_block / from_dense_block (the loops of
``FusionTreeBackend::to_dense_block`` fusion_tree_backend.cpp:1856-1973 and ``::from_dense_block`` :1680-1853), one tree pair at a
time with ``einsum`` / ``tensordot``, in ``np.longdouble``.

The tree-pair tensor ``S[k_a..., k_b...] = sum_kc conj(X_alpha[k_a..., kc]) X_beta[k_b..., kc]`` is built in float64 by the same numpy
expression as in the module under test -- it is an input of both sides, its rounding is common to them -- and widened after.

``absolute=True`` runs the same sums on |S|_1 and |value|_1 (|z|_1 = |re| + |im|), ``count=True`` on ones: S and P of the bounds in
tests/tree_dense_cases.py."""
import numpy as np


def abs1(x):
    x = np.asarray(x)
    return np.abs(x.real) + np.abs(x.imag)


def leg_positions(dense):
    """per leg {sector key: (start, d, m)} and the dimension of every dense axis"""
    where, dims = [], []
    for leg in dense.legs:
        pos, off = {}, 0
        for key, m in leg:
            d = int(dense.sector_dims[key])
            pos[key] = (off, d, int(m))
            off += d * int(m)
        where.append(pos)
        dims.append(off)
    return where, dims


def pair_tensor(cod_dense, dom_dense, alpha, beta):
    return np.tensordot(np.conj(cod_dense.tensors[alpha]), dom_dense.tensors[beta], ([-1], [-1]))


def _mode(x, absolute, count):
    if count:
        return np.ones(np.shape(x), dtype=np.longdouble)
    if absolute:
        return abs1(x).astype(np.longdouble)
    return np.asarray(x).astype(np.clongdouble if np.iscomplexobj(x) else np.longdouble)


def _region(cw, dw, xa, yb):
    at = [cw[l][key] for l, key in enumerate(xa.uncoupled)] + [dw[l][key] for l, key in enumerate(yb.uncoupled)]
    sl = tuple(slice(s, s + d * m) for s, d, m in at)
    return sl, [d for _, d, _ in at], [m for _, _, m in at]


def to_dense(data, codomain, domain, cod_dense, dom_dense, absolute=False, count=False):
    """the dense tensor with the axes (codomain legs..., domain legs reversed), longdouble / clongdouble"""
    J, K = codomain.num_legs, domain.num_legs
    L = J + K
    (cw, cdims), (dw, ddims) = leg_positions(cod_dense), leg_positions(dom_dense)
    cplx = any(np.iscomplexobj(b) for b in data.blocks) or any(np.iscomplexobj(X) for td in (cod_dense, dom_dense) for X in td.tensors.values())
    res = np.zeros(cdims + ddims, dtype=np.clongdouble if cplx and not (absolute or count) else np.longdouble)
    for (i, j), blk in zip(data.block_inds.tolist(), data.blocks):
        for xa in codomain.tree_blocks[i]:
            for yb in domain.tree_blocks[j]:
                sl, dims, mults = _region(cw, dw, xa, yb)
                S = _mode(pair_tensor(cod_dense, dom_dense, xa.tree, yb.tree), absolute, count)
                T = _mode(np.asarray(blk)[xa.start:xa.stop, yb.start:yb.stop], absolute, count).reshape(mults)
                term = np.multiply.outer(S, T).transpose([p for l in range(L) for p in (l, L + l)])
                res[sl] += term.reshape([d * m for d, m in zip(dims, mults)])
    return res.transpose(list(range(J)) + list(range(L - 1, J - 1, -1)))


def from_dense(a, codomain, domain, cod_dense, dom_dense, absolute=False, count=False):
    """{(i, j): block} for every common coupled sector, longdouble / clongdouble; nothing is discarded"""
    from cyten_amd import fusion_tree as ft
    J, K = codomain.num_legs, domain.num_legs
    L = J + K
    (cw, _), (dw, _) = leg_positions(cod_dense), leg_positions(dom_dense)
    a = _mode(a, absolute, count).transpose(list(range(J)) + list(range(L - 1, J - 1, -1)))
    cplx = np.iscomplexobj(a) or any(np.iscomplexobj(X) for td in (cod_dense, dom_dense) for X in td.tensors.values())
    res = {}
    for i, j in ft.common_sectors(codomain, domain):
        blk = np.zeros((codomain.block_size(i), domain.block_size(j)), dtype=np.clongdouble if cplx and not (absolute or count) else np.longdouble)
        for xa in codomain.tree_blocks[i]:
            for yb in domain.tree_blocks[j]:
                sl, dims, mults = _region(cw, dw, xa, yb)
                S = pair_tensor(cod_dense, dom_dense, xa.tree, yb.tree)
                dc = cod_dense.tensors[xa.tree].shape[-1]
                S = _mode(S, absolute, count) if (absolute or count) else np.conj(_mode(S, False, False))
                region = a[sl].reshape([x for d, m in zip(dims, mults) for x in (d, m)])
                region = region.transpose([2 * l for l in range(L)] + [2 * l + 1 for l in range(L)])
                tile = np.tensordot(S, region, L) if L else S * region
                blk[xa.start:xa.stop, yb.start:yb.stop] = (tile / (1 if count else np.longdouble(dc))).reshape(xa.stop - xa.start, yb.stop - yb.start)
        res[(i, j)] = blk
    return res
