"""Plain-numpy statement of leg pipes, ``combine_legs`` and ``split_legs`` on ``cyten_amd.workloads.TensorSpec`` data: the
structural reference (pipes, block tables, legs, ``num_codomain``) of ``tests/test_leg_pipes.py`` and the producer of the
expected blocks of the GPU tests.  Everything goes through DENSE arrays and explicit loops over basis states and sector
combinations -- no strides, no placement tables -- so that it shares no mechanism with ``cyten_amd.abelian``.

Conventions: every leg carries a sign, charge rule sum_k sign_k q_k = 0; sector ``Q`` of a pipe satisfies
``sign * Q = sum_k sign_k q_k`` under the moduli."""
import itertools
from dataclasses import dataclass, field

import numpy as np

from abelian_tensor_ref import _reduced, _slices, to_dense
from cyten_amd import workloads as wl


@dataclass
class PipeSpec(wl.LegSpec):
    legs: list = field(default_factory=list)
    cstyle: bool = True
    block_ind_map: np.ndarray = None
    block_ind_map_slices: np.ndarray = None
    basis_perm: np.ndarray = None


def _combinations(legs, cstyle):
    """sector-index combinations in C order (last leg fastest) or F order (first leg fastest)"""
    ranges = [range(len(l.mults)) for l in legs]
    if cstyle:
        return list(itertools.product(*ranges))
    return [c[::-1] for c in itertools.product(*ranges[::-1])]


def make_pipe(moduli, legs, sign=+1, cstyle=True) -> PipeSpec:
    combos = _combinations(legs, cstyle)
    charge = {}
    for c in combos:
        q = np.zeros(len(moduli), dtype=np.int64)
        for l, i in zip(legs, c):
            q = q + l.sign * l.sectors[i]
        charge[c] = tuple(int(x) for x in _reduced(sign * q, moduli))
    sectors = sorted(set(charge.values()), key=lambda q: q[::-1])       # last column is the primary key, as for every leg
    fill = [0] * len(sectors)
    rows = []
    for c in combos:
        J = sectors.index(charge[c])
        size = int(np.prod([int(l.mults[i]) for l, i in zip(legs, c)], dtype=np.int64))
        rows.append((fill[J], fill[J] + size) + tuple(c) + (J,))
        fill[J] += size
    # sorted by J, the order inside a J kept (Python's sort is stable)
    rows.sort(key=lambda r: r[-1])
    bim = np.array(rows, dtype=np.int64).reshape(len(rows), len(legs) + 3)
    bim_slices = np.array([sum(1 for r in rows if r[-1] < J) for J in range(len(sectors) + 1)], dtype=np.int64)
    # basis states: one after the other, in the order the pipe lists them
    dims = [int(l.mults.sum()) for l in legs]
    sl = [_slices(l) for l in legs]
    offsets = np.concatenate([[0], np.cumsum(fill)]).astype(int)
    perm = np.full(int(sum(fill)), -1, dtype=np.int64)
    for r in rows:
        start, c, J = r[0], r[2:-1], r[-1]
        inner = [range(int(l.mults[i])) for l, i in zip(legs, c)]
        states = list(itertools.product(*inner)) if cstyle else [s[::-1] for s in itertools.product(*inner[::-1])]
        for n_state, s in enumerate(states):
            dense_index = tuple(int(sl[k][c[k]]) + s[k] for k in range(len(legs)))
            perm[offsets[J] + start + n_state] = np.ravel_multi_index(dense_index, dims) if dims else 0
    return PipeSpec(np.array(sectors, dtype=np.int64).reshape(len(sectors), len(moduli)), np.array(fill, dtype=np.int64), sign,
                    list(legs), cstyle, bim, bim_slices, perm)


def dual_pipe(moduli, pipe: PipeSpec) -> PipeSpec:
    return make_pipe(moduli, [wl.flip(l) if not isinstance(l, PipeSpec) else dual_pipe(moduli, l) for l in pipe.legs], -pipe.sign,
                     pipe.cstyle)


def result_layout(n, groups):
    """[(group number or None, source legs)] in result order: a pipe stands where the first-listed leg of its group stood"""
    first = {g[0]: k for k, g in enumerate(groups)}
    grouped = {i for g in groups for i in g}
    out = []
    for i in range(n):
        if i in first:
            out.append((first[i], list(groups[first[i]])))
        elif i not in grouped:
            out.append((None, [i]))
    return out


def dense_combine(dense, layout, pipes):
    """take(dense.transpose(order).reshape(merged), basis_perm) along every combined axis"""
    order = [i for _, src in layout for i in src]
    x = dense.transpose(order)
    merged = [int(np.prod([dense.shape[i] for i in src], dtype=np.int64)) for _, src in layout]
    x = x.reshape(merged)
    for axis, (g, _) in enumerate(layout):
        if g is not None:
            x = np.take(x, pipes[g].basis_perm, axis=axis)
    return x


def _cut(moduli, legs, dense, rows, num_codomain):
    rows = sorted(set(map(tuple, rows)), key=lambda r: r[::-1])
    sl = [_slices(l) for l in legs]
    blocks = [np.array(dense[tuple(slice(sl[k][i], sl[k][i + 1]) for k, i in enumerate(row))], copy=True) for row in rows]
    return wl.TensorSpec(tuple(moduli), list(legs), np.array(rows, dtype=np.int64).reshape(len(rows), len(legs)), blocks, num_codomain)


def combine(t, groups, signs=None, cstyle=True, pipes=None, num_codomain=None):
    """(result TensorSpec, pipes).  Block table: the rows the old blocks land in; blocks: cut out of the dense result."""
    n = len(t.legs)
    groups = [[int(i) % n for i in g] for g in groups]
    styles = [cstyle] * len(groups) if isinstance(cstyle, bool) else list(cstyle)
    signs = [+1] * len(groups) if signs is None else list(signs)
    if pipes is None:
        pipes = [make_pipe(t.moduli, [t.legs[i] for i in g], sg, cs) for g, sg, cs in zip(groups, signs, styles)]
    layout = result_layout(n, groups)
    legs = [t.legs[src[0]] if g is None else pipes[g] for g, src in layout]
    rows = []
    for row in t.block_inds.tolist():
        new = []
        for g, src in layout:
            if g is None:
                new.append(row[src[0]])
            else:
                want = [row[i] for i in src]
                hit = [r for r in pipes[g].block_ind_map.tolist() if r[2:-1] == want]
                assert len(hit) == 1
                new.append(hit[0][-1])
        rows.append(new)
    if num_codomain is None:
        num_codomain = sum(1 for _, src in layout if src[0] < t.num_codomain)
    dtype = complex if any(np.iscomplexobj(b) for b in t.blocks) else float
    dense = dense_combine(to_dense(t, dtype), layout, pipes)
    return _cut(t.moduli, legs, dense, rows, num_codomain), pipes


def dense_split(dense, legs, split):
    """the inverse of dense_combine on the axes `split` (pipes of `legs`), constituents in place"""
    shape = []
    for i, l in enumerate(legs):
        shape += [int(c.mults.sum()) for c in l.legs] if i in split else [int(l.mults.sum())]
    x = dense
    for i in split:
        inv = np.argsort(legs[i].basis_perm)
        x = np.take(x, inv, axis=i)
    return x.reshape(shape)


def split(t, leg_idcs=None):
    """every old block yields one new block per element of the product of the block_ind_map rows inside its sectors"""
    n = len(t.legs)
    if leg_idcs is None:
        leg_idcs = [i for i, l in enumerate(t.legs) if isinstance(l, PipeSpec)]
    leg_idcs = sorted(int(i) % n for i in leg_idcs)
    for i in leg_idcs:
        if not isinstance(t.legs[i], PipeSpec):
            raise ValueError('Not a LegPipe.')
    legs = []
    for i, l in enumerate(t.legs):
        legs += list(l.legs) if i in leg_idcs else [l]
    num_codomain = sum(len(t.legs[i].legs) if i in leg_idcs else 1 for i in range(t.num_codomain))
    rows = []
    for row in t.block_inds.tolist():
        options = []
        for i, l in enumerate(t.legs):
            if i in leg_idcs:
                options.append([tuple(r[2:-1]) for r in l.block_ind_map.tolist() if r[-1] == row[i]])
            else:
                options.append([(row[i],)])
        for pick in itertools.product(*options):
            rows.append([j for part in pick for j in part])
    dtype = complex if any(np.iscomplexobj(b) for b in t.blocks) else float
    dense = dense_split(to_dense(t, dtype), t.legs, leg_idcs)
    return _cut(t.moduli, legs, dense, rows, num_codomain)


def permute(t, perm):
    legs = [t.legs[p] for p in perm]
    rows = t.block_inds[:, perm] if len(t.blocks) else np.zeros((0, len(perm)), np.int64)
    order = np.lexsort(rows.T) if len(t.blocks) else []
    return wl.TensorSpec(t.moduli, legs, rows[order] if len(t.blocks) else rows, [t.blocks[i].transpose(perm) for i in order],
                         t.num_codomain)
