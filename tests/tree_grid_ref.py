"""numpy restatement of ``FusionTreeBackend::from_grid`` (src/backends/fusion_tree_backend.cpp:3375-3518) and
``::from_tree_pairs`` (:3186-3263), loop for loop: the result allocated as zeros for every common coupled sector, per grid
entry the codomain forests and the domain forests of its blocks, the two six-axis reshapes, the accumulation into the slice
of the stacked multiplicities, and ``discard_zero_blocks`` at the end.  Trees are matched by their POSITION inside the forest,
as the reference does (:3424-3433); ``cyten_amd.fusion_tree.from_grid`` matches them by key.

A forest is a maximal run of consecutive trees of one coupled sector with equal ``uncoupled`` keys (``iter_forest_blocks``
yields contiguous slices); the spaces handed to this file keep the trees of a forest together."""
import numpy as np


def abs1(x):
    x = np.asarray(x)
    return np.abs(x.real) + np.abs(x.imag)


def forests(space, i):
    """[(uncoupled, start, stop, multiplicities)] of the coupled sector i, in tree order"""
    out = []
    for tb in space.tree_blocks[i]:
        if out and out[-1][0] == tuple(tb.uncoupled):
            assert out[-1][3] == tuple(tb.multiplicities)          # the multiplicities belong to the uncoupled sectors
            out[-1][2] = tb.stop
        else:
            out.append([tuple(tb.uncoupled), tb.start, tb.stop, tuple(tb.multiplicities)])
    return [tuple(f) for f in out]


def _forest_slice(space, i, uncoupled):
    for u, start, stop, mults in forests(space, i):
        if u == uncoupled:
            return start, stop, mults
    raise KeyError(uncoupled)


def from_grid_ref(grid, new_codomain, new_domain, left_slices, right_slices, factors=None, eps=0.0, discard=True, absolute=False):
    """-> {(i, j): block}.  ``absolute``: the same loop on |.|_1 of the data and of the factors (the S of the bounds)."""
    common = [(i, j) for i, s in enumerate(new_codomain.sectors.tolist()) for j, t in enumerate(new_domain.sectors.tolist()) if s == t]
    cplx = any(np.iscomplexobj(b) for row in grid for op in row if op is not None for b in op.blocks)
    if factors is not None:
        cplx = cplx or any(complex(factors[i][j]).imag != 0 for i, row in enumerate(grid) for j, op in enumerate(row) if op is not None)
    dtype = np.float64 if absolute or not cplx else np.complex128
    data = {(i, j): np.zeros((new_codomain.block_size(i), new_domain.block_size(j)), dtype=dtype) for i, j in common}    # (:3391)
    of_sector = {tuple(new_domain.sectors[j].tolist()): (i, j) for i, j in common}
    for i, row in enumerate(grid):
        for j, op in enumerate(row):
            if op is None:
                continue                                                                                                # (:3397)
            f = 1.0 if factors is None else factors[i][j]
            for n, (ic, jd) in enumerate(op.block_inds.tolist()):
                coupled = tuple(op.domain.sectors[jd].tolist())
                if coupled not in of_sector:
                    continue                                                                                            # (:3412)
                i_new, j_new = of_sector[coupled]
                op_blk = abs1(op.blocks[n]) * abs1(f) if absolute else op.blocks[n] * f
                for unc, c0, c1, op_m in forests(op.codomain, ic):                                                      # (:3409)
                    op_codom0, op_codom_rest = op_m[0], int(np.prod(op_m[1:], dtype=np.int64))
                    op_num_cod = (c1 - c0) // max(1, op_codom0 * op_codom_rest)                                         # (:3424)
                    n0, n1, new_m = _forest_slice(new_codomain, i_new, unc)                                             # (:3431)
                    num_cod = (n1 - n0) // max(1, new_m[0] * op_codom_rest)
                    Ls = slice(left_slices[unc[0]][i], left_slices[unc[0]][i + 1])                                      # (:3438)
                    for und, d0, d1, op_dm in forests(op.domain, jd):                                                   # (:3442)
                        op_dom_rest, op_dom_last = int(np.prod(op_dm[:-1], dtype=np.int64)), op_dm[-1]
                        op_num_dom = (d1 - d0) // max(1, op_dom_rest * op_dom_last)
                        m0, m1, new_dm = _forest_slice(new_domain, j_new, und)                                          # (:3466)
                        num_dom = (m1 - m0) // max(1, op_dom_rest * new_dm[-1])
                        Rs = slice(right_slices[und[-1]][j], right_slices[und[-1]][j + 1])                              # (:3476)
                        piece = op_blk[c0:c1, d0:d1].reshape(op_num_cod, op_codom0, op_codom_rest, op_num_dom, op_dom_rest, op_dom_last)
                        block = data[(i_new, j_new)][n0:n1, m0:m1].copy()                                               # (:3485)
                        final = block.shape
                        block = block.reshape(num_cod, new_m[0], op_codom_rest, num_dom, op_dom_rest, new_dm[-1])
                        block[:, Ls, :, :, :, Rs] = block[:, Ls, :, :, :, Rs] + piece                                   # (:3499-3506)
                        data[(i_new, j_new)][n0:n1, m0:m1] = block.reshape(final)
    if discard:
        data = {k: b for k, b in data.items() if not np.abs(b).max(initial=0.0) <= eps}                                # (:3516)
    return data


def from_tree_pairs_ref(trees, codomain, domain, dtype):
    """-> {(i, j): block}; raises KeyError for an uncovered tree pair (:3247-3249)"""
    J, K = codomain.num_legs, domain.num_legs
    out, done = {}, set()
    for i, s in enumerate(codomain.sectors.tolist()):
        for j, t in enumerate(domain.sectors.tolist()):
            if s != t:
                continue
            block = np.zeros((codomain.block_size(i), domain.block_size(j)), dtype=dtype)
            is_zero = True
            for xb in codomain.tree_blocks[i]:
                for yb in domain.tree_blocks[j]:
                    tb = trees.get((xb.tree, yb.tree))
                    if tb is None:
                        continue
                    assert tuple(tb.shape) == tuple(xb.multiplicities) + tuple(yb.multiplicities)[::-1]
                    tb = np.transpose(tb, list(range(J)) + list(range(J + K - 1, J - 1, -1)))                           # (:3231)
                    block[xb.start:xb.stop, yb.start:yb.stop] = tb.reshape(xb.stop - xb.start, yb.stop - yb.start)
                    is_zero = False
                    done.add((xb.tree, yb.tree))
            if not is_zero:
                out[(i, j)] = block
    for k in trees:
        if k not in done:
            raise KeyError(k)
    return out
