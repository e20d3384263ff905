"""to_dense_block / from_dense_block on fusion-tree tensors (ONE launch each) against the per-forest route, on the device.

    python scripts/tree_dense_bench.py [chi ...] [--reps N] [--out FILE] [--launch-only]

An SU(2) tensor (v, p) <- (v, p): p a site of spin 1/2, v a bond leg with the sectors of ``make_su2_golden.leg`` over the spins
0 .. 2 whose dimension sum m_j (2 j + 1) is about chi; the tree tensors are Clebsch-Gordan coefficients from sympy.  The
default chi = 1768 makes the dense tensor (2 chi)^2 * 8 = 1.0e8 bytes.

Two routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise, profiler off; both directions:

  call     fusion_tree.to_dense_block -> ONE cyb_tree_to_dense_f64 launch; fusion_tree.from_dense_block -> ONE
           cyb_tree_from_dense_f64 launch + the reductions of the tolerance check and of discard_zero_blocks
  forest   the reference's sequence of block-backend calls through the same HipBlockBackend: per pair of trees of every
           forest pair zeros, conj, tdot, get_item, reshape, outer, +, then permute_axes, reshape and an accumulating set_item
           into a zero-filled dense tensor (fusion_tree_backend.cpp:1532-1604, :1881-1950); backwards get_item, reshape,
           permute_axes, two tdot, trace_partial, a division, reshape and set_item into zero-filled blocks, a norm per block
           and the norm of the dense tensor (:1606-1677, :1761-1838)

Printed per chi (one JSON line): median / min / max milliseconds of both routes in both directions, their C-ABI calls by name,
the numbers of regions / tiles and terms, and the algorithmic bytes of the two launches (forward: every dense element written
once, every block tile of a term read once; backward: every dense element of a region read once, every tile written once).
``--launch-only`` runs just the two backend launches and the yardstick -- ``cyb_outer_weighted_f64`` writing a tile of the same
(2 chi)^2 elements (a chi x chi tile (x) a 2 x 2 tile) -- for a profiler run of its own, which is where kernel times come from:
``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/tree_dense_bench.py --launch-only --reps 7``."""
import argparse
import functools
import itertools
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cyten_amd import fusion_tree as ft  # noqa: E402
from make_su2_golden import leg  # noqa: E402
from tree_trace_bench import HBM_STREAM_TBS, count_calls, space, timed  # noqa: E402


@functools.lru_cache(maxsize=None)
def cg_tensor(a2, b2, c2):
    """X[ma, mb, mc] = <ja ma jb mb | jc mc>, index i of a sector counts m = -j + i"""
    from sympy import Rational
    from sympy.physics.quantum.cg import CG
    X = np.zeros((a2 + 1, b2 + 1, c2 + 1))
    for ia, ib, ic in itertools.product(range(a2 + 1), range(b2 + 1), range(c2 + 1)):
        ma, mb, mc = -a2 + 2 * ia, -b2 + 2 * ib, -c2 + 2 * ic
        if ma + mb == mc:
            X[ia, ib, ic] = float(CG(Rational(a2, 2), Rational(ma, 2), Rational(b2, 2), Rational(mb, 2), Rational(c2, 2), Rational(mc, 2)).doit())
    return X


def side(legs, tag):
    """(TreeSpace, TreeDense) of a two-leg side; a tree is (tag, (ja, jb), (J,))"""
    sp = space(legs, tag)
    dims = {j: j + 1 for lg in legs for j in lg}
    tensors = {tb.tree: cg_tensor(tb.tree[1][0], tb.tree[1][1], tb.tree[2][0]) for tbs in sp.tree_blocks for tb in tbs}
    return sp, ft.TreeDense(tuple([(j, lg[j]) for j in sorted(lg)] for lg in legs), dims, tensors)


def _positions(dense):
    out = []
    for lg in dense.legs:
        pos, off = {}, 0
        for key, m in lg:
            pos[key] = (off, dense.sector_dims[key], m)
            off += dense.sector_dims[key] * m
        out.append(pos)
    return out


def _forests(sp):
    """per coupled sector: [(uncoupled, [TreeBlock, ...])], forests in the order of their first tree"""
    res = []
    for tbs in sp.tree_blocks:
        fs = {}
        for tb in tbs:
            fs.setdefault(tb.uncoupled, []).append(tb)
        res.append(list(fs.items()))
    return res


def forest_to_dense(bb, data, cod, dom, cd, dd, dev_tensors):
    """the reference's loop, one pair of trees at a time through the block backend"""
    J, K = cod.num_legs, dom.num_legs
    N = J + K
    cw, dw = _positions(cd), _positions(dd)
    shape = [sum(d * m for _, d, m in pos.values()) for pos in cw + dw]
    res = bb.zeros(shape)
    cf, df = _forests(cod), _forests(dom)
    for n, (i, j) in enumerate(data.block_inds.tolist()):
        for b_unc, betas in df[j]:
            for a_unc, alphas in cf[i]:
                at = [cw[l][k] for l, k in enumerate(a_unc)] + [dw[l][k] for l, k in enumerate(b_unc)]
                dims, mults = [d for _, d, _ in at], [m for _, _, m in at]
                entries = bb.zeros(dims + mults)
                for xa in alphas:
                    splitting = bb.conj(dev_tensors[xa.tree])
                    for yb in betas:
                        sym = bb.tdot(splitting, dev_tensors[yb.tree], [-1], [-1])
                        deg = bb.reshape(bb.get_item(data.blocks[n], (slice(xa.start, xa.stop), slice(yb.start, yb.stop))), mults)
                        entries = entries + bb.outer(sym, deg)
                entries = bb.permute_axes(entries, [p for l in range(N) for p in (l, l + N)])
                entries = bb.reshape(entries, [d * m for d, m in zip(dims, mults)])
                sl = tuple(slice(s, s + d * m) for s, d, m in at)
                bb.set_item(res, sl, bb.get_item(res, sl) + entries)
    return bb.permute_axes(res, list(range(J)) + list(range(N - 1, J - 1, -1)))


def forest_from_dense(bb, a, cod, dom, cd, dd, dev_tensors, tol=1e-8):
    J, K = cod.num_legs, dom.num_legs
    N = J + K
    cw, dw = _positions(cd), _positions(dd)
    a = bb.permute_axes(a, list(range(J)) + list(range(N - 1, J - 1, -1)))
    cf, df = _forests(cod), _forests(dom)
    rows, blocks, proj = [], [], 0.0
    for i, j in ft.common_sectors(cod, dom):
        block = bb.zeros((cod.block_size(i), dom.block_size(j)))
        dc = float(cod.qdims[i])
        for b_unc, betas in df[j]:
            for a_unc, alphas in cf[i]:
                at = [cw[l][k] for l, k in enumerate(a_unc)] + [dw[l][k] for l, k in enumerate(b_unc)]
                entries = bb.get_item(a, tuple(slice(s, s + d * m) for s, d, m in at))
                entries = bb.reshape(entries, [x for _, d, m in at for x in (d, m)])
                entries = bb.permute_axes(entries, list(range(0, 2 * N, 2)) + list(range(1, 2 * N, 2)))
                for xa in alphas:
                    Yp = bb.tdot(entries, dev_tensors[xa.tree], list(range(J)), list(range(J)))
                    for yb in betas:
                        YX = bb.tdot(Yp, bb.conj(dev_tensors[yb.tree]), list(range(K)), list(range(K)))
                        tree_block = bb.trace_partial(YX, [-2], [-1], list(range(N))) / dc
                        bb.set_item(block, (slice(xa.start, xa.stop), slice(yb.start, yb.stop)),
                                    bb.reshape(tree_block, (xa.stop - xa.start, yb.stop - yb.start)))
        nrm = bb.norm(block)
        if nrm <= 1e-14:
            continue
        rows.append((i, j))
        blocks.append(block)
        proj += dc * nrm * nrm
    if tol != 0.0:
        a2 = bb.norm(a) ** 2
        if a2 - proj > (tol * tol + 32 * 2.0 ** -53) * a2:
            raise ValueError('not symmetric up to tolerance')
    return ft.FusionTreeData(np.array(rows, dtype=np.int64).reshape(len(rows), 2), blocks)


def capture(bb, name, fn):
    """the arguments of the one call of ``bb.<name>`` that `fn` makes"""
    real, seen = getattr(bb, name), []
    setattr(bb, name, lambda *args: (seen.append(args), real(*args))[1])
    try:
        fn()
    finally:
        delattr(bb, name)
    (args,) = seen
    return args


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[1768])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--launch-only', action='store_true', help='run the two backend launches and the yardstick alone (for a profiler run)')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    for chi in args.chi:
        tj, m = leg([0, 1, 2, 3, 4], chi)
        v, p = {int(j): int(x) for j, x in zip(tj, m)}, {1: 1}
        (cod, cd), (dom, dd) = side([v, p], 'c'), side([v, p], 'd')
        rows = ft.common_sectors(cod, dom)
        data = ft.FusionTreeData(rows, [bb.random_normal((cod.block_size(i), dom.block_size(j)), seed=7 + n) for n, (i, j) in enumerate(rows)])
        dev_tensors = {k: bb.as_block(X) for td in (cd, dd) for k, X in td.tensors.items()}
        sp = (cod, dom, cd, dd)
        dense = ft.to_dense_block(bb, data, *sp)
        D = dense.shape[0] * dense.shape[1]            # the dense tensor as a D x D matrix, D = 2 chi
        fwd_call = lambda: ft.to_dense_block(bb, data, *sp)                            # noqa: E731
        bwd_call = lambda: ft.from_dense_block(bb, dense, *sp)                         # noqa: E731
        fwd_forest = lambda: forest_to_dense(bb, data, *sp, dev_tensors)               # noqa: E731
        bwd_forest = lambda: forest_from_dense(bb, dense, *sp, dev_tensors)            # noqa: E731
        view, regions = capture(bb, 'tree_to_dense_many', fwd_call)
        (outputs,) = capture(bb, 'tree_from_dense_many', bwd_call)
        fwd_bytes = 8 * sum(math.prod(d * x for d, x in zip(dims, mults)) + len(terms) * math.prod(mults) for _, dims, mults, _, terms in regions)
        bwd_bytes = 8 * sum(math.prod(dst.shape) * (1 + len(terms) * math.prod(dims)) for dst, _, dims, _, _, terms in outputs)
        fwd_launch = lambda: bb.tree_to_dense_many(view, regions)                      # noqa: E731
        bwd_launch = lambda: bb.tree_from_dense_many(outputs)                          # noqa: E731
        ya, yb, ydst = bb.random_normal((D // 2, D // 2), seed=3), bb.random_normal((2, 2), seed=4), bb.empty_many([(D, D)])[0]
        yard = lambda: bb.tree_outer_many([(ydst, [(ya, yb, 1.0)])])                   # noqa: E731
        res = dict(chi=chi, bond_sectors=v, dense_shape=list(dense.shape), dense_bytes=8 * math.prod(dense.shape), blocks=len(rows),
                   regions=len(regions), forward_terms=sum(len(r[4]) for r in regions), tiles=len(outputs), forward_bytes=fwd_bytes,
                   backward_bytes=bwd_bytes, yardstick_bytes=8 * (D * D + (D // 2) ** 2 + 4), hbm_stream_TBps=HBM_STREAM_TBS)
        med = statistics.median
        stats = lambda ts: dict(median=med(ts), min=min(ts), max=max(ts))              # noqa: E731
        if args.launch_only:
            for _ in range(args.warmup + args.reps):
                fwd_launch(), bwd_launch(), yard()
            bb.synchronize()
        else:
            # the two routes compute the same thing
            ref_dense = bb.to_numpy(fwd_forest())
            got_dense = bb.to_numpy(dense)
            assert np.abs(got_dense - ref_dense).max() <= 1e-12 * np.abs(ref_dense).max()
            g, l = bwd_call(), bwd_forest()
            assert g.block_inds.tolist() == l.block_inds.tolist() == data.block_inds.tolist()
            for x, y, z in zip(g.blocks, l.blocks, data.blocks):
                y = bb.to_numpy(y)
                assert np.abs(bb.to_numpy(x) - y).max() <= 1e-12 * np.abs(y).max() and np.abs(bb.to_numpy(z) - y).max() <= 1e-12 * np.abs(y).max()
            res.update(forward_call_calls=count_calls(bb, fwd_call), forward_forest_calls=sum(count_calls(bb, fwd_forest).values()),
                       backward_call_calls=count_calls(bb, bwd_call), backward_forest_calls=sum(count_calls(bb, bwd_forest).values()))
            routes = dict(forward_call=fwd_call, forward_forest=fwd_forest, backward_call=bwd_call, backward_forest=bwd_forest,
                          forward_launch=fwd_launch, backward_launch=bwd_launch, yardstick_launch=yard)
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            times = {k: [] for k in routes}
            for _ in range(args.reps):
                for k, fn in routes.items():
                    times[k].append(timed(bb, fn))
            res.update({k + '_ms': stats(ts) for k, ts in times.items()})
            res.update(reps=args.reps, forward_speedup_median=med(times['forward_forest']) / med(times['forward_call']),
                       backward_speedup_median=med(times['backward_forest']) / med(times['backward_call']),
                       forward_faster_beyond_spread=max(times['forward_call']) < min(times['forward_forest']),
                       backward_faster_beyond_spread=max(times['backward_call']) < min(times['backward_forest']))
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
