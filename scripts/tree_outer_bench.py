"""Fusion-tree outer (ONE launch) against the per-pair route, on the device.

    python scripts/tree_outer_bench.py [chi ...] [--reps N] [--out FILE] [--grouped-only]

SU(2)-shaped structures built from the fusion rules alone (the spaces of scripts/tree_trace_bench.py); the right operand has one
leg per side, so every amplitude of ``FusionTree::outer`` is 1 (src/symmetries/trees.cpp:1248-1258) and the tables follow from
the fusion rules:

  operator  a: (s, s) -> (s, s), b: s -> s on a site leg s with the spins 0, 1/2, 1 and multiplicity 1 -- building a
            three-site operator from site operators: many tiny tiles, independent of chi
  chi       a: (v, p) -> v with a bond leg v (spins 0 .. 2, multiplicities that add up to chi) and p of spin 1/2, b: p -> p --
            a chi-sized tensor times a site operator: the result is a store stream of tiles as large as a's

Two routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise, profiler off:

  grouped   fusion_tree.outer -> ONE cyb_outer_weighted_f64 launch (+ the reductions of discard_zero_blocks)
  pairs     the route available before: the reference's double loop (fusion_tree_backend.cpp:2626-2664) with its
            block-backend calls per pair of tree pairs -- outer, permute_axes, combine_legs, and get_item, mul, + and
            set_item per new tree pair, into zero-filled blocks

Printed per case (one JSON line): median / min / max milliseconds of both routes, their C-ABI calls by name, the numbers of
tiles and terms, the host share of the grouped call (the call with ``tree_outer_many`` replaced by a no-op), and the algorithmic
bytes of the launch computed from the record shapes (every tile written once, every source tile of a term read once).  The
yardstick ``tensor_outer_many`` (``cyb_outer_grouped_*``, the project's store stream) runs on the (A, B) pairs of the terms.
Kernel times come from a profiler run of its own:
``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/tree_outer_bench.py 4096 --reps 5 --grouped-only``."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cyten_amd import fusion_tree as ft  # noqa: E402
from tree_trace_bench import HBM_STREAM_TBS, WEIGHTS, count_calls, fuse, space, timed  # noqa: E402


def outer_table(left, right, tag):
    """TreeOuter of a side whose right factor has one leg: the new tree appends the leg and the new coupling, amplitude 1"""
    table = {}
    for (cur,), ta in zip(left.sectors.tolist(), left.tree_blocks):
        for xa in ta:
            _, unc, chain = xa.tree
            for (s,), tb in zip(right.sectors.tolist(), right.tree_blocks):
                table[(xa.tree, tb[0].tree)] = [((tag, unc + (s,), chain + (c,)), 1.0) for c in fuse(cur, s)]
    return ft.TreeOuter(table)


def pair_route(bb, a, a_cod, a_dom, b, b_cod, b_dom, n_cod, n_dom, ct, dt):
    """the reference's loop, one pair of tree pairs at a time through the block backend"""
    rows = ft.common_sectors(n_cod, n_dom)
    new = dict(zip(rows, bb.zeros_many([(n_cod.block_size(i), n_dom.block_size(j)) for i, j in rows])))
    block_of_dom = {j: (i, j) for i, j in rows}

    def tree_blocks(data, cod, dom):
        for n, (i, j) in enumerate(data.block_inds.tolist()):
            for xb in cod.tree_blocks[i]:
                for yb in dom.tree_blocks[j]:
                    yield xb, yb, bb.get_item(data.blocks[n], (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))

    for xa, ya, A in tree_blocks(a, a_cod, a_dom):
        for xb, yb, B in tree_blocks(b, b_cod, b_dom):
            blk = bb.outer(A, B)
            blk = bb.permute_axes(blk, [0, 2, 1, 3])
            blk = bb.combine_legs(blk, [[0, 1], [2, 3]])
            for new_dom_tree, dom_amp in dt.table[(ya.tree, yb.tree)]:
                j_new, ny = n_dom.tree_block_slice(new_dom_tree)
                key = block_of_dom.get(j_new)
                if key is None:
                    continue
                for new_cod_tree, cod_amp in ct.table[(xa.tree, xb.tree)]:
                    i_new, nx = n_cod.tree_block_slice(new_cod_tree)
                    if n_cod.sectors[i_new].tolist() != n_dom.sectors[j_new].tolist():
                        continue
                    sl = (slice(nx.start, nx.stop), slice(ny.start, ny.stop))
                    bb.set_item(new[key], sl, bb.get_item(new[key], sl) + bb.mul(float(np.conj(cod_amp) * dom_amp), blk))
    return ft.FusionTreeData(np.array(rows, dtype=np.int64).reshape(len(rows), 2), [new[r] for r in rows])


def record_shapes(bb, fn):
    """(outputs of the tree_outer_many call `fn` makes, tiles, terms, algorithmic bytes: 8 per element written and per source
    element of a term read)"""
    real, seen = bb.tree_outer_many, []
    bb.tree_outer_many = lambda outputs: (seen.append(list(outputs)), real(seen[-1]))[1]
    try:
        fn()
    finally:
        del bb.tree_outer_many
    (outputs,) = seen
    nbytes = sum(8 * (math.prod(dst.shape) + sum(math.prod(x.shape) + math.prod(y.shape) for x, y, _ in terms)) for dst, terms in outputs)
    return outputs, len(outputs), sum(len(t) for _, t in outputs), nbytes


def host_only(bb, fn):
    """`fn` with the launch taken out: what the host spends on tables, views and records"""
    bb.tree_outer_many = lambda outputs: None
    try:
        return timed(bb, fn)
    finally:
        del bb.tree_outer_many


def cases(chi):
    s = {0: 1, 1: 1, 2: 1}
    v = {k: max(1, round(chi * w)) for k, w in WEIGHTS.items()}
    p = {1: 1}
    return [('operator', [s, s], [s, s], [s], [s]), ('chi', [v, p], [v], [p], [p])]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[512, 4096])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--grouped-only', action='store_true', help='run the grouped route and the yardstick alone (for a profiler run)')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    done = set()
    for chi in args.chi:
        for name, ac, ad, bc, bd in cases(chi):
            if name == 'operator' and name in done:
                continue                        # (does not depend on chi)
            done.add(name)
            a_cod, a_dom, b_cod, b_dom = space(ac, 'c'), space(ad, 'd'), space(bc, 'c'), space(bd, 'd')
            n_cod, n_dom = space(ac + bc, 'c'), space(ad + bd, 'd')
            ct, dt = outer_table(a_cod, b_cod, 'c'), outer_table(a_dom, b_dom, 'd')

            def rand(cod, dom, seed):
                rows = ft.common_sectors(cod, dom)
                return ft.FusionTreeData(rows, [bb.random_normal((cod.block_size(i), dom.block_size(j)), seed=seed + n)
                                                for n, (i, j) in enumerate(rows)])

            a, b = rand(a_cod, a_dom, 7), rand(b_cod, b_dom, 1007)
            fargs = (a, a_cod, a_dom, b, b_cod, b_dom, n_cod, n_dom, ct, dt)
            grouped = lambda: ft.outer(bb, *fargs)                                     # noqa: E731
            pairs = lambda: pair_route(bb, *fargs)                                     # noqa: E731
            outputs, tiles, terms, nbytes = record_shapes(bb, grouped)
            term_pairs = [(x, y) for _, ts in outputs for x, y, _ in ts]
            yard = lambda: bb.tensor_outer_many(term_pairs, 1)                         # noqa: E731
            yard_bytes = sum(8 * (math.prod(x.shape) * math.prod(y.shape) + math.prod(x.shape) + math.prod(y.shape)) for x, y in term_pairs)
            res = dict(case=name, chi=None if name == 'operator' else chi, a_blocks=len(a.blocks), b_blocks=len(b.blocks), tiles=tiles, terms=terms,
                       algorithmic_bytes=nbytes, yardstick_bytes=yard_bytes)
            if not args.grouped_only:
                g, l = grouped(), pairs()           # the two routes compute the same thing
                lb = {tuple(r): bb.to_numpy(blk) for r, blk in zip(l.block_inds.tolist(), l.blocks)}
                for r, blk in zip(g.block_inds.tolist(), g.blocks):
                    x, y = bb.to_numpy(blk), lb[tuple(r)]
                    assert np.abs(x - y).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(y).max(initial=0.0)), (name, r)
                res.update(grouped_calls=count_calls(bb, grouped), pairs_calls=count_calls(bb, pairs))
                res['pairs_launches'] = sum(res['pairs_calls'].values())
            for _ in range(args.warmup):
                grouped(), yard()
                if not args.grouped_only:
                    pairs()
            tg, tl, ty, th = [], [], [], []
            for _ in range(args.reps):
                tg.append(timed(bb, grouped))
                ty.append(timed(bb, yard))
                th.append(host_only(bb, lambda: ft.outer(bb, *fargs, discard=False)))
                if not args.grouped_only:
                    tl.append(timed(bb, pairs))
            med = statistics.median
            res.update(grouped_ms=dict(median=med(tg), min=min(tg), max=max(tg)), grouped_host_only_ms=dict(median=med(th), min=min(th), max=max(th)),
                       yardstick_ms=dict(median=med(ty), min=min(ty), max=max(ty)),
                       grouped_TBps_over_call=nbytes / (med(tg) * 1e-3) / 1e12, hbm_stream_TBps=HBM_STREAM_TBS)
            if tl:
                res.update(pairs_ms=dict(median=med(tl), min=min(tl), max=max(tl)), speedup_median=med(tl) / med(tg),
                           grouped_faster_beyond_spread=max(tg) < min(tl))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
