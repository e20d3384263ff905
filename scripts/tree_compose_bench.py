"""Fusion-tree partial_compose (ONE launch) against the per-term route, on the device.

    python scripts/tree_compose_bench.py [chi ...] [--reps N] [--out FILE] [--grouped-only]

SU(2)-shaped structures built from the fusion rules (the spaces of scripts/tree_trace_bench.py): a bond leg v (spins 0 .. 2,
multiplicities that add up to chi) and a physical leg p of spin 1/2 with the multiplicity 2:

  site      a: (v, p) -> v, b: p -> p contracted with leg 1 of a's codomain -- a site operator applied to an MPS tensor.  The
            one-leg b has no vertex: every amplitude of ``insert_at`` is 1 (src/symmetries/trees.cpp:1248-1255).  K = N = 2.
  gate      a: (v, p, p) -> v, b: (p, p) -> (p, p) contracted with legs 1, 2 of a's codomain -- a two-site gate applied to a
            two-site tensor.  The amplitudes are the F symbols of scripts/make_su2_golden.py (Racah formula).  K = N = 4.

Two routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise, profiler off:

  grouped   fusion_tree.partial_compose -> ONE cyb_compose_weighted_f64 launch (+ the reductions of discard_zero_blocks)
  terms     the route available before: the reference's five-deep loop (fusion_tree_backend.cpp:2756-2863) with its
            block-backend calls per innermost iteration -- get_item, reshape, tdot, permute_axes, reshape, mul, get_item, + and
            set_item, into zero-filled blocks

Printed per case (one JSON line): median / min / max milliseconds of both routes, their C-ABI calls by name, the numbers of
strips and terms, the host share of the grouped call (the call with ``tree_compose_many`` replaced by a no-op), and the
algorithmic bytes of the launch computed from the record shapes (every strip written once, the strip of a and the tile of b
of every term read once).  The yardstick is ``cyb_outer_weighted_f64`` (``tree_outer_many``) in the same run on an equal byte
count: one 1 x 1 (x) H x W tile per strip, the H x W source sized so that reading it and writing the tile move the bytes of
that strip's record.  Kernel times come from a profiler run of its own:
``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/tree_compose_bench.py 4096 --reps 5 --grouped-only``."""
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


def insert_tables(v, p, n_legs):
    """TreeInsert of b's `n_legs` (1 or 2) physical legs into leg 1 of the outer trees (j_v, e; c) of a's codomain"""
    outer_trees, table = {}, {}
    es = [1] if n_legs == 1 else [0, 2]
    if n_legs == 2:
        from make_su2_golden import racah_F
    for jv in sorted(v):
        for e in es:
            for c in fuse(jv, e):
                key = ('o', jv, e, c)
                outer_trees.setdefault((c,), []).append((key, (e,), v[jv], 1))
                if n_legs == 1:
                    trees = [(('c', (jv, 1), (c,)), 1.0)]
                    bkeys = [('c', (1,), ()), ('d', (1,), ())]
                else:
                    trees = [(('c', (jv, 1, 1), (f, c)), racah_F(jv, 1, 1, c, f, e)) for f in fuse(jv, 1) if c in fuse(f, 1)]
                    bkeys = [('c', (1, 1), (e,)), ('d', (1, 1), (e,))]
                for bk in bkeys:
                    table[(key, bk)] = trees
    return ft.TreeInsert('codomain', 1, outer_trees, table)


def term_route(bb, a, a_cod, a_dom, b, b_cod, b_dom, n_cod, n_dom, insert):
    """the reference's loop in the codomain (:2828-2857), one innermost iteration at a time through the block backend"""
    where_c = {tuple(s): k for k, s in enumerate(n_cod.sectors.tolist())}
    where_d = {tuple(s): k for k, s in enumerate(n_dom.sectors.tolist())}
    where_b = {tuple(s): k for k, s in enumerate(b_dom.sectors.tolist())}
    rows, blocks = [], []
    for n, (i, _) in enumerate(a.block_inds.tolist()):
        coupled = tuple(a_cod.sectors[i].tolist())
        if coupled not in where_c or coupled not in where_d:
            continue
        i_new, j_new = where_c[coupled], where_d[coupled]
        new = bb.zeros_many([(n_cod.block_size(i_new), n_dom.block_size(j_new))])[0]
        for tree, b_sector, dm0, dm2 in insert.outer_trees.get(coupled, ()):
            jb = where_b[tuple(b_sector)]
            nb = b.block_ind_from_domain_sector(jb)
            for xb in b_cod.tree_blocks[int(b.block_inds[nb, 0])]:
                for yb in b_dom.tree_blocks[jb]:
                    b_tree_block = bb.get_item(b.blocks[nb], (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))
                    N, K = b_tree_block.shape
                    for old_tree, amp_old in insert.table[(tree, yb.tree)]:
                        _, old = a_cod.tree_block_slice(old_tree)
                        a_forest = bb.get_item(a.blocks[n], (slice(old.start, old.stop), slice(None)))
                        a_forest = bb.reshape(a_forest, [dm0, K, dm2, -1])
                        for new_tree, amp_new in insert.table[(tree, xb.tree)]:
                            _, nw = n_cod.tree_block_slice(new_tree)
                            contribution = bb.tdot(a_forest, b_tree_block, [1], [1])
                            contribution = bb.permute_axes(contribution, [0, 3, 1, 2])
                            contribution = bb.reshape(contribution, [dm0 * N * dm2, -1])
                            sl = (slice(nw.start, nw.stop), slice(None))
                            bb.set_item(new, sl, bb.get_item(new, sl) + bb.mul(float(np.conj(amp_old) * amp_new), contribution))
        rows.append((i_new, j_new))
        blocks.append(new)
    return ft.FusionTreeData(np.array(rows, dtype=np.int64).reshape(len(rows), 2), blocks)


def record_shapes(bb, fn):
    """(outputs of the tree_compose_many call `fn` makes, strips, terms, algorithmic bytes per strip: 8 per element written
    and per source element of a term read)"""
    real, seen = bb.tree_compose_many, []
    bb.tree_compose_many = lambda outputs: (seen.append(list(outputs)), real(seen[-1]))[1]
    try:
        fn()
    finally:
        del bb.tree_compose_many
    (outputs,) = seen
    nbytes = [8 * (math.prod(dst.shape) + sum(math.prod(x.shape) + math.prod(y.shape) for x, y, _ in terms)) for dst, _, _, _, terms in outputs]
    return outputs, len(outputs), sum(len(o[4]) for o in outputs), nbytes


def host_only(bb, fn):
    """`fn` with the launch taken out: what the host spends on tables, views and records"""
    bb.tree_compose_many = lambda outputs: None
    try:
        return timed(bb, fn)
    finally:
        del bb.tree_compose_many


def yardstick(bb, outputs, nbytes):
    """one cyb_outer_weighted_f64 call that moves the bytes of every strip's record: dst = 1 * [[1]] (x) src, src and dst of
    (elements of the strip, columns of the strip) so that 8 * (src + dst + 1) is the byte count of the record"""
    one = bb.as_block(np.ones((1, 1)))
    shapes = []
    for (dst, *_), nb in zip(outputs, nbytes):
        w = dst.shape[1]
        shapes.append((max(1, round(nb / 16 / w)), w))
    srcs = [bb.random_normal(sh, seed=99 + k) for k, sh in enumerate(shapes)]
    dsts = bb.zeros_many(shapes)
    recs = [(d, [(one, s, 1.0)]) for d, s in zip(dsts, srcs)]
    return (lambda: bb.tree_outer_many(recs)), sum(8 * (2 * h * w + 1) for h, w in shapes)


def cases(chi):
    v = {k: max(1, round(chi * w)) for k, w in WEIGHTS.items()}
    p = {1: 2}
    return [('site', v, p, 1), ('gate', v, p, 2)]


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
    for chi in args.chi:
        for name, v, p, n_legs in cases(chi):
            a_cod, a_dom = space([v] + [p] * n_legs, 'c'), space([v], 'd')
            b_cod, b_dom = space([p] * n_legs, 'c'), space([p] * n_legs, 'd')
            insert = insert_tables(v, p, n_legs)

            def rand(cod, dom, seed):
                rows = ft.common_sectors(cod, dom)
                return ft.FusionTreeData(rows, [bb.random_normal((cod.block_size(i), dom.block_size(j)), seed=seed + n)
                                                for n, (i, j) in enumerate(rows)])

            a, b = rand(a_cod, a_dom, 7), rand(b_cod, b_dom, 1007)
            fargs = (a, a_cod, a_dom, b, b_cod, b_dom, a_cod, a_dom, insert)
            grouped = lambda: ft.partial_compose(bb, *fargs)                           # noqa: E731
            terms_route = lambda: term_route(bb, *fargs)                               # noqa: E731
            outputs, strips, terms, nbytes = record_shapes(bb, grouped)
            yard, yard_bytes = yardstick(bb, outputs, nbytes)
            res = dict(case=name, chi=chi, a_blocks=len(a.blocks), b_blocks=len(b.blocks), strips=strips, terms=terms,
                       algorithmic_bytes=sum(nbytes), yardstick_bytes=yard_bytes)
            if not args.grouped_only:
                g, l = grouped(), terms_route()     # the two routes compute the same thing
                lb = {tuple(r): bb.to_numpy(blk) for r, blk in zip(l.block_inds.tolist(), l.blocks)}
                for r, blk in zip(g.block_inds.tolist(), g.blocks):
                    x, y = bb.to_numpy(blk), lb[tuple(r)]
                    assert np.abs(x - y).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(y).max(initial=0.0)), (name, r)
                res.update(grouped_calls=count_calls(bb, grouped), terms_calls=count_calls(bb, terms_route))
                res['terms_launches'] = sum(res['terms_calls'].values())
            for _ in range(args.warmup):
                grouped(), yard()
                if not args.grouped_only:
                    terms_route()
            tg, tl, ty, th = [], [], [], []
            for _ in range(args.reps):
                tg.append(timed(bb, grouped))
                ty.append(timed(bb, yard))
                th.append(host_only(bb, lambda: ft.partial_compose(bb, *fargs, discard=False)))
                if not args.grouped_only:
                    tl.append(timed(bb, terms_route))
            med = statistics.median
            res.update(grouped_ms=dict(median=med(tg), min=min(tg), max=max(tg)), grouped_host_only_ms=dict(median=med(th), min=min(th), max=max(th)),
                       yardstick_ms=dict(median=med(ty), min=min(ty), max=max(ty)),
                       grouped_TBps_over_call=sum(nbytes) / (med(tg) * 1e-3) / 1e12, yardstick_TBps_over_call=yard_bytes / (med(ty) * 1e-3) / 1e12,
                       hbm_stream_TBps=HBM_STREAM_TBS)
            if tl:
                res.update(terms_ms=dict(median=med(tl), min=min(tl), max=max(tl)), speedup_median=med(tl) / med(tg),
                           grouped_faster_beyond_spread=max(tg) < min(tl))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
