"""Fusion-tree partial trace (ONE launch) against the per-tree-pair route, on the device.

    python scripts/tree_trace_bench.py [chi ...] [--reps N] [--out FILE] [--grouped-only]

An SU(2)-shaped structure built from the fusion rules alone: a bond leg v with the spins 0, 1/2, 1, 3/2, 2 and multiplicities
that add up to chi, a physical leg p of spin 1/2 with multiplicity 1.  The four legs [v, p, p-bar, v-bar] are arranged as step 1
of the partial trace (``transform_tensor``) leaves them, the traced pair adjacent on one side:

  physical  codomain (v, p, p-bar), domain (v):   pair (1, 2) -- tiny traced extents, two terms per tile, many elements
  bond      codomain (v, v-bar, p), domain (p):   pair (0, 1) -- few elements, sums as long as a bond multiplicity
  full      codomain (v, v-bar, p, p-bar), no domain: both pairs, the 1 x 1 result

The factors of the tables are made up (1 / sqrt(dim)): their values do not matter for the time.  Two routes run alternately
in one process after a warm-up, each timed by a host clock around work that ends in a device synchronise, profiler off:

  grouped   fusion_tree.partial_trace -> ONE cyb_trace_weighted_f64 launch (+ the reductions of discard_zero_blocks)
  pairs     the route available before: the reference's loop (fusion_tree_backend.cpp:3092-3159) with its seven
            block-backend calls per tree pair -- get_item, reshape, trace_partial, reshape, mul, get_item, + and set_item

Printed per case (one JSON line): median / min / max milliseconds of both routes, their C-ABI calls by name, the numbers of
tree pairs, tiles and terms, and the algorithmic bytes of the launch computed from the record shapes (every term's addends
read once, every tile written once) over the grouped call time.  Kernel times come from a profiler run of its own:
``rocprofv3 --kernel-trace --stats -- python scripts/tree_trace_bench.py 4096 --reps 5 --grouped-only``."""
import argparse
import collections
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cyten_amd import fusion_tree as ft  # noqa: E402

HBM_STREAM_TBS = 6.3      # MI355X_MICROARCH.md: achievable streaming rate
WEIGHTS = {0: 0.10, 1: 0.25, 2: 0.30, 3: 0.25, 4: 0.10}        # twice the spin -> share of chi


class CountingLib:
    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


def fuse(a, b):
    """twice the spins of a x b"""
    return range(abs(a - b), a + b + 1, 2)


def space(legs, tag):
    """TreeSpace of a product of legs ({twice the spin: multiplicity}): a tree is (tag, uncoupled spins, the couplings after
    the second, third, ... leg); coupled sector = the last coupling"""
    trees = collections.defaultdict(list)

    def rec(k, cur, unc, chain):
        if k == len(legs):
            trees[cur].append(((tag, unc, chain), tuple(legs[i][s] for i, s in enumerate(unc)), unc))
            return
        for s in sorted(legs[k]):
            for c in fuse(cur, s):
                rec(k + 1, c, unc + (s,), chain + (c,))

    if legs:
        for s in sorted(legs[0]):
            rec(1, s, (s,), ())
    else:
        trees[0].append(((tag, (), ()), (), ()))
    coupled = sorted(trees)
    return ft.TreeSpace.from_multiplicities(np.array(coupled)[:, None], [[t[1] for t in trees[c]] for c in coupled],
                                            [c + 1.0 for c in coupled], len(legs), [[t[0] for t in trees[c]] for c in coupled],
                                            [[t[2] for t in trees[c]] for c in coupled])


def trace_table(sp, positions):
    """TreeTrace of a side: a tree is on the diagonal if the two spins of every pair agree and the sectors left and right of
    the pair do (partial_trace_helper, fusion_tree_backend.cpp:2565-2583); the new tree drops the pair and its two couplings"""
    table = {}
    for tbs in sp.tree_blocks:
        for tb in tbs:
            tag, unc, chain = tb.tree
            full, unc, f, ok = [unc[0]] + list(chain), list(unc), 1.0, True
            for k in sorted(positions, reverse=True):
                left = 0 if k == 0 else full[k - 1]
                if unc[k] != unc[k + 1] or left != full[k + 1]:
                    ok = False
                    break
                f /= math.sqrt(unc[k] + 1.0)
                del unc[k:k + 2], full[k:k + 2]
            if ok:
                table[tb.tree] = ((tag, tuple(unc), tuple(full[1:])), f)
    return ft.TreeTrace(tuple(positions), table)


def pair_route(bb, data, cod, dom, n_cod, n_dom, ct, dt):
    """step 2 of the reference, one tree pair at a time through the block backend"""
    J = cod.num_legs
    tr1 = list(ct.positions if ct else ()) + [J + k for k in (dt.positions if dt else ())]
    tr2 = [k + 1 for k in tr1]
    remain = [k for k in range(J + dom.num_legs) if k not in tr1 and k not in tr2]
    where_c = {tuple(s): k for k, s in enumerate(n_cod.sectors.tolist())}
    where_d = {tuple(s): k for k, s in enumerate(n_dom.sectors.tolist())}
    rows = ft.common_sectors(n_cod, n_dom)
    new = dict(zip(rows, bb.zeros_many([(n_cod.block_size(i), n_dom.block_size(j)) for i, j in rows])))
    for n, (i_old, j_old) in enumerate(data.block_inds.tolist()):
        s = tuple(dom.sectors[j_old].tolist())
        if s not in where_c or s not in where_d:
            continue
        blk = new[(where_c[s], where_d[s])]
        for xb in cod.tree_blocks[i_old]:
            hit = ct.table.get(xb.tree) if ct else (xb.tree, 1.0)
            if hit is None:
                continue
            _, nx = n_cod.tree_block_slice(hit[0])
            for yb in dom.tree_blocks[j_old]:
                hit2 = dt.table.get(yb.tree) if dt else (yb.tree, 1.0)
                if hit2 is None:
                    continue
                _, ny = n_dom.tree_block_slice(hit2[0])
                old = bb.get_item(data.blocks[n], (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))
                old = bb.reshape(old, list(xb.multiplicities) + list(yb.multiplicities))
                part = bb.trace_partial(old, tr1, tr2, remain)
                part = bb.reshape(part, (nx.stop - nx.start, ny.stop - ny.start))
                part = bb.mul(hit[1] * np.conj(hit2[1]), part)
                key = (slice(nx.start, nx.stop), slice(ny.start, ny.stop))
                bb.set_item(blk, key, bb.get_item(blk, key) + part)
    return ft.FusionTreeData(np.array(rows, dtype=np.int64).reshape(len(rows), 2), [new[r] for r in rows])


def timed(bb, fn):
    bb.synchronize()
    t0 = time.perf_counter()
    fn()
    bb.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_calls(bb, fn):
    real = bb.lib
    bb.lib = CountingLib(real)
    try:
        fn()
        return dict(bb.lib.calls)
    finally:
        bb.lib = real


def record_shapes(bb, fn):
    """(tiles, terms, algorithmic bytes) of the tree_trace_many call `fn` makes: 8 bytes per addend read and per element written"""
    real, seen = bb.tree_trace_many, []
    bb.tree_trace_many = lambda outputs: (seen.append(list(outputs)), real(seen[-1]))[1]
    try:
        fn()
    finally:
        del bb.tree_trace_many
    (outputs,) = seen
    nbytes = 0
    for dst, terms in outputs:
        R = math.prod(dst.shape)
        nbytes += 8 * R * (1 + sum(math.prod(src.shape[i] for i in idcs1) for src, idcs1, _, _, _ in terms))
    return len(outputs), sum(len(t) for _, t in outputs), nbytes


def cases(chi):
    v = {s: max(1, round(chi * w)) for s, w in WEIGHTS.items()}
    p = {1: 1}
    return [('physical', [v, p, p], [v], (1,)), ('bond', [v, v, p], [p], (0,)), ('full', [v, v, p, p], [], (0, 2))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[512, 4096])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--grouped-only', action='store_true', help='run the grouped route alone (for a profiler run)')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    for chi in args.chi:
        for name, cod_legs, dom_legs, positions in cases(chi):
            cod, dom = space(cod_legs, 'c'), space(dom_legs, 'd')
            ct = trace_table(cod, positions)
            dropped = {a for k in positions for a in (k, k + 1)}
            n_cod, n_dom = space([leg for a, leg in enumerate(cod_legs) if a not in dropped], 'c'), dom
            rows = ft.common_sectors(cod, dom)
            data = ft.FusionTreeData(rows, [bb.random_normal((cod.block_size(i), dom.block_size(j)), seed=7 + n) for n, (i, j) in enumerate(rows)])
            grouped = lambda: ft.partial_trace(bb, data, cod, dom, n_cod, n_dom, ct, None)      # noqa: E731
            pairs = lambda: pair_route(bb, data, cod, dom, n_cod, n_dom, ct, None)               # noqa: E731
            n_pairs = sum(1 for i, j in rows for xb in cod.tree_blocks[i] if xb.tree in ct.table for _ in dom.tree_blocks[j])
            tiles, terms, nbytes = record_shapes(bb, grouped)
            res = dict(case=name, chi=chi, blocks=len(rows), tree_blocks=sum(len(t) for t in cod.tree_blocks), tree_pairs_on_diagonal=n_pairs,
                       tiles=tiles, terms=terms, algorithmic_bytes=nbytes)
            if not args.grouped_only:
                g, l = grouped(), pairs()           # the two routes compute the same thing
                lb = {tuple(r): bb.to_numpy(b) for r, b in zip(l.block_inds.tolist(), l.blocks)}
                for r, b in zip(g.block_inds.tolist(), g.blocks):
                    x, y = bb.to_numpy(b), lb[tuple(r)]
                    assert np.abs(x - y).max(initial=0.0) <= 1e-10 * max(1.0, np.abs(y).max(initial=0.0)), (name, r)
                res.update(grouped_calls=count_calls(bb, grouped), pairs_calls=count_calls(bb, pairs))
                res['pairs_launches'] = sum(res['pairs_calls'].values())
            for _ in range(args.warmup):
                grouped()
                if not args.grouped_only:
                    pairs()
            tg, tl = [], []
            for _ in range(args.reps):
                tg.append(timed(bb, grouped))
                if not args.grouped_only:
                    tl.append(timed(bb, pairs))
            res.update(grouped_ms=dict(median=statistics.median(tg), min=min(tg), max=max(tg)),
                       grouped_TBps_over_call=nbytes / (statistics.median(tg) * 1e-3) / 1e12, hbm_stream_TBps=HBM_STREAM_TBS)
            if tl:
                res.update(pairs_ms=dict(median=statistics.median(tl), min=min(tl), max=max(tl)),
                           speedup_median=statistics.median(tl) / statistics.median(tg), grouped_faster_beyond_spread=max(tg) < min(tl))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
