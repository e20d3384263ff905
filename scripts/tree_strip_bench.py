"""Factorized fusion-tree moves (braids inside one side: ONE strip launch per side) against the pair route, on the device.

    python scripts/tree_strip_bench.py [chi ...] [--reps N] [--out FILE]

SU(2)-shaped structures built from the fusion rules alone (the spaces of scripts/tree_trace_bench.py): a bond leg v with the
spins 0 .. 2 and multiplicities that add up to chi, a site leg p of spin 1/2.  The coefficients are stand-ins of the right
sparsity (a 2 x 2 rotation where two couplings mix, 1 where one does): the symmetry layer hands them over as data, and no
route's time depends on their values.

  exchange  (v, p, p) <- v, the two physical legs of a two-site wave function exchanged: a codomain pass, 1-2 terms per strip
  dagger    v <- (v, p, p), the daggered shape: a domain pass, 1-2 terms per strip
  both      (v, p, p) <- (v', p, p) with v' an eighth of v, the physical legs of both sides exchanged: two passes
  inner     v <- (a, b) with a an eighth of v and b of spin 1/2 with the multiplicity 8, the two domain legs exchanged: the new
            innermost level is a with the stride 8 -- the innermost level moves, the loads are gathered 8 bytes at a time

Routes, run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise, profiler off; medians of --reps (default 7) with their spread, and the C-ABI calls of each by name:

  strip      fusion_tree.transform_tensor_factorized -> ONE cyb_tree_strip_f64 launch per side into blocks that are not zero-filled
  pair       fusion_tree.transform_tensor fed the multiplied-out pair mapping: one zero fill and ONE
             cyb_lincomb_strided_batched_f64 launch over |codomain trees| x |domain trees| update records
  launch     the ``tree_strip_many`` calls of `strip` alone, on the captured records
  yardstick  ONE contiguous ``copy_many`` of as many bytes as `launch` moves (reads + writes)

Kernel times come from a profiler run of its own:
``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/tree_strip_bench.py 4096``."""
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
from tree_trace_bench import HBM_STREAM_TBS, WEIGHTS, count_calls, space, timed  # noqa: E402

ROTATION = ((0.6, 0.8), (-0.8, 0.6))


def swapped(legs, k, tag):
    """(new space, table, axes): the legs k and k + 1 of space(legs) exchanged.  A tree (tag, uncoupled, couplings) goes to the
    trees with the two uncoupled spins exchanged and any admissible coupling between them (none to choose for k = 0)"""
    old = space(legs, tag)
    new_legs = list(legs)
    new_legs[k], new_legs[k + 1] = legs[k + 1], legs[k]
    new = space(new_legs, tag.upper())
    by_frame = {}
    for tbs in new.tree_blocks:
        for tb in tbs:
            _, unc, chain = tb.tree
            frame = (unc, chain[:k - 1] + chain[k:]) if k else (unc, chain)
            by_frame.setdefault(frame, []).append(tb.tree)
    table = {}
    for tbs in old.tree_blocks:
        for tb in tbs:
            _, unc, chain = tb.tree
            unc2 = unc[:k] + (unc[k + 1], unc[k]) + unc[k + 2:]
            cands = sorted(by_frame.get((unc2, chain[:k - 1] + chain[k:]) if k else (unc2, chain), []))
            cands = [t for t in cands if t[2][-1:] == chain[-1:]]             # (the coupled sector stays)
            assert 1 <= len(cands) <= 2
            a = 0 if len(cands) == 1 or chain[k - 1] == cands[0][2][k - 1] else 1
            table[tb.tree] = {t: (ROTATION[a][b] if len(cands) == 2 else 1.0) for b, t in enumerate(cands)}
    axes = list(range(len(legs)))
    axes[k], axes[k + 1] = k + 1, k
    return old, new, table, axes


def product_mapping(cod, dom, splitting, fusion):
    """the two maps multiplied out into the data of a TreePairMapping; None: the identity"""
    a = splitting if splitting is not None else {tb.tree: {tb.tree: 1.0} for tbs in cod.tree_blocks for tb in tbs}
    b = fusion if fusion is not None else {tb.tree: {tb.tree: 1.0} for tbs in dom.tree_blocks for tb in tbs}
    mapping = {}
    for X, ta in a.items():
        sx = cod.sectors[cod.tree_block_slice(X)[0]].tolist()
        for Y, tb in b.items():
            if dom.sectors[dom.tree_block_slice(Y)[0]].tolist() == sx:
                mapping[(X, Y)] = {(x2, y2): ca * cb for x2, ca in ta.items() for y2, cb in tb.items()}
    return mapping


def cases(chi):
    v = {k: max(1, round(chi * w)) for k, w in WEIGHTS.items()}
    v8 = {k: max(1, m // 8) for k, m in v.items()}
    p, b = {1: 1}, {1: 8}
    # (name, codomain legs, exchanged codomain position or None, domain legs, exchanged domain position or None)
    return [('exchange', [v, p, p], 1, [v], None), ('dagger', [v], None, [v, p, p], 1), ('both', [v, p, p], 1, [v8, p, p], 1),
            ('inner', [v], None, [v8, b], 0)]


def captured_launches(bb, fn):
    """the record lists of the ``tree_strip_many`` calls `fn` makes"""
    real, seen = bb.tree_strip_many, []
    bb.tree_strip_many = lambda outs: (seen.append(list(outs)), real(seen[-1]))[1]
    try:
        fn()
    finally:
        del bb.tree_strip_many
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[4096])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    for chi in args.chi:
        for name, cod_legs, kc, dom_legs, kd in cases(chi):
            J, K = len(cod_legs), len(dom_legs)
            N = J + K
            if kc is None:
                cod = n_cod = space(cod_legs, 'c')
                splitting, c_idcs = None, list(range(J))
            else:
                cod, n_cod, splitting, c_idcs = swapped(cod_legs, kc, 'c')
            if kd is None:
                dom = n_dom = space(dom_legs, 'd')
                fusion, axes2 = None, list(range(K))
            else:
                dom, n_dom, fusion, axes2 = swapped(dom_legs, kd, 'd')
            d_idcs = [(N - 1) - a for a in axes2]
            rows = ft.common_sectors(cod, dom)
            data = ft.FusionTreeData(rows, [bb.random_normal((cod.block_size(i), dom.block_size(j)), seed=7 + n) for n, (i, j) in enumerate(rows)])
            mapping = product_mapping(cod, dom, splitting, fusion)
            strip = lambda: ft.transform_tensor_factorized(bb, data, cod, dom, n_cod, n_dom, c_idcs, d_idcs, splitting, fusion)      # noqa: E731
            pair = lambda: ft.transform_tensor(bb, data, cod, dom, n_cod, n_dom, c_idcs, d_idcs, mapping)                            # noqa: E731
            held = []                          # (the result of the captured call: its blocks are the destinations of `launch`)
            calls = captured_launches(bb, lambda: held.append(strip()))
            launch = lambda: [bb.tree_strip_many(outs) for outs in calls]                                                            # noqa: E731
            n_written = sum((stop - start) * dst.shape[1 - side] for outs in calls for dst, side, start, stop, _, _, _ in outs)
            n_read = sum((stop - start) * dst.shape[1 - side] * len(terms) for outs in calls for dst, side, start, stop, _, _, terms in outs)
            n_yard = (n_written + n_read + 1) // 2
            flat = bb.empty_many([(n_yard,), (n_yard,)])
            yard = lambda: bb.copy_many([(flat[0], flat[1])])                                                                        # noqa: E731
            g, f = strip(), pair()             # the two routes compute the same thing
            fb = {tuple(r): bb.to_numpy(blk) for r, blk in zip(f.block_inds.tolist(), f.blocks)}
            assert sorted(fb) == sorted(tuple(r) for r in g.block_inds.tolist())
            worst = max(float(np.abs(bb.to_numpy(blk) - fb[tuple(r)]).max(initial=0.0)) for r, blk in zip(g.block_inds.tolist(), g.blocks))
            assert worst <= 1e-12, (name, worst)
            res = dict(case=name, chi=chi, blocks=len(g.blocks), codomain_trees=sum(len(t) for t in n_cod.tree_blocks),
                       domain_trees=sum(len(t) for t in n_dom.tree_blocks), strips=sum(len(o) for o in calls),
                       strip_terms=sum(len(o[6]) for outs in calls for o in outs), pair_records=sum(len(v) for v in mapping.values()),
                       max_terms_per_strip=max(len(o[6]) for outs in calls for o in outs), elements_written=n_written,
                       algorithmic_bytes=8 * (n_written + n_read), yardstick_bytes=16 * n_yard, max_abs_diff_to_pair=worst,
                       strip_calls=count_calls(bb, strip), pair_calls=count_calls(bb, pair))
            routes = dict(strip=strip, pair=pair, launch=launch, yardstick=yard)
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            times = {k: [] for k in routes}
            for _ in range(args.reps):
                for k, fn in routes.items():
                    times[k].append(timed(bb, fn))
            med = statistics.median
            for k, t in times.items():
                res[k + '_ms'] = dict(median=med(t), min=min(t), max=max(t))
            res.update(launch_TBps=8 * (n_written + n_read) / (med(times['launch']) * 1e-3) / 1e12,
                       yardstick_TBps=16 * n_yard / (med(times['yardstick']) * 1e-3) / 1e12, hbm_stream_TBps=HBM_STREAM_TBS,
                       launch_over_yardstick=med(times['launch']) / med(times['yardstick']),
                       speedup_over_pair=med(times['pair']) / med(times['strip']),
                       strip_faster_than_pair_beyond_spread=max(times['strip']) < min(times['pair']))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as fh:
                    fh.write(line + '\n')
            del held, calls, flat, data, g, f, fb


if __name__ == '__main__':
    main()
