"""Fusion-tree from_grid (ONE launch, every element written once) against the routes available before, on the device.

    python scripts/tree_grid_bench.py [chi ...] [--reps N] [--out FILE]

SU(2)-shaped structures built from the fusion rules alone (the spaces of scripts/tree_trace_bench.py): a bond leg v with the
spins 0 .. 2 and multiplicities that add up to chi, a site leg p of spin 1/2.

  direct_sum  [[A, None], [None, B]] of (v, p) <- v tensors: adding two MPS; both legs double
  expand      [[A, P]] of (v, p) <- v and (v, p) <- v' with v' an eighth of v: subspace expansion; only the domain leg is
              stacked, so every window is a column range of its tile (runs shorter than the rows of the result)
  mpo         a 5 x 5 grid of (w, p) <- (p, w) operators on a trivial w: identities on the diagonal, operators in the first
              column and the last row, None elsewhere -- independent of chi, bound by the cost of a call

Three routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise, profiler off; medians of --reps (default 7) with their spread, and the C-ABI calls of each by name:

  place       fusion_tree.from_grid -> ONE cyb_tree_place_f64 launch into blocks that are not zero-filled
  forest      the reference's loop (fusion_tree_backend.cpp:3394-3515) on HipBlockBackend blocks: zeros, then per (entry, block,
              codomain forest, domain forest) get_item, reshape, copy_block, reshape, get_item, +, set_item, reshape, set_item.
              (Two-leg sides: a forest of these spaces is one tree.)
  zero_copy   zeros_many + ONE copy_many of (window, entry tile) pairs: the result is written twice

Beside them the launch alone (``tree_place_many`` on the captured records) and, as the streaming yardstick, ONE contiguous
``copy_many`` of as many elements as the windows hold.  Kernel times come from a profiler run of its own:
``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/tree_grid_bench.py 4096``."""
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


def stack(parts):
    """(stacked multiplicities, cumulative table) of one-leg multiplicity dicts"""
    keys = sorted({k for p in parts for k in p})
    table = {k: [0] + np.cumsum([p.get(k, 0) for p in parts]).tolist() for k in keys}
    return {k: table[k][-1] for k in keys}, table


def build(bb, rows, cols, present, cod_rest, dom_rest, seed=7):
    """grid entries on (rows[i], *cod_rest) <- (*dom_rest, cols[j]) for the cells in `present`, the new spaces and the tables"""
    (rm, left), (cm, right) = stack(rows), stack(cols)
    n_cod, n_dom = space([rm] + cod_rest, 'c'), space(dom_rest + [cm], 'd')
    grid = []
    for i, r in enumerate(rows):
        g = []
        for j, c in enumerate(cols):
            if (i, j) not in present:
                g.append(None)
                continue
            cod, dom = space([r] + cod_rest, 'c'), space(dom_rest + [c], 'd')
            rws = ft.common_sectors(cod, dom)
            data = ft.FusionTreeData(rws, [bb.random_normal((cod.block_size(a), dom.block_size(b)), seed=seed + 100 * (5 * i + j) + n)
                                           for n, (a, b) in enumerate(rws)])
            g.append(ft.TreeTensor(data, cod, dom))
        grid.append(g)
    return grid, n_cod, n_dom, left, right


def windows_of(bb, grid, n_cod, n_dom, left, right):
    """(block shapes, copy windows) of the result: a window is (block, rows, first run column, runs, run width, run pitch, tile)"""
    seen, orig = [], ft._place_windows
    ft._place_windows = lambda b, shapes, cplx, ws: (seen.append((shapes, [w for w in ws if w.h and w.nq and w.wn])), orig(b, shapes, cplx, ws))[1]
    try:
        ft.from_grid(bb, grid, n_cod, n_dom, left, right, discard=False)
    finally:
        ft._place_windows = orig
    return seen[0]


def _window_view(bb, out, w):
    tile = bb.get_item(out, (slice(w.x0, w.x1), slice(w.y0, w.y1)))
    t3 = bb.reshape(tile, (w.x1 - w.x0, w.nq, (w.y1 - w.y0) // w.nq))
    return bb.get_item(t3, (slice(w.r0, w.r0 + w.h), slice(None), slice(w.c0, w.c0 + w.wn)))


def zero_copy_route(bb, shapes, windows):
    outs = bb.zeros_many(shapes)
    bb.copy_many([(_window_view(bb, outs[w.n], w), bb.reshape(w.src, (w.h, w.nq, w.wn))) for w in windows if w.src is not None])
    return outs


def forest_route(bb, grid, n_cod, n_dom, left, right):
    """the reference's loop; trees are matched by key (a forest of a two-leg side holds one tree)"""
    rows = ft.common_sectors(n_cod, n_dom)
    new = dict(zip(rows, bb.zeros_many([(n_cod.block_size(i), n_dom.block_size(j)) for i, j in rows])))
    of_sector = {tuple(n_dom.sectors[j].tolist()): (i, j) for i, j in rows}
    for i, row in enumerate(grid):
        for j, op in enumerate(row):
            if op is None:
                continue
            for n, (ic, jd) in enumerate(op.block_inds.tolist()):
                key = of_sector.get(tuple(op.domain.sectors[jd].tolist()))
                if key is None:
                    continue
                for xe in op.codomain.tree_blocks[ic]:
                    _, x = n_cod.tree_block_slice(xe.tree)
                    rest_c = math.prod(x.multiplicities[1:])
                    Ls = slice(left[xe.uncoupled[0]][i], left[xe.uncoupled[0]][i + 1])
                    for ye in op.domain.tree_blocks[jd]:
                        _, y = n_dom.tree_block_slice(ye.tree)
                        rest_d = math.prod(y.multiplicities[:-1])
                        Rs = slice(right[ye.uncoupled[-1]][j], right[ye.uncoupled[-1]][j + 1])
                        if xe.stop == xe.start or ye.stop == ye.start:
                            continue
                        piece = bb.get_item(op.blocks[n], (slice(xe.start, xe.stop), slice(ye.start, ye.stop)))
                        piece = bb.reshape(piece, (1, xe.multiplicities[0], rest_c, 1, rest_d, ye.multiplicities[-1]))
                        sl = (slice(x.start, x.stop), slice(y.start, y.stop))
                        block = bb.copy_block(bb.get_item(new[key], sl))
                        final = block.shape
                        block = bb.reshape(block, (1, x.multiplicities[0], rest_c, 1, rest_d, y.multiplicities[-1]))
                        k6 = (slice(None), Ls, slice(None), slice(None), slice(None), Rs)
                        bb.set_item(block, k6, bb.get_item(block, k6) + piece)
                        bb.set_item(new[key], sl, bb.reshape(block, final))
    return ft.discard_zero_blocks(bb, ft.FusionTreeData(np.array(rows, dtype=np.int64).reshape(len(rows), 2), [new[r] for r in rows]), 0.0)


def cases(chi):
    v = {k: max(1, round(chi * w)) for k, w in WEIGHTS.items()}
    v8 = {k: max(1, m // 8) for k, m in v.items()}
    p, w = {1: 1}, {0: 1}
    mpo = {(k, k) for k in range(5)} | {(k, 0) for k in range(5)} | {(4, k) for k in range(5)}
    return [('direct_sum', [v, v], [v, v], {(0, 0), (1, 1)}, [p], []), ('expand', [v], [v, v8], {(0, 0), (0, 1)}, [p], []),
            ('mpo', [w] * 5, [w] * 5, mpo, [p], [p])]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[4096])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    done = set()
    for chi in args.chi:
        for name, rows, cols, present, cod_rest, dom_rest in cases(chi):
            if name == 'mpo' and name in done:
                continue                        # (does not depend on chi)
            done.add(name)
            grid, n_cod, n_dom, left, right = build(bb, rows, cols, present, cod_rest, dom_rest)
            gargs = (grid, n_cod, n_dom, left, right)
            shapes, windows = windows_of(bb, *gargs)
            place = lambda: ft.from_grid(bb, *gargs)                                   # noqa: E731
            forest = lambda: forest_route(bb, *gargs)                                  # noqa: E731
            zero_copy = lambda: zero_copy_route(bb, shapes, windows)                   # noqa: E731
            outs = bb.empty_many(shapes)
            records = [(_window_view(bb, outs[w.n], w), w.src, w.n_row, w.coeff) for w in windows]
            launch = lambda: bb.tree_place_many(records)                               # noqa: E731
            n_el = sum(w.h * w.nq * w.wn for w in windows)
            n_src = sum(w.h * w.nq * w.wn for w in windows if w.src is not None)
            flat = bb.empty_many([(n_el,), (n_el,)])
            yard = lambda: bb.copy_many([(flat[0], flat[1])])                          # noqa: E731
            g, f, z = place(), forest(), zero_copy()            # the three routes compute the same thing
            fb = {tuple(r): bb.to_numpy(blk) for r, blk in zip(f.block_inds.tolist(), f.blocks)}
            assert len(g.blocks) == len(z) == len(shapes)
            for r, blk, zb in zip(g.block_inds.tolist(), g.blocks, z):
                assert np.array_equal(bb.to_numpy(blk), fb[tuple(r)]) and np.array_equal(bb.to_numpy(blk), bb.to_numpy(zb)), (name, r)
            res = dict(case=name, chi=None if name == 'mpo' else chi, entries=len(present), result_blocks=len(shapes), windows=len(windows),
                       zero_windows=sum(w.src is None for w in windows), elements_written=n_el, algorithmic_bytes=8 * (n_el + n_src),
                       yardstick_bytes=16 * n_el, place_calls=count_calls(bb, place), forest_calls=count_calls(bb, forest),
                       zero_copy_calls=count_calls(bb, zero_copy))
            res['forest_launches'] = sum(res['forest_calls'].values())
            routes = dict(place=place, forest=forest, zero_copy=zero_copy, launch=launch, yardstick=yard)
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
            res.update(launch_TBps=8 * (n_el + n_src) / (med(times['launch']) * 1e-3) / 1e12,
                       yardstick_TBps=16 * n_el / (med(times['yardstick']) * 1e-3) / 1e12, hbm_stream_TBps=HBM_STREAM_TBS,
                       speedup_over_forest=med(times['forest']) / med(times['place']),
                       speedup_over_zero_copy=med(times['zero_copy']) / med(times['place']),
                       place_faster_than_zero_copy_beyond_spread=max(times['place']) < min(times['zero_copy']))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as fh:
                    fh.write(line + '\n')


if __name__ == '__main__':
    main()
