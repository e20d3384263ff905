"""scale_axis, mask_contract and inner of fusion-tree tensors (ONE tree_axis_many / inner_weighted_many call each) against the
per-tree-block route, on the device.

    python scripts/tree_ops_bench.py [chi ...] [--reps N] [--warmup N] [--out FILE]

The tensor has the SU(2) x U(1) structure of tests/golden/su2_chi512.npz: the codomain is (bond leg, site, site) with the 296
fusion trees of its 28 coupled sectors -- a tree's rows are the multiplicity of its bond-leg sector, the site legs have
multiplicity 1 -- and the domain is one leg with as many columns per coupled sector as the codomain has rows.  `chi` scales
the multiplicities of the bond leg by chi / 512.  The operations act on the bond leg (leg 0, 296 records of row ranges) and on
the domain leg (28 records of column ranges).

Two routes run alternately in one process after a warm-up:

  grouped   fusion_tree.scale_axis / mask_contract / inner: one descriptor list, one launch
  loop      per tree block: get_item (the rows of the tree), reshape to the multiplicities, scale_axis_many / mask_gather_many,
            reshape back, copy_many into the rows of the tree in the result block; for the norm one norm_many and one host
            wait per coupled sector

Each call is timed between two device events recorded in the stream around it, followed by a device synchronise, so the time
holds the host side of the call (building and uploading the descriptors) as a user sees it.  For the grouped route a second
figure is taken behind a stretch of other device work that hides the host side: the device time of the call, from which the
achieved bandwidth follows as (bytes read + bytes written) / time with the bytes computed from the shapes.  One JSON line per
operation and chi: median / min / max milliseconds of both routes, the device time and GB/s of the grouped one.  The results of
the two routes are compared before anything is timed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cyten_amd import _lib  # noqa: E402
from cyten_amd import fusion_tree as ft  # noqa: E402


def spaces(chi):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'su2_chi512.npz'))
    f = chi / int(z['chi'])
    mult = {tuple(s): max(1, int(round(int(m) * f))) for s, m in zip(z['h_sectors'].tolist(), z['h_mults'].tolist())}
    by_key: dict = {}
    for r in sorted(z['h_rows_old'].tolist(), key=lambda r: (r[0], r[1], r[-2])):
        by_key.setdefault((r[0], r[1]), []).append(r)
    keys = sorted(by_key)
    mults = [[(mult[(r[2], r[3])], 1, 1) for r in by_key[k]] for k in keys]
    names = [[tuple(r[:-2]) for r in by_key[k]] for k in keys]
    unc = [[((r[2], r[3]), 's', 's') for r in by_key[k]] for k in keys]
    qd = np.array([k[1] + 1.0 for k in keys])
    cod = ft.TreeSpace.from_multiplicities(keys, mults, qd, 3, names, unc)
    dom = ft.TreeSpace.from_multiplicities(keys, [[(int(cod.block_size(i)),)] for i in range(len(keys))], qd, 1,
                                           [[('d', k)] for k in keys], [[(k,)] for k in keys])
    bond_keys = sorted(mult)
    bond = ft.TreeSpace.from_multiplicities(bond_keys, [[(mult[k],)] for k in bond_keys], None, 1, [[('b', k)] for k in bond_keys],
                                            [[(k,)] for k in bond_keys])
    return cod, dom, bond


def loop_axis(bb, data, cod, dom, leg, per_key, what, mask=None):
    """the per-tree-block route: slice, reshape, one block-backend call, reshape back, set the slice of the result"""
    side, idx = ft._parse_leg(cod, dom, leg)
    space = dom if side else cod
    new_space = space if what == 'scale' else ft._masked_space(space, idx, mask, True)
    shapes = [(cod.block_size(i), new_space.block_size(j)) if side else (new_space.block_size(i), dom.block_size(j)) for i, j in data.block_inds.tolist()]
    outs = bb.zeros_many(shapes)
    for (i, j), blk, out in zip(data.block_inds.tolist(), data.blocks, outs):
        other = blk.shape[0] if side else blk.shape[1]
        for tb in space.tree_blocks[j if side else i]:
            key = tb.uncoupled[idx]
            nb = new_space.tree_block_slice(tb.tree)[1]
            t = bb.get_item(blk, (slice(None), slice(tb.start, tb.stop)) if side else (slice(tb.start, tb.stop), slice(None)))
            t = bb.reshape(bb.contiguous(t), ((other,) + tb.multiplicities) if side else (tb.multiplicities + (other,)))
            ax = idx + 1 if side else idx
            r = bb.scale_axis_many([(t, per_key[key], ax)])[0] if what == 'scale' else bb.mask_gather_many([(t, per_key[key], ax)])[0]
            dst = bb.get_item(out, (slice(None), slice(nb.start, nb.stop)) if side else (slice(nb.start, nb.stop), slice(None)))
            bb.copy_many([(dst, bb.reshape(r, dst.shape))])
    return outs


def loop_norm(bb, data, cod):
    q = cod.qdims[data.block_inds[:, 0]]
    return float(np.sqrt(sum(float(qi) * bb.norm_many([b]) ** 2 for qi, b in zip(q, data.blocks))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[512, 2048, 8192])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    e0, e1 = bb.ctx.event(), bb.ctx.event()
    pad = bb.empty_many([(1 << 25,), (1 << 25,)])

    def busy():
        for _ in range(6):
            _lib.check(bb.lib.cyb_memcpy_d2d(bb.ctx.handle, C.c_void_p(pad[0].ptr), C.c_void_p(pad[1].ptr), 8 << 25))

    def timed(fn, hide_host=False):
        bb.synchronize()
        if hide_host:
            busy()
        bb.ctx.record(e0)
        fn()
        bb.ctx.record(e1)
        bb.synchronize()
        return bb.ctx.elapsed_ms(e0, e1)

    def stats(ts):
        return dict(median=statistics.median(ts), min=min(ts), max=max(ts))

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    for chi in args.chi:
        rng = np.random.default_rng(7)
        cod, dom, bond = spaces(chi)
        rows = [(i, i) for i in range(cod.num_sectors)]
        data = ft.FusionTreeData(rows, [bb.as_block(rng.standard_normal((cod.block_size(i), dom.block_size(i)))) for i in range(cod.num_sectors)])
        n_elem = sum(b.size for b in data.blocks)
        bond_keys = ft.leg_keys(bond)
        diag = ft.FusionTreeData([(k, k) for k in range(bond.num_sectors)], [bb.as_block(rng.random(int(m)) + 0.5) for m in bond.multiplicities])
        keep = [np.sort(rng.choice(int(m), size=(int(m) + 1) // 2, replace=False)) for m in bond.multiplicities]
        mask = ft.TreeMask(bond_keys, [int(m) for m in bond.multiplicities], keep)
        ddiag = ft.FusionTreeData(rows, [bb.as_block(rng.random(dom.block_size(i)) + 0.5) for i in range(dom.num_sectors)])
        dkeep = [np.sort(rng.choice(int(m), size=(int(m) + 1) // 2, replace=False)) for m in dom.multiplicities]
        dmask = ft.TreeMask(ft.leg_keys(dom), [int(m) for m in dom.multiplicities], dkeep)
        f_of = dict(zip(bond_keys, diag.blocks))
        k_of = dict(zip(bond_keys, keep))
        cases = {
            'scale_axis bond leg': (lambda: ft.scale_axis(bb, data, cod, dom, diag, bond, 0).blocks,
                                    lambda: loop_axis(bb, data, cod, dom, 0, f_of, 'scale'), 2.0),
            'scale_axis domain leg': (lambda: ft.scale_axis(bb, data, cod, dom, ddiag, dom, 3).blocks,
                                      lambda: loop_axis(bb, data, cod, dom, 3, dict(zip(ft.leg_keys(dom), ddiag.blocks)), 'scale'), 2.0),
            'mask_contract bond leg': (lambda: ft.mask_contract(bb, data, cod, dom, mask, 0, discard=False)[0].blocks,
                                       lambda: loop_axis(bb, data, cod, dom, 0, k_of, 'mask', mask), 1.0),
            'mask_contract domain leg': (lambda: ft.mask_contract(bb, data, cod, dom, dmask, 3, discard=False)[0].blocks,
                                         lambda: loop_axis(bb, data, cod, dom, 3, dict(zip(ft.leg_keys(dom), dkeep)), 'mask', dmask), 1.0),
        }
        for name, (grouped, loop, traffic) in cases.items():
            g, l = grouped(), loop()
            for x, y in zip(g, l):
                gx, ly = bb.to_numpy(x), bb.to_numpy(y)
                assert np.array_equal(gx, ly), name
            for _ in range(args.warmup):
                grouped(), loop()
            tg, tl, td = [], [], []
            for _ in range(args.reps):
                tg.append(timed(grouped))
                tl.append(timed(loop))
                td.append(timed(grouped, hide_host=True))
            nbytes = 8 * n_elem * traffic        # scale: read + write everything; mask: read half, write half
            emit(dict(op=name, chi=chi, tree_blocks=sum(len(t) for t in cod.tree_blocks), elements=n_elem, grouped_ms=stats(tg), loop_ms=stats(tl),
                      speedup_median=statistics.median(tl) / statistics.median(tg), grouped_device_ms=stats(td),
                      grouped_GBps_best=nbytes / (min(td) * 1e-3) / 1e9))
        want = loop_norm(bb, data, cod)
        got = ft.norm(bb, data, cod)
        assert abs(got - want) <= 1e-12 * want and abs(ft.inner(bb, data, data, cod, do_dagger=True) - want ** 2) <= 1e-12 * want ** 2
        for _ in range(args.warmup):
            ft.norm(bb, data, cod), loop_norm(bb, data, cod)
        tg, tl, ti = [], [], []
        for _ in range(args.reps):
            tg.append(timed(lambda: ft.norm(bb, data, cod)))
            tl.append(timed(lambda: loop_norm(bb, data, cod)))
            ti.append(timed(lambda: ft.inner(bb, data, data, cod, do_dagger=True)))
        emit(dict(op='norm / inner', chi=chi, blocks=len(data.blocks), elements=n_elem, grouped_norm_ms=stats(tg), loop_norm_ms=stats(tl),
                  grouped_inner_ms=stats(ti), speedup_median=statistics.median(tl) / statistics.median(tg),
                  inner_GBps_best=2 * 8 * n_elem / (min(ti) * 1e-3) / 1e9))


if __name__ == '__main__':
    main()
