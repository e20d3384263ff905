"""Krylov vectors of fusion-tree tensors as pools with quantum-dimension weights, on the device.

    python scripts/tree_krylov_bench.py [chi ...] [--reps N] [--out FILE]        (default chi: 512 2048 8192)

Two structures from tests/golden/su2_chi512.npz, scaled by chi / 512 as scripts/tree_ops_bench.py scales them: 'su2' (the
coupled sectors J of the compose list, blocks rows x cols, quantum dimension 2J + 1) and 'su2xu1' (28 coupled sectors, the
three-leg codomain with its 296 fusion trees against a one-leg domain).  Per structure and chi, one JSON line each for

  cgs2      one fused CGS2 step (m = 20, passes = 2) through cyb_gram_schmidt_weighted_f64 against the unweighted
            cyb_gram_schmidt_f64 on the same n: both move (3 m + 5) n words, the weighted one n / 256 more
  lanczos   one Lanczos step (matvec, inner, two lincombs, norm, scale) of X -> A X B on the pools (_FlatTreeOps) against
            the same step on tensors (flat=False, _TreeTensorOps)

The two routes of a line alternate in one process after a warm-up; a call is timed between two device events followed by
a device synchronise, so a step holds its host side and its downloads as a user sees them.  Kernel times come from a
separate rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cyten_amd import fusion_tree as ft  # noqa: E402
from cyten_amd import krylov  # noqa: E402
from tree_ops_bench import spaces as su2xu1_spaces  # noqa: E402


def su2_spaces(chi):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'su2_chi512.npz'))
    f = chi / int(z['chi'])
    rows = [[int(x) for x in r] for r in z['compose'].tolist()]            # (J2, rows, K, cols) per coupled sector
    sec = [[r[0]] for r in rows]
    qd = np.array([r[0] + 1.0 for r in rows])
    size = lambda m: max(1, int(round(m * f)))
    cod = ft.TreeSpace.from_multiplicities(sec, [[(size(r[1]),)] for r in rows], qd, 1)
    dom = ft.TreeSpace.from_multiplicities(sec, [[(size(r[3]),)] for r in rows], qd, 1)
    return cod, dom


def structures(chi):
    cod, dom, _ = su2xu1_spaces(chi)
    return {'su2': su2_spaces(chi), 'su2xu1': (cod, dom)}


def _symmetric(rng, n):
    a = rng.standard_normal((n, n)) / np.sqrt(max(n, 1))
    return 0.5 * (a + a.T)


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

    def timed(fn):
        bb.synchronize()
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

    def alternate(a, b):
        for _ in range(args.warmup):
            a(), b()
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(a))
            tb.append(timed(b))
        return ta, tb

    for chi in args.chi:
        for name, (cod, dom) in structures(chi).items():
            rng = np.random.default_rng(7)
            pairs = ft.common_sectors(cod, dom)
            tens = lambda c, d, blocks: ft.TreeTensor(ft.FusionTreeData([(k, k) for k in range(len(blocks))], [bb.as_block(b) for b in blocks]), c, d)
            A = tens(cod, cod, [_symmetric(rng, cod.block_size(i)) for i, _ in pairs])
            B = tens(dom, dom, [_symmetric(rng, dom.block_size(j)) for _, j in pairs])
            psi = tens(cod, dom, [rng.standard_normal((cod.block_size(i), dom.block_size(j))) for i, j in pairs])
            H = krylov.TreeChainOperator(bb, [('compose_left', A), ('compose_right', B)], cod, dom)
            F = krylov._FlatTreeOps(bb, H, psi, False)
            T = krylov._TreeTensorOps(bb, H)
            n, m = F.total, 20
            elements = sum(r * c for r, c in F.shapes)

            # the fused CGS2 step, weighted against unweighted, on the same pool length
            basis = [bb.ctx.empty(n).normal_() for _ in range(m)]
            w0 = bb.ctx.empty(n).normal_()
            w = w0.clone()
            out = bb.ctx.empty(m + 1)
            unweighted = copy.copy(F.layout)          # the same pool with the table dropped: the unweighted entry runs
            unweighted.weights, unweighted.weighted = np.zeros(0), False
            U = krylov._FlatOps(bb, H, psi, layout=unweighted)
            tw, tu = alternate(lambda: F._gs(basis, w, 2, out), lambda: U._gs(basis, w, 2, out))
            nbytes = (3 * m + 5) * n * 8
            emit(dict(op='cgs2', structure=name, chi=chi, n=n, elements=elements, blocks=len(F.shapes), m=m, weighted_ms=stats(tw),
                      unweighted_ms=stats(tu), weighted_over_unweighted_median=statistics.median(tw) / statistics.median(tu),
                      weighted_TBps_best=nbytes / (min(tw) * 1e-3) / 1e12, unweighted_TBps_best=nbytes / (min(tu) * 1e-3) / 1e12))

            # one Lanczos step on pools against the same step on tensors
            def step(V, v_prev, v):
                x = V.matvec(v)
                alpha = float(np.real(V.inner(x, v)))
                x = V.lincomb(1.0, x, -alpha, v)
                x = V.lincomb(1.0, x, -0.5, v_prev)
                beta = V.norm(x)
                return V.scale(1.0 / beta, x)
            pf = F.enter(psi)
            pf = F.scale(1.0 / F.norm(pf), pf)
            pt = T.scale(1.0 / T.norm(psi), psi)
            a, b = step(F, pf, pf), step(T, pt, pt)
            got = {tuple(r): bb.to_numpy(x) for r, x in zip(F.leave(a).block_inds.tolist(), F.leave(a).blocks)}
            for r, x in zip(b.block_inds.tolist(), b.blocks):
                want = bb.to_numpy(x)
                assert np.abs(got[tuple(r)] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (name, chi, r)
            tf, tt = alternate(lambda: step(F, pf, pf), lambda: step(T, pt, pt))
            emit(dict(op='lanczos', structure=name, chi=chi, n=n, elements=elements, blocks=len(F.shapes), pools_ms=stats(tf), tensors_ms=stats(tt),
                      tensors_over_pools_median=statistics.median(tt) / statistics.median(tf)))


if __name__ == '__main__':
    main()
