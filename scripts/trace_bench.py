"""Grouped partial trace against the per-block route, on the device.

    python scripts/trace_bench.py [chi ...] [--reps N] [--out FILE]

Tensor [v(+), p(+), p(-), v(-)] with v = workloads.u1_leg(chi) and the two-state physical leg of the U(1) MPS config, all
charge-allowed blocks.  Three traces:

  physical  pair (1, 2): every on-diagonal block is read once in full, the result has the v x v block structure
  bond      pair (0, 3): only block diagonals are read, the result is a p x p tensor
  full      trace_full:  one number

For each, two routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a
device synchronise:

  grouped   abelian.partial_trace -> ONE cyb_trace_grouped_f64 launch
  loop      the only route without it: bb.trace_partial per on-diagonal block (a contiguous copy of the block and a grouped
            GEMM against a vector of ones each) and one Block `+` per further contribution to the same result block

Printed per case (one JSON line): median / min / max milliseconds of both routes, their C-ABI calls by name, whether the slowest
grouped run beat the fastest loop run, and for `physical` the algorithmic bytes (on-diagonal sources read once + results
written) over the grouped time.  The results of the two routes are compared before anything is timed."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cyten_amd import abelian as ab  # noqa: E402
from cyten_amd import workloads as wl  # noqa: E402

HBM_STREAM_TBS = 6.3      # MI355X_MICROARCH.md: achievable streaming rate


class CountingLib:
    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


def loop_partial_trace(bb, t, pairs):
    """partial_trace block by block: the host matching of abelian.partial_trace, then bb.trace_partial per block and
    Block.__add__ per accumulation (the shape of abelian.cpp:3016-3029)"""
    maps = [ab.dual_sector_map(t.symmetry, t.legs[i], t.legs[j]) for i, j in pairs]
    idcs1, idcs2 = [i for i, _ in pairs], [j for _, j in pairs]
    remaining = [k for k in range(t.nlegs) if k not in idcs1 + idcs2]
    acc = {}
    for blk, row in zip(t.blocks, t.block_inds):
        if any(m[row[i]] != row[j] for (i, j), m in zip(pairs, maps)):
            continue
        part = bb.trace_partial(blk, idcs1, idcs2, remaining)
        key = tuple(int(row[k]) for k in remaining)
        acc[key] = acc[key] + part if key in acc else part
    if not remaining:
        return float(bb.to_numpy(acc[()]).reshape(())) if acc else 0.0
    keys = sorted(acc, key=lambda k: k[::-1])
    return ab.AbelianTensor(t.symmetry, [t.legs[k] for k in remaining], [acc[k] for k in keys], np.array(keys, dtype=np.int64),
                            sum(1 for k in remaining if k < t.num_codomain))


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[1024, 4096])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    for chi in args.chi:
        v = wl.u1_leg(chi, 2.0)
        p = wl.make_leg((0,), [[-1], [1]], [1, 1], +1)
        spec = wl.random_tensor((0,), [v, p, wl.flip(p), wl.flip(v)], np.random.default_rng(wl.DEFAULT_SEED), num_codomain=2)
        t = ab.AbelianTensor.from_spec(bb, spec)
        for name, pairs in [('physical', [(1, 2)]), ('bond', [(0, 3)]), ('full', [(0, 3), (1, 2)])]:
            grouped = (lambda: ab.trace_full(bb, t)) if name == 'full' else (lambda: ab.partial_trace(bb, t, pairs))
            loop = lambda: loop_partial_trace(bb, t, pairs)
            # the two routes compute the same thing
            g, l = grouped(), loop()
            if name == 'full':
                scale = sum(float(np.abs(np.einsum('abba->ab', b)).sum()) for b, r in zip(spec.blocks, spec.block_inds) if r[0] == r[3] and r[1] == r[2])
                assert abs(g - l) <= 1e-12 * scale, (g, l)
            else:
                assert np.array_equal(g.block_inds, l.block_inds)
                for x, y in zip(g.blocks, l.blocks):
                    x, y = bb.to_numpy(x), bb.to_numpy(y)
                    assert np.abs(x - y).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(y).max(initial=0.0))
            calls_g, calls_l = count_calls(bb, grouped), count_calls(bb, loop)
            for _ in range(args.warmup):
                grouped()
                loop()
            tg, tl = [], []
            for _ in range(args.reps):
                tg.append(timed(bb, grouped))
                tl.append(timed(bb, loop))
            on_diag = [b for b, r in zip(spec.blocks, spec.block_inds) if all(r[i] == r[j] for i, j in pairs)]
            res = dict(case=name, chi=chi, blocks=len(spec.blocks), on_diagonal=len(on_diag),
                       grouped_ms=dict(median=statistics.median(tg), min=min(tg), max=max(tg)),
                       loop_ms=dict(median=statistics.median(tl), min=min(tl), max=max(tl)),
                       speedup_median=statistics.median(tl) / statistics.median(tg),
                       grouped_faster_beyond_spread=max(tg) < min(tl),
                       grouped_calls=calls_g, loop_calls=calls_l, loop_launches=sum(calls_l.values()))
            if name == 'physical':
                out_elems = sum(int(np.prod(b.shape)) for b in g.blocks)
                nbytes = 8 * (sum(b.size for b in on_diag) + out_elems)
                res.update(algorithmic_bytes=nbytes, grouped_TBps=nbytes / (statistics.median(tg) * 1e-3) / 1e12,
                           grouped_TBps_best=nbytes / (min(tg) * 1e-3) / 1e12, hbm_stream_TBps=HBM_STREAM_TBS)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
