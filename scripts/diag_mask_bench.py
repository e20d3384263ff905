"""Singular values after a decomposition: the grouped segment kernels against the per-sector route, on the device.

    python scripts/diag_mask_bench.py [chi ...] [--reps N] [--out FILE] [--grouped-only]

For the bond legs ``workloads.u1_leg(chi)`` and ``workloads.u1u1_leg(chi)`` (default chi = 1024 and 4096; 59 sectors for
U(1) x U(1) at chi = 4096) a seeded list of singular values per sector -- descending inside a sector, normalised over the bond --
and U / Vh blocks of a two-site update (``2k x k`` and ``k x 2k`` for a sector of multiplicity k).  The timed pipeline is what a
bond update does with S: keep S above a cutoff (the median: half the bond survives), project U / S / Vh, report the entropy:

    flags = diagonal_compare(S, 'ge', cutoff);  mask = diagonal_to_mask(flags)
    U, S, Vh = svd_apply_mask(U, S, Vh, mask);  entropy(p)          with p = S^2 prepared outside the timed region

Two routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise:

  grouped   the functions above: one cyb_seg_binary, one cyb_seg_compact (+ its 8 n download), one cyb_mask_gather_batched_f64,
            one cyb_seg_reduce (+ its 16 n download)
  loop      a Python loop over the sectors with the single-block methods, the calls the reference's per-sector loops issue
            (abelian.cpp:1707-1728, :646-673, :3163-3173): ``block >= cutoff``, ``any``, the download of the flags, ``apply_mask``
            of the three blocks, and for the entropy ``block * stable_log(block)`` and ``sum_all``

Printed per case (one JSON line): median / min / max milliseconds of both routes, their C-ABI calls by name, the number of
host synchronisations (downloads) of each, whether the slowest grouped run beat the fastest loop run, and the bytes the entropy
reduction reads.  The results of the two routes are compared before anything is timed.

Kernel times come from a separate profiler run of the grouped route alone, each step under its own time limit:

    timeout -k 10 300 python scripts/diag_mask_bench.py 1024 4096 --out bench.jsonl && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d prof -o diag_mask -- python scripts/diag_mask_bench.py 4096 --grouped-only --reps 50

(the kernels are seg_binary_kernel, seg_compact_kernel, seg_reduce_kernel and the mask gather)."""
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

HBM_STREAM_TBS = 6.3      # MI355X_MICROARCH.md: achievable streaming rate (the figure DESIGN.md 4.8 quotes)


class CountingLib:
    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


def bond(bb, leg_spec, moduli, seed):
    """(U, S, Vh, p) of a bond over `leg_spec`: tensors with the new leg last / first and DiagonalTensors"""
    rng = np.random.default_rng(seed)
    sym = ab.Symmetry(list(moduli))
    new = ab.Leg(sym, leg_spec.sectors, leg_spec.mults, +1)
    rows, cols = ab.Leg(sym, new.sectors, 2 * new.mults, +1), ab.Leg(sym, new.sectors, 2 * new.mults, -1)
    s = [np.sort(np.abs(rng.standard_normal(int(k))))[::-1] * 10.0 ** -rng.uniform(0, 6) for k in new.mults]
    norm = np.sqrt(sum(float(np.sum(x * x)) for x in s))
    s = [x / norm for x in s]
    inds = np.array([[i, i] for i in range(new.nsec)], dtype=np.int64)
    U = ab.AbelianTensor(sym, [rows, new.dual()], [bb.as_block(rng.standard_normal((2 * int(k), int(k)))) for k in new.mults], inds, 1)
    Vh = ab.AbelianTensor(sym, [new, cols], [bb.as_block(rng.standard_normal((int(k), 2 * int(k)))) for k in new.mults], inds, 1)
    S = ab.DiagonalTensor(sym, new, [bb.as_block(x) for x in s], np.arange(new.nsec))
    p = ab.DiagonalTensor(sym, new, [bb.as_block(x * x) for x in s], np.arange(new.nsec))
    return U, S, Vh, p, float(np.median(np.concatenate(s)))


def grouped_route(bb, U, S, Vh, p, cutoff):
    mask = ab.diagonal_to_mask(bb, ab.diagonal_compare(bb, S, 'ge', cutoff))
    U2, S2, V2 = ab.svd_apply_mask(bb, U, S, Vh, mask)
    return U2.blocks, S2.blocks, V2.blocks, ab.entropy(bb, p)


def loop_route(bb, U, S, Vh, p, cutoff):
    """the same with the single-block methods, one sector at a time"""
    Ub, Sb, Vb = [], [], []
    for u, s, vh in zip(U.blocks, S.blocks, Vh.blocks):
        flags = s >= cutoff                              # cyb_compare_f64
        if not bb.any(flags):                            # a launch and an 8-byte download (abelian.cpp:1709)
            continue
        m = bb.to_numpy(flags)                           # (the reference: sum_all, and to_numpy for the basis permutation, :1715-1727)
        Ub.append(bb.apply_mask(u, m, 1))                # one gather launch and one upload of the positions each
        Sb.append(bb.apply_mask(s, m, 0))
        Vb.append(bb.apply_mask(vh, m, 0))
    ent = 0.0
    for blk in p.blocks:                                 # p * stable_log(p) and the trace, sector by sector
        ent -= bb.sum_all(blk * bb.stable_log(blk, 1e-30))
    return Ub, Sb, Vb, ent


def timed(bb, fn):
    bb.synchronize()
    t0 = time.perf_counter()
    fn()
    bb.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_calls(bb, fn):
    real, real_d2h = bb.lib, bb.ctx.d2h
    bb.lib = CountingLib(real)
    downloads = []
    bb.ctx.d2h = lambda src, n, *a, **k: downloads.append(int(n)) or real_d2h(src, n, *a, **k)
    try:
        fn()
        return dict(bb.lib.calls), len(downloads)
    finally:
        bb.lib, bb.ctx.d2h = real, real_d2h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[1024, 4096])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--grouped-only', action='store_true', help='run the grouped route alone (for a profiler run)')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    for chi in args.chi:
        for name, leg, moduli in (('u1', wl.u1_leg(chi), (0,)), ('u1u1', wl.u1u1_leg(chi), (0, 0))):
            U, S, Vh, p, cutoff = bond(bb, leg, moduli, wl.DEFAULT_SEED)
            grouped = lambda: grouped_route(bb, U, S, Vh, p, cutoff)
            loop = lambda: loop_route(bb, U, S, Vh, p, cutoff)
            if args.grouped_only:
                for _ in range(args.warmup + args.reps):
                    grouped()
                bb.synchronize()
                continue
            g, l = grouped(), loop()                    # the two routes compute the same thing
            for x, y in zip(g[:3], l[:3]):
                assert len(x) == len(y) and all(np.array_equal(bb.to_numpy(a), bb.to_numpy(b)) for a, b in zip(x, y))
            assert abs(g[3] - l[3]) <= 1e-12 * abs(l[3]), (g[3], l[3])
            (calls_g, sync_g), (calls_l, sync_l) = count_calls(bb, grouped), count_calls(bb, loop)
            for _ in range(args.warmup):
                grouped()
                loop()
            tg, tl = [], []
            for _ in range(args.reps):
                tg.append(timed(bb, grouped))
                tl.append(timed(bb, loop))
            res = dict(case=name, chi=chi, sectors=S.leg.nsec, values=S.leg.dim, kept=int(sum(b.shape[0] for b in g[1])),
                       grouped_ms=dict(median=statistics.median(tg), min=min(tg), max=max(tg)),
                       loop_ms=dict(median=statistics.median(tl), min=min(tl), max=max(tl)),
                       speedup_median=statistics.median(tl) / statistics.median(tg),
                       grouped_faster_beyond_spread=max(tg) < min(tl),
                       grouped_calls=calls_g, grouped_downloads=sync_g, loop_calls=calls_l, loop_call_total=sum(calls_l.values()),
                       loop_downloads=sync_l, entropy=g[3], reduce_bytes=8 * S.leg.dim, hbm_stream_TBps=HBM_STREAM_TBS)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
