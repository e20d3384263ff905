"""Grouped tensor product (abelian.outer -> ONE cyb_outer_grouped launch) against the per-pair route, on the device.

    python scripts/outer_bench.py [chi ...] [--reps N] [--out FILE] [--kernel-only]

Two regimes:

  (a) operator building: site operator [p, p*] (x) site operator at d = 2, 3, 4 with U(1) and U(1) x U(1), every sector of
      multiplicity 1 and of multiplicity 2: 4 to 16 pairs of tiny blocks.
  (b) store stream: a bond-sized two-leg tensor [v, v*] with v = workloads.u1_leg(chi), all charge-allowed blocks, (x) a
      [p, p*] operator at d = 4 (four 1 x 1 blocks): the result is four times the size of the bond tensor.

Two routes run alternately in one process after a warm-up, each timed by a host clock around work that ends in a device
synchronise:

  grouped   abelian.outer -> bb.tensor_outer_many -> one launch, results contiguous
  loop      the route without it: bb.tensor_outer (a grouped-GEMM launch with K = 1 and a permuted view) + bb.contiguous (a
            strided copy) per pair of blocks, over the same lexsorted pair list

Printed per case (one JSON line): median / min / max milliseconds of both routes, their C-ABI calls by name and whether the
slowest grouped run beat the fastest loop run.  For (b) also, between device events in the stream (behind a stretch of other
work, so that the host side of the call is hidden): the time of the grouped
call and of a contiguous device-to-device copy of as many bytes as the result holds (the library's strided-copy kernel on a
contiguous block, and the runtime's memcpy), hence the achieved store bandwidth next to the copy's.  `--kernel-only` runs the
grouped call of (b) alone a few times: the run to put under ``rocprofv3 --kernel-trace --stats`` for the kernel time.  The
results of the two routes are compared before anything is timed."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cyten_amd import _lib  # noqa: E402
from cyten_amd import abelian as ab  # noqa: E402
from cyten_amd import workloads as wl  # noqa: E402


class CountingLib:
    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


def loop_outer(bb, a, b):
    """abelian.outer with one bb.tensor_outer + bb.contiguous per pair of blocks"""
    K = a.num_codomain
    l_a, l_b = len(a.blocks), len(b.blocks)
    ia, ib = np.tile(np.arange(l_a), l_b), np.repeat(np.arange(l_b), l_a)
    rows = np.concatenate([a.block_inds[ia, :K], b.block_inds[ib], a.block_inds[ia, K:]], axis=1)
    order = np.lexsort(rows.T)
    blocks = [bb.contiguous(bb.tensor_outer(a.blocks[i], b.blocks[j], K)) for i, j in zip(ia[order].tolist(), ib[order].tolist())]
    return ab.AbelianTensor(a.symmetry, list(a.legs[:K]) + list(b.legs) + list(a.legs[K:]), blocks, rows[order], K + b.num_codomain)


def timed(bb, fn):
    bb.synchronize()
    t0 = time.perf_counter()
    fn()
    bb.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_timed(bb, fn, events, busy):
    """milliseconds between two events recorded in the stream around `fn`; `busy` first enqueues about two milliseconds of
    other work, so that the host side of `fn` runs while the device is still occupied and the events bracket device time"""
    e0, e1 = events
    bb.ctx.sync_stream()
    busy()
    _lib.check(bb.lib.cyb_event_record(bb.ctx.handle, e0))
    fn()
    _lib.check(bb.lib.cyb_event_record(bb.ctx.handle, e1))
    bb.synchronize()
    ms = C.c_float()
    _lib.check(bb.lib.cyb_event_elapsed_ms(e0, e1, C.byref(ms)))
    return float(ms.value)


def count_calls(bb, fn):
    real = bb.lib
    bb.lib = CountingLib(real)
    try:
        fn()
        return dict(bb.lib.calls)
    finally:
        bb.lib = real


def stats(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def site_operator(bb, moduli, d, mult, rng):
    if len(moduli) == 1:
        secs = [[2 * k - (d - 1)] for k in range(d)]
    else:
        secs = [[k, 2 * k - (d - 1)] for k in range(d)]
    p = wl.make_leg(moduli, secs, [mult] * d, +1)
    return ab.AbelianTensor.from_spec(bb, wl.random_tensor(moduli, [p, wl.flip(p)], rng, num_codomain=1))


def compare_routes(bb, a, b, args):
    grouped, loop = (lambda: ab.outer(bb, a, b)), (lambda: loop_outer(bb, a, b))
    g, l = grouped(), loop()
    assert np.array_equal(g.block_inds, l.block_inds)
    for x, y in zip(g.blocks, l.blocks):
        assert x.is_contiguous() and np.array_equal(bb.to_numpy(x), bb.to_numpy(y))
    calls_g, calls_l = count_calls(bb, grouped), count_calls(bb, loop)
    for _ in range(args.warmup):
        grouped()
        loop()
    tg, tl = [], []
    for _ in range(args.reps):
        tg.append(timed(bb, grouped))
        tl.append(timed(bb, loop))
    return g, dict(pairs=len(g.blocks), grouped_ms=stats(tg), loop_ms=stats(tl), speedup_median=statistics.median(tl) / statistics.median(tg),
                   grouped_faster_beyond_spread=max(tg) < min(tl), grouped_calls=calls_g, loop_calls=calls_l, loop_launches=sum(calls_l.values()))


def bond_pair(bb, chi):
    rng = np.random.default_rng(wl.DEFAULT_SEED)
    v = wl.u1_leg(chi, 2.0)
    a = ab.AbelianTensor.from_spec(bb, wl.random_tensor((0,), [v, wl.flip(v)], rng, num_codomain=1))
    return a, site_operator(bb, (0,), 4, 1, rng)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[1024, 2048, 8192])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--kernel-only', action='store_true', help='only the grouped call of regime (b), for a profiler run')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    if args.kernel_only:
        for chi in args.chi:
            a, b = bond_pair(bb, chi)
            for _ in range(args.warmup + args.reps):
                ab.outer(bb, a, b)
            bb.synchronize()
            emit(dict(case='kernel-only', chi=chi, calls=args.warmup + args.reps,
                      out_bytes=8 * 4 * sum(int(np.prod(x.shape)) for x in a.blocks)))
        return

    rng = np.random.default_rng(wl.DEFAULT_SEED)
    for moduli in ((0,), (0, 0)):
        for d in (2, 3, 4):
            for mult in (1, 2):
                a, b = site_operator(bb, moduli, d, mult, rng), site_operator(bb, moduli, d, mult, rng)
                _, res = compare_routes(bb, a, b, args)
                emit(dict(case='operator', symmetry='U1' if len(moduli) == 1 else 'U1xU1', d=d, mult=mult, **res))

    events = []
    for _ in range(2):
        ev = C.c_void_p()
        _lib.check(bb.lib.cyb_event_create(C.byref(ev)))
        events.append(ev)
    pad = bb.empty_many([(1 << 26,), (1 << 26,)])             # 2 x 512 MB

    def busy():
        for _ in range(8):
            _lib.check(bb.lib.cyb_memcpy_d2d(bb.ctx.handle, C.c_void_p(pad[0].ptr), C.c_void_p(pad[1].ptr), 8 << 26))

    for chi in args.chi:
        a, b = bond_pair(bb, chi)
        g, res = compare_routes(bb, a, b, args)
        n_out = sum(int(np.prod(x.shape)) for x in g.blocks)
        nbytes = 8 * n_out
        src, dst = bb.empty_many([(n_out,)])[0], bb.empty_many([(n_out,)])[0]
        routes = dict(grouped=lambda: ab.outer(bb, a, b), copy_kernel=lambda: bb.copy_many([(dst, src)]),
                      memcpy=lambda: _lib.check(bb.lib.cyb_memcpy_d2d(bb.ctx.handle, C.c_void_p(dst.ptr), C.c_void_p(src.ptr), nbytes)))
        ev_ms = {k: [] for k in routes}
        for k, fn in routes.items():
            for _ in range(args.warmup):
                fn()
        for _ in range(args.reps):
            for k, fn in routes.items():
                ev_ms[k].append(event_timed(bb, fn, events, busy))
        res.update(case='store-stream', chi=chi, a_blocks=len(a.blocks), out_bytes=nbytes,
                   event_ms={k: stats(v) for k, v in ev_ms.items()},
                   event_TBps_best={k: nbytes / (min(v) * 1e-3) / 1e12 for k, v in ev_ms.items()},
                   grouped_share_of_copy_kernel=min(ev_ms['copy_kernel']) / min(ev_ms['grouped']),
                   grouped_share_of_memcpy=min(ev_ms['memcpy']) / min(ev_ms['grouped']))
        emit(res)
    del pad
    for ev in events:
        bb.lib.cyb_event_destroy(ev)


if __name__ == '__main__':
    main()
