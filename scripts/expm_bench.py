"""exp of a tensor through ONE matrix_exp_many call against the loop over the per-block bb.matrix_exp, on the device.

    python scripts/expm_bench.py [chi ...] [--reps N] [--only gate|u1|u1u1] [--out FILE]

  gate   a two-site gate exp(-0.05i h): four legs [p, p, p*, p*] with a U(1) local dimension of 8 per site (charges 0 .. 7), so that
         the matrix of pipes has 15 sectors of 1 .. 8 rows; h real symmetric, the factor complex
  u1     exp(t) of a two-leg tensor on workloads.u1_leg(chi) (chi arguments; default 1024), symmetric blocks, Gaussian / sqrt(n)
  u1u1   the same on workloads.u1u1_leg(chi) (default 4096)

Both routes are ``abelian.exp`` on the same tensor and the same backend; the second one sees the backend with
``matrix_exp_many`` hidden, so that exp falls back to ``bb.matrix_exp`` per diagonal block (18 GEMM launches, 18
linear_combination launches, s squarings and a download of the 1-norm per block).  The routes run alternately in one process
after a warm-up, each call timed with HIP events around it (the stream is idle at the first event).  Their results are
compared before anything is timed.  Printed per case (one JSON line): the sector sizes, how many blocks fit the in-LDS kernel,
median / min / max milliseconds of both routes, the ratio of the medians, the C-ABI calls of one call by name and the downloads
of one call, the largest relative difference between the two results."""
import argparse
import collections
import json
import os
import statistics
import sys

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


class PerBlock:
    """the backend with matrix_exp_many hidden: abelian.exp loops over bb.matrix_exp"""
    matrix_exp_many = None

    def __init__(self, bb):
        self._bb = bb

    def __getattr__(self, name):
        return getattr(self._bb, name)


def timed(bb, e0, e1, fn):
    bb.synchronize()
    bb.ctx.record(e0)
    fn()
    bb.ctx.record(e1)
    return bb.ctx.elapsed_ms(e0, e1)


def count_calls(bb, fn):
    real_lib, real_d2h = bb.lib, bb.ctx.d2h
    bb.lib = CountingLib(real_lib)
    downloads = []

    def d2h(src, n, *args, **kw):
        downloads.append(int(n))
        return real_d2h(src, n, *args, **kw)
    bb.ctx.d2h = d2h
    try:
        fn()
        calls = {k: v for k, v in bb.lib.calls.items() if k != 'cyb_last_error'}
        return calls, len(downloads)
    finally:
        bb.lib = real_lib
        del bb.ctx.d2h


def gate_tensor(rng):
    p = wl.make_leg((0,), np.arange(8)[:, None], np.ones(8, dtype=np.int64), +1)
    legs = [p, p, wl.flip(p), wl.flip(p)]
    inds = wl.allowed_block_inds((0,), legs)
    h = rng.standard_normal((64, 64))
    h = (h + h.T) / 2          # as a matrix from (p2*, p1*) reversed to (p1, p2): entry [(a, b), (a', b')]
    blocks = [np.array(h[8 * a + b, 8 * a2 + b2]).reshape(1, 1, 1, 1) for a, b, b2, a2 in inds.tolist()]
    return wl.TensorSpec((0,), legs, inds, blocks, 2)


def square_tensor(rng, leg, moduli):
    legs = [leg, wl.flip(leg)]
    inds = wl.allowed_block_inds(moduli, legs)
    blocks = []
    for i, _ in inds.tolist():
        n = int(leg.mults[i])
        g = rng.standard_normal((n, n)) / np.sqrt(n)
        blocks.append((g + g.T) / 2)
    return wl.TensorSpec(moduli, legs, inds, blocks, 1)


def measure(bb, name, chi, spec, factor, reps, warmup):
    t = ab.AbelianTensor.from_spec(bb, spec)
    loop = PerBlock(bb)
    many_fn = lambda: ab.exp(bb, t, factor)        # noqa: E731
    loop_fn = lambda: ab.exp(loop, t, factor)      # noqa: E731
    got, want = many_fn(), loop_fn()
    assert np.array_equal(got.block_inds, want.block_inds)
    diff = max(float(np.abs(bb.to_numpy(x) - bb.to_numpy(y)).max() / np.abs(bb.to_numpy(y)).max()) for x, y in zip(got.blocks, want.blocks)
               if x.size and np.abs(bb.to_numpy(y)).max() > 0)
    k = t.nlegs // 2
    lead = t.legs[0] if k == 1 else ab.LegPipe.from_legs(t.symmetry, t.legs[:k], +1)
    sizes = [int(m) for m in lead.mults]
    limit = _lib.CYB_EXPM_SMALL_MAX_N_C128 if isinstance(factor, complex) else _lib.CYB_EXPM_SMALL_MAX_N_F64
    calls_many, dl_many = count_calls(bb, many_fn)
    calls_loop, dl_loop = count_calls(bb, loop_fn)
    for _ in range(warmup):
        many_fn()
        loop_fn()
    e0, e1 = bb.ctx.event(), bb.ctx.event()
    tm, tl = [], []
    for _ in range(reps):
        tm.append(timed(bb, e0, e1, many_fn))
        tl.append(timed(bb, e0, e1, loop_fn))
    mm, ml = statistics.median(tm), statistics.median(tl)
    return dict(case=name, chi=chi, factor=str(factor), sectors=len(sizes), rows_min=min(sizes), rows_max=max(sizes),
                in_lds=sum(1 for n in sizes if n <= limit), beyond=sum(1 for n in sizes if n > limit), reps=reps,
                many_ms=dict(median=mm, min=min(tm), max=max(tm)), per_block_ms=dict(median=ml, min=min(tl), max=max(tl)),
                per_block_over_many=ml / mm, many_faster_beyond_spread=bool(max(tm) < min(tl)),
                many_calls=calls_many, many_calls_total=sum(calls_many.values()), many_downloads=dl_many,
                per_block_calls_total=sum(calls_loop.values()), per_block_downloads=dl_loop, max_rel_difference=diff)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--only', default=None, choices=['gate', 'u1', 'u1u1'])
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    rng = np.random.default_rng(20240611)
    todo = [('gate', 8, lambda: gate_tensor(rng), -0.05j)]
    for chi in args.chi or [1024]:
        todo.append(('u1', chi, lambda chi=chi: square_tensor(rng, wl.u1_leg(chi), (0,)), 1.0))
    for chi in args.chi or [4096]:
        todo.append(('u1u1', chi, lambda chi=chi: square_tensor(rng, wl.u1u1_leg(chi), (0, 0)), 1.0))
    for name, chi, make, factor in todo:
        if args.only and name != args.only:
            continue
        line = json.dumps(measure(bb, name, chi, make(), factor, args.reps, args.warmup))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
