"""combine_legs on a device-resident placement plan against the routes that exist without it, on the device.

    python scripts/leg_pipe_bench.py [chi ...] [--reps N] [--only theta_u1|theta_u1u1|mpo] [--out FILE]
    python scripts/leg_pipe_bench.py --kernel-trace FILE_kernel_trace.csv      (summarise a rocprofv3 --kernel-trace run)

theta_u1, theta_u1u1: the two-site theta of workloads.config_u1_mps(chi) / config_u1u1_mps(chi), fused into a matrix twice:

  plan     abelian.combine_legs(theta, [[0, 1], [2, 3]], signs=[+1, -1]) -- plan cached, one cyb_place_plan_enqueue
  parent   abelian.combine_legs_to_matrix(theta, 2) -- one descriptor per block marshalled, classified, cut and uploaded by
           cyb_copy_strided_batched in every call

mpo: the MPO-applied MPS tensor, tdot of an MPS tensor with the W of workloads.config_heff, legs permuted (views) to
[vL, wL, p, vR, wR], then the (v, w) pairs fused:

  plan     abelian.combine_legs(permuted, [[0, 1], [3, 4]])
  generic  the same call on the same backend with its plans hidden: zeros_many + copy_many of views

The two routes of a case run alternately in one process after a warm-up, each timed by a host clock around work that ends in
a device synchronise.  The results of the two routes are compared bit for bit before anything is timed.  Printed per case (one
JSON line): median / min / max milliseconds of both routes, the ratio of the medians, the C-ABI calls of one call by name, the
host-to-device bytes of one call, and the verdicts the script checks itself: `plan_within_parent_spread` (plan median <= other
median + (other max - other min)) and `plan_faster_beyond_spread` (max plan < min other)."""
import argparse
import collections
import csv
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
COPY_DESC_BYTES, ITEM_BYTES = 216, 24


class CountingLib:
    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self.calls[name] += 1
            return fn(*args)
        return wrapper


class NoPlans:
    """the backend with its placement plans hidden: combine_legs takes the generic zeros_many + copy_many route"""
    place_plan = None

    def __init__(self, bb):
        self._bb = bb

    def __getattr__(self, name):
        return getattr(self._bb, name)


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


def chunk_for(total):
    """the work-item size of csrc/copy_kernels.h"""
    c = ((total // 2048) + 1023) & ~1023
    return min(1 << 16, max(8192, c))


def parent_upload_bytes(blocks):
    """what cyb_copy_strided_batched uploads for the row-run scatter of these blocks: descriptors + work items"""
    sizes = [b.size for b in blocks if b.size]
    chunk = chunk_for(sum(sizes))
    return COPY_DESC_BYTES * len(sizes) + ITEM_BYTES * sum(-(-s // chunk) for s in sizes)


def same_blocks(bb, xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert x.shape == y.shape and np.array_equal(bb.to_numpy(x), bb.to_numpy(y))


def measure(bb, name, chi, plan_fn, other_fn, other_name, reps, warmup, extra):
    calls_p, calls_o = count_calls(bb, plan_fn), count_calls(bb, other_fn)
    for _ in range(warmup):
        plan_fn()
        other_fn()
    tp, to = [], []
    for _ in range(reps):
        tp.append(timed(bb, plan_fn))
        to.append(timed(bb, other_fn))
    mp, mo = statistics.median(tp), statistics.median(to)
    res = dict(case=name, chi=chi, reps=reps, plan_ms=dict(median=mp, min=min(tp), max=max(tp)),
               **{other_name + '_ms': dict(median=mo, min=min(to), max=max(to))}, ratio_of_medians=mp / mo,
               plan_within_parent_spread=bool(mp <= mo + (max(to) - min(to))), plan_faster_beyond_spread=bool(max(tp) < min(to)),
               plan_calls=calls_p, **{other_name + '_calls': calls_o}, **extra)
    return res


def case_theta(bb, which, chi, reps, warmup):
    A, B = wl.config_u1_mps(chi) if which == 'theta_u1' else wl.config_u1u1_mps(chi)
    theta = ab.compose(bb, ab.AbelianTensor.from_spec(bb, A), ab.AbelianTensor.from_spec(bb, B), 1)
    plan_fn = lambda: ab.combine_legs(bb, theta, [[0, 1], [2, 3]], signs=[+1, -1])    # noqa: E731
    parent_fn = lambda: ab.combine_legs_to_matrix(bb, theta, 2)                      # noqa: E731
    got, mv = plan_fn(), parent_fn()
    same_blocks(bb, got.blocks, mv.blocks)
    read = 8 * sum(b.size for b in theta.blocks)
    written = 8 * sum(b.size for b in got.blocks)
    covers = read == written
    extra = dict(blocks=len(theta.blocks), result_blocks=len(got.blocks), covers=covers,
                 plan_h2d_bytes=8 * (len(theta.blocks) + len(got.blocks)), parent_h2d_bytes=parent_upload_bytes(theta.blocks),
                 # read theta once + write the occupied entries once (+ the zero fill of the result where it is issued)
                 algorithmic_bytes_plan=2 * read + (0 if covers else written), algorithmic_bytes_parent=2 * read + written,
                 hbm_stream_TBps=HBM_STREAM_TBS)
    return measure(bb, which, chi, plan_fn, parent_fn, 'parent', reps, warmup, extra)


def case_mpo(bb, chi, reps, warmup):
    A, _ = wl.config_u1_mps(chi)
    W = wl.config_heff(chi, charged_mpo=True)['W1']
    a, w = ab.AbelianTensor.from_spec(bb, A), ab.AbelianTensor.from_spec(bb, W)
    t = ab.tdot(bb, a, w, [1], [2])                 # [vL, vR, p, wL, wR]
    t = ab.permute_legs(bb, t, [0, 3, 2, 1, 4])     # [vL, wL, p, vR, wR], strided views
    hidden = NoPlans(bb)
    plan_fn = lambda: ab.combine_legs(bb, t, [[0, 1], [3, 4]])          # noqa: E731
    generic_fn = lambda: ab.combine_legs(hidden, t, [[0, 1], [3, 4]])   # noqa: E731
    got, want = plan_fn(), generic_fn()
    assert np.array_equal(got.block_inds, want.block_inds)
    same_blocks(bb, got.blocks, want.blocks)
    extra = dict(blocks=len(t.blocks), result_blocks=len(got.blocks), bytes_moved=2 * 8 * sum(b.size for b in t.blocks),
                 plan_h2d_bytes=8 * (len(t.blocks) + len(got.blocks)))
    return measure(bb, 'mpo', chi, plan_fn, generic_fn, 'generic', reps, warmup, extra)


def summarize_trace(path):
    """per kernel of the copy family: launches, median / min / max microseconds, from a rocprofv3 kernel trace (csv)"""
    dur = collections.defaultdict(list)
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Kernel_Name']
            for key in ('place_strided_kernel', 'place_transpose64_kernel', 'place_transpose_kernel', 'copy_strided_kernel',
                        'copy_transpose64_kernel', 'copy_transpose_kernel', 'fillBuffer'):
                if key in name:
                    wide = '<16B>' if ('__vector' in name or 'ext_vector' in name or 'Dv2' in name) else ''
                    grid = row.get('Grid_Size_X', row.get('Grid_Size', '?'))
                    dur[f'{key}{wide} grid={grid}'].append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3)
                    break
    for key, d in sorted(dur.items()):
        print(json.dumps(dict(kernel=key, launches=len(d), median_us=statistics.median(d), min_us=min(d), max_us=max(d))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('chi', nargs='*', type=int, default=[1024, 4096])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, choices=['theta_u1', 'theta_u1u1', 'mpo'])
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--kernel-trace', default=None, help='summarise this rocprofv3 kernel trace instead of measuring')
    args = ap.parse_args()
    if args.kernel_trace:
        return summarize_trace(args.kernel_trace)
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    for chi in args.chi:
        for which in ('theta_u1', 'theta_u1u1', 'mpo'):
            if args.only and which != args.only:
                continue
            if which != 'mpo' and chi != max(args.chi):
                continue        # (the thetas are compared at the largest size only: the parent route's sizes of interest)
            res = case_mpo(bb, chi, args.reps, args.warmup) if which == 'mpo' else case_theta(bb, which, chi, args.reps, args.warmup)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
