"""Device side of the guard-band GEMM cases (tests/gemm_guard_cases.py): the arenas in device memory and the two entry
points of the C ABI as `launch` callables -- imported by tests/test_gpu_gemm_guard.py.

Run as a program it is the child process of `test_planner_switches`: the class-0, tail-split and streaming-kernel groups
(exact data) under whatever CYB_GEMM_* switches the parent put into the environment (they are read once per process).
Prints OK or raises."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_guard_cases as gc   # noqa: E402
from cyten_amd import _lib   # noqa: E402

ENTRIES = ('plan', 'enqueue')


class DeviceMemory:
    """`memory` of gemm_guard_cases.run: every arena is one block of the backend, 16-byte aligned."""

    def __init__(self, bb):
        self.bb, self.blocks = bb, {}

    def upload(self, arr):
        blk = self.bb.empty_block((arr.size + 1,))
        shift = (blk.ptr // 8) % 2
        self.bb.ctx.h2d(blk.buf, arr, blk.offset + shift)
        addr = blk.ptr + 8 * shift
        self.blocks[addr] = (blk, shift)
        return addr

    def download(self, addr, n):
        blk, shift = self.blocks[addr]
        self.bb.synchronize()
        return self.bb.ctx.d2h(blk.buf, n, np.float64, blk.offset + shift)


def launcher(bb, entry, runs=1, info=None):
    """`launch` of gemm_guard_cases.run.  'plan': cyb_gemm_plan_create, `runs` times cyb_gemm_plan_run on the SAME plan,
    destroy; 'enqueue': cyb_gemm_grouped_enqueue_f64 `runs` times.  `info` (a dict) receives cyb_gemm_plan_info."""
    lib, ctx = bb.lib, bb.ctx.handle

    def plan(probs, n_probs, segs, n_segs):
        handle = C.c_void_p()
        bb.ctx.sync_stream()
        _lib.check(lib.cyb_gemm_plan_create(ctx, C.byref(handle), probs, n_probs, segs, n_segs))
        try:
            if info is not None:
                nt, nl = C.c_int64(), C.c_int32()
                _lib.check(lib.cyb_gemm_plan_info(handle, None, None, C.byref(nt), C.byref(nl)))
                info.update(n_tiles=nt.value, n_launches=nl.value)
            for _ in range(runs):
                _lib.check(lib.cyb_gemm_plan_run(ctx, handle))
        finally:
            _lib.check(lib.cyb_gemm_plan_destroy(handle))

    def enqueue(probs, n_probs, segs, n_segs):
        bb.ctx.sync_stream()
        for _ in range(runs):
            _lib.check(lib.cyb_gemm_grouped_enqueue_f64(ctx, probs, n_probs, segs, n_segs))
        bb.synchronize()            # the descriptor arrays are read by the call itself, the kernels run behind it

    return {'plan': plan, 'enqueue': enqueue}[entry]


def run_case(bb, case, entry, runs=1, info=None):
    return gc.run(case, launcher(bb, entry, runs, info), DeviceMemory(bb))


def twice_refs(case):
    """What the same beta = 1, alpha = 1 call leaves when it runs twice: C0 + 2 A B (exact data)."""
    return [2 * p.ref - gc._view(case.cout0, p.c_off, (p.spec.M, p.spec.N), (p.ldc, 1)) for p in case.probs]


def main():
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    n_cu = bb.ctx.n_cu
    skinny_on = not (os.environ.get('CYB_GEMM_SKINNY') and int(os.environ['CYB_GEMM_SKINNY']) == 0)
    groups = [('class0 %s beta=%g' % (lay, beta), gc.class0_specs(n_cu, lay, beta)) for lay, beta in
              (('cr', 0.0), ('rc', 1.0))]
    groups += [('tail split', gc.tail_split_specs(n_cu)), ('skinny', gc.skinny_specs())]
    for name, specs in groups:
        case = gc.build_case(specs, 11)
        for entry in ENTRIES:
            info = {}
            rep = gc.check(case, run_case(bb, case, entry, 1, info))
            assert rep.clean, f'{name} [{entry}]: {rep}'
            if name == 'skinny' and entry == 'plan':
                assert info['n_launches'] == (2 if skinny_on else 1), info
    print('OK')


if __name__ == '__main__':
    main()
