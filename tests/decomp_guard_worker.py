"""Device side of the guard-band decomposition cases (tests/decomp_guard_cases.py): the arenas in device memory (the
DeviceMemory of gemm_guard_worker.py) and the ten batched entries of the C ABI as the `launch` callable of
decomp_guard_cases.run -- imported by tests/test_gpu_decomp_guard.py."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decomp_guard_cases as dg   # noqa: E402
from gemm_guard_worker import DeviceMemory   # noqa: E402


def launcher(bb):
    """`launch` of decomp_guard_cases.run: ONE call of the entry of `kind`, then a synchronisation; the status comes back
    as it is (a refused call is a result, not an exception)."""
    lib, ctx = bb.lib, bb.ctx.handle

    def launch(kind, descs, n, flags, want_info, want_rank):
        bb.ctx.sync_stream()
        info = (C.c_int32 * max(n, 1))(*([-77] * max(n, 1))) if want_info else None
        rank = (C.c_int32 * max(n, 1))(*([-77] * max(n, 1))) if want_rank else None
        fn = getattr(lib, dg.ENTRY[kind])
        if kind == 'svd_ex':
            st = fn(ctx, descs, n, info, flags, rank)
        elif kind == 'eigh_ex':
            st = fn(ctx, descs, n, info, flags)
        elif kind in ('qr', 'cqr'):
            st = fn(ctx, descs, n)
        else:
            st = fn(ctx, descs, n, info)
        bb.synchronize()
        return st, (list(info[:n]) if want_info else None), (list(rank[:n]) if want_rank else None)

    return launch


def run_case(bb, case, nan=False, launches=1):
    return dg.run(case, launcher(bb), DeviceMemory(bb), nan, launches)


def uploaded(bb, case):
    """Both arenas on the device: (memory, (base_in, base_out))."""
    mem = DeviceMemory(bb)
    return mem, (mem.upload(case.ain.view(np.float64)), mem.upload(case.aout0.view(np.float64)))


def untouched(mem, bases, case):
    gin = mem.download(bases[0], case.ain.size // 8).view(np.uint8)
    gout = mem.download(bases[1], case.aout0.size // 8).view(np.uint8)
    return np.array_equal(gin, case.ain) and np.array_equal(gout, case.aout0)
