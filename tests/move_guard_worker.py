"""Device side of the guard-band data-movement cases (tests/move_guard_cases.py): the arenas in device memory (the
DeviceMemory of gemm_guard_worker.py) and the entry points of the C ABI as the `launch` callable of move_guard_cases.run
-- imported by tests/test_gpu_move_guard.py."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import move_guard_cases as mc   # noqa: E402
from gemm_guard_worker import DeviceMemory   # noqa: E402
from cyten_amd import _lib   # noqa: E402

ENTRY = {'gather': 'cyb_mask_gather_batched_f64', 'scatter': 'cyb_mask_scatter_batched_f64', 'scale': 'cyb_scale_axis_batched_f64',
         'cexpand': 'cyb_complex_expand_batched_f64', 'lincomb_f64': 'cyb_lincomb_strided_batched_f64',
         'lincomb_c128': 'cyb_lincomb_strided_batched_c128'}


def status(bb, op, arrays, elem_size):
    """The status of ONE call of the entry point of `op` (the descriptor arrays are read by the call itself)."""
    bb.ctx.sync_stream()
    if op == 'copy':
        return bb.lib.cyb_copy_strided_batched(bb.ctx.handle, arrays[0], arrays[1], elem_size)
    return getattr(bb.lib, ENTRY[op])(bb.ctx.handle, *arrays)


def launcher(bb):
    def launch(op, arrays, elem_size):
        _lib.check(status(bb, op, arrays, elem_size))
        bb.synchronize()
    return launch


def run_case(bb, case, launches=1):
    return mc.run(case, launcher(bb), DeviceMemory(bb), launches)


def refused(bb, op, arrays, elem_size):
    """True when the call is refused with CYB_ERR_INVALID (nothing is launched then)."""
    return status(bb, op, arrays, elem_size) == _lib.CYB_ERR_INVALID


def mask_desc(x, out, idx, outer, axis, inner, n_keep):
    d = (_lib.MaskDesc * 1)()
    d[0].x, d[0].out, d[0].idx = x, out, idx
    d[0].outer, d[0].axis, d[0].inner, d[0].n_keep = outer, axis, inner, n_keep
    return d, C.c_int64(1)
