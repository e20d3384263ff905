"""The plan of the Jacobi sweep kernel (``csrc/jacobi_plan.h``), checked on the host under ASan and UBSan.

``jacobi_plan.cpp`` includes only that header.  The driver sizes the zeroed counter block, the granule regions and the
descriptor image of a sweep from the plan's layout and the launch indexes them by the same struct: for lists of one to six
matrices on 4 ... 256 workgroup slots the program requires that the parts per pair fit the slots, the flag bases and image
regions are disjoint, what a plan uses never exceeds what was reserved, and the shared-workgroup ranges cover the entries
exactly once.  Parts, split and convergence rule are pinned by cases worked out by hand.
"""
import subprocess
from pathlib import Path

from test_qr_strip_chunks_host import _compiler

ROOT = Path(__file__).resolve().parent.parent


def test_jacobi_plan(tmp_path):
    exe = tmp_path / 'jacobi_plan'
    cmd = [_compiler(), '-std=c++17', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', str(ROOT / 'cyten_amd' / 'csrc'), str(ROOT / 'tests' / 'jacobi_plan.cpp'), '-o', str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, f'{" ".join(cmd)}\n{res.stdout}\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, f'{res.stdout}\n{res.stderr}'
    assert 'no mismatch' in res.stdout, res.stdout
