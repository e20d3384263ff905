"""The plan of the QR-preconditioned SVD pipeline (``csrc/svd_plan.h``), checked on the host under ASan and UBSan.

``svd_plan.cpp`` includes only that header.  The driver carves its workspace by the plan's layout and copies whole ranges
of it in one go; for lists of one to six blocks with extents from {1, 2, 63, 64, 65, 128, 200} the program requires that
every piece lies inside the total, the pieces are disjoint and (outside the header and the index lists) 256-byte aligned,
the host-read header covers exactly the ``sig``, ``bad``, ``dev`` and ``ctl`` words, ``dev`` begins where ``bad`` ends and
the index lists are contiguous.  The deflation split, the two route rules at their edges, the columns of the null rows and
the tiny / direct / pipeline split of a list are pinned by cases worked out by hand.
"""
import subprocess
from pathlib import Path

from test_qr_strip_chunks_host import _compiler

ROOT = Path(__file__).resolve().parent.parent


def test_svd_plan(tmp_path):
    exe = tmp_path / 'svd_plan'
    cmd = [_compiler(), '-std=c++17', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', str(ROOT / 'cyten_amd' / 'csrc'), str(ROOT / 'tests' / 'svd_plan.cpp'), '-o', str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, f'{" ".join(cmd)}\n{res.stdout}\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, f'{res.stdout}\n{res.stderr}'
    assert 'no mismatch' in res.stdout, res.stdout
