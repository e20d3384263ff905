"""The chunk rules and the cutter of ``csrc/flat_items.h``, checked on the host under ASan and UBSan.

``flat_items_cut.cpp`` includes only that header.  It compares every chunk rule with literals worked out by hand from the
formulas the kernels have always used (a different cut is a different summation order), and for seeded lists of totals
that hold 0, 1, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 it requires that the items cover every record exactly once,
in ascending order, none longer than the chunk.
"""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _compiler() -> str:
    exe = shutil.which('c++')
    if exe:
        return exe
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    for cand in (Path(hipcc).resolve().parent / 'clang++', Path(hipcc).resolve().parent.parent / 'llvm' / 'bin' / 'clang++',
                 Path(hipcc).resolve().parent.parent / 'lib' / 'llvm' / 'bin' / 'clang++'):
        if cand.exists():
            return str(cand)
    raise RuntimeError('neither a host c++ nor the clang++ beside hipcc was found')


def test_flat_items_cut(tmp_path):
    exe = tmp_path / 'flat_items_cut'
    cmd = [_compiler(), '-std=c++17', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', str(ROOT / 'cyten_amd' / 'csrc'), str(ROOT / 'tests' / 'flat_items_cut.cpp'), '-o', str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, f'{" ".join(cmd)}\n{res.stdout}\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, f'{res.stdout}\n{res.stderr}'
    assert 'no mismatch' in res.stdout, res.stdout
