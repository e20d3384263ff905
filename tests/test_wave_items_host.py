"""The work items and the cursor of ``csrc/wave_items.h``, walked on the host under ASan and UBSan.

``wave_items_walk.cpp`` includes only that header.  For each instantiation the fusion-tree kernels use it builds seeded
records, cuts them with the shared functions, walks every lane of every item with the shared start and advance, and
requires at every unit the digits and stream offsets that division of the flat index gives, and every unit exactly once.
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


def test_wave_items_walk(tmp_path):
    exe = tmp_path / 'wave_items_walk'
    cmd = [_compiler(), '-std=c++17', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', str(ROOT / 'cyten_amd' / 'csrc'), str(ROOT / 'tests' / 'wave_items_walk.cpp'), '-o', str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, f'{" ".join(cmd)}\n{res.stdout}\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, f'{res.stdout}\n{res.stderr}'
    assert 'no mismatch' in res.stdout, res.stdout
